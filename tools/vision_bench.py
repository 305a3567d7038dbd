"""The mean-pool head of the vision-branch classifier on the device: the HIP kernel pair (ops.token_mean_norm over csrc/tokenpool.hip)
against the torch statement of the same lines (ops.token_mean_norm_torch: slice, mean, LayerNorm and their autograd backward), forward +
backward, on the same device buffers; and, as a smoke figure only, one forward + backward step of a 2-layer one_piece_g_256.

    python tools/vision_bench.py [--iters 50] [--rounds 7] [--step-timeout 240] [--out profiles/vision_head_mi355x.json]

Shapes: H = 1536 (the g model), B = 64 at S = 257 / 577 / 1025 (256^2, 384^2, 512^2 images) and B = 128 at S = 257; bf16.

Method: every shape runs in a process of its own under its own time limit (the parent never opens the device; it stops at the first
step that fails or runs out of time, and the steps it did not reach are recorded as "not measured").  Inside a step: device events around
`iters` forward + backward calls, both routes warmed up first, the two routes alternating round by round; the median over the rounds and
their spread, in microseconds per call (forward + backward with their launch gaps: a call time, not a kernel time).  Achieved bytes/s =
the algorithmic bytes of the op -- x read once and its gradient written once, 4 B S H, plus the [B, H]-sized rows -- over the HIP
route's call time.  The activation tensors are 25 - 200 MB against 256 MiB of Infinity Cache: between back-to-back calls part of x and
of dx stays on the die, so these rates are NOT HBM rates; both routes are measured under the same condition.  There is no CPU mode:
without a device the tool fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H = 1536
SHAPES = [("256px_b64", 64, 257), ("384px_b64", 64, 577), ("512px_b64", 64, 1025), ("256px_b128", 128, 257)]
MODEL_STEP = "g256_2layer_step"


def algorithmic_bytes(B, S, Hh):
    """forward: x without its CLS rows (2 B (S - 1) H), y (2 B H), pooled (4 B H); backward: dy (2 B H), pooled (4 B H), dx (2 B S H),
    the two [H] parts.  The split partials (at most 64 B H floats, read back at once) and the [H] vectors of w / b are left out."""
    return 2 * B * (S - 1) * Hh + 6 * B * Hh + 6 * B * Hh + 2 * B * S * Hh + 8 * Hh


def _events(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def head_step(name, B, S, iters, rounds):
    import torch
    from one_peace_amd import hip, ops
    hip.lib()
    dev = "cuda:0"
    g = torch.Generator().manual_seed(S)
    x = torch.randn(B, S, H, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
    w = (1.0 + 0.1 * torch.randn(H, generator=g)).to(dev, torch.bfloat16).requires_grad_(True)
    b = (0.1 * torch.randn(H, generator=g)).to(dev, torch.bfloat16).requires_grad_(True)
    dy = torch.randn(B, H, generator=g).to(dev, torch.bfloat16)
    routes = {"hip": ops.token_mean_norm, "torch": ops.token_mean_norm_torch}

    def call(fn):
        x.grad = w.grad = b.grad = None
        fn(x, w, b, 1e-5).backward(dy)

    outs, grads = {}, {}
    for r, fn in routes.items():
        call(fn)
        outs[r], grads[r] = fn(x, w, b, 1e-5).detach().float(), x.grad.detach().float()
    agree = float((outs["hip"] - outs["torch"]).norm() / outs["torch"].norm())
    agree_dx = float((grads["hip"] - grads["torch"]).norm() / grads["torch"].norm())
    for fn in routes.values():
        for _ in range(10):
            call(fn)
    torch.cuda.synchronize()
    times = {r: [] for r in routes}
    for _ in range(rounds):
        for r, fn in routes.items():
            times[r].append(_events(lambda: call(fn), iters))
    row = {"shape": name, "B": B, "S": S, "H": H, "iters": iters, "rounds": rounds, "algorithmic_bytes": algorithmic_bytes(B, S, H),
           "rel_diff_y_hip_vs_torch": agree, "rel_diff_dx_hip_vs_torch": agree_dx}
    for r in routes:
        row[r + "_us"] = statistics.median(times[r])
        row[r + "_us_min_max"] = [min(times[r]), max(times[r])]
    row["hip_algorithmic_TB_per_s"] = row["algorithmic_bytes"] / (row["hip_us"] * 1e-6) / 1e12
    row["torch_over_hip"] = row["torch_us"] / row["hip_us"]
    return row


def model_step(iters, rounds):
    import torch
    from one_peace_amd import hip
    from one_peace_amd.one_peace_vision import one_piece_g_256
    hip.lib()
    dev = "cuda:0"
    torch.manual_seed(0)
    B = 16
    m = one_piece_g_256(layers=2, num_classes=1000, drop_path_rate=0.1).to(dev).to(torch.bfloat16).train()
    images = torch.randn(B, 3, 256, 256, device=dev, dtype=torch.bfloat16)
    target = torch.randint(0, 1000, (B,), device=dev)

    def step():
        m.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(m(images).float(), target).backward()

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    times = [_events(step, iters) for _ in range(rounds)]
    return {"shape": MODEL_STEP, "what": "smoke figure: one forward + backward of one_piece_g_256(layers=2), bf16, training mode",
            "B": B, "image": 256, "iters": iters, "rounds": rounds, "step_us": statistics.median(times), "step_us_min_max": [min(times), max(times)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per process step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vision_head_mi355x.json"))
    ap.add_argument("--one", default=None, help="(internal) run this step in this process and print its JSON row")
    args = ap.parse_args()
    import torch
    if args.one is not None:
        if not torch.cuda.is_available():
            sys.exit("vision_bench: no GPU -- timings are taken on the MI355X only")
        if args.one == MODEL_STEP:
            row = model_step(max(args.iters // 5, 5), args.rounds)
        else:
            name, B, S = next(s for s in SHAPES if s[0] == args.one)
            row = head_step(name, B, S, args.iters, args.rounds)
        row["device"] = torch.cuda.get_device_name(0)
        print("ROW " + json.dumps(row))
        return
    steps = [s[0] for s in SHAPES] + [MODEL_STEP]
    results, device, stopped = [], None, None
    for name in steps:
        if stopped is not None:
            results.append({"shape": name, "status": "not measured", "why": "not started: step %s %s" % stopped})
            continue
        cmd = [sys.executable, os.path.abspath(__file__), "--one", name, "--iters", str(args.iters), "--rounds", str(args.rounds)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            stopped = (name, "ran past its %d s limit" % args.step_timeout)
            results.append({"shape": name, "status": "not measured", "why": stopped[1]})
            continue
        rows = [line[4:] for line in r.stdout.splitlines() if line.startswith("ROW ")]
        if r.returncode != 0 or not rows:
            stopped = (name, "ended with status %d" % r.returncode)
            results.append({"shape": name, "status": "not measured", "why": stopped[1], "output_tail": r.stdout[-2000:]})
            continue
        row = json.loads(rows[-1])
        device = row.pop("device", device)
        row["status"] = "measured"
        results.append(row)
        print(json.dumps(row), flush=True)
    rec = {"tool": "tools/vision_bench.py", "device": device,
           "what": "forward + backward call time, microseconds; median of `rounds` windows of `iters` calls, the two routes alternating",
           "note": "x and dx (25 - 200 MB) stay partly in the 256 MiB Infinity Cache between back-to-back calls: algorithmic bytes over "
                   "call time is not an HBM rate", "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if stopped is not None:
        sys.exit("vision_bench: step %s %s" % stopped)


if __name__ == "__main__":
    main()
