"""Temporal attention of the video branch on the device: ops.temporal_attention (csrc/frameattn.hip, the packed q|k|v rows read where
they lie) against (a) the torch statement on the same buffers (ops.temporal_attention_torch: the two rearranges, bmm, fp32 softmax, bmm
and their autograd backward) and (b) the project's existing attention entry on rearranged copies (rows regrouped so that a sequence's T
frames are contiguous, hip.attn_fwd / hip.attn_bwd with the key axis padded to 128, results regrouped back): what the layer would cost
without the kernel.  Forward + backward.  And, as a smoke figure only, one forward + backward of a 2-layer OnePeaceVideoViT.

    python tools/video_bench.py [--iters 50] [--rounds 7] [--step-timeout 240] [--out profiles/temporal_attn_mi355x.json]

Shapes: B = 2 clips, N = 257 tokens, 24 heads of 64 (H = 1536), T = 8, 16 and 32 frames; bf16.

Method: every shape runs in a process of its own under its own time limit (the parent never opens the device; it stops at the first
step that fails or runs out of time, and the steps it did not reach are recorded as "not measured").  Inside a step, after a warm-up of
every route: device events around `iters` forward + backward calls, the routes alternating round by round; the median over the rounds
and their spread, in microseconds per call (a call time: launch gaps, allocations and autograd included).  Kernel time: the same events
around `iters` back-to-back launches of op_attn_frames_fwd, resp. _bwd, alone on preallocated buffers (the queue never runs dry, so
this is the kernels' own time plus the launch boundary).  Algorithmic bytes: forward 4 R H 2 B (q, k, v read, out written), backward
7 R H 2 B (q, k, v, dout read, dq, dk, dv written), R = B T N; over the kernel time.  The buffers are 38 - 150 MB against 256 MiB of
Infinity Cache: between back-to-back calls part of them stays on the die, so these rates are NOT HBM rates; every route is measured
under the same condition.  There is no CPU mode: without a device the tool fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

B, N, HEADS = 2, 257, 24
H = HEADS * 64
SHAPES = [("T8", 8), ("T16", 16), ("T32", 32)]
MODEL_STEP = "video_2layer_step"


def _events(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def attn_step(name, T, iters, rounds):
    import torch
    from one_peace_amd import hip, ops
    hip.lib()
    dev = "cuda:0"
    R = B * T * N
    g = torch.Generator().manual_seed(T)
    qkv = torch.randn(R, 3 * H, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
    dout = torch.randn(R, H, generator=g).to(dev, torch.bfloat16)
    scale = 0.125

    def autograd_call(fn):
        def call():
            qkv.grad = None
            fn(qkv, B, T, N, HEADS, scale).backward(dout)
            return qkv.grad
        return call

    def regroup(x, a, b):  # rows (B, a, b) -> rows (B, b, a): one pass over the whole matrix
        return x.view(B, a, b, x.shape[1]).permute(0, 2, 1, 3).contiguous().view(-1, x.shape[1])

    state = {}

    def existing_entry():
        x = regroup(qkv.detach(), T, N)                                                   # a sequence's T frames contiguous
        out, lse = hip.attn_fwd(x[:, :H], x[:, H:2 * H], x[:, 2 * H:], 3 * H, B * N, T, HEADS, scale)
        state["out"] = regroup(out, N, T)
        d = regroup(dout, T, N)
        dqkv, _ = hip.attn_bwd(x[:, :H], x[:, H:2 * H], x[:, 2 * H:], 3 * H, d, out, lse, B * N, T, HEADS, scale)
        return regroup(dqkv, N, T)

    routes = {"hip": autograd_call(ops.temporal_attention), "torch": autograd_call(ops.temporal_attention_torch),
              "existing_entry": existing_entry}
    grads = {r: fn().detach().float().clone() for r, fn in routes.items()}
    out_hip = ops.temporal_attention(qkv, B, T, N, HEADS, scale).detach().float()
    out_torch = ops.temporal_attention_torch(qkv, B, T, N, HEADS, scale).detach().float()
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    row = {"shape": name, "B": B, "T": T, "N": N, "heads": HEADS, "rows": R, "iters": iters, "rounds": rounds,
           "rel_diff_out_hip_vs_torch": rel(out_hip, out_torch), "rel_diff_out_existing_vs_torch": rel(state["out"].float(), out_torch),
           "rel_diff_dqkv_hip_vs_torch": rel(grads["hip"], grads["torch"]),
           "rel_diff_dqkv_existing_vs_torch": rel(grads["existing_entry"], grads["torch"])}
    del grads, out_hip, out_torch
    for fn in routes.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    times = {r: [] for r in routes}
    for _ in range(rounds):
        for r, fn in routes.items():
            times[r].append(_events(fn, iters))
    for r in routes:
        row[r + "_us"] = statistics.median(times[r])
        row[r + "_us_min_max"] = [min(times[r]), max(times[r])]
    q, k, v = (qkv.detach()[:, i * H:(i + 1) * H] for i in range(3))
    out = torch.empty(R, H, dtype=torch.bfloat16, device=dev)
    dqkv = torch.empty(R, 3 * H, dtype=torch.bfloat16, device=dev)
    kern = {"fwd": lambda: hip.attn_frames_fwd(q, k, v, B, T, N, HEADS, scale, out=out),
            "bwd": lambda: hip.attn_frames_bwd(q, k, v, dout, B, T, N, HEADS, scale, dqkv=dqkv)}
    for which, nbytes in (("fwd", 4 * R * H * 2), ("bwd", 7 * R * H * 2)):
        for _ in range(5):
            kern[which]()
        torch.cuda.synchronize()
        ts = [_events(kern[which], iters) for _ in range(rounds)]
        row["kernel_%s_us" % which] = statistics.median(ts)
        row["kernel_%s_us_min_max" % which] = [min(ts), max(ts)]
        row["algorithmic_bytes_%s" % which] = nbytes
        row["kernel_%s_algorithmic_TB_per_s" % which] = nbytes / (row["kernel_%s_us" % which] * 1e-6) / 1e12
    row["torch_over_hip"] = row["torch_us"] / row["hip_us"]
    row["existing_entry_over_hip"] = row["existing_entry_us"] / row["hip_us"]
    return row


def model_step(iters, rounds):
    import torch
    from one_peace_amd import hip
    from one_peace_amd.one_peace_vision import OnePeaceVideoViT, VideoRecognizer, freeze_for_adapters
    hip.lib()
    dev = "cuda:0"
    torch.manual_seed(0)
    T = 16
    net = OnePeaceVideoViT(attention_heads=HEADS, num_frames=T, layers=2, dropout=0.0, drop_path_rate=0.1)
    net.init_weights()
    m = VideoRecognizer(net, 400).to(dev).to(torch.bfloat16).train()
    freeze_for_adapters(m)
    video = torch.randn(B, 3, T, 256, 256, device=dev, dtype=torch.bfloat16)
    target = torch.randint(0, 400, (B,), device=dev)

    def step():
        m.zero_grad(set_to_none=True)
        torch.nn.functional.cross_entropy(m(video).float(), target).backward()

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    times = [_events(step, iters) for _ in range(rounds)]
    return {"shape": MODEL_STEP, "what": "smoke figure: one forward + backward of VideoRecognizer(OnePeaceVideoViT(layers=2, 24 heads, "
            "H = 1536)), bf16, training mode, frozen for adapters", "B": B, "T": T, "image": 256, "iters": iters, "rounds": rounds,
            "step_us": statistics.median(times), "step_us_min_max": [min(times), max(times)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=240, help="seconds per process step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "temporal_attn_mi355x.json"))
    ap.add_argument("--one", default=None, help="(internal) run this step in this process and print its JSON row")
    args = ap.parse_args()
    import torch
    if args.one is not None:
        if not torch.cuda.is_available():
            sys.exit("video_bench: no GPU -- timings are taken on the MI355X only")
        if args.one == MODEL_STEP:
            row = model_step(max(args.iters // 5, 5), args.rounds)
        else:
            name, T = next(s for s in SHAPES if s[0] == args.one)
            row = attn_step(name, T, args.iters, args.rounds)
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
    rec = {"tool": "tools/video_bench.py", "device": device,
           "what": "forward + backward call time, microseconds; median of `rounds` windows of `iters` calls, the routes alternating; "
                   "kernel_*: back-to-back launches of the entry alone",
           "note": "the buffers (38 - 150 MB) stay partly in the 256 MiB Infinity Cache between back-to-back calls: algorithmic bytes over "
                   "time is not an HBM rate", "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if stopped is not None:
        sys.exit("video_bench: step %s %s" % stopped)


if __name__ == "__main__":
    main()
