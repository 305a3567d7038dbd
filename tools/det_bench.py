"""Window attention of the detection branch on the device: ops.window_attention (csrc/windowattn.hip, the packed q|k|v rows read where
they lie, the shared bias and the decomposed relative positions inside the kernel) against (a) the torch statement of the same window
block on the same buffers (ops.window_attention_torch: partition and unpartition copies, the expanded bias add, the decomposed add, fp32
softmax and their autograd backward) and (b) the project's existing attention entry on partitioned copies (ops.spatial_attention with a
frozen relative-position handle and NO decomposed term: it cannot do more; the partition and unpartition copies count in its time).
Forward + backward.  And, as a smoke figure only, one forward + backward of a 4-layer OnePeaceDetViT (three window blocks, one global).

    python tools/det_bench.py [--iters 20] [--rounds 7] [--step-timeout 300] [--out profiles/window_attn_mi355x.json]

Shapes: 24 heads of 64 (H = 1536), an 80 x 80 grid (25 windows of 16 x 16), B = 1 and 2; bf16.

Method: every shape runs in a process of its own under its own time limit (the parent never opens the device; it stops at the first
step that fails or runs out of time, and the steps it did not reach are recorded as "not measured").  Inside a step, after a warm-up of
every route: device events around `iters` forward + backward calls, the routes alternating round by round; the median over the rounds
and their spread, in microseconds per call (a call time: launch gaps, allocations and autograd included).  Kernel time: the same events
around `iters` back-to-back launches of op_attn_window_fwd, resp. _bwd, alone on preallocated buffers, with rel on and off and (backward)
with slabs and parts on and off.  Algorithmic bytes: forward 4 R H 2 B (q, k, v read, out written), backward 7 R H 2 B, R = B * 6400;
algorithmic flops: forward 4 * 256 * 64 per (query, head) for the two main products (+ 6 % for Q rel^T), backward 10 * 256 * 64.  The
buffers are 79 - 275 MB against 256 MiB of Infinity Cache: between back-to-back calls part of them stays on the die, so bytes over time
is NOT an HBM rate; every route is measured under the same condition.  For orientation the record also gives the distance to 16 us of
HBM time and 13.5 us of matrix time per sample of the forward (5 TB/s; the GEMM family's sustained rate).  There is no CPU mode: without
a device the tool fails."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADS, GRID = 24, 80
H = HEADS * 64
SHAPES = [("B1", 1), ("B2", 2)]
MODEL_STEP = "det_4layer_step"
HBM_US_PER_SAMPLE, MATRIX_US_PER_SAMPLE = 16.0, 13.5


def _events(fn, iters):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def attn_step(name, B, iters, rounds):
    import torch
    from one_peace_amd import hip, ops
    from one_peace_amd.one_peace_vision.det_vit import make_bucket_position
    hip.lib()
    dev = "cuda:0"
    R = B * GRID * GRID
    g = torch.Generator().manual_seed(B)
    qkv = torch.randn(R, 3 * H, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
    dout = torch.randn(R, H, generator=g).to(dev, torch.bfloat16)
    table = (0.5 * torch.randn(31 * 31 + 3, HEADS, generator=g)).to(dev, torch.bfloat16)
    bucket = make_bucket_position(16).to(dev)
    bias = torch.nn.functional.embedding(bucket, table).permute(2, 0, 1).contiguous().requires_grad_(True)
    rel_h = (0.1 * torch.randn(31, 64, generator=g)).to(dev, torch.bfloat16).requires_grad_(True)
    rel_w = (0.1 * torch.randn(31, 64, generator=g)).to(dev, torch.bfloat16).requires_grad_(True)
    scale = 0.125
    leaves = (qkv, bias, rel_h, rel_w)

    def autograd_call(fn):
        def call():
            for t in leaves:
                t.grad = None
            fn(qkv, bias, rel_h, rel_w, B, GRID, GRID, HEADS, 16, scale).backward(dout)
            return qkv.grad
        return call

    handle = ops.RelPosBias(table, bucket.to(torch.int32), 256)
    nw = GRID // 16

    def existing_entry():
        qkv.grad = None
        x = qkv.view(B, nw, 16, nw, 16, 3 * H).permute(0, 1, 3, 2, 4, 5).reshape(B * nw * nw * 256, 3 * H)       # window_partition
        o = ops.spatial_attention(x, handle, B * nw * nw, 256, HEADS, scale)
        o = o.view(B, nw, nw, 16, 16, H).permute(0, 1, 3, 2, 4, 5).reshape(R, H)                                   # window_unpartition
        o.backward(dout)
        return qkv.grad

    routes = {"hip": autograd_call(ops.window_attention), "torch": autograd_call(ops.window_attention_torch),
              "existing_entry_no_rel": existing_entry}
    grads, tables = {}, {}
    for r, fn in routes.items():
        grads[r] = fn().detach().float().clone()
        tables[r] = [t.grad.detach().float().clone() for t in leaves[1:] if t.grad is not None]
    with torch.no_grad():
        out_hip = ops.window_attention(qkv, bias, rel_h, rel_w, B, GRID, GRID, HEADS, 16, scale).float()
        out_torch = ops.window_attention_torch(qkv, bias, rel_h, rel_w, B, GRID, GRID, HEADS, 16, scale).float()
    rel = lambda a, b: float((a - b).norm() / b.norm())  # noqa: E731
    row = {"shape": name, "B": B, "grid": GRID, "heads": HEADS, "rows": R, "iters": iters, "rounds": rounds,
           "rel_diff_out_hip_vs_torch": rel(out_hip, out_torch), "rel_diff_dqkv_hip_vs_torch": rel(grads["hip"], grads["torch"])}
    for nm, a, b in zip(("dbias", "drel_h", "drel_w"), tables["hip"], tables["torch"]):
        row["rel_diff_%s_hip_vs_torch" % nm] = rel(a, b)
    # a wrong route must not be timed unnoticed: both routes are bf16 statements of one function, so they differ by a few bf16
    # roundings (2^-8 each; the torch route rounds its scores and probabilities, the kernels do not) -- 0.05 is ten times that, and
    # a route that computes something else is off by order 1
    bad = {k: v for k, v in row.items() if k.startswith("rel_diff_") and not v <= 0.05}
    if bad or len(tables["hip"]) != 3:
        sys.exit("det_bench: the routes disagree: %s" % bad)
    del grads, tables, out_hip, out_torch
    for fn in routes.values():
        for _ in range(3):
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
    bk, rh, rw = bias.detach(), rel_h.detach(), rel_w.detach()
    out = torch.empty(R, H, dtype=torch.bfloat16, device=dev)
    dqkv = torch.empty(R, 3 * H, dtype=torch.bfloat16, device=dev)
    parts, slabs = hip.attn_window_parts(B, GRID, GRID, HEADS)
    drel = torch.empty(parts, 2, 31, 64, dtype=torch.float32, device=dev)
    dbias = torch.empty(slabs, HEADS, 256, 256, dtype=torch.float32, device=dev)
    row["parts"], row["slabs"] = parts, slabs
    kern = {
        "fwd_rel": lambda: hip.attn_window_fwd(q, k, v, bk, rh, rw, B, GRID, GRID, HEADS, scale, out=out),
        "fwd_norel": lambda: hip.attn_window_fwd(q, k, v, bk, None, None, B, GRID, GRID, HEADS, scale, out=out),
        "bwd_rel": lambda: hip.attn_window_bwd(q, k, v, bk, rh, rw, dout, B, GRID, GRID, HEADS, scale, dqkv=dqkv),
        "bwd_norel": lambda: hip.attn_window_bwd(q, k, v, bk, None, None, dout, B, GRID, GRID, HEADS, scale, dqkv=dqkv),
        "bwd_rel_slabs_parts": lambda: hip.attn_window_bwd(q, k, v, bk, rh, rw, dout, B, GRID, GRID, HEADS, scale, dqkv=dqkv,
                                                           drel_part=drel, dbias_slabs=dbias),
        "bwd_norel_slabs": lambda: hip.attn_window_bwd(q, k, v, bk, None, None, dout, B, GRID, GRID, HEADS, scale, dqkv=dqkv,
                                                       dbias_slabs=dbias),
    }
    for which, fn in kern.items():
        fwd = which.startswith("fwd")
        nbytes = (4 if fwd else 7) * R * H * 2
        flops = (4 if fwd else 10) * 256 * 64 * R * HEADS
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = [_events(fn, iters) for _ in range(rounds)]
        us = statistics.median(ts)
        row["kernel_%s_us" % which] = us
        row["kernel_%s_us_min_max" % which] = [min(ts), max(ts)]
        row["kernel_%s_algorithmic_TB_per_s" % which] = nbytes / (us * 1e-6) / 1e12
        row["kernel_%s_algorithmic_TFLOP_per_s" % which] = flops / (us * 1e-6) / 1e12
    row["kernel_fwd_rel_over_hbm_time"] = row["kernel_fwd_rel_us"] / (HBM_US_PER_SAMPLE * B)
    row["kernel_fwd_rel_over_matrix_time"] = row["kernel_fwd_rel_us"] / (MATRIX_US_PER_SAMPLE * B)
    row["torch_over_hip"] = row["torch_us"] / row["hip_us"]
    row["existing_entry_no_rel_over_hip"] = row["existing_entry_no_rel_us"] / row["hip_us"]
    return row


def model_step(iters, rounds):
    import torch
    from one_peace_amd import hip
    from one_peace_amd.one_peace_vision import OnePeaceDetViT
    hip.lib()
    dev = "cuda:0"
    torch.manual_seed(0)
    m = OnePeaceDetViT(attention_heads=HEADS, bucket_size=GRID, layers=4, window_size=16, window_block_indexes=(0, 1, 2),
                       use_decomposed_rel_pos=True, drop_path_rate=0.1).to(dev).to(torch.bfloat16).train()
    image = torch.randn(1, 3, 16 * GRID, 16 * GRID, device=dev, dtype=torch.bfloat16)

    def step():
        m.zero_grad(set_to_none=True)
        m(image)["last_feat"].float().square().mean().backward()

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    times = [_events(step, iters) for _ in range(rounds)]
    return {"shape": MODEL_STEP, "what": "smoke figure: one forward + backward of OnePeaceDetViT(layers=4: three window blocks and one "
            "global block, 24 heads, H = 1536, decomposed rel pos, shared bias trained), bf16, training mode", "B": 1, "image": 16 * GRID,
            "iters": iters, "rounds": rounds, "step_us": statistics.median(times), "step_us_min_max": [min(times), max(times)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds per process step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "window_attn_mi355x.json"))
    ap.add_argument("--one", default=None, help="(internal) run this step in this process and print its JSON row")
    args = ap.parse_args()
    import torch
    if args.one is not None:
        if not torch.cuda.is_available():
            sys.exit("det_bench: no GPU -- timings are taken on the MI355X only")
        if args.one == MODEL_STEP:
            row = model_step(max(args.iters // 5, 3), args.rounds)
        else:
            name, B = next(s for s in SHAPES if s[0] == args.one)
            row = attn_step(name, B, args.iters, args.rounds)
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
    rec = {"tool": "tools/det_bench.py", "device": device,
           "what": "forward + backward call time, microseconds; median of `rounds` windows of `iters` calls, the routes alternating; "
                   "kernel_*: back-to-back launches of the entry alone",
           "note": "the buffers (79 - 275 MB) stay partly in the 256 MiB Infinity Cache between back-to-back calls: algorithmic bytes over "
                   "time is not an HBM rate", "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)
    if stopped is not None:
        sys.exit("det_bench: step %s %s" % stopped)


if __name__ == "__main__":
    main()
