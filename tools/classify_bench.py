"""Single-query attention pooling of the fine-tuning head on the device: the HIP kernel pair (ops.attention_pool over
csrc/attnpool.hip) against the torch statement of the same lines (ops.attention_pool_torch: the reference's bmm / masked_fill_ /
softmax / bmm), forward + backward, on the same device buffers.

    python tools/classify_bench.py [--iters 200] [--rounds 7] [--out profiles/attn_pool_mi355x.json]

Shapes: B = 128, heads = 24, hd = 64 (the 4B model's head) at S = 256 (image head: 16 x 16 patches), S = 71 (the text keys of a vqa
batch) and S = 749 (15 s of audio); bf16; right padding of every second sample to 3/4 of S for the text and audio shapes.

Method: device events around `iters` forward + backward calls, every shape and route warmed up first, the two routes alternating round
by round in one process; the median over the rounds and their spread, in microseconds per call (forward + backward, launch gaps
included: a call time, not a kernel time).  Achieved bytes/s = the algorithmic bytes of the op -- forward 4 B S H + 4 B heads S + 2 B H,
backward 8 B S H + 4 B heads S + 6 B H -- over the HIP route's call time.  There is no CPU mode: without a device the tool fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("image", 128, 256, 24, 64, False), ("vqa_text", 128, 71, 24, 64, True), ("audio_15s", 128, 749, 24, 64, True)]


def algorithmic_bytes(B, S, heads, hd):
    H = heads * hd
    return (4 * B * S * H + 4 * B * heads * S + 2 * B * H) + (8 * B * S * H + 4 * B * heads * S + 6 * B * H)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attn_pool_mi355x.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("classify_bench: no GPU -- timings are taken on the MI355X only")
    from one_peace_amd import hip, ops
    hip.lib()
    dev = "cuda:0"
    routes = {"hip": ops.attention_pool, "torch": ops.attention_pool_torch}
    results = []
    for name, B, S, heads, hd, padded in SHAPES:
        H = heads * hd
        g = torch.Generator().manual_seed(S)
        k = torch.randn(B, S, H, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
        v = torch.randn(B, S, H, generator=g).to(dev, torch.bfloat16).requires_grad_(True)
        q = (torch.randn(1, 1, heads, hd, generator=g) * 0.02).to(dev, torch.bfloat16).requires_grad_(True)
        dout = torch.randn(B, H, generator=g).to(dev, torch.bfloat16)
        pad = torch.zeros(B, S, dtype=torch.bool)
        if padded:
            pad[1::2, (3 * S) // 4:] = True
        pad = pad.to(dev)

        def call(fn):
            k.grad = v.grad = q.grad = None
            fn(k, v, q, pad).backward(dout)

        outs = {r: fn(k, v, q, pad).detach().float() for r, fn in routes.items()}
        agree = float((outs["hip"] - outs["torch"]).norm() / outs["torch"].norm())
        for fn in routes.values():
            for _ in range(10):
                call(fn)
        torch.cuda.synchronize()
        times = {r: [] for r in routes}
        for _ in range(args.rounds):
            for r, fn in routes.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    call(fn)
                e1.record()
                e1.synchronize()
                times[r].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        row = {"shape": name, "B": B, "S": S, "heads": heads, "hd": hd, "padded": padded, "iters": args.iters, "rounds": args.rounds,
               "algorithmic_bytes": algorithmic_bytes(B, S, heads, hd), "rel_diff_hip_vs_torch": agree}
        for r in routes:
            row[r + "_us"] = statistics.median(times[r])
            row[r + "_us_min_max"] = [min(times[r]), max(times[r])]
        row["hip_achieved_TB_per_s"] = row["algorithmic_bytes"] / (row["hip_us"] * 1e-6) / 1e12
        row["torch_over_hip"] = row["torch_us"] / row["hip_us"]
        results.append(row)
        print(json.dumps(row))
    rec = {"tool": "tools/classify_bench.py", "device": torch.cuda.get_device_name(0), "what": "forward + backward call time, microseconds",
           "results": results}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
