"""Times op_sim_topk (csrc/retrieval.hip) against the two ways of retrieving that form the score matrix, in one run:

  gemm_f32    op_gemm_nt writing the full fp32 score matrix (EPI_F32): the floor of any materialising approach (no top-k at all)
  torch       torch.matmul (bf16, hipBLASLt) + torch.topk(k) on the [M, N] scores

    python tools/retrieval_bench.py [--reps 20] [--shapes coco_i2t,coco_t2i,search,gallery] [--out FILE]

Shapes (D = 1536, the 4B model's embedding width, k = 10): COCO 5 000 images x 25 010 captions in both directions, a search shape
(64 queries x 10^6 gallery rows) and a gallery-scale shape (10^5 x 10^6), whose 400 GB score matrix only op_sim_topk can do without.
Each method is warmed up, then timed with device events one call at a time; the median of --reps calls is reported (the
gallery-scale shape takes --reps-big).  op_gemm_nt needs N % 8 == 0: at N = 25 010 its gallery is zero-padded to 25 016 rows.
One JSON line per (shape, method): milliseconds, TFLOP/s of the 2 M N D operations, and the ratio to gemm_f32.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from one_peace_amd import hip  # noqa: E402

SHAPES = {"coco_i2t": (5000, 25010), "coco_t2i": (25010, 5000), "search": (64, 1000000), "gallery": (100000, 1000000)}
D, K = 1536, 10


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out), min(out), max(out)


def unit(rows, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.randn(rows, D, device="cuda", generator=g)
    return torch.nn.functional.normalize(x, dim=1).to(torch.bfloat16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-big", type=int, default=5)
    ap.add_argument("--shapes", default="coco_i2t,coco_t2i,search,gallery")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "retrieval_bench.py measures on the GPU"
    rows = []
    for name in args.shapes.split(","):
        M, N = SHAPES[name]
        q, g = unit(M, 1), unit(N, 2)
        flop = 2.0 * M * N * D
        big = name == "gallery"
        reps = args.reps_big if big else args.reps
        res = {}
        splits = hip.lib().op_sim_topk_splits(M, N, 0)
        res["sim_topk"] = timed(lambda: hip.sim_topk(q, g, K), reps, warmup=1 if big else 3)
        if not big:
            Np = (N + 7) // 8 * 8
            gp = g if Np == N else torch.cat([g, g.new_zeros(Np - N, D)])
            c = torch.empty(M, Np, dtype=torch.float32, device="cuda")
            res["gemm_f32"] = timed(lambda: hip.gemm_nt(q, [gp], out=c, epilogue=hip.EPI_F32), reps)
            del c
            res["torch"] = timed(lambda: torch.topk(q @ g.t(), K, dim=1), reps)
            torch.cuda.empty_cache()
        for method, (med, lo, hi) in res.items():
            row = {"shape": name, "M": M, "N": N, "D": D, "k": K, "method": method, "ms": round(med, 4), "ms_min": round(lo, 4),
                   "ms_max": round(hi, 4), "reps": reps, "tflops": round(flop / med / 1e9, 1)}
            if method == "sim_topk":
                row["splits"] = splits
            if "gemm_f32" in res:
                row["x_gemm_f32"] = round(med / res["gemm_f32"][0], 3)
            rows.append(row)
            print(json.dumps(row), flush=True)
        del q, g
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
