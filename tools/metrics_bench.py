"""Times the per-class average precision of the MAP metric three ways on one GPU, from fp32 logits [N, C] on the device to ap [C]:

  reference   the reference's path end to end (one_peace/metrics/map.py:35-44): torch.sigmoid -> .cpu().numpy() ->
              sklearn.metrics.average_precision_score(targets, preds, average=None), i.e. a device-to-host copy and one host sort per
              class.  Without scikit-learn on the box the host part is ops.average_precision's CPU route instead, and the row says so.
  torch_sort  the same formula with torch.sort / cumsum / cummin on the device (the torch statement in ops.py, on CUDA tensors)
  hip         torch.sigmoid + ops.average_precision: op_average_precision (csrc/metrics.hip) behind the wrapper's checks (one sync)
  hip_kernel  hip.average_precision alone on ready fp32 scores and uint8 targets (device events)

    python tools/metrics_bench.py [--reps 20] [--reps-host 3] [--shapes fsd50k,audioset] [--out FILE]

Shapes: N = 10 231 x C = 200 (the FSD50K evaluation split) and N = 20 000 x C = 527.  Targets are Bernoulli with a mean of 3 positives
per row -- a benchmark input, not a claim about the real label density -- logits are normal with standard deviation 4.  Every method is
warmed up and then timed one call at a time, the host clock around a device synchronise (device events for hip_kernel); medians are
reported.  One JSON line per (shape, method) with the ratio to the reference path, the host CPU's name, and the largest distance of the
kernel's values from the reference path's.
"""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from one_peace_amd import hip, ops  # noqa: E402

SHAPES = {"fsd50k": (10231, 200), "audioset": (20000, 527)}


def host_cpu():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


def timed_host(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def timed_events(fn, reps, warmup):
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


def reference_path():
    """(callable(logits, targets) -> numpy ap [C], description)"""
    try:
        import sklearn
        from sklearn.metrics import average_precision_score
    except ImportError:
        def fallback(logits, targets):
            return ops.average_precision(torch.sigmoid(logits).cpu(), targets.cpu())[0].numpy()
        return fallback, "no scikit-learn here: sigmoid -> .cpu() -> ops.average_precision CPU route (torch %d threads)" % torch.get_num_threads()

    def path(logits, targets):
        preds = torch.sigmoid(logits).cpu().numpy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return average_precision_score(targets.cpu().numpy(), preds, average=None)
    return path, "sigmoid -> .cpu().numpy() -> scikit-learn %s average_precision_score(average=None)" % sklearn.__version__


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reps-host", type=int, default=3)
    ap.add_argument("--shapes", default="fsd50k,audioset")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "metrics_bench.py measures on the GPU"
    ref, ref_what = reference_path()
    cpu = host_cpu()
    rows = []
    for name in args.shapes.split(","):
        N, C = SHAPES[name]
        g = torch.Generator(device="cuda").manual_seed(1)
        logits = torch.randn(N, C, device="cuda", generator=g) * 4
        targets = (torch.rand(N, C, device="cuda", generator=g) < 3.0 / C).float()
        sig, y8 = torch.sigmoid(logits), targets.to(torch.uint8)
        res = {"reference": timed_host(lambda: ref(logits, targets), args.reps_host, 1),
               "torch_sort": timed_host(lambda: ops._average_precision_torch(torch.sigmoid(logits), targets != 0), args.reps, 3),
               "hip": timed_host(lambda: ops.average_precision(torch.sigmoid(logits), targets), args.reps, 3),
               "hip_kernel": timed_events(lambda: hip.average_precision(sig, y8), args.reps, 3)}
        want = torch.from_numpy(ref(logits, targets))
        got = ops.average_precision(torch.sigmoid(logits), targets)[0].cpu()
        for method, (med, lo, hi) in res.items():
            row = {"shape": name, "N": N, "C": C, "positives_per_class": round(float(targets.sum()) / C, 1), "method": method,
                   "ms": round(med, 4), "ms_min": round(lo, 4), "ms_max": round(hi, 4),
                   "reps": args.reps_host if method == "reference" else args.reps, "x_reference": round(med / res["reference"][0], 5)}
            if method == "reference":
                row.update(what=ref_what, host_cpu=cpu)
            if method == "hip":
                row["max_abs_diff_to_reference"] = float((got - want).abs().max())
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
