"""The fused AdamW step with and without the fp32 master copy (csrc/elementwise.hip: adamw_kernel<GROUPS, MASTER>).

    python tools/adamw_master_bench.py [--numel 3890000000] [--groups 84] [--launches 25] [--warmup 5] [--out FILE]
    python tools/adamw_master_bench.py --lost-updates [--lr 5e-4 2e-4 7e-5 8.5e-6 9.3e-7] [--steps 1 10]

Timing: the flat buffers of the 4B model (3.89e9 elements, rounded to a multiple of 8) and a table of 84 groups like the model's (42
layer ids x decay / no decay, lr scales 0.9^k), clipping on (the sum of squares is computed once, outside the timed launches).  Every
launch has its own pair of device events; the two kernels alternate launch by launch after the warm-up, so both see the same
machine; the median, minimum and maximum per kernel in ms, the algorithmic bytes per parameter (22 and 28), the achieved TB/s, and
`master_over_plain_bytes_per_s`, the ratio of the two rates.  One JSON record.  Before timing, the last vector of the buffers (element
index past 2^31) is checked against the torch statement of the step.  There is no CPU mode: without a device the tool fails.

--lost-updates: the share of bf16 parameters that steps leave bit-identical, on a stand-in distribution -- p = bf16(N(0, 0.02^2)),
2^20 elements, r = 0.5 clamp(N(0, 1), +-3) standing for m_hat / (sqrt(v_hat) + eps), wd = 0.05 -- for a list of lr_g.  The moments are
set so that ONE kernel step applies exactly lr_g r (g = 0, m = r / beta1, v = 1 / beta2, step 10^6: bias corrections of 1), and are
reset before every step.  Per lr_g and number of steps: the share of p unchanged without the master, of p unchanged with it (after
one step from a master equal to p it is the same share: the cast rounds the same value), and of masters unchanged.  Plain tensor
comparison on the host.  It is a stand-in, not a training run."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BETAS, EPS, WD = (0.9, 0.98), 1e-6, 0.05
BYTES = {"plain": 22, "master": 28}  # p r+w 4 | master r+w 8 + p w 2;  g r 2;  m and v r+w 16


def group_table(numel, n_groups, dev):
    """n_groups / 2 layer ids, each a large decayed group and a small one without decay (0.2 % of the layer), lr scale 0.9^k."""
    layers = max(n_groups // 2, 1)
    n8 = numel // 8
    ends, scales, wds = [], [], []
    for k in range(layers):
        hi = n8 * (k + 1) // layers
        lo = ends[-1] if ends else 0
        small = max((hi - lo) // 500, 1)
        if n_groups >= 2 and hi - small > lo:
            ends += [hi - small, hi]
            scales += [0.9 ** (layers - 1 - k)] * 2
            wds += [WD, 0.0]
        else:
            ends.append(hi)
            scales.append(0.9 ** (layers - 1 - k))
            wds.append(WD)
    assert ends[-1] == n8 and all(a < b for a, b in zip(ends, ends[1:])) and len(ends) <= 256
    return (torch.tensor(ends, dtype=torch.int64, device=dev), torch.tensor(scales, dtype=torch.float32, device=dev),
            torch.tensor(wds, dtype=torch.float32, device=dev))


def filled(numel, dtype, dev, scale, seed, positive=False, chunk=1 << 28):
    out = torch.empty(numel, dtype=dtype, device=dev)
    gen = torch.Generator(device=dev).manual_seed(seed)
    for lo in range(0, numel, chunk):
        x = torch.randn(min(chunk, numel - lo), generator=gen, device=dev) * scale
        out[lo:lo + x.numel()] = x.abs() if positive else x
    return out


def bench(args):
    from one_peace_amd import hip
    dev = "cuda"
    numel = args.numel // 8 * 8
    end8, scale, wd = group_table(numel, args.groups, dev)
    p = filled(numel, torch.bfloat16, dev, 0.02, 1)
    g = filled(numel, torch.bfloat16, dev, 1e-3, 2)
    state = {k: (filled(numel, torch.float32, dev, 1e-3, 3), filled(numel, torch.float32, dev, 1e-6, 4, positive=True)) for k in BYTES}
    p_plain, master = p.clone(), p.float()
    sq = hip.sqnorm(g)
    lr, step, clip = 5e-4, 1000, 1.0

    def launch(kind):
        m, v = state[kind]
        if kind == "plain":
            hip.adamw_step_groups(p_plain, g, m, v, end8, scale, wd, lr, BETAS[0], BETAS[1], EPS, step, 1.0, sq, clip)
        else:
            hip.adamw_step_groups_master(p, master, g, m, v, end8, scale, wd, lr, BETAS[0], BETAS[1], EPS, step, 1.0, sq, clip)

    # the last vector, at an element index past 2^31 for the default size, against the torch statement of one step
    tail = slice(numel - 8, numel)
    m0, v0, w0 = state["master"][0][tail].clone(), state["master"][1][tail].clone(), master[tail].clone()
    launch("master")
    torch.cuda.synchronize()
    c = min(1.0, clip / (float(sq.double().sqrt()) + 1e-6))
    gt = g[tail].double() * c
    m1 = BETAS[0] * m0.double() + (1 - BETAS[0]) * gt
    v1 = BETAS[1] * v0.double() + (1 - BETAS[1]) * gt * gt
    lr_g = lr * float(scale[-1])
    want = w0.double() * (1 - float(wd[-1]) * lr_g) - lr_g * ((1 - BETAS[1] ** step) ** 0.5 / (1 - BETAS[0] ** step)) * m1 / (v1.sqrt() + EPS)
    err = float((master[tail].double() - want).abs().max())
    assert err <= 1e-6 * float(want.abs().max()) + 1e-9, "last vector: master off by %g" % err
    assert torch.equal(p[tail], master[tail].to(torch.bfloat16)), "last vector: p is not bf16(master)"

    for _ in range(args.warmup):
        for kind in BYTES:
            launch(kind)
    torch.cuda.synchronize()
    ev = {k: [] for k in BYTES}
    for _ in range(args.launches):
        for kind in BYTES:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(kind)
            b.record()
            ev[kind].append((a, b))
    torch.cuda.synchronize()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "numel": numel, "groups": int(end8.numel()),
           "launches_each": args.launches, "warmup_each": args.warmup, "clip": True, "order": "alternating, one event pair per launch"}
    for kind in BYTES:
        ms = [a.elapsed_time(b) for a, b in ev[kind]]
        med = statistics.median(ms)
        rec[kind] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                     "bytes_per_param": BYTES[kind], "tb_per_s": round(BYTES[kind] * numel / (med * 1e-3) / 1e12, 4)}
    rec["master_over_plain_bytes_per_s"] = round(rec["master"]["tb_per_s"] / rec["plain"]["tb_per_s"], 4)
    rec["master_over_plain_ms"] = round(rec["master"]["ms_median"] / rec["plain"]["ms_median"], 4)
    assert bool(torch.isfinite(master[tail]).all()) and bool(torch.isfinite(p_plain[tail].float()).all())
    return [rec]


def lost_updates(args):
    from one_peace_amd import hip
    dev = "cuda"
    n = 1 << 20
    gen = torch.Generator().manual_seed(0)
    p0 = (torch.randn(n, generator=gen) * 0.02).to(torch.bfloat16).to(dev)
    r = (0.5 * torch.randn(n, generator=gen).clamp(-3, 3)).to(dev)
    g = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    m0, v0 = r / BETAS[0], torch.full((n,), 1.0 / BETAS[1], device=dev)
    end8 = torch.tensor([n // 8], dtype=torch.int64, device=dev)
    one, wd = torch.ones(1, device=dev), torch.full((1,), WD, device=dev)
    same = lambda a, b: float((a.view(torch.int16) == b.view(torch.int16)).double().mean()) if a.dtype == torch.bfloat16 else float(  # noqa: E731
        (a.view(torch.int32) == b.view(torch.int32)).double().mean())
    recs = []
    for lr in args.lr:
        for steps in args.steps:
            p_plain, p_mast, master = p0.clone(), p0.clone(), p0.float()
            for _ in range(steps):
                m, v = m0.clone(), v0.clone()
                hip.adamw_step_groups(p_plain, g, m, v, end8, one, wd, lr, BETAS[0], BETAS[1], 0.0, 10 ** 6)
                m, v = m0.clone(), v0.clone()
                hip.adamw_step_groups_master(p_mast, master, g, m, v, end8, one, wd, lr, BETAS[0], BETAS[1], 0.0, 10 ** 6)
            torch.cuda.synchronize()
            recs.append({"lr_g": lr, "steps": steps, "p_unchanged_without_master": round(same(p_plain, p0), 4),
                         "p_unchanged_with_master": round(same(p_mast, p0), 4), "master_unchanged": round(same(master, p0.float()), 4)})
    return recs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=int, default=3890000000)
    ap.add_argument("--groups", type=int, default=84)
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--lost-updates", action="store_true")
    ap.add_argument("--lr", type=float, nargs="+", default=[5e-4, 2e-4, 7e-5, 8.5e-6, 9.3e-7])
    ap.add_argument("--steps", type=int, nargs="+", default=[1, 10])
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("adamw_master_bench: no GPU; this tool measures on the device only")
    if not args.lost_updates and args.launches < 20:
        sys.exit("adamw_master_bench: at least 20 timed launches of each kernel")
    import one_peace_amd  # noqa: F401
    recs = lost_updates(args) if args.lost_updates else bench(args)
    lines = [json.dumps(r) for r in recs]
    print("\n".join(lines), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
