"""The fp32 weight average (ema.FlatEMA) beside the fused AdamW step: what each way of keeping it costs (csrc/elementwise.hip:
ema_step_kernel, adamw_kernel<GROUPS, MASTER, EMA>).

    python tools/ema_bench.py [--numel 3890000000] [--groups 84] [--launches 25] [--warmup 5] [--layers 40] [--out FILE]

The buffers and the table of tools/adamw_master_bench.py: the flat buffers of the 4B model (3.89e9 elements, rounded to a multiple
of 8), 84 groups, clipping on (the sum of squares is computed once, outside the timed launches), plus the fp32 average.  Routes, each
timed with its own pair of device events per launch, alternating launch by launch after the warm-up so that all see the same machine:

    plain, master                 the AdamW step alone (op_adamw_step_groups / _master): 22 and 28 B/param
    plain+ema, master+ema         that step followed by op_ema_step, two launches inside one event pair: 32 and 38 B/param
    fused, fused_master           op_adamw_step_groups_ema without / with the master: 30 and 36 B/param
    torch_rule                    the reference's rule per tensor in torch over views of the same buffers cut to the 4B model's parameter
                                  shapes (bench.build_model with one layer, its layer repeated --layers times): the fp32 cast of the
                                  parameter, mul_, add_, and the cast of the average back into a bf16 EMA model (utils/ema_module.py:
                                  137-151): 32 B/param

Per route: the median, minimum and maximum in ms, the algorithmic bytes per parameter and the achieved TB/s; `ema_extra_ms` is the
median a route adds to its AdamW step alone; `default_route` is "fused" only if the fused median is below the pair's median with and
without the master.  One JSON record.  Before timing, the last vector of the buffers (element index past 2^31 at the default size)
must come out of the fused entry bit for bit as out of the pair.  There is no CPU mode: without a device the tool fails."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.adamw_master_bench import BETAS, EPS, filled, group_table  # noqa: E402

DECAY = 0.9999
BYTES = {"plain": 22, "master": 28, "plain+ema": 32, "master+ema": 38, "fused": 30, "fused_master": 36, "torch_rule": 32}
ALONE = {"plain+ema": "plain", "fused": "plain", "master+ema": "master", "fused_master": "master"}


def model_shapes(layers):
    """The 4B retrieval model's parameter shapes without building it: one layer built, its shapes repeated."""
    import bench
    one = bench.build_model(1, "cpu")
    named = [(n, tuple(p.shape)) for n, p in one.named_parameters()]
    return [s for n, s in named if ".layers.0." not in n] + [s for n, s in named if ".layers.0." in n] * layers


def views(shapes, numel, *buffers):
    """Per-tensor views of the flat buffers, every start aligned to 8 elements as FlatParameters lays them out; what is left is one vector."""
    out, off = [], 0
    for s in shapes:
        k = 1
        for d in s:
            k *= d
        if off + k > numel:
            break
        out.append(tuple(b[off:off + k].view(s) for b in buffers))
        off += (k + 7) // 8 * 8
    if off < numel:
        out.append(tuple(b[off:] for b in buffers))
    return out


def bench(args):
    from one_peace_amd import hip
    from one_peace_amd.ema import _f32
    dev = "cuda"
    numel = args.numel // 8 * 8
    end8, scale, wd = group_table(numel, args.groups, dev)
    p = filled(numel, torch.bfloat16, dev, 0.02, 1)
    g = filled(numel, torch.bfloat16, dev, 1e-3, 2)
    m, v = filled(numel, torch.float32, dev, 1e-3, 3), filled(numel, torch.float32, dev, 1e-6, 4, positive=True)
    p_plain, master, e = p.clone(), p.float(), p.float()
    ema_model = p.clone()
    per_tensor = views(model_shapes(args.layers), numel, e, p_plain, ema_model)
    sq = hip.sqnorm(g)
    lr, step, clip = 5e-4, 1000, 1.0
    keep, take = _f32(DECAY), _f32(1.0 - DECAY)
    hyper = (end8, scale, wd, lr, BETAS[0], BETAS[1], EPS, step)

    def launch(kind):
        if kind in ("plain", "plain+ema"):
            hip.adamw_step_groups(p_plain, g, m, v, *hyper, 1.0, sq, clip)
        elif kind in ("master", "master+ema"):
            hip.adamw_step_groups_master(p, master, g, m, v, *hyper, 1.0, sq, clip)
        if kind.endswith("+ema"):
            hip.ema_step(e, p_plain if kind == "plain+ema" else p, keep, take)
        elif kind == "fused":
            hip.adamw_step_groups_ema(p_plain, None, g, m, v, e, *hyper, keep, take, 1.0, sq, clip)
        elif kind == "fused_master":
            hip.adamw_step_groups_ema(p, master, g, m, v, e, *hyper, keep, take, 1.0, sq, clip)
        elif kind == "torch_rule":
            with torch.no_grad():
                for ev, pv, bv in per_tensor:
                    ev.mul_(DECAY)
                    ev.add_(pv.to(dtype=ev.dtype), alpha=1 - DECAY)
                    bv.copy_(ev)

    # the last vector: the fused entry against the pair from the same state, bit for bit
    tail = slice(numel - 8, numel)
    for fused, pair, params in (("fused", "plain+ema", p_plain), ("fused_master", "master+ema", p)):
        bufs = (params, master, m, v, e)
        before = [b[tail].clone() for b in bufs]
        launch(fused)
        got = [b[tail].clone() for b in bufs]
        for b, old in zip(bufs, before):
            b[tail] = old
        launch(pair)
        torch.cuda.synchronize()
        for name, a, b in zip(("p", "master", "m", "v", "ema"), got, bufs):
            assert torch.equal(a.view(torch.int16), b[tail].view(torch.int16)), "last vector: %s of %s differs from %s" % (name, fused, pair)
        assert not torch.equal(e[tail], before[4]), "last vector: the average did not move"

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
           "launches_each": args.launches, "warmup_each": args.warmup, "clip": True, "decay": DECAY,
           "torch_rule_tensors": len(per_tensor), "order": "alternating, one event pair per launch (per pair of launches for the +ema routes)"}
    for kind in BYTES:
        ms = [a.elapsed_time(b) for a, b in ev[kind]]
        med = statistics.median(ms)
        rec[kind] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4),
                     "bytes_per_param": BYTES[kind], "tb_per_s": round(BYTES[kind] * numel / (med * 1e-3) / 1e12, 4)}
    for kind, alone in ALONE.items():
        rec[kind]["ema_extra_ms"] = round(rec[kind]["ms_median"] - rec[alone]["ms_median"], 4)
    wins = [rec["fused"]["ms_median"] < rec["plain+ema"]["ms_median"], rec["fused_master"]["ms_median"] < rec["master+ema"]["ms_median"]]
    rec["fused_below_pair"] = {"plain": wins[0], "master": wins[1]}
    rec["default_route"] = "fused" if all(wins) else "pair"
    assert bool(torch.isfinite(e[tail]).all()) and bool(torch.isfinite(master[tail]).all())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=int, default=3890000000)
    ap.add_argument("--groups", type=int, default=84)
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--layers", type=int, default=40)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ema_bench: no GPU; this tool measures on the device only")
    if args.launches < 20:
        sys.exit("ema_bench: at least 20 timed launches of each route")
    import one_peace_amd  # noqa: F401
    line = json.dumps(bench(args))
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
