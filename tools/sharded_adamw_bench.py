"""The AdamW step over one rank's shard of the optimiser state (op_adamw_step_shard, optim.ShardedFusedAdamW) beside the whole-buffer
step on the same buffers (csrc/elementwise.hip: adamw_kernel<GROUPS, MASTER, EMA>, one kernel for both).

    python tools/sharded_adamw_bench.py [--numel 3890000000] [--groups 84] [--world 8] [--rank 7] [--launches 25] [--warmup 5] [--out FILE]

One GPU.  The buffers and the table of tools/adamw_master_bench.py: the flat buffers of the 4B model (3.89e9 elements, rounded to a
multiple of 8), 84 groups, clipping on (the sum of squares of the full gradient is computed once, outside the timed launches), plus the
fp32 master and average.  For the four arrangements (plain, master, ema, master+ema) two routes, each timed with its own pair of device
events per launch, alternating launch by launch after the warm-up so that all see the same machine:

    full    the whole-buffer entry (op_adamw_step_groups / _master / _ema): 22, 28, 30 and 36 B/param
    shard   op_adamw_step_shard over the shard of --rank of --world and, inside the same event pair, a second launch over the
            replicated tail if there is one (distributed.shard_layout); its state buffers are the range's slices of the full ones

Per route: median, minimum and maximum in ms, the algorithmic bytes per parameter of the range and the achieved TB/s; per arrangement
`shard_over_full_ms` (expected near 1 / world: the same bytes per parameter over 1 / world of the parameters) and `state_bytes_per_rank`
at world 1 and --world.  Before timing, the last vector of the range (element index past 2^31 for the last rank at the default size)
must come out of the shard entry bit for bit as out of the full launch from the same state.  The all-gather of the updated shards
crosses xGMI and cannot be measured on one GPU: it is recorded as "unmeasured" with its algorithmic size.  One JSON record.  There is no
CPU mode: without a device the tool fails."""
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
ARRANGEMENTS = {"plain": (False, False, 22), "master": (True, False, 28), "ema": (False, True, 30), "master+ema": (True, True, 36)}


def bench(args):
    from one_peace_amd import hip
    from one_peace_amd.distributed import shard_layout
    from one_peace_amd.ema import _f32
    dev = "cuda"
    numel = args.numel // 8 * 8
    lay = shard_layout(numel, args.world, args.rank)
    assert lay.shard8 > 0, "the buffer has fewer vectors than ranks"
    end8, scale, wd = group_table(numel, args.groups, dev)
    p = filled(numel, torch.bfloat16, dev, 0.02, 1)
    g = filled(numel, torch.bfloat16, dev, 1e-3, 2)
    m, v = filled(numel, torch.float32, dev, 1e-3, 3), filled(numel, torch.float32, dev, 1e-6, 4, positive=True)
    master, e = p.float(), p.float()
    sq = hip.sqnorm(g)
    lr, step, clip = 5e-4, 1000, 1.0
    keep, take = _f32(DECAY), _f32(1.0 - DECAY)
    hyper = (end8, scale, wd, lr, BETAS[0], BETAS[1], EPS, step)

    def launch(kind, route):
        with_master, with_ema, _ = ARRANGEMENTS[kind]
        if route == "shard":
            for a, b, _ in lay.ranges:  # the range's slices of the full state buffers are range-local buffers
                hip.adamw_step_shard(p, g, a // 8, (b - a) // 8, m[a:b], v[a:b], master[a:b] if with_master else None,
                                     e[a:b] if with_ema else None, *hyper, keep, take, 1.0, sq, clip)
        elif with_ema:
            hip.adamw_step_groups_ema(p, master if with_master else None, g, m, v, e, *hyper, keep, take, 1.0, sq, clip)
        elif with_master:
            hip.adamw_step_groups_master(p, master, g, m, v, *hyper, 1.0, sq, clip)
        else:
            hip.adamw_step_groups(p, g, m, v, *hyper, 1.0, sq, clip)

    # the last vector of the range: the shard entry against the full launch from the same state, bit for bit
    last = lay.ranges[-1][1]
    tail = slice(last - 8, last)
    bufs = (p, master, m, v, e)
    for kind in ARRANGEMENTS:
        before = [b[tail].clone() for b in bufs]
        launch(kind, "shard")
        got = [b[tail].clone() for b in bufs]
        for b, old in zip(bufs, before):
            b[tail] = old
        launch(kind, "full")
        torch.cuda.synchronize()
        for name, x, b in zip(("p", "master", "m", "v", "ema"), got, bufs):
            assert torch.equal(x.view(torch.int16), b[tail].view(torch.int16)), "last vector of the range: %s of the %s shard launch " \
                "differs from the full launch" % (name, kind)
        assert not torch.equal(m[tail], before[2]), "last vector of the range: the step moved nothing"

    routes = [(kind, route) for kind in ARRANGEMENTS for route in ("full", "shard")]
    for _ in range(args.warmup):
        for r in routes:
            launch(*r)
    torch.cuda.synchronize()
    ev = {r: [] for r in routes}
    for _ in range(args.launches):
        for r in routes:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            launch(*r)
            b.record()
            ev[r].append((a, b))
    torch.cuda.synchronize()
    rec = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__, "numel": numel, "groups": int(end8.numel()),
           "world": args.world, "rank": args.rank, "shard_elements": 8 * lay.shard8, "tail_elements": 8 * lay.tail8,
           "launches_each": args.launches, "warmup_each": args.warmup, "clip": True, "decay": DECAY,
           "order": "alternating, one event pair per launch (shard and tail launch share a pair)"}
    for kind, (with_master, with_ema, bpp) in ARRANGEMENTS.items():
        out = {}
        for route, n in (("full", numel), ("shard", lay.local_numel)):
            ms = [a.elapsed_time(b) for a, b in ev[(kind, route)]]
            med = statistics.median(ms)
            out[route] = {"ms_median": round(med, 4), "ms_min": round(min(ms), 4), "ms_max": round(max(ms), 4), "elements": n,
                          "bytes_per_param": bpp, "tb_per_s": round(bpp * n / (med * 1e-3) / 1e12, 4)}
        out["shard_over_full_ms"] = round(out["shard"]["ms_median"] / out["full"]["ms_median"], 4)
        out["shard_over_full_elements"] = round(lay.local_numel / numel, 6)
        per_el = 4 * (2 + with_master + with_ema)
        out["state_bytes_per_rank"] = {"world_1": per_el * numel, "world_%d" % args.world: per_el * lay.local_numel}
        rec[kind] = out
    rec["all_gather"] = {"ms": "unmeasured", "why": "one GPU: the gather of the updated bf16 shards crosses xGMI",
                         "bytes_per_param_received_per_rank": round(2.0 * (args.world - 1) / args.world, 4),
                         "bytes_received_per_rank": 2 * 8 * lay.shard8 * (args.world - 1)}
    assert all(bool(torch.isfinite(b[tail].float()).all()) for b in bufs)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--numel", type=int, default=3890000000)
    ap.add_argument("--groups", type=int, default=84)
    ap.add_argument("--world", type=int, default=8)
    ap.add_argument("--rank", type=int, default=7)
    ap.add_argument("--launches", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sharded_adamw_bench: no GPU; this tool measures on the device only")
    if args.launches < 20:
        sys.exit("sharded_adamw_bench: at least 20 timed launches of each route")
    import one_peace_amd  # noqa: F401
    line = json.dumps(bench(args))
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()
