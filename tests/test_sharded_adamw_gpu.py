"""The optimiser state sharded over data-parallel ranks on the device (csrc/elementwise.hip: adamw_kernel<GROUPS, MASTER, EMA> with the
global index of its first vector, through hip.adamw_step_shard, optim.ShardedFusedAdamW and the sharded ema.FlatEMA).  The criterion
is bit equality with the whole-buffer step, which tests/test_adamw_fp64_gpu.py, test_adamw_master_gpu.py and test_ema_gpu.py hold
against fp64 -- so there is no tolerance here.

  a  the entry over a range against hip.adamw_step_groups / _master / _ema over the whole buffer, from the same state: the four
     arrangements, steps 1 and 1000, clipping off and on (the sum of squares of the FULL gradient), the table adamw_ref.AWKWARD_GROUPS;
     ranges = every shard and tail of worlds 2, 3 and 8 and hand-placed ones.  Inside the range p, m, v, master and ema are the full
     launch's bits; p outside the range and all of g are untouched; every buffer sits between guard regions.  An empty range writes
     nothing
  b  ShardedFusedAdamW with one process standing in for every rank of worlds 1, 2, 3 and 8: every rank's own ranges assembled are the
     FusedAdamW buffers
  c  tools/sharded_adamw_check.py: 2 ranks over gloo on one device; 1 rank over RCCL with the collectives forced (the in-place gather)"""
import copy
import os
import socket
import subprocess
import sys

import pytest
import torch

from tests import adamw_ref as R
from tests import ema_ref as E

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
GUARD = 4096  # elements on either side of every buffer (a multiple of 8: the vector accesses stay aligned)
DECAY = 0.99
ARRANGEMENTS = {"plain": (False, False), "master": (True, False), "ema": (False, True), "master-ema": (True, True)}


def hipmod():
    from one_peace_amd import hip
    return hip


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


class Guarded:
    """A device copy of `t` between two guard regions filled with a canary; looked at on the device."""

    def __init__(self, t):
        self.whole = torch.full((t.numel() + 2 * GUARD,), -1234.5, dtype=t.dtype, device=DEV)
        self.t = self.whole[GUARD:GUARD + t.numel()]
        self.t.copy_(t)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        return bool((self.whole[:GUARD] == -1234.5).all()) and bool((self.whole[-GUARD:] == -1234.5).all())


# ------------------------------------------------------------------------------------------------------------------ a
COUNTS = R.AWKWARD_GROUPS
N8 = sum(COUNTS)
ENDS = [sum(COUNTS[:k + 1]) for k in range(len(COUNTS))]
BIG = COUNTS.index(524288 + 3)


def _ranges():
    """(name, first8, count8): the shards and tails of worlds 2, 3 and 8, then the hand-placed ranges."""
    from one_peace_amd.distributed import shard_layout
    out = []
    for world in (2, 3, 8):
        for rank in range(world):
            lay = shard_layout(8 * N8, world, rank)
            out.append(("w%dr%d" % (world, rank), lay.first8, lay.shard8))
        if lay.tail8:
            out.append(("w%dtail" % world, lay.tail_first8, lay.tail8))
    assert COUNTS[:2] == (1, 1) and COUNTS[-2:] == (1, 1) and ENDS[BIG - 1] == 706 and N8 % 8 != 0
    out += [("on-a-group-end", ENDS[4], 300),                          # starts exactly where group 5 starts
            ("one-after-a-group-end", ENDS[4] + 1, 300),
            ("inside-the-one-vector-groups", 1, 100),                  # starts on the second of the two leading one-vector groups
            ("inside-the-closing-one-vector-groups", N8 - 2, 2),
            ("across-the-big-group", ENDS[BIG - 1] - 6, COUNTS[BIG] + 16),  # more than one grid stride; ends in the group after it
            ("inside-the-big-group", ENDS[BIG - 1] + 12345, 524288 + 3 - 20000),
            ("one-vector", ENDS[5], 1),
            ("one-vector-mid-group", ENDS[5] + 77, 1),
            ("the-last-vector", N8 - 1, 1),
            ("everything", 0, N8)]
    return out


def _full_launch(hip, kind, p, master, g, m, v, e, hyper, keep, take, gs, sq, clip_norm):
    with_master, with_ema = ARRANGEMENTS[kind]
    if with_ema:
        hip.adamw_step_groups_ema(p, master if with_master else None, g, m, v, e, *hyper, keep, take, gs, sq, clip_norm)
    elif with_master:
        hip.adamw_step_groups_master(p, master, g, m, v, *hyper, gs, sq, clip_norm)
    else:
        hip.adamw_step_groups(p, g, m, v, *hyper, gs, sq, clip_norm)


@pytest.mark.parametrize("clip", [False, True], ids=["noclip", "clip"])
@pytest.mark.parametrize("step", [1, 1000], ids=["t1", "t1000"])
@pytest.mark.parametrize("kind", list(ARRANGEMENTS))
def test_a_range_gets_the_bits_of_the_full_launch(kind, step, clip):
    from one_peace_amd.ema import _f32
    hip = hipmod()
    with_master, with_ema = ARRANGEMENTS[kind]
    lr, b1, b2, eps, _ = R.HYPER[0]
    master, p, g, m, v, e, gs, clip_norm = E.case_state(8 * N8, step, clip)  # host state, shared with tests/test_ema_gpu.py, never written
    if not with_master:
        master = p.float()  # unused; the reference below needs some buffer
    hyper = R.device_group_tables(COUNTS) + (lr, b1, b2, eps, step)
    keep, take = _f32(DECAY), _f32(1.0 - DECAY)
    old = {k: t.to(DEV) for k, t in dict(p=p, master=master, g=g, m=m, v=v, e=e).items()}
    sq = hip.sqnorm(old["g"]) if clip else None
    ref = {k: t.clone() for k, t in old.items()}  # the whole-buffer launch, once
    _full_launch(hip, kind, ref["p"], ref["master"], ref["g"], ref["m"], ref["v"], ref["e"], hyper, keep, take, gs, sq, clip_norm)
    torch.cuda.synchronize()
    assert float((bits(ref["p"]) != bits(old["p"])).double().mean()) >= 0.9, "the full step leaves the parameters as they were"
    assert same(ref["g"], old["g"])
    state = ["m", "v"] + (["master"] if with_master else []) + (["e"] if with_ema else [])
    for name, first8, count8 in _ranges():
        what = "%s-t%d-%s %s [%d, +%d)" % (kind, step, "clip" if clip else "noclip", name, first8, count8)
        a, b = 8 * first8, 8 * (first8 + count8)
        G = {"p": Guarded(old["p"]), "g": Guarded(old["g"])}
        G.update({k: Guarded(old[k][a:b]) for k in state})
        hip.adamw_step_shard(G["p"].t, G["g"].t, first8, count8, G["m"].t, G["v"].t, G["master"].t if with_master else None,
                             G["e"].t if with_ema else None, *hyper, keep, take, gs, sq, clip_norm)
        torch.cuda.synchronize()
        for k, buf in G.items():
            assert buf.intact(), "%s: the guard regions of %s were written" % (what, k)
        assert same(G["g"].t, old["g"]), "%s: the gradient buffer was written" % what
        assert same(G["p"].t[:a], old["p"][:a]) and same(G["p"].t[b:], old["p"][b:]), "%s: p outside the range was written" % what
        assert same(G["p"].t[a:b], ref["p"][a:b]), "%s: p inside the range differs from the full launch" % what
        for k in state:
            assert same(G[k].t, ref[k][a:b]), "%s: %s differs from the full launch" % (what, k)
        assert not same(G["m"].t, old["m"][a:b]), "%s: the range was not stepped" % what


def test_an_empty_range_writes_nothing():
    hip = hipmod()
    lr, b1, b2, eps, _ = R.HYPER[0]
    master, p, g, m, v, e, gs, clip_norm = E.case_state(8 * N8, 1000, False)
    end8, scale, wd = R.device_group_tables(COUNTS)
    n = 8 * 64
    host = dict(p=p, g=g, m=m[:n], v=v[:n], master=master[:n], e=e[:n])
    G = {k: Guarded(t) for k, t in host.items()}
    L = hip.lib()
    for first8 in (0, 193, N8):
        rc = L.op_adamw_step_shard(hip.ptr(G["p"].t), hip.ptr(G["g"].t), 8 * N8, first8, 0, hip.ptr(G["m"].t), hip.ptr(G["v"].t),
                                   hip.ptr(G["master"].t), hip.ptr(G["e"].t), hip.ptr(end8), hip.ptr(scale), hip.ptr(wd), end8.numel(),
                                   lr, b1, b2, eps, 1000, 1.0, None, 0.0, 0.99, 0.01, hip.stream())
        assert rc == 0
        empty = torch.empty(0, dtype=torch.float32, device=DEV)
        hip.adamw_step_shard(G["p"].t, G["g"].t, first8, 0, empty, empty, None, None, end8, scale, wd, lr, b1, b2, eps, 1000)
    torch.cuda.synchronize()
    for k, buf in G.items():
        assert buf.intact() and same(buf.t, host[k].to(DEV)), k
    with pytest.raises(RuntimeError):  # a state buffer that does not cover the range never reaches the kernel
        hip.adamw_step_shard(G["p"].t, G["g"].t, 0, 65, G["m"].t, G["v"].t, None, None, end8, scale, wd, lr, b1, b2, eps, 1000)
    with pytest.raises(RuntimeError):  # nor a range past the end
        hip.adamw_step_shard(G["p"].t, G["g"].t, N8 - 63, 64, G["m"].t, G["v"].t, None, None, end8, scale, wd, lr, b1, b2, eps, 1000)
    torch.cuda.synchronize()
    for k, buf in G.items():
        assert buf.intact() and same(buf.t, host[k].to(DEV)), k


# ------------------------------------------------------------------------------------------------------------------ b
WORLDS = (1, 2, 3, 8)
STEPS = 3
HYPER = dict(lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05)
GRAD_SCALE, CLIP_NORM = 0.25, 0.05
_BASE, _REF = {}, {}


def _check_tool():
    from tools import sharded_adamw_check as C
    return C


def _flat(model):
    from one_peace_amd.distributed import FlatParameters
    return FlatParameters(model, *_check_tool().groups_of(model))


def _base():
    if not _BASE:
        model = _check_tool().build_module(WORLDS).to(DEV).to(torch.bfloat16)
        numel = _flat(copy.deepcopy(model)).numel
        gen = torch.Generator().manual_seed(5)
        _BASE["model"] = model
        _BASE["grads"] = [(0.3 * torch.randn(numel, generator=gen)).to(torch.bfloat16).to(DEV) for _ in range(STEPS)]
    return _BASE["model"], _BASE["grads"]


def _reference(kind):
    """FusedAdamW over the whole buffer, once per arrangement: after every step (params, exp_avg, exp_avg_sq, master, shadow, norm)."""
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd.optim import FusedAdamW
    if kind not in _REF:
        with_master, with_ema = ARRANGEMENTS[kind]
        model, grads = _base()
        flat = _flat(copy.deepcopy(model))
        ema = FlatEMA(flat, decay=0.9, start_update=2) if with_ema else None
        opt = FusedAdamW(flat, master_weights=with_master, ema=ema, **HYPER)
        snaps = []
        for g in grads:
            flat.grads.copy_(g)
            norm = opt.step(grad_scale=GRAD_SCALE, clip_norm=CLIP_NORM)
            assert float(norm) > 10 * CLIP_NORM
            snaps.append(tuple(None if t is None else t.clone() for t in (
                flat.params, opt.exp_avg, opt.exp_avg_sq, opt.master, ema.shadow if ema else None, norm)))
        _REF[kind] = snaps
    return _REF[kind]


@pytest.mark.parametrize("kind", list(ARRANGEMENTS))
@pytest.mark.parametrize("world", WORLDS)
def test_the_ranks_own_ranges_assemble_to_the_unsharded_buffers(world, kind):
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd.optim import ShardedFusedAdamW
    with_master, with_ema = ARRANGEMENTS[kind]
    model, grads = _base()
    snaps = _reference(kind)
    ranks = []
    for rank in range(world):
        flat = _flat(copy.deepcopy(model))
        ema = FlatEMA(flat, decay=0.9, start_update=2, shard=(rank, world)) if with_ema else None
        opt = ShardedFusedAdamW(flat, rank=rank, world=world, master_weights=with_master, ema=ema, **HYPER)
        lay = opt.layout
        assert lay.shard8 == (flat.numel // 8) // world and lay.tail8 == (flat.numel // 8) % world and (world == 1 or lay.tail8 > 0)
        assert opt.exp_avg.numel() == opt.exp_avg_sq.numel() == 8 * (lay.shard8 + lay.tail8)
        assert opt.state_bytes() == (8 + 4 * with_master + 4 * with_ema) * 8 * (lay.shard8 + lay.tail8)
        assert not with_master or opt.master.numel() == lay.local_numel
        assert not with_ema or ema.shadow.numel() == lay.local_numel
        ranks.append((flat, opt, ema, lay))
    numel = ranks[0][0].numel
    for step, g in enumerate(grads):
        ref = dict(zip(("p", "m", "v", "master", "e"), snaps[step][:5]))
        got = {k: torch.full_like(t, float("nan")) for k, t in ref.items() if t is not None}
        for flat, opt, ema, lay in ranks:
            what = "%s world %d rank %d step %d" % (kind, world, lay.rank, step + 1)
            flat.grads.copy_(g)
            before = flat.params.clone()
            norm = opt.step(GRAD_SCALE, CLIP_NORM) if world == 1 else opt.step_local(GRAD_SCALE, CLIP_NORM)
            assert same(norm, snaps[step][5]), "%s: the norm" % what
            own = torch.zeros(numel, dtype=torch.bool, device=DEV)
            for a, b, lo in lay.ranges:
                own[a:b] = True
                got["p"][a:b] = flat.params[a:b]
                for k, t in (("m", opt.exp_avg), ("v", opt.exp_avg_sq), ("master", opt.master), ("e", ema.shadow if ema else None)):
                    if t is not None:
                        got[k][a:b] = t[lo:lo + b - a]
            assert same(flat.params[~own], before[~own]), "%s: parameters outside the own ranges were written" % what
            assert same(flat.grads, g), "%s: the gradients were written" % what
            assert not with_ema or ema.num_updates == step + 1
        torch.cuda.synchronize()
        for k in got:
            assert same(got[k], ref[k]), "%s world %d step %d: the assembled %s is not FusedAdamW's" % (kind, world, step + 1, k)
        for flat, _, _, _ in ranks:
            with torch.no_grad():
                flat.params.copy_(ref["p"])  # what gather_params brings
    if world == 1:  # wholly FusedAdamW, through step(): the gather had nobody to talk to
        flat, opt, ema, _ = ranks[0]
        assert same(flat.params, snaps[-1][0]) and same(opt.exp_avg, snaps[-1][1]) and same(opt.exp_avg_sq, snaps[-1][2])


def test_sharded_ema_step_alone_on_the_device():
    """FlatEMA(shard=).step(): hip.ema_step on the two ranges, against the full average's launch."""
    from one_peace_amd.ema import FlatEMA
    model, grads = _base()
    flat = _flat(copy.deepcopy(model))
    full = FlatEMA(flat, decay=0.9)
    parts = [FlatEMA(flat, decay=0.9, shard=(r, 3)) for r in range(3)]
    for g in grads:
        with torch.no_grad():
            flat.params.add_(g)
        for e in [full] + parts:
            e.step()
    torch.cuda.synchronize()
    assert not same(full.shadow, flat.params.float())
    for e in parts:
        assert e.num_updates == STEPS and same(e.shadow, e.layout.take(full.shadow))


# ------------------------------------------------------------------------------------------------------------------ c
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _run_check_tool(nproc, extra_env):
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(nproc), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "sharded_adamw_check.py")]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    log = r.stdout + r.stderr
    assert r.returncode == 0, log[-8000:]  # the ranks' own tracebacks come before torchrun's summary
    assert log.count("sharded check: IDENTICAL") == nproc, log[-3000:]
    assert log.count("ShardedFusedAdamW") == nproc, log[-3000:]
    return log


def test_two_ranks_over_gloo_on_one_device():
    _run_check_tool(2, {"ONEPEACE_DIST_BACKEND": "gloo", "ONEPEACE_SINGLE_DEVICE_DEBUG": "1"})


def test_one_rank_over_rccl_with_the_collectives_forced():
    """World 1 with ONEPEACE_FORCE_COLLECTIVES: the gradient all-reduce and the IN-PLACE all-gather of the parameters run through RCCL."""
    log = _run_check_tool(1, {"ONEPEACE_FORCE_COLLECTIVES": "1"})
    assert "rank 0 of 1" in log
