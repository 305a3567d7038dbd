"""The optimiser state sharded over data-parallel ranks, without a GPU: distributed.shard_layout; the C entry op_adamw_step_shard
(declared, exported, in the ctypes table, every refusal before any launch); optim.ShardedTorchAdamW and the sharded ema.FlatEMA with
one process standing in for every rank of worlds 1, 2, 3 and 8 against optim.TorchAdamW, bit for bit; tools/sharded_adamw_check.py
over gloo; and TorchAdamW / FlatEMA themselves against their rule as it stood before it was factored, written out here.

No tolerance anywhere: the update rule does not depend on the position of an element, so a rank's ranges must hold the bits the
unsharded step stores (which tests/test_adamw_ref_cpu.py, test_adamw_master_cpu.py and test_ema_cpu.py hold against fp64)."""
import copy
import ctypes
import os
import re
import socket
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLDS = (1, 2, 3, 8)
STEPS = 3
HYPER = dict(lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05)
GRAD_SCALE, CLIP_NORM = 0.25, 0.05


def bits(t):
    return t.detach().contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


# ------------------------------------------------------------------------------------------------------------------
# the layout
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", (1, 2, 3, 8, 16))
@pytest.mark.parametrize("numel8", (1, 7, 8, 9, 1000, 1001))
def test_shards_are_equal_disjoint_aligned_and_the_tail_is_short(numel8, world):
    from one_peace_amd.distributed import shard_layout
    lays = [shard_layout(8 * numel8, world, r) for r in range(world)]
    S8 = numel8 // world
    covered = torch.zeros(8 * numel8, dtype=torch.int32)
    for r, lay in enumerate(lays):
        assert (lay.shard8, lay.tail8, lay.first8, lay.tail_first8) == (S8, numel8 - world * S8, r * S8, world * S8)
        assert 0 <= lay.tail8 < world and lay.local_numel == 8 * (S8 + lay.tail8) and lay.gathered_numel == 8 * world * S8
        local = 0
        for a, b, lo in lay.ranges:
            assert a % 8 == 0 and b % 8 == 0 and lo == local and 0 <= a < b <= 8 * numel8
            local += b - a
        assert local == lay.local_numel
        full = torch.arange(8 * numel8)
        assert torch.equal(lay.take(full), torch.cat([full[8 * r * S8:8 * (r + 1) * S8], full[8 * world * S8:]]))
        covered[8 * r * S8:8 * (r + 1) * S8] += 1           # the shard: this rank alone
    assert bool((covered[:8 * world * S8] == 1).all()) and bool((covered[8 * world * S8:] == 0).all())  # the tail: everybody's
    if world == 1:
        assert lays[0].ranges == [(0, 8 * numel8, 0)] and lays[0].tail8 == 0
    if S8 == 0:
        assert all(lay.ranges == [(0, 8 * numel8, 0)] for lay in lays), "everything is tail"


def test_the_layout_refuses_what_it_cannot_place():
    from one_peace_amd.distributed import resolve_shard, shard_layout
    for numel, world, rank in ((12, 2, 0), (16, 0, 0), (16, 2, 2), (16, 2, -1)):
        with pytest.raises(ValueError):
            shard_layout(numel, world, rank)
    assert resolve_shard(None, None) == (0, 1) and resolve_shard(2, 3) == (2, 3)
    with pytest.raises(ValueError):
        resolve_shard(1, None)


# ------------------------------------------------------------------------------------------------------------------
# the C entry
# ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib_path():
    import importlib.util
    spec = importlib.util.spec_from_file_location("onepeace_build", os.path.join(ROOT, "one-peace_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


SHARD_ARGS = ["void* p", "const void* g", "int64_t numel", "int64_t first8", "int64_t count8", "float* m", "float* v", "float* master",
              "float* ema", "const int64_t* group_end8", "const float* group_lr_scale", "const float* group_weight_decay",
              "int64_t n_groups", "float lr", "float beta1", "float beta2", "float eps", "int64_t step", "float grad_scale",
              "const float* grad_sqnorm", "float clip_norm", "float ema_keep", "float ema_take", "void* stream"]


def test_the_entry_is_declared_exported_and_in_the_ctypes_table(lib_path):
    from one_peace_amd import hip
    text = open(os.path.join(ROOT, "include", "onepeace_hip.h")).read()
    found = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+op_adamw_step_shard\s*\(([^;]*?)\)\s*;", text, re.S)
    assert found, "op_adamw_step_shard is not declared in include/onepeace_hip.h"
    comment = " ".join(found.group(1).replace("*", " ").split())
    for words in ("optim/adam.py:58-70", "optim/distributed_fused_adam.py", "Additive: op_abi_version() stays 10"):
        assert words in comment, words
    assert [" ".join(a.split()) for a in found.group(2).split(",")] == SHARD_ARGS
    res, argtypes = hip.SIGNATURES["op_adamw_step_shard"]
    P, I, F = ctypes.c_void_p, ctypes.c_int64, ctypes.c_float
    assert res is ctypes.c_int and argtypes == [P, P, I, I, I, P, P, P, P, P, P, P, I, F, F, F, F, I, F, P, F, F, F, P]
    assert callable(hip.adamw_step_shard)
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "op_adamw_step_shard" in {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert hip.lib().op_abi_version() == 10


FAKE = 1 << 20  # never followed: every check comes before the launch


def _shard_call(L, **kw):
    a = dict(p=FAKE, g=FAKE + (1 << 12), numel=800, first8=10, count8=20, m=FAKE + (2 << 12), v=FAKE + (3 << 12), master=None, ema=None,
             end8=FAKE + (4 << 12), scale=FAKE + (5 << 12), wd=FAKE + (6 << 12), n_groups=4, step=1)
    a.update(kw)
    return L.op_adamw_step_shard(a["p"], a["g"], a["numel"], a["first8"], a["count8"], a["m"], a["v"], a["master"], a["ema"], a["end8"],
                                 a["scale"], a["wd"], a["n_groups"], 1e-3, 0.9, 0.98, 1e-6, a["step"], 1.0, None, 0.0, 0.0, 0.0, None)


REFUSED = {
    "null p": dict(p=None), "null g": dict(g=None), "null m": dict(m=None), "null v": dict(v=None), "null group_end8": dict(end8=None),
    "null group_lr_scale": dict(scale=None), "null group_weight_decay": dict(wd=None),
    "numel % 8": dict(numel=804), "first8 < 0": dict(first8=-1), "count8 < 0": dict(count8=-1),
    "past the end": dict(first8=81, count8=20), "past the end by one": dict(first8=0, count8=101),
    "a start past the end": dict(first8=101, count8=0), "an overflowing sum": dict(first8=2 ** 62, count8=2 ** 62),
    "no groups": dict(n_groups=0), "257 groups": dict(n_groups=257), "step 0": dict(step=0),
    "ema on master": dict(master=FAKE + (7 << 12), ema=FAKE + (7 << 12)),
    "ema inside master": dict(master=FAKE + (7 << 12), ema=FAKE + (7 << 12) + 4 * 159),
    "master inside ema": dict(ema=FAKE + (7 << 12), master=FAKE + (7 << 12) + 4 * 159),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_the_entry_refuses_before_any_launch(lib_path, name):
    """No device is needed: the pointers are never followed, and a call that got as far as a launch would fail differently."""
    from one_peace_amd import hip
    L = hip.lib()
    assert _shard_call(L, **REFUSED[name]) == -22, name
    assert L.op_last_error().startswith(b"adamw_shard: "), L.op_last_error()


def test_an_empty_range_is_ok_without_a_launch(lib_path):
    from one_peace_amd import hip
    L = hip.lib()
    for first8 in (0, 10, 100):  # 100 = numel / 8: the empty range at the very end
        assert _shard_call(L, first8=first8, count8=0) == 0
    assert _shard_call(L, first8=10, count8=0, master=FAKE + (7 << 12), ema=FAKE + (8 << 12)) == 0


# ------------------------------------------------------------------------------------------------------------------
# one process standing in for every rank
# ------------------------------------------------------------------------------------------------------------------
def _module():
    sys.path.insert(0, ROOT)
    from tools import sharded_adamw_check as C
    return C


def _flat(model):
    from one_peace_amd.distributed import FlatParameters
    C = _module()
    return FlatParameters(model, *C.groups_of(model))


_BASE = {}


def _base():
    """The module (bf16), and per step one gradient buffer: built once, never written."""
    if not _BASE:
        C = _module()
        model = C.build_module(WORLDS).to(torch.bfloat16)
        numel = _flat(copy.deepcopy(model)).numel
        gen = torch.Generator().manual_seed(5)
        _BASE["model"] = model
        _BASE["grads"] = [(0.3 * torch.randn(numel, generator=gen)).to(torch.bfloat16) for _ in range(STEPS)]
    return _BASE["model"], _BASE["grads"]


_REF = {}


def _reference(master, with_ema):
    """TorchAdamW over the whole buffer: after every step (params, exp_avg, exp_avg_sq, master, shadow, norm).  Computed once."""
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd.optim import TorchAdamW
    key = (master, with_ema)
    if key not in _REF:
        model, grads = _base()
        flat = _flat(copy.deepcopy(model))
        ema = FlatEMA(flat, decay=0.9, start_update=2) if with_ema else None
        opt = TorchAdamW(flat, master_weights=master, ema=ema, **HYPER)
        snaps = []
        for g in grads:
            flat.grads.copy_(g)
            norm = opt.step(grad_scale=GRAD_SCALE, clip_norm=CLIP_NORM)
            assert float(norm) > 10 * CLIP_NORM  # clipping is active
            snaps.append(tuple(None if t is None else t.clone() for t in (
                flat.params, opt.exp_avg, opt.exp_avg_sq, opt.master, ema.shadow if ema else None, norm)))
        _REF[key] = (flat.numel, [e[2:] for e in flat.entries], snaps)
    return _REF[key]


def test_the_module_has_layer_decay_groups_and_a_tail_at_every_world():
    from one_peace_amd.distributed import shard_layout
    model, _ = _base()
    flat = _flat(copy.deepcopy(model))
    assert flat.numel % 8 == 0 and (flat.numel // 8) % 3 != 0
    assert len({g[2] for g in flat.groups}) >= 4 and {g[3] for g in flat.groups} == {True, False}
    for world in WORLDS[1:]:
        lay = shard_layout(flat.numel, world, 0)
        assert lay.tail8 > 0 and lay.shard8 > 0
        bounds = {g[0] for g in flat.groups}
        assert any(8 * r * lay.shard8 not in bounds for r in range(1, world)), "every shard starts on a group boundary"


@pytest.mark.parametrize("master,with_ema", [(False, False), (True, False), (False, True), (True, True)],
                         ids=["plain", "master", "ema", "master-ema"])
@pytest.mark.parametrize("world", WORLDS)
def test_every_rank_holds_the_bits_of_the_unsharded_step(world, master, with_ema):
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd.optim import ShardedTorchAdamW
    model, grads = _base()
    numel, _, snaps = _reference(master, with_ema)
    for rank in range(world):
        flat = _flat(copy.deepcopy(model))
        ema = FlatEMA(flat, decay=0.9, start_update=2, shard=(rank, world)) if with_ema else None
        opt = ShardedTorchAdamW(flat, rank=rank, world=world, master_weights=master, ema=ema, **HYPER)
        lay = opt.layout
        assert (lay.rank, lay.world) == (rank, world) and opt.exp_avg.numel() == opt.exp_avg_sq.numel() == lay.local_numel
        assert opt.state_bytes() == (8 + 4 * master + 4 * with_ema) * lay.local_numel
        assert (opt.master is None) == (not master) and (not master or opt.master.numel() == lay.local_numel)
        own = torch.zeros(numel, dtype=torch.bool)
        for a, b, _ in lay.ranges:
            own[a:b] = True
        assert int(own.sum()) == lay.local_numel
        for step, g in enumerate(grads):
            ref_p, ref_m, ref_v, ref_master, ref_e, ref_norm = snaps[step]
            what = "world %d rank %d step %d" % (world, rank, step + 1)
            flat.grads.copy_(g)
            before = flat.params.clone()
            norm = opt.step_local(grad_scale=GRAD_SCALE, clip_norm=CLIP_NORM)
            assert same(norm, ref_norm), what
            assert same(flat.params[~own], before[~own]), "%s: step_local wrote parameters outside its ranges" % what
            assert same(flat.params[own], ref_p[own]), "%s: params" % what
            assert not same(flat.params[own], before[own]), "%s: the step moved nothing" % what
            assert same(opt.exp_avg, lay.take(ref_m)) and same(opt.exp_avg_sq, lay.take(ref_v)), "%s: moments" % what
            if master:
                assert same(opt.master, lay.take(ref_master)), "%s: master" % what
            if with_ema:
                assert ema.num_updates == step + 1 and same(ema.shadow, lay.take(ref_e)), "%s: ema" % what
            assert same(flat.grads, g), "%s: the gradients were written" % what
            with torch.no_grad():
                flat.params.copy_(ref_p)  # what gather_params would bring: every other rank's slice
        if world == 1:  # the shard is everything
            assert same(opt.exp_avg, snaps[-1][1]) and bool(own.all())
            opt.gather_params()  # nobody to talk to: a no-op, not an error
        else:
            with pytest.raises(RuntimeError, match="process group"):
                opt.step(grad_scale=GRAD_SCALE, clip_norm=CLIP_NORM)  # the collective step needs real ranks


def test_sync_master_reads_only_the_own_ranges():
    from one_peace_amd.optim import ShardedTorchAdamW
    model, _ = _base()
    flat = _flat(copy.deepcopy(model))
    opt = ShardedTorchAdamW(flat, rank=1, world=3, master_weights=True, **HYPER)
    with torch.no_grad():
        flat.params.copy_(torch.arange(flat.numel).remainder(251).to(torch.bfloat16))
    assert not same(opt.master, opt.layout.take(flat.params).float())
    opt.sync_master()
    assert same(opt.master, opt.layout.take(flat.params).float())
    with pytest.raises(RuntimeError):
        ShardedTorchAdamW(_flat(copy.deepcopy(model)), rank=1, world=3, **HYPER).sync_master()


def test_a_sharded_optimiser_takes_only_its_own_sharded_ema():
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd.optim import ShardedTorchAdamW, TorchAdamW
    model, _ = _base()
    flat = _flat(copy.deepcopy(model))
    for bad in (FlatEMA(flat), FlatEMA(flat, shard=(1, 2)), FlatEMA(flat, shard=(0, 3))):
        with pytest.raises(ValueError):
            ShardedTorchAdamW(flat, rank=0, world=2, ema=bad, **HYPER)
    with pytest.raises(ValueError):
        TorchAdamW(flat, ema=FlatEMA(flat, shard=(0, 2)), **HYPER)  # and the unsharded one no sharded average
    with pytest.raises(ValueError):
        ShardedTorchAdamW(flat, rank=0, world=2, ema=FlatEMA(_flat(copy.deepcopy(model)), shard=(0, 2)), **HYPER)  # other buffers
    ShardedTorchAdamW(flat, rank=0, world=2, ema=FlatEMA(flat, shard=(0, 2)), **HYPER)


def test_sharded_ema_step_alone_and_restore_keep_the_own_ranges():
    from one_peace_amd.ema import FlatEMA
    model, _ = _base()
    live = copy.deepcopy(model)
    flat = _flat(live)
    full = FlatEMA(flat, decay=0.9)
    parts = [FlatEMA(flat, decay=0.9, shard=(r, 3)) for r in range(3)]
    gen = torch.Generator().manual_seed(9)
    for _ in range(3):
        with torch.no_grad():
            flat.params.add_((0.1 * torch.randn(flat.numel, generator=gen)).to(torch.bfloat16))
        for e in [full] + parts:
            e.step()
    used = torch.zeros(flat.numel, dtype=torch.bool)
    for _, _, o, k in flat.entries:
        used[o:o + k] = True
    state, fp32 = full.ema_state(live), full.fp32_params()
    for e in parts:
        lay = e.layout
        assert e.num_updates == 3 and e.shadow.numel() == lay.local_numel and same(e.shadow, lay.take(full.shadow))
        for kwargs, want in (((state, fp32), full.shadow), ((state,), full.shadow.to(torch.bfloat16).float())):
            other = FlatEMA(flat, decay=0.9, shard=(lay.rank, lay.world))
            other.shadow.fill_(-7.0)
            other.restore(*kwargs)
            got, u = other.shadow, lay.take(used)
            assert same(got[u], lay.take(want)[u]) and bool((got[~u] == -7.0).all())
        with pytest.raises(RuntimeError, match="process group"):
            e.full_shadow()  # collective: one process cannot stand in for it
    one = FlatEMA(flat, decay=0.9, shard=(0, 1))  # world 1: everything local
    assert same(one.full_shadow(), flat.params.float()) and one.full_shadow() is not one.shadow
    with one.applied():
        pass
    assert full.layout is None and full.full_shadow() is full.shadow


# ------------------------------------------------------------------------------------------------------------------
# real ranks over gloo
# ------------------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


@pytest.mark.parametrize("ranks", (2, 3))
def test_the_check_tool_over_gloo(ranks):
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(ranks), "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tools", "sharded_adamw_check.py"), "--cpu"]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, OMP_NUM_THREADS="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert (r.stdout + r.stderr).count("sharded check: IDENTICAL") == ranks, (r.stdout + r.stderr)[-4000:]


# ------------------------------------------------------------------------------------------------------------------
# what was factored still gives the bits it gave
# ------------------------------------------------------------------------------------------------------------------
def _parent_torch_adamw_step(params, grads, groups, exp_avg, exp_avg_sq, master, step_count, lr, betas, eps, weight_decay, grad_scale,
                             clip_norm):
    """optim.TorchAdamW.step as it stood before the rule was factored out for the sharded class, on plain tensors."""
    b1, b2 = betas
    g = grads.float() * grad_scale
    norm = g.norm() if clip_norm > 0 else None
    if norm is not None and master is not None:
        norm = torch.linalg.vector_norm(g, dtype=torch.float64).float()
    if norm is not None:
        g = g * (clip_norm / (norm + 1e-6)).clamp(max=1.0)
    exp_avg.mul_(b1).add_(g, alpha=1 - b1)
    exp_avg_sq.mul_(b2).addcmul_(g, g, value=1 - b2)
    update = exp_avg / (exp_avg_sq.sqrt() + eps)
    bias = (1 - b2 ** step_count) ** 0.5 / (1 - b1 ** step_count)
    for start, end, scale, decays in groups:
        if end <= start:
            continue
        pf = params[start:end].float() if master is None else master[start:end]
        if decays and weight_decay != 0:
            pf = pf + pf * (-weight_decay * lr * scale)
        new = pf - lr * scale * bias * update[start:end]
        if master is not None:
            master[start:end].copy_(new)
            new = master[start:end].to(params.dtype)
        params[start:end].copy_(new)
    return norm


@pytest.mark.parametrize("master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("clip", [0.0, CLIP_NORM], ids=["noclip", "clip"])
def test_torch_adamw_and_the_full_ema_give_the_bits_they_gave(master, clip):
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd.optim import TorchAdamW
    model, grads = _base()
    flat = _flat(copy.deepcopy(model))
    ema = FlatEMA(flat, decay=0.9, start_update=2)
    opt = TorchAdamW(flat, master_weights=master, ema=ema, **HYPER)
    p = flat.params.detach().clone()
    m, v = torch.zeros(flat.numel), torch.zeros(flat.numel)
    mast = p.float() if master else None
    shadow = p.float()
    for step, g in enumerate(grads, start=1):
        flat.grads.copy_(g)
        norm = opt.step(grad_scale=GRAD_SCALE, clip_norm=clip)
        with torch.no_grad():
            want = _parent_torch_adamw_step(p, g, flat.groups, m, v, mast, step, HYPER["lr"], HYPER["betas"], HYPER["eps"],
                                            HYPER["weight_decay"], GRAD_SCALE, clip)
            d = 0.0 if step < 2 else 0.9          # FlatEMA.step as it stood: the reference's two lines on the whole buffers
            shadow.mul_(d)
            shadow.add_(p.to(shadow.dtype), alpha=1.0 - d)
        assert (norm is None and want is None) or same(norm, want)
        assert same(flat.params, p) and same(opt.exp_avg, m) and same(opt.exp_avg_sq, v), "step %d" % step
        assert not master or same(opt.master, mast)
        assert ema.num_updates == step and same(ema.shadow, shadow) and ema.shadow.numel() == flat.numel
    assert not same(shadow, p.float()) and not same(p, _flat(copy.deepcopy(model)).params), "the case moved nothing"
