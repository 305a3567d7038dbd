"""AdamW with an fp32 master copy, without a GPU: optim.TorchAdamW(master_weights=True) -- the readable statement of the rule and
the CPU route -- against the fp64 statement of tests/adamw_ref.py under the criteria of tests/adamw_master_ref.py; the two
100-step cases whose updates the bf16-only arrangement rounds away; the criteria themselves against an fp32 emulation of
the order of adamw_kernel<GROUPS, MASTER> with planted errors; the reference's FP16Optimizer arithmetic (tests/golden/adamw_master.pt);
sync_master(), the ABI entry, and FusedAdamW's refusal to run without a GPU."""
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

from tests import adamw_master_ref as M
from tests import adamw_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, step, gradient scale, parameter scale, HYPER index): steps 1 and 1000, both parameter scales; 1e-3 is paired with lr 5e-4 as
# adamw_ref.py's note on later-step states asks
ONE_STEP = ((2040, 1, 1e-2, 1.0, 0), (2040, 1000, 1e-2, 1.0, 0), (8 * 773, 1000, 30.0, 1e-3, 1), (8 * 773, 1, 1e-6, 1.0, 1),
            (8, 2, 1e-2, 1.0, 2))
GROUPS = {8: (1,), 2040: (1, 1, 62, 64, 65, 61, 1), 8 * 773: (255, 257, 1, 259, 1)}  # in 8-element vectors


def _tables(n, wd0):
    counts = GROUPS[n]
    assert 8 * sum(counts) == n
    scale, wd = R.group_tables(len(counts), wd0)
    return counts, scale, wd


def _stand_in_flat(master, g, counts, scale, wd):
    """What TorchAdamW reads of a FlatParameters: the flat bf16 buffers and the group list."""
    ends = torch.cumsum(torch.tensor(counts), 0) * 8
    groups = [(int(e) - 8 * c, int(e), s, w != 0.0) for e, c, s, w in zip(ends, counts, scale, wd)]
    return SimpleNamespace(params=master.to(torch.bfloat16), grads=g.clone(), groups=groups, numel=master.numel())


@pytest.mark.parametrize("case", ONE_STEP, ids=lambda c: "n%d-t%d-g%g-p%g-hp%d" % c)
def test_torch_adamw_with_master_one_step_against_fp64(case):
    from one_peace_amd.optim import TorchAdamW
    n, step, gscale, pscale, hp = case
    lr, b1, b2, eps, wd0 = (R.f32(x) for x in R.HYPER[hp])  # the values the C ABI would carry
    counts, scale, wd = _tables(n, wd0)
    master, p, g, m, v = M.make_master_state(n, step, gscale, pscale, seed=11)
    assert not torch.equal(master, p.float())
    flat = _stand_in_flat(master, g, counts, scale, wd)
    opt = TorchAdamW(flat, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd0, master_weights=True)
    opt.master.copy_(master)
    opt.exp_avg.copy_(m)
    opt.exp_avg_sq.copy_(v)
    opt.step_count = step - 1
    assert opt.step() is None
    exp = R.Expected(master, g, m, v, step, lr, b1, b2, eps, lr_scale=R.expand_groups(counts, scale),
                     weight_decay=R.expand_groups(counts, wd))
    M.assert_step(exp, opt.master, flat.params, opt.exp_avg, opt.exp_avg_sq, "torch %r" % (case,))
    assert torch.equal(flat.grads.view(torch.int16), g.view(torch.int16))


def test_torch_adamw_without_master_is_unchanged_and_keeps_no_master():
    from one_peace_amd.optim import TorchAdamW
    n, step = 2040, 1000
    lr, b1, b2, eps, wd0 = (R.f32(x) for x in R.HYPER[1])
    counts, scale, wd = _tables(n, wd0)
    p, g, m, v = R.make_state(n, step, 1e-2, 1.0, seed=12)
    flat = _stand_in_flat(p.float(), g, counts, scale, wd)
    opt = TorchAdamW(flat, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd0)
    assert opt.master is None
    with pytest.raises(RuntimeError):
        opt.sync_master()
    opt.exp_avg.copy_(m)
    opt.exp_avg_sq.copy_(v)
    opt.step_count = step - 1
    opt.step()
    exp = R.Expected(p, g, m, v, step, lr, b1, b2, eps, lr_scale=R.expand_groups(counts, scale), weight_decay=R.expand_groups(counts, wd))
    exp.assert_step(flat.params, opt.exp_avg, opt.exp_avg_sq, "bf16-only")


@pytest.mark.parametrize("name", list(M.HUNDRED))
def test_hundred_small_steps_accumulate_only_with_a_master(name):
    from one_peace_amd.optim import TorchAdamW
    M.assert_hundred(name, TorchAdamW, "cpu")


# ------------------------------------------------------------------------------------------------------------------
# the criteria against planted errors
# ------------------------------------------------------------------------------------------------------------------
# lr 1e-2 with wd 0.05: the decay term, 5e-4 |p| in the decayed groups, is a quarter of half a bf16 spacing -- enough elements round
# differently with and without it; the other two plants move the master by ~2^-9 |p| against delta = 8 * 2^-24 (|p| + |u|)
PLANT_STATES = ((2040, 1), (8 * 773, 1000))


def _emulated(n, step, planted, clip):
    lr, b1, b2, eps, wd0 = R.HYPER[0]
    counts, scale, wd = _tables(n, wd0)
    master, p, g, m, v = M.make_master_state(n, step, 1e-2, 1.0, seed=13)
    kw = dict(grad_scale=0.25, clip_norm=R.CLIP_NORM if clip else 0.0, lr_scale=R.expand_groups(counts, scale),
              weight_decay=R.expand_groups(counts, wd))
    if clip:  # a norm above the threshold
        g = (g.float() * (4 * 10.0 * R.CLIP_NORM / float(g.float().norm()))).to(torch.bfloat16)
        kw["sqnorm"] = torch.tensor(float(R.sqnorm_fp64(g)), dtype=torch.float32)
    exp = R.Expected(master, g, m, v, step, lr, b1, b2, eps, **kw)
    out = M.emulate_master_fp32(master, p, g, m, v, step, lr, b1, b2, eps, planted=planted, **kw)
    return M.figures(exp, *out)


@pytest.mark.parametrize("n,step", PLANT_STATES)
@pytest.mark.parametrize("clip", [False, True])
def test_the_clean_emulation_passes_the_criteria(n, step, clip):
    f = _emulated(n, step, None, clip)
    assert M.passes(f), f


@pytest.mark.parametrize("n,step", PLANT_STATES)
@pytest.mark.parametrize("planted", M.PLANTED)
def test_a_planted_error_fails_the_criteria(n, step, planted):
    f = _emulated(n, step, planted, False)
    assert not M.passes(f), (planted, f)
    if planted == "p_rounded_before_decay":  # the master is right; only the cast shows it
        assert f["master_bad"] == 0 and f["p_bad"] > 0, f
    else:
        assert f["master_bad"] > 0.9 * f["n"], f


# ------------------------------------------------------------------------------------------------------------------
# the reference's arithmetic
# ------------------------------------------------------------------------------------------------------------------
def test_torch_adamw_with_master_follows_the_reference_fp16_optimizer(golden_dir):
    from one_peace_amd.optim import TorchAdamW
    fx = torch.load(os.path.join(golden_dir, "adamw_master.pt"), weights_only=False)
    worst = M.run_fixture(fx, TorchAdamW, "cpu")
    assert worst <= 1.0


def test_the_fixture_holds_tensors_and_plain_numbers_only(golden_dir):
    path = os.path.join(golden_dir, "adamw_master.pt")
    assert os.path.getsize(path) < 1000000
    fx = torch.load(path, weights_only=True)  # refuses anything but tensors, numbers, strings and plain containers
    assert len(fx["after"]) == len(fx["optim"]["lr"]) == 3
    assert all(t.dtype == (torch.float32 if k.endswith("#master") or k.endswith("#norm") else torch.bfloat16)
               for snap in fx["after"] for k, t in snap.items())


# ------------------------------------------------------------------------------------------------------------------
# sync_master, ABI, no GPU
# ------------------------------------------------------------------------------------------------------------------
def test_sync_master_makes_the_next_step_start_from_an_outside_write():
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.optim import TorchAdamW
    lr, b1, b2, eps, wd0 = 1e-5, 0.9, 0.98, 1e-6, 0.0
    results = {}
    for sync in (False, True):
        model = M.EightParams(1.0).to(torch.bfloat16)
        flat = FlatParameters(model)
        opt = TorchAdamW(flat, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd0, master_weights=True)
        with torch.no_grad():
            flat.params.copy_(torch.arange(2, 10).to(torch.bfloat16))  # weights loaded after the optimiser was built
        assert torch.equal(model.w.detach().float(), torch.arange(2, 10).float())
        if sync:
            opt.sync_master()
            assert torch.equal(opt.master, torch.arange(2, 10).float())
        model.w.grad.fill_(0.01)
        opt.step()
        results[sync] = (opt.master.clone(), flat.params.clone())
    exp = R.Expected(torch.arange(2, 10).float(), torch.full((8,), 0.01).to(torch.bfloat16), torch.zeros(8), torch.zeros(8), 1,
                     lr, b1, b2, eps)
    assert bool(((results[True][0].double() - exp.p).abs() <= exp.delta).all())
    assert torch.equal(results[True][1].float(), torch.arange(2, 10).float())  # a 1e-5 step does not move these bf16 values
    # documented: without sync_master the outside write is overwritten by the cast of the old master
    assert bool((results[False][0] < 1.0).all()) and bool((results[False][1] == 1.0).all())


def _header_args(name):
    text = open(os.path.join(ROOT, "include", "onepeace_hip.h")).read()
    found = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, text, re.S)
    assert found, "%s is not declared in include/onepeace_hip.h" % name
    return [a.strip() for a in found.group(1).split(",")]


def test_abi_entry_and_ctypes_arity():
    from one_peace_amd import hip
    args = _header_args("op_adamw_step_groups_master")
    old = _header_args("op_adamw_step_groups")
    assert len(args) == 19 and args[1] == "float* master" and args[:1] + args[2:] == old
    res, argtypes = hip.SIGNATURES["op_adamw_step_groups_master"]
    old_res, old_types = hip.SIGNATURES["op_adamw_step_groups"]
    assert res is ctypes.c_int and len(argtypes) == 19 and argtypes[:1] + argtypes[2:] == old_types and argtypes[1] is ctypes.c_void_p
    assert callable(hip.adamw_step_groups_master)
    if os.path.exists(hip.LIB_PATH):
        L = ctypes.CDLL(hip.LIB_PATH)
        assert hasattr(L, "op_adamw_step_groups_master")
        L.op_abi_version.restype = ctypes.c_int
        assert L.op_abi_version() == 10


def test_fused_adamw_with_master_raises_on_cpu_tensors():
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.optim import FusedAdamW
    flat = FlatParameters(M.EightParams(1.0).to(torch.bfloat16))  # host tensors: what every machine without a GPU has
    for kw in ({}, {"master_weights": True}):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            FusedAdamW(flat, **kw)
