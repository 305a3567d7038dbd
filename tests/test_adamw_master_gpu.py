"""AdamW with an fp32 master copy on the device (csrc/elementwise.hip: adamw_kernel<GROUPS, MASTER> through hip.adamw_step_groups_master
and optim.FusedAdamW(master_weights=True)) under the criteria of tests/adamw_master_ref.py: for EVERY element the stored master within
delta of the fp64 step from the old master, the stored bf16 parameter bit-identical to the round-to-nearest-even cast of the stored
master, the moments inside their bounds.

  a  one step: adamw_ref.SIZES as a single group, the awkward and the full (256) group tables, steps 1 and 1000, with and without
     clipping (the device's own sum of squares goes into the reference).  The master has a non-zero low half in every element and the
     result must differ from what the bf16 parameter would have given; the parameter buffer holds NaNs before the call (it is never
     read); every buffer sits between guard regions.  And from a master that IS float(p): p, m and v bit-identical to what
     hip.adamw_step_groups stores from the same inputs
  b  refused calls: 257 groups, a null master -- nothing launched, nothing written
  c  the two 100-step cases through FusedAdamW, with and without the master
  d  tests/golden/adamw_master.pt (the reference's FP16Optimizer arithmetic) through FusedAdamW(master_weights=True)
  e  the default FusedAdamW keeps no master and calls the old entry point
  f  non-finite gradients, as the existing kernels treat them"""
import copy
import math

import pytest
import torch

from tests import adamw_master_ref as M
from tests import adamw_ref as R
from tests import ema_ref as E

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096  # elements on either side of every buffer (a multiple of 8: the vector loads stay aligned)


def hipmod():
    from one_peace_amd import hip
    return hip


class Guarded:
    """A device copy of `t` between two guard regions filled with a canary."""

    def __init__(self, t):
        self.canary = torch.tensor(-1234.5, dtype=t.dtype)
        self.whole = torch.full((t.numel() + 2 * GUARD,), float(self.canary), dtype=t.dtype, device=DEV)
        self.t = self.whole[GUARD:GUARD + t.numel()]
        self.t.copy_(t)
        assert self.t.data_ptr() % 16 == 0

    def intact(self):
        w = self.whole.cpu()
        return bool((w[:GUARD] == self.canary).all()) and bool((w[-GUARD:] == self.canary).all())


# ------------------------------------------------------------------------------------------------------------------ a
CASES = [("awkward", R.AWKWARD_GROUPS, t, clip) for t in (1, 1000) for clip in (False, True)] + [
    ("full", R.FULL_GROUPS, t, clip) for t in (1, 1000) for clip in (False, True)] + [
    ("single%d" % n, (n // 8,), t, clip) for n, t, clip in zip(R.SIZES, (1, 1000, 1, 1000), (False, True, True, False))] + [
    ("single%d" % n, (n // 8,), t, clip) for n, t, clip in zip(R.SIZES[:2], (1000, 1), (False, False))]


@pytest.mark.parametrize("name,counts,step,clip", CASES, ids=lambda x: None if isinstance(x, tuple) else str(x))
def test_master_step_against_fp64(name, counts, step, clip):
    hip = hipmod()
    what = "%s-t%d-%s" % (name, step, "clip" if clip else "noclip")
    n = 8 * sum(counts)
    lr, b1, b2, eps, _ = R.HYPER[0 if step == 1 else 1]  # from non-zero moments: lr 5e-4 (adamw_ref.py's note on delta and step size)
    gs, clip_norm = (0.25, R.CLIP_NORM) if clip else (1.0, 0.0)
    master, p, g, m, v = M.make_master_state(n, step, 1e-2, 1.0, seed=2)
    if clip:  # the clip states of adamw_ref.py: the scaled norm 40 x the threshold, moments at the scale of the clipped gradient
        _, g, m, v = R.make_clip_state(n, gs, "above", step, seed=2)
        R.assert_clip_landing(g, gs, "above")
    end8, scale, wd = R.device_group_tables(counts)
    G = {k: Guarded(t) for k, t in dict(p=torch.full_like(p, float("nan")), master=master, g=g, m=m, v=v).items()}
    sq = None
    if clip:
        sq = hip.sqnorm(G["g"].t)
        assert R.norm_used(sq, g) <= 1.0
    lr_el, wd_el = R.expand_groups(counts, scale.cpu()), R.expand_groups(counts, wd.cpu())
    exp = R.Expected(master, g, m, v, step, lr, b1, b2, eps, grad_scale=gs, clip_norm=clip_norm, sqnorm=sq, lr_scale=lr_el,
                     weight_decay=wd_el)
    hip.adamw_step_groups_master(G["p"].t, G["master"].t, G["g"].t, G["m"].t, G["v"].t, end8, scale, wd, lr, b1, b2, eps, step, gs,
                                 sq, clip_norm)
    torch.cuda.synchronize()
    for k, b in G.items():
        assert b.intact(), "%s: the guard regions of %s were written" % (what, k)
    assert torch.equal(M.bits16(G["g"].t), M.bits16(g)), "the gradient buffer was written"
    M.assert_step(exp, G["master"].t, G["p"].t, G["m"].t, G["v"].t, what)
    # the fp64 result a step from the bf16 parameter would have had: E.p - (master - p) (1 - wd lr_g)
    from_p = exp.p - (master.double() - p.double()) * (1.0 - R.f32(wd_el) * (R.f32(lr) * R.f32(lr_el)))
    apart = ((G["master"].t.cpu().double() - from_p).abs() > exp.delta).double().mean()
    assert float(apart) >= 0.99, "%s: only %.4f of the masters differ from a step taken from the bf16 parameter" % (what, float(apart))


@pytest.mark.parametrize("name,counts,step,clip", CASES, ids=lambda x: None if isinstance(x, tuple) else str(x))
def test_master_step_matches_the_plain_step_bit_for_bit(name, counts, step, clip):
    """With master == float(p) both routes start the update from the same fp32 number, so they must store the same p, m and v: the
    link between hip.adamw_step_groups and hip.adamw_step_groups_master that test_ema_gpu.py's bitwise test (whose states, buffers and
    changed-share condition this follows) has for the fused entry.  adamw_master_ref.emulate_master_fp32 from these states changes
    0.993 ... 1.000 of the bf16 parameters on the CPU, so neither route passes by leaving p alone."""
    hip = hipmod()
    what = "%s-t%d-%s" % (name, step, "clip" if clip else "noclip")
    lr, b1, b2, eps, _ = R.HYPER[0]
    _, p, g, m, v, _, gs, clip_norm = E.case_state(8 * sum(counts), step, clip)
    hyper = R.device_group_tables(counts) + (lr, b1, b2, eps, step)
    plain = {k: Guarded(t) for k, t in dict(p=p, g=g, m=m, v=v).items()}
    mast = {k: Guarded(t) for k, t in dict(p=torch.full_like(p, float("nan")), master=p.float(), g=g, m=m, v=v).items()}
    sq = hip.sqnorm(plain["g"].t) if clip else None
    hip.adamw_step_groups(plain["p"].t, plain["g"].t, plain["m"].t, plain["v"].t, *hyper, gs, sq, clip_norm)
    hip.adamw_step_groups_master(mast["p"].t, mast["master"].t, mast["g"].t, mast["m"].t, mast["v"].t, *hyper, gs, sq, clip_norm)
    torch.cuda.synchronize()
    for route, G in (("plain", plain), ("master", mast)):
        for k, b in G.items():
            assert b.intact(), "%s: the guard regions of %s (%s route) were written" % (what, k, route)
        assert torch.equal(M.bits(G["g"].t), M.bits(g)), "%s: the %s route wrote the gradient buffer" % (what, route)
    for k in ("p", "m", "v"):
        assert torch.equal(M.bits(mast[k].t), M.bits(plain[k].t)), "%s: %s differs between the master and the plain route" % (what, k)
    assert M.cast_matches(mast["p"].t, mast["master"].t) == 0, "%s: p is not bf16(master)" % what
    share = E.changed_share(plain["p"].t, p)
    assert share >= 0.9, "%s: only %.3f of the bf16 parameters changed in the step" % (what, share)


# ------------------------------------------------------------------------------------------------------------------ b
def _refusal_state(n_groups):
    counts = (1,) * n_groups
    master, p, g, m, v = M.make_master_state(8 * n_groups, 2, 1e-2, 1.0, seed=3)
    host = dict(p=p, master=master, g=g, m=m, v=v)
    return host, {k: t.to(DEV) for k, t in host.items()}, R.device_group_tables(counts)


def _untouched(host, dev):
    return all(torch.equal(dev[k].cpu().view(torch.int16), host[k].view(torch.int16)) for k in host)


def test_master_step_rejects_257_groups():
    hip = hipmod()
    host, d, (end8, scale, wd) = _refusal_state(257)
    lr, b1, b2, eps, _ = R.HYPER[0]
    with pytest.raises(RuntimeError):
        hip.adamw_step_groups_master(d["p"], d["master"], d["g"], d["m"], d["v"], end8, scale, wd, lr, b1, b2, eps, 2)
    torch.cuda.synchronize()
    assert _untouched(host, d)
    k = 2048
    hip.adamw_step_groups_master(d["p"][:k], d["master"][:k], d["g"][:k], d["m"][:k], d["v"][:k], end8[:256], scale[:256], wd[:256],
                                 lr, b1, b2, eps, 2)  # 256 are taken
    torch.cuda.synchronize()
    assert not torch.equal(d["master"][:k].cpu(), host["master"][:k]) and M.cast_matches(d["p"][:k], d["master"][:k]) == 0
    assert torch.equal(d["master"][k:].cpu(), host["master"][k:])


def test_master_step_rejects_a_null_master():
    hip = hipmod()
    host, d, (end8, scale, wd) = _refusal_state(16)
    lr, b1, b2, eps, _ = R.HYPER[0]
    with pytest.raises(RuntimeError):
        hip.adamw_step_groups_master(d["p"], None, d["g"], d["m"], d["v"], end8, scale, wd, lr, b1, b2, eps, 2)
    torch.cuda.synchronize()
    assert _untouched(host, d)


# ------------------------------------------------------------------------------------------------------------------ c
@pytest.mark.parametrize("name", list(M.HUNDRED))
def test_hundred_small_steps_accumulate_only_with_a_master(name):
    from one_peace_amd.optim import FusedAdamW
    M.assert_hundred(name, FusedAdamW, DEV)


# ------------------------------------------------------------------------------------------------------------------ d
def test_fused_adamw_with_master_follows_the_reference_fp16_optimizer(golden_dir):
    import os
    from one_peace_amd.optim import FusedAdamW
    fx = torch.load(os.path.join(golden_dir, "adamw_master.pt"), weights_only=False)
    assert M.run_fixture(fx, FusedAdamW, DEV) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ e
def test_the_default_fused_adamw_keeps_no_master_and_calls_the_old_entry(monkeypatch):
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.optim import FusedAdamW
    hip = hipmod()
    calls = {"old": 0, "master": 0}
    old, new = hip.adamw_step_groups, hip.adamw_step_groups_master

    def count(key, fn):
        def wrapper(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return wrapper

    monkeypatch.setattr(hip, "adamw_step_groups", count("old", old))
    monkeypatch.setattr(hip, "adamw_step_groups_master", count("master", new))
    for master_weights, want in ((False, {"old": 1, "master": 0}), (True, {"old": 1, "master": 1})):
        model = M.EightParams(1.0).to(DEV).to(torch.bfloat16)
        flat = FlatParameters(model)
        opt = FusedAdamW(flat, lr=1e-2, master_weights=master_weights) if master_weights else FusedAdamW(flat, lr=1e-2)
        assert (opt.master is not None) == master_weights
        model.w.grad.fill_(0.01)
        opt.step()
        torch.cuda.synchronize()
        assert calls == want, (master_weights, calls)
        assert bool((flat.params.cpu().float() < 1.0).all())
    with pytest.raises(RuntimeError):
        FusedAdamW(FlatParameters(M.EightParams(1.0).to(DEV).to(torch.bfloat16))).sync_master()


def test_sync_master_on_the_device():
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.optim import FusedAdamW
    model = M.EightParams(1.0).to(DEV).to(torch.bfloat16)
    flat = FlatParameters(model)
    opt = FusedAdamW(flat, lr=1e-5, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.0, master_weights=True)
    with torch.no_grad():
        flat.params.copy_(torch.arange(2, 10).to(torch.bfloat16))
    opt.sync_master()
    model.w.grad.fill_(0.01)
    opt.step()
    torch.cuda.synchronize()
    exp = R.Expected(torch.arange(2, 10).float(), torch.full((8,), 0.01).to(torch.bfloat16), torch.zeros(8), torch.zeros(8), 1,
                     1e-5, 0.9, 0.98, 1e-6)
    M.assert_step(exp, opt.master, flat.params, opt.exp_avg, opt.exp_avg_sq, "after sync_master")


# ------------------------------------------------------------------------------------------------------------------ f
_BIG = {}
POS = R.STRIDE + 8 * 12345 + 3  # in the second grid stride
LR, B1, B2, EPS, WD0 = 5e-4, 0.9, 0.98, 1e-6, 0.05


def _big_opt(step):
    """FusedAdamW(master_weights=True) over TwoStrides with a master that is not bf16-exact and, for step > 1, Adam-like moments."""
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.optim import FusedAdamW
    n = R.SIZES[3]
    if not _BIG:
        _BIG["model"] = R.TwoStrides().to(torch.bfloat16)
        _BIG["state"] = M.make_master_state(n, 1000, 1e-2, 1.0, seed=8)
    flat = FlatParameters(copy.deepcopy(_BIG["model"]).to(DEV))
    assert flat.numel == n
    master, p, g, m, v = _BIG["state"]
    opt = FusedAdamW(flat, lr=LR, betas=(B1, B2), eps=EPS, weight_decay=WD0, master_weights=True)
    with torch.no_grad():
        flat.params.copy_(p)
    opt.sync_master()
    opt.master.copy_(master)
    flat.grads.copy_(g)
    if step > 1:
        opt.exp_avg.copy_(m)
        opt.exp_avg_sq.copy_(v)
    opt.step_count = step - 1
    counts = [(e - s) // 8 for s, e, _, _ in flat.groups]
    scale = R.expand_groups(counts, [gr[2] for gr in flat.groups])
    wd = R.expand_groups(counts, [WD0 if gr[3] else 0.0 for gr in flat.groups])
    return flat, opt, scale, wd


def _host(flat, opt):
    return tuple(t.detach().cpu().clone() for t in (opt.master, flat.grads, opt.exp_avg, opt.exp_avg_sq))


def test_a_nan_gradient_poisons_master_and_parameters_of_the_whole_clipped_step():
    flat, opt, _, _ = _big_opt(1000)
    flat.grads[POS] = float("nan")
    norm = opt.step(grad_scale=0.25, clip_norm=R.CLIP_NORM)
    torch.cuda.synchronize()
    assert math.isnan(float(norm))
    left = [int(torch.isfinite(t).sum()) for t in (opt.master, flat.params, opt.exp_avg, opt.exp_avg_sq)]
    assert left == [0, 0, 0, 0], "finite master, p, m, v elements after a step whose gradient norm is NaN: %s" % left


def test_an_inf_gradient_zeroes_the_clipped_step_and_poisons_only_itself():
    flat, opt, scale, wd = _big_opt(1000)
    flat.grads[POS] = float("inf")
    master, g, m, v = _host(flat, opt)
    norm = opt.step(grad_scale=0.25, clip_norm=R.CLIP_NORM)
    torch.cuda.synchronize()
    assert float(norm) == math.inf
    check = torch.ones(flat.numel, dtype=torch.bool)
    check[POS] = False
    exp = R.Expected(master, g, m, v, 1000, LR, B1, B2, EPS, grad_scale=0.25, clip_norm=R.CLIP_NORM, sqnorm=(norm / 0.25) ** 2,
                     lr_scale=scale, weight_decay=wd, check=check)
    assert bool((exp.m[check] == R.f32(B1) * m.double()[check]).all()), "the reference's g' is not 0 where g is finite"
    M.assert_step(exp, opt.master, flat.params, opt.exp_avg, opt.exp_avg_sq, "inf")
    for t in (opt.master, flat.params, opt.exp_avg, opt.exp_avg_sq):
        assert math.isnan(float(t[POS])), "inf * 0 is NaN"


def test_a_nan_gradient_without_clipping_stays_in_its_element():
    flat, opt, scale, wd = _big_opt(1)
    pos = flat.numel - 1
    flat.grads[pos] = float("nan")
    master, g, m, v = _host(flat, opt)
    assert opt.step(grad_scale=0.25, clip_norm=0.0) is None
    torch.cuda.synchronize()
    check = torch.ones(flat.numel, dtype=torch.bool)
    check[pos] = False
    exp = R.Expected(master, g, m, v, 1, LR, B1, B2, EPS, grad_scale=0.25, lr_scale=scale, weight_decay=wd, check=check)
    M.assert_step(exp, opt.master, flat.params, opt.exp_avg, opt.exp_avg_sq, "nan without clipping")
    for t in (opt.master, flat.params, opt.exp_avg, opt.exp_avg_sq):
        assert not math.isfinite(float(t[pos]))
