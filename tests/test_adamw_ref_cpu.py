"""Tests of the instrument behind tests/test_adamw_fp64_gpu.py (tests/adamw_ref.py); no GPU needed.

* adamw_fp64 against the oracle's adamw_step / clip_coef on random bf16 states, and against optim.TorchAdamW.step over a small
  FlatParameters on the CPU, to fp32 accuracy.
* bf16_rne against torch's own fp32 -> bf16 rounding, and on ties, powers of two and the subnormal range.
* an fp32 emulation of the kernels' operation order inside the interval and moment criteria at every case of the GPU matrix, with
  the anti-vacuity cap met on the reference alone.
* the same emulation OUTSIDE the interval criterion under each planted error: decay applied after the update, eps inside the
  square root, the bias correction of step t - 1, the clip coefficient left out.  A planted error that passed would mean the
  criterion cannot see that class of bug."""
import math

import pytest
import torch

from oracle import onepeace_oracle as O
from tests import adamw_ref as R

F32_EPS = 2.0 ** -23


def test_bf16_rne_rounds_once_to_nearest_even():
    x = torch.randn(100000, generator=torch.Generator().manual_seed(1)) * 3.0
    assert torch.equal(R.bf16_rne(x.double()), x.to(torch.bfloat16).double())
    one, q = 1.0, 2.0 ** -7                                    # bf16 spacing in [1, 2) is 2^-7, just below 1 it is 2^-8
    x = torch.tensor([one + q / 2, one + 3 * q / 2, one + q / 2 + 2.0 ** -40, one - q / 4, one - q / 4 - 2.0 ** -40,
                      2.0 - q / 2, 0.0, -(one + q / 2), 2.0 ** -133 * 1.5, 2.0 ** -134, 2.0 ** -126 - 2.0 ** -134], dtype=torch.float64)
    want = torch.tensor([one, one + 2 * q, one + q, one, one - q / 2, 2.0, 0.0, -one, 2.0 ** -132, 0.0, 2.0 ** -126],
                        dtype=torch.float64)
    assert torch.equal(R.bf16_rne(x), want)
    # a cast through fp32 rounds twice: 1 + q/2 + 2^-40 first falls onto the tie 1 + q/2, then to even (1); one rounding gives 1 + q
    assert float(x[2].float().to(torch.bfloat16)) == one and float(R.bf16_rne(x[2:3])) == one + q


@pytest.mark.parametrize("step,clip", [(1, 0.0), (3, 0.0), (1000, 3.0), (7, 0.05)])
def test_adamw_fp64_agrees_with_the_oracle(step, clip):
    n = 4096
    lr, b1, b2, eps, wd = R.HYPER[0]
    p, g, m, v = R.make_state(n, step, 1e-2, 1.0, seed=step)
    gs = 0.25
    total, coef = O.clip_coef([g.float() * gs], clip)
    if clip > 0:
        want = float(R.clip_coef_fp64(gs, clip, R.sqnorm_fp64(g)))
        assert (want < 1.0) == (clip < 1.0) and abs(float(coef) - want) <= 8 * F32_EPS * want
    pr, mr, vr = p.clone(), m.clone(), v.clone()
    O.adamw_step(pr, g.float() * gs * coef, mr, vr, step, lr=lr, beta1=b1, beta2=b2, eps=eps, weight_decay=wd)
    p64, m64, v64, u = R.adamw_fp64(p, g, m, v, step, lr, b1, b2, eps, grad_scale=gs, clip_norm=clip, weight_decay=wd)
    assert float((mr.double() - m64).abs().max()) <= 16 * F32_EPS * float(m64.abs().max())
    assert float((vr.double() - v64).abs().max()) <= 16 * F32_EPS * float(v64.abs().max())
    # the oracle stores bf16: half a bf16 ulp (at most 2^-8 relative) plus its fp32 roundings
    assert bool(((pr.double() - p64).abs() <= 2.0 ** -8 * p64.abs() + 16 * F32_EPS * (p.double().abs() + u.abs())).all())


class _Small(torch.nn.Module):
    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(3)
        self.a = torch.nn.Parameter(torch.randn(7, generator=gen))
        self.b = torch.nn.Parameter(torch.randn(33, 5, generator=gen))
        self.c = torch.nn.Parameter(torch.randn(64, generator=gen))
        self.d = torch.nn.Parameter(torch.randn(9, 16, generator=gen))


@pytest.mark.parametrize("clip", [0.0, 0.25])
def test_adamw_fp64_agrees_with_torch_adamw_over_flat_parameters(clip):
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.optim import TorchAdamW
    scales = {"a": 1.0, "b": 0.65, "c": 0.65, "d": 0.4225}
    flat = FlatParameters(_Small(), lr_scale=lambda name, p: scales[name])   # fp32 parameters: no storage rounding in the way
    b1, b2, eps, wd0, gs = 0.9, 0.98, 1e-6, 0.05, 0.25
    opt = TorchAdamW(flat, lr=1e-3, betas=(b1, b2), eps=eps, weight_decay=wd0)
    counts = [(e - s) // 8 for s, e, _, _ in flat.groups]
    scale = R.expand_groups(counts, [g[2] for g in flat.groups])
    wd = R.expand_groups(counts, [wd0 if g[3] else 0.0 for g in flat.groups])
    gen = torch.Generator().manual_seed(4)
    for step in (1, 2, 3):
        lr = 1e-3 * step
        opt.set_lr(lr)
        for _, prm, _, _ in flat.entries:
            prm.grad.copy_(torch.randn(prm.shape, generator=gen) * 0.1)
        p, g, m, v = (t.detach().clone() for t in (flat.params, flat.grads, opt.exp_avg, opt.exp_avg_sq))
        norm = opt.step(grad_scale=gs, clip_norm=clip)
        p64, m64, v64, u = R.adamw_fp64(p, g, m, v, step, lr, b1, b2, eps, grad_scale=gs, clip_norm=clip, lr_scale=scale,
                                        weight_decay=wd)
        if clip > 0:
            want = gs * math.sqrt(float(R.sqnorm_fp64(g)))
            assert want > clip and abs(float(norm) - want) <= 8 * F32_EPS * want
        # the group scales and the decay go through fp32 on one side only: layer-decay scales such as 0.65 are not fp32 numbers
        tol = 32 * F32_EPS
        assert bool(((flat.params.double() - p64).abs() <= tol * (p.double().abs() + u.abs())).all())
        assert bool(((opt.exp_avg.double() - m64).abs() <= tol * (m.double().abs() + (gs * g.double()).abs())).all())
        assert bool(((opt.exp_avg_sq.double() - v64).abs() <= tol * (v.double() + (gs * g.double()) ** 2)).all())


def _emulated(p, g, m, v, step, lr, b1, b2, eps, planted=None, groups=False, **kw):
    if groups:  # the arithmetic of adamw_kernel<GROUPS = true>: lr * lr_scale and the decay multiplier formed per group in fp32
        n = p.numel()
        kw = dict(kw, lr_scale=torch.ones(n) if "lr_scale" not in kw else kw["lr_scale"],
                  weight_decay=torch.as_tensor(kw.get("weight_decay", 0.0), dtype=torch.float32).expand(n))
    return R.emulate_fp32(p, g, m, v, step, lr, b1, b2, eps, planted=planted, **kw)


@pytest.mark.parametrize("case", R.STEP_CASES, ids=R.step_case_id)
def test_emulated_kernel_order_meets_the_criteria_on_the_step_matrix(case):
    n, hp, step, gscale, pscale = case
    lr, b1, b2, eps, wd = R.HYPER[hp]
    p, g, m, v = R.make_state(n, step, gscale, pscale)
    exp = R.Expected(p, g, m, v, step, lr, b1, b2, eps, weight_decay=wd)
    exp.assert_step(*_emulated(p, g, m, v, step, lr, b1, b2, eps, weight_decay=wd), what="single range")
    exp.assert_step(*_emulated(p, g, m, v, step, lr, b1, b2, eps, weight_decay=wd, groups=True), what="groups")


@pytest.mark.parametrize("case", R.CLIP_CASES, ids=R.clip_case_id)
def test_emulated_kernel_order_meets_the_criteria_on_the_clip_matrix(case):
    n, gs, at, step = case
    lr, b1, b2, eps, wd = R.HYPER[0]
    p, g, m, v = R.make_clip_state(n, gs, at, step)
    R.assert_clip_landing(g, gs, at)
    sq = torch.tensor(float(R.sqnorm_fp64(g)), dtype=torch.float32)   # stands in for the device's fp32 sum
    kw = dict(grad_scale=gs, clip_norm=R.CLIP_NORM, sqnorm=sq, weight_decay=wd)
    exp = R.Expected(p, g, m, v, step, lr, b1, b2, eps, **kw)
    exp.assert_step(*_emulated(p, g, m, v, step, lr, b1, b2, eps, **kw), what=R.clip_case_id(case))


@pytest.mark.parametrize("name,counts", [("awkward", R.AWKWARD_GROUPS), ("full", R.FULL_GROUPS)])
def test_emulated_kernel_order_meets_the_criteria_on_the_group_tables(name, counts):
    assert len(R.FULL_GROUPS) == 256 and sum(R.FULL_GROUPS) > 524288 and max(R.AWKWARD_GROUPS) > 524288
    n, step = 8 * sum(counts), 1000
    lr, b1, b2, eps, _ = R.HYPER[0]
    scale, wd = R.group_tables(len(counts))
    assert all((scale[k], wd[k]) != (scale[k + 1], wd[k + 1]) and scale[k] != scale[k + 1] for k in range(len(counts) - 1))
    scale, wd = R.expand_groups(counts, scale), R.expand_groups(counts, wd)
    p, g, m, v = R.make_state(n, step, 1e-2, 1.0, seed=2)
    exp = R.Expected(p, g, m, v, step, lr, b1, b2, eps, lr_scale=scale, weight_decay=wd)
    got = R.emulate_fp32(p, g, m, v, step, lr, b1, b2, eps, lr_scale=scale, weight_decay=wd)
    exp.assert_step(*got, what=name)
    # a lookup that is off by one vector at the group boundaries is seen
    off = R.emulate_fp32(p, g, m, v, step, lr, b1, b2, eps, lr_scale=torch.roll(scale, 8), weight_decay=torch.roll(wd, 8))
    assert exp.figures(*off)["p_bad"] > 0


@pytest.mark.parametrize("planted", R.PLANTED)
def test_planted_error_fails_the_interval_criterion(planted):
    n, step, gs = 65536, 2, 0.25
    lr, b1, b2, eps, wd = R.HYPER[0]
    p, g, m, v = R.make_clip_state(n, gs, "above", step, seed=5)
    kw = dict(grad_scale=gs, clip_norm=R.CLIP_NORM, weight_decay=wd)
    exp = R.Expected(p, g, m, v, step, lr, b1, b2, eps, **kw)
    exp.assert_p(_emulated(p, g, m, v, step, lr, b1, b2, eps, **kw)[0], what="unplanted")
    assert exp.figures(*_emulated(p, g, m, v, step, lr, b1, b2, eps, planted=planted, **kw))["p_bad"] > 0, planted


def test_non_finite_norms_in_the_reference():
    g = torch.tensor([1.0, 2.0, float("nan")])
    assert math.isnan(float(R.clip_coef_fp64(0.25, 3.0, R.sqnorm_fp64(g))))
    assert float(R.clip_coef_fp64(0.25, 3.0, torch.tensor(math.inf))) == 0.0
    assert float(R.clip_coef_fp64(0.25, 0.0, torch.tensor(math.nan))) == 1.0
    gp = R.scaled_grad_fp64(torch.tensor([1.0, math.inf]), 0.25, 3.0)
    assert float(gp[0]) == 0.0 and math.isnan(float(gp[1]))
