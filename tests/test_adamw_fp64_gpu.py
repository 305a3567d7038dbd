"""The optimiser kernels (csrc/elementwise.hip: adamw_kernel without and with GROUPS, sqnorm_partial_kernel, sqnorm_final_kernel) against
the fp64 statement of tests/adamw_ref.py, one step at a time from a given state, under the criteria derived there: the stored bf16
parameter inside [bf16(ref - delta), bf16(ref + delta)] for EVERY element, the moments within 4 fp32 roundings of the magnitudes
they sum, the sum of squares within its summation bound and bit-reproducible.  Every case first asserts, on the reference alone,
that fewer than 1e-3 of its intervals hold two bf16 values.

  a  op_adamw_step: sizes up to two grid strides plus a ragged third, three hyperparameter sets, steps 1 ... 10^6, gradients 1e-20 ... 30
  b  clipping and grad_scale: the norm well below, within 1e-3 of, and well above the threshold; the device's own sum of squares
     goes into the reference, so an ulp in the norm cannot flip the clamp there; slices sharing one global norm; norm edge cases
  c  op_adamw_step_groups: awkward, full (256) and single group tables; 257 groups rejected with the buffers untouched
  d  FusedAdamW over FlatParameters, five steps, every step against the state copied before it
  e  non-finite gradients: a NaN poisons the whole step when clipping is on (as optim.TorchAdamW), an inf only itself

Each case appends one line to adamw_fp64_report.txt in the tests' output directory (tests/util.py: out_dir()): the case, the
largest share of the p / m / v budgets used (p: the multiple of delta the reference must move by to round to what was stored),
the two-valued share, and the norm's error over its bound."""
import copy
import math
import os

import pytest
import torch

from tests import adamw_ref as R
from tests.util import out_dir

pytestmark = pytest.mark.gpu
DEV = "cuda"


def hipmod():
    from one_peace_amd import hip
    return hip


def report(case, f=None, norm=None, note=""):
    f = f or {}
    fmt = lambda k: "%.3f" % f[k] if k in f else "-"  # noqa: E731
    line = "%s  p %s  m %s  v %s  two_valued %s  norm %s%s" % (
        case, fmt("p_used"), fmt("m_used"), fmt("v_used"), "%.2e" % f["two_valued"] if f else "-",
        "%.3f" % norm if norm is not None else "-", "  " + note if note else "")
    with open(os.path.join(out_dir(), "adamw_fp64_report.txt"), "a") as fh:
        fh.write(line + "\n")
    print(line)


def to_dev(p, g, m, v):
    return p.to(DEV), g.to(DEV), m.to(DEV), v.to(DEV)


def checked_sqnorm(hip, gd, g):
    """hip.sqnorm twice (same bits) and against the fp64 sum; returns the device scalar and error / bound."""
    sq = hip.sqnorm(gd).clone()
    again = hip.sqnorm(gd)
    assert torch.equal(sq.view(torch.int32), again.view(torch.int32)), "the sum of squares is not reproducible"
    used = R.norm_used(sq, g)
    return sq, used


# ------------------------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("case", R.STEP_CASES, ids=R.step_case_id)
def test_adamw_step_against_fp64(case):
    hip = hipmod()
    n, hp, step, gscale, pscale = case
    lr, b1, b2, eps, wd = R.HYPER[hp]
    p, g, m, v = R.make_state(n, step, gscale, pscale)
    exp = R.Expected(p, g, m, v, step, lr, b1, b2, eps, weight_decay=wd)
    exp.assert_vacuity(R.step_case_id(case))
    pd, gd, md, vd = to_dev(p, g, m, v)
    hip.adamw_step(pd, gd, md, vd, lr, b1, b2, eps, wd, step)
    torch.cuda.synchronize()
    f = exp.figures(pd, md, vd)
    report("a/" + R.step_case_id(case), f)
    assert torch.equal(gd.cpu().view(torch.int16), g.view(torch.int16)), "the gradient buffer was written"
    exp.assert_step(pd, md, vd, R.step_case_id(case))


# ------------------------------------------------------------------------------------------------------------------ b
@pytest.mark.parametrize("case", R.CLIP_CASES, ids=R.clip_case_id)
def test_adamw_step_clipped_and_scaled_against_fp64(case):
    hip = hipmod()
    n, gs, at, step = case
    lr, b1, b2, eps, wd = R.HYPER[0]
    p, g, m, v = R.make_clip_state(n, gs, at, step)
    R.assert_clip_landing(g, gs, at)
    pd, gd, md, vd = to_dev(p, g, m, v)
    sq, used = checked_sqnorm(hip, gd, g)
    exp = R.Expected(p, g, m, v, step, lr, b1, b2, eps, grad_scale=gs, clip_norm=R.CLIP_NORM, sqnorm=sq, weight_decay=wd)
    exp.assert_vacuity(R.clip_case_id(case))
    hip.adamw_step(pd, gd, md, vd, lr, b1, b2, eps, wd, step, gs, sq, R.CLIP_NORM)
    torch.cuda.synchronize()
    report("b/" + R.clip_case_id(case), exp.figures(pd, md, vd), used)
    assert used <= 1.0, "sum of squares off by %.2f of its bound" % used
    exp.assert_step(pd, md, vd, R.clip_case_id(case))


@pytest.mark.parametrize("at", list(R.CLIP_AT))
def test_adamw_step_on_slices_sharing_one_global_norm(at):
    """trainer.py:917-935: grads * 1/world, clip_grad_norm(3.0) over ALL parameters (two ranges here), one launch per range."""
    hip = hipmod()
    n, cut, gs, step = 8192, 4096 + 8 * 11, 0.25, 1000
    lr, b1, b2, eps, wd = R.HYPER[0]
    p, g, m, v = R.make_clip_state(n, gs, at, step, seed=1)
    R.assert_clip_landing(g, gs, at)
    pd, gd, md, vd = to_dev(p, g, m, v)
    sq, used = checked_sqnorm(hip, gd, g)
    exp = R.Expected(p, g, m, v, step, lr, b1, b2, eps, grad_scale=gs, clip_norm=R.CLIP_NORM, sqnorm=sq, weight_decay=wd)
    for s_, e_ in ((0, cut), (cut, n)):
        hip.adamw_step(pd[s_:e_], gd[s_:e_], md[s_:e_], vd[s_:e_], lr, b1, b2, eps, wd, step, gs, sq, R.CLIP_NORM)
    torch.cuda.synchronize()
    report("b/slices-%s" % at, exp.figures(pd, md, vd), used)
    assert used <= 1.0
    exp.assert_step(pd, md, vd, "slices " + at)


def test_sqnorm_of_a_buffer_whose_only_nonzero_vector_is_the_last():
    hip = hipmod()
    n = R.NORM_STRIDE + 8
    g = torch.zeros(n, dtype=torch.bfloat16)
    g[-8:] = torch.tensor([1.5, -2.0, 0.375, 3.0, -0.0625, 7.0, 1.0, -5.0], dtype=torch.bfloat16)
    sq, used = checked_sqnorm(hip, g.to(DEV), g)
    report("b/norm-last-vector", norm=used)
    assert used <= 1.0, "got %r, fp64 %r" % (float(sq), float(R.sqnorm_fp64(g)))


def test_sqnorm_of_squares_that_are_subnormal():
    """2^-70 everywhere: the squares, 2^-140, are subnormal in fp32 and their sum is exact if they are kept.  Either the fp64 value
    within the bound or exactly 0 (squares flushed) is accepted; the report says which the device does."""
    hip = hipmod()
    n = R.NORM_STRIDE + 8
    g = torch.full((n,), 2.0 ** -70, dtype=torch.bfloat16)
    sq, used = checked_sqnorm(hip, g.to(DEV), g)
    flushed = float(sq) == 0.0
    report("b/norm-subnormal-squares", norm=used, note="squares flushed to zero" if flushed else "gradual underflow kept")
    assert flushed or used <= 1.0, "got %r, fp64 %r" % (float(sq), float(R.sqnorm_fp64(g)))


# ------------------------------------------------------------------------------------------------------------------ c
GROUP_CASES = [("awkward", R.AWKWARD_GROUPS, t, clip) for t in (1, 1000) for clip in (False, True)] + [
    ("full", R.FULL_GROUPS, t, clip) for t in (1, 1000) for clip in (False, True)] + [
    ("single%d" % n, (n // 8,), t, clip) for n, t, clip in zip(R.SIZES, (1, 1000, 1, 1000), (False, True, True, False))]


@pytest.mark.parametrize("name,counts,step,clip", GROUP_CASES, ids=lambda x: None if isinstance(x, tuple) else str(x))
def test_adamw_step_groups_against_fp64(name, counts, step, clip):
    hip = hipmod()
    what = "%s-t%d-%s" % (name, step, "clip" if clip else "noclip")
    n = 8 * sum(counts)
    lr, b1, b2, eps, _ = R.HYPER[0]
    gs, clip_norm = (0.25, R.CLIP_NORM) if clip else (1.0, 0.0)
    p, g, m, v = R.make_state(n, step, 1e-2, 1.0, seed=2)
    end8, scale, wd = R.device_group_tables(counts)
    pd, gd, md, vd = to_dev(p, g, m, v)
    sq = used = None
    if clip:
        sq, used = checked_sqnorm(hip, gd, g)
    exp = R.Expected(p, g, m, v, step, lr, b1, b2, eps, grad_scale=gs, clip_norm=clip_norm, sqnorm=sq,
                     lr_scale=R.expand_groups(counts, scale.cpu()), weight_decay=R.expand_groups(counts, wd.cpu()))
    exp.assert_vacuity(what)
    hip.adamw_step_groups(pd, gd, md, vd, end8, scale, wd, lr, b1, b2, eps, step, gs, sq, clip_norm)
    torch.cuda.synchronize()
    report("c/" + what, exp.figures(pd, md, vd), used)
    assert used is None or used <= 1.0
    assert torch.equal(gd.cpu().view(torch.int16), g.view(torch.int16)), "the gradient buffer was written"
    exp.assert_step(pd, md, vd, what)


def test_adamw_step_groups_rejects_257_groups():
    hip = hipmod()
    counts = (1,) * 257
    n = 8 * len(counts)
    p, g, m, v = R.make_state(n, 2, 1e-2, 1.0, seed=3)
    end8, scale, wd = R.device_group_tables(counts)
    pd, gd, md, vd = to_dev(p, g, m, v)
    lr, b1, b2, eps, _ = R.HYPER[0]
    with pytest.raises(RuntimeError):
        hip.adamw_step_groups(pd, gd, md, vd, end8, scale, wd, lr, b1, b2, eps, 2)
    torch.cuda.synchronize()
    assert torch.equal(pd.cpu().view(torch.int16), p.view(torch.int16)) and torch.equal(gd.cpu().view(torch.int16), g.view(torch.int16))
    assert torch.equal(md.cpu(), m) and torch.equal(vd.cpu(), v)
    hip.adamw_step_groups(pd[:2048], gd[:2048], md[:2048], vd[:2048], end8[:256], scale[:256], wd[:256], lr, b1, b2, eps, 2)  # 256 are taken
    torch.cuda.synchronize()
    assert not torch.equal(pd[:2048].cpu().view(torch.int16), p[:2048].view(torch.int16))


# ------------------------------------------------------------------------------------------------------------------ d
class Small(torch.nn.Module):
    def __init__(self, seed=0):
        super().__init__()
        gen = torch.Generator().manual_seed(seed)
        mk = lambda *s: torch.nn.Parameter(torch.randn(*s, generator=gen))  # noqa: E731
        self.scalar, self.seven, self.nine, self.vec = mk(1), mk(7), mk(9), mk(1536)
        self.small, self.mat = mk(3, 5), mk(257, 64)


def _small_flat(seed=0):
    from one_peace_amd.distributed import FlatParameters
    scales = {"scalar": 1.0, "seven": 0.65, "nine": 0.65, "vec": 0.4225, "small": 0.4225, "mat": 1.0}
    model = Small(seed).to(DEV).to(torch.bfloat16)
    flat = FlatParameters(model, no_decay=lambda name, p: p.dim() <= 1 or name == "small", lr_scale=lambda name, p: scales[name])
    return model, flat


def _flat_tables(flat, weight_decay):
    """FlatParameters.groups expanded to one lr scale / weight decay per element, and the mask of the alignment padding."""
    counts = [(e - s) // 8 for s, e, _, _ in flat.groups]
    scale = R.expand_groups(counts, [g[2] for g in flat.groups])
    wd = R.expand_groups(counts, [weight_decay if g[3] else 0.0 for g in flat.groups])
    pad = torch.ones(flat.numel, dtype=torch.bool)
    for _, _, off, k in flat.entries:
        pad[off:off + k] = False
    return scale, wd, pad


@pytest.mark.parametrize("clip_norm", [0.0, 1.0])
def test_fused_adamw_five_steps_against_fp64(clip_norm):
    from one_peace_amd.optim import FusedAdamW
    model, flat = _small_flat()
    assert len({g[2] for g in flat.groups}) >= 3 and {g[3] for g in flat.groups} == {True, False}
    b1, b2, eps, wd0, gs = 0.9, 0.98, 1e-6, 0.05, 0.25
    opt = FusedAdamW(flat, lr=1e-3, betas=(b1, b2), eps=eps, weight_decay=wd0)
    scale, wd, pad = _flat_tables(flat, wd0)
    assert int(pad.sum()) > 0
    gen = torch.Generator().manual_seed(5)
    for step in range(1, 6):
        lr = 1e-3 * (0.5 + 0.37 * step)
        opt.set_lr(lr)
        for _, prm, _, _ in flat.entries:  # fresh gradients through the views, as backward writes them: the padding stays zero
            prm.grad.copy_(torch.randn(prm.shape, generator=gen) * 0.012 * step)
        p, g, m, v = (t.detach().cpu().clone() for t in (flat.params, flat.grads, opt.exp_avg, opt.exp_avg_sq))
        sq = hipmod().sqnorm(flat.grads) if clip_norm > 0 else None  # the bits the step derives its coefficient from
        norm = opt.step(grad_scale=gs, clip_norm=clip_norm)
        torch.cuda.synchronize()
        assert opt.step_count == step
        used = None
        if clip_norm > 0:
            want = gs * math.sqrt(float(R.sqnorm_fp64(g)))
            used = abs(float(norm) - want) / (R.norm_bound(g.numel()) * want)  # the norm carries half the relative error of its square
            assert used <= 1.0, "returned norm %r, fp64 %r" % (float(norm), want)
            assert (want > clip_norm) == (step >= 3), "steps 1-2 are meant to stay below the threshold, 3-5 above (%g)" % want
        else:
            assert norm is None
        exp = R.Expected(p, g, m, v, step, lr, b1, b2, eps, grad_scale=gs, clip_norm=clip_norm,
                         sqnorm=sq, lr_scale=scale, weight_decay=wd)
        f = exp.assert_step(flat.params, opt.exp_avg, opt.exp_avg_sq, "step %d" % step)
        report("d/clip%g-step%d" % (clip_norm, step), f, used)
        for buf in (flat.params, opt.exp_avg, opt.exp_avg_sq):
            assert not bool(buf.cpu()[pad].any()), "alignment padding was written"
        for _, prm, off, k in flat.entries:
            assert prm.data_ptr() == flat.params[off:off + k].data_ptr() and prm.grad.data_ptr() == flat.grads[off:off + k].data_ptr()


# ------------------------------------------------------------------------------------------------------------------ e
_BIG = {}


def _big():
    """One module, its gradients and its fp64-ready CPU copies for all cases of (e); the cases work on copies."""
    if not _BIG:
        model = R.TwoStrides().to(torch.bfloat16)
        g = (torch.randn(R.SIZES[3], generator=torch.Generator().manual_seed(8)) * 1e-2).to(torch.bfloat16)
        _BIG.update(model=model, g=g)
    return _BIG["model"], _BIG["g"]


def _big_flat():
    from one_peace_amd.distributed import FlatParameters
    model, g = _big()
    flat = FlatParameters(copy.deepcopy(model).to(DEV))
    assert flat.numel == R.SIZES[3] == g.numel()
    return flat, g


POSITIONS = {"first": 0, "last": R.SIZES[3] - 1, "second_stride": R.STRIDE + 8 * 12345 + 3}


@pytest.mark.parametrize("where", list(POSITIONS))
def test_a_nan_gradient_poisons_the_whole_clipped_step(where):
    from one_peace_amd.optim import FusedAdamW, TorchAdamW
    hip = hipmod()
    results = {}
    for cls in (FusedAdamW, TorchAdamW):
        flat, g = _big_flat()
        opt = cls(flat, lr=1e-2, betas=(0.9, 0.98), eps=1e-6, weight_decay=0.05)
        flat.grads.copy_(g)
        flat.grads[POSITIONS[where]] = float("nan")
        if cls is FusedAdamW:
            assert math.isnan(float(hip.sqnorm(flat.grads)))
        norm = opt.step(grad_scale=0.25, clip_norm=R.CLIP_NORM)
        torch.cuda.synchronize()
        assert math.isnan(float(norm)), "%s returned the norm %r" % (cls.__name__, float(norm))
        results[cls.__name__] = [int(torch.isfinite(t).sum()) for t in (flat.params, opt.exp_avg, opt.exp_avg_sq)]
        del opt, flat
    report("e/nan-%s" % where, note="finite p, m, v left: fused %s torch %s" % (results["FusedAdamW"], results["TorchAdamW"]))
    assert results["TorchAdamW"] == [0, 0, 0], results
    assert results["FusedAdamW"] == [0, 0, 0], "finite p, m, v elements after a step whose gradient norm is NaN: %s" % results


@pytest.mark.parametrize("n", [2040, R.SIZES[3]])
def test_a_nan_gradient_poisons_the_whole_clipped_single_range_step(n):
    hip = hipmod()
    lr, b1, b2, eps, wd = R.HYPER[0]
    p, g, m, v = R.make_state(n, 1000, 1e-2, 1.0, seed=4)
    g[n - 8 * 3 - 2] = float("nan")
    pd, gd, md, vd = to_dev(p, g, m, v)
    sq = hip.sqnorm(gd)
    assert math.isnan(float(sq))
    hip.adamw_step(pd, gd, md, vd, lr, b1, b2, eps, wd, 1000, 0.25, sq, R.CLIP_NORM)
    torch.cuda.synchronize()
    left = [int(torch.isfinite(t).sum()) for t in (pd, md, vd)]
    assert left == [0, 0, 0], "finite p, m, v elements after a step whose gradient norm is NaN: %s" % left


def test_an_inf_gradient_zeroes_the_clipped_step_and_poisons_only_itself():
    from one_peace_amd.optim import FusedAdamW
    flat, g = _big_flat()
    lr, b1, b2, eps, wd0 = 1e-2, 0.9, 0.98, 1e-6, 0.05
    opt = FusedAdamW(flat, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd0)
    gen = torch.Generator().manual_seed(9)
    opt.exp_avg.copy_(torch.randn(flat.numel, generator=gen) * 1e-2)
    opt.exp_avg_sq.copy_(opt.exp_avg.cpu() ** 2 + torch.rand(flat.numel, generator=gen) * 1e-4)
    opt.step_count = 999
    pos = POSITIONS["second_stride"]
    flat.grads.copy_(g)
    flat.grads[pos] = float("inf")
    p, gg, m, v = (t.detach().cpu().clone() for t in (flat.params, flat.grads, opt.exp_avg, opt.exp_avg_sq))
    norm = opt.step(grad_scale=0.25, clip_norm=R.CLIP_NORM)
    torch.cuda.synchronize()
    assert float(norm) == math.inf
    scale, wd, _ = _flat_tables(flat, wd0)
    check = torch.ones(flat.numel, dtype=torch.bool)
    check[pos] = False
    exp = R.Expected(p, gg, m, v, 1000, lr, b1, b2, eps, grad_scale=0.25, clip_norm=R.CLIP_NORM, sqnorm=(norm / 0.25) ** 2,
                     lr_scale=scale, weight_decay=wd, check=check)
    assert bool((exp.m[check] == R.f32(b1) * m.double()[check]).all()), "the reference's g' is not 0 where g is finite"
    f = exp.assert_step(flat.params, opt.exp_avg, opt.exp_avg_sq, "inf")
    report("e/inf", f)
    for t in (flat.params, opt.exp_avg, opt.exp_avg_sq):
        assert math.isnan(float(t[pos])), "inf * 0 is NaN"


def test_a_nan_gradient_without_clipping_stays_in_its_element():
    from one_peace_amd.optim import FusedAdamW
    flat, g = _big_flat()
    lr, b1, b2, eps, wd0 = 1e-2, 0.9, 0.98, 1e-6, 0.05
    opt = FusedAdamW(flat, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd0)
    pos = POSITIONS["last"]
    flat.grads.copy_(g)
    flat.grads[pos] = float("nan")
    p, gg, m, v = (t.detach().cpu().clone() for t in (flat.params, flat.grads, opt.exp_avg, opt.exp_avg_sq))
    assert opt.step(grad_scale=0.25, clip_norm=0.0) is None
    torch.cuda.synchronize()
    scale, wd, _ = _flat_tables(flat, wd0)
    check = torch.ones(flat.numel, dtype=torch.bool)
    check[pos] = False
    exp = R.Expected(p, gg, m, v, 1, lr, b1, b2, eps, grad_scale=0.25, lr_scale=scale, weight_decay=wd, check=check)
    f = exp.assert_step(flat.params, opt.exp_avg, opt.exp_avg_sq, "nan without clipping")
    report("e/nan-noclip", f)
    for t in (flat.params, opt.exp_avg, opt.exp_avg_sq):
        assert not math.isfinite(float(t[pos]))
