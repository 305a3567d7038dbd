"""The fp32 weight average on the device (csrc/elementwise.hip: ema_step_kernel through hip.ema_step, adamw_kernel<true, MASTER, true>
through hip.adamw_step_groups_ema, ema.FlatEMA, optim.FusedAdamW(ema=)) under the criterion of tests/ema_ref.py.

  a  hip.ema_step against fp64 for every element: adamw_ref.SIZES x decay 0.9999 / 0.99 / 0; guards intact, p unwritten; decay 0 copies
  b  the fused entry without and with the master: p, master, m, v bit-identical to the unfused entries from the same inputs, the average
     bit-identical to hip.ema_step on that p and inside the fp64 criterion, g unwritten, guards intact, >= 0.9 of the bf16 parameters
     changed by the step (what makes a stale parameter visible), two runs bit-identical
  c  refused calls: a null average, 257 groups, the average aliasing the master, an average or master that does not cover the
     parameters -- nothing launched, nothing written
  d  tests/golden/ema.pt (the reference's EMAModule) through FusedAdamW(master_weights=True, ema=)
  e  which entries FusedAdamW calls, with and without ema
  f  FlatEMA.applied() on the device, with the cached transposed weights
  g  non-finite gradients"""
import math

import pytest
import torch

from tests import adamw_master_ref as M
from tests import adamw_ref as R
from tests import ema_ref as E
from tests.test_adamw_master_gpu import DEV, Guarded, hipmod

pytestmark = pytest.mark.gpu

# ------------------------------------------------------------------------------------------------------------------ a
@pytest.mark.parametrize("decay", [0.9999, 0.99, 0.0])
@pytest.mark.parametrize("n", R.SIZES)
def test_ema_step_against_fp64(n, decay):
    hip = hipmod()
    _, p, _, _, _, e, _, _ = E.case_state(n, 1000, False)
    keep, take = E.coefficients(decay)
    G = {"e": Guarded(e), "p": Guarded(p)}
    hip.ema_step(G["e"].t, G["p"].t, keep, take)
    torch.cuda.synchronize()
    assert G["e"].intact() and G["p"].intact(), "a guard region was written"
    assert torch.equal(M.bits16(G["p"].t), M.bits16(p)), "the parameters were written"
    E.assert_step(G["e"].t, e, p, keep, take, "ema_step n%d decay %g" % (n, decay))
    if decay == 0.0:
        assert torch.equal(G["e"].t.cpu(), p.float())
    else:
        assert not torch.equal(G["e"].t.cpu(), e)


# ------------------------------------------------------------------------------------------------------------------ b
CASES = [("awkward", R.AWKWARD_GROUPS, t, clip) for t in (1, 1000) for clip in (False, True)] + [
    ("full", R.FULL_GROUPS, t, clip) for t in (1, 1000) for clip in (False, True)] + [
    ("single%d" % n, (n // 8,), t, clip) for n in R.SIZES for t in (1, 1000) for clip in (False, True)]


@pytest.mark.parametrize("with_master", [False, True], ids=["plain", "master"])
@pytest.mark.parametrize("name,counts,step,clip", CASES, ids=lambda x: None if isinstance(x, tuple) else str(x))
def test_fused_step_matches_the_unfused_pair_bit_for_bit(name, counts, step, clip, with_master):
    hip = hipmod()
    what = "%s-t%d-%s-%s" % (name, step, "clip" if clip else "noclip", "master" if with_master else "plain")
    n = 8 * sum(counts)
    lr, b1, b2, eps, _ = R.HYPER[0]
    master, p, g, m, v, e, gs, clip_norm = E.case_state(n, step, clip)
    decay = 0.99 if step == 1 else 0.9999
    keep, take = E.coefficients(decay)
    end8, scale, wd = R.device_group_tables(counts)
    p_in = torch.full_like(p, float("nan")) if with_master else p  # with a master the parameter buffer is never read
    hyper = (end8, scale, wd, lr, b1, b2, eps, step)

    # the unfused pair from the same inputs
    u = {k: t.to(DEV) for k, t in dict(p=p_in, master=master, g=g, m=m, v=v, e=e).items()}
    sq = hip.sqnorm(u["g"]) if clip else None
    if with_master:
        hip.adamw_step_groups_master(u["p"], u["master"], u["g"], u["m"], u["v"], *hyper, gs, sq, clip_norm)
    else:
        hip.adamw_step_groups(u["p"], u["g"], u["m"], u["v"], *hyper, gs, sq, clip_norm)
    hip.ema_step(u["e"], u["p"], keep, take)

    runs = []
    for _ in range(2):
        G = {k: Guarded(t) for k, t in dict(p=p_in, master=master, g=g, m=m, v=v, e=e).items()}
        hip.adamw_step_groups_ema(G["p"].t, G["master"].t if with_master else None, G["g"].t, G["m"].t, G["v"].t, G["e"].t, *hyper,
                                  keep, take, gs, sq, clip_norm)
        torch.cuda.synchronize()
        for k, b in G.items():
            assert b.intact(), "%s: the guard regions of %s were written" % (what, k)
        runs.append({k: M.bits(b.t) for k, b in G.items()})
    got, again = runs
    new_p = G["p"].t.cpu()
    # (i) the optimiser's part is what the unfused entry stores
    for k in ("p", "m", "v") + (("master",) if with_master else ()):
        assert torch.equal(got[k], M.bits(u[k])), "%s: %s differs from the unfused entry" % (what, k)
    if not with_master:
        assert torch.equal(got["master"], M.bits(master)), "%s: the master buffer was written without a master" % what
    # (ii) the average is what ema_step makes of that p, and inside the criterion
    assert torch.equal(got["e"], M.bits(u["e"])), "%s: the average differs from hip.ema_step on the new parameters" % what
    E.assert_step(G["e"].t, e, new_p, keep, take, what)
    # (iii)
    assert torch.equal(got["g"], M.bits(g)), "%s: the gradient buffer was written" % what
    # (iv) a stale parameter would show: the step changed the bf16 value of (nearly) every element
    share = E.changed_share(new_p, p)
    assert share >= 0.9, "%s: only %.3f of the bf16 parameters changed in the step" % (what, share)
    # (v)
    for k in got:
        assert torch.equal(got[k], again[k]), "%s: two runs differ in %s" % (what, k)


# ------------------------------------------------------------------------------------------------------------------ c
def _refusal_state(n_groups):
    counts = (1,) * n_groups
    master, p, g, m, v, e = E.make_ema_state(8 * n_groups, 2, seed=3)
    host = dict(p=p, master=master, g=g, m=m, v=v, e=e)
    return host, {k: t.to(DEV) for k, t in host.items()}, R.device_group_tables(counts)


def _untouched(host, dev):
    return all(torch.equal(M.bits(dev[k]), M.bits(host[k])) for k in host)


def _fused(hip, d, tables, master, ema, sl=slice(None), groups=slice(None)):
    end8, scale, wd = (t[groups] for t in tables)
    lr, b1, b2, eps, _ = R.HYPER[0]
    keep, take = E.coefficients(0.99)
    hip.adamw_step_groups_ema(d["p"][sl], master, d["g"][sl], d["m"][sl], d["v"][sl], ema, end8, scale, wd, lr, b1, b2, eps, 2, keep, take)


@pytest.mark.parametrize("with_master", [False, True], ids=["plain", "master"])
def test_fused_step_rejects_a_null_average(with_master):
    hip = hipmod()
    host, d, tables = _refusal_state(16)
    with pytest.raises(RuntimeError):
        _fused(hip, d, tables, d["master"] if with_master else None, None)
    torch.cuda.synchronize()
    assert _untouched(host, d)


def test_fused_step_rejects_257_groups():
    hip = hipmod()
    host, d, tables = _refusal_state(257)
    with pytest.raises(RuntimeError):
        _fused(hip, d, tables, d["master"], d["e"])
    torch.cuda.synchronize()
    assert _untouched(host, d)
    k = slice(0, 2048)
    _fused(hip, d, tables, d["master"][k], d["e"][k], k, slice(0, 256))  # 256 are taken
    torch.cuda.synchronize()
    assert not torch.equal(d["e"][k].cpu(), host["e"][k]) and M.cast_matches(d["p"][k], d["master"][k]) == 0
    assert torch.equal(d["e"][2048:].cpu(), host["e"][2048:]) and torch.equal(d["master"][2048:].cpu(), host["master"][2048:])


def test_fused_step_rejects_an_average_that_overlaps_the_master():
    hip = hipmod()
    host, d, tables = _refusal_state(16)
    with pytest.raises(RuntimeError):
        _fused(hip, d, tables, d["master"], d["master"])
    both = torch.cat([d["master"], d["e"]])  # two ranges of one allocation that share 64 elements
    before = both.clone()
    with pytest.raises(RuntimeError):
        _fused(hip, d, tables, both[:128], both[64:192])
    torch.cuda.synchronize()
    assert _untouched(host, d) and torch.equal(M.bits(both), M.bits(before))
    _fused(hip, d, tables, both[:128], both[128:])  # adjacent is not overlapping
    torch.cuda.synchronize()
    assert not torch.equal(M.bits(both[128:]), M.bits(before[128:]))


def test_the_wrappers_reject_an_average_that_does_not_cover_the_parameters():
    """The kernels run over p.numel() elements: a shorter, strided or non-fp32 average (or master) is refused before any launch."""
    hip = hipmod()
    host, d, tables = _refusal_state(16)
    keep, take = E.coefficients(0.99)
    wide = torch.zeros(256, dtype=torch.float32, device=DEV)
    for bad in (d["e"][:120], wide[::2], d["e"].double(), d["p"].clone()):
        with pytest.raises((RuntimeError, TypeError)):
            hip.ema_step(bad, d["p"], keep, take)
        with pytest.raises((RuntimeError, TypeError)):
            _fused(hip, d, tables, None, bad)
        with pytest.raises((RuntimeError, TypeError)):
            _fused(hip, d, tables, bad, d["e"])
    torch.cuda.synchronize()
    assert _untouched(host, d) and not bool(wide.any())


# ------------------------------------------------------------------------------------------------------------------ d
def test_fused_adamw_with_ema_follows_the_reference_ema_module(golden_dir):
    import os
    from one_peace_amd.optim import FusedAdamW
    fx = torch.load(os.path.join(golden_dir, "adamw_master.pt"), weights_only=False)
    fe = torch.load(os.path.join(golden_dir, "ema.pt"), weights_only=False)
    worst, worst_ref, _, compared = E.run_golden(fx, fe, FusedAdamW, DEV)  # asserts run_fixture's criteria and the copy of step 1
    assert worst <= 1.0 and worst_ref <= 1.0 and compared > 20000


# ------------------------------------------------------------------------------------------------------------------ e
def test_which_entries_fused_adamw_calls_with_and_without_ema(monkeypatch):
    """Without ema: the entries of before, none of the new ones.  With ema: ONE fused call per step, with or without the master, and
    neither hip.ema_step nor an old entry -- the fused entry is the route profiles/ema_mi355x.json found faster than the pair."""
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd.optim import FusedAdamW
    hip = hipmod()
    names = ("adamw_step_groups", "adamw_step_groups_master", "adamw_step_groups_ema", "ema_step")
    calls = dict.fromkeys(names, 0)

    def count(key, fn):
        def wrapper(*a, **kw):
            calls[key] += 1
            return fn(*a, **kw)
        return wrapper

    for k in names:
        monkeypatch.setattr(hip, k, count(k, getattr(hip, k)))
    for master_weights in (False, True):
        for with_ema in (False, True):
            for k in names:
                calls[k] = 0
            model = M.EightParams(1.0).to(DEV).to(torch.bfloat16)
            flat = FlatParameters(model)
            ema = FlatEMA(flat, decay=0.5) if with_ema else None
            opt = FusedAdamW(flat, lr=1e-2, master_weights=master_weights, ema=ema)
            for _ in range(2):
                model.w.grad.fill_(0.01)
                opt.step()
            torch.cuda.synchronize()
            if with_ema:
                want = {"adamw_step_groups_ema": 2}
                assert ema.num_updates == 2 and bool((ema.shadow < 1.0).all()) and bool((ema.shadow > flat.params.float()).all())
            else:
                want = {"adamw_step_groups_master" if master_weights else "adamw_step_groups": 2}
            assert calls == dict(dict.fromkeys(names, 0), **want), (master_weights, with_ema, calls)
            assert bool((flat.params.cpu().float() < 1.0).all())


# ------------------------------------------------------------------------------------------------------------------ f
def test_applied_on_the_device_refreshes_the_cached_transposed_weights():
    from one_peace_amd import ops
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd.optim import FusedAdamW
    torch.manual_seed(5)
    model = torch.nn.Linear(64, 128).to(DEV).to(torch.bfloat16)
    flat = FlatParameters(model)
    ema = FlatEMA(flat, decay=0.9)
    opt = FusedAdamW(flat, lr=1e-2, master_weights=True, ema=ema)
    for _ in range(3):
        flat.grads.copy_(torch.randn(flat.numel, device=DEV).to(torch.bfloat16))
        opt.step()
    wt = ops._transposed(model.weight)  # the cached copy the input-gradient GEMMs read
    assert torch.equal(wt, model.weight.detach().t())
    before, master = flat.params.clone(), opt.master.clone()
    want = ema.shadow.to(torch.bfloat16)
    assert E.changed_share(want, before) > 0.5
    pick = torch.eye(64, device=DEV)[:16].to(torch.bfloat16)
    o = {n: o for n, _, o, _ in flat.entries}["weight"]
    with ema.applied():
        assert torch.equal(M.bits(flat.params), M.bits(want))
        avg_w = want[o:o + 64 * 128].view(128, 64)
        assert torch.equal(model.weight.detach(), avg_w)
        inside = ops._transposed(model.weight)
        assert inside.data_ptr() == wt.data_ptr() and torch.equal(inside, avg_w.t()), "the cached transposed weight is not the averaged one"
        # a forward with one-hot rows picks single weights: exact whatever GEMM runs it
        assert torch.equal(pick @ inside, avg_w.t()[:16]) and torch.equal(torch.nn.functional.linear(pick, model.weight), avg_w.t()[:16])
    torch.cuda.synchronize()
    assert torch.equal(M.bits(flat.params), M.bits(before)), "the parameters did not come back bit for bit"
    assert torch.equal(M.bits(opt.master), M.bits(master)), "the master was touched"
    assert torch.equal(ops._transposed(model.weight), before[o:o + 64 * 128].view(128, 64).t()), "the caches were not refreshed on exit"
    assert torch.equal(ema.shadow.to(torch.bfloat16), want)


# ------------------------------------------------------------------------------------------------------------------ g
class OneVector(torch.nn.Module):
    """STRIDE + 8 parameters: the last vector is the first of a second grid stride."""

    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(R.SIZES[2]))


POS = R.SIZES[2] - 3


def _poisoned(master_weights, value):
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.ema import FlatEMA
    from one_peace_amd.optim import FusedAdamW
    n = R.SIZES[2]
    _, p, g, _, _, e, _, _ = E.case_state(n, 1, False)
    flat = FlatParameters(OneVector().to(DEV).to(torch.bfloat16), no_decay=lambda name, q: False)
    with torch.no_grad():
        flat.params.copy_(p)
    ema = FlatEMA(flat, decay=0.99)
    ema.shadow.copy_(e)
    opt = FusedAdamW(flat, lr=1e-2, master_weights=master_weights, ema=ema)
    flat.grads.copy_(g)
    flat.grads[POS] = value
    return flat, ema, opt, p, e


@pytest.mark.parametrize("master_weights", [False, True], ids=["plain", "master"])
def test_a_nan_gradient_without_clipping_reaches_only_its_own_element_of_the_average(master_weights):
    flat, ema, opt, p, e = _poisoned(master_weights, float("nan"))
    assert opt.step(grad_scale=0.25, clip_norm=0.0) is None
    torch.cuda.synchronize()
    shadow = ema.shadow.cpu()
    finite = torch.isfinite(shadow)
    assert int((~finite).sum()) == 1 and not bool(finite[POS]), "non-finite elements of the average: %d" % int((~finite).sum())
    keep, take = E.coefficients(0.99)
    E.assert_step(shadow, e, flat.params, keep, take, "nan without clipping", check=finite)
    assert E.changed_share(flat.params, p) >= 0.9


def test_a_nan_gradient_makes_the_whole_average_nan_with_the_clipped_step():
    """As the unfused pair would: the clip coefficient is NaN, every parameter comes out NaN, and the average of NaN parameters is NaN."""
    flat, ema, opt, _, _ = _poisoned(False, float("nan"))
    norm = opt.step(grad_scale=0.25, clip_norm=R.CLIP_NORM)
    torch.cuda.synchronize()
    assert math.isnan(float(norm))
    assert int(torch.isfinite(ema.shadow).sum()) == 0 and int(torch.isfinite(flat.params.float()).sum()) == 0
