"""Shared by tests/test_adamw_master_cpu.py and tests/test_adamw_master_gpu.py: AdamW with an fp32 master copy of the bf16
parameters (csrc/elementwise.hip: adamw_kernel<GROUPS, MASTER>; optim.FusedAdamW / TorchAdamW with master_weights=True) on top of the
fp64 statement and the states of tests/adamw_ref.py.  Plain torch on the CPU; nothing here needs a GPU.

Criteria for ONE step from a given state (master_old fp32, g bf16, m, v fp32), for every element, with
E = adamw_ref.Expected(master_old, g, m, v, ...) -- adamw_fp64 takes the fp32 master as `p` as it stands:

  master   |master' - E.p| <= E.delta = 8 * 2^-24 * (|master_old| + |u|): the fp32 roundings adamw_ref.py derives delta from.  The
           bf16 interval and TWO_VALUED_CAP of adamw_ref.py play no part: the fp32 value itself is compared.
  p        p' == master'.to(bfloat16), bit for bit (torch's cast is round-to-nearest-even): the kernel's own rounding, of the value
           it stored.  NaNs are compared as NaNs.
  m, v     inside E.m_bound / E.v_bound.

Many steps: the error of a run against the fp64 run from the same start is held to the SUM of the per-step deltas of the fp64
run (a step's rounding errors are charged to that step's |p| + |u|; an error carried in p passes through the next step with a
factor 1 - wd lr_g <= 1, and the errors carried in m and v are what delta charges to |u|)."""
import math

import torch

from tests import adamw_ref as R


def bits16(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def bits(t):
    """The bit pattern of a bf16 or fp32 tensor, for comparisons in which a NaN equals itself and -0 differs from 0."""
    t = t.detach().cpu().contiguous()
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def cast_matches(p, master):
    """Number of elements where p is not the round-to-nearest-even bf16 of master (a NaN matches a NaN)."""
    p, want = p.detach().cpu(), master.detach().cpu().to(torch.bfloat16)
    both_nan = torch.isnan(p) & torch.isnan(want)
    return int(((bits16(p) != bits16(want)) & ~both_nan).sum())


def figures(exp, master, p, m, v):
    """Violation counts of the one-step criteria and the largest share of each budget used, on exp.check."""
    c = exp.check
    ms, mm, vv = (t.detach().to("cpu", torch.float64)[c] for t in (master, m, v))
    em, e1, e2 = (ms - exp.p[c]).abs(), (mm - exp.m[c]).abs(), (vv - exp.v[c]).abs()
    mx = lambda t: float(torch.nan_to_num(t, nan=math.inf).max()) if t.numel() else 0.0  # noqa: E731
    pc, wc = p.detach().cpu()[c], master.detach().cpu()[c]
    return {"master_bad": int((~(em <= exp.delta[c])).sum()), "p_bad": cast_matches(pc, wc),
            "m_bad": int((~(e1 <= exp.m_bound[c])).sum()), "v_bad": int((~(e2 <= exp.v_bound[c])).sum()),
            "master_used": mx(em / exp.delta[c]), "m_used": mx(e1 / exp.m_bound[c]), "v_used": mx(e2 / exp.v_bound[c]), "n": int(c.sum())}


def passes(f):
    return f["master_bad"] == 0 and f["p_bad"] == 0 and f["m_bad"] == 0 and f["v_bad"] == 0


def assert_step(exp, master, p, m, v, what=""):
    f = figures(exp, master, p, m, v)
    print("%s: master %.3f of delta, m %.3f, v %.3f of the bound; p != bf16(master) in %d of %d" % (
        what, f["master_used"], f["m_used"], f["v_used"], f["p_bad"], f["n"]))
    assert passes(f), "%s: outside the criteria: master %d, p %d, m %d, v %d of %d elements (worst master %.2f delta, m %.2f, v %.2f)" % (
        what, f["master_bad"], f["p_bad"], f["m_bad"], f["v_bad"], f["n"], f["master_used"], f["m_used"], f["v_used"])
    return f


def make_master_state(n, step, gscale, pscale, seed=0):
    """adamw_ref.make_state with the parameter drawn as fp32: a master whose low 16 bits are non-zero in EVERY element (so that
    bf16(master) != master everywhere), and p = bf16(master) as a step leaves the pair.  Returns master, p, g, m, v.

    |master| is kept above 2^-6 pscale.  adamw_ref.py's note on delta: the rounding error of m reaches u as up to ~6.5 * 2^-24 *
    step_size whatever is left of m, inside delta only where |p_old| >~ step_size.  Its bf16 interval forgives that in the few
    elements of N(0, 1) that lie near zero; the fp32 comparison made here does not (at lr 1e-2 and 8M elements the expected number of
    elements with 8 |p| below their m-error is ~16).  With the floor, 2^-6 > 0.81 * 1e-2, the largest step size the cases use at
    parameter scale 1; a kernel treats a parameter near zero like any other."""
    _, g, m, v = R.make_state(n, step, gscale, pscale, seed)
    gen = torch.Generator().manual_seed(1000 * seed + 41)
    master = torch.randn(n, generator=gen) * pscale
    master = torch.where(master < 0, -1.0, 1.0) * master.abs().clamp_min(2.0 ** -6 * pscale)
    bits = master.view(torch.int32)
    low = torch.randint(1, 1 << 16, (n,), generator=gen, dtype=torch.int32)
    master = ((bits & ~0xFFFF) | low).view(torch.float32).clone()
    assert bool(((master.view(torch.int32) & 0xFFFF) != 0).all()) and bool(torch.isfinite(master).all())
    return master, master.to(torch.bfloat16), g, m, v


# ------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the operation order of adamw_kernel<GROUPS, MASTER> (no FMA contraction), with planted errors
# ------------------------------------------------------------------------------------------------------------------
PLANTED = ("master_read_from_bf16_p", "p_rounded_before_decay", "master_stored_as_bf16")


def emulate_master_fp32(master, p, g, m, v, step, lr, beta1, beta2, eps, grad_scale=1.0, clip_norm=0.0, sqnorm=None, lr_scale=1.0,
                        weight_decay=0.0, planted=None):
    """Returns (master', p' bf16, m', v').  The expressions are adamw_ref.emulate_fp32's for the group tables, with the master
    in the place of float(p)."""
    F = lambda x: torch.tensor(x, dtype=torch.float32) if not torch.is_tensor(x) else x.float()  # noqa: E731
    lr, b1, b2, eps, gs = F(lr), F(beta1), F(beta2), F(eps), F(grad_scale)
    bc1, bc2 = 1.0 - float(b1.double()) ** step, 1.0 - float(b2.double()) ** step
    lr_g = lr * F(lr_scale)
    step_size = lr_g * F(math.sqrt(bc2) / bc1)
    decay_mul = 1.0 - F(weight_decay) * lr_g
    if clip_norm > 0:
        sq = F(float(R.sqnorm_fp64(g))) if sqnorm is None else F(sqnorm).cpu()
        c = F(clip_norm).double() / (gs.double().abs() * sq.double().sqrt() + 1e-6)
        gs = (gs.double() * c).float() if bool(c < 1.0) or bool(c != c) else gs
    gr = g.float() * gs
    m = m * b1 + (1.0 - b1) * gr
    v = v * b2 + (1.0 - b2) * gr * gr
    upd = step_size * (m / (v.sqrt() + eps))
    pf = p.float() if planted == "master_read_from_bf16_p" else master
    new = pf * decay_mul - upd
    pb = (pf - upd).to(torch.bfloat16) if planted == "p_rounded_before_decay" else new.to(torch.bfloat16)
    if planted == "master_stored_as_bf16":
        new = new.to(torch.bfloat16).float()
    return new, pb, m, v


# ------------------------------------------------------------------------------------------------------------------
# the two deterministic 100-step cases: updates far below half a bf16 spacing of the parameter
# ------------------------------------------------------------------------------------------------------------------
# (start value, lr, the bf16 value the master arrangement ends on); gradient 0.01 throughout, beta (0.9, 0.98), eps 1e-6, wd 0
HUNDRED = {"one": (1.0, 1e-4, 0.98828125), "small": (0.02, 1e-5, 0.01904296875)}
HUNDRED_GRAD, HUNDRED_BETAS, HUNDRED_EPS, HUNDRED_STEPS = 0.01, (0.9, 0.98), 1e-6, 100


class EightParams(torch.nn.Module):
    """One vector (8 elements) holding the start value of a 100-step case."""

    def __init__(self, value):
        super().__init__()
        self.w = torch.nn.Parameter(torch.full((8,), float(value)))


def hundred_fp64(name):
    """The fp64 run of a case from the bf16 start value: the final parameter and the sum of the per-step deltas (scalars)."""
    start, lr, _ = HUNDRED[name]
    p = torch.full((1,), start).to(torch.bfloat16).double()
    g = torch.full((1,), HUNDRED_GRAD).to(torch.bfloat16)
    m, v, budget = torch.zeros(1), torch.zeros(1), 0.0
    for t in range(1, HUNDRED_STEPS + 1):
        p1, m, v, u = R.adamw_fp64(p, g, m, v, t, lr, HUNDRED_BETAS[0], HUNDRED_BETAS[1], HUNDRED_EPS)
        budget += R.P_ULPS * R.U32 * float(p.abs() + u.abs())
        p = p1
    return float(p), budget


def run_hundred(name, opt_cls, device, master_weights):
    """A case through opt_cls over FlatParameters of EightParams in bf16; returns (start bf16, optimiser, flat)."""
    from one_peace_amd.distributed import FlatParameters
    start, lr, _ = HUNDRED[name]
    model = EightParams(start).to(device).to(torch.bfloat16)
    flat = FlatParameters(model)
    p0 = flat.params.detach().cpu().clone()
    opt = opt_cls(flat, lr=lr, betas=HUNDRED_BETAS, eps=HUNDRED_EPS, weight_decay=0.0, master_weights=master_weights)
    for _ in range(HUNDRED_STEPS):
        model.w.grad.fill_(HUNDRED_GRAD)
        opt.step()
    return p0, opt, flat


def assert_hundred(name, opt_cls, device):
    start, lr, end_bf16 = HUNDRED[name]
    p0, opt, flat = run_hundred(name, opt_cls, device, False)
    assert opt.master is None
    assert torch.equal(bits16(flat.params), bits16(p0)), "%s: the bf16-only arrangement was expected to lose every update" % name
    p0, opt, flat = run_hundred(name, opt_cls, device, True)
    ref, budget = hundred_fp64(name)
    got_m, got_p = opt.master.detach().cpu().double(), flat.params.detach().cpu()
    err = float((got_m - ref).abs().max())
    print("%s/%s: master %.9g (fp64 %.9g), error %.3g of the summed delta %.3g; bf16 %r" % (
        name, opt_cls.__name__, float(got_m[0]), ref, err / budget, budget, float(got_p[0])))
    assert not torch.equal(bits16(got_p), bits16(p0)), "%s: the bf16 copy has not moved" % name
    assert err <= budget, "%s: master off by %.3g, %.2f of the summed per-step delta" % (name, err, err / budget)
    assert cast_matches(got_p, opt.master) == 0
    assert float(R.bf16_rne(torch.tensor(ref, dtype=torch.float64))) == end_bf16, "the case itself moved"
    assert bool((got_p.double() == end_bf16).all()), (name, got_p)


# ------------------------------------------------------------------------------------------------------------------
# tests/golden/adamw_master.pt: the reference's FP16Optimizer arrangement on the micro model, three steps
# ------------------------------------------------------------------------------------------------------------------
def run_fixture(fx, opt_cls, device):
    """opt_cls(master_weights=True) over the fixture's model, groups and gradients, next to two fp64 runs of the rule over the flat
    layout.  Both fp32 runs round their gradient norm on their own (the reference's fp32 norm of per-parameter fp32 norms is 1.2e-6
    off the exact one, 20 fp32 roundings; where |g'| is near eps the update follows the norm with a third of that, beyond delta), so
    each is held to the fp64 run that is given ITS norm, as tests/test_adamw_fp64_gpu.py gives the device's sum of squares to its
    reference.  After every step:
      * the optimiser's master within the summed per-step delta of the fp64 run with the norm the step returned,
      * the reference's masters within the summed per-step delta of the fp64 run with the norm the reference recorded (the fp64
        statement IS the reference's arithmetic),
      * the two norms within 4e-6 of each other: (32 + n / 262144) fp32 roundings for the device's sum (adamw_ref.norm_bound), the
        1.2e-6 above for the reference's,
      * p == bf16(master), and equal to the reference's bf16 cast wherever the two masters round alike.
    Returns the largest share of the budget the optimiser's master used."""
    from oracle import synth
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.optim import reference_param_groups
    from tests.model_util import build_retrieval, load_synth
    cfg, oc = fx["cfg"], fx["optim"]
    m = load_synth(build_retrieval(dict(cfg), fx["vocab"]), fx["shapes"]).to(device).to(torch.bfloat16)
    no_decay, lr_scale = reference_param_groups(m, cfg["layers"], oc["layer_decay"])
    flat = FlatParameters(m, no_decay=no_decay, lr_scale=lr_scale)
    # hyperparameters as the C ABI carries them (adamw_ref.py: rounded to fp32 first), for the torch route too
    opt = opt_cls(flat, lr=R.f32(oc["lr"][0]), betas=(R.f32(oc["betas"][0]), R.f32(oc["betas"][1])), eps=R.f32(oc["eps"]),
                  weight_decay=R.f32(oc["weight_decay"]), master_weights=True)
    assert opt.master.dtype == torch.float32 and opt.master.numel() == flat.numel
    counts = [(e - s) // 8 for s, e, _, _ in flat.groups]
    scale = R.expand_groups(counts, [g[2] for g in flat.groups])
    wd = R.expand_groups(counts, [oc["weight_decay"] if g[3] else 0.0 for g in flat.groups])
    p0 = flat.params.detach().cpu().double()
    runs = {k: dict(p=p0, m=torch.zeros_like(p0), v=torch.zeros_like(p0), budget=torch.zeros_like(p0)) for k in ("own", "ref")}
    worst, worst_ref, unlike, compared = 0.0, 0.0, 0, 0
    for step, lr in enumerate(oc["lr"], start=1):
        opt.zero_grad()
        for n, p in m.named_parameters():
            p.grad.copy_(synth.optim_grad(n, p.shape, step).to(device))
        opt.set_lr(R.f32(lr))
        g = flat.grads.detach().cpu().clone()
        norm = opt.step(clip_norm=oc["clip_norm"])
        norms = {"own": float(norm), "ref": float(fx["grad_norms"][step - 1])}
        print("step %d: gradient norm %.7f, the reference's %.7f" % (step, norms["own"], norms["ref"]))
        assert abs(norms["own"] - norms["ref"]) <= 4e-6 * norms["ref"], (step, norms)
        for k, r in runs.items():
            old = r["p"]
            r["p"], r["m"], r["v"], u = R.adamw_fp64(old, g, r["m"], r["v"], step, lr, oc["betas"][0], oc["betas"][1], oc["eps"],
                                                     clip_norm=oc["clip_norm"], sqnorm=norms[k] ** 2, lr_scale=scale, weight_decay=wd)
            r["budget"] = r["budget"] + R.P_ULPS * R.U32 * (old.abs() + u.abs())
        master = opt.master.detach().cpu()
        params = flat.params.detach().cpu()
        assert cast_matches(params, master) == 0, "step %d: p is not bf16(master)" % step
        err = (master.double() - runs["own"]["p"]).abs() / runs["own"]["budget"].clamp_min(R.TINY)
        worst = max(worst, float(err.max()))
        assert bool((err <= 1.0).all()), "step %d: master off by %.2f of the summed per-step delta" % (step, float(err.max()))
        snap = fx["after"][step - 1]
        for n, _, o, k in flat.entries:
            ref = snap[n + "#master"]
            j = ref.numel()
            e = (ref.double() - runs["ref"]["p"][o:o + j]).abs() / runs["ref"]["budget"][o:o + j]
            worst_ref = max(worst_ref, float(e.max()))
            assert bool((e <= 1.0).all()), "step %d: the reference's %s is %.2f of the budget off the fp64 statement" % (step, n, float(e.max()))
            # | |a| - |b| | <= |a - b|: both within their budgets of fp64 runs that differ by the norm alone, + the stored norm's rounding
            want = float(snap[n + "#norm"])
            assert abs(float(master[o:o + k].double().norm()) - want) <= 3 * float(runs["own"]["budget"][o:o + k].norm()) + R.U32 * want, (step, n)
            same = master[o:o + j].to(torch.bfloat16) == ref.to(torch.bfloat16)
            assert torch.equal(params[o:o + j][same], snap[n + "#bf16"][same]), (step, n)
            unlike += int((~same).sum())
            compared += j
        # masters within ~2^-20 relative of each other straddle a bf16 rounding boundary (every 2^-8 relative) in ~2^-12 of the elements
        assert unlike <= 1e-3 * compared, (step, unlike, compared)
    print("fixture/%s: master at most %.3f, the reference's masters %.3f of the summed per-step delta; %d of %d bf16 casts differ" % (
        opt_cls.__name__, worst, worst_ref, unlike, compared))
    return worst
