"""Shared by tests/test_ema_cpu.py and tests/test_ema_gpu.py: the fp32 weight average (one-peace_amd/ema.py; csrc/elementwise.hip:
ema_step_kernel, adamw_kernel<GROUPS, MASTER, EMA>) stated in fp64, its acceptance criterion, an fp32 emulation with planted faults and the
seeded states, on top of tests/adamw_ref.py and tests/adamw_master_ref.py.  Plain torch on the CPU; nothing here needs a GPU.

The rule:   e' = keep e + take p^      keep = float32(decay), take = float32(1.0 - decay) (the subtraction in double), p^ the bf16
parameter as stored after the optimiser step, e the fp32 average.  The two coefficients cross the C ABI as float, so the fp64
statement starts from the fp32 numbers.

Criterion, for EVERY element, with E = keep e + take p^ in fp64:

    |got - E| <= 2^-24 (|keep e| + |take p^| + |E|) + 2^-149

derived, not measured: fl32(keep e) is off by at most 2^-24 |keep e|; an fma then rounds the exact take p^ + fl32(keep e) once, at most
2^-24 |E| (1 + 2^-24) -- and if the sum is not contracted, the product take p^ is rounded too, 2^-24 |take p^|.  2^-149 is the smallest
fp32 denormal (gradual underflow or flush to zero of the last bit).  Over K steps a run is held to the SUM of the per-step bounds of
the fp64 run from the same start: an error carried in e passes through the next step with the factor keep <= 1."""
import torch

from tests import adamw_master_ref as M
from tests import adamw_ref as R

DENORM = 2.0 ** -149


def coefficients(decay):
    """(keep, take) as the fp32 numbers the kernels receive, widened to fp64."""
    return R.f32(decay), R.f32(1.0 - decay)


def expected(e, p_hat, keep, take):
    """E and the per-element bound, fp64.  e: fp32 (or the fp64 of an fp64 run), p_hat: bf16."""
    e, p = e.detach().to("cpu", torch.float64), p_hat.detach().to("cpu", torch.float64)
    a, b = keep * e, take * p
    E = a + b
    return E, R.U32 * (a.abs() + b.abs() + E.abs()) + DENORM


def figures(got, e_old, p_hat, keep, take, check=None):
    """Violations of the criterion and the largest share of the bound used (a NaN is a violation), on `check` (default: all)."""
    E, bound = expected(e_old, p_hat, keep, take)
    err = (got.detach().to("cpu", torch.float64) - E).abs()
    if check is not None:
        err, bound = err[check], bound[check]
    used = torch.nan_to_num(err / bound, nan=float("inf"))
    return {"bad": int((~(err <= bound)).sum()), "used": float(used.max()) if used.numel() else 0.0, "n": err.numel()}


def assert_step(got, e_old, p_hat, keep, take, what="", check=None):
    f = figures(got, e_old, p_hat, keep, take, check)
    print("%s: EMA at most %.3f of the bound, %d of %d outside" % (what, f["used"], f["bad"], f["n"]))
    assert f["bad"] == 0, "%s: %d of %d EMA elements outside the bound (worst %.2f of it)" % (what, f["bad"], f["n"], f["used"])
    return f


def apart(planted, e_old, p_hat, keep, take):
    """Share of elements whose planted value is more than TWICE the bound from E: what a planted-fault case must assert of its state
    before it relies on the criterion rejecting the fault."""
    E, bound = expected(e_old, p_hat, keep, take)
    return float(((planted.detach().double() - E).abs() > 2 * bound).double().mean())


def rejected(planted, e_old, p_hat, keep, take):
    """Share of elements the criterion rejects."""
    f = figures(planted, e_old, p_hat, keep, take)
    return f["bad"] / f["n"]


class Fp64Run:
    """The fp64 run of the rule from a start, with the summed per-step bound."""

    def __init__(self, e0):
        self.e = e0.detach().to("cpu", torch.float64).clone()
        self.budget = torch.zeros_like(self.e)

    def step(self, p_hat, keep, take):
        E, bound = expected(self.e, p_hat, keep, take)
        self.e, self.budget = E, self.budget + bound

    def used(self, got):
        err = (got.detach().to("cpu", torch.float64) - self.e).abs()
        return float(torch.nan_to_num(err / self.budget, nan=float("inf")).max())


# ------------------------------------------------------------------------------------------------------------------
# states
# ------------------------------------------------------------------------------------------------------------------
LR = 1e-2        # adamw_ref.HYPER[0].  With P_SCALE a step moves a parameter by many bf16 spacings (~2^-8 * 1e-3 = 4e-6) also in the
P_SCALE = 1e-3   # group with the smallest lr scale of adamw_ref.group_tables, 0.65^11: lr_g = 8.8e-5 -- the changed share the tests assert
G_SCALE = 1e-2


def make_ema_state(n, step, seed=0, clip=None):
    """master (fp32, low half non-zero), p = bf16(master), g, m, v as adamw_master_ref.make_master_state at P_SCALE; with
    clip = (grad_scale, where) the gradient and moments of adamw_ref.make_clip_state.  e: an fp32 average that LAGS the parameters --
    |e| in [1/8, 1/4) |p|, same sign, low half non-zero.  The lag is what the planted-fault cases need: the bound grows with |e|, the
    faults with |p| (a bf16 rounding of p, a stale p), and with |e| ~ |p| the share of elements whose bf16 rounding error is within
    twice the bound would be ~1 % at decay 0.99 -- with an average this far behind, the 99 % the cases assert holds with room."""
    master, p, g, m, v = M.make_master_state(n, step, G_SCALE, P_SCALE, seed)
    if clip is not None:
        _, g, m, v = R.make_clip_state(n, clip[0], clip[1], step, seed)
    gen = torch.Generator().manual_seed(1000 * seed + 53)
    e = p.float() * (0.125 + 0.125 * torch.rand(n, generator=gen))
    low = torch.randint(1, 1 << 16, (n,), generator=gen, dtype=torch.int32)
    e = ((e.view(torch.int32) & ~0xFFFF) | low).view(torch.float32).clone()
    assert bool(torch.isfinite(e).all())
    return master, p, g, m, v, e


_STATES = {}


def case_state(n, step, clip):
    """Host state of a one-step case, built once and shared by the GPU tests (they work on copies): master, p, g, m, v, e
    (+ grad_scale, clip_norm)."""
    key = (n, step, clip)
    if key not in _STATES:
        gs, clip_norm = (0.25, R.CLIP_NORM) if clip else (1.0, 0.0)
        st = make_ema_state(n, step, seed=2, clip=(gs, "above") if clip else None)
        if clip:
            R.assert_clip_landing(st[2], gs, "above")
        _STATES[key] = st + (gs, clip_norm)
    return _STATES[key]


def changed_share(p_new, p_old):
    """Share of elements whose bf16 value the step changed."""
    return float((M.bits16(p_new) != M.bits16(p_old)).double().mean())


# ------------------------------------------------------------------------------------------------------------------
# fp32 emulation (torch on the CPU: the product and the sum rounded separately, as the two reference lines do it) with planted faults
# ------------------------------------------------------------------------------------------------------------------
PLANTED = ("stale_parameter", "keep_and_take_swapped", "unrounded_parameter", "shadow_through_bf16")


def emulate_ema_fp32(e, p_old, p_new_f32, decay, planted=None):
    """e' from the fp32 result of the optimiser step (p_new_f32; the stored parameter is its bf16 cast) in fp32 arithmetic."""
    keep = torch.tensor(decay, dtype=torch.float32)
    take = torch.tensor(1.0 - decay, dtype=torch.float32)
    if planted == "keep_and_take_swapped":
        keep, take = take, keep
    src = p_new_f32.to(torch.bfloat16).float()
    if planted == "stale_parameter":
        src = p_old.float()
    elif planted == "unrounded_parameter":
        src = p_new_f32.float()
    out = e * keep + take * src
    return out.to(torch.bfloat16).float() if planted == "shadow_through_bf16" else out


# ------------------------------------------------------------------------------------------------------------------
# tests/golden/ema.pt: the reference's EMAModule (fp32, decay 0.999, ema_start_update 2) over the three steps of adamw_master.pt
# ------------------------------------------------------------------------------------------------------------------
def fixture_model(fx, device):
    """The fixture's model in bf16 and its FlatParameters with the reference's groups, as adamw_master_ref.run_fixture builds them."""
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.optim import reference_param_groups
    from tests.model_util import build_retrieval, load_synth
    cfg = fx["cfg"]
    model = load_synth(build_retrieval(dict(cfg), fx["vocab"]), fx["shapes"]).to(device).to(torch.bfloat16)
    no_decay, lr_scale = reference_param_groups(model, cfg["layers"], fx["optim"]["layer_decay"])
    return model, FlatParameters(model, no_decay=no_decay, lr_scale=lr_scale)


def run_golden(fx_master, fx_ema, base_cls, device):
    """base_cls(master_weights=True, ema=FlatEMA(decay, start_update of the fixture)) through adamw_master_ref.run_fixture -- whose
    criteria for the parameters and the master hold unchanged -- with the average looked at after every step, on the stored elements:

      * step 1 (updates 1 < start_update) is a copy: the average equals float(p) bit for bit, everywhere;
      * where the optimiser's bf16 parameters equal the reference's in every step so far (adamw_master.pt's `#bf16`; the two fp32
        masters round apart in < 1e-3 of the elements, as run_fixture allows), the average and the reference's are both within the
        summed per-step bound of the fp64 run over the reference's parameters.
    Returns the worst share of that budget the optimiser's average used, the reference's, the number of compared elements whose fp32
    average is not bit-identical to the reference's, and the number compared."""
    from one_peace_amd.ema import FlatEMA
    seen = []

    class WithEMA(base_cls):
        def __init__(self, flat, **kw):
            super().__init__(flat, ema=FlatEMA(flat, decay=fx_ema["ema"]["decay"], start_update=fx_ema["ema"]["start_update"]), **kw)

        def step(self, *a, **kw):
            out = super().step(*a, **kw)
            seen.append((self.flat, self.ema.num_updates, self.ema.shadow.detach().cpu().clone(), self.flat.params.detach().cpu().clone()))
            return out

    assert M.run_fixture(fx_master, WithEMA, device) <= 1.0
    assert [s[1] for s in seen] == [1, 2, 3]
    flat = seen[0][0]
    assert torch.equal(seen[0][2], seen[0][3].float()), "the first step (updates < start_update) is not a copy"
    worst, worst_ref, unlike_bits, compared, total = 0.0, 0.0, 0, 0, 0
    for n, _, o, _ in flat.entries:
        j = fx_ema["after"][0][n + "#ema"].numel()
        run, same = None, torch.ones(j, dtype=torch.bool)
        for step, (_, _, shadow, params) in enumerate(seen, start=1):
            ref_p, ref_e = fx_master["after"][step - 1][n + "#bf16"], fx_ema["after"][step - 1][n + "#ema"]
            keep, take = coefficients(fx_ema["decays"][step - 1])
            run = Fp64Run(ref_p.float()) if run is None else run  # the start does not matter: the first step has keep = 0
            run.step(ref_p, keep, take)
            same &= M.bits16(params[o:o + j]) == M.bits16(ref_p)
            if bool(same.any()):
                err = (shadow[o:o + j].double() - run.e).abs()[same] / run.budget[same]
                err_ref = (ref_e.double() - run.e).abs()[same] / run.budget[same]
                worst, worst_ref = max(worst, float(err.max())), max(worst_ref, float(err_ref.max()))
                if step == len(seen):
                    unlike_bits += int((shadow[o:o + j].view(torch.int32) != ref_e.view(torch.int32))[same].sum())
        compared += int(same.sum())
        total += j
    assert compared >= 0.999 * total, (compared, total)
    print("ema fixture/%s: average at most %.3f, the reference's %.3f of the summed bound; %d of %d compared elements differ in bits" % (
        base_cls.__name__, worst, worst_ref, unlike_bits, compared))
    return worst, worst_ref, unlike_bits, compared
