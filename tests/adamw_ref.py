"""Shared by tests/test_adamw_ref_cpu.py, tests/test_adamw_fp64_gpu.py and the AdamW tests of tests/test_ops_gpu.py: the fused
AdamW step (csrc/elementwise.hip: adamw_kernel<GROUPS, MASTER, EMA>) and the global gradient norm (sqnorm_*_kernel) stated in fp64,
the acceptance criteria for ONE step from a given state, an fp32 emulation of the kernels' operation order with planted errors,
and the seeded states and case lists.  Plain torch on the CPU; nothing here needs a GPU.

The rule (oracle/onepeace_oracle.py: adamw_step, clip_coef; one_peace/optim/adam.py:186-253, fairseq/utils.py:349-397):

    c    = min(1, clip_norm / (|grad_scale| sqrt(sqnorm) + 1e-6))        (1 without clipping; NaN stays NaN)
    g'   = g grad_scale c
    m    = beta1 m + (1 - beta1) g'          v = beta2 v + (1 - beta2) g'^2
    u    = lr_g sqrt(1 - beta2^t) / (1 - beta1^t) * m / (sqrt(v) + eps)          lr_g = lr lr_scale
    p    = p (1 - wd lr_g) - u

Hyperparameters cross the C ABI as float: they are rounded to fp32 FIRST and used as doubles from there on, otherwise the
reference and the kernel differ by 3e-8 relative before any arithmetic happens.

Criteria (derived from the roundings of one step, not from what a kernel returned):

  p    delta = 8 * 2^-24 * (|p_old| + |u|) covers the fp32 roundings of decay_mul, step_size, lr * lr_scale, the quotient, sqrtf and
       the final subtraction, with or without FMA contraction.  The stored bf16 must lie in
       [bf16(ref - delta), bf16(ref + delta)] (round-to-nearest-even), for EVERY element.  The share of elements whose two ends
       differ (`two_valued`) must stay below TWO_VALUED_CAP: otherwise the interval would accept a neighbouring bf16 too often.
  m    |m - m64| <= 4 * 2^-24 * (|beta1 m_old| + |(1 - beta1) g'|) + 2^-126      (against the magnitudes: m cancels)
  v    |v - v64| <= 4 * 2^-24 * (|beta2 v_old| + |(1 - beta2) g'^2|) + 2^-126    (the floor takes flush-to-zero or gradual underflow)
  norm |s - s64| <= (ceil(n / 262144) + 32) * 2^-24 * s64: the sequential per-thread sum of n / 262144 non-negative terms
       (1024 workgroups x 256 threads), then the wave, block and final folds.

What the states and cases keep to, and why (reasoned from the criteria, checked with `emulate_fp32`, not fitted to a kernel):

  * delta charges the roundings of m to |p_old| + |u|.  m cancels (beta1 m_old against (1 - beta1) g'), and its rounding error,
    up to 4 * 2^-24 * (|beta1 m_old| + |(1 - beta1) g'|), reaches u as step_size * error / (sqrt(v) + eps) whatever is left of m.
    With Adam's own moments, m^2 <= v up to a factor near 1, that is at most ~6.5 * 2^-24 * step_size: inside delta where
    |p_old| >~ step_size, beyond it where |p_old| + |u| << step_size.  So later-step states are drawn with v = m^2 + U(0,1) g^2
    (a state with m^2 >> v, which Adam cannot reach, multiplies the error by |m| / sqrt(v)), and the cases that start from
    non-zero moments pair the parameter scale 1e-3 with lr <= 5e-4 or with gradients below eps.  The emulation at lr = 1e-2,
    parameters of 1e-3 and random moments leaves the interval by 1 ... 7 delta on one or two elements in 4M ... 8M: a limit of
    the criterion (bf16 parameters far smaller than the step are not a working point of the optimiser), not a finding about a
    kernel.
  * the clip coefficient multiplies every gradient and, squared, every (1 - beta2) g'^2: its error counts twice in v.  Formed in
    fp32 (sqrtf, + 1e-6f, the quotient, the product with grad_scale) it took v to 1.19 x its bound on the device and in the
    emulation; the kernels now form it in fp64 and round the scale once (clipped_grad_scale), which `emulate_fp32` mirrors.
    v under active clipping remains the tightest figure (0.94 of the bound measured)."""
import math

import torch

U32 = 2.0 ** -24            # fp32 unit roundoff
TINY = 2.0 ** -126          # smallest normal fp32
P_ULPS, M_ULPS = 8.0, 4.0
TWO_VALUED_CAP = 1e-3
STRIDE = 2048 * 256 * 8     # elements one grid stride of the AdamW kernels covers (ew_grid caps the grid at 2048 workgroups)
NORM_STRIDE = 1024 * 256 * 8  # the same for the sum of squares (1024 workgroups)
SIZES = (8, 2040, STRIDE + 8, 2 * STRIDE + 8 * 773)  # one vector; < one workgroup; first element of a 2nd stride; 2 strides + ragged
HYPER = ((1e-2, 0.9, 0.98, 1e-6, 0.05), (5e-4, 0.9, 0.98, 1e-6, 0.05), (2e-6, 0.9, 0.999, 1e-8, 0.0))  # lr, beta1, beta2, eps, wd

# (n, HYPER index, step, gradient scale, parameter scale): every value of every dimension, the two large sizes with the first two
# hyperparameter sets at steps 1 and 1000; the pairing of parameter scale 1e-3 with lr and step follows the note above.
STEP_CASES = (
    (SIZES[2], 0, 1, 1e-2, 1.0), (SIZES[2], 1, 1000, 30.0, 1e-3), (SIZES[2], 1, 1, 1e-6, 1.0), (SIZES[2], 0, 1000, 1e-2, 1.0),
    (SIZES[3], 0, 1, 1e-20, 1e-3), (SIZES[3], 1, 1000, 1e-2, 1.0), (SIZES[3], 1, 1, 30.0, 1e-3), (SIZES[3], 0, 1000, 1e-6, 1.0),
    (SIZES[2], 2, 10 ** 6, 1e-2, 1e-3),
    (8, 2, 2, 1e-2, 1.0), (8, 0, 1, 30.0, 1e-3), (8, 1, 10 ** 6, 1e-20, 1.0),
    (2040, 2, 10 ** 6, 1e-6, 1.0), (2040, 0, 2, 1e-20, 1e-3), (2040, 1, 10 ** 6, 30.0, 1.0), (2040, 2, 1000, 1e-2, 1e-3),
)


def step_case_id(c):
    return "n%d-hp%d-t%d-g%g-p%g" % c


def f32(x):
    """A hyperparameter as the C ABI (c_float) or a float device table passes it on: rounded to fp32, then widened to fp64."""
    if torch.is_tensor(x):
        return x.detach().to("cpu", torch.float32).double()
    return float(torch.tensor(float(x), dtype=torch.float32))


def bf16_rne(x):
    """fp64 -> the nearest bf16 value (ties to even, gradual underflow), returned as fp64.  One rounding: a cast through fp32
    would round twice.  Overflow is not modelled (no test gets near it)."""
    _, e = torch.frexp(x)                                       # |x| in [2^(e-1), 2^e)
    q = torch.ldexp(torch.ones_like(x), torch.clamp(e - 1, min=-126) - 7)
    return torch.round(x / q) * q                               # x / q is exact; torch.round rounds halves to even


def _quantum(x):
    _, e = torch.frexp(x)
    return torch.ldexp(torch.ones_like(x), torch.clamp(e - 1, min=-126) - 7)


def make_state(n, step, gscale, pscale, seed=0):
    """bf16 p and g, fp32 m and v.  Step 1 starts from zero moments; later steps from random ones, m signed and v >= 0 at the
    square of the gradient scale."""
    gen = torch.Generator().manual_seed(1000 * seed + 17)
    p = (torch.randn(n, generator=gen) * pscale).to(torch.bfloat16)
    g = (torch.randn(n, generator=gen) * gscale).to(torch.bfloat16)
    if step == 1:
        return p, g, torch.zeros(n), torch.zeros(n)
    m = torch.randn(n, generator=gen) * gscale
    v = m * m + torch.rand(n, generator=gen) * gscale * gscale
    return p, g, m, v


def sqnorm_fp64(g):
    return (g.detach().to("cpu", torch.float64) ** 2).sum()


def clip_coef_fp64(grad_scale, clip_norm, sqnorm):
    """min(1, clip_norm / (|grad_scale| sqrt(sqnorm) + 1e-6)) as an fp64 scalar tensor; a NaN norm gives NaN, +inf gives 0."""
    if not clip_norm > 0:
        return torch.ones((), dtype=torch.float64)
    norm = abs(f32(grad_scale)) * torch.as_tensor(sqnorm).detach().to("cpu", torch.float64).sqrt()
    return (f32(clip_norm) / (norm + 1e-6)).clamp(max=1.0)


def scaled_grad_fp64(g, grad_scale=1.0, clip_norm=0.0, sqnorm=None):
    """g' = g * grad_scale * clip coefficient.  sqnorm defaults to the fp64 sum of squares of g."""
    g = g.detach().to("cpu", torch.float64)
    if clip_norm > 0 and sqnorm is None:
        sqnorm = sqnorm_fp64(g)
    return g * (f32(grad_scale) * clip_coef_fp64(grad_scale, clip_norm, sqnorm))


def adamw_fp64(p, g, m, v, step, lr, beta1, beta2, eps, grad_scale=1.0, clip_norm=0.0, sqnorm=None, lr_scale=1.0,
               weight_decay=0.0):
    """One step in fp64: returns the new (p, m, v) and u, the update term.  lr_scale and weight_decay: scalars or per-element
    vectors (a group table expanded with `expand_groups`)."""
    p, m, v = (t.detach().to("cpu", torch.float64) for t in (p, m, v))
    lr, b1, b2, eps, lr_scale, wd = f32(lr), f32(beta1), f32(beta2), f32(eps), f32(lr_scale), f32(weight_decay)
    gp = scaled_grad_fp64(g, grad_scale, clip_norm, sqnorm)
    m = b1 * m + (1.0 - b1) * gp
    v = b2 * v + (1.0 - b2) * gp * gp
    lr_g = lr * lr_scale
    u = lr_g * (math.sqrt(1.0 - b2 ** step) / (1.0 - b1 ** step)) * (m / (v.sqrt() + eps))
    return p * (1.0 - wd * lr_g) - u, m, v, u


def expand_groups(counts, values):
    """A per-group table -> one value per element; counts are in 8-element vectors."""
    return torch.repeat_interleave(torch.as_tensor(values, dtype=torch.float32), torch.as_tensor(counts) * 8)


class Expected:
    """The fp64 result of one step from (p, g, m, v) and the acceptance intervals around it.  `check` marks the elements the
    criteria apply to (default: all); the others are for the caller to judge (a planted non-finite gradient)."""

    def __init__(self, p, g, m, v, step, lr, beta1, beta2, eps, grad_scale=1.0, clip_norm=0.0, sqnorm=None, lr_scale=1.0,
                 weight_decay=0.0, check=None):
        kw = dict(grad_scale=grad_scale, clip_norm=clip_norm, sqnorm=sqnorm)
        self.p, self.m, self.v, self.u = adamw_fp64(p, g, m, v, step, lr, beta1, beta2, eps, lr_scale=lr_scale,
                                                    weight_decay=weight_decay, **kw)
        p0, m0, v0 = (t.detach().to("cpu", torch.float64) for t in (p, m, v))
        gp = scaled_grad_fp64(g, **kw)
        b1, b2 = f32(beta1), f32(beta2)
        self.delta = P_ULPS * U32 * (p0.abs() + self.u.abs())
        self.lo, self.hi = bf16_rne(self.p - self.delta), bf16_rne(self.p + self.delta)
        self.m_bound = M_ULPS * U32 * ((b1 * m0).abs() + ((1.0 - b1) * gp).abs()) + TINY
        self.v_bound = M_ULPS * U32 * ((b2 * v0).abs() + (1.0 - b2) * gp * gp) + TINY
        self.check = torch.ones_like(self.p, dtype=torch.bool) if check is None else check.cpu()
        assert bool(torch.isfinite(self.p[self.check]).all()), "the reference itself is not finite where it is checked"
        self.two_valued = float((self.lo != self.hi)[self.check].double().mean())

    def figures(self, got_p, got_m, got_v):
        """Violation counts and, per quantity, the largest share of its budget a result uses: |got - ref| / bound for m and v; for
        p the multiple of delta that ref must move by to round to the stored bf16 (0 where bf16(ref) is what was stored)."""
        c = self.check
        gp_, gm, gv = (t.detach().to("cpu", torch.float64)[c] for t in (got_p, got_m, got_v))
        ref, delta = self.p[c], self.delta[c]
        bad_p = ~((gp_ >= self.lo[c]) & (gp_ <= self.hi[c]))   # a NaN is a violation
        s = torch.sign(ref - gp_)
        q = _quantum(gp_)
        half = gp_ + s * q / 2                                  # the neighbour towards ref: half a quantum below a power of two
        nb = torch.where(bf16_rne(half) == half, half, gp_ + s * q)
        excess = ((ref - (gp_ + nb) / 2) * s).clamp_min(0)
        p_used = torch.where(excess > 0, excess / delta, torch.zeros_like(excess))
        em, ev = (gm - self.m[c]).abs(), (gv - self.v[c]).abs()
        bad_m, bad_v = ~(em <= self.m_bound[c]), ~(ev <= self.v_bound[c])
        mx = lambda t: float(torch.nan_to_num(t, nan=math.inf).max()) if t.numel() else 0.0  # noqa: E731
        return {"p_bad": int(bad_p.sum()), "m_bad": int(bad_m.sum()), "v_bad": int(bad_v.sum()), "p_used": mx(p_used),
                "m_used": mx(em / self.m_bound[c]), "v_used": mx(ev / self.v_bound[c]), "two_valued": self.two_valued,
                "n": int(c.sum())}

    def assert_vacuity(self, what=""):
        assert self.two_valued < TWO_VALUED_CAP, "%s: %.2e of the intervals hold two bf16 values (cap %.0e)" % (
            what, self.two_valued, TWO_VALUED_CAP)

    def assert_p(self, got_p, what=""):
        self.assert_vacuity(what)
        z = torch.zeros_like(self.m)
        f = self.figures(got_p, z, z)
        assert f["p_bad"] == 0, "%s: %d of %d parameters outside [bf16(ref - delta), bf16(ref + delta)] (worst %.2f delta)" % (
            what, f["p_bad"], f["n"], f["p_used"])
        return f

    def assert_step(self, got_p, got_m, got_v, what=""):
        self.assert_vacuity(what)
        f = self.figures(got_p, got_m, got_v)
        assert f["p_bad"] == 0 and f["m_bad"] == 0 and f["v_bad"] == 0, (
            "%s: outside the criteria: p %d, m %d, v %d of %d elements (worst p %.2f delta, m %.2f, v %.2f of the bound)" % (
                what, f["p_bad"], f["m_bad"], f["v_bad"], f["n"], f["p_used"], f["m_used"], f["v_used"]))
        return f


def norm_bound(n):
    return (math.ceil(n / 262144) + 32) * U32


def norm_used(got_sq, g):
    """|got - s64| / (bound * s64) for the sum of squares of g."""
    ref = float(sqnorm_fp64(g))
    return abs(float(got_sq) - ref) / (norm_bound(g.numel()) * ref)


# ------------------------------------------------------------------------------------------------------------------
# fp32 emulation of the kernels' operation order (no FMA contraction), with planted errors
# ------------------------------------------------------------------------------------------------------------------
PLANTED = ("decay_after_update", "eps_inside_sqrt", "bias_of_previous_step", "clip_left_out")


def emulate_fp32(p, g, m, v, step, lr, beta1, beta2, eps, grad_scale=1.0, clip_norm=0.0, sqnorm=None, lr_scale=None,
                 weight_decay=0.0, planted=None):
    """What adamw_kernel computes without GROUPS (lr_scale None) or with it (lr_scale and weight_decay per element), in torch fp32 on the
    CPU: returns (p bf16, m, v).  sqnorm: an fp32 scalar as op_sqnorm leaves it (default: the fp64 sum rounded to fp32)."""
    F = lambda x: torch.tensor(x, dtype=torch.float32) if not torch.is_tensor(x) else x.float()  # noqa: E731
    lr, b1, b2, eps, gs = F(lr), F(beta1), F(beta2), F(eps), F(grad_scale)
    t = step - 1 if planted == "bias_of_previous_step" else step
    bc1, bc2 = 1.0 - float(b1.double()) ** t, 1.0 - float(b2.double()) ** t
    if lr_scale is None:
        step_size = F(float(lr.double()) * math.sqrt(bc2) / bc1)
        decay_mul = 1.0 - F(weight_decay) * lr
    else:
        lr_g = lr * F(lr_scale)
        step_size = lr_g * F(math.sqrt(bc2) / bc1)
        decay_mul = 1.0 - F(weight_decay) * lr_g
    if clip_norm > 0 and planted != "clip_left_out":
        sq = F(float(sqnorm_fp64(g))) if sqnorm is None else F(sqnorm).cpu()
        c = F(clip_norm).double() / (gs.double().abs() * sq.double().sqrt() + 1e-6)  # clipped_grad_scale: the coefficient in fp64,
        gs = (gs.double() * c).float() if bool(c < 1.0) or bool(c != c) else gs       # ONE rounding of the scale g is multiplied by
    gr = g.float() * gs
    m = m * b1 + (1.0 - b1) * gr
    v = v * b2 + (1.0 - b2) * gr * gr
    denom = (v + eps).sqrt() if planted == "eps_inside_sqrt" else v.sqrt() + eps
    pf = p.float()
    if planted == "decay_after_update":
        pf = (pf - step_size * (m / denom)) * decay_mul
    else:
        pf = pf * decay_mul - step_size * (m / denom)
    return pf.to(torch.bfloat16), m, v


# ------------------------------------------------------------------------------------------------------------------
# group tables (lists of vector counts) for adamw_kernel<GROUPS = true>
# ------------------------------------------------------------------------------------------------------------------
# boundaries mid-wave and mid-workgroup; one-vector groups first, in the middle and last; one group longer than a grid stride
# (524 288 vectors), so a thread's second vector lies in another group than its first, and for some threads in the same one
AWKWARD_GROUPS = (1, 1, 62, 64, 65, 255, 257, 1, 524288 + 3, 7, 300000, 1, 1)
# the maximum of 256 groups: runs of three one-vector groups between mixed sizes, one group of 400 000 vectors; > 524 288 in all
FULL_GROUPS = tuple(1 if k % 8 < 3 else (400000 if k == 100 else 37 + (k * 911) % 5000) for k in range(256))


def group_tables(n_groups, weight_decay=0.05):
    """lr scales 0.65^(k mod 12) and decay alternating on / off: two adjacent groups never share both values, so an off-by-one in
    the lookup changes every boundary vector.  (The exponent wraps so that the scales of a long table stay in fp32's range.)"""
    return [0.65 ** (k % 12) for k in range(n_groups)], [weight_decay if k % 2 == 0 else 0.0 for k in range(n_groups)]


def device_group_tables(counts, device="cuda"):
    """group_tables for a list of vector counts as the entries take them: (end8 int64, lr scale fp32, weight decay fp32) on `device`."""
    scale, wd = group_tables(len(counts))
    end8 = torch.cumsum(torch.tensor(counts, dtype=torch.int64), 0)
    return end8.to(device), torch.tensor(scale, dtype=torch.float32, device=device), torch.tensor(wd, dtype=torch.float32, device=device)


class TwoStrides(torch.nn.Module):
    """2 * STRIDE + 8 * 773 parameters: a decayed matrix of two grid strides and a vector without decay."""

    def __init__(self):
        super().__init__()
        gen = torch.Generator().manual_seed(7)
        self.mat = torch.nn.Parameter(torch.randn(2048, 4096, generator=gen))
        self.vec = torch.nn.Parameter(torch.randn(8 * 773, generator=gen))


# ------------------------------------------------------------------------------------------------------------------
# clipping: gradients whose scaled norm lands at a chosen place relative to the threshold
# ------------------------------------------------------------------------------------------------------------------
CLIP_NORM = 3.0
CLIP_AT = {"below": 0.05, "just_below": 1.0 - 5e-4, "just_above": 1.0 + 5e-4, "above": 40.0}  # |grad_scale| ||g|| / CLIP_NORM
GRAD_SCALES = (1.0, 0.25, -1.0 / 64)
# (n, grad_scale, where the norm lands, step): every pairing at n = 2040; at two strides + ragged every landing place and every scale
CLIP_CASES = tuple((SIZES[3],) + c for c in ((1.0, "below", 1), (0.25, "just_below", 1000), (-1.0 / 64, "just_above", 1),
                                             (0.25, "above", 1000), (1.0, "above", 1), (-1.0 / 64, "below", 1000))) + tuple(
    (2040, gs, at, (1, 1000)[(i + j) % 2]) for i, gs in enumerate(GRAD_SCALES) for j, at in enumerate(CLIP_AT))


def clip_case_id(c):
    return "n%d-gs%g-%s-t%d" % c


def make_clip_state(n, grad_scale, at, step, seed=0):
    """As make_state at parameter scale 1, with g scaled so that |grad_scale| ||g|| = CLIP_AT[at] * CLIP_NORM before its rounding to
    bf16 (which moves the norm by ~2^-9 / sqrt(n) relative: far less than the 5e-4 the near cases keep from the threshold), and
    moments at the scale of the clipped gradient."""
    gen = torch.Generator().manual_seed(1000 * seed + 29)
    p = torch.randn(n, generator=gen).to(torch.bfloat16)
    g = torch.randn(n, generator=gen, dtype=torch.float64)
    g = (g * (CLIP_AT[at] * CLIP_NORM / (abs(grad_scale) * float(g.norm())))).to(torch.bfloat16)
    if step == 1:
        return p, g, torch.zeros(n), torch.zeros(n)
    gscale = min(CLIP_AT[at], 1.0) * CLIP_NORM / math.sqrt(n)
    m = torch.randn(n, generator=gen) * gscale
    v = m * m + torch.rand(n, generator=gen) * gscale * gscale
    return p, g, m, v


def assert_clip_landing(g, grad_scale, at):
    """The reference's own check that a clip case is what its name says."""
    r = abs(f32(grad_scale)) * math.sqrt(float(sqnorm_fp64(g))) / CLIP_NORM
    ok = {"below": r < 0.1, "just_below": 1.0 - 1e-3 < r < 1.0, "just_above": 1.0 < r < 1.0 + 1e-3, "above": r > 10.0}[at]
    assert ok, "norm / clip_norm = %.6f is not '%s'" % (r, at)
    return r
