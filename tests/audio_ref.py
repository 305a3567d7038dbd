"""Shared by tests/test_audio_ref_cpu.py and tests/test_audio_fp64_gpu.py: the fused first block of the audio feature extractor
(csrc/audio.hip: op_audio_conv1_ln_gelu_fwd / _bwd, Conv1d(1 -> C, k = 10, stride) -> LayerNorm(C) -> GELU straight from the waveform) in
fp64, its per-element error budget, the seeded input families, the mirror of a_grid and the row walk, the case list, and an fp32
re-statement of both kernels (`emulate_conv1_*`) with its mutants.  Nothing here needs a GPU: every function runs on whatever device its
inputs live on.  bf, half_ulp_bf16, the exact GELU, the guarded buffers and the gate are those of tests/gemm_ref.py and tests/ln_ref.py.

Every input holds bf16 VALUES, so the reference and a kernel see the same numbers.

THE STORED CONVOLUTION OUTPUT  v = bf16(a)
The kernel DEFINES a as the fp32 chain  a = fma(w[c][j], s[j], a), j = 0 ... 9, from a = 0, then ONE fp32 addition of b0[c] (conv_row;
the build has no fast-math and the FMAs are explicit builtins, so the order is the source's).  conv_chain re-states that chain in fp64:
the product p of two bf16 numbers has 16 significant bits and is exact in fp64, and rounding fl64(a + p) to fp32 gives the fused
multiply-add BIT FOR BIT.  Proof that the two roundings act as one: if fl64(a + p) = a + p there is only one.  Otherwise a + p spans
more than 53 bits, so the smaller operand lies wholly below bit 53 - 24 = 29 of the larger one (a has 24 significant bits, p has 16):
|smaller| < 2^-29 |larger|.  The larger operand is an fp32 number (a 16-bit number is one too), fl64(a + p) lies within 2^-28 of it in
relative terms, and the nearest fp32 rounding midpoint lies 2^-25 away: fl64(a + p) is not a midpoint, and away from midpoints
rounding to 53 bits first cannot change the fp32 result.  The addition of b0 (8 bits) is the same case.  So v is part of the kernel's
documented arithmetic, not a fit, and the statistics are gated GIVEN v.  tests/test_audio_ref_cpu.py checks the chain's soundness: it lies
within  E_a = (10 + [bias]) u (sum_j |w_j s_j| + |b0|)  of the exact convolution, and bf(chain) = bf(exact) wherever the exact value is
farther than E_a from a bf16 rounding midpoint.  In the `exact` family (small dyadic inputs) every operation of the chain is exact:
there v = bf(exact convolution) without any chain, which proves the convolution independently of the order of its terms.

THE BUDGET (u = 2^-24; derived from the kernels' operation counts, nothing is fitted to what a kernel returned)
Forward: given v, mean / rstd / y take ln_ref.fwd_budget(v, lnw, lnb, eps, gelu=True).  This kernel sums a row with 8 sequential
additions per lane and 6 butterfly levels, no LDS stage (inactive lanes of C <= 504 add exact zeros): depth 14; ln_ref.depth(C) = 15 is
used as it is, one more than needed.  mean and rstd are gated as the fp32 numbers they are.  `exact` family: mean must EQUAL its exact
value where C is a power of two (1 / C and the integer sums are exact; at other C within E_mean).  rstd and y keep fwd_budget there:
rsqrtf is inexact on every input and the centred squares need 31 bits, so a gate of "R and the GELU term only" is not attainable.

Backward (mean, rstd are INPUTS, given to the reference as they are): dx, dlnw, dlnb take ln_ref.bwd_budget(..., gelu=True) with the
depth of the row sums replaced by this kernel's:
    grid = min(1024, ceil(rows / 4)),  trips = ceil(rows / (4 grid)),  Dw = trips + 3 + ceil(grid / 8) + 8
(register accumulation, three LDS additions, partials_reduce*).  The kernel rounds dx to bf16 before it enters dW0 / db0; the reference
uses q = bf(dx_exact) and, as ln_ref.geglu_product does, E_q = one bf16 ulp at |dx| + E_dx where dx_exact lies within E_dx of a rounding
midpoint (the device may round to the other neighbour), 0 elsewhere.
    E_dW0[c][j] = (Dw + 1) u sum_r |q s_rj| + sum_r E_q |s_rj|,     E_db0[c] = Dw u sum_r |q| + sum_r E_q
plus u |exact + base| for the fold; the gate adds the ONE bf16 rounding R of the output: |got - exact| <= R + E per element, reported as
the share |err| / (R + E) and, after the slash, (|err| - R) / E.
Two CONDITIONS keep the near-midpoint allowance from hiding a failure (asserted on the CPU): (1) in every family without non-finite
values at most 5 % of the dx elements carry E_q != 0; (2) over the elements of dW0 the median of (largest single-row term |q s|) /
(R + E) is at least 8 -- one missing row lies far above the gate.

MEASURED on the MI355X (profiles/audio_fp64_errors_mi355x.txt, one line per case of tests/test_audio_fp64_gpu.py; 166 cases, all
inside the gate, guards intact, both launches of every case bit-identical).  Largest share / largest part of E used, per output:
y 1.00 / 0.28, mean 0.10 / 0.05, rstd 0.23 / 0.18, dW0 1.00 / 0.85 (a launch of one row, where a sum is one term and E is E_q alone),
db0 1.00 / 0.69, dlnw 1.00 / 0.01, dlnb 1.00 / 0.01.  (A bf16 output's share is close to 1 wherever the exact value lies close to a
rounding midpoint; the second figure is what the kernel uses of the fp32 allowance.)  RECORD below holds the same figures.
"""
import torch

from tests import ln_ref
from tests.gemm_ref import C_GELU, SENTINEL, bf, cdiv, check_guard, gelu_erf, gelu_erf_grad, guarded, guarded_from, half_ulp_bf16  # noqa: F401
from tests.ln_ref import BF, F32, U, _affine, _gelu32, _gelu_grad32, gate  # noqa: F401

# RECORD: the largest share / the largest part of E used, per output, over the cases of profiles/audio_fp64_errors_mi355x.txt
RECORD = {"y": (1.0, 0.28), "mean": (0.1, 0.05), "rstd": (0.23, 0.18), "dW0": (1.0, 0.85), "db0": (1.0, 0.69), "dlnw": (1.0, 0.01),
          "dlnb": (1.0, 0.01)}     # (tests/test_audio_ref_cpu.py compares it with the committed record)

AK = 10
A_MAX_BLOCKS = 1024


# ----------------------------------------------------------------------------------------------------------------------
# MIRROR of csrc/audio.hip: a_grid and the persistent row walk (a wave per row, four rows per workgroup, stride 4 grid)
# ----------------------------------------------------------------------------------------------------------------------
def a_grid(rows):
    return max(1, min(A_MAX_BLOCKS, cdiv(rows, 4)))


def trips(rows):
    return cdiv(rows, 4 * a_grid(rows))


def wgrad_depth(rows):
    return trips(rows) + 3 + cdiv(a_grid(rows), 8) + 8


def wav_len(rows, stride):
    return stride * (rows - 1) + AK


def patches(wav, rows, stride):
    """[rows, 10]: row r holds wav[stride r ... stride r + 9]."""
    return wav.unfold(0, AK, stride)[:rows]


# ----------------------------------------------------------------------------------------------------------------------
# closed forms in fp64
# ----------------------------------------------------------------------------------------------------------------------
def conv_chain(S, w0, b0):
    """The kernel's fp32 chain re-stated in fp64 (module docstring).  S [rows, 10], w0 [C, 10], b0 [C] | None, fp64 tensors holding bf16
    values.  Returns the fp32 number a as fp64."""
    a = torch.zeros(S.shape[0], w0.shape[0], dtype=torch.float64, device=S.device)
    for j in range(AK):
        a = (a + S[:, j, None] * w0[None, :, j]).float().double()
    if b0 is not None:
        a = (a + b0).float().double()
    return a


def conv_exact(S, w0, b0):
    """(exact convolution, E_a)."""
    ex, T = S @ w0.t(), S.abs() @ w0.abs().t()
    if b0 is not None:
        ex, T = ex + b0, T + b0.abs()
    return ex, (AK + (b0 is not None)) * U * T


def fwd_ref(wav, w0, b0, lnw, lnb, rows, stride, eps, chain=True):
    """dict: S, v, y, mean, rstd and the budgets E_y, E_mean, E_rstd.  chain=False (`exact` family): v = bf(exact convolution)."""
    S = patches(wav, rows, stride)
    v = bf(conv_chain(S, w0, b0) if chain else conv_exact(S, w0, b0)[0])
    y, mean, rstd = ln_ref.ln_fwd_ref(v, lnw, lnb, eps, True)
    e_y, e_mean, e_rstd = ln_ref.fwd_budget(v, lnw, lnb, eps, True)
    return dict(S=S, v=v, y=y, mean=mean, rstd=rstd, E_y=e_y, E_mean=e_mean, E_rstd=e_rstd)


def dx_rounded(dx, e_dx):
    """(q = bf(dx), E_q)."""
    q = bf(dx)
    near = (half_ulp_bf16(dx) - (dx - q).abs()) <= e_dx
    return q, torch.where(near & (dx != 0), 2 * half_ulp_bf16(dx.abs() + e_dx), torch.zeros_like(dx))


def bwd_ref(dy, S, v, lnw, lnb, mean, rstd, bias, base=None):
    """name -> (exact, E) for dW0 [C, 10], db0 (with bias), dlnw, dlnb, and "dx" -> (dx, E_dx, q, E_q).  base: dict name -> tensor when
    accumulating."""
    rows = v.shape[0]
    Dw = wgrad_depth(rows)
    lbase = None if base is None else (base["dlnw"], base["dlnb"])
    _, dlw, dlb = ln_ref.ln_bwd_ref(dy, v, lnw, lnb, mean, rstd, True, base=lbase)
    e_dx, e_dlw, e_dlb, (dx, _) = ln_ref.bwd_budget("bwd", dy, v, lnw, lnb, mean, rstd, True, base=lbase, dw_depth=Dw)
    q, e_q = dx_rounded(dx, e_dx)
    Sa = S.abs()
    dw, e_dw = q.t() @ S, (Dw + 1) * U * (q.abs().t() @ Sa) + e_q.t() @ Sa
    db, e_db = q.sum(0), Dw * U * q.abs().sum(0) + e_q.sum(0)
    if base is not None:
        dw, db = dw + base["dW0"], db + base["db0"]
    out = {"dW0": (dw, e_dw + U * dw.abs()), "dlnw": (dlw, e_dlw), "dlnb": (dlb, e_dlb), "dx": (dx, e_dx, q, e_q)}
    if bias:
        out["db0"] = (db, e_db + U * db.abs())
    return out


def single_row_ratio(ref, S):
    """Condition 2: per element of dW0 the largest single-row term |q s| over R + E."""
    dw, e_dw = ref["dW0"]
    q = ref["dx"][2]
    big = (q.abs()[:, :, None] * S.abs()[:, None, :]).amax(0)
    return big / (half_ulp_bf16(dw.abs() + e_dw) + e_dw)


# ----------------------------------------------------------------------------------------------------------------------
# input families
# ----------------------------------------------------------------------------------------------------------------------
FAMILIES = ("unit", "offset", "silence", "wide", "exact", "nonfinite")
AFFINE = ("both", "none", "lnb_null", "dlnb_null")     # lnw / lnb both given | both null | lnb null alone | both given, dlnb not asked for
OUTPUTS = ("dW0", "db0", "dlnw", "dlnb")


def _b(t):
    return t.to(BF).float()


class Inputs:
    """wav [stride (rows - 1) + 10], w0 [C, 10], b0, lnw, lnb [C] | None, dy [rows, C], base: name -> tensor (the accumulation targets'
    contents); fp32 CPU tensors holding bf16 values."""


def make_inputs(family, rows, C, stride=5, bias=True, affine="both", seed=0):
    """unit: N(0, 1) waveform, w0 = 0.4 N, b0 = 0.1 N, lnw = 1 + 0.1 N, lnb = 0.1 N, dy = N(0, 1).
    offset: the waveform is 4 + 1.5 N (its spread about 50 bf16 ulps of the DC part) and the channels share the tap vector 0.3, so that a
    row's channel mean is about 50 times its channel spread: the cancellation case of the statistics.
    silence: a quarter of the waveform from its middle, and its last eighth, are zero (a sample's padded tail, a silent sample).
    wide: blocks of 8 rows scaled by 2^-10 ... 2^10.  exact: small integers and powers of two (every fp32 operation of the chain, of the
    row sum and of the mean is exact).  nonfinite: one NaN at a third and one +-inf at two thirds of the waveform."""
    g = torch.Generator().manual_seed(9000 + 1000 * FAMILIES.index(family) + seed)
    n = wav_len(rows, stride)
    r = Inputs()
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    ri = lambda *s: torch.randint(-2, 3, s, generator=g).float()  # noqa: E731
    wav, w0, b0, lnw, lnb, dy = rn(n), 0.4 * rn(C, AK), 0.1 * rn(C), 1 + 0.1 * rn(C), 0.1 * rn(C), rn(rows, C)
    base = {"dW0": rn(C, AK), "db0": rn(C), "dlnw": rn(C), "dlnb": rn(C)}
    if family == "offset":
        wav, w0 = 4 + 1.5 * wav, 0.3 + 0.05 * w0
    elif family == "silence":
        wav[n // 2:n // 2 + n // 4] = 0
        wav[n - n // 8 - AK:] = 0
    elif family == "wide":
        wav = torch.ldexp(wav, (torch.arange(n) // (8 * stride)) % 21 - 10)
    elif family == "exact":
        wav, w0, b0, lnb, dy = ri(n), ri(C, AK), ri(C), 0.5 * ri(C), ri(rows, C)
        lnw = torch.ldexp(torch.ones(C), torch.randint(-1, 2, (C,), generator=g)) * (1 - 2 * torch.randint(0, 2, (C,), generator=g)).float()
        base = {k: ri(*v.shape) for k, v in base.items()}
    elif family == "nonfinite":
        wav[n // 3] = float("nan")
        wav[(2 * n) // 3] = float("inf") if seed % 2 == 0 else -float("inf")
    elif family != "unit":
        raise ValueError(family)
    r.wav, r.w0, r.dy = _b(wav), _b(w0), _b(dy)
    r.b0 = _b(b0) if bias else None
    r.lnw = _b(lnw) if affine != "none" else None
    r.lnb = _b(lnb) if affine in ("both", "dlnb_null") else None
    r.base = {k: _b(v) for k, v in base.items()}
    r.rows, r.C, r.stride, r.wants = rows, C, stride, wanted(bias, affine)
    return r


def wanted(bias, affine):
    """The gradients a launch asks for (dW0 always)."""
    return tuple(k for k, on in (("dW0", True), ("db0", bias), ("dlnw", affine != "none"), ("dlnb", affine == "both")) if on)


def to64(v, device=None):
    if isinstance(v, dict):
        return {k: to64(x, device) for k, x in v.items()}
    return None if v is None else v.to(device or v.device).double()


def silent_rows(S):
    return (S == 0).all(1)


def touched_rows(S):
    """Rows that read a non-finite waveform sample."""
    return ~torch.isfinite(S).all(1)


# ----------------------------------------------------------------------------------------------------------------------
# fp32 re-statements of the kernels (CPU: they show the budget attainable, and their mutants show the gates sharp)
# ----------------------------------------------------------------------------------------------------------------------
MUTANTS = {   # name -> (the kernels it changes, the family whose gate must catch it, rows, C)
    "conv_unrounded": ("fwd", "unit", 4100, 64),             # the convolution output is not rounded to bf16 before the statistics
    "taps_reversed": ("fwd", "unit", 4100, 64),
    "bias_ignored": ("fwd", "unit", 4100, 64),
    "var_one_pass": ("fwd", "offset", 4100, 64),             # E[x^2] - mean^2
    "rows_past_grid_skipped": ("fwd bwd", "unit", 4100, 64),  # `row += gridDim.x * 4` never taken
    "dy_of_next_trip": ("bwd", "unit", 4100, 64),            # cur = nxt one trip early
    "dx_without_m2": ("bwd", "unit", 4100, 64),              # the xhat m2 term dropped
    "dx_unrounded": ("bwd", "exact", 4100, 64),
    "dw_transposed": ("bwd", "unit", 4100, 64),              # dW0 written as [10][C]
    "fourth_wave_left_out": ("bwd", "unit", 4100, 64),       # the LDS fold adds three of the four waves
    "accumulate_ignored": ("bwd", "unit", 4100, 64),
    "lane0_params": ("fwd bwd", "unit", 1030, 264),          # channels from 8 * 32 upwards read lane 0's parameters
}


def _params32(r, mutant):
    C = r.w0.shape[0]
    idx = torch.arange(C)
    if mutant == "lane0_params":
        idx = torch.where(idx >= 256, idx % 8, idx)
    pick = lambda t: None if t is None else t.float()[idx]  # noqa: E731
    w0 = pick(r.w0)
    if mutant == "taps_reversed":
        w0 = w0.flip(1)
    lnw, lnb = _affine(pick(r.lnw), pick(r.lnb), C, w0)
    return w0, (None if mutant == "bias_ignored" else pick(r.b0)), lnw, lnb


def _v32(r, mutant):
    w0, b0, lnw, lnb = _params32(r, mutant)
    S = patches(r.wav.float(), r.rows, r.stride)
    a = conv_chain(S.double(), w0.double(), None if b0 is None else b0.double()).float()     # (the fp32 FMA chain: conv_chain's docstring)
    return S, (a if mutant == "conv_unrounded" else a.to(BF).float()), lnw, lnb


def emulate_conv1_fwd(r, eps, mutant=None):
    """r: Inputs.  Returns y (bf16), mean, rstd (fp32)."""
    S, v, lnw, lnb = _v32(r, mutant)
    mean, d, rstd = ln_ref._stats32(v, eps, mutant if mutant == "var_one_pass" else None)
    y = _gelu32(d * rstd[:, None] * lnw + lnb, None).to(BF)
    if mutant == "rows_past_grid_skipped":
        k = 4 * a_grid(r.rows)
        y[k:], mean[k:], rstd[k:] = 0, 0, 0
    return y, mean, rstd


def emulate_conv1_bwd(r, mean, rstd, accumulate=False, mutant=None):
    """mean, rstd: fp32 [rows].  Returns name -> bf16 tensor for the gradients r.wants."""
    S, v, lnw, lnb = _v32(r, mutant)
    rows, C = v.shape
    dy, rstep = r.dy.float(), 4 * a_grid(rows)
    if mutant == "dy_of_next_trip" and rows > rstep:
        dy = dy.clone()
        dy[:rows - rstep] = r.dy[rstep:]
    xh = (v - mean[:, None]) * rstd[:, None]
    g = dy * _gelu_grad32(xh * lnw + lnb, None)
    gw = g * lnw
    inv = torch.tensor(1.0, dtype=F32) / C
    m1, m2 = gw.sum(1, keepdim=True) * inv, (gw * xh).sum(1, keepdim=True) * inv
    if mutant == "dx_without_m2":
        m2 = 0 * m2
    dx = rstd[:, None] * (gw - m1 - xh * m2)
    if mutant != "dx_unrounded":
        dx = dx.to(BF).float()
    keep = torch.ones(rows, dtype=torch.bool)
    if mutant == "rows_past_grid_skipped":
        keep[rstep:] = False
    if mutant == "fourth_wave_left_out":
        keep[3::4] = False
    g, xh, dx, S = g[keep], xh[keep], dx[keep], S[keep]
    out = {"dW0": dx.t() @ S, "db0": dx.sum(0), "dlnw": (g * xh).sum(0), "dlnb": g.sum(0)}
    if mutant == "dw_transposed":
        out["dW0"] = out["dW0"].t().contiguous().view(C, AK)
    if accumulate and mutant != "accumulate_ignored":
        out = {k: t + r.base[k] for k, t in out.items()}
    return {k: out[k].to(BF) for k in r.wants}


# ----------------------------------------------------------------------------------------------------------------------
# the cases of the GPU test
# ----------------------------------------------------------------------------------------------------------------------
ROWS = (1, 3, 5, 4096, 4097, 8195)     # one partial workgroup, ... , exactly one trip, one wave with two trips, some waves with three
CS = (8, 64, 264, 504, 512)            # one active lane, ..., 33 and 63 active lanes, all 64
STRIDES = (5, 1, 16)
EPS = 1e-5


class AudioCase:
    def __init__(self, family, rows, C, stride, bias, affine, accumulate, chained=False):
        self.family, self.rows, self.C, self.stride, self.bias, self.affine, self.accumulate = family, rows, C, stride, bias, affine, accumulate
        self.chained = chained     # the backward runs on the forward kernel's own statistics
        self.id = "%s%s-%dx%d-s%d-b%d-%s-acc%d" % ("chained-" if chained else "", family, rows, C, stride, bias, affine, accumulate)

    def inputs(self):
        return make_inputs(self.family, self.rows, self.C, self.stride, self.bias, self.affine)


def _cases():
    c = []
    for ri, rows in enumerate(ROWS):
        for ci, C in enumerate(CS):
            for fi, family in enumerate(FAMILIES):
                if rows < 5 and family in ("silence", "nonfinite"):     # (no whole silent row; a sample would touch one row only)
                    continue
                stride = 5 if family == "nonfinite" else STRIDES[(ri + ci + fi) % 3]
                t = 7 * (5 * ri + ci) + 3 * fi     # (walks the 16 argument combinations; the CPU test checks that all of them occur)
                c.append(AudioCase(family, rows, C, stride, t % 2 == 0, AFFINE[(t // 2) % 4], (t // 8) % 2))
    for fi, family in enumerate(FAMILIES):
        c.append(AudioCase(family, 4097, CS[1 + fi % 4], 5, fi % 2 == 0, AFFINE[fi % 2], fi % 2, chained=True))
    ids = [x.id for x in c]
    assert len(set(ids)) == len(ids), [k for k in ids if ids.count(k) > 1][:3]
    return c


CASES = _cases()
