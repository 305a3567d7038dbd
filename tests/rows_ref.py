"""Shared by tests/test_rows_ref_cpu.py and tests/test_rows_fp64_gpu.py: the row-wise backward kernels of csrc/elementwise.hip in
closed-form fp64 -- op_colsum, op_colsum_segments, op_resid_bwd, op_gamma_grad_finish, op_scale_rows, op_geglu_bwd and
op_transpose_scaled / op_transpose_batched -- the per-element error budget, the seeded input families, the mirror of the dispatch,
the case lists, and an fp32 re-statement of every kernel (`emulate_*`) with its mutants.  Nothing here needs a GPU: every function
runs on whatever device its inputs live on.  bf, half_ulp_bf16, the exact GELU, C_GELU, make_vec and the guarded buffers are those of
tests/gemm_ref.py; the gate's arithmetic and gather_rows are those of tests/ln_ref.py.

Every input holds bf16 VALUES (rowscale, rowdot and g0 hold fp32 values), so the reference and a kernel see the same numbers.

THE BUDGET (derived from the kernels' operation counts; u = 2^-24; nothing below is fitted to what a kernel returned)

Column sums (op_colsum, op_colsum_segments, dgamma / dbias / g0 of op_resid_bwd).  A wave adds its rows one after the other
(rows per wave = ceil(M / (4 parts)) additions), the four waves of a workgroup meet in LDS (3 additions), the fold adds the `parts`
partials in 8 groups (ceil(parts / 8) additions each) and the 8 groups one after the other (8 additions).  A term of the sum passes
through at most
      D = rows per wave + 3 + ceil(parts / 8) + 8
additions.  One rounding more per product that formed the term (s x y: 2; s x or x y: 1; none for the plain sum), one for `* mul`
(gamma in the dbias fold), one for `+ base` (accumulate):
      E = (D + those) u T,      T = |mul| sum|term| + |base|
and the output's ONE rounding R: half a bf16 ulp at |exact| + E for a bf16 output, u |exact| for an fp32 one (g0, fp32 colsum).
(`a += s * x * y` may be contracted into a fused multiply-add: one rounding fewer, never one more.)

op_gamma_grad_finish.  Wave w adds the slots w, w + 4, ... in four chains while 16 more slots are left and in one chain after that
(finish_chains: the mirror); the chains meet as (a0 + a1) + (a2 + a3), the four waves likewise: D = longest chain + 2 + 2.  Every pair
adds one product b g0 and its addition (2), accumulate one more:
      E = (D + 2 pairs + [accumulate]) u T,      T = sum|rowdot| + sum|b g0| + |base|

dbranch / op_scale_rows.  E = 2 u |exact|: rs * dout * gamma is two fp32 products (one with g0 or without gamma).  This is NOT bit
equality with bf16(fp32 product) computed another way: rowscale is a full fp32 number, so the product is rounded twice, in an order
the kernels do not share (resid_bwd: (rs dout) gamma; scale_rows: dout (rs gamma)).

op_geglu_bwd.  The two lines at the end of tests/ln_ref.py's docstring with E_dg = 0 (dg is an input here):
      E_dh0 = |dg h1| (C_GELU + 2) u max(1, |gelu'(h0)|) + 2 u |dh0|
      E_dh1 = |dg| C_GELU u |h0| + 2 u |dh1|
C_GELU is the project's constant of tests/gemm_ref.py.  In the far negative tail the error of gelu_parts is RELATIVE (tests/ln_ref.py:
1.2 % at h0 = -8.6) and far inside these ABSOLUTE bounds.  At h0 = +-3e38 the kernel forms dg * h0 before it multiplies by Phi: the
`sweep` family keeps |dg| <= 1 so that this intermediate stays inside fp32, as every gradient that can meet such an h0 would have to.

Transposes.  No budget.  The unscaled transpose moves bits; the scaled one rounds an EXACT product of two bf16 numbers once, so the
result must equal bf(scale * in) bit for bit.

Underflow.  The `wide` family with gamma = 1e-30 takes rs * dout * gamma below 2^-126.  fp32 and bf16 keep subnormals (gradual
underflow: an absolute error below 2^-149 per operation, against R >= 2^-134), so no term is added for it.

THE GATE is |got - exact| <= R + E per element; the figure reported is the SHARE |got - exact| / (R + E), which must stay <= 1; got
is non-finite exactly where exact is.  In the `integer` family every fp32 operation is exact: E is taken as 0 there (the share is
against R alone) and fp32 outputs must be equal.

MEASURED on the MI355X (profiles/rows_fp64_errors_mi355x.txt, one line per case of tests/test_rows_fp64_gpu.py, 714 cases, all inside
the gate).  Largest share |err| / (R + E) and, after the slash, largest (|err| - R) / E per output: colsum 1.00 / 0.12 (the share is 1 only
on the `integer` family, where E = 0 and a sum lands on a rounding tie); colsum_segments 1.00 / 0; resid_bwd dbranch 1.00 / 0.78,
dgamma 1.00 / 0.06, dbias 1.00 / 0.08, g0 (fp32) 0.16 / 0.13; gamma_grad_finish 1.00 / 0; scale_rows 1.00 / 0.69; geglu_bwd dh0 1.00 /
0.42, dh1 1.00 / 0.33; the transposes bit for bit.  A bf16 output's share is close to 1 wherever the exact value lies close to a
rounding midpoint; the second figure is what the kernels use of the fp32 allowance beyond that rounding."""
import torch

from tests.gemm_ref import (C_GELU, SENTINEL, bf, cdiv, check_guard, gelu_erf, gelu_erf_grad, guarded, guarded_from,  # noqa: F401
                            half_ulp_bf16, make_vec)
from tests.ln_ref import BF, F32, U, _gelu32, _gelu_grad32, gather_rows
from tests.ln_ref import gate as _gate

FAMILIES = ("unit", "offset", "cancel", "wide", "integer", "dropped", "nonfinite")
GEGLU_FAMILIES = ("sweep", "nonfinite")


# ----------------------------------------------------------------------------------------------------------------------
# the mirror of the dispatch
# ----------------------------------------------------------------------------------------------------------------------
# MIRROR of csrc/elementwise.hip: CS_MAX_PARTS and the `parts` clamp of op_colsum / op_resid_bwd / op_colsum_segments; the row walk of
# colsum_partial_kernel / resid_bwd_kernel (m0 = blockIdx.y * 4 + wid, step = gridDim.y * 4); ew_grid; the slot loop of
# gamma_grad_finish_kernel; and of csrc/common.h: partials_reduce_kernel / partials_reduce3_kernel (8 groups, then 8 additions).
CS_MAX_PARTS = 256


def cs_parts(M):
    return max(1, min(CS_MAX_PARTS, cdiv(M, 64)))


def cs_rows_per_wave(M):
    return cdiv(M, 4 * cs_parts(M))


def cs_depth(M):
    parts = cs_parts(M)
    return cs_rows_per_wave(M) + 3 + cdiv(parts, 8) + 8


def ew_grid(items):
    return max(1, min(2048, cdiv(items, 256)))


def ew_trips(items):
    return cdiv(items, 256 * ew_grid(items))


def finish_chains(slots):
    """Per wave w: (the four chains of slot indices a0 ... a3, the slots among a0 that the tail loop adds)."""
    out = []
    for w in range(4):
        a, tail, s = [[], [], [], []], [], w
        while s + 12 < slots:
            for i in range(4):
                a[i].append(s + 4 * i)
            s += 16
        while s < slots:
            a[0].append(s)
            tail.append(s)
            s += 4
        out.append((a, tail))
    return out


def finish_depth(slots):
    return max(len(c) for a, _ in finish_chains(slots) for c in a) + 2 + 2


def route_cs(M, N):
    return "parts=%d rpw=%d cb=%d" % (cs_parts(M), cs_rows_per_wave(M), cdiv(N, 512))


# ----------------------------------------------------------------------------------------------------------------------
# closed forms in fp64 (no autograd); every one returns (exact, E)
# ----------------------------------------------------------------------------------------------------------------------
def row_scale(rowscale, rps, M, like):
    """[M, 1]: rowscale[m // rps], or ones."""
    if rowscale is None:
        return torch.ones(M, 1, dtype=like.dtype, device=like.device)
    return rowscale.to(like.dtype).repeat_interleave(rps)[:M, None]


def _sum_budget(terms, nround, M, mul, base, exact_E=True):
    S, A = terms.sum(0), terms.abs().sum(0)
    k = cs_depth(M) + nround
    if mul is not None:
        S, A, k = S * mul, A * mul.abs(), k + 1
    if base is not None:
        S, A, k = S + base, A + base.abs(), k + 1
    return S, (k * U * A if exact_E else torch.zeros_like(A))


def colsum_ref(x, y=None, rowscale=None, rps=1, mul=None, base=None, budget=True):
    """out[n] = base[n] + mul[n] sum_m rowscale[m // rps] x[m][n] y[m][n]  ->  (exact, E).  budget=False (the `integer` family): E = 0."""
    t, k = x, 0
    if rowscale is not None:
        t, k = t * row_scale(rowscale, rps, x.shape[0], x), k + 1
    if y is not None:
        t, k = t * y, k + 1
    return _sum_budget(t, k, x.shape[0], mul, base, budget)


def colsum_segments_ref(x, n_seg, seg_cols, bases=None, budget=True):
    """[(exact, E)] per segment of x [M, n_seg seg_cols]; bases: per segment a base or None."""
    return [_sum_budget(x[:, i * seg_cols:(i + 1) * seg_cols], 0, x.shape[0], None, None if bases is None else bases[i], budget) for i in range(n_seg)]


def resid_bwd_ref(dout, y=None, gamma=None, rowscale=None, rps=1, dgamma=False, dbias=False, g0=False, base=None, dout_rows=None, budget=True):
    """The gradient of out = resid + rowscale[m // rps] gamma[n] y[m][n]: a dict of (exact, E) for dbranch and the sums asked for.
    With g0, dbranch carries no gamma.  base = (dgamma base, dbias base) when accumulating.  dout_rows: row m of the pass is row
    dout_rows[m] of dout, a row of zeros where negative."""
    d = gather_rows(dout, dout_rows)
    M = d.shape[0]
    t = d * row_scale(rowscale, rps, M, d)
    k = 0 if rowscale is None else 1
    br = t if (gamma is None or g0) else t * gamma
    out = {"dbranch": (br, (2 * U * br.abs() if budget else torch.zeros_like(br)))}
    if dgamma:
        out["dgamma"] = _sum_budget(t * y, k + 1, M, None, None if base is None else base[0], budget)
    if dbias:
        out["dbias"] = _sum_budget(t, k, M, gamma, None if base is None else base[1], budget)
    if g0:
        out["g0"] = _sum_budget(t, k, M, None, None, budget)
    return out


def gamma_grad_finish_ref(rowdot, pairs, base=None, budget=True):
    """dgamma[n] = base[n] + sum_s rowdot[s][n] + sum_i b_i[n] g0_i[n]; a pair with a null bias adds nothing."""
    S, A = rowdot.sum(0), rowdot.abs().sum(0)
    k = finish_depth(rowdot.shape[0]) + 2 * len(pairs)
    for b, g in pairs:
        if b is not None:
            S, A = S + b * g, A + (b * g).abs()
    if base is not None:
        S, A, k = S + base, A + base.abs(), k + 1
    return S, (k * U * A if budget else torch.zeros_like(A))


def scale_rows_ref(dout, gamma=None, rowscale=None, rps=1, budget=True):
    e = dout * row_scale(rowscale, rps, dout.shape[0], dout)
    if gamma is not None:
        e = e * gamma
    return e, (2 * U * e.abs() if budget else torch.zeros_like(e))


def geglu_bwd_ref(dg, h0, h1):
    """((dh0, E), (dh1, E)) of g = gelu(h0) h1."""
    gp, ge = gelu_erf_grad(h0), gelu_erf(h0)
    dh0, dh1 = dg * h1 * gp, dg * ge
    e0 = (dg * h1).abs() * (C_GELU + 2) * U * gp.abs().clamp_min(1.0) + 2 * U * dh0.abs()
    e1 = dg.abs() * C_GELU * U * h0.abs() + 2 * U * dh1.abs()
    return (dh0, e0), (dh1, e1)


def transpose_ref(x, scale=None):
    """out[c][r] = bf(scale[r] x[r][c]) as a bf16 tensor (bits are compared)."""
    x = x.double()
    if scale is not None:
        x = bf(x * scale.double()[:, None])
    return x.t().contiguous().to(BF)


def gate(got, exact, E, rounding, what):
    """(failures, largest share |err| / (R + E), largest (|err| - R) / E: what of the fp32 allowance is used beyond the output's rounding).
    The arithmetic is tests/ln_ref.gate's; on top of it got must be non-finite exactly where exact is."""
    fails, share, over = _gate(got, exact, E, rounding, what)
    wrong = torch.isfinite(exact) != torch.isfinite(got.double())
    if bool(wrong.any()):
        i = tuple(wrong.nonzero()[0].tolist())
        fails.append("%s%s: got %r where exact is %r (%d elements differ in finiteness)" % (what, list(i), float(got[i]), float(exact[i]), int(wrong.sum())))
    return fails, share, over


# ----------------------------------------------------------------------------------------------------------------------
# input families (CPU, seeded; fp32 tensors holding bf16 values unless said otherwise)
# ----------------------------------------------------------------------------------------------------------------------
def _gen(family, seed):
    return torch.Generator().manual_seed(31000 + 1000 * (FAMILIES + GEGLU_FAMILIES).index(family) + seed)


def _b(t):
    return t.to(BF).float()


def neg_entries(M):
    """The entries of a row table that are negative in every family: the first and last row of the pass and the rows on both sides of
    every step boundary of the row walk (step = 4 parts)."""
    step = 4 * cs_parts(M)
    return sorted({0, M - 1} | {r for b in range(step, M, step) for r in (b - 1, b)})


def make_gamma(family, N, seed=0):
    """bf16 [N]: 0.1 ... 1.1, every fifth negative; 0, 1e-6, 1e-30 in front (not in `integer`: +-(0.5, 1, 2)); `wide`: columns scaled by
    powers of two over +-30 binades."""
    g = make_vec("integer" if family == "integer" else "unit", N, 40 + seed, "gamma")
    if family != "integer":
        if family == "wide":
            e = torch.randint(-30, 31, (N,), generator=_gen(family, 41 + seed))
            e[3], e[N - 1] = 30, -30
            g = torch.ldexp(g, e)
        g[0], g[1], g[2] = 0.0, 1e-6, 1e-30
    return _b(g)


def make_rowscale(family, B, seed=0):
    """fp32 [B] (full fp32 numbers: 1 / keep of a drawn keep probability).  integer: 0.5, 1, 2.  cancel: symmetric (sample i and B - 1 - i
    share it).  dropped: runs of zeros including the first and the last sample."""
    g = _gen(family, 50 + seed)
    if family == "integer":
        return make_vec("integer", B, 51 + seed, "rowscale")
    rs = 1.0 / (0.7 + 0.3 * torch.rand(B, generator=g))
    if family == "cancel":
        rs = torch.minimum(rs, rs.flip(0))
    if family == "dropped":
        run = torch.arange(B) % 5 < 2      # samples 0, 1, 5, 6, ... dropped
        run[0] = run[B - 1] = True
        rs = torch.where(run, torch.zeros(B), rs)
    return rs.float()


class RowsIn:
    """The operands of one colsum / resid_bwd / scale_rows case.  dout, y [M, N]; gamma, mul, base0, base1 [N] (bf16 values); rowscale
    fp32 [M / rps]; table int32 [M] and full [M + 5, N]: dout's rows scattered into a larger matrix whose other rows hold NaN."""


def make_rows(family, M, N, rps=1, seed=0):
    g = _gen(family, seed)
    r = RowsIn()
    r.M, r.N, r.rps, r.family = M, N, rps, family
    if family == "integer":
        d, y = torch.randint(-2, 3, (M, N), generator=g).float(), torch.randint(-2, 3, (M, N), generator=g).float()
        r.mul, r.base0, r.base1 = (torch.randint(-2, 3, (N,), generator=g).float() for _ in range(3))
    else:
        d, y = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
        r.mul, r.base0, r.base1 = (_b(torch.randn(N, generator=g)) for _ in range(3))
        r.mul[N - 1] = -r.mul[N - 1].abs() - 0.5
        r.mul = _b(r.mul)
    if family == "offset":
        d, y = d + 8.0, y + 8.0
    elif family == "cancel":      # row M - 1 - i mirrors row i with the opposite sign: T >> |exact|
        h = M // 2
        d, y = _b(d), _b(y)
        d[M - h:] = -d[:h].flip(0)
        y[M - h:] = y[:h].flip(0)
    elif family == "wide":
        e = torch.randint(-30, 31, (M,), generator=g)
        e[0], e[M - 1] = -30, 30
        d = torch.ldexp(d, e[:, None])
    r.rowscale = make_rowscale(family, M // rps, seed)
    r.gamma = make_gamma(family, N, seed)
    neg = set(neg_entries(M))
    if family == "dropped":
        neg |= {m for m in range(M) if float(r.rowscale[m // rps]) == 0.0}
    r.bad = None
    if family == "nonfinite":      # one NaN and one Inf in rows that every route keeps
        kept = [m for m in range(M) if m not in neg] or [0]
        r.bad = ((kept[len(kept) // 2], N // 3), (kept[len(kept) // 3], N - 1))
        d[r.bad[0]], d[r.bad[1]] = float("nan"), float("inf")
    r.dout, r.y = _b(d), _b(y)
    total = M + 5
    tab = torch.randperm(total - 1, generator=g)[:M].to(torch.int32) + 1      # (row 0 of the larger matrix is never named)
    tab[sorted(neg)] = -1
    r.table = tab
    r.full = torch.full((total, N), float("nan"))
    keep = tab >= 0
    r.full[tab[keep].long()] = r.dout[keep]
    return r


def make_finish(family, slots, N, seed=0):
    """rowdot fp32 [slots, N] (full fp32 numbers), three (bias bf16 [N], g0 fp32 [N]) pairs, base bf16 [N]."""
    g = _gen(family, 300 + seed)
    if family == "integer":
        rd = torch.randint(-4, 5, (slots, N), generator=g).float()
        pairs = [(torch.randint(-2, 3, (N,), generator=g).float(), torch.randint(-4, 5, (N,), generator=g).float()) for _ in range(3)]
        return rd, pairs, torch.randint(-2, 3, (N,), generator=g).float()
    rd = torch.randn(slots, N, generator=g)
    if family == "offset":
        rd = rd + 8.0
    elif family == "cancel" and slots > 1:
        h = slots // 2
        rd[slots - h:] = -rd[:h].flip(0)
    elif family == "wide":
        rd = torch.ldexp(rd, torch.randint(-30, 31, (slots, 1), generator=g))
    elif family == "nonfinite":
        rd[slots // 2, N // 3], rd[slots - 1, N - 1] = float("nan"), float("inf")
    pairs = [(_b(torch.randn(N, generator=g)), torch.randn(N, generator=g) * sd) for sd in (2.0, 8.0, 1.0)]
    return rd, pairs, _b(torch.randn(N, generator=g))


SWEEP = [-12.0, -10.0, -8.625, -8.5625, -8.6875, -8.0, -6.0, -5.0, -4.0, -3.0, -2.0, -1.0, -0.5, -0.0, 0.0, 0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 8.0,
         8.5625, 10.0, 12.0, -3e38, 3e38]      # (-8.625 is bf16(-8.6); -8.5625 and -8.6875 are its neighbours)


def make_geglu(family, numel, seed=0):
    """dg, h0, h1 (bf16 values, flat).  sweep: h0 walks SWEEP and a fine grid over [-12, 12], |dg| <= 1.  nonfinite: N(0, 2) with one NaN
    and one Inf in dg."""
    g = _gen(family, 400 + seed)
    dg, h1 = torch.randn(numel, generator=g), torch.randn(numel, generator=g)
    i = torch.arange(numel)
    if family == "sweep":
        fine = ((i * 37) % 3073).float() * (24.0 / 3072) - 12.0
        h0 = torch.where(i % 2 == 0, torch.tensor(SWEEP)[(i // 2) % len(SWEEP)], fine)
        dg = dg.clamp(-1.0, 1.0)
    else:
        h0 = 2 * torch.randn(numel, generator=g)
        dg[numel // 3], dg[numel - 2] = float("nan"), float("inf")
    return _b(dg), _b(h0), _b(h1)


def make_transpose(rows, cols, seed=0):
    """in [rows, cols], scale [rows] (bf16 values, N(0, 1): every product is exact in fp32)."""
    g = _gen("unit", 500 + seed + 7 * rows + cols)
    return _b(torch.randn(rows, cols, generator=g)), _b(0.1 + torch.rand(rows, generator=g))


def guarded_ld(shape, dtype, ld, pad_rows=2, device="cpu"):
    """guarded() for a 2-D view of ANY leading dimension ld >= cols (the transposes' scalar route wants one that is no multiple of 4):
    the same sentinel and the same `_guard` record, so check_guard applies."""
    it, pat = SENTINEL[dtype]
    rows, cols = shape
    assert ld >= cols
    buf = torch.full((rows + 2 * pad_rows, ld), pat, dtype=it, device=device).view(dtype)
    view = buf[pad_rows:pad_rows + rows, :cols]
    mask = torch.ones(buf.shape, dtype=torch.bool, device=device)
    mask[pad_rows:pad_rows + rows, :cols] = False
    view._guard = (buf, mask)
    return view


# ----------------------------------------------------------------------------------------------------------------------
# fp32 re-statements of the kernels (CPU: they show the budgets attainable, and their mutants show the gates sharp)
# ----------------------------------------------------------------------------------------------------------------------
MUTANTS = {
    "colsum": ("rowscale_by_row", "odd_tail_dropped", "rows_past_clamp_dropped", "last_col_block_dropped", "partials_bf16", "base_after_rounding"),
    "resid_bwd": ("rowscale_by_row", "pair_second_scale", "odd_tail_dropped", "rows_past_clamp_dropped", "last_col_block_dropped", "partials_bf16",
                  "base_after_rounding", "gamma_missing_dbias", "gamma_in_dbranch_g0", "neg_entry_reads_row0", "y_through_table"),
    "gamma_grad_finish": ("slots_past_unroll_dropped", "null_bias_as_one", "base_after_rounding"),
    "scale_rows": ("rowscale_by_row",),
    "geglu_bwd": ("tanh_gelu", "dh1_from_grad"),
    "transpose": ("scale_by_column",),
}


def _scale32(rowscale, rps, M, mutant=None, pairs=False):
    if rowscale is None:
        return None
    m = torch.arange(M)
    s = rowscale.float()[(m.clamp_max(rowscale.numel() - 1) if mutant == "rowscale_by_row" else m // rps)]
    if mutant == "pair_second_scale" and pairs:      # the second row of a pair (an odd trip of its wave) takes the first row's scale
        step = 4 * cs_parts(M)
        odd = (m // step) % 2 == 1
        s = torch.where(odd, s[(m - step).clamp_min(0)], s)
    return s[:, None]


def _wave_sums(t, mutant=None, unroll=1):
    """fp32 terms [M, N] -> the partials [parts, N]: every wave adds its rows in order, the four waves of a part meet in LDS."""
    M, N = t.shape
    parts = cs_parts(M)
    step, rpw = 4 * parts, max(1, cs_rows_per_wave(M))
    pad = torch.zeros(rpw * step, N, dtype=F32)
    pad[:M] = t
    if mutant == "rows_past_clamp_dropped":
        pad[64 * CS_MAX_PARTS:] = 0
    pad = pad.view(rpw, step, N)
    if mutant == "odd_tail_dropped" and unroll > 1:      # the rows after a wave's last full unrolled trip
        cnt = (M - torch.arange(step) + step - 1).clamp_min(0) // step
        k = torch.arange(rpw)[:, None]
        pad = torch.where((k >= (cnt // unroll * unroll)[None, :])[:, :, None], torch.zeros((), dtype=F32), pad)
    acc = torch.zeros(step, N, dtype=F32)
    for k in range(rpw):
        acc = acc + pad[k]
    if mutant == "last_col_block_dropped" and N % 512:
        acc[:, N // 512 * 512:] = 0
    w = acc.view(parts, 4, N)
    p = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    return _b(p) if mutant == "partials_bf16" else p


def _fold(p, mul, base, dtype, mutant=None):
    """partials_reduce_kernel: 8 groups of partials, the groups one after the other, `* mul`, `+ base`, ONE rounding."""
    parts, N = p.shape
    g = torch.zeros(cdiv(parts, 8) * 8, N, dtype=F32)
    g[:parts] = p
    g = g.view(-1, 8, N)
    a = torch.zeros(8, N, dtype=F32)
    for k in range(g.shape[0]):
        a = a + g[k]
    t = torch.zeros(N, dtype=F32)
    for i in range(8):
        t = t + a[i]
    if mul is not None:
        t = t * mul.float()
    if base is None:
        return t.to(dtype)
    if mutant == "base_after_rounding":
        return (t.to(dtype).float() + base.float()).to(dtype)
    return (t + base.float()).to(dtype)


def emulate_colsum(x, y=None, rowscale=None, rps=1, mul=None, base=None, dtype=BF, mutant=None):
    x = x.float()
    s = _scale32(rowscale, rps, x.shape[0], mutant)
    t = x if s is None else s * x
    if y is not None:
        t = t * y.float()
    return _fold(_wave_sums(t, mutant, 4 if (y is None and rowscale is None) else 1), mul, base, dtype, mutant)


def emulate_colsum_segments(x, n_seg, seg_cols, bases=None, mutant=None):
    return [emulate_colsum(x[:, i * seg_cols:(i + 1) * seg_cols], base=None if bases is None else bases[i], mutant=mutant) for i in range(n_seg)]


def emulate_resid_bwd(dout, y=None, gamma=None, rowscale=None, rps=1, dgamma=False, dbias=False, g0=False, base=None, dout_rows=None, mutant=None):
    """A dict like resid_bwd_ref's: dbranch, dgamma, dbias (bf16), g0 (fp32)."""
    dout = dout.float()
    d = gather_rows(dout, dout_rows)
    M = d.shape[0]
    if mutant == "neg_entry_reads_row0" and dout_rows is not None:
        d = torch.where((dout_rows < 0)[:, None], dout[0][None, :], d)
    s = _scale32(rowscale, rps, M, mutant, pairs=True)
    t = d if s is None else s * d
    gv = None if (gamma is None or (g0 and mutant != "gamma_in_dbranch_g0")) else gamma.float()
    out = {"dbranch": (t if gv is None else t * gv).to(BF)}
    p1 = _wave_sums(t, mutant, 2) if (dbias or g0) else None
    if dgamma:
        yy = y.float()
        if mutant == "y_through_table" and dout_rows is not None:
            yy = gather_rows(yy, torch.where(dout_rows < 0, dout_rows, dout_rows % M))
        out["dgamma"] = _fold(_wave_sums(t * yy, mutant, 2), None, None if base is None else base[0], BF, mutant)
    if dbias:
        out["dbias"] = _fold(p1, None if mutant == "gamma_missing_dbias" else gamma, None if base is None else base[1], BF, mutant)
    if g0:
        out["g0"] = _fold(p1, None, None, F32, mutant)
    return out


def emulate_gamma_grad_finish(rowdot, pairs, base=None, mutant=None):
    rowdot = rowdot.float()
    N = rowdot.shape[1]
    waves = []
    for a, tail in finish_chains(rowdot.shape[0]):
        sums = []
        for chain in a:
            acc = torch.zeros(N, dtype=F32)
            for s in chain:
                if not (mutant == "slots_past_unroll_dropped" and s in tail):
                    acc = acc + rowdot[s]
            sums.append(acc)
        waves.append((sums[0] + sums[1]) + (sums[2] + sums[3]))
    t = (waves[0] + waves[1]) + (waves[2] + waves[3])
    for b, g in pairs:
        b32 = (torch.ones(N) if mutant == "null_bias_as_one" else torch.zeros(N)) if b is None else b.float()
        t = t + b32 * g.float()
    if base is None:
        return t.to(BF)
    if mutant == "base_after_rounding":
        return (t.to(BF).float() + base.float()).to(BF)
    return (t + base.float()).to(BF)


def emulate_scale_rows(dout, gamma=None, rowscale=None, rps=1, mutant=None):
    d = dout.float()
    s = _scale32(rowscale, rps, d.shape[0], mutant)
    s = torch.ones(1, 1) if s is None else s
    return (d * (s * gamma.float()) if gamma is not None else d * s).to(BF)


def emulate_geglu_bwd(dg, h0, h1, mutant=None):
    dg, h0, h1 = dg.float(), h0.float(), h1.float()
    gp = _gelu_grad32(h0, mutant)
    return (dg * h1 * gp).to(BF), (dg * gp if mutant == "dh1_from_grad" else dg * _gelu32(h0, mutant)).to(BF)


def emulate_transpose(x, scale=None, mutant=None):
    x = x.float()
    if scale is not None:
        sc = scale.float()
        x = x * (sc[torch.arange(x.shape[1]) % sc.numel()][None, :] if mutant == "scale_by_column" else sc[:, None])
    return x.to(BF).t().contiguous()


# ----------------------------------------------------------------------------------------------------------------------
# the case lists (the smallest shapes at which each thing can still go wrong; none is a workload shape)
# ----------------------------------------------------------------------------------------------------------------------
M_SMALL, M_BIG = (1, 3, 4, 5, 63, 64, 65, 257), (16384, 16385, 16384 + 2 * 1024 + 5)
N_SMALL, N_BIG = (8, 64, 512, 520, 1536), (8, 64)
RPS = (1, 3, 7, 64, "M")


def rps_choices(M):
    return [M if r == "M" else r for r in RPS if r == "M" or (r <= M and M % r == 0)]


# every combination of op_resid_bwd's optional arguments that its argument checks admit:
# (gamma, rowscale, sums, accumulate, table); sums: which of dgamma / dbias / g0 are asked for (dgamma and g0 are alternatives)
SUMS = ((), ("dgamma",), ("dbias",), ("dgamma", "dbias"), ("g0",), ("g0", "dbias"))
RESID_COMBOS = [(ga, rs, sums, acc, tab) for tab in (False, True) for ga in (False, True) for rs in (False, True) for sums in SUMS
                for acc in ((False, True) if set(sums) & {"dgamma", "dbias"} else (False,))]
# op_colsum: (y, rowscale, mul, fp32 out, accumulate)
COLSUM_COMBOS = [(y, rs, mul, f32, acc) for y in (False, True) for rs in (False, True) for mul in (False, True) for f32 in (False, True)
                 for acc in (False, True)]
PER_CASE = 8      # combinations a case launches: the list is walked round-robin, so the cases together launch every combination many times


class RowsCase:
    def __init__(self, op, M, N, family, index):
        self.op, self.M, self.N, self.family, self.index = op, M, N, family, index
        ch = rps_choices(M)
        self.rps = ch[index % len(ch)]
        self.id = "%s-%dx%d-rps%d-%s" % (op, M, N, self.rps, family)

    def combos(self):
        allc = RESID_COMBOS if self.op == "resid_bwd" else COLSUM_COMBOS
        # (a stride coprime with both list lengths: consecutive cases start at different places and every combination is reached)
        return [allc[(self.index * PER_CASE * 7 + j * 7) % len(allc)] for j in range(PER_CASE)]


# Every family meets these shapes -- but `unit` stays at M <= 257: tests/test_rows_ref_cpu.py asserts that on `unit` the median of E / R is
# at most 1 / 4 in every bf16 case, and past the clamp the derived budget does not meet that (D = 60 at M = 16385: E = 60 u 0.8 M = 0.047
# against half a bf16 ulp of 0.125 ... 0.25 at |sum| ~ 128: a median of 0.30 over the 8 columns of 16385 x 8 with x y terms).  The case is
# shrunk, the budget is not touched: past the clamp `dropped` (unit rows of which two in five are zeroed) stands in for `unit`.
FAMILY_SHAPES = ((65, 520), (257, 1536), (16385, 8), (M_BIG[2], 64))


def _rows_cases(op, product=False):
    """The cases of the CPU test: every shape with one family (the families rotate) and every family at FAMILY_SHAPES.  product=True
    (the GPU test, where a case costs some 30 ms): those first, then the rest of the product shapes x families."""
    c, seen = [], set()

    def add(M, N, family):
        if family == "unit" and M > 257:
            family = "dropped"      # (the condition on `unit`, see FAMILY_SHAPES)
        if (M, N, family) not in seen and not (family == "nonfinite" and M < 5):
            seen.add((M, N, family))
            c.append(RowsCase(op, M, N, family, len(c)))
    shapes = [(M, N) for M in M_SMALL for N in N_SMALL] + [(M, N) for M in M_BIG for N in N_BIG]
    for M, N in FAMILY_SHAPES:
        for f in FAMILIES:
            add(M, N, f)
    for i, (M, N) in enumerate(shapes):
        add(M, N, FAMILIES[i % len(FAMILIES)])
    if product:
        for M, N in shapes:
            for f in FAMILIES:
                add(M, N, f)
    return c


COLSUM_CASES, RESID_CASES = _rows_cases("colsum"), _rows_cases("resid_bwd")
COLSUM_PRODUCT, RESID_PRODUCT = _rows_cases("colsum", True), _rows_cases("resid_bwd", True)
# (n_seg, seg_cols, M, which output is null or None, family)
SEGMENT_CASES = [(n, sc, M, (1 if (n, sc, M) == (3, 192, 777) else None), FAMILIES[(2 * i + j + 3 * k) % 7])
                 for i, n in enumerate((1, 2, 3)) for j, sc in enumerate((8, 192, 520)) for k, M in enumerate((5, 777))]
FINISH_SLOTS, FINISH_N = (1, 3, 4, 5, 12, 13, 16, 17, 29, 144), (1, 63, 64, 65, 200)
FINISH_FAMILIES = ("unit", "offset", "cancel", "wide", "integer", "nonfinite")
# (slots, N, number of pairs, family): every slot count meets every N, the pair count and the family rotate
FINISH_CASES = [(s, n, (i + j) % 4, FINISH_FAMILIES[(2 * i + j) % 6]) for i, s in enumerate(FINISH_SLOTS) for j, n in enumerate(FINISH_N)]
GEGLU_NUMEL = (8, 8 * 255, 8 * 257, 4194304 + 24)
GEGLU_CASES = [(n, f) for n in GEGLU_NUMEL for f in GEGLU_FAMILIES]
# (2730 x 1536 is the last size of ONE trip: 2730 * 192 = 524160 <= 2048 * 256 = 524288 < 2731 * 192; 2731 and 2732 take a second trip)
SCALE_SHAPES = ((5, 8), (70, 520), (2730, 1536), (2731, 1536), (2732, 1536))
def scale_rps(M):
    """rows per sample of a scale_rows case: a divisor strictly between 1 and M where the list has one (70: 7), else 1 or M."""
    ch = rps_choices(M)
    return ch[len(ch) // 2] if M < 100 else ch[M % 2 - 1]


# (M, N, family, gamma, rowscale): the family and the optional operands rotate over the small shapes; the large ones meet both operands
SCALE_CASES = [(M, N, f, (i + k) % 2 == 0, (i + k) % 3 != 1) for k, (M, N) in enumerate(SCALE_SHAPES[:2]) for i, f in enumerate(FAMILIES)] + \
              [(M, N, f, ga, rs) for (M, N) in SCALE_SHAPES[2:] for f, ga, rs in (("unit", True, True), ("dropped", False, True), ("wide", True, False))]
# (rows, cols, ld_in, ld_out) -- None: contiguous; an ld that is no multiple of 4 takes the scalar route on that side
TRANSPOSE_SHAPES = ((3, 8, None, None), (64, 64, None, None), (65, 67, 67, None), (65, 67, 72, 70), (65, 67, 67, 68), (1, 1, None, None),
                    (257, 136, None, None), (257, 136, 136, 258))
TRANSPOSE_TABLES = ((0,), (2, 6), (0, 1, 3, 5, 7))      # descriptors of one batched launch, as indices into TRANSPOSE_SHAPES; scaled alternately


# ----------------------------------------------------------------------------------------------------------------------
# a combination of optional arguments -> the keyword arguments that the references and the emulations share
# ----------------------------------------------------------------------------------------------------------------------
def colsum_kwargs(r, combo):
    y, rs, mul, f32, acc = combo
    return dict(y=r.y if y else None, rowscale=r.rowscale if rs else None, rps=r.rps, mul=r.mul if mul else None, base=r.base0 if acc else None)


def resid_kwargs(r, combo):
    """(dout, keyword arguments): dout is the larger matrix when the combination reads through the row table."""
    ga, rs, sums, acc, tab = combo
    kw = dict(y=r.y if "dgamma" in sums else None, gamma=r.gamma if ga else None, rowscale=r.rowscale if rs else None, rps=r.rps,
              dgamma="dgamma" in sums, dbias="dbias" in sums, g0="g0" in sums, base=(r.base0, r.base1) if acc else None,
              dout_rows=r.table if tab else None)
    return (r.full if tab else r.dout), kw


def to64(v, device=None):
    """Tensors (also inside tuples, lists and dicts) as fp64 on `device`; row tables stay integers."""
    if isinstance(v, torch.Tensor):
        return v.to(device) if v.dtype == torch.int32 else v.to(device).double()
    if isinstance(v, dict):
        return {k: to64(x, device) for k, x in v.items()}
    if isinstance(v, (tuple, list)):
        return type(v)(to64(x, device) for x in v)
    return v


def combo_name(combo):
    return "/".join("+".join(c) or "-" if isinstance(c, tuple) else str(int(c)) for c in combo)
