"""Shared by tests/test_ln_ref_cpu.py and tests/test_ln_fp64_gpu.py: the LayerNorm family of csrc/layernorm.hip in closed-form fp64
(ln_fwd / ln_bwd with the optional GELU, the row table, `add` and `accumulate`; ln_geglu_fwd / ln_geglu_bwd), the per-element error
budget, the seeded input families, the mirror of the dispatch, the case lists, and an fp32 re-statement of every kernel (`emulate_*`)
with its mutants.  Nothing here needs a GPU: every function runs on whatever device its inputs live on.  bf, half_ulp_bf16, the
exact GELU and the guarded buffers are those of tests/gemm_ref.py.

Every input of a bf16 case holds bf16 VALUES, so the reference and a kernel see the same numbers.

THE BUDGET (derived from the kernels' operation counts; u = 2^-24; nothing below is fitted to what a kernel returned)

A row of `cols` numbers is summed by 64 NW lanes: CH 8 sequential adds per lane, 6 levels of the wave's butterfly, NW partials through
LDS.  A term of the sum passes through at most  D = 8 CH + 6 + NW  additions, so  |sum^ - sum| <= D u sum|x_i|.

  mean = sum * fl(1 / cols): two more roundings (one more for the division)
      E_mean = (D + 3) u  sum|x| / cols
  var: d_i = fl(x_i - mean^), then sum d_i^2 / cols + eps.  With e = mean^ - mean, sum (c_i - e)^2 = sum c_i^2 + cols e^2 (the centred
  c_i sum to zero: a wrong mean enters only in the second order -- what the "centred second pass" of the header buys).  Each term:
  2 u for d_i^2's operand, u for the product; the sum D u; the product with 1 / cols 2 u; the addition of eps u:
      rel(var + eps) = (D + 6) u + E_mean^2 / (var + eps)
  rstd = rsqrtf(.): documented at 1 ulp, taken as 2 ulp = 4 u:
      rho = rel(rstd) = (D + 6) u / 2 + 4 u + E_mean^2 / (2 (var + eps))
  mean and rstd are gated as the fp32 numbers they are: |mean^ - mean| <= E_mean, |rstd^ - rstd| <= rho rstd.
  t = ((x - mean^) rstd^) w + b:  the subtraction (|e| + u |c|), the product with rstd^ (rho + u), with w (u), the addition of b (u):
      E_t = |w| rstd E_mean + |xhat w| (rho + 4 u) + u |t|
  GELU on top (the device's erf is Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7 on erfc, + __expf and the reciprocal: the c_gelu
  treatment of tests/gemm_ref.py, C_GELU u max(|t|, |gelu t|) = C_GELU u |t|; |gelu''| <= 0.8):
      E_y = (|gelu'(t)| + E_t) E_t + C_GELU u |t|
  The stored value adds ONE rounding R: half a bf16 ulp at |exact| + E for a bf16 output, u |exact| for an fp32 one.  The gate is
      |got - exact| <= R + E        per element, and the figure reported is the SHARE |got - exact| / (R + E) (must stay <= 1).

Backward (mean^, rstd^ are INPUTS: the kernel's own forward statistics, given to the reference as they are):
  xhat^ = fl(fl(x - mean) rstd): 2 u |xhat|.  With GELU g = dy gelu'_dev(fl(xhat^ w + b)): the argument is off by E_a = 3 u |xhat w| +
  u |t|, gelu'_dev = Phi + t phi by C_GELU u (Phi's error; t phi <= 0.24 with a relative error of a few u) plus its own rounding and the
  product's:  E_g = |dy| (0.8 E_a + (C_GELU + 2) u max(1, |gelu'|))   (0 without GELU: g = dy).
  c1 = sum(g w) / cols: u per term, D u the sum, 2 u the division:   E_c1 = (D + 3) u sum|g w| / cols + sum(|w| E_g) / cols
  c2 = sum(g w xhat) / cols: 4 u per term:                           E_c2 = (D + 6) u sum|g w xhat| / cols + sum(|w xhat| E_g) / cols
  dx = rstd (g w - c1 - xhat c2) (+ add):
      E_dx = rstd (|w| E_g + E_c1 + |xhat| E_c2 + 3 u |g w| + 2 u |c1| + 4 u |xhat c2|) + u |dx| (+ u |dx + add|)
  dw = sum_rows g xhat, db = sum_rows g: a term is added once per trip in a lane's register, then folded over the 4 waves of a workgroup
  (NW = 1: 3 additions) and over the workgroups' partials by partials_reduce3_kernel (ceil(grid / 8) sequential additions + 8):
      Dw = trips + 3 [NW = 1] + ceil(grid / 8) + 8      (<= rows + 8 for every launch of more than 3 rows; the route gives the number)
      E_dw = (Dw + 3) u sum_rows|g xhat| + sum_rows(|xhat| E_g),   E_db = Dw u sum_rows|g| + sum_rows E_g
  and the fold's  T(t + base)  adds u |exact| before the rounding R of the output type.

GeGLU: g = bf16(gelu_dev(h0) h1) is re-created by both kernels.  The fp32 product is off by E_P = C_GELU u max(|h0|, |gelu h0|) |h1| +
2 u |P|; where the exact product lies closer than E_P to a midpoint between two bf16 numbers the device may round to the OTHER
neighbour: E_g0 = E_P + one bf16 ulp (at |P| + E_P) there, 0 elsewhere (a few elements in 10^4 at h0 > -2, most elements at
h0 < -4, where E_g0 is of the order 1e-6 |h1|).  E_P, not the ulp alone: gelu_parts (csrc/common.h) forms 0.5 erfc as
0.5 t poly(t) e^(-u^2), whose error in the far tail is RELATIVE -- about a percent (1.2 % measured at h0 = -8.6 on the MI355X, case
D-geglu_fwd-8197x2048-constant, whose constant rows make that product the row's mean): far inside the documented absolute bound
1.5e-7, but above the 0.4 % of half a bf16 ulp, so the device's product there lies several of ITS OWN bf16 ulps from the exact one.
In that tail E_P is the prescribed c_gelu bound (absolute), NOT a tight one: it over-allows by orders of magnitude relative to the
product, which is harmless in absolute size (about 1e-6 |h1|) except on exactly constant rows, where rstd = eps^(-1/2) lets y move by
rstd |w| E_P -- a few bf16 ulps of b.  E_g0 enters the mean (sum E_g0 / cols), the variance
((2 sum|c| E_g0 + sum E_g0^2) / cols), xhat (rstd E_g0) and through them y, c2, dh0, dh1 and dw.
  dh0 = dg h1 gelu'(h0):  |h1 gelu'| E_dg + |dg h1| (C_GELU + 2) u max(1, |gelu'|) + 2 u |dh0|
  dh1 = dg gelu(h0):      |gelu h0| E_dg + |dg| C_GELU u |h0| + 2 u |dh1|
with E_dg = E_dx of the LayerNorm backward without GELU (+ rstd |c2| rstd E_g0 for the element's own xhat)."""
import math

import torch

from tests.gemm_ref import C_GELU, bf, cdiv, check_guard, gelu_erf, gelu_erf_grad, guarded, guarded_from, half_ulp_bf16  # noqa: F401

U = 2.0 ** -24
BF, F32 = torch.bfloat16, torch.float32
MIB64 = 64 << 20


# ----------------------------------------------------------------------------------------------------------------------
# the mirror of the dispatch
# ----------------------------------------------------------------------------------------------------------------------
# MIRROR of csrc/layernorm.hip: LN_ROUTES / ln_route / ln_with_route (the cols ladder every entry point goes through), ln_streams with
# ln_fwd_dispatch / ln_bwd_dispatch (the non-temporal rule; never for the q8 forward, always for ln_geglu_fwd_dispatch and
# op_ln_geglu_bwd), ln_grid, and the caps g_ln_blocks_fwd, g_ln_blocks_bwd (512), OP_LN_GEGLU_BLOCKS_FWD (2048),
# OP_LN_GEGLU_BLOCKS_BWD (512).  A build that overrides the macros changes which route a case reaches,
# not whether the case is correct.
CAPS = {"fwd": 512, "fwd_q8": 512, "bwd": 512, "geglu_fwd": 2048, "geglu_fwd_q8": 2048, "geglu_bwd": 512}


def ch_nw(cols):
    assert cols % 8 == 0 and 0 < cols <= 8192
    for lim, c in ((512, (1, 1)), (1024, (2, 1)), (1536, (3, 1)), (2048, (4, 1)), (4096, (2, 4)), (6144, (3, 4)), (8192, (4, 4))):
        if cols <= lim:
            return c


def ln_grid(rows, nw, cap):
    return max(1, min(cap, cdiv(rows, 4) if nw == 1 else rows))


def route(kind, rows, cols, dtype=BF, stats=True):
    """(CH, NW, nt, trips of the busiest row group, whether some row group is idle).  nt: the non-temporal variant (the GeGLU kernels
    have no other)."""
    CH, NW = ch_nw(cols)
    grid = ln_grid(rows, NW, CAPS[kind])
    groups = grid * 4 if NW == 1 else grid
    size = 2 if dtype == BF else 4
    big = rows * cols * size >= MIB64
    nt = {"fwd": big and stats, "fwd_q8": False, "bwd": big}.get(kind, True)
    return CH, NW, bool(nt), cdiv(rows, groups), groups > rows


def depth(cols):
    CH, NW = ch_nw(cols)
    return 8 * CH + 6 + NW


def wgrad_depth(kind, rows, cols, dtype=BF):
    CH, NW, _, trips, _ = route(kind, rows, cols, dtype)
    return trips + (3 if NW == 1 else 0) + cdiv(ln_grid(rows, NW, CAPS[kind]), 8) + 8


# ----------------------------------------------------------------------------------------------------------------------
# closed forms in fp64 (no autograd)
# ----------------------------------------------------------------------------------------------------------------------
def gather_rows(x, x_rows):
    """The launch's rows of the larger matrix x: row r is x[x_rows[r]], a row of zeros where the entry is negative."""
    if x_rows is None:
        return x
    idx = x_rows.long()
    return torch.where((idx >= 0)[:, None], x[idx.clamp_min(0)], torch.zeros((), dtype=x.dtype, device=x.device))


def _affine(w, b, cols, like):
    one = torch.ones(cols, dtype=like.dtype, device=like.device)
    return (one if w is None else w), (0 * one if b is None else b)


def ln_fwd_ref(x, w, b, eps, gelu, x_rows=None):
    """y, mean, rstd of LayerNorm (biased variance, eps inside the root) (+ exact-erf GELU)."""
    x = gather_rows(x, x_rows)
    w, b = _affine(w, b, x.shape[1], x)
    mean = x.mean(1)
    c = x - mean[:, None]
    rstd = ((c * c).mean(1) + eps) ** -0.5
    t = c * rstd[:, None] * w + b
    return (gelu_erf(t) if gelu else t), mean, rstd


def ln_bwd_ref(dy, x, w, b, mean, rstd, gelu, add=None, x_rows=None, base=None):
    """dx [rows of dy], dw, db from the statistics GIVEN.  With x_rows, row r of dx belongs to row x_rows[r] of the larger matrix (the
    rows of negative entries are not stored: see scatter_rows) and `add` is gathered the same way.  base = (dw, db) to accumulate onto."""
    x = gather_rows(x, x_rows)
    w, b = _affine(w, b, x.shape[1], x)
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gelu_erf_grad(xh * w + b) if gelu else dy
    gw = g * w
    dx = rstd[:, None] * (gw - gw.mean(1, keepdim=True) - xh * (gw * xh).mean(1, keepdim=True))
    if add is not None:
        dx = dx + gather_rows(add, x_rows)
    dw, db = (g * xh).sum(0), g.sum(0)
    if base is not None:
        dw, db = dw + base[0], db + base[1]
    return dx, dw, db


def scatter_rows(full, upd, x_rows):
    """`full` with its rows x_rows[r] >= 0 replaced by upd[r] (a copy)."""
    out = full.clone()
    if x_rows is None:
        out[:] = upd
        return out
    keep = x_rows >= 0
    out[x_rows[keep].long()] = upd[keep].to(out.dtype)
    return out


def geglu_product(h0, h1):
    """(g = the product rounded to bf16, E_g0 = a bf16 ulp where the device's fp32 product may round to the other neighbour)."""
    P = gelu_erf(h0) * h1
    g = bf(P)
    half = half_ulp_bf16(P)
    e_p = U * (C_GELU * torch.maximum(h0.abs(), gelu_erf(h0).abs()) * h1.abs() + 2 * P.abs())
    near = (half - (P - g).abs()) <= e_p
    return g, torch.where(near & (P != 0), e_p + 2 * half_ulp_bf16(P.abs() + e_p), torch.zeros_like(P))


def ln_geglu_fwd_ref(h0, h1, w, b, eps):
    g, _ = geglu_product(h0, h1)
    return ln_fwd_ref(g, w, b, eps, False)


def ln_geglu_bwd_ref(dy, h0, h1, w, mean, rstd, base=None):
    """dh0, dh1, dw, db; g is re-created as bf16(gelu(h0) h1)."""
    g, _ = geglu_product(h0, h1)
    dg, dw, db = ln_bwd_ref(dy, g, w, None, mean, rstd, False, base=base)
    return dg * h1 * gelu_erf_grad(h0), dg * gelu_erf(h0), dw, db


# ----------------------------------------------------------------------------------------------------------------------
# the budget (module docstring)
# ----------------------------------------------------------------------------------------------------------------------
def fwd_budget(x, w, b, eps, gelu, x_rows=None, e_g0=None):
    """E of y, mean, rstd (fp64 tensors; the output rounding R is the gate's).  e_g0: the GeGLU product's possible flip."""
    x = gather_rows(x, x_rows)
    cols = x.shape[1]
    w, b = _affine(w, b, cols, x)
    D = depth(cols)
    y, mean, rstd = ln_fwd_ref(x, w, b, eps, False)
    c = x - mean[:, None]
    v = (c * c).mean(1) + eps
    e_mean = (D + 3) * U * x.abs().mean(1)
    rel_v = (D + 6) * U + e_mean ** 2 / v
    e_x = torch.zeros_like(x)
    if e_g0 is not None:
        e_mean = e_mean + e_g0.mean(1)
        rel_v = (D + 6) * U + (e_mean ** 2 + (2 * c.abs() * e_g0 + e_g0 ** 2).mean(1)) / v
        e_x = e_g0
    rho = 0.5 * rel_v + 4 * U
    xhw = (c * rstd[:, None] * w).abs()
    e_t = w.abs() * rstd[:, None] * (e_mean[:, None] + e_x) + xhw * (rho[:, None] + 4 * U) + U * y.abs()
    e_y = (gelu_erf_grad(y).abs() + e_t) * e_t + C_GELU * U * y.abs() if gelu else e_t
    return e_y, e_mean, rho * rstd


def bwd_budget(kind, dy, x, w, b, mean, rstd, gelu, add=None, x_rows=None, base=None, e_g0=None, out_dtype=None, dw_depth=None):
    """E of dx (the launch's rows), dw, db.  kind ("bwd" | "geglu_bwd") and out_dtype (the kernel's, default bf16) give the route and
    with it the depth of the dw / db sums; dw_depth replaces that depth for a kernel with a row walk of its own (tests/audio_ref.py)."""
    x = gather_rows(x, x_rows)
    rows, cols = x.shape
    w, b = _affine(w, b, cols, x)
    D = depth(cols)
    Dw = wgrad_depth(kind, rows, cols, BF if out_dtype is None else out_dtype) if dw_depth is None else dw_depth
    r = rstd[:, None]
    xh = (x - mean[:, None]) * r
    e_g = torch.zeros_like(x)
    g = dy
    if gelu:
        t = xh * w + b
        gp = gelu_erf_grad(t)
        g = dy * gp
        e_g = dy.abs() * (0.8 * U * (3 * (xh * w).abs() + t.abs()) + (C_GELU + 2) * U * gp.abs().clamp_min(1.0))
    e_xh = torch.zeros_like(x) if e_g0 is None else r * e_g0      # (the GeGLU product's flip)
    gw = g * w
    c1, c2 = gw.mean(1, keepdim=True), (gw * xh).mean(1, keepdim=True)
    e_c1 = (D + 3) * U * gw.abs().mean(1, keepdim=True) + (w.abs() * e_g).mean(1, keepdim=True)
    e_c2 = (D + 6) * U * (gw * xh).abs().mean(1, keepdim=True) + ((w * xh).abs() * e_g + gw.abs() * e_xh).mean(1, keepdim=True)
    dx = r * (gw - c1 - xh * c2)
    e_dx = r * (w.abs() * e_g + e_c1 + xh.abs() * e_c2 + c2.abs() * e_xh + U * (3 * gw.abs() + 2 * c1.abs() + 4 * (xh * c2).abs())) + U * dx.abs()
    if add is not None:
        e_dx = e_dx + U * (dx + gather_rows(add, x_rows)).abs()
    dw, db = (g * xh).sum(0), g.sum(0)
    e_dw = (Dw + 3) * U * (g * xh).abs().sum(0) + (xh.abs() * e_g + g.abs() * e_xh).sum(0)
    e_db = Dw * U * g.abs().sum(0) + e_g.sum(0)
    if base is not None:
        dw, db = dw + base[0], db + base[1]
    return e_dx, e_dw + U * dw.abs(), e_db + U * db.abs(), (dx, e_xh)


def geglu_fwd_budget(h0, h1, w, b, eps):
    g, e_g0 = geglu_product(h0, h1)
    return fwd_budget(g, w, b, eps, False, e_g0=e_g0)


def geglu_bwd_budget(dy, h0, h1, w, mean, rstd, base=None):
    """E of dh0, dh1, dw, db."""
    g, e_g0 = geglu_product(h0, h1)
    e_dg, e_dw, e_db, (dg, _) = bwd_budget("geglu_bwd", dy, g, w, None, mean, rstd, False, base=base, e_g0=e_g0)
    gp, ge = gelu_erf_grad(h0), gelu_erf(h0)
    e0 = (h1 * gp).abs() * e_dg + (dg * h1).abs() * (C_GELU + 2) * U * gp.abs().clamp_min(1.0) + 2 * U * (dg * h1 * gp).abs()
    e1 = ge.abs() * e_dg + dg.abs() * C_GELU * U * h0.abs() + 2 * U * (dg * ge).abs()
    return e0, e1, e_dw, e_db


def gate(got, exact, E, rounding, what):
    """Per element |got - exact| <= R + E.  rounding: "bf16" | "f32".  Returns (failures, the largest share |err| / (R + E), the
    largest (|err| - R) / E: what of the fp32 allowance is used beyond the output's rounding -- a bf16 output's share is close to 1
    wherever the exact value lies close to a rounding midpoint); elements whose exact value is not finite are left out (the callers
    check those)."""
    got, exact, E = got.double(), exact.double(), E.double().expand_as(exact)
    fin = torch.isfinite(exact) & torch.isfinite(E)
    z = torch.zeros_like(exact)
    ex, Em = torch.where(fin, exact, z), torch.where(fin, E, z)
    R = half_ulp_bf16(ex.abs() + Em) if rounding == "bf16" else U * ex.abs()
    err = torch.where(fin, (got - exact).abs(), z)
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)
    lim = R + Em
    share = torch.where(err <= lim, err / lim.clamp_min(1e-300), torch.full_like(err, float("inf")))
    share = torch.where(err == 0, z, share)
    fails = []
    bad = err > lim
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        fails.append("%s%s: |%.9g - %.9g| = %.3e > R %.3e + E %.3e (%d of %d elements)" % (
            what, list(i), float(got[i]), float(exact[i]), float(err[i]), float(R[i]), float(Em[i]), int(bad.sum()), bad.numel()))
    over = torch.where(err > R, (err - R) / Em.clamp_min(1e-300), z)
    return fails, (float(share.max()) if share.numel() else 0.0), (float(over.max()) if over.numel() else 0.0)


# ----------------------------------------------------------------------------------------------------------------------
# input families
# ----------------------------------------------------------------------------------------------------------------------
FAMILIES = ("normal", "offset", "tiny", "constant", "outlier", "rowscale", "gelu_tails")


def _gen(family, seed):
    return torch.Generator().manual_seed(7000 + 1000 * FAMILIES.index(family) + seed)


def _store(t, dtype):
    return t.to(dtype).float() if dtype == BF else t.float()


def make_x(family, rows, cols, dtype=BF, seed=0):
    """[rows, cols] fp32 (bf16 values for dtype bf16).  normal: N(0, 2^2).  offset: row means ~64 (bf16) / ~1000 (fp32) that differ per
    row, sigma 4 / 1.  tiny: sigma 1e-3.  constant: every third row exactly constant.  outlier: one entry of ~1000 per row, in the last
    chunk for row 0, elsewhere for the others.  rowscale: row r times 2^(r mod 21 - 10).  gelu_tails: N(0, 1) (its w, b: make_wb)."""
    g = _gen(family, seed)
    x = torch.randn(rows, cols, generator=g)
    r = torch.arange(rows)
    if family == "normal":
        x = 2 * x
    elif family == "offset":
        m = torch.randn(rows, 1, generator=g)
        x = (64 + 8 * m + 4 * x) if dtype == BF else (1000 + 100 * m + x)
    elif family == "tiny":
        x = 1e-3 * x
    elif family == "constant":
        x = _store(2 * x, dtype)
        cst = _store(3 * torch.randn(rows, 1, generator=g), dtype)
        x = torch.where((r % 3 == 1)[:, None], cst.expand(rows, cols), x)
    elif family == "outlier":
        x = 2 * x
        x[r, (cols - 1 - 13 * r) % cols] = 1000.0 + r.float() % 7
    elif family == "rowscale":
        x = torch.ldexp(2 * x, (r % 21 - 10)[:, None])
    elif family != "gelu_tails":
        raise ValueError(family)
    return _store(x, dtype)


def make_dy(family, rows, cols, dtype=BF, seed=0):
    """N(0, 1), or (family rowscale) row r times 2^(r mod 21 - 10)."""
    x = torch.randn(rows, cols, generator=_gen("normal", 100 + seed))
    if family == "rowscale":
        x = torch.ldexp(x, (torch.arange(rows) % 21 - 10)[:, None])
    return _store(x, dtype)


def make_wb(family, cols, dtype=BF, seed=0, wide=False):
    """w = 1 + 0.1 N, b = 0.1 N; gelu_tails: w = 2 (1 + 0.1 N), so that the pre-activations span about +-6 (sometimes 8);
    wide: |w| from 2^-6 to 2^6."""
    g = _gen(family, 200 + seed)
    w, b = 1 + 0.1 * torch.randn(cols, generator=g), 0.1 * torch.randn(cols, generator=g)
    if family == "gelu_tails":
        w = 2 * w
    if wide:
        w = torch.ldexp(w, torch.arange(cols) % 13 - 6)
    return _store(w, dtype), _store(b, dtype)


def make_h(family, rows, cols, seed=0):
    """h0, h1 of the GeGLU kernels (bf16 values).  offset: h0 ~ 4, h1 ~ 64 (a product of large mean); gelu_tails: h0 ~ N(0, 2^2)."""
    h0, h1 = make_x(family, rows, cols, BF, seed + 10), make_x(family, rows, cols, BF, seed + 11)
    if family == "offset":
        h0 = _store(h0 / 16, BF)
    elif family == "gelu_tails":
        h0 = _store(2 * h0, BF)
    return h0, h1


def make_row_table(rows, rows_total, seed=0):
    """int32 [rows]: distinct rows of a larger matrix in a scrambled order, about one in seven dropped (-1); entry 1 always."""
    g = torch.Generator().manual_seed(4242 + seed)
    t = torch.randperm(rows_total, generator=g)[:rows].to(torch.int32)
    drop = torch.rand(rows, generator=g) < 0.15
    if rows > 3:
        drop[1] = True
    t[drop] = -1
    return t


# ----------------------------------------------------------------------------------------------------------------------
# fp32 re-statements of the kernels (CPU only: they show the budgets attainable, and their mutants show the gates sharp)
# ----------------------------------------------------------------------------------------------------------------------
MUTANTS = ("var_one_pass", "var_unbiased", "eps_outside_root", "dx_without_c2", "dx_without_w", "tanh_gelu", "stats_of_unrounded_product",
           "chunk_unwritten", "stale_prefetch", "add_on_unmapped_row", "accumulate_ignored")
RSQRT2 = 1.0 / math.sqrt(2.0)


def _gelu32(t, mutant):
    if mutant == "tanh_gelu":
        return 0.5 * t * (1 + torch.tanh(0.7978845608 * (t + 0.044715 * t ** 3)))
    return 0.5 * t * torch.special.erfc(-t * RSQRT2)


def _gelu_grad32(t, mutant):
    if mutant == "tanh_gelu":
        a = 0.7978845608 * (t + 0.044715 * t ** 3)
        th = torch.tanh(a)
        return 0.5 * (1 + th) + 0.5 * t * (1 - th * th) * 0.7978845608 * (1 + 3 * 0.044715 * t * t)
    return 0.5 * torch.special.erfc(-t * RSQRT2) + t * torch.exp(-0.5 * t * t) * 0.3989422804


def _stale(t, rstep):
    """Row r holds the data of row r - rstep (the prefetch handed over one trip late)."""
    out = t.clone()
    out[rstep:] = t[:-rstep]
    return out


def _stats32(x, eps, mutant):
    cols = x.shape[1]
    inv = torch.tensor(1.0, dtype=F32) / cols
    mean = x.sum(1) * inv
    d = x - mean[:, None]
    var = (d * d).sum(1) * inv
    if mutant == "var_one_pass":
        var = (x * x).sum(1) * inv - mean * mean
    elif mutant == "var_unbiased":
        var = (d * d).sum(1) / (cols - 1)
    rstd = 1 / (var.clamp_min(0).sqrt() + eps) if mutant == "eps_outside_root" else torch.rsqrt(var + eps)
    return mean, d, rstd


def _unwritten(y, prefill=0.0):
    y[y.shape[0] // 2, -8:] = prefill     # the last 8-column chunk of one row keeps what the buffer held
    return y


def emulate_ln_fwd(x, w, b, eps, gelu, dtype=BF, x_rows=None, mutant=None, rstep=2):
    """x, w, b: fp32 tensors.  Returns y (as `dtype`), mean, rstd (fp32)."""
    x = gather_rows(x.float(), x_rows)
    if mutant == "stale_prefetch":
        x = _stale(x, rstep)
    w, b = _affine(w, b, x.shape[1], x)
    mean, d, rstd = _stats32(x, eps, mutant)
    t = d * rstd[:, None] * w + b
    y = (_gelu32(t, mutant) if gelu else t).to(dtype)
    return (_unwritten(y) if mutant == "chunk_unwritten" else y), mean, rstd


def emulate_ln_bwd(dy, x, w, b, mean, rstd, gelu, dtype=BF, add=None, x_rows=None, dx_full=None, base=None, mutant=None, rstep=2):
    """Returns (dx, dw, db).  Without x_rows dx has the launch's rows; with x_rows it is dx_full (the larger matrix as it was) with the
    mapped rows replaced.  base = (dw, db) as `dtype` when accumulating."""
    xg, dy = gather_rows(x.float(), x_rows), dy.float()
    if mutant == "stale_prefetch":
        xg, dy = _stale(xg, rstep), _stale(dy, rstep)
    w, b = _affine(w, b, xg.shape[1], xg)
    xh = (xg - mean[:, None]) * rstd[:, None]
    g = dy * _gelu_grad32(xh * w + b, mutant) if gelu else dy
    gw = g if mutant == "dx_without_w" else g * w
    inv = torch.tensor(1.0, dtype=F32) / xg.shape[1]
    c1, c2 = gw.sum(1, keepdim=True) * inv, (gw * xh).sum(1, keepdim=True) * inv
    if mutant == "dx_without_c2":
        c2 = 0 * c2
    o = rstd[:, None] * (gw - c1 - xh * c2)
    if add is not None:
        o = o + gather_rows(add.float(), x_rows)
    o = o.to(dtype)
    if mutant == "chunk_unwritten":
        o = _unwritten(o)
    if x_rows is not None:
        full = scatter_rows(dx_full.to(dtype), o, x_rows)
        if mutant == "add_on_unmapped_row":     # `src >= 0` forgotten in the store: the row lands on row 0 of the larger matrix
            un = (x_rows < 0).nonzero()
            if un.numel():
                full[0] = (o[un[0, 0]].float() + (add[0].float() if add is not None else 0)).to(dtype)
        o = full
    dw, db = (g * xh).sum(0), g.sum(0)
    if base is not None and mutant != "accumulate_ignored":
        dw, db = dw + base[0].float(), db + base[1].float()
    return o, dw.to(dtype), db.to(dtype)


def _product32(h0, h1, mutant=None):
    return (_gelu32(h0.float(), mutant) * h1.float()).to(BF).float()


def emulate_ln_geglu_fwd(h0, h1, w, b, eps, mutant=None, rstep=2):
    h0, h1 = h0.float(), h1.float()
    if mutant == "stale_prefetch":
        h0, h1 = _stale(h0, rstep), _stale(h1, rstep)
    g = _product32(h0, h1, mutant)
    if mutant == "stats_of_unrounded_product":
        g = _gelu32(h0, None) * h1
    return emulate_ln_fwd(g, w, b, eps, False, BF, mutant=mutant if mutant in ("var_one_pass", "var_unbiased", "eps_outside_root", "chunk_unwritten") else None)


def emulate_ln_geglu_bwd(dy, h0, h1, w, mean, rstd, base=None, mutant=None, rstep=2):
    """Returns dh0, dh1, dw, db (bf16)."""
    h0, h1, dy = h0.float(), h1.float(), dy.float()
    if mutant == "stale_prefetch":
        h0, h1, dy = _stale(h0, rstep), _stale(h1, rstep), _stale(dy, rstep)
    g = _product32(h0, h1, mutant)
    w1, _ = _affine(w, None, g.shape[1], g)
    xh = (g - mean[:, None]) * rstd[:, None]
    gw = dy if mutant == "dx_without_w" else dy * w1
    inv = torch.tensor(1.0, dtype=F32) / g.shape[1]
    c1, c2 = gw.sum(1, keepdim=True) * inv, (gw * xh).sum(1, keepdim=True) * inv
    if mutant == "dx_without_c2":
        c2 = 0 * c2
    dg = rstd[:, None] * (gw - c1 - xh * c2)
    o0, o1 = (dg * h1 * _gelu_grad32(h0, mutant)).to(BF), (dg * _gelu32(h0, mutant)).to(BF)
    if mutant == "chunk_unwritten":
        o0 = _unwritten(o0)
    dw, db = (dy * xh).sum(0), dy.sum(0)
    if base is not None and mutant != "accumulate_ignored":
        dw, db = dw + base[0].float(), db + base[1].float()
    return o0, o1, dw.to(BF), db.to(BF)


# ----------------------------------------------------------------------------------------------------------------------
# the cases of the GPU test (the CPU test proves the coverage claims from route())
# ----------------------------------------------------------------------------------------------------------------------
class LnCase:
    """One LayerNorm forward + backward (kind "ln") or GeGLU forward / backward (kind "geglu_fwd" | "geglu_bwd") of the GPU test.
    halves: h0 / h1 (and dh0 / dh1) are the halves of one [rows, 2 cols] matrix."""

    def __init__(self, group, kind, rows, cols, dtype=BF, gelu=False, family="normal", dyfam="normal", wide=False, eps=1e-5, halves=True):
        self.group, self.kind, self.rows, self.cols, self.dtype, self.gelu = group, kind, rows, cols, dtype, gelu
        self.family, self.dyfam, self.wide, self.eps, self.halves = family, dyfam, wide, eps, halves
        self.id = "%s-%s-%dx%d-%s%s-%s%s%s%s%s" % (group, kind, rows, cols, "bf16" if dtype == BF else "f32", "-gelu" if gelu else "", family,
                                                   "-dyrs" if dyfam == "rowscale" else "", "-wide" if wide else "",
                                                   "" if eps == 1e-5 else "-eps%g" % eps, "" if halves or kind == "ln" else "-contig")

    def kinds(self):
        return ("fwd", "bwd") if self.kind == "ln" else (self.kind,)

    def elements(self):
        return self.rows * self.cols


A_COLS, B_COLS = (72, 520, 1536, 2048), (2056, 4104, 6144, 8192)
A_ROWS, B_ROWS = 4101, 1029
NT_CASES = ((16384, 2048, BF), (4096, 8192, BF), (2048, 8192, F32))


def _cases():
    c = []
    add = lambda *a, **k: c.append(LnCase(*a, **k))  # noqa: E731
    fams = list(FAMILIES)
    # A: one wave per row, three trips.  The families rotate over the shapes (every family meets NW = 1 and NW = 4).
    for i, cols in enumerate(A_COLS):
        add("A", "ln", A_ROWS, cols, family=fams[i % 7], dyfam=("normal", "rowscale")[i % 2])
        add("A", "ln", A_ROWS, cols, gelu=True, family=("gelu_tails", "normal", "outlier", "rowscale")[i])
    add("A", "ln", A_ROWS, 520, F32, family="offset")
    add("A", "ln", A_ROWS, 2048, F32, family="tiny", dyfam="rowscale")
    add("A", "ln", A_ROWS, 72, family="outlier")
    add("A", "ln", A_ROWS, 520, family="rowscale")
    add("A", "ln", A_ROWS, 1536, family="gelu_tails", gelu=True, wide=True)
    add("A", "ln", A_ROWS, 520, family="normal", wide=True)
    for eps in (1e-6, 1e-3):     # (1e-5 is every other case's)
        add("A", "ln", A_ROWS, 520, family="tiny", eps=eps)
        add("B", "ln", B_ROWS, 4104, family="tiny", eps=eps, gelu=True)
    # B: a workgroup per row, three trips
    for i, cols in enumerate(B_COLS):
        add("B", "ln", B_ROWS, cols, family=fams[(i + 3) % 7], dyfam=("rowscale", "normal")[i % 2])
    add("B", "ln", B_ROWS, 2056, F32, family="offset")
    add("B", "ln", B_ROWS, 8192, F32, family="normal", gelu=True)
    add("B", "ln", B_ROWS, 6144, gelu=True, family="gelu_tails")
    add("B", "ln", B_ROWS, 2056, family="normal")
    add("B", "ln", B_ROWS, 4104, family="offset")
    add("B", "ln", B_ROWS, 6144, family="tiny")
    add("B", "ln", B_ROWS, 8192, family="constant", wide=True)
    # C: one trip and ragged tails
    for rows in (1, 3, 5, 2049):
        for j, cols in enumerate((8, 64, 1544)):
            add("C", "ln", rows, cols, family=fams[(rows + j) % 7], gelu=bool((rows + j) % 2))
    add("C", "ln", 5, 64, F32, family="constant", gelu=True)
    add("C", "ln", 2049, 4104, family="normal")
    for cols in (520, 1536, 2048) + B_COLS:     # one trip on the classes the three widths above do not reach
        add("C", "ln", 5, cols, family="outlier")
    for cols in (512, 1024, 4096):     # the widest row of the three classes whose maximum no case above reaches
        add("C", "ln", 5, cols, family="outlier")
    # D: the GeGLU pair
    for i, cols in enumerate(A_COLS):
        add("D", "geglu_fwd", 8197, cols, family=fams[i % 7])
        add("D", "geglu_bwd", A_ROWS, cols, family=fams[(i + 4) % 7], dyfam=("normal", "rowscale")[i % 2])
        add("D", "geglu_fwd", 5, cols, family="gelu_tails")
        add("D", "geglu_bwd", 5, cols, family="gelu_tails")
    for cols in (512, 1024, 4096):     # (as in group C: the class maxima no other width reaches)
        add("D", "geglu_fwd", 5, cols, family="gelu_tails")
        add("D", "geglu_bwd", 5, cols, family="gelu_tails")
    for i, cols in enumerate((2056, 6144)):
        add("D", "geglu_fwd", 2053, cols, family=("offset", "gelu_tails")[i])
    for i, cols in enumerate(B_COLS):
        add("D", "geglu_bwd", B_ROWS, cols, family=fams[i % 7], wide=(i == 1))
        add("D", "geglu_fwd", 3, cols, family="normal")
        add("D", "geglu_bwd", 3, cols, family="rowscale")
    # three trips under the forward's cap of 2048 workgroups (the rows above give it two), on every (CH, NW) class
    for i, cols in enumerate(A_COLS):
        add("D", "geglu_fwd", 16389, cols, family=("normal", "outlier", "rowscale", "gelu_tails")[i])
    for i, cols in enumerate(B_COLS):
        add("D", "geglu_fwd", 4101, cols, family=("normal", "tiny", "constant", "rowscale")[i])
    add("D", "geglu_fwd", 8197, 520, family="normal", halves=False)
    add("D", "geglu_bwd", A_ROWS, 520, family="normal", halves=False)
    ids = [x.id for x in c]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1][:3]
    return c


CASES = _cases()


def by_group(group, kind=None):
    return [c for c in CASES if c.group == group and (kind is None or c.kind == kind)]
