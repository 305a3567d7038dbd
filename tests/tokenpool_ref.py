"""Shared by tests/test_vision_cpu.py and tests/test_tokenpool_gpu.py: op_token_mean_ln_fwd / op_token_mean_ln_bwd of csrc/tokenpool.hip
in closed-form fp64 from the bf16 inputs, with the per-element error budget of every output.  Nothing here needs a GPU.  bf,
half_ulp_bf16 and cdiv are those of tests/gemm_ref.py.

THE BUDGET (derived from operation counts; u = 2^-24, g(n) = n u / (1 - n u) is the bound of n fp32 roundings in a row; nothing below
is fitted to what a kernel returned).  Every bound holds for ANY order of a sum: the kernels' fixed orders only make it loose.

Forward, from x (bf16 values), w, b (bf16 values), eps:
  pooled  S - 1 terms: S - 2 additions and the division by S - 1.      E_pool = g(S - 1) mean_s |x|
  mean    H terms of pooled (each off by E_pool), H - 1 additions and the division:
                                                                        E_mean = mean_h E_pool + g(H) mean_h |pooled|
  rstd    d = pooled - mean carries  dd = E_pool + E_mean + u |d|;  a square carries 2 |d| dd + dd^2 + u d^2;  H of them are added and
          divided:  E_var = mean_h (2 |d| dd + dd^2) + g(H + 1) mean_h d^2  (that the squares are taken around the ROUNDED mean is in
          dd);  then + eps, the square root and the reciprocal, one rounding each, and one to spare:
                                                                        E_rstd = rstd (E_var / (2 (var + eps)) + 4 u)
  y       (d rstd) w + b: three roundings on the product chain, one on the sum, then ONE rounding to bf16:
                                                                        E_y = |w| (rstd dd + |d| E_rstd) + 4 u (|d rstd w| + |b|)
                                                                        R_y = half a bf16 ulp at |y| + E_y
Backward, from dy (bf16 values), w, and the STORED fp32 pooled, mean, rstd (inputs of the entry: exact here; `fwd_err` adds what they
carry when the comparison is against a reference that starts from x):
  xhat    (pooled - mean) rstd: two roundings.                          dxh = 2 u |xhat| [+ rstd (E_pool + E_mean) + |d| E_rstd]
  g       dy w: a product of two bf16 numbers, exact in fp32.
  c1      mean_h g:  H - 1 additions and the division.                   E_c1 = g(H) mean_h |g|
  c2      mean_h (g xhat):  a product (or a fused one), H - 1 additions, the division.
                                                                        E_c2 = mean_h (|g| dxh) + g(H + 1) mean_h |g xhat|
  dx      rstd (g - c1 - xhat c2) / (S - 1): five roundings on magnitudes bounded by M = rstd (|g| + |c1| + |xhat c2|) / (S - 1), the
          errors of c1, c2 and xhat scaled the same way, then ONE rounding to bf16 (the CLS row is +0 exactly):
              E_dx = rstd (E_c1 + |xhat| E_c2 + |c2| dxh) / (S - 1) + 5 u M [+ M E_rstd / rstd],    R_dx = half a bf16 ulp at |dx| + E_dx
  dw_part sum_b dy xhat: per term |dy| dxh and a product, B - 1 additions.   E_dw = sum_b |dy| dxh + g(B) sum_b |dy xhat|
  db_part sum_b dy: B - 1 additions.                                          E_db = g(B) sum_b |dy|
fp32 outputs get R = u |exact| on top (the last rounding, counted once more on purpose: it keeps an exact zero budget from meaning
"bit equality with fp64").

THE GATE is |got - exact| <= R + E per element; the figure reported is the largest |got - exact| / (R + E), which must stay <= 1, and
got is finite wherever exact is."""
import torch

from tests.gemm_ref import bf, cdiv, half_ulp_bf16  # noqa: F401

U = 2.0 ** -24
BF16_SENTINEL = 0x7FA5  # a NaN: anything read from a guard element shows in the outputs


def g(n):
    n = max(int(n), 0)
    return n * U / (1.0 - n * U)


def make_inputs(B, S, H, seed=0, with_affine=True):
    """x, dy, w, b as fp64 tensors holding bf16 values.  x: unit normal around a per-column offset (the mean does not cancel to zero)."""
    gen = torch.Generator().manual_seed(1000 * seed + 7 * B + 3 * S + H)
    x = bf(torch.randn(B, S, H, generator=gen, dtype=torch.float64) + 0.5 * torch.randn(1, 1, H, generator=gen, dtype=torch.float64))
    dy = bf(torch.randn(B, H, generator=gen, dtype=torch.float64))
    w = bf(1.0 + 0.25 * torch.randn(H, generator=gen, dtype=torch.float64)) if with_affine else None
    b = bf(0.25 * torch.randn(H, generator=gen, dtype=torch.float64)) if with_affine else None
    return x, dy, w, b


def forward_ref(x, w, b, eps):
    """x fp64 [B, S, H] -> dict of exact outputs and their budgets (R, E) per element."""
    B, S, H = x.shape
    xs = x[:, 1:, :]
    pooled = xs.mean(dim=1)
    E_pool = g(S - 1) * xs.abs().mean(dim=1)
    mean = pooled.mean(dim=1)
    E_mean = E_pool.mean(dim=1) + g(H) * pooled.abs().mean(dim=1)
    d = pooled - mean[:, None]
    var = (d * d).mean(dim=1)
    rstd = 1.0 / torch.sqrt(var + eps)
    dd = E_pool + E_mean[:, None] + U * d.abs()
    E_var = (2 * d.abs() * dd + dd * dd).mean(dim=1) + g(H + 1) * var
    E_rstd = rstd * (E_var / (2 * (var + eps)) + 4 * U)
    wv = torch.ones(H, dtype=torch.float64) if w is None else w
    bv = torch.zeros(H, dtype=torch.float64) if b is None else b
    y = d * rstd[:, None] * wv + bv
    E_y = wv.abs() * (rstd[:, None] * dd + d.abs() * E_rstd[:, None]) + 4 * U * ((d * rstd[:, None] * wv).abs() + bv.abs())
    return {"pooled": (pooled, U * pooled.abs(), E_pool), "mean": (mean, U * mean.abs(), E_mean), "rstd": (rstd, U * rstd, E_rstd),
            "y": (y, half_ulp_bf16(y.abs() + E_y), E_y)}


def backward_ref(dy, pooled, w, mean, rstd, S, fwd_err=None):
    """dy fp64 [B, H] (bf16 values); pooled, mean, rstd fp64 (the stored fp32 values, or exact ones with fwd_err = (E_pool, E_mean,
    E_rstd)) -> dict of exact outputs and budgets.  dx is [B, S, H] with the CLS row zero."""
    B, H = dy.shape
    d = pooled - mean[:, None]
    xhat = d * rstd[:, None]
    dxh = 2 * U * xhat.abs()
    rel_rstd = torch.zeros(B, dtype=torch.float64)
    if fwd_err is not None:
        E_pool, E_mean, E_rstd = fwd_err
        dxh = dxh + rstd[:, None] * (E_pool + E_mean[:, None]) + d.abs() * E_rstd[:, None]
        rel_rstd = E_rstd / rstd
    wv = torch.ones(H, dtype=torch.float64) if w is None else w
    gg = dy * wv
    c1 = gg.mean(dim=1, keepdim=True)
    c2 = (gg * xhat).mean(dim=1, keepdim=True)
    E_c1 = g(H) * gg.abs().mean(dim=1, keepdim=True)
    E_c2 = (gg.abs() * dxh).mean(dim=1, keepdim=True) + g(H + 1) * (gg * xhat).abs().mean(dim=1, keepdim=True)
    tokens = float(S - 1)
    row = rstd[:, None] * (gg - c1 - xhat * c2) / tokens
    M = rstd[:, None] * (gg.abs() + c1.abs() + (xhat * c2).abs()) / tokens
    E_row = rstd[:, None] * (E_c1 + xhat.abs() * E_c2 + c2.abs() * dxh) / tokens + 5 * U * M + M * rel_rstd[:, None]
    dx = row[:, None, :].expand(B, S, H).clone()
    dx[:, 0, :] = 0
    E_dx = E_row[:, None, :].expand(B, S, H).clone()
    E_dx[:, 0, :] = 0
    R_dx = half_ulp_bf16(dx.abs() + E_dx)
    R_dx[:, 0, :] = 0  # the CLS row is +0 exactly
    dw = (dy * xhat).sum(dim=0)
    E_dw = (dy.abs() * dxh).sum(dim=0) + g(B) * (dy * xhat).abs().sum(dim=0)
    db = dy.sum(dim=0)
    E_db = g(B) * dy.abs().sum(dim=0)
    return {"dx": (dx, R_dx, E_dx), "dw_part": (dw, U * dw.abs(), E_dw), "db_part": (db, U * db.abs(), E_db)}


def share(got, ref):
    """The largest |got - exact| / (R + E) of one output (0 / 0 counts as 0); inf where got is not finite."""
    exact, R, E = ref
    got = got.detach().double().cpu().reshape(exact.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err, allowed = (got - exact).abs(), R + E
    ratio = torch.where(err == 0, torch.zeros_like(err), err / allowed)
    return float(ratio.max()) if ratio.numel() else 0.0


# the mirror of csrc/tokenpool.hip: tp_splits (TP_ROWS = 64, TP_MAX_SPLITS = 16)
def splits(S):
    rows = max(64, cdiv(S - 1, 16))
    return rows, cdiv(S - 1, rows)


def guarded3(B, S, H, dtype, device, ld_extra=8, pad_rows=1):
    """A [B, S, H] view with row stride H + ld_extra and pad_rows spare rows after every sample (and in front of the first), inside a
    buffer filled with BF16_SENTINEL.  Returns (view, buffer, mask of the guard elements)."""
    assert dtype == torch.bfloat16
    ld = H + ld_extra
    buf = torch.full((B, S + pad_rows, ld), BF16_SENTINEL, dtype=torch.int16, device=device)
    front = torch.full((pad_rows * ld,), BF16_SENTINEL, dtype=torch.int16, device=device)
    whole = torch.cat([front, buf.flatten()])
    body = whole[pad_rows * ld:].view(B, S + pad_rows, ld)
    view = body.view(torch.bfloat16)[:, :S, :H]
    mask = torch.ones_like(whole, dtype=torch.bool)
    mask[pad_rows * ld:].view(B, S + pad_rows, ld)[:, :S, :H] = False
    return view, whole, mask


def guard_touched(whole, mask):
    return int(((whole != BF16_SENTINEL) & mask).sum())
