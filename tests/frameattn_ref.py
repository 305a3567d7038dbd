"""Shared by tests/test_frameattn_cpu.py and tests/test_frameattn_gpu.py: op_attn_frames_fwd / op_attn_frames_bwd of csrc/frameattn.hip
in closed-form fp64 from the bf16 inputs, with the per-element error budget of every output, an fp32 restatement of the kernel's
arithmetic with three deliberately wrong variants, and guarded buffers.  Nothing here needs a GPU.  bf and half_ulp_bf16 are those of
tests/gemm_ref.py.

Tensors are [B, T, N, heads, 64] (the kernels' element (b, t, n, h, d)); a sequence is (b, n, h) over t.

THE BUDGET (derived from operation counts; u = 2^-24, g(n) = n u / (1 - n u) is the bound of n fp32 roundings in a row; nothing below is
fitted to what a kernel returned).  Every bound holds for ANY order of a sum: the kernels' fixed orders only make it loose.  Terms of
second order in u are left out; they are 2^-24 of the terms kept.
  s     scale * (q . k): a 64-term dot (the products of two bf16 numbers are exact in fp32), then one product.
                                                                        E_s = |scale| g(64) sum_d |q k| + u |s|
  e     exp(s - m), m the largest COMPUTED score.  A common error of m multiplies every e of the row by one factor, which cancels in
        every quotient below, so it is not charged.  The argument carries a = E_s + 2 u |s - m| (the score, the subtraction), expf
        at most 4 u more:                                                 r_e = expm1(a) + 4 u           (relative)
  l     sum_t' e: T terms.                                                r_l = (sum e r_e) / l + g(T)   (relative)
  p     e * (1 / l): a reciprocal (2 u allowed) and a product.           r_p = r_e + r_l + 3 u          (relative)
  out   (sum_t' e v) / l: T fused terms, the reciprocal and a product, then ONE rounding to bf16:
            E_out = (sum p |v| r_e + g(T) sum p |v| + |out| r_l) (1 + 2 r_l) + 4 u |out|,    R_out = half a bf16 ulp at |out| + E_out
  dp    dout . v: a 64-term dot.                                         E_dp = g(64) sum_d |dout v|
  c     (sum_t' e dp) / l.              E_c = sum p (r_e |dp| + E_dp) + g(T) sum p |dp| + |c| (r_l + 3 u)
  ds    p (dp - c): a subtraction and a product.                         E_ds = p (E_dp + E_c) + |ds| (r_p + 2 u)
  dq    scale * sum_t' ds k;   dk  scale * sum_t ds q:   T fused terms and the factor, then ONE rounding to bf16:
            E = |scale| (sum E_ds |k| + g(T) sum |ds k|) + u |dq|     (q for k and the sum over t for dk)
  dv    sum_t p dout: T fused terms.    E_dv = sum p r_p |dout| + g(T) sum p |dout|
THE GATE is |got - exact| <= R + E per element, R = half a bf16 ulp at |exact| + E; the figure reported is the largest
|got - exact| / (R + E), which must stay <= 1, and got is finite wherever exact is."""
import numpy as np
import torch

from tests.gemm_ref import bf, half_ulp_bf16  # noqa: F401

U = 2.0 ** -24
BF16_SENTINEL = 0x7FA5  # a NaN: anything read from a guard element shows in the outputs
HD = 64


def g(n):
    n = max(int(n), 0)
    return n * U / (1.0 - n * U)


def f32(x):
    """The fp32 value the entry receives for a Python float."""
    return float(np.float32(x))


def make_inputs(B, T, N, heads, seed=0, spread=1.0):
    """q, k, v, dout as fp64 tensors [B, T, N, heads, 64] holding bf16 values.  spread scales q and k: scale * q . k has a standard
    deviation of about spread^2 at scale = 1 / 8."""
    gen = torch.Generator().manual_seed(100000 * seed + 1000 * B + 100 * T + 10 * N + heads)
    mk = lambda s: bf(s * torch.randn(B, T, N, heads, HD, generator=gen, dtype=torch.float64))  # noqa: E731
    return mk(spread), mk(spread), mk(1.0), mk(1.0)


def _seq(x):
    """[B, T, N, heads, 64] -> [B, N, heads, T, 64]: one sequence per (b, n, h)."""
    return x.permute(0, 2, 3, 1, 4)


def _unseq(x):
    return x.permute(0, 3, 1, 2, 4)


def _softmax_parts(q, k, scale):
    T = q.shape[-2]
    s = scale * torch.einsum("...td,...ud->...tu", q, k)
    E_s = abs(scale) * g(HD) * torch.einsum("...td,...ud->...tu", q.abs(), k.abs()) + U * s.abs()
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - m)
    r_e = torch.expm1(E_s + 2 * U * (s - m).abs()) + 4 * U
    l = e.sum(dim=-1, keepdim=True)
    r_l = (e * r_e).sum(dim=-1, keepdim=True) / l + g(T)
    p = e / l
    r_p = r_e + r_l + 3 * U
    return p, r_e, r_l, r_p


def forward_ref(q, k, v, scale):
    """fp64 [B, T, N, heads, 64] (bf16 values), scale (the fp32 value) -> {"out": (exact, R, E)}."""
    q, k, v = _seq(q), _seq(k), _seq(v)
    T = q.shape[-2]
    p, r_e, r_l, _ = _softmax_parts(q, k, scale)
    out = torch.einsum("...tu,...ud->...td", p, v)
    E = (torch.einsum("...tu,...ud->...td", p * r_e, v.abs()) + g(T) * torch.einsum("...tu,...ud->...td", p, v.abs())
         + out.abs() * r_l) * (1 + 2 * r_l) + 4 * U * out.abs()
    out, E = _unseq(out), _unseq(E)
    return {"out": (out, half_ulp_bf16(out.abs() + E), E)}


def backward_ref(q, k, v, dout, scale):
    """-> {"dq": ..., "dk": ..., "dv": ...}, each (exact, R, E), [B, T, N, heads, 64]."""
    q, k, v, do = _seq(q), _seq(k), _seq(v), _seq(dout)
    T = q.shape[-2]
    p, r_e, r_l, r_p = _softmax_parts(q, k, scale)
    dp = torch.einsum("...td,...ud->...tu", do, v)
    E_dp = g(HD) * torch.einsum("...td,...ud->...tu", do.abs(), v.abs())
    c = (p * dp).sum(dim=-1, keepdim=True)
    E_c = (p * (r_e * dp.abs() + E_dp)).sum(dim=-1, keepdim=True) + g(T) * (p * dp.abs()).sum(dim=-1, keepdim=True) + c.abs() * (r_l + 3 * U)
    ds = p * (dp - c)
    E_ds = p * (E_dp + E_c) + ds.abs() * (r_p + 2 * U)
    dq = scale * torch.einsum("...tu,...ud->...td", ds, k)
    E_dq = abs(scale) * (torch.einsum("...tu,...ud->...td", E_ds, k.abs()) + g(T) * torch.einsum("...tu,...ud->...td", ds.abs(), k.abs())) \
        + U * dq.abs()
    dk = scale * torch.einsum("...tu,...td->...ud", ds, q)
    E_dk = abs(scale) * (torch.einsum("...tu,...td->...ud", E_ds, q.abs()) + g(T) * torch.einsum("...tu,...td->...ud", ds.abs(), q.abs())) \
        + U * dk.abs()
    dv = torch.einsum("...tu,...td->...ud", p, do)
    E_dv = torch.einsum("...tu,...td->...ud", p * r_p, do.abs()) + g(T) * torch.einsum("...tu,...td->...ud", p, do.abs())
    res = {}
    for name, exact, E in (("dq", dq, E_dq), ("dk", dk, E_dk), ("dv", dv, E_dv)):
        exact, E = _unseq(exact), _unseq(E)
        res[name] = (exact, half_ulp_bf16(exact.abs() + E), E)
    return res


def share(got, ref):
    """The largest |got - exact| / (R + E) of one output (0 / 0 counts as 0); inf where got is not finite."""
    exact, R, E = ref
    got = got.detach().double().cpu().reshape(exact.shape)
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    err, allowed = (got - exact).abs(), R + E
    ratio = torch.where(err == 0, torch.zeros_like(err), err / allowed)
    return float(ratio.max()) if ratio.numel() else 0.0


# ---- an fp32 restatement of the kernels' arithmetic on the FLAT rows, and three wrong variants ------------------------------------------
def restate_fp32(q, k, v, dout, scale, B, T, N, heads, variant=None):
    """q, k, v, dout: [B * T * N, heads * 64] (bf16 values, any float dtype), rows ordered (b, t, n).  fp32 arithmetic as the kernels
    do it (scores and p in fp32, one rounding to bf16 at the end) -> out, dq, dk, dv as fp64 [B, T, N, heads, 64] holding bf16 values.
    variant: None, or one of the mistakes the budget must catch: "swapped_strides" (the rows taken as (b, n, t)), "no_scale",
    "p_bf16" (the probabilities rounded to bf16 before the second product, as the reference's bf16 run does)."""
    def seq(x):
        x = x.float().reshape(B * T * N, heads, HD)
        if variant == "swapped_strides":
            return x.view(B, N, T, heads, HD).permute(0, 1, 3, 2, 4)
        return x.view(B, T, N, heads, HD).permute(0, 2, 3, 1, 4)

    def unseq(x):
        if variant == "swapped_strides":
            return x.permute(0, 1, 3, 2, 4).reshape(B * T * N, heads, HD).view(B, T, N, heads, HD)
        return x.permute(0, 3, 1, 2, 4)
    sc = torch.tensor(1.0 if variant == "no_scale" else scale, dtype=torch.float32)
    qs, ks, vs, dos = seq(q), seq(k), seq(v), seq(dout)
    s = sc * torch.einsum("...td,...ud->...tu", qs, ks)
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    inv = 1.0 / e.sum(dim=-1, keepdim=True)
    p = e * inv
    pv = p.to(torch.bfloat16).float() if variant == "p_bf16" else p
    out = torch.einsum("...tu,...ud->...td", pv, vs)
    dp = torch.einsum("...td,...ud->...tu", dos, vs)
    ds = pv * (dp - (pv * dp).sum(dim=-1, keepdim=True))
    dq = sc * torch.einsum("...tu,...ud->...td", ds, ks)
    dk = sc * torch.einsum("...tu,...td->...ud", ds, qs)
    dv = torch.einsum("...tu,...td->...ud", pv, dos)
    return {n: bf(unseq(t).double()) for n, t in (("out", out), ("dq", dq), ("dk", dk), ("dv", dv))}


def rows(x):
    """[B, T, N, heads, 64] -> the kernels' rows [B * T * N, heads * 64]."""
    B, T, N, heads, hd = x.shape
    return x.reshape(B * T * N, heads * hd)


# ---- guarded device buffers ------------------------------------------------------------------------------------------------------------
def guarded_rows(R, cols, ld, device, pad_rows=1):
    """A [R, cols] bf16 view with row stride ld >= cols and pad_rows spare rows in front and behind, inside a buffer filled with
    BF16_SENTINEL (the view itself too, until it is written).  Returns (view, buffer, mask of the guard elements)."""
    whole = torch.full(((R + 2 * pad_rows) * ld,), BF16_SENTINEL, dtype=torch.int16, device=device)
    body = whole[pad_rows * ld:(pad_rows + R) * ld].view(R, ld)
    mask = torch.ones_like(whole, dtype=torch.bool)
    mask[pad_rows * ld:(pad_rows + R) * ld].view(R, ld)[:, :cols] = False
    return body.view(torch.bfloat16)[:, :cols], whole, mask


def guard_touched(whole, mask):
    return int(((whole != BF16_SENTINEL) & mask).sum())
