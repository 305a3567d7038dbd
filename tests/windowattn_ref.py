"""Shared by tests/test_windowattn_cpu.py and tests/test_windowattn_gpu.py: op_attn_window_fwd / op_attn_window_bwd of
csrc/windowattn.hip in closed-form fp64 from the bf16 inputs, with the per-element error budget of every output, an fp32 restatement of
the kernels' arithmetic with six deliberately wrong variants, and guarded buffers (those of tests/frameattn_ref.py).  Nothing here needs
a GPU.  bf and half_ulp_bf16 are those of tests/gemm_ref.py, C_ACC is its constant for sums accumulated on the matrix pipe.

Tensors are [B, Hg, Wg, heads, 64] (the kernels' element (b, y, x, h, d)); a sequence is (b, window, h) over the 256 tokens
i = 16 (y % 16) + x % 16 of a 16 x 16 window.  bias is [heads, 256, 256], rel_h and rel_w are [31, 64].

THE BUDGET (derived from operation counts; u = 2^-24, g(n) = n u / (1 - n u) bounds n fp32 roundings in a row; an fp32 sum of n terms is
charged C g(n) times the sum of the terms' magnitudes, C = C_ACC on the matrix pipe and 1 elsewhere; hb(x) is half a bf16 ulp at |x|,
charged for every operand the header says is rounded to bf16 before a matrix-pipe product and carried linearly through that product;
nothing below is fitted to what a kernel returned).  Every bound holds for ANY order of a sum.  Terms of second order in u are left out.
  Th    q . rel_h[iy - jy + 15], Tw likewise: 64-term dots on the matrix pipe.       E_T = C_ACC g(64) sum_d |q rel|
  s     scale (q . k) + bias + Th + Tw: a 64-term dot on the matrix pipe, a product, three additions (4 u of the magnitude sum M_s).
                                             E_s = |scale| C_ACC g(64) sum_d |q k| + E_Th + E_Tw + 4 u M_s
  e     exp(s - m), m the largest COMPUTED score (a common error of m cancels in every quotient).  The argument carries
        a = E_s + 2 u |s - m|; exp is v_exp_f32 of the argument times log2 e (2 u |s - m| + 2 u); the backward reaches m tile by tile:
        the term meets at most nine factors exp(m' - m''), whose exponents add up to at most |s - m| (2 u |s - m| + 2 u each in the
        worst case, bounded together by 4 u |s - m| + 18 u) and nine products:     r_e = expm1(a) + 8 u |s - m| + 50 u       (relative)
  l     sum_j e: 256 terms.                                                          r_l = (sum e r_e) / l + g(256)            (relative)
  p     e (1 / l): a reciprocal (2 u allowed) and a product.                         r_p = r_e + r_l + 3 u                     (relative)
  out   (sum_j bf16(e) v) / l, 256 terms on the matrix pipe, then ONE rounding to bf16:
            E_out = ((sum_j (e r_e + hb(e (1 + r_e))) |v| + C_ACC g(256) sum_j e |v|) / l + |out| r_l) (1 + 2 r_l) + 4 u |out|
  dp    dout . v: a 64-term dot on the matrix pipe.                                  E_dp = C_ACC g(64) sum_d |dout v|
  c     (sum_j e dp) / l, an fp32 sum of 256 fused terms from the resident e and dp (NOT from a rounded out):
            E_c = sum_j p (r_e |dp| + E_dp) + g(256) sum_j p |dp| + |c| (r_l + 3 u)
  ds    p (dp - c).                                                                  E_ds = p (E_dp + E_c) + |ds| (r_p + 2 u)
  dTh   sum_jx ds, dTw sum_jy ds: 16 terms.                                          E_dT = sum E_ds + g(16) sum |ds|
  dq    scale sum_j bf16(ds) k + sum_jy bf16(dTh) rel_h[.] + sum_jx bf16(dTw) rel_w[.]: 256 + 32 + 32 terms on the matrix pipe, one
        product in between, then ONE rounding to bf16:
            E_dq = |scale| sum_j (E_ds + hb(|ds| + E_ds)) |k| + sum (E_dT + hb(|dT| + E_dT)) |rel|
                   + (C_ACC g(320) + u) (|scale| sum_j |ds k| + sum |dTh rel_h| + sum |dTw rel_w|)
  dk    scale sum_i bf16(ds) q:   E_dk = |scale| (sum_i (E_ds + hb(|ds| + E_ds)) |q| + C_ACC g(256) sum_i |ds q|) + u |dk|
  dv    sum_i bf16(p) dout:       E_dv = sum_i (p r_p + hb(p (1 + r_p))) |dout| + C_ACC g(256) sum_i p |dout|
  dbias sum over (b, window) of ds in fp32 (the slabs, then the caller's sum, taken in fp64 by the tests): n = B * windows terms.
                                  E_dbias = sum E_ds + g(n) sum |ds|
  drel  sum over (b, window, head, i) of bf16(dT) q: 256 terms per (b, window, head) on the matrix pipe, then an fp32 sum over the
        n' = B * windows * heads items in the worst split:
                                  E_drel = sum (E_dT + hb(|dT| + E_dT)) |q| + (C_ACC g(256) + g(n')) sum |dT q|
  fp32 underflow: at hard scores e = exp(s - m) falls below 2^-126, where v_exp_f32 may flush to zero and products round in the
  denormal range.  Every e, p and ds carries an ABSOLUTE t = 2^-125 more, carried through c (t sum |dp|), ds (t |dp - c| + t), out
  (t sum |v|) and dv (t sum |dout|); the terms are below 1e-35 and matter only where everything else is of that size (dbias, fp32).
THE GATE is |got - exact| <= R + E per element, R = half a bf16 ulp at |exact| + E for the bf16 outputs and 0 for the fp32 ones
(dbias, drel); the figure reported is the largest |got - exact| / (R + E), which must stay <= 1, and got is finite wherever exact is."""
import torch

from tests.frameattn_ref import BF16_SENTINEL, U, f32, g, guard_touched, guarded_rows, share  # noqa: F401
from tests.gemm_ref import C_ACC, bf, half_ulp_bf16  # noqa: F401

HD = 64
W = 16
TINY = 2.0 ** -125
N = W * W
_I = torch.arange(N)
IH = (_I[:, None] >> 4) - (_I[None, :] >> 4) + (W - 1)   # [i][j]: iy - jy + 15
IW = (_I[:, None] & 15) - (_I[None, :] & 15) + (W - 1)   # [i][j]: ix - jx + 15


def make_inputs(B, Hg, Wg, heads, seed=0, spread=1.0, bias_mag=1.0, rel_mag=0.25):
    """q, k, v, dout fp64 [B, Hg, Wg, heads, 64], bias [heads, 256, 256], rel_h, rel_w [31, 64], all holding bf16 values.  spread
    scales q and k: scale * q . k has a standard deviation of about spread^2 at scale = 1 / 8."""
    gen = torch.Generator().manual_seed(100000 * seed + 1000 * B + 100 * Hg + 10 * Wg + heads)
    mk = lambda s, *shape: bf(s * torch.randn(*shape, generator=gen, dtype=torch.float64))  # noqa: E731
    q, k = mk(spread, B, Hg, Wg, heads, HD), mk(spread, B, Hg, Wg, heads, HD)
    v, dout = mk(1.0, B, Hg, Wg, heads, HD), mk(1.0, B, Hg, Wg, heads, HD)
    return q, k, v, dout, mk(bias_mag, heads, N, N), mk(rel_mag, 2 * W - 1, HD), mk(rel_mag, 2 * W - 1, HD)


def win(x, swap=False):
    """[B, Hg, Wg, heads, 64] -> [B, nh, nw, heads, 256, 64]: one sequence per (b, window, h), token i = 16 (y % 16) + x % 16
    (swap: i = 16 (x % 16) + y % 16, a mistake)."""
    B, Hg, Wg, heads, hd = x.shape
    x = x.reshape(B, Hg // W, W, Wg // W, W, heads, hd)
    x = x.permute(0, 1, 3, 5, 4, 2, 6) if swap else x.permute(0, 1, 3, 5, 2, 4, 6)
    return x.reshape(B, Hg // W, Wg // W, heads, N, hd)


def unwin(x, swap=False):
    B, nh, nw, heads, _, hd = x.shape
    x = x.reshape(B, nh, nw, heads, W, W, hd)
    x = x.permute(0, 1, 5, 2, 4, 3, 6) if swap else x.permute(0, 1, 4, 2, 5, 3, 6)
    return x.reshape(B, nh * W, nw * W, heads, hd)


def _gather(qr, idx):
    """qr [..., 256, 31] -> [..., 256, 256]: entry (i, j) = qr[..., i, idx[i, j]]."""
    return qr[..., _I[:, None], idx]


def _scatter(ds, idx):
    """ds [..., 256, 256] -> [..., 256, 31]: entry (i, r) = sum_j ds[..., i, j] [idx[i, j] == r]."""
    out = ds.new_zeros(ds.shape[:-1] + (2 * W - 1,))
    return out.scatter_add_(-1, idx.expand(ds.shape), ds)


def _softmax_parts(q, k, bias, rel_h, rel_w, scale):
    qk = torch.einsum("...id,...jd->...ij", q, k)
    s = scale * qk
    M = s.abs()
    E = abs(scale) * C_ACC * g(HD) * torch.einsum("...id,...jd->...ij", q.abs(), k.abs())
    if bias is not None:
        s = s + bias
        M = M + bias.abs()
    if rel_h is not None:
        for rel, idx in ((rel_h, IH), (rel_w, IW)):
            t = _gather(q @ rel.T, idx)
            s = s + t
            M = M + t.abs()
            E = E + C_ACC * g(HD) * _gather(q.abs() @ rel.abs().T, idx)
    E_s = E + 4 * U * M
    m = s.max(dim=-1, keepdim=True).values
    e = torch.exp(s - m)
    r_e = torch.expm1(E_s + 2 * U * (s - m).abs()) + 8 * U * (s - m).abs() + 50 * U
    l = e.sum(dim=-1, keepdim=True)
    r_l = (e * r_e).sum(dim=-1, keepdim=True) / l + g(N)
    p = e / l
    r_p = r_e + r_l + 3 * U
    return e, l, p, r_e, r_l, r_p


def forward_ref(q, k, v, bias, rel_h, rel_w, scale):
    """fp64 [B, Hg, Wg, heads, 64] (bf16 values), scale (the fp32 value) -> {"out": (exact, R, E)}."""
    q, k, v = win(q), win(k), win(v)
    e, l, p, r_e, r_l, _ = _softmax_parts(q, k, bias, rel_h, rel_w, scale)
    out = p @ v
    E = (((e * r_e + half_ulp_bf16(e * (1 + r_e))) @ v.abs() + C_ACC * g(N) * (e @ v.abs())) / l + out.abs() * r_l) * (1 + 2 * r_l) \
        + 4 * U * out.abs() + TINY * v.abs().sum(dim=-2, keepdim=True)
    out, E = unwin(out), unwin(E)
    return {"out": (out, half_ulp_bf16(out.abs() + E), E)}


def backward_ref(q, k, v, dout, bias, rel_h, rel_w, scale):
    """-> {"dq", "dk", "dv": (exact, R, E) [B, Hg, Wg, heads, 64]; "dbias": (exact, 0, E) [heads, 256, 256] when bias is given;
    "drel": (exact, 0, E) [2, 31, 64] when rel_h is given}."""
    q, k, v, do = win(q), win(k), win(v), win(dout)
    B, nh, nw, heads = q.shape[:4]
    e, l, p, r_e, r_l, r_p = _softmax_parts(q, k, bias, rel_h, rel_w, scale)
    dp = do @ v.transpose(-1, -2)
    E_dp = C_ACC * g(HD) * (do.abs() @ v.abs().transpose(-1, -2))
    c = (p * dp).sum(dim=-1, keepdim=True)
    E_c = (p * (r_e * dp.abs() + E_dp)).sum(dim=-1, keepdim=True) + g(N) * (p * dp.abs()).sum(dim=-1, keepdim=True) + c.abs() * (r_l + 3 * U) \
        + TINY * dp.abs().sum(dim=-1, keepdim=True)
    ds = p * (dp - c)
    E_ds = p * (E_dp + E_c) + ds.abs() * (r_p + 2 * U) + TINY * ((dp - c).abs() + 1)
    Eb_ds = E_ds + half_ulp_bf16(ds.abs() + E_ds)      # with the rounding to bf16 in front of a product
    dq = scale * (ds @ k)
    M_dq = abs(scale) * (ds.abs() @ k.abs())
    E_dq = abs(scale) * (Eb_ds @ k.abs())
    res = {}
    if rel_h is not None:
        drel, E_drel = [], []
        for rel, idx in ((rel_h, IH), (rel_w, IW)):
            G = _scatter(ds, idx)
            E_G = _scatter(E_ds, idx) + g(W) * _scatter(ds.abs(), idx)
            Eb_G = E_G + half_ulp_bf16(G.abs() + E_G)
            dq = dq + G @ rel
            M_dq = M_dq + G.abs() @ rel.abs()
            E_dq = E_dq + Eb_G @ rel.abs()
            drel.append(torch.einsum("...ir,...id->rd", G, q))
            E_drel.append(torch.einsum("...ir,...id->rd", Eb_G, q.abs())
                          + (C_ACC * g(N) + g(B * nh * nw * heads)) * torch.einsum("...ir,...id->rd", G.abs(), q.abs()))
        drel, E_drel = torch.stack(drel), torch.stack(E_drel)
        res["drel"] = (drel, torch.zeros_like(drel), E_drel)
    E_dq = E_dq + (C_ACC * g(N + 4 * W) + U) * M_dq
    dk = scale * (ds.transpose(-1, -2) @ q)
    E_dk = abs(scale) * (Eb_ds.transpose(-1, -2) @ q.abs() + C_ACC * g(N) * (ds.abs().transpose(-1, -2) @ q.abs())) + U * dk.abs()
    dv = p.transpose(-1, -2) @ do
    E_dv = (p * r_p + half_ulp_bf16(p * (1 + r_p))).transpose(-1, -2) @ do.abs() + C_ACC * g(N) * (p.transpose(-1, -2) @ do.abs()) \
        + TINY * do.abs().sum(dim=-2, keepdim=True)
    for name, exact, E in (("dq", dq, E_dq), ("dk", dk, E_dk), ("dv", dv, E_dv)):
        exact, E = unwin(exact), unwin(E)
        res[name] = (exact, half_ulp_bf16(exact.abs() + E), E)
    if bias is not None:
        dbias = ds.sum(dim=(0, 1, 2))
        E_dbias = E_ds.sum(dim=(0, 1, 2)) + g(B * nh * nw) * ds.abs().sum(dim=(0, 1, 2))
        res["dbias"] = (dbias, torch.zeros_like(dbias), E_dbias)
    return res


# ---- an fp32 restatement of the kernels' arithmetic, and six wrong variants --------------------------------------------------------------
VARIANTS = ("swap_yx", "rel_scaled_q", "rel_negated", "no_dT_in_dq", "neighbour_head_bias", "c_from_out")


def restate_fp32(q, k, v, dout, bias, rel_h, rel_w, scale, variant=None):
    """q, k, v, dout: [B, Hg, Wg, heads, 64] (bf16 values, any float dtype).  fp32 arithmetic with the kernels' roundings to bf16 (e
    before e v, p before p^T dout, ds before its products, dTh / dTw before theirs, each output once) -> out, dq, dk, dv as fp64
    [B, Hg, Wg, heads, 64] holding bf16 values, dbias and drel as fp64 holding fp32 values.  variant: None, or one of VARIANTS, the
    mistakes the budget must catch: the in-window index taken as 16 ix + iy; the decomposed term taken from the scaled q; the relative
    index negated (jy - iy + 15); dTh and dTw left out of dq; the bias of the neighbouring head; c taken from the bf16-rounded out."""
    swap = variant == "swap_yx"
    rb = lambda t: t.to(torch.bfloat16).float()  # noqa: E731
    qs, ks, vs, dos = (win(t.float(), swap) for t in (q, k, v, dout))
    sc = torch.tensor(scale, dtype=torch.float32)
    ih, iw = (2 * (W - 1) - IH, 2 * (W - 1) - IW) if variant == "rel_negated" else (IH, IW)
    s = sc * (qs @ ks.transpose(-1, -2))
    if bias is not None:
        b = bias.float()
        s = s + (b.roll(-1, 0) if variant == "neighbour_head_bias" else b)
    if rel_h is not None:
        qr = sc * qs if variant == "rel_scaled_q" else qs
        s = s + _gather(qr @ rel_h.float().T, ih) + _gather(qr @ rel_w.float().T, iw)
    e = torch.exp(s - s.max(dim=-1, keepdim=True).values)
    l = e.sum(dim=-1, keepdim=True)
    inv = 1.0 / l
    out = (rb(e) @ vs) * inv
    p = e * inv
    dp = dos @ vs.transpose(-1, -2)
    c = (dos * rb(out)).sum(dim=-1, keepdim=True) if variant == "c_from_out" else (p * dp).sum(dim=-1, keepdim=True)
    ds = p * (dp - c)
    dq = sc * (rb(ds) @ ks)
    drel = None
    if rel_h is not None:
        Gh, Gw = _scatter(ds, ih), _scatter(ds, iw)
        if variant != "no_dT_in_dq":
            dq = dq + rb(Gh) @ rel_h.float() + rb(Gw) @ rel_w.float()
        drel = torch.stack([torch.einsum("...ir,...id->rd", rb(G), qs) for G in (Gh, Gw)]).double()
    dk = sc * (rb(ds).transpose(-1, -2) @ qs)
    dv = rb(p).transpose(-1, -2) @ dos
    res = {n: bf(unwin(t, swap).double()) for n, t in (("out", out), ("dq", dq), ("dk", dk), ("dv", dv))}
    if bias is not None:
        db = ds.sum(dim=(0, 1, 2))
        res["dbias"] = (db.roll(1, 0) if variant == "neighbour_head_bias" else db).double()
    if drel is not None:
        res["drel"] = drel
    return res


def rows(x):
    """[B, Hg, Wg, heads, 64] -> the kernels' rows [B * Hg * Wg, heads * 64]."""
    B, Hg, Wg, heads, hd = x.shape
    return x.reshape(B * Hg * Wg, heads * hd)


def shares(got, ref):
    """{name: largest observed / allowed} over the outputs both dicts hold."""
    return {n: share(got[n], ref[n]) for n in ref if n in got}
