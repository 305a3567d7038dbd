"""Window attention without a GPU: ops.window_attention_torch against a direct restatement of detectron2's window_partition / padding /
window_unpartition around the core of det/models/onepeace.py:197-213, values and gradients, on grids that need padding in both axes and
for window sizes 4 and 16; the fp64 reference and budget of tests/windowattn_ref.py against torch.autograd and against an fp32
restatement of the kernels' arithmetic, with six wrong variants the budget must catch; the ABI symbols and the entries' limit checks
(which run before the device is touched)."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

from tests import windowattn_ref as WR


def _partition(x, w):
    """detectron2's window_partition: [B, H, W, C] -> [B * windows, w, w, C], zero padding at the bottom and the right."""
    B, H, Wd, C = x.shape
    ph, pw = (w - H % w) % w, (w - Wd % w) % w
    if ph or pw:
        x = F.pad(x, (0, 0, 0, pw, 0, ph))
    Hp, Wp = H + ph, Wd + pw
    x = x.view(B, Hp // w, w, Wp // w, w, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, w, w, C), (Hp, Wp)


def _unpartition(win, w, pad_hw, hw):
    Hp, Wp = pad_hw
    H, Wd = hw
    B = win.shape[0] // (Hp * Wp // w // w)
    x = win.view(B, Hp // w, Wp // w, w, w, -1).permute(0, 1, 3, 2, 4, 5).contiguous().view(B, Hp, Wp, -1)
    return x[:, :H, :Wd].contiguous()


def _get_rel_pos(size, rel_pos):
    """detectron2's get_rel_pos for q_size == k_size and a table of 2 * size - 1 rows (no interpolation)."""
    c = torch.arange(size)
    return rel_pos[(c[:, None] - c[None, :]) + (size - 1)]


def _direct(x, wq, bq, wk, wv, bv, bias, rel_h, rel_w, heads, w):
    """The reference's window block between the first LayerNorm and the sub-LayerNorm on ITS layout: the normed map x [B, H, W, D] is
    padded and partitioned, projected (so a padded token gets q = bq, k = 0, v = bv), and run through :197-213 with the window bias
    expanded as :398-401 and add_decomposed_rel_pos restated; then unpartitioned and cropped."""
    B, H, Wd, D = x.shape
    xw, pad_hw = _partition(x, w)
    Bw, hd, L = xw.shape[0], D // heads, w * w
    proj = lambda wt, b: F.linear(xw, wt, b).reshape(Bw, L, heads, hd).permute(0, 2, 1, 3).reshape(Bw * heads, L, hd)  # noqa: E731
    q, k, v = proj(wq, bq), proj(wk, None), proj(wv, bv)
    attn = (q * hd ** -0.5) @ k.transpose(-2, -1)
    if bias is not None:
        attn = attn + bias.unsqueeze(0).expand(Bw, -1, -1, -1).reshape(-1, L, L)
    if rel_h is not None:
        Rh, Rw = _get_rel_pos(w, rel_h), _get_rel_pos(w, rel_w)
        r_q = q.reshape(Bw * heads, w, w, hd)
        th = torch.einsum("bhwc,hkc->bhwk", r_q, Rh)
        tw = torch.einsum("bhwc,wkc->bhwk", r_q, Rw)
        attn = (attn.view(-1, w, w, w, w) + th[:, :, :, :, None] + tw[:, :, :, None, :]).view(-1, L, L)
    a = attn.softmax(dim=-1) @ v
    a = a.view(Bw, heads, w, w, hd).permute(0, 2, 3, 1, 4).reshape(Bw, w, w, D)
    return _unpartition(a, w, pad_hw, (H, Wd))


@pytest.mark.parametrize("B,Hg,Wg,heads,hd,w,tables", [(1, 20, 24, 2, 8, 16, "both"), (2, 20, 24, 2, 8, 4, "both"), (1, 32, 16, 1, 16, 16, "both"),
                                                       (1, 10, 7, 3, 4, 4, "bias"), (2, 8, 12, 2, 8, 4, "rel"), (1, 9, 9, 1, 8, 4, "none")])
def test_torch_statement_is_the_reference_arrangement_in_fp64(B, Hg, Wg, heads, hd, w, tables):
    from one_peace_amd import ops
    torch.manual_seed(B * 100 + Hg + w)
    D = heads * hd
    mk = lambda *s: torch.randn(*s, dtype=torch.float64, requires_grad=True)  # noqa: E731
    x, wq, bq, wk, wv, bv = mk(B, Hg, Wg, D), mk(D, D), mk(D), mk(D, D), mk(D, D), mk(D)
    bias = mk(heads, w * w, w * w) if tables in ("both", "bias") else None
    rel_h, rel_w = (mk(2 * w - 1, hd), mk(2 * w - 1, hd)) if tables in ("both", "rel") else (None, None)
    leaves = [t for t in (x, wq, bq, wk, wv, bv, bias, rel_h, rel_w) if t is not None]
    cot = torch.randn(B, Hg, Wg, D, dtype=torch.float64)
    want = _direct(x, wq, bq, wk, wv, bv, bias, rel_h, rel_w, heads, w)
    dwant = torch.autograd.grad((want * cot).sum(), leaves)
    # the project's statement: the packed projection of the rows, and the projection of a zero row for the padded positions
    qkv = F.linear(x.reshape(B * Hg * Wg, D), torch.cat([wq, wk, wv]), torch.cat([bq, torch.zeros_like(bq), bv]))
    pad_row = torch.cat([bq, torch.zeros_like(bq), bv])
    got = ops.window_attention_torch(qkv, bias, rel_h, rel_w, B, Hg, Wg, heads, w, pad_row=pad_row)
    assert ops.window_attention(qkv, bias, rel_h, rel_w, B, Hg, Wg, heads, w, pad_row=pad_row).equal(got)   # fp64 on the CPU: torch route
    dgot = torch.autograd.grad((got * cot.reshape(-1, D)).sum(), leaves)
    assert (got.view(B, Hg, Wg, D) - want).abs().max() <= 1e-11
    for a, b in zip(dgot, dwant):
        assert (a - b).abs().max() <= 1e-10 * max(1.0, float(b.abs().max()))
    with pytest.raises(ValueError):
        ops.window_attention(qkv, bias, rel_h, rel_w, B, Hg + 1, Wg, heads, w)


def test_padding_defaults_to_a_zero_row_and_other_dtypes_run():
    from one_peace_amd import ops
    torch.manual_seed(3)
    B, Hg, Wg, heads, hd, w = 1, 6, 5, 2, 8, 4
    qkv = torch.randn(B * Hg * Wg, 3 * heads * hd, dtype=torch.float64)
    bias, rel = torch.randn(heads, 16, 16, dtype=torch.float64), torch.randn(7, hd, dtype=torch.float64)
    a = ops.window_attention_torch(qkv, bias, rel, rel, B, Hg, Wg, heads, w)
    b = ops.window_attention_torch(qkv, bias, rel, rel, B, Hg, Wg, heads, w, pad_row=torch.zeros(3 * heads * hd, dtype=torch.float64))
    assert a.equal(b)
    for dt, tol in ((torch.float32, 1e-5), (torch.float16, 2e-2)):
        c = ops.window_attention(qkv.to(dt), bias.to(dt), rel.to(dt), rel.to(dt), B, Hg, Wg, heads, w)
        assert c.dtype == dt and (c.double() - a).abs().max() <= tol * max(1.0, float(a.abs().max()))


def test_fp64_reference_agrees_with_autograd():
    from one_peace_amd import ops
    B, Hg, Wg, heads = 2, 16, 32, 2
    q, k, v, dout, bias, rel_h, rel_w = WR.make_inputs(B, Hg, Wg, heads, seed=1)
    qkv = torch.cat([WR.rows(q), WR.rows(k), WR.rows(v)], dim=1).requires_grad_(True)
    bias, rel_h, rel_w = (t.clone().requires_grad_(True) for t in (bias, rel_h, rel_w))
    out = ops.window_attention_torch(qkv, bias, rel_h, rel_w, B, Hg, Wg, heads, 16, 0.125)
    d, db, dh, dw = torch.autograd.grad((out * WR.rows(dout)).sum(), (qkv, bias, rel_h, rel_w))
    H = heads * 64
    det = lambda t: t.detach()  # noqa: E731
    fwd = WR.forward_ref(q, k, v, det(bias), det(rel_h), det(rel_w), 0.125)
    bwd = WR.backward_ref(q, k, v, dout, det(bias), det(rel_h), det(rel_w), 0.125)
    assert (out.detach() - WR.rows(fwd["out"][0])).abs().max() <= 1e-12
    for i, name in enumerate(("dq", "dk", "dv")):
        assert (d[:, i * H:(i + 1) * H] - WR.rows(bwd[name][0])).abs().max() <= 1e-11, name
    assert (db - bwd["dbias"][0]).abs().max() <= 1e-11
    assert (torch.stack([dh, dw]) - bwd["drel"][0]).abs().max() <= 1e-10


# a 32 x 32 grid (four windows), two heads: ordinary scores; hard scores (about +-60) with a bias of magnitude about 30; another scale
CASES = [dict(B=1, heads=2, spread=1.0, scale=0.125, bias_mag=1.0), dict(B=1, heads=2, spread=2.8, scale=0.125, bias_mag=30.0),
         dict(B=2, heads=2, spread=1.5, scale=0.3, bias_mag=4.0)]


@pytest.fixture(scope="module", params=range(len(CASES)))
def case(request):
    c = dict(CASES[request.param])
    q, k, v, dout, bias, rel_h, rel_w = WR.make_inputs(c["B"], 32, 32, c["heads"], seed=3 + request.param, spread=c["spread"],
                                                       bias_mag=c["bias_mag"])
    scale = WR.f32(c["scale"])
    c.update(q=q, k=k, v=v, dout=dout, bias=bias, rel_h=rel_h, rel_w=rel_w, scale=scale,
             ref=dict(WR.forward_ref(q, k, v, bias, rel_h, rel_w, scale), **WR.backward_ref(q, k, v, dout, bias, rel_h, rel_w, scale)))
    return c


def _restated(c, variant=None):
    return WR.restate_fp32(c["q"], c["k"], c["v"], c["dout"], c["bias"], c["rel_h"], c["rel_w"], c["scale"], variant)


def test_fp32_restatement_stays_inside_the_budget(case):
    shares = WR.shares(_restated(case), case["ref"])
    assert set(shares) == {"out", "dq", "dk", "dv", "dbias", "drel"}
    assert all(s <= 1.0 for s in shares.values()), shares


def test_restatement_without_tables_stays_inside_the_budget():
    q, k, v, dout, bias, rel_h, rel_w = WR.make_inputs(1, 16, 32, 1, seed=9)
    for b, rh, rw in ((None, None, None), (bias, None, None), (None, rel_h, rel_w)):
        ref = dict(WR.forward_ref(q, k, v, b, rh, rw, 0.125), **WR.backward_ref(q, k, v, dout, b, rh, rw, 0.125))
        shares = WR.shares(WR.restate_fp32(q, k, v, dout, b, rh, rw, 0.125), ref)
        assert ("dbias" in shares) == (b is not None) and ("drel" in shares) == (rh is not None)
        assert all(s <= 1.0 for s in shares.values()), shares


@pytest.mark.parametrize("variant", WR.VARIANTS)
def test_wrong_variants_leave_the_budget(case, variant):
    shares = WR.shares(_restated(case, variant), case["ref"])
    assert max(shares.values()) > 1.0, shares
    must = {"swap_yx": ("out", "dq", "dk", "dv"), "rel_scaled_q": ("out",), "rel_negated": ("out",), "no_dT_in_dq": ("dq",),
            "neighbour_head_bias": ("out", "dbias"), "c_from_out": ("dq", "dk")}[variant]
    assert all(shares[n] > 1.0 for n in must), shares


def test_abi_symbols_and_limits_without_a_device():
    from one_peace_amd import hip
    L = hip.lib()
    for name in ("op_attn_window_fwd", "op_attn_window_bwd", "op_attn_window_parts"):
        assert getattr(L, name) is not None and name in hip.SIGNATURES
    assert L.op_abi_version() == 10
    EINVAL = -22
    buf = ctypes.create_string_buffer(4096 + 16)
    a = (ctypes.addressof(buf) + 15) & ~15          # a 16-byte aligned host address: the checks come before anything is launched
    P = ctypes.c_void_p

    def fwd(q=a, k=a, v=a, ld=192, bias=a, rel_h=a, rel_w=a, out=a, ldo=64, B=1, Hg=16, Wg=16, heads=1, hd=64, window=16):
        return L.op_attn_window_fwd(P(q), P(k), P(v), ld, P(bias), P(rel_h), P(rel_w), P(out), ldo, B, Hg, Wg, heads, hd, window, 0.125, None)

    def bwd(dq=a, ldg=192, ldo=64, Hg=16, hd=64, dout=a, drel=None, slabs=None, rel_w=a, B=1):
        return L.op_attn_window_bwd(P(a), P(a), P(a), 192, P(a), P(a), P(rel_w), P(dout), ldo, P(dq), P(a), P(a), ldg, P(drel), P(slabs),
                                    B, Hg, 16, 1, hd, 16, 0.125, None)
    assert fwd(B=0) == 0 and bwd(B=0) == 0 and fwd(B=0, bias=None, rel_h=None, rel_w=None) == 0
    bad = [fwd(hd=32), fwd(hd=128), fwd(window=8), fwd(window=14), fwd(Hg=20), fwd(Wg=24), fwd(Hg=0), fwd(heads=0), fwd(B=-1), fwd(ld=190),
           fwd(ld=56), fwd(ldo=60), fwd(ldo=56), fwd(heads=2, ld=64), fwd(q=a + 2), fwd(v=a + 8), fwd(out=a + 4), fwd(bias=a + 8),
           fwd(rel_h=a + 2), fwd(q=None), fwd(out=None), fwd(rel_h=None), fwd(rel_w=None), fwd(B=1 << 20, Hg=1 << 9, Wg=1 << 9, heads=2),
           bwd(hd=8), bwd(Hg=40), bwd(ldg=60), bwd(ldg=66), bwd(ldo=8), bwd(dq=a + 2), bwd(dq=None), bwd(dout=a + 6), bwd(drel=a + 4),
           bwd(slabs=a + 8), bwd(rel_w=None)]
    assert all(rc == EINVAL for rc in bad), bad
    assert fwd(B=1 << 20, Hg=1 << 9, Wg=1 << 9, heads=2) == EINVAL and b"2^31" in L.op_last_error()
    fwd(Hg=20)
    assert b"20 x 16" in L.op_last_error()
    # the shares: none empty, the same for every call with the same (B, windows, heads)
    for B, windows, heads in ((1, 1, 1), (1, 25, 24), (2, 25, 24), (1, 4, 3), (7, 1, 300)):
        assert hip.attn_window_parts(B, 16, 16 * windows, heads) == hip.attn_window_parts(B, 16 * windows, 16, heads)
        parts, slabs = hip.attn_window_parts(B, 16, 16 * windows, heads)
        per = -(-B * windows // slabs)
        assert parts == slabs * heads and 1 <= slabs <= B * windows and (slabs - 1) * per < B * windows
