"""Temporal attention without a GPU: ops.temporal_attention_torch against the reference's arrangement (explicit rearranges + the core of
MultiheadAttention.forward, onepeace.py:234-247 as called from :331-337) in fp64, values and gradients; the fp64 reference and budget of
tests/frameattn_ref.py against torch.autograd and against an fp32 restatement of the kernels' arithmetic, with three wrong variants the
budget must catch; the ABI symbols and the entries' limit checks (which run before the device is touched)."""
import ctypes

import pytest
import torch

from tests import frameattn_ref as FR

try:  # the reference's own tool; without it the same two index maps as views
    from einops import rearrange
except ImportError:
    def rearrange(x, pattern, **sizes):
        if pattern == "n (b t) d -> t (b n) d":
            n, bt, d = x.shape
            return x.view(n, bt // sizes["t"], sizes["t"], d).permute(2, 1, 0, 3).reshape(sizes["t"], -1, d)
        assert pattern == "t (b n) d -> n (b t) d"
        t, bn, d = x.shape
        return x.view(t, bn // sizes["n"], sizes["n"], d).permute(2, 1, 0, 3).reshape(sizes["n"], -1, d)


def _reference_arrangement(x_qkv, B, T, N, heads, scaling):
    """onepeace.py on the reference's own layout.  x_qkv: [N, B * T, 3 H] -- the packed projections of the layer's x [n, (b t), d] -- is
    rearranged as :331 does, run through :234-247 (views, q *= scaling, bmm, softmax, bmm, transpose back) and rearranged back as :337."""
    H = x_qkv.shape[-1] // 3
    hd = H // heads
    xt = rearrange(x_qkv, "n (b t) d -> t (b n) d", t=T)
    tgt_len, bsz, _ = xt.shape
    q, k, v = (xt[..., i * H:(i + 1) * H].contiguous().view(tgt_len, bsz * heads, hd).transpose(0, 1) for i in range(3))
    q = q * scaling
    w = torch.softmax(torch.bmm(q, k.transpose(1, 2)), dim=-1)
    attn = torch.bmm(w, v).transpose(0, 1).contiguous().view(tgt_len, bsz, H)
    return rearrange(attn, "t (b n) d -> n (b t) d", n=N)


@pytest.mark.parametrize("B,T,N,heads,hd", [(2, 4, 3, 2, 8), (1, 5, 2, 3, 16), (3, 1, 4, 1, 64)])
def test_torch_statement_is_the_reference_arrangement_in_fp64(B, T, N, heads, hd):
    from one_peace_amd import ops
    torch.manual_seed(B * 100 + T)
    H = heads * hd
    qkv = torch.randn(B * T * N, 3 * H, dtype=torch.float64, requires_grad=True)      # the project's rows (b, t, n)
    cot = torch.randn(B * T * N, H, dtype=torch.float64)
    got = ops.temporal_attention_torch(qkv, B, T, N, heads)
    assert ops.temporal_attention(qkv, B, T, N, heads).equal(got)                      # fp64 on the CPU takes the torch route
    (dgot,) = torch.autograd.grad((got * cot).sum(), qkv)
    ref_in = qkv.detach().view(B * T, N, 3 * H).transpose(0, 1).clone().requires_grad_(True)   # [n, (b t), 3 H]
    want = _reference_arrangement(ref_in, B, T, N, heads, hd ** -0.5)
    (dwant,) = torch.autograd.grad((want * cot.view(B * T, N, H).transpose(0, 1)).sum(), ref_in)
    assert (got.view(B * T, N, H).transpose(0, 1) - want).abs().max() <= 1e-12
    assert (dgot.view(B * T, N, 3 * H).transpose(0, 1) - dwant).abs().max() <= 1e-12
    with pytest.raises(ValueError):
        ops.temporal_attention(qkv, B, T + 1, N, heads)


def test_fp64_reference_agrees_with_autograd():
    from one_peace_amd import ops
    B, T, N, heads = 2, 5, 3, 2
    q, k, v, dout = FR.make_inputs(B, T, N, heads, seed=1)
    qkv = torch.cat([FR.rows(q), FR.rows(k), FR.rows(v)], dim=1).requires_grad_(True)
    out = ops.temporal_attention_torch(qkv, B, T, N, heads, 0.125)
    (d,) = torch.autograd.grad((out * FR.rows(dout)).sum(), qkv)
    H = heads * 64
    fwd, bwd = FR.forward_ref(q, k, v, 0.125), FR.backward_ref(q, k, v, dout, 0.125)
    assert (out.detach() - FR.rows(fwd["out"][0])).abs().max() <= 1e-12
    for i, name in enumerate(("dq", "dk", "dv")):
        assert (d[:, i * H:(i + 1) * H] - FR.rows(bwd[name][0])).abs().max() <= 1e-12, name


CASES = [dict(B=2, T=16, N=5, heads=3, spread=1.0, scale=0.125), dict(B=1, T=32, N=3, heads=2, spread=2.8, scale=0.125),
         dict(B=2, T=7, N=4, heads=2, spread=1.5, scale=0.3)]


@pytest.fixture(scope="module", params=range(len(CASES)))
def case(request):
    c = dict(CASES[request.param])
    q, k, v, dout = FR.make_inputs(c["B"], c["T"], c["N"], c["heads"], seed=3 + request.param, spread=c["spread"])
    scale = FR.f32(c["scale"])
    c.update(q=q, k=k, v=v, dout=dout, scale=scale, ref=dict(FR.forward_ref(q, k, v, scale), **FR.backward_ref(q, k, v, dout, scale)))
    return c


def _restated(c, variant=None):
    return FR.restate_fp32(FR.rows(c["q"]), FR.rows(c["k"]), FR.rows(c["v"]), FR.rows(c["dout"]), c["scale"], c["B"], c["T"], c["N"],
                           c["heads"], variant)


def test_fp32_restatement_stays_inside_the_budget(case):
    got = _restated(case)
    for name in ("out", "dq", "dk", "dv"):
        assert FR.share(got[name], case["ref"][name]) <= 1.0, (name, FR.share(got[name], case["ref"][name]))


@pytest.mark.parametrize("variant", ["swapped_strides", "no_scale", "p_bf16"])
def test_wrong_variants_leave_the_budget(case, variant):
    got = _restated(case, variant)
    shares = {name: FR.share(got[name], case["ref"][name]) for name in ("out", "dq", "dk", "dv")}
    assert shares["out"] > 1.0, shares
    assert all(s > 1.0 for s in shares.values()), shares


def test_abi_symbols_and_limits_without_a_device():
    from one_peace_amd import hip
    L = hip.lib()
    for name in ("op_attn_frames_fwd", "op_attn_frames_bwd"):
        assert getattr(L, name) is not None and name in hip.SIGNATURES
    assert L.op_abi_version() == 10
    EINVAL = -22
    buf = ctypes.create_string_buffer(4096 + 16)
    a = (ctypes.addressof(buf) + 15) & ~15          # a 16-byte aligned host address: the checks come before anything is launched
    P = ctypes.c_void_p

    def fwd(q=a, k=a, v=a, ld=192, out=a, ldo=64, B=1, T=4, N=2, heads=1, hd=64):
        return L.op_attn_frames_fwd(P(q), P(k), P(v), ld, P(out), ldo, B, T, N, heads, hd, 0.125, None)

    def bwd(dq=a, ldg=192, ldo=64, T=4, hd=64, dout=a):
        return L.op_attn_frames_bwd(P(a), P(a), P(a), 192, P(dout), ldo, P(dq), P(a), P(a), ldg, 1, T, 2, 1, hd, 0.125, None)
    assert fwd(B=0) == 0 and L.op_attn_frames_bwd(P(a), P(a), P(a), 192, P(a), 64, P(a), P(a), P(a), 192, 0, 4, 2, 1, 64, 0.125, None) == 0
    bad = [fwd(hd=32), fwd(hd=128), fwd(T=0), fwd(T=33), fwd(N=0), fwd(heads=0), fwd(B=-1), fwd(ld=190), fwd(ld=56), fwd(ldo=60),
           fwd(ldo=56), fwd(heads=2, ld=64), fwd(q=a + 2), fwd(v=a + 8), fwd(out=a + 4), fwd(q=None), fwd(out=None),
           fwd(B=1 << 20, N=1 << 10, heads=2), bwd(hd=8), bwd(T=40), bwd(ldg=60), bwd(ldg=66), bwd(ldo=8), bwd(dq=a + 2), bwd(dq=None),
           bwd(dout=a + 6)]
    assert all(rc == EINVAL for rc in bad), bad
    assert fwd(B=1 << 20, N=1 << 10, heads=2) == EINVAL and b"2^31" in L.op_last_error()
    fwd(T=33)
    assert b"T = 33" in L.op_last_error()
