"""Tests of the instrument behind tests/test_attention_fp64_gpu.py (tests/attention_ref.py); no GPU needed.

* attn_exact against autograd on the formula of the op tests (softmax(q k^T scale + bias, -inf on masked keys) v) in fp64,
  and against the oracle's attention (oracle/onepeace_oracle.py: self_attention).
* the rounding model inside the gate for every input family x pad pattern, with finite results everywhere.
* every mutant of the model outside the gate, under the margins the GPU file uses:
    a drop_last_key_ds          the last valid key's dS dropped for one (sample, head)
    b attend_first_padded       the first masked key attended in one sample
    c skip_rescale              the running-max rescale of the last key tile skipped for one 16-query block
    d bias_block_transposed     one 16 x 32 bias block read transposed
    e delta_neighbour_head      delta taken from the neighbouring head
    f dbias_last_chunk_missing  the last (partial) batch chunk missing from the summed dbias
    g lse_without_bias          lse missing the bias term for one 16-query block
  A mutant that passed would mean the inputs or the norm cannot see that class of bug."""
import pytest
import torch

from oracle import onepeace_oracle as O
from tests import attention_ref as R

F64_EPS = 2.0 ** -52


def _case(family, pad_name, S, B=3, heads=2, per_sample=False):
    pad = R.make_pad(pad_name, B, S)
    assert pad is not None or pad_name == "none", "pattern %s needs a longer sequence than %d" % (pad_name, S)
    q, k, v, bias, dout = R.make_inputs(family, B, heads, S, pad, per_sample_bias=per_sample)
    return q, k, v, bias, pad, dout


def _autograd(q, k, v, bias, pad, dout, scale):
    q, k, v = (t.double().requires_grad_(True) for t in (q, k, v))
    bias = bias.double().requires_grad_(True)
    s = (q * scale) @ k.transpose(-1, -2) + (bias[None] if bias.dim() == 3 else bias)
    if pad is not None:
        s = s.masked_fill(pad[:, None, None, :], float("-inf"))
    out = torch.softmax(s, dim=-1) @ v
    lse = torch.logsumexp(s, dim=-1)
    out.backward(dout.double())
    return {"out": out.detach(), "lse": lse.detach(), "dq": q.grad, "dk": k.grad, "dv": v.grad, "dbias": bias.grad}


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("pad_name", ["none", "tail", "hole"])
@pytest.mark.parametrize("family", ["unit", "peaked", "offset"])
def test_exact_matches_autograd(family, pad_name, per_sample):
    q, k, v, bias, pad, dout = _case(family, pad_name, 97, per_sample=per_sample)
    ex = R.attn_exact(q, k, v, bias, pad, dout, R.SCALE)
    ref = _autograd(q, k, v, bias, pad, dout, R.SCALE)
    for kind in R.KINDS:
        # sums of <= 97 (dbias: 3) products in fp64, two different association orders: a few ulps of the largest entry each
        tol = 64 * F64_EPS * float(ref[kind].abs().max())
        assert float((ex[kind] - ref[kind]).abs().max()) <= tol, kind


def test_exact_matches_oracle_attention():
    """oracle self_attention with identity out_proj and no sub-LayerNorm is softmax(q k^T / 8 + bias) v on the projected q, k, v.
    The oracle takes its softmax in fp32 (s.float(), as the reference model does), so agreement is to fp32 roundoff of P, not fp64."""
    S, B, heads = 50, 2, 2
    H = heads * R.HD
    g = torch.Generator().manual_seed(3)
    x = torch.randn(S, B, H, generator=g, dtype=torch.float64)
    sd = {"a.%s_proj.weight" % n: torch.randn(H, H, generator=g, dtype=torch.float64) / H ** 0.5 for n in "qkv"}
    sd["a.q_proj.bias"] = torch.randn(H, generator=g, dtype=torch.float64)
    sd["a.v_proj.bias"] = torch.randn(H, generator=g, dtype=torch.float64)
    sd["a.out_proj.weight"] = torch.eye(H, dtype=torch.float64)
    sd["a.out_proj.bias"] = torch.zeros(H, dtype=torch.float64)
    pad = R.make_pad("tail", B, S)
    bias = torch.randn(heads, S, S, generator=g, dtype=torch.float64)
    full = bias[None].expand(B, -1, -1, -1).masked_fill(pad[:, None, None, :], float("-inf"))
    ref = O.self_attention(x, sd, "a", heads, bias=full)                      # [S, B, H]
    hd = lambda t: t.reshape(S, B, heads, R.HD).permute(1, 2, 0, 3)
    q = hd(O.linear(x, sd["a.q_proj.weight"], sd["a.q_proj.bias"]))
    k = hd(O.linear(x, sd["a.k_proj.weight"]))
    v = hd(O.linear(x, sd["a.v_proj.weight"], sd["a.v_proj.bias"]))
    ex = R.attn_exact(q, k, v, bias, pad, torch.zeros_like(q), R.SCALE)
    got = ex["out"].permute(2, 0, 1, 3).reshape(S, B, H)
    # every P entry carries <= a few fp32 ulps relative error in the oracle; out is a convex combination of |v| <= max|v|
    assert float((got - ref).abs().max()) <= 8 * R.U32 * float(v.abs().max())


@pytest.mark.parametrize("S", [64, 257, 321])
@pytest.mark.parametrize("pad_name", R.PADS)
@pytest.mark.parametrize("family", R.FAMILIES)
def test_rounding_model_is_inside_the_gate(family, pad_name, S):
    q, k, v, bias, pad, dout = _case(family, pad_name, S)
    ex = R.attn_exact(q, k, v, bias, pad, dout)
    md = R.attn_rounding_model(q, k, v, bias, pad, dout)
    for kind in R.KINDS:   # the finite-value condition (offset, bias_dominant: no overflow in exp), for every family
        assert bool(torch.isfinite(ex[kind]).all()) and bool(torch.isfinite(md[kind]).all()), kind
    failures, _ = R.gate(md, ex, md)
    assert not failures, failures
    if pad_name == "one_valid":
        # closed form: P = 1 on the one valid key, so out = v[key], dS = P (dout . v - dout . out) = 0 exactly: dq = dk = 0, and
        # dv[key] = the column sum of dout, 0 elsewhere -- in the model up to ITS bf16 rounding of dv and nothing else
        for r in (ex, md):
            assert float(r["dq"].abs().max()) == 0.0 and float(r["dk"].abs().max()) == 0.0
        want = torch.zeros_like(ex["dv"])
        for b in range(pad.shape[0]):
            key = int((~pad[b]).nonzero()[0])
            want[b, :, key] = dout[b].double().sum(-2)
            assert torch.equal(ex["out"][b], v[b, :, key].double()[:, None, :].expand(-1, S, -1))
        assert float((ex["dv"] - want).abs().max()) <= 8 * F64_EPS * float(want.abs().max())
        assert torch.equal(md["dv"], R.bf(ex["dv"]))


MUTANT_CASES = [("drop_last_key_ds", "unit"), ("drop_last_key_ds", "peaked"), ("attend_first_padded", "edge_pad"),
                ("skip_rescale", "ascending"), ("bias_block_transposed", "bias_dominant"), ("delta_neighbour_head", "unit"),
                ("delta_neighbour_head", "peaked"), ("dbias_last_chunk_missing", "unit"), ("dbias_last_chunk_missing", "peaked"),
                ("lse_without_bias", "bias_dominant")]


@pytest.mark.parametrize("mutant,family,S", [(m, f, S) for m, f in MUTANT_CASES for S in (64, 257, 321)
                                             if not (m == "skip_rescale" and S <= 64)])   # (one key tile: no rescale to skip)
def test_every_mutant_fails_the_gate(mutant, family, S):
    q, k, v, bias, pad, dout = _case(family, "tail", S)
    ex = R.attn_exact(q, k, v, bias, pad, dout)
    md = R.attn_rounding_model(q, k, v, bias, pad, dout)
    mu = R.attn_rounding_model(q, k, v, bias, pad, dout, mutant=mutant, chunk=2)
    failures, _ = R.gate(mu, ex, md)
    assert failures, "mutant %s passes the gate on %s, S = %d (margins %s)" % (mutant, family, S, R.MARGINS)
