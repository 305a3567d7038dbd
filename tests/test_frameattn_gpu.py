"""op_attn_frames_fwd / op_attn_frames_bwd (csrc/frameattn.hip) on the MI355X against the fp64 restatement and the derived per-element
budget of tests/frameattn_ref.py: every output of every shape, on the packed row stride and on a padded one, inside NaN-guarded buffers
(dq | dk | dv pre-filled with the sentinel: every element must be written, nothing around them touched); hard scores (about +-60) and
all-equal scores; bit-equal reruns; the bits of a sequence unchanged when B, N or heads grow around it; the autograd function of
ops.temporal_attention and its torch route.  The largest observed / allowed ratio per output goes to frameattn_fp64_report.txt in the
tests' output directory.

MEASURED on the MI355X (profiles/frameattn_fp64_report.txt, one line per T of the first test and per kind of the second): largest ratio
0.991 (dv at T = 3; a rounding next to a midpoint of the bf16 outputs), 0.884 at hard scores, exactly 0 at T = 1 (p = 1: out = v,
dv = dout, dq = dk = 0)."""
import os

import pytest
import torch

from tests import frameattn_ref as FR
from tests.util import OUT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPORT = os.path.join(OUT, "frameattn_fp64_report.txt")
SCALE = 0.125
# T: a single frame (p = 1), two, an odd count inside the 8-frame tile, a full 8-frame tile, one past the 16-frame tile (the 32-frame
# tile half empty), the largest.  N, B, heads: one, odd counts; heads = 3 leaves the last head group of every tile width partly empty.
TS = (1, 2, 3, 8, 17, 32)
NS, BS, HEADS = (1, 5, 17), (1, 3), (1, 3)
_cache = {}
_report_started = []


def _hip():
    from one_peace_amd import hip
    return hip


def _case(B, T, N, heads, spread=1.0, equal=False):
    """Inputs and fp64 references of a shape, computed once and left unchanged."""
    key = (B, T, N, heads, spread, equal)
    if key not in _cache:
        q, k, v, dout = FR.make_inputs(B, T, N, heads, seed=2, spread=spread)
        if equal:  # every key of a sequence is the same row: all T scores of a query are equal, p = 1 / T
            k = k[:, :1].expand_as(k).contiguous()
        scale = FR.f32(SCALE)
        _cache[key] = dict(q=q, k=k, v=v, dout=dout, ref=dict(FR.forward_ref(q, k, v, scale), **FR.backward_ref(q, k, v, dout, scale)))
    return _cache[key]


def _report(lines):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a" if _report_started else "w") as f:   # one report per session, not one per suite run ever made
        _report_started.append(True)
        for line in lines:
            f.write(line + "\n")


def _run(c, B, T, N, heads, padded):
    """Forward and backward of one case through the ctypes wrappers, every buffer guarded.  Returns the outputs as [B, T, N, heads, 64]
    device tensors and the number of guard elements touched."""
    hip = _hip()
    R, H = B * T * N, heads * 64
    extra = 8 if padded else 0
    qkv, w_qkv, m_qkv = FR.guarded_rows(R, 3 * H, 3 * H + extra, DEV)
    for i, name in enumerate(("q", "k", "v")):
        qkv[:, i * H:(i + 1) * H] = FR.rows(c[name]).to(torch.bfloat16).to(DEV)
    out, w_out, m_out = FR.guarded_rows(R, H, H + 2 * extra, DEV)
    dout, w_do, m_do = FR.guarded_rows(R, H, H + 3 * extra, DEV)
    dout.copy_(FR.rows(c["dout"]).to(torch.bfloat16).to(DEV))
    dqkv, w_dq, m_dq = FR.guarded_rows(R, 3 * H, 3 * H + extra, DEV)      # pre-filled with the sentinel
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    hip.attn_frames_fwd(q, k, v, B, T, N, heads, SCALE, out=out)
    hip.attn_frames_bwd(q, k, v, dout, B, T, N, heads, SCALE, dqkv=dqkv)
    torch.cuda.synchronize()
    touched = sum(FR.guard_touched(w, m) for w, m in ((w_qkv, m_qkv), (w_out, m_out), (w_do, m_do), (w_dq, m_dq)))
    shape = (B, T, N, heads, 64)
    res = {"out": out.reshape(shape), "dq": dqkv[:, :H].reshape(shape), "dk": dqkv[:, H:2 * H].reshape(shape),
           "dv": dqkv[:, 2 * H:].reshape(shape)}
    return res, touched


@pytest.mark.parametrize("T", TS)
def test_every_output_within_the_fp64_budget(T):
    worst = {n: 0.0 for n in ("out", "dq", "dk", "dv")}
    for N in NS:
        for B in BS:
            for heads in HEADS:
                c = _case(B, T, N, heads)
                for padded in (False, True):
                    got, touched = _run(c, B, T, N, heads, padded)
                    assert touched == 0, (B, T, N, heads, padded, touched)
                    for name in worst:
                        s = FR.share(got[name], c["ref"][name])
                        worst[name] = max(worst[name], s)
                        assert s <= 1.0, (name, B, T, N, heads, padded, s)
    _report(["T=%-2d  N in %s, B in %s, heads in %s, packed and padded ld:  " % (T, NS, BS, HEADS)
             + "  ".join("%s %.3f" % (n, worst[n]) for n in worst)])


@pytest.mark.parametrize("kind", ["hard", "equal"])
def test_hard_and_equal_scores(kind):
    B, T, N, heads = 2, 32, 5, 3
    c = _case(B, T, N, heads, spread=4.0, equal=False) if kind == "hard" else _case(B, T, N, heads, equal=True)
    scores = SCALE * torch.einsum("btnhd,bunhd->bnhtu", c["q"], c["k"])
    if kind == "hard":   # scale * q . k has a standard deviation of about 16: the extremes of 30 720 scores lie near +-60
        assert 45 < float(scores.max()) < 90 and -90 < float(scores.min()) < -45, (float(scores.min()), float(scores.max()))
    else:
        assert float((scores - scores[..., :1]).abs().max()) == 0.0
    got, touched = _run(c, B, T, N, heads, False)
    assert touched == 0
    shares = {n: FR.share(got[n], c["ref"][n]) for n in ("out", "dq", "dk", "dv")}
    _report(["%-5s scores, B=2 T=32 N=5 heads=3:  " % kind + "  ".join("%s %.3f" % kv for kv in shares.items())])
    assert all(s <= 1.0 for s in shares.values()), shares
    if kind == "equal":  # p = 1 / T: the output is the mean of the frames' values
        want = c["v"].mean(dim=1, keepdim=True).expand_as(c["v"])
        assert float((got["out"].double().cpu() - want).abs().max()) <= float(FR.half_ulp_bf16(want.abs()).max()) * 1.01


def test_two_runs_give_the_same_bits_and_a_sequence_does_not_see_its_neighbours():
    B, T, N, heads = 3, 17, 5, 3
    c = _case(B, T, N, heads)
    first, _ = _run(c, B, T, N, heads, False)
    again, _ = _run(c, B, T, N, heads, True)
    for name in first:
        assert torch.equal(first[name].view(torch.int16), again[name].view(torch.int16)), name
    b0, n0, h0 = 1, 3, 2   # the same sequence alone: B = N = heads = 1
    alone = {k: c[k][b0:b0 + 1, :, n0:n0 + 1, h0:h0 + 1].contiguous() for k in ("q", "k", "v", "dout")}
    got, _ = _run(alone, 1, T, 1, 1, False)
    for name in first:
        assert torch.equal(got[name].view(torch.int16), first[name][b0:b0 + 1, :, n0:n0 + 1, h0:h0 + 1].contiguous().view(torch.int16)), name
    wide = {k: c[k][:, :, n0:n0 + 1].contiguous() for k in ("q", "k", "v", "dout")}   # N shrinks to 1, B and heads stay
    got, _ = _run(wide, B, T, 1, heads, False)
    for name in first:
        assert torch.equal(got[name].view(torch.int16), first[name][:, :, n0:n0 + 1].contiguous().view(torch.int16)), name


def test_autograd_function_and_routes():
    from one_peace_amd import hip, ops
    B, T, N, heads = 2, 8, 5, 3
    H = heads * 64
    c = _case(B, T, N, heads)
    qkv = torch.cat([FR.rows(c[n]) for n in ("q", "k", "v")], dim=1).to(torch.bfloat16).to(DEV).requires_grad_(True)
    dout = FR.rows(c["dout"]).to(torch.bfloat16).to(DEV)
    calls = []
    fwd, bwd = hip.attn_frames_fwd, hip.attn_frames_bwd
    hip.attn_frames_fwd = lambda *a, **k: calls.append("fwd") or fwd(*a, **k)
    hip.attn_frames_bwd = lambda *a, **k: calls.append("bwd") or bwd(*a, **k)
    try:
        out = ops.temporal_attention(qkv, B, T, N, heads)            # scale defaults to 1 / sqrt(64)
        (out * dout).sum().backward()
        assert calls == ["fwd", "bwd"]
        f32 = ops.temporal_attention(qkv.detach().float(), B, T, N, heads)          # fp32 on the device: the torch route
        odd = ops.temporal_attention(torch.randn(B * T * N, 3 * 2 * 32, device=DEV, dtype=torch.bfloat16), B, T, N, 2)   # hd = 32
        assert calls == ["fwd", "bwd"]
    finally:
        hip.attn_frames_fwd, hip.attn_frames_bwd = fwd, bwd
    shape = (B, T, N, heads, 64)
    assert FR.share(out.detach().reshape(shape), c["ref"]["out"]) <= 1.0
    for i, name in enumerate(("dq", "dk", "dv")):
        assert FR.share(qkv.grad[:, i * H:(i + 1) * H].reshape(shape), c["ref"][name]) <= 1.0, name
    assert f32.dtype == torch.float32 and tuple(odd.shape) == (B * T * N, 64)
    assert float((f32.double().cpu().reshape(shape) - c["ref"]["out"][0]).abs().max()) < 1e-4
