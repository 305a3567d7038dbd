"""op_attn_window_fwd / op_attn_window_bwd (csrc/windowattn.hip) on the MI355X against the fp64 restatement and the derived per-element
budget of tests/windowattn_ref.py: every output of every shape, on the packed row stride and on a padded one, with all four
combinations of bias / rel given or NULL, inside NaN-guarded buffers (every output pre-filled with the sentinel: every element must be
written, nothing around them touched), slabs and parts requested and not requested; hard scores (about +-60) with a bias of magnitude
about 30, and all-equal scores; bit-equal reruns; the bits of a window unchanged when B, the grid and heads grow around it; the limits;
the autograd function of ops.window_attention against the reference and its torch route.  The largest observed / allowed ratio per
output goes to windowattn_fp64_report.txt in the tests' output directory."""
import ctypes
import os

import pytest
import torch

from tests import windowattn_ref as WR
from tests.util import OUT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
REPORT = os.path.join(OUT, "windowattn_fp64_report.txt")
SCALE = 0.125
# one window; two windows stacked in y; three side by side in x; 2 x 2.  Every workgroup of the backward has ONE (b, window) item at
# these sizes (B * windows <= 256 / heads); test_several_items_per_workgroup covers the walk over a share of several.
GRIDS = ((16, 16), (32, 16), (16, 48), (32, 32))
BS, HEADS = (1, 2), (1, 3)
TABLES = ((True, True), (True, False), (False, True), (False, False))   # (bias, rel) given
NAMES = ("out", "dq", "dk", "dv", "dbias", "drel")
F32_SENTINEL = 0x7FC00A5A
_cache = {}
_report_started = []


def _hip():
    from one_peace_amd import hip
    return hip


def _case(B, Hg, Wg, heads, spread=1.0, bias_mag=1.0, equal=False):
    """Inputs of a shape and, per combination of tables, the fp64 references: computed once and left unchanged."""
    key = (B, Hg, Wg, heads, spread, bias_mag, equal)
    if key not in _cache:
        q, k, v, dout, bias, rel_h, rel_w = WR.make_inputs(B, Hg, Wg, heads, seed=2, spread=spread, bias_mag=bias_mag)
        if equal:  # every key of a window is the same row and there are no tables: all 256 scores of a query are equal
            k = k.view(B, Hg // 16, 16, Wg // 16, 16, heads, 64)[:, :, :1, :, :1].expand(B, Hg // 16, 16, Wg // 16, 16, heads, 64)
            k = k.reshape(B, Hg, Wg, heads, 64).contiguous()
        _cache[key] = dict(q=q, k=k, v=v, dout=dout, bias=bias, rel_h=rel_h, rel_w=rel_w, refs={})
    return _cache[key]


def _ref(c, with_bias, with_rel):
    if (with_bias, with_rel) not in c["refs"]:
        b = c["bias"] if with_bias else None
        rh, rw = (c["rel_h"], c["rel_w"]) if with_rel else (None, None)
        scale = WR.f32(SCALE)
        c["refs"][(with_bias, with_rel)] = dict(WR.forward_ref(c["q"], c["k"], c["v"], b, rh, rw, scale),
                                                **WR.backward_ref(c["q"], c["k"], c["v"], c["dout"], b, rh, rw, scale))
    return c["refs"][(with_bias, with_rel)]


def _report(lines):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a" if _report_started else "w") as f:   # one report per session, not one per suite run ever made
        _report_started.append(True)
        for line in lines:
            f.write(line + "\n")


def _guarded_f32(shape, pad=64):
    n = 1
    for s in shape:
        n *= s
    whole = torch.full((n + 2 * pad,), F32_SENTINEL, dtype=torch.int32, device=DEV)
    return whole[pad:pad + n].view(torch.float32).view(shape), whole, pad, n


def _f32_guard_touched(whole, pad, n):
    return int((whole[:pad] != F32_SENTINEL).sum()) + int((whole[pad + n:] != F32_SENTINEL).sum())


def _run(c, B, Hg, Wg, heads, padded, with_bias, with_rel, extras):
    """Forward and backward of one case through the ctypes wrappers, every buffer guarded.  extras: ask for the slabs and parts the
    tables allow.  Returns the outputs ([B, Hg, Wg, heads, 64] device tensors; dbias and drel summed over their leading axis in fp64)
    and the number of guard elements touched."""
    hip = _hip()
    R, H = B * Hg * Wg, heads * 64
    extra = 8 if padded else 0
    qkv, w_qkv, m_qkv = WR.guarded_rows(R, 3 * H, 3 * H + extra, DEV)
    for i, name in enumerate(("q", "k", "v")):
        qkv[:, i * H:(i + 1) * H] = WR.rows(c[name]).to(torch.bfloat16).to(DEV)
    out, w_out, m_out = WR.guarded_rows(R, H, H + 2 * extra, DEV)
    dout, w_do, m_do = WR.guarded_rows(R, H, H + 3 * extra, DEV)
    dout.copy_(WR.rows(c["dout"]).to(torch.bfloat16).to(DEV))
    dqkv, w_dq, m_dq = WR.guarded_rows(R, 3 * H, 3 * H + extra, DEV)      # pre-filled with the sentinel
    bias = c["bias"][:heads].to(torch.bfloat16).to(DEV).contiguous() if with_bias else None
    rel_h, rel_w = ((c["rel_h"].to(torch.bfloat16).to(DEV), c["rel_w"].to(torch.bfloat16).to(DEV)) if with_rel else (None, None))
    parts, slabs = hip.attn_window_parts(B, Hg, Wg, heads)
    drel = _guarded_f32((parts, 2, 31, 64)) if extras and with_rel else None
    dbias = _guarded_f32((slabs, heads, 256, 256)) if extras and with_bias else None
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]
    hip.attn_window_fwd(q, k, v, bias, rel_h, rel_w, B, Hg, Wg, heads, SCALE, out=out)
    hip.attn_window_bwd(q, k, v, bias, rel_h, rel_w, dout, B, Hg, Wg, heads, SCALE, dqkv=dqkv,
                        drel_part=drel[0] if drel else None, dbias_slabs=dbias[0] if dbias else None)
    torch.cuda.synchronize()
    touched = sum(WR.guard_touched(w, m) for w, m in ((w_qkv, m_qkv), (w_out, m_out), (w_do, m_do), (w_dq, m_dq)))
    shape = (B, Hg, Wg, heads, 64)
    res = {"out": out.reshape(shape), "dq": dqkv[:, :H].reshape(shape), "dk": dqkv[:, H:2 * H].reshape(shape),
           "dv": dqkv[:, 2 * H:].reshape(shape)}
    for name, buf in (("drel", drel), ("dbias", dbias)):
        if buf is not None:
            touched += _f32_guard_touched(*buf[1:])
            res[name + "_raw"] = buf[0]
            res[name] = buf[0].double().sum(0)      # a sentinel left in place is a NaN here
    return res, touched


@pytest.mark.parametrize("grid", GRIDS)
def test_every_output_within_the_fp64_budget(grid):
    Hg, Wg = grid
    worst = {n: 0.0 for n in NAMES}
    for B in BS:
        for heads in HEADS:
            c = _case(B, Hg, Wg, heads)
            for with_bias, with_rel in TABLES:
                ref = _ref(c, with_bias, with_rel)
                for padded in (False, True):
                    got, touched = _run(c, B, Hg, Wg, heads, padded, with_bias, with_rel, extras=not padded)
                    assert touched == 0, (B, grid, heads, padded, with_bias, with_rel, touched)
                    shares = WR.shares(got, ref)
                    assert set(shares) == {"out", "dq", "dk", "dv"} | ({"dbias"} if with_bias and not padded else set()) \
                        | ({"drel"} if with_rel and not padded else set())
                    for name, s in shares.items():
                        print("grid", grid, "B", B, "heads", heads, "bias", with_bias, "rel", with_rel, "padded", padded, name, "%.3f" % s)
                        worst[name] = max(worst[name], s)
                    assert all(s <= 1.0 for s in shares.values()), (B, grid, heads, padded, with_bias, with_rel, shares)
    _report(["grid %2d x %2d  B in %s, heads in %s, bias / rel given or not, packed and padded ld:  " % (Hg, Wg, BS, HEADS)
             + "  ".join("%s %.3f" % (n, worst[n]) for n in worst)])


@pytest.mark.parametrize("kind", ["hard", "equal"])
def test_hard_and_equal_scores(kind):
    B, Hg, Wg, heads = 2, 32, 16, 3
    if kind == "hard":   # scale * q . k has a standard deviation of about 16, the bias of about 30: extremes beyond +-60
        c = _case(B, Hg, Wg, heads, spread=4.0, bias_mag=30.0)
        s = SCALE * torch.einsum("...id,...jd->...ij", WR.win(c["q"]), WR.win(c["k"])) + c["bias"]
        assert float(s.max()) > 60 and float(s.min()) < -60 and 20 < float(c["bias"].abs().mean()) < 40
        tables = (True, True)
    else:
        c = _case(B, Hg, Wg, heads, equal=True)
        s = SCALE * torch.einsum("...id,...jd->...ij", WR.win(c["q"]), WR.win(c["k"]))
        assert float((s - s[..., :1]).abs().max()) == 0.0
        tables = (False, False)
    got, touched = _run(c, B, Hg, Wg, heads, False, *tables, extras=True)
    assert touched == 0
    shares = WR.shares(got, _ref(c, *tables))
    _report(["%-5s scores, B=2 grid 32 x 16 heads=3:  " % kind + "  ".join("%s %.3f" % kv for kv in shares.items())])
    assert all(x <= 1.0 for x in shares.values()), shares
    if kind == "equal":  # p = 1 / 256: the output is the mean of the window's values
        want = WR.unwin(WR.win(c["v"]).mean(dim=-2, keepdim=True).expand(-1, -1, -1, -1, 256, -1))
        assert float((got["out"].double().cpu() - want).abs().max()) <= float(WR.half_ulp_bf16(want.abs()).max()) * 1.01


def test_two_runs_give_the_same_bits_and_a_window_does_not_see_its_neighbours():
    B, Hg, Wg, heads = 2, 32, 32, 3
    c = _case(B, Hg, Wg, heads)
    first, _ = _run(c, B, Hg, Wg, heads, False, True, True, extras=True)
    again, _ = _run(c, B, Hg, Wg, heads, True, True, True, extras=True)
    for name in ("out", "dq", "dk", "dv"):
        assert torch.equal(first[name].view(torch.int16), again[name].view(torch.int16)), name
    for name in ("drel_raw", "dbias_raw"):
        assert torch.equal(first[name].view(torch.int32), again[name].view(torch.int32)), name
    b0, wy, wx, h0 = 1, 1, 0, 2   # the same window alone: B = 1, a 16 x 16 grid, one head with its own bias
    sl = (slice(b0, b0 + 1), slice(16 * wy, 16 * wy + 16), slice(16 * wx, 16 * wx + 16), slice(h0, h0 + 1))
    alone = {k: c[k][sl].contiguous() for k in ("q", "k", "v", "dout")}
    alone.update(bias=c["bias"][h0:h0 + 1], rel_h=c["rel_h"], rel_w=c["rel_w"])
    got, _ = _run(alone, 1, 16, 16, 1, False, True, True, extras=False)
    for name in ("out", "dq", "dk", "dv"):
        assert torch.equal(got[name].view(torch.int16), first[name][sl].contiguous().view(torch.int16)), name
    tall = {k: c[k][:, :, 16 * wx:16 * wx + 16].contiguous() for k in ("q", "k", "v", "dout")}   # the grid shrinks in x, B and heads stay
    tall.update(bias=c["bias"], rel_h=c["rel_h"], rel_w=c["rel_w"])
    got, _ = _run(tall, B, Hg, 16, heads, False, True, True, extras=True)
    for name in ("out", "dq", "dk", "dv"):
        assert torch.equal(got[name].view(torch.int16), first[name][:, :, 16 * wx:16 * wx + 16].contiguous().view(torch.int16)), name


def _per(B, Hg, Wg, heads):
    """(slabs, items per share, items of the last share) of the backward when slabs or parts are asked for."""
    parts, slabs = _hip().attn_window_parts(B, Hg, Wg, heads)
    bw = B * (Hg // 16) * (Wg // 16)
    per = -(-bw // slabs)
    assert parts == slabs * heads and (slabs - 1) * per < bw <= slabs * per
    return slabs, per, bw - (slabs - 1) * per


def test_several_items_per_workgroup():
    """24 heads, B = 3, 32 x 32: 12 (b, window) items in 6 shares of 2 -- a workgroup's second item adds into its dbias slab and its
    drel part and reuses every LDS region.  All six outputs against the fp64 budget, bit-equal reruns (slabs and parts too), the same
    dq, dk, dv bits with one item per workgroup (no slabs, no parts) and for a window that is the SECOND item of its share run alone."""
    B, Hg, Wg, heads = 3, 32, 32, 24
    slabs, per, last = _per(B, Hg, Wg, heads)
    assert (slabs, per, last) == (6, 2, 2)
    c = _case(B, Hg, Wg, heads)
    ref = _ref(c, True, True)
    first, touched = _run(c, B, Hg, Wg, heads, False, True, True, extras=True)
    assert touched == 0 and tuple(first["dbias_raw"].shape) == (slabs, heads, 256, 256)
    shares = WR.shares(first, ref)
    _report(["24 heads, B=3 grid 32 x 32, %d items per workgroup:  " % per + "  ".join("%s %.3f" % kv for kv in shares.items())])
    assert set(shares) == set(NAMES) and all(x <= 1.0 for x in shares.values()), shares
    again, touched = _run(c, B, Hg, Wg, heads, True, True, True, extras=True)
    assert touched == 0
    for name in ("out", "dq", "dk", "dv"):
        assert torch.equal(first[name].view(torch.int16), again[name].view(torch.int16)), name
    for name in ("drel_raw", "dbias_raw"):
        assert torch.equal(first[name].view(torch.int32), again[name].view(torch.int32)), name
    single, touched = _run(c, B, Hg, Wg, heads, False, True, True, extras=False)       # one item per workgroup
    assert touched == 0
    for name in ("dq", "dk", "dv"):
        assert torch.equal(first[name].view(torch.int16), single[name].view(torch.int16)), name
    b0, wy, wx, h0 = 1, 0, 1, 17   # item b0 * 4 + 1 = 5: the second of share 2
    sl = (slice(b0, b0 + 1), slice(16 * wy, 16 * wy + 16), slice(16 * wx, 16 * wx + 16), slice(h0, h0 + 1))
    alone = {k: c[k][sl].contiguous() for k in ("q", "k", "v", "dout")}
    alone.update(bias=c["bias"][h0:h0 + 1], rel_h=c["rel_h"], rel_w=c["rel_w"])
    got, _ = _run(alone, 1, 16, 16, 1, False, True, True, extras=True)
    for name in ("out", "dq", "dk", "dv"):
        assert torch.equal(got[name].view(torch.int16), first[name][sl].contiguous().view(torch.int16)), name


def test_uneven_shares_sum_to_the_samples_own_slabs_and_parts():
    """24 heads, B = 11, one window each: 6 shares, five of 2 items and a last one of 1.  No fp64 reference is needed: the sum of the
    slabs (parts) must be the sum over the samples of what each sample gives alone, up to the fp32 additions in between -- at most two
    per element and route, each within u = 2^-24 of the magnitudes added: |difference| <= 4 u sum_b |alone_b|."""
    B, heads = 11, 24
    slabs, per, last = _per(B, 16, 16, heads)
    assert (slabs, per, last) == (6, 2, 1)
    c = _case(B, 16, 16, heads)
    whole, touched = _run(c, B, 16, 16, heads, False, True, True, extras=True)
    assert touched == 0
    want = {"dbias": 0.0, "drel": 0.0}
    mag = {"dbias": 0.0, "drel": 0.0}
    for b in range(B):
        one = {k: c[k][b:b + 1].contiguous() for k in ("q", "k", "v", "dout")}
        one.update(bias=c["bias"], rel_h=c["rel_h"], rel_w=c["rel_w"])
        got, _ = _run(one, 1, 16, 16, heads, False, True, True, extras=True)
        for name in ("out", "dq", "dk", "dv"):
            assert torch.equal(got[name].view(torch.int16), whole[name][b:b + 1].contiguous().view(torch.int16)), (name, b)
        for name in want:
            want[name] = want[name] + got[name]
            mag[name] = mag[name] + got[name + "_raw"].double().abs().sum(0)
    for name in want:
        assert bool(((whole[name] - want[name]).abs() <= 4 * WR.U * mag[name]).all()), name
        assert float(want[name].abs().max()) > 0


def test_limits_return_einval_without_a_launch():
    hip = _hip()
    L = hip.lib()
    R, H = 16 * 16, 64
    qkv, w_qkv, m_qkv = WR.guarded_rows(R, 3 * H, 3 * H, DEV)
    out, w_out, m_out = WR.guarded_rows(R, H, H, DEV)
    P = lambda t, off=0: ctypes.c_void_p(t.data_ptr() + off)  # noqa: E731
    q, k, v = qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:]

    def fwd(Hg=16, Wg=16, hd=64, window=16, ld=192, ldo=64, off=0, heads=1):
        return L.op_attn_window_fwd(P(q), P(k), P(v), ld, None, None, None, P(out, off), ldo, 1, Hg, Wg, heads, hd, window, SCALE, hip.stream())
    bad = [fwd(Hg=20), fwd(Wg=8), fwd(hd=32), fwd(window=8), fwd(ld=188), fwd(ldo=60), fwd(off=2), fwd(heads=2, ldo=64)]
    assert all(rc == -22 for rc in bad), bad
    assert L.op_attn_window_bwd(P(q), P(k), P(v), 192, None, None, None, P(out), 64, P(qkv), P(qkv), P(qkv), 190, None, None, 1, 16, 16, 1, 64,
                                16, SCALE, hip.stream()) == -22
    torch.cuda.synchronize()
    assert bool((w_out == WR.BF16_SENTINEL).all()) and bool((w_qkv == WR.BF16_SENTINEL).all())    # nothing was launched
    with pytest.raises(RuntimeError):
        hip.attn_window_fwd(q, k, v, None, torch.zeros(31, 64, dtype=torch.bfloat16, device=DEV), None, 1, 16, 16, 1, SCALE)


def test_autograd_function_and_routes():
    from one_peace_amd import hip, ops
    B, Hg, Wg, heads = 2, 32, 16, 3
    H = heads * 64
    c = _case(B, Hg, Wg, heads)
    ref = _ref(c, True, True)
    dev = lambda t: t.to(torch.bfloat16).to(DEV).requires_grad_(True)  # noqa: E731
    qkv = dev(torch.cat([WR.rows(c[n]) for n in ("q", "k", "v")], dim=1))
    bias, rel_h, rel_w = dev(c["bias"]), dev(c["rel_h"]), dev(c["rel_w"])
    dout = WR.rows(c["dout"]).to(torch.bfloat16).to(DEV)
    calls = []
    fwd, bwd = hip.attn_window_fwd, hip.attn_window_bwd
    hip.attn_window_fwd = lambda *a, **k: calls.append("fwd") or fwd(*a, **k)
    hip.attn_window_bwd = lambda *a, **k: calls.append(("bwd", k.get("want_drel"), k.get("want_dbias"))) or bwd(*a, **k)
    try:
        out = ops.window_attention(qkv, bias, rel_h, rel_w, B, Hg, Wg, heads, 16)           # scale defaults to 1 / sqrt(64)
        (out * dout).sum().backward()
        assert calls == ["fwd", ("bwd", True, True)]
        frozen = ops.window_attention(qkv, bias.detach(), rel_h.detach(), rel_w.detach(), B, Hg, Wg, heads, 16)   # frozen tables: no
        torch.autograd.grad((frozen * dout).sum(), qkv)                                                            # slabs, no parts
        assert calls[2:] == ["fwd", ("bwd", False, False)] and torch.equal(frozen, out)
        n = len(calls)
        leaves = [t.detach().float().requires_grad_(True) for t in (qkv, bias, rel_h, rel_w)]
        f32 = ops.window_attention(*leaves, B, Hg, Wg, heads, 16)                            # fp32 on the device: the torch route
        g32 = torch.autograd.grad((f32 * dout.float()).sum(), leaves)
        odd = ops.window_attention(torch.randn(B * 8 * 8, 3 * 2 * 32, device=DEV, dtype=torch.bfloat16), None, None, None, B, 8, 8, 2, 4)
        assert len(calls) == n
    finally:
        hip.attn_window_fwd, hip.attn_window_bwd = fwd, bwd
    shape = (B, Hg, Wg, heads, 64)
    shares = {"out": WR.share(out.detach().reshape(shape), ref["out"])}
    for i, name in enumerate(("dq", "dk", "dv")):
        shares[name] = WR.share(qkv.grad[:, i * H:(i + 1) * H].reshape(shape), ref[name])
    # the table gradients leave the function in the tables' dtype: one more rounding to bf16
    for name, got in (("dbias", bias.grad), ("drel", torch.stack([rel_h.grad, rel_w.grad]))):
        exact, _, E = ref[name]
        shares[name] = WR.share(got, (exact, WR.half_ulp_bf16(exact.abs() + E), E))
    _report(["ops.window_attention through autograd, B=2 grid 32 x 16 heads=3:  " + "  ".join("%s %.3f" % kv for kv in shares.items())])
    assert all(s <= 1.0 for s in shares.values()), shares
    # the torch route of the same call (fp32 on the device) states the same function
    assert f32.dtype == torch.float32 and tuple(odd.shape) == (B * 64, 64)
    assert float((f32.detach().double().cpu().reshape(shape) - ref["out"][0]).abs().max()) < 1e-4
    for i, name in enumerate(("dq", "dk", "dv")):
        assert float((g32[0][:, i * H:(i + 1) * H].double().cpu().reshape(shape) - ref[name][0]).abs().max()) < 1e-3, name
    assert float((g32[1].double().cpu() - ref["dbias"][0]).abs().max()) < 1e-3
    assert float((torch.stack(g32[2:]).double().cpu() - ref["drel"][0]).abs().max()) < 1e-2
