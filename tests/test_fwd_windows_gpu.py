"""Forward GEMMs of a residual branch over row windows (ops.SKIP_ZERO_FWD): op_live_mwindows_fwd against the NumPy rule of
tests/test_fwd_windows_cpu.py, and op_gemm_nt_grouped_windows_fwd against the dense launches, bit for bit.

The activation rows of a dropped sample are NOT zero in the forward; the dense launch multiplies them and the epilogue (or a later
kernel) multiplies the result by ps = 0.  The listed launch computes the windows of kept samples only -- the same operands in the same
K order through the same epilogue -- and the list-building launch fills the rest: +0 in a plain output, the residual input's rows in
the branch output."""
import ctypes

import numpy as np
import pytest
import torch

from tests import dgrad_windows_ref as R
from tests.test_dgrad_windows_cpu import PATTERNS, patterns, three_segments
from tests.test_fwd_windows_cpu import fill_rule

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
NS = 256     # columns of a weight segment
GUARD = 320  # rows behind every output: a window that starts at the last sample reaches up to 255 rows past M
TOTAL = three_segments("none")[1]


def _dev_segs(segs):
    return [(torch.tensor(ps, dtype=torch.float32, device=DEV) * 1.25, r0, S, B) for ps, r0, S, B in segs]


def _per_row(segs):
    """the multipliers of the lock-step attention branch: one per row, a sample's is the one of its first row"""
    return torch.cat([torch.tensor(np.repeat(ps, S), dtype=torch.float32, device=DEV) * 1.25 for ps, _, S, _ in segs])


def _guarded(cols, rows=TOTAL):
    buf = torch.full((rows + GUARD, cols), float("nan"), dtype=BF, device=DEV)
    return buf, buf[:rows]


# ------------------------------------------------------------------------------------------------------------------
# fill
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", ["257x6", "250x6", "64x8", "three"])
def test_fill_against_the_numpy_rule(case, pattern):
    from one_peace_amd import hip
    if case == "three":
        segs, total = three_segments(pattern)
    else:
        S, B = (int(v) for v in case.split("x"))
        segs, total = [(patterns(B)[pattern], 0, S, B)], S * B
    whole = [(i, 0, 0) for i in range(len(segs))]
    src = torch.randn(total, 64, generator=torch.Generator(device="cpu").manual_seed(total)).to(BF).to(DEV)
    nan_plain, nan_copy = np.full((total + GUARD, 512), np.nan, np.float32), np.full((total + GUARD, 64), np.nan, np.float32)
    want_plain, filled = fill_rule(segs, total, nan_plain)
    want_copy, _ = fill_rule(segs, total, nan_copy, src.float().cpu().numpy())
    per_row = _per_row(segs)
    for dsegs in (_dev_segs(segs), [(per_row[r0:], r0, S, B, S) for _, r0, S, B in segs]):
        (bp, plain), (bc, copy) = _guarded(512, total), _guarded(64, total)
        got = hip.live_mwindows_fwd(dsegs, [whole], [plain, copy], [None, src])
        torch.cuda.synchronize()
        assert int(got[0][1].item()) == len(R.expected_windows(segs, whole))
        f = torch.from_numpy(filled).to(DEV)
        assert not bool(torch.signbit(plain[f]).any())                       # +0
        for have, want in ((bp, want_plain), (bc, want_copy)):               # rows outside the fill and the guard band stay NaN
            assert np.array_equal(have.float().cpu().numpy(), want, equal_nan=True)


# ------------------------------------------------------------------------------------------------------------------
# operands and dense references: computed once, never changed
# ------------------------------------------------------------------------------------------------------------------
_OPS, _DENSE = {}, {}
RS = [slice(r0, r0 + S * B) for _, r0, S, B in three_segments("none")[0]]


def _operands(K):
    """A [3554, K], non-zero in every row; per segment three weights [256, K]; two bias vectors, a layer-scale vector with a zero and
    negative entries, a residual matrix."""
    if K not in _OPS:
        g = torch.Generator(device="cpu").manual_seed(K)
        A = torch.randn(TOTAL, K, generator=g).to(BF).to(DEV)
        Ws = [[(torch.randn(NS, K, generator=g) * 0.05).to(BF).to(DEV) for _ in range(3)] for _ in range(3)]
        bs = [torch.randn(NS, generator=g).to(BF).to(DEV) for _ in range(3)]
        gamma = torch.randn(NS, generator=g)
        gamma[3], gamma[7] = 0.0, -abs(float(gamma[7])) - 0.5
        X = torch.randn(TOTAL, NS, generator=g).to(BF).to(DEV)
        assert bool((A != 0).any(dim=1).all())
        _OPS[K] = (A, Ws, bs, gamma.to(BF).to(DEV), X)
    return _OPS[K]


def _dense_bias(K, grouped, A=None):
    from one_peace_amd import hip
    key = ("bias", K, grouped)
    if A is not None or key not in _DENSE:
        A0, Ws, bs, _, _ = _operands(K)
        a = A0 if A is None else A
        if grouped:  # wi_0 | wi_1 of each segment: N = 2 x 256, no bias
            d = torch.cat([hip.gemm_nt(a[r].contiguous(), Ws[i][:2], n_seg=NS, N=2 * NS, splitk=False) for i, r in enumerate(RS)])
        else:        # q | k | v over all rows: N = 3 x 256, biases b, none, b
            d = hip.gemm_nt(a, Ws[0], [bs[0], None, bs[0]], n_seg=NS, N=3 * NS, splitk=False)
        if A is not None:
            return d
        _DENSE[key] = d
    return _DENSE[key]


def _dense_resid(K, grouped, segs, A=None):
    from one_peace_amd import hip
    A0, Ws, bs, gamma, X = _operands(K)
    a = A0 if A is None else A
    if grouped:  # down-projection + residual of each segment: per-sample multipliers, rows_per_sample = S
        return torch.cat([hip.gemm_nt(a[r].contiguous(), [Ws[i][0]], [bs[i]], epilogue=hip.EPI_RESID, resid=X[r], gamma=gamma, rowscale=ps,
                                      rows_per_sample=S, splitk=False) for i, (r, (ps, _, S, _)) in enumerate(zip(RS, _dev_segs(segs)))])
    return hip.gemm_nt(a, [Ws[0][0]], [bs[0]], epilogue=hip.EPI_RESID, resid=X, gamma=gamma, rowscale=_per_row(segs), rows_per_sample=1,
                       splitk=False)


def _members(segs, grouped):
    return [(i, i, sg[1]) for i, sg in enumerate(segs)] if grouped else [(i, 0, 0) for i in range(len(segs))]


def _computed(segs, grouped):
    prob_rows = [(r.start, r.stop - r.start) for r in RS] if grouped else [(0, TOTAL)]
    return torch.from_numpy(R.computed_rows(segs, _members(segs, grouped), prob_rows, TOTAL)).to(DEV)


def _listed_bias(K, segs, grouped, tune=None, A=None):
    from one_peace_amd import hip
    A0, Ws, bs, _, _ = _operands(K)
    a = A0 if A is None else A
    buf, out = _guarded((2 if grouped else 3) * NS)
    (win,) = hip.live_mwindows_fwd(_dev_segs(segs), [_members(segs, grouped)], [out], [None])
    if grouped:
        ok = hip.gemm_nt_windows_fwd([a[r] for r in RS], [Ws[i][:2] for i in range(3)], None, [out[r] for r in RS], win, NS,
                                     max_row_stride=257, tune=tune)
    else:
        ok = hip.gemm_nt_windows_fwd([a], [Ws[0]], [[bs[0], None, bs[0]]], [out], win, NS, max_row_stride=257, tune=tune)
    torch.cuda.synchronize()
    assert ok
    assert bool(torch.isnan(buf[TOTAL:]).all()), "a window wrote behind the last row"
    return out, int(win[1].item())


def _listed_resid(K, segs, grouped, tune=None, A=None):
    from one_peace_amd import hip
    A0, Ws, bs, gamma, X = _operands(K)
    a = A0 if A is None else A
    buf, out = _guarded(NS)
    if grouped:
        (win,) = hip.live_mwindows_fwd(_dev_segs(segs), [_members(segs, True)], [out], [X])
        ok = hip.gemm_nt_windows_fwd([a[r] for r in RS], [[Ws[i][0]] for i in range(3)], [[bs[i]] for i in range(3)], [out[r] for r in RS], win,
                                     NS, epilogue=hip.EPI_RESID, resids=[X[r] for r in RS], gammas=[gamma] * 3,
                                     rowscales=[q[0] for q in _dev_segs(segs)], rows_per_sample=[sg[2] for sg in segs], max_row_stride=257,
                                     tune=tune)
    else:
        per_row = _per_row(segs)
        (win,) = hip.live_mwindows_fwd([(per_row[r0:], r0, S, B, S) for _, r0, S, B in segs], [_members(segs, False)], [out], [X])
        ok = hip.gemm_nt_windows_fwd([a], [[Ws[0][0]]], [[bs[0]]], [out], win, NS, epilogue=hip.EPI_RESID, resids=[X], gammas=[gamma],
                                     rowscales=[per_row], rows_per_sample=[1], max_row_stride=257, tune=tune)
    torch.cuda.synchronize()
    assert ok
    assert bool(torch.isnan(buf[TOTAL:]).all()), "a window wrote behind the last row"
    return out, int(win[1].item())


# ------------------------------------------------------------------------------------------------------------------
# listed bias launch: q | k | v over all rows, grouped wi_0 | wi_1
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("K", [128, 1536])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_listed_bias_launch_equals_the_dense_rows_and_skips_the_rest(pattern, K, grouped):
    segs, _ = three_segments(pattern)
    out, n = _listed_bias(K, segs, grouped)
    dense = _dense_bias(K, grouped)
    c = _computed(segs, grouped)
    assert n == len(R.expected_windows(segs, _members(segs, grouped)))
    assert not bool(torch.isnan(out).any()), "a row nobody wrote"
    assert torch.equal(out[c], dense[c]), float((out[c].float() - dense[c].float()).abs().max())
    # control: the rows no window reaches are +0, and the dense product is not
    assert bool((out[~c] == 0).all()) and not bool(torch.signbit(out[~c]).any())
    assert bool((dense[~c] != 0).any(dim=1).all())


# ------------------------------------------------------------------------------------------------------------------
# listed residual launch: out-proj over all rows (per-row multipliers), grouped down-projection (per-sample multipliers)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("K", [128, 6144])
@pytest.mark.parametrize("pattern", PATTERNS)
def test_listed_residual_launch_equals_the_dense_launch(pattern, K, grouped):
    segs, _ = three_segments(pattern)
    out, n = _listed_resid(K, segs, grouped)
    dense = _dense_resid(K, grouped, segs)
    assert n == len(R.expected_windows(segs, _members(segs, grouped)))
    assert torch.equal(out, dense), float((out.float() - dense.float()).abs().max())  # (NaN nowhere: a NaN is not equal to itself)
    X = _operands(K)[4]
    kept = torch.from_numpy(np.concatenate([np.repeat(ps != 0, S) for ps, _, S, _ in segs])).to(DEV)
    assert torch.equal(out[~kept], X[~kept])
    if kept.any():
        assert bool((out[kept] != X[kept]).any(dim=1).all())  # the branch was added


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("K", [128, 6144])
def test_the_residual_windows_really_skip(K, grouped):
    """Control: NaN in the A rows no window touches.  The listed output has none and is the dense output of the clean operand; the
    dense launch on the same operand has NaN."""
    segs, _ = three_segments("alternating")
    c = _computed(segs, grouped)
    assert int((~c).sum()) > TOTAL // 4
    A = _operands(K)[0].clone()
    A[~c] = float("nan")
    out, _ = _listed_resid(K, segs, grouped, A=A)
    assert not bool(torch.isnan(out).any())
    assert torch.equal(out, _dense_resid(K, grouped, segs))
    assert bool(torch.isnan(_dense_resid(K, grouped, segs, A=A)[~c]).any(dim=1).all())


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("keep", [1.0, 0.0])
def test_every_sample_kept_and_every_sample_dropped(keep, grouped):
    """(three_segments gives each segment another pattern.)  All kept: every row comes from a window and equals the dense launch.  All
    dropped: only the strided window of the image samples' last rows is listed; q | k | v is +0 but for those six rows, the branch
    output is the residual input."""
    segs = [(np.full_like(ps, keep), r0, S, B) for ps, r0, S, B in three_segments("none")[0]]
    c = _computed(segs, grouped)
    out, n = _listed_bias(128, segs, grouped)
    assert torch.equal(out[c], _dense_bias(128, grouped)[c]) and bool((out[~c] == 0).all()) and not bool(torch.signbit(out[~c]).any())
    res, n2 = _listed_resid(128, segs, grouped)
    assert torch.equal(res, _dense_resid(128, grouped, segs))
    if keep:
        assert bool(c.all()) and n == n2 == len(R.expected_windows(segs, _members(segs, grouped)))
    else:
        assert n == n2 == 1 and int(c.sum()) == 6 and torch.equal(res, _operands(128)[4])


@pytest.mark.parametrize("grouped", [False, True])
def test_one_tile_per_workgroup_form_gives_the_same_bits(grouped):
    """tune sched 7: a dense grid of one-tile workgroups, the ones past the count leave at once."""
    segs, _ = three_segments("adjacent")
    for fn in (_listed_bias, _listed_resid):
        a, b = fn(128, segs, grouped)[0], fn(128, segs, grouped, tune=7 << 20)[0]
        assert torch.equal(a, b) and not bool(torch.isnan(a).any())


# ------------------------------------------------------------------------------------------------------------------
# limits
# ------------------------------------------------------------------------------------------------------------------
def test_limits_are_refused_not_launched():
    from one_peace_amd import hip
    L = hip.lib()
    EINVAL = -22
    segs, _ = three_segments("alternating")
    A, Ws, bs, gamma, X = _operands(128)
    buf, out = _guarded(NS)
    (win,) = hip.live_mwindows_fwd(_dev_segs(segs), [_members(segs, False)], [out], [X])
    torch.cuda.synchronize()
    before = buf.clone()
    i64 = ctypes.c_int64
    pa = lambda ts, n=3: hip._ptr_array(ts, n)  # noqa: E731

    def launch(**kw):
        a = dict(nprob=1, A=pa([A], 1), M=(i64 * 1)(TOTAL), lda=A.stride(0), B=pa([Ws[0][0]]), ldb=128, n_seg=NS, bias=pa([bs[0]]),
                 C=pa([out], 1), ldc=NS, resid=pa([X], 1), ldr=NS, gamma=pa([gamma], 1), rowscale=pa([_per_row(segs)], 1),
                 rps=(i64 * 1)(1), N=NS, K=128, epilogue=hip.EPI_RESID, windows=hip.ptr(win[0]), count=hip.ptr(win[1]),
                 max_windows=win[0].numel() // 2, max_row_stride=257, tune=0)
        a.update(kw)
        return L.op_gemm_nt_grouped_windows_fwd(a["nprob"], a["A"], a["M"], a["lda"], a["B"], a["ldb"], a["n_seg"], a["bias"], a["C"], a["ldc"],
                                                a["resid"], a["ldr"], a["gamma"], a["rowscale"], a["rps"], a["N"], a["K"], a["epilogue"],
                                                a["windows"], a["count"], a["max_windows"], a["max_row_stride"], a["tune"], hip.stream())
    assert launch(windows=None) == EINVAL and launch(count=None) == EINVAL and launch(B=None) == EINVAL
    assert launch(resid=None) == EINVAL and launch(resid=pa([None], 1)) == EINVAL            # the residual epilogue needs its residual
    assert launch(windows=ctypes.c_void_p(win[0].data_ptr() + 4)) == EINVAL                  # an entry is read with one 8-byte load
    assert launch(max_row_stride=0) == EINVAL and launch(max_row_stride=65536) == EINVAL
    assert launch(max_row_stride=(1 << 23) // NS) == EINVAL                                  # max_row_stride * ld < 2^23
    assert launch(max_windows=0) == EINVAL and launch(nprob=4) == EINVAL
    assert launch(n_seg=128) == EINVAL and launch(n_seg=0) == EINVAL and launch(epilogue=hip.EPI_GEGLU) == EINVAL
    assert launch(ldr=NS + 4) == EINVAL
    assert launch(rps=(i64 * 1)(1 << 31)) == EINVAL                                          # rows * rows_per_sample < 2^32

    def fill(**kw):
        one = lambda v: (i64 * 1)(v)  # noqa: E731
        a = dict(nout=1, out=pa([out], 1), src=pa([X], 1), src_ld=one(NS))
        a.update(kw)
        lst, cnt = win
        return L.op_live_mwindows_fwd(1, pa([_dev_segs(segs)[0][0]], 1), one(1), one(0), one(64), one(8), one(0), one(0), (i64 * 2)(0, -1),
                                      (i64 * 2)(0, 0), (i64 * 2)(0, 0), 1, pa([lst], 1), pa([cnt], 1), one(lst.numel() // 2), a["nout"], a["out"],
                                      one(NS), one(NS), one(TOTAL), a["src"], a["src_ld"], hip.stream())
    assert fill(src=None) == EINVAL and fill(src_ld=None) == EINVAL and fill(nout=0) == EINVAL
    assert fill(src=pa([X[:, 1:]], 1)) == EINVAL                                              # 16-byte loads
    assert fill(src_ld=(i64 * 1)(NS + 4)) == EINVAL and fill(src_ld=(i64 * 1)(NS - 8)) == EINVAL
    assert fill(src=pa([out], 1)) == EINVAL                                                   # a copy onto itself
    torch.cuda.synchronize()
    assert np.array_equal(buf.float().cpu().numpy(), before.float().cpu().numpy(), equal_nan=True), "a refused call wrote something"
