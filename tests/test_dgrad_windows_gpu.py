"""Input-gradient GEMMs over row windows (ops.SKIP_ZERO_DGRAD): op_live_mwindows against the NumPy restatement in
tests/dgrad_windows_ref.py, and op_gemm_nt_grouped_windows against the dense launch, bit for bit.

The rows of a sample stochastic depth dropped are zero in dy; the dense launch turns them into +0 rows of dy W^T.  The listed launch
computes the windows of kept samples only (the same operands in the same K order) and the list-building launch writes the +0 rows.
The last rows of the 257-row samples ride in the same launch as a strided window."""
import numpy as np
import pytest
import torch

from tests import dgrad_windows_ref as R
from tests.test_dgrad_windows_cpu import PATTERNS, patterns, three_segments

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16
N_OUT = 512
GUARD = 320  # rows behind the output: a window that starts at the last sample reaches up to 255 rows past M


def _dev_segs(segs):
    return [(torch.tensor(ps, dtype=torch.float32, device=DEV) * 1.25, r0, S, B) for ps, r0, S, B in segs]


def _read(lst, cnt):
    n = int(cnt.item())
    assert 0 <= n <= lst.numel() // 2
    w = lst[:2 * n].tolist()
    return n, sorted((w[2 * i] >> 28, w[2 * i] & ((1 << 28) - 1), w[2 * i + 1] & 0xffff, w[2 * i + 1] >> 16) for i in range(n))


# ------------------------------------------------------------------------------------------------------------------
# lists and zero rows
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", ["257x6", "250x6", "64x8", "100x16", "three"])
def test_lists_and_zero_rows_against_the_numpy_rule(case, pattern):
    from one_peace_amd import hip
    if case == "three":
        segs, total = three_segments(pattern)
    else:
        S, B = (int(v) for v in case.split("x"))
        segs, total = [(patterns(B)[pattern], 0, S, B)], S * B
    whole = [(i, 0, 0) for i in range(len(segs))]
    per_seg = [[(i, 0, sg[1])] for i, sg in enumerate(segs)]
    grouped = [(i, i, sg[1]) for i, sg in enumerate(segs)]
    for lists in ([whole], per_seg + [grouped]):
        outs = [torch.full((total + GUARD, c), float("nan"), dtype=BF, device=DEV) for c in (N_OUT, 64)]
        got = hip.live_mwindows(_dev_segs(segs), lists, [o[:total] for o in outs])
        torch.cuda.synchronize()
        for (lst, cnt), members in zip(got, lists):
            want = sorted(R.expected_windows(segs, members))
            n, have = _read(lst, cnt)
            assert n == len(want) and have == want, (n, len(want))
        zeroed = torch.from_numpy(R.zero_filled_rows(segs, total)).to(DEV)
        for o in outs:
            assert bool((o[:total][zeroed] == 0).all()) and not bool(torch.signbit(o[:total][zeroed]).any())   # +0
            assert bool(torch.isnan(o[:total][~zeroed]).all()) and bool(torch.isnan(o[total:]).all())
    # the per-row multipliers of the lock-step attention branch: sample b's multiplier is the one of its first row
    per_row = torch.cat([torch.tensor(np.repeat(ps, S), dtype=torch.float32, device=DEV) for ps, _, S, _ in segs])
    got = hip.live_mwindows([(per_row[r0:], r0, S, B, S) for _, r0, S, B in segs], [whole], [])
    torch.cuda.synchronize()
    assert _read(*got[0])[1] == sorted(R.expected_windows(segs, whole))


# ------------------------------------------------------------------------------------------------------------------
# GEMM
# ------------------------------------------------------------------------------------------------------------------
_OPS = {}


def _operands(K):
    """text | image | audio rows (8 x 64, 6 x 257, 6 x 250 = 3554) of one activation matrix, a weight per segment, and the dense
    products (no K-split) of the whole matrix with weight 0 and of each segment with its own weight: computed once, never changed."""
    if K not in _OPS:
        g = torch.Generator(device="cpu").manual_seed(K)
        _, total = three_segments("none")
        A = torch.randn(total, K, generator=g).to(BF).to(DEV)
        Ws = [(torch.randn(N_OUT, K, generator=g) * 0.05).to(BF).to(DEV) for _ in range(3)]
        _OPS[K] = (A, Ws)
    return _OPS[K]


def _dense(A, W):
    from one_peace_amd import hip
    return hip.gemm_nt(A, [W], splitk=False)


def _row_mask(segs, total):
    m = np.zeros(total, dtype=bool)
    for ps, r0, S, B in segs:
        m[r0:r0 + S * B] = np.repeat(ps != 0, S)
    return m


def _listed(K, segs, total, grouped, zero_rows):
    """(output [total, N], count, dense product of the same operand): one problem over all rows with weight 0, or a problem per segment
    with its own weight in ONE launch.  The output is pre-filled with NaN and has a NaN guard band behind it."""
    from types import SimpleNamespace
    from one_peace_amd import hip, ops
    A, Ws = _operands(K)
    sgs = [SimpleNamespace(S=S) for _, _, S, _ in segs]
    if zero_rows:
        A = A * torch.from_numpy(_row_mask(segs, total)).to(DEV).to(BF).unsqueeze(1)
    buf = torch.full((total + GUARD, N_OUT), float("nan"), dtype=BF, device=DEV)
    out = buf[:total]
    rs = [slice(r0, r0 + S * B) for _, r0, S, B in segs]
    if grouped:
        members = [(i, i, sg[1]) for i, sg in enumerate(segs)]
        (win,) = hip.live_mwindows(_dev_segs(segs), [members], [out])
        assert ops._dgrad_listed([A[r] for r in rs], Ws, [out[r] for r in rs], win, sgs)
        dense = torch.cat([_dense(A[r].contiguous(), W) for r, W in zip(rs, Ws)])
    else:
        members = [(i, 0, 0) for i in range(len(segs))]
        (win,) = hip.live_mwindows(_dev_segs(segs), [members], [out])
        assert ops._dgrad_listed([A], [Ws[0]], [out], win, sgs)
        dense = _dense(A, Ws[0])
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[total:]).all()), "a window wrote behind the last row"
    prob_rows = [(r.start, r.stop - r.start) for r in rs] if grouped else [(0, total)]
    return out, int(win[1].item()), dense, R.computed_rows(segs, members, prob_rows, total)


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("K", [128, 4608])
@pytest.mark.parametrize("pattern", ["none", "alternating", "adjacent", "first_only", "last_only"])
def test_listed_input_gradient_equals_the_dense_launch(pattern, K, grouped):
    segs, total = three_segments(pattern)
    out, n, dense, _ = _listed(K, segs, total, grouped, True)
    assert not bool(torch.isnan(out).any()), "a row nobody wrote"
    assert torch.equal(out, dense), float((out.float() - dense.float()).abs().max())
    members = [(i, i, sg[1]) for i, sg in enumerate(segs)] if grouped else [(i, 0, 0) for i in range(3)]
    assert n == len(R.expected_windows(segs, members))
    assert float(dense.float().abs().sum()) > 0


@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("K", [128, 4608])
def test_the_windows_really_skip(K, grouped):
    """Control: non-zero rows under a mask that marks them dropped are NOT multiplied -- they come out +0 where no window reaches them
    (a kept neighbour's window reaches the first rows of the next sample: those equal the dense product) and differ from the dense
    product."""
    segs, total = three_segments("alternating")
    out, _, dense, computed = _listed(K, segs, total, grouped, False)
    c = torch.from_numpy(computed).to(DEV)
    assert torch.equal(out[c], dense[c])
    assert bool((out[~c] == 0).all()) and not bool(torch.signbit(out[~c]).any())
    assert int((~c).sum()) > total // 4 and bool((dense[~c] != 0).any(dim=1).all())


@pytest.mark.parametrize("grouped", [False, True])
def test_all_dropped(grouped):
    """Only the strided window of the image samples' last rows is listed (it multiplies zero rows); every row is +0."""
    segs, total = three_segments("all")
    segs = [(np.zeros_like(ps), r0, S, B) for ps, r0, S, B in segs]
    out, n, dense, _ = _listed(128, segs, total, grouped, True)
    assert n == 1
    assert bool((out == 0).all()) and not bool(torch.signbit(out).any()) and torch.equal(out, dense)


def test_one_tile_per_workgroup_form_gives_the_same_bits():
    """tune sched 7: a dense grid of one-tile workgroups, the ones past the count leave at once."""
    from one_peace_amd import hip
    segs, total = three_segments("adjacent")
    A, Ws = _operands(128)
    A = A * torch.from_numpy(_row_mask(segs, total)).to(DEV).to(BF).unsqueeze(1)
    outs = []
    for tune in (0, 7 << 20):
        out = torch.full((total, N_OUT), float("nan"), dtype=BF, device=DEV)
        (win,) = hip.live_mwindows(_dev_segs(segs), [[(i, 0, 0) for i in range(3)]], [out])
        assert hip.gemm_nt_windows([A], [Ws[0]], [out], win, 257, tune=tune)
        outs.append(out)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]) and not bool(torch.isnan(outs[0]).any())
