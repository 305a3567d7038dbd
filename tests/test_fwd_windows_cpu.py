"""The forward GEMMs of a residual branch over row windows (ops.SKIP_ZERO_FWD): what the fill must guarantee, and when the dense
launches take over, checked without a GPU.

The lists are those of the input gradients (tests/dgrad_windows_ref.py).  The launch that builds them FILLS the rows of every unit
(sample / aligned tile) it did not list: +0 in a plain output (q | k | v, h0 | h1), a copy of the residual input's rows in the
branch output -- what the dense epilogue's fma(0, y, res) gives for a dropped sample."""
import os

import numpy as np
import pytest
import torch

from tests import dgrad_windows_ref as R
from tests.test_dgrad_windows_cpu import PATTERNS, patterns, three_segments


def fill_rule(segs, total, out, src=None):
    """NumPy rule of the fill: `out` [>= total rows] with the rows of R.zero_filled_rows set to +0 (src None) or to src's rows."""
    filled = R.zero_filled_rows(segs, total)
    res = np.array(out, copy=True)
    res[:total][filled] = 0.0 if src is None else np.asarray(src)[:total][filled]
    return res, filled


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", ["257x6", "250x6", "64x8", "100x16", "785x3", "three"])
def test_every_row_is_computed_or_filled(case, pattern):
    if case == "three":
        segs, total = three_segments(pattern)
    else:
        S, B = (int(v) for v in case.split("x"))
        segs, total = [(patterns(B)[pattern], 0, S, B)], S * B
    layouts = [([(i, 0, 0) for i in range(len(segs))], [(0, total)]),                                        # q|k|v, out-proj
               ([(i, i, sg[1]) for i, sg in enumerate(segs)], [(sg[1], sg[2] * sg[3]) for sg in segs])]      # grouped FFN launches
    kept_row = np.zeros(total, dtype=bool)
    for ps, row0, S, B in segs:
        kept_row[row0:row0 + S * B] = np.repeat(ps != 0, S)
    rng = np.random.default_rng(1)
    resid = rng.standard_normal((total + 7, 8)).astype(np.float32)
    nan = np.full((total + 7, 8), np.nan, dtype=np.float32)
    for members, prob_rows in layouts:
        computed = R.computed_rows(segs, members, prob_rows, total)
        plain, filled = fill_rule(segs, total, nan)
        copied, _ = fill_rule(segs, total, nan, resid)
        assert (computed | filled).all(), "a row nobody writes"
        assert computed[kept_row].all() and not (filled & kept_row).any(), "a kept row must come from a window, never from the fill"
        # the fill: +0 (sign bit clear) / the residual's rows; every other row and the rows behind the matrix untouched
        assert (plain[:total][filled] == 0).all() and not np.signbit(plain[:total][filled]).any()
        assert np.array_equal(copied[:total][filled], resid[:total][filled])
        assert np.isnan(plain[:total][~filled]).all() and np.isnan(copied[:total][~filled]).all()
        assert np.isnan(plain[total:]).all() and np.isnan(copied[total:]).all()
        # a dropped sample's rows a neighbour's window reaches are filled AND computed (the GEMM runs later on the stream)
        if pattern == "alternating" and case in ("250x6", "three"):
            assert (computed & filled).any()


def _segs(S=(64, 257, 250), B=(8, 6, 6), none=False):
    out, row0 = [], 0
    for s, b in zip(S, B):
        out.append((None if none else torch.ones(b), row0, s, b, 1))
        row0 += s * b
    return out, row0


def test_the_switch_comes_from_the_environment_and_defaults_to_on():
    from one_peace_amd import ops
    assert ops.SKIP_ZERO_FWD == (os.environ.get("ONEPEACE_SKIP_ZERO_FWD", "1") != "0")


def test_when_the_dense_launches_take_over(monkeypatch):
    """ops._fwd_windows_apply decides from shapes and flags alone."""
    from one_peace_amd import hip, ops
    segs, total = _segs()
    dev = torch.device("cpu")
    good = [(total, 768, 128, hip.EPI_BIAS, True), (total, 256, 128, hip.EPI_RESID, True)]
    monkeypatch.setattr(ops, "SKIP_ZERO_FWD", True)
    assert ops._fwd_windows_apply(segs, 1, 2, good, dev)
    assert not ops._fwd_windows_apply(segs, 1, 2, good, dev, flags=False)      # y wanted / fp8 / kept / row tables / a padded segment
    assert not ops._fwd_windows_apply(_segs(none=True)[0], 1, 2, good, dev)     # no multipliers (layer 0, eval, teacher passes)
    assert ops._fwd_windows_apply(segs[:1] + _segs(none=True)[0][1:], 1, 2, good, dev)  # some segment has them
    for bad in ((total, 768 + 128, 128, hip.EPI_BIAS, True),     # N % 256
                (total, 768, 160, hip.EPI_BIAS, True),           # K % 64
                (total, 768, 64, hip.EPI_BIAS, True),            # K < 128
                (total, 1 << 15, 128, hip.EPI_BIAS, True),       # 257 * ld >= 2^23: the strided window's row stride
                (1 << 21, 768, 128, hip.EPI_BIAS, True)):        # M * ld >= 2^30
        assert not ops._fwd_windows_apply(segs, 1, 2, good[1:] + [bad], dev), bad
    assert not ops._fwd_windows_apply([(torch.ones(1 << 20), 0, 257, 1 << 20, 1)], 1, 2, good, dev)  # S * B >= 2^28: the entry format
    assert not ops._fwd_windows_apply([(torch.ones(8, dtype=torch.float64), 0, 64, 8, 1)], 1, 2, good, dev)
    assert not ops._fwd_windows_apply([(torch.ones(4), 0, 64, 8, 1)], 1, 2, good, dev)               # fewer multipliers than samples
    assert not ops._fwd_windows_apply(segs * 2, 1, 2, good, dev) and not ops._fwd_windows_apply(segs, 5, 2, good, dev)
    # a dense launch that would split K (a few row tiles, long K): a window never splits, so its bits would differ
    M, N, K = 512, 512, 1536

    def host_scratch(M, N, K, epilogue, device):  # (hip.splitk_scratch's rule with host memory: the real one asks for a GPU stream)
        if epilogue in (hip.EPI_BIAS, hip.EPI_RESID) and (K >= 2048 or M <= 1024):
            return torch.empty(min(hip.SPLITK_WS_BYTES, 32 * M * N), dtype=torch.uint8)
        return None
    monkeypatch.setattr(hip, "splitk_scratch", host_scratch)
    ws = hip.splitk_scratch(M, N, K, hip.EPI_BIAS, dev)
    assert ws is not None and hip.gemm_plan(M, N, K, hip.EPI_BIAS, False, ws.numel())[1] > 1
    assert not ops._fwd_windows_apply([(torch.ones(8), 0, 64, 8, 1)], 1, 2, [(M, N, K, hip.EPI_BIAS, False)], dev)
    monkeypatch.setattr(ops, "SKIP_ZERO_FWD", False)                            # ONEPEACE_SKIP_ZERO_FWD=0
    assert not ops._fwd_windows_apply(segs, 1, 2, good, dev)
