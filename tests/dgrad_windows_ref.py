"""NumPy restatement of the row windows of the input-gradient GEMMs (hip.mwindow_rule, op_live_mwindows, ops._dgrad_listed).

A residual branch under the multiplier form of stochastic depth has all-zero gradient rows for the samples it dropped.  Its input
gradients dy W^T run over 256-row windows instead of the aligned 256-row grid:

  * a segment whose samples nearly fill whole windows (S' = S - 1 when S % 256 == 1, else S; ceil(S' / 256) * 256 <= 1.05 S') lists
    ceil(S' / 256) windows per KEPT sample, from the sample's first row on; with S % 256 == 1 the last rows of all samples, kept or
    not, form strided windows (row stride S, 256 samples to a window) of the same launch;
  * any other segment lists the aligned 256-row tiles (from the segment's first row on) that hold a row of a kept sample;
  * the launch that builds the lists writes +0 into the rows of every sample (first form) or tile (second form) it did not list.

Segments: (ps [B] or None = all kept, row0, S, B); a list's members: (segment index, problem index, row of the row matrix at which
the problem's operand starts); an entry: (problem, first row inside the problem, row stride, rows)."""
import numpy as np


def window_rule(S):
    """(windows per kept sample, or 0 for aligned tiles; whether every sample's last row goes to strided windows)"""
    odd = S > 1 and S % 256 == 1
    Sp = S - 1 if odd else S
    n = -(-Sp // 256)
    return (n, odd) if n * 256 * 100 <= 105 * Sp else (0, False)


def _kept(ps, B):
    return np.ones(B, dtype=bool) if ps is None else np.asarray(ps)[:B] != 0


def expected_windows(segs, members):
    out = []
    for i, prob, base in members:
        ps, row0, S, B = segs[i]
        kept = _kept(ps, B)
        wps, odd = window_rule(S)
        if wps:
            out += [(prob, row0 - base + int(b) * S + 256 * w, 1, 256) for b in np.flatnonzero(kept) for w in range(wps)]
        else:
            row_kept = np.repeat(kept, S)
            out += [(prob, row0 - base + 256 * t, 1, 256) for t in range(-(-S * B // 256)) if row_kept[256 * t:256 * t + 256].any()]
        if odd:
            out += [(prob, row0 - base + b0 * S + S - 1, S, min(256, B - b0)) for b0 in range(0, B, 256)]
    return out


def zero_filled_rows(segs, total):
    """bool [total]: rows of the row matrix the list-building launch sets to +0"""
    z = np.zeros(total, dtype=bool)
    for ps, row0, S, B in segs:
        kept = _kept(ps, B)
        if window_rule(S)[0]:
            z[row0:row0 + S * B] = ~np.repeat(kept, S)
        else:
            row_kept = np.repeat(kept, S)
            for t in range(-(-S * B // 256)):
                if not row_kept[256 * t:256 * t + 256].any():
                    z[row0 + 256 * t:row0 + min(256 * t + 256, S * B)] = True
    return z


def computed_rows(segs, members, prob_rows, total):
    """bool [total]: rows some window of the list writes (clipped to its problem: prob_rows[p] = (first row, rows))"""
    c = np.zeros(total, dtype=bool)
    for prob, r, stride, rows in expected_windows(segs, members):
        p0, n = prob_rows[prob]
        c[p0 + r:p0 + min(r + stride * rows, n):stride] = True
    return c


def dense_tiles(prob_rows):
    return sum(-(-n // 256) for _, n in prob_rows)
