"""The row windows of the input-gradient GEMMs (tests/dgrad_windows_ref.py): what the rule must guarantee, checked without a GPU."""
import numpy as np
import pytest

from tests import dgrad_windows_ref as R

PATTERNS = ("none", "all", "alternating", "adjacent", "first_only", "last_only")


def patterns(B):
    p = {"none": np.ones(B), "all": np.zeros(B), "alternating": np.ones(B), "adjacent": np.ones(B), "first_only": np.zeros(B),
         "last_only": np.zeros(B)}
    p["alternating"][::2] = 0
    p["adjacent"][[B // 2 - 1, B // 2]] = 0
    p["first_only"][0] = 1
    p["last_only"][B - 1] = 1
    return p


def three_segments(pattern, B=(8, 6, 6), S=(64, 257, 250)):
    """text | image | audio in one matrix, each segment with another pattern"""
    segs, row0 = [], 0
    for i in range(3):
        segs.append((patterns(B[i])[PATTERNS[(PATTERNS.index(pattern) + i) % len(PATTERNS)]], row0, S[i], B[i]))
        row0 += S[i] * B[i]
    return segs, row0


def test_the_rule_at_the_sequence_lengths_in_use():
    assert R.window_rule(257) == (1, True)    # image 224 / 16: one window per sample + the strided row
    assert R.window_rule(250) == (1, False)   # audio: 6 surplus rows per window
    assert R.window_rule(1025) == (4, True)
    assert R.window_rule(512) == (2, False)
    for S in (1, 16, 64, 100, 243, 258, 785):
        assert R.window_rule(S) == (0, False), S
    assert R.window_rule(244) == (1, False)   # 256 / 244 = 1.049
    from one_peace_amd import hip
    for S in range(1, 1300):
        assert hip.mwindow_rule(S) == R.window_rule(S), S


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("case", ["257x6", "250x6", "64x8", "100x16", "785x3", "three"])
def test_every_kept_row_is_computed_and_every_other_row_is_zeroed(case, pattern):
    if case == "three":
        segs, total = three_segments(pattern)
    else:
        S, B = (int(v) for v in case.split("x"))
        segs, total = [(patterns(B)[pattern], 0, S, B)], S * B
    layouts = [([(i, 0, 0) for i in range(len(segs))], [(0, total)])]                       # one problem over all rows
    layouts.append(([(i, i, sg[1]) for i, sg in enumerate(segs)], [(sg[1], sg[2] * sg[3]) for sg in segs]))  # a problem per segment
    kept_row = np.zeros(total, dtype=bool)
    for ps, row0, S, B in segs:
        kept_row[row0:row0 + S * B] = np.repeat(ps != 0, S)
    for members, prob_rows in layouts:
        wins = R.expected_windows(segs, members)
        assert all(0 <= r and r + (n - 1) * st < prob_rows[p][1] if st > 1 else 0 <= r < prob_rows[p][1] for p, r, st, n in wins), \
            "a window starts outside its problem, or a strided one leaves it"
        assert len(set(wins)) == len(wins)
        computed = R.computed_rows(segs, members, prob_rows, total)
        zeroed = R.zero_filled_rows(segs, total)
        assert computed[kept_row].all(), "a row of a kept sample that no launch computes"
        assert (computed | zeroed).all(), "a row nobody writes"
        assert not (zeroed & kept_row).any(), "a kept row is zeroed"
        if not kept_row.any():
            assert all(st > 1 for _, _, st, _ in wins) and zeroed.all()  # (only the strided windows, which take every sample)
        if kept_row.all():
            assert not zeroed.any()


def test_window_count_over_the_headline_drop_schedule():
    """128 samples per modality (text 64, image 257, audio 250 rows), 40 layers with drop rates linspace(0, 0.4, 40), independent
    masks, 5 seeded draws: the windows over all rows (the strided one of the image rows included) are at most 0.85 of the 286 aligned
    tiles (the simulation gives 0.83); skipping on the aligned grid alone would keep 0.95."""
    rng = np.random.default_rng(0)
    S, B = (64, 257, 250), 128
    row0 = [0, S[0] * B, (S[0] + S[1]) * B]
    total = sum(S) * B
    dense = R.dense_tiles([(0, total)])
    assert dense == 286
    wins = aligned = n = 0
    for _ in range(5):
        for rate in np.linspace(0, 0.4, 40):
            segs = [((rng.random(B) >= rate).astype(np.float32), row0[i], S[i], B) for i in range(3)]
            wins += len(R.expected_windows(segs, [(i, 0, 0) for i in range(3)]))
            kept_row = np.concatenate([np.repeat(q[0] != 0, q[2]) for q in segs])
            aligned += sum(bool(kept_row[256 * t:256 * t + 256].any()) for t in range(dense))
            n += 1
    assert wins / (n * dense) <= 0.85, wins / (n * dense)
    assert 0.80 <= wins / (n * dense), "fewer windows than kept samples need: the rule lost rows"
    assert aligned / (n * dense) >= 0.93
