"""Backward work of the samples stochastic depth dropped is skipped, bit for bit (ops.SKIP_ZERO_BACKWARD).

The multiplier form of stochastic depth multiplies a dropped sample's branch output by ps = 0; in backward op_resid_bwd writes
ps * dout, so the rows of a dropped sample are exactly zero in every gradient matrix of the branch.  A weight gradient is a GEMM whose
K dimension is the token rows: a 64-row K-tile inside dropped samples multiplies a zero operand tile.  op_live_ktiles lists the tiles
that hold a row of a kept sample, op_gemm_tn_grouped_lists walks that list.  Every check here is torch.equal: an fp32 accumulator that
starts at +0 is not changed by +-0 products."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import synth
from tests.model_util import TinyDictionary, load_synth

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF = torch.bfloat16


# ------------------------------------------------------------------------------------------------------------------
# K-tile lists
# ------------------------------------------------------------------------------------------------------------------
def _ps_patterns(B):
    pats = {"none": np.ones(B), "all": np.zeros(B), "first_last": np.ones(B), "adjacent": np.ones(B), "alternating": np.ones(B)}
    pats["first_last"][[0, B - 1]] = 0
    pats["adjacent"][[B // 2, B // 2 + 1]] = 0
    pats["alternating"][::2] = 0
    if B == 16:  # more for the weight gradient: a long run of dropped tiles inside the steady loop, and lists of three and of two tiles
        pats["middle_run"], pats["one_kept"], pats["first_kept"] = np.ones(B), np.zeros(B), np.zeros(B)
        pats["middle_run"][3:12] = 0
        pats["one_kept"][5] = 1
        pats["first_kept"][0] = 1
    return pats


def _live_ref(segs, row0, rows):
    """NumPy restatement: tile t of the problem is live when one of its 64 rows belongs to a sample with ps != 0."""
    live_row = np.zeros(row0 + rows + 64, dtype=bool)
    for ps, r0, S, B in segs:
        for b in range(B):
            lo, hi = r0 + b * S, min(r0 + (b + 1) * S, live_row.size)
            if ps is None or ps[b] != 0:
                live_row[lo:hi] = True
    return [t for t in range(rows // 64) if live_row[row0 + 64 * t:row0 + 64 * t + 64].any()]


def _check_lists(segs_np, probs):
    from one_peace_amd import hip
    segs = [(torch.tensor(ps, dtype=torch.float32, device=DEV) * 1.25 if ps is not None else None, r0, S, B) for ps, r0, S, B in segs_np]
    got = hip.live_ktiles(segs, probs, torch.device(DEV))
    torch.cuda.synchronize()
    for (lst, cnt), (row0, rows) in zip(got, probs):
        want = _live_ref(segs_np, row0, rows)
        n = int(cnt.item())
        assert n == len(want), (n, len(want))
        assert lst[:n].tolist() == want
    return got


@pytest.mark.parametrize("pattern", ["none", "all", "first_last", "adjacent", "alternating"])
def test_live_ktiles_one_segment_where_a_tile_is_a_sample(pattern):
    ps = _ps_patterns(8)[pattern]
    _check_lists([(ps, 0, 64, 8)], [(0, 512)])


@pytest.mark.parametrize("pattern", ["none", "all", "first_last", "adjacent", "alternating"])
def test_live_ktiles_one_segment_misaligned(pattern):
    """S = 100, 16 samples: 25 tiles, a tile straddles up to two samples."""
    ps = _ps_patterns(16)[pattern]
    _check_lists([(ps, 0, 100, 16)], [(0, 1600)])


@pytest.mark.parametrize("pattern", ["none", "all", "first_last", "adjacent", "alternating"])
def test_live_ktiles_three_segments_whole_matrix_and_per_segment(pattern):
    """Text / image / audio segments (S = 64 / 257 / 250, 4 samples each), each padded to a multiple of 64 rows; one problem over the
    whole matrix (q|k|v, out-proj), one per segment (the FFN weights); the FFN pattern is another one than the attention pattern.
    Also the per-row form the lock-step attention branch uses (S = 1, one multiplier per row)."""
    pats = _ps_patterns(4)
    names = sorted(pats)
    S = (64, 257, 250)
    rows = [(4 * s + 63) // 64 * 64 for s in S]
    row0 = [0, rows[0], rows[0] + rows[1]]
    total = sum(rows)
    segs = [(pats[names[(names.index(pattern) + i) % len(names)]], row0[i], S[i], 4) for i in range(3)]
    _check_lists(segs, [(0, total)] + [(row0[i], rows[i]) for i in range(3)])
    per_row = np.zeros(total)
    for ps, r0, s, B in segs:
        per_row[r0:r0 + s * B] = np.repeat(ps, s)
    _check_lists([(per_row, 0, 1, total)], [(0, total)])


# ------------------------------------------------------------------------------------------------------------------
# weight gradient
# ------------------------------------------------------------------------------------------------------------------
_WG = {}


def _wg_operands():
    """Three problems of ONE launch: outputs 256 x 256, 512 x 256, 384 x 256 (guarded edge), K = 1600 rows = 16 samples x 100."""
    if not _WG:
        g = torch.Generator(device="cpu").manual_seed(5)
        K = 1600
        for i, M in enumerate((256, 512, 384)):
            A = torch.randn(K, M, generator=g).to(BF).to(DEV)
            B = torch.randn(K, 256, generator=g).to(BF).to(DEV)
            C0 = torch.randn(M, 256, generator=g).to(BF).to(DEV)
            W = (torch.randn(M, 256, generator=g) * 0.1).to(BF).to(DEV)
            gam = (torch.rand(M, generator=g) + 0.5).to(BF).to(DEV)
            _WG[i] = (A, B, C0, W, gam)
    return _WG


def _wg_run(ps_np, lists, accumulate, side=False, zero_rows=True):
    """C (and rowdot) of the three problems; lists: walk the live K-tile lists of ps; zero_rows: True = the dropped samples' rows of A
    are zero, False = A as it is, (lo, hi) = rows lo .. hi - 1 are zero."""
    from one_peace_amd import hip
    ps = torch.tensor(ps_np, dtype=torch.float32, device=DEV)
    rowmask = ps.repeat_interleave(100).ne(0).to(BF).unsqueeze(1)
    if isinstance(zero_rows, tuple):
        rowmask = torch.ones_like(rowmask)
        rowmask[zero_rows[0]:zero_rows[1]] = 0
        zero_rows = True
    probs, outs, rds, kts = [], [], [], []
    for i in range(3):
        A, B, C0, W, gam = _wg_operands()[i]
        Az = A * rowmask if zero_rows else A
        C = C0.clone()
        use_side = side and i < 2  # (the row dot needs full 256 x 256 tiles: not the guarded 384-row problem)
        rd = torch.full((2, A.shape[1]), 7.0, dtype=torch.float32, device=DEV) if use_side else None
        probs.append((Az, B, C, accumulate or use_side, (W, rd, gam) if use_side else None))
        outs.append(C)
        rds.append(rd)
        kts.append(hip.live_ktiles([(ps, 0, 100, 16)], [(0, 1600)], torch.device(DEV))[0] if lists else None)
    assert hip.gemm_tn_grouped(probs, ktiles=kts if lists else None)
    torch.cuda.synchronize()
    return outs, rds


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("pattern", ["none", "first_last", "adjacent", "alternating", "middle_run", "one_kept", "first_kept"])
def test_listed_weight_gradient_equals_the_full_product(pattern, accumulate):
    ps = _ps_patterns(16)[pattern]
    full, _ = _wg_run(ps, False, accumulate)
    got, _ = _wg_run(ps, True, accumulate)
    for a, b in zip(full, got):
        assert torch.equal(a, b), float((a.float() - b.float()).abs().max())


def test_listed_weight_gradient_with_rowdot_and_rscale():
    ps = _ps_patterns(16)["alternating"]
    full, rd_full = _wg_run(ps, False, True, side=True)
    got, rd_got = _wg_run(ps, True, True, side=True)
    for a, b in zip(full, got):
        assert torch.equal(a, b)
    for a, b in zip(rd_full[:2], rd_got[:2]):
        assert torch.equal(a, b) and bool((a != 7.0).all())


@pytest.mark.parametrize("accumulate", [False, True])
def test_all_dropped_weight_gradient(accumulate):
    """An empty list: an accumulated gradient keeps its input, a fresh one is zero; the row dots are written (zeros)."""
    ps = np.zeros(16)
    got, _ = _wg_run(ps, True, accumulate)
    full, _ = _wg_run(ps, False, accumulate)
    for i in range(3):
        want = _wg_operands()[i][2] if accumulate else torch.zeros_like(got[i])
        assert torch.equal(got[i], want) and torch.equal(got[i], full[i])
    got, rd = _wg_run(ps, True, True, side=True)
    for i in range(3):
        assert torch.equal(got[i], _wg_operands()[i][2])
    assert all(bool((r == 0).all()) for r in rd[:2])


def test_the_list_really_skips():
    """Control: non-zero rows under a list that marks them dropped are NOT multiplied -- the result differs from the full product and
    equals the product of the matrix with those rows zeroed."""
    ps = _ps_patterns(16)["adjacent"]
    full, _ = _wg_run(ps, False, False, zero_rows=False)
    got, _ = _wg_run(ps, True, False, zero_rows=False)
    assert all(not torch.equal(a, b) for a, b in zip(full, got))
    # samples 8 and 9 = rows 800 .. 999: the tiles 13 and 14 (rows 832 .. 959) lie inside them and are left out; zero exactly those rows
    want, _ = _wg_run(np.ones(16), False, False, zero_rows=(832, 960))
    assert all(torch.equal(a, b) for a, b in zip(want, got))


# ------------------------------------------------------------------------------------------------------------------
# model level
# ------------------------------------------------------------------------------------------------------------------
def test_training_step_is_bit_identical_with_and_without_the_skip():
    """One lock-step tri-modal training step of a 2-layer model (drop-path 0.4, fixed seed, 64 samples per modality so that every
    weight-gradient problem has K % 64 == 0 and rides on the grouped launch): ops.SKIP_ZERO_BACKWARD on and off (what
    ONEPEACE_SKIP_ZERO_BACKWARD=0 sets) give the same loss and the same flat gradient buffer, bit for bit.  The masks are Bernoulli(0.6)
    draws of a seeded generator plus two runs of dropped neighbours (text samples 0 .. 7 in the attention branch, image samples 4 .. 15 in
    the FFN branch), so that whole K-tiles are certain to be left out (a text sample is 16 rows, an image sample 17)."""
    from one_peace_amd import hip, ops
    from one_peace_amd.criterions.contrastive import TriModalContrastiveCriterion
    from one_peace_amd.distributed import FlatParameters
    from one_peace_amd.one_peace.one_peace_retrieval import OnePeaceRetrievalModel
    from one_peace_amd.transformer import transformer_encoder as TE
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    cfg = dict(embed_dim=256, ffn_embed_dim=512, layers=2, attention_heads=4, image_rel_bucket_size=4, text_bucket_size=256,
               audio_bucket_size=512)
    B = 64
    inp = synth.synth_inputs(B, text_len=15, image_res=64, audio_samples=8000, vocab=1000)
    inp = {k: (v.to(DEV).to(BF) if v.is_floating_point() else v.to(DEV)) for k, v in inp.items()}
    orig, orig_live, orig_scales = ops.SKIP_ZERO_BACKWARD, hip.live_ktiles, TE.TransformerEncoder._draw_path_scales
    mask = torch.bernoulli(torch.full((2, 3 * B), 0.6), generator=torch.Generator(device="cpu").manual_seed(3)).bool()
    mask[0, :8] = False
    mask[1, B + 4:B + 16] = False

    def fixed_scales(self, nb, device):
        assert nb == 3 * B
        return [(None, None), ((mask[0].float() / 0.6).to(device), (mask[1].float() / 0.6).to(device))]
    res, calls = {}, {}
    try:
        TE.TransformerEncoder._draw_path_scales = fixed_scales
        for on in (True, False):
            ops.SKIP_ZERO_BACKWARD = on
            calls[on] = []

            def counted(segs, probs, device, _on=on):
                out = orig_live(segs, probs, device)
                calls[_on].append(out)
                return out
            hip.live_ktiles = counted
            enc = one_peace_encoder_config(drop_path_rate=0.4, layer_scale_init_value=1e-1, **cfg)
            torch.manual_seed(0)
            m = load_synth(OnePeaceRetrievalModel(SimpleNamespace(encoder=enc, copy_rel_pos_table=False), TinyDictionary(1000), "val"))
            m = m.to(DEV).to(BF).train()
            fl = FlatParameters(m)
            loss, _, _ = TriModalContrastiveCriterion(None, 0.0, lock_step=True)(m, {"net_input": inp, "nsentences": B})
            fl.zero_grad()
            loss.backward()
            torch.cuda.synchronize()
            res[on] = (loss.detach().clone(), fl.grads.detach().clone())
    finally:
        ops.SKIP_ZERO_BACKWARD, hip.live_ktiles, TE.TransformerEncoder._draw_path_scales = orig, orig_live, orig_scales
    assert not calls[False]
    # layer 0 has drop-path 0 (linspace), layer 1 has 0.4: one launch for its attention branch, one for its FFN branch
    assert len(calls[True]) >= 2, len(calls[True])
    counts = [int(c.item()) for out in calls[True] for _, c in out]
    sizes = [lst.numel() for out in calls[True] for lst, _ in out]
    assert any(c < n for c, n in zip(counts, sizes)), (counts, sizes)  # some tile really was left out
    assert torch.equal(res[True][0], res[False][0])
    assert torch.equal(res[True][1], res[False][1])
    assert float(res[True][1].float().abs().sum()) > 0
