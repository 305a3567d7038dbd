"""csrc/masks.hip on the device: op_mask_patches / op_mask_words / op_mask_blocks against tests/masks_ref.py on the same keys, the
reference's recorded cases (tests/golden/pretrain_masks.pt), and the two generators in front of the pretraining criteria.  Outputs sit
between guard regions, every case runs twice with identical bits, every comparison is exact."""
import ctypes
import math
import os

import pytest
import torch

from one_peace_amd import hip, ops
from one_peace_amd.pretrain_masks import AudioTextPretrainMasks, ImageTextPretrainMasks
from tests import masks_ref as MR
from tests.test_photometric_gpu import GUARD, Guarded
from tests.test_pretrain_masks_cpu import BLOCK_T, TABLE, block_inputs, rand_keys, run_fixture, word_batch

pytestmark = pytest.mark.gpu
DEV = "cuda"


def twice(call, specs):
    """call(outs) on two sets of guarded output buffers, pre-filled with 0xAB; specs: (shape, dtype) per output, or None.  The guards are
    intact, the two runs agree bit for bit; the outputs of the first run on the host."""
    runs = []
    for _ in range(2):
        gs = [None if s is None else Guarded(s[0], s[1]) for s in specs]
        for g in gs:
            if g is not None:
                g.raw[GUARD:GUARD + g.n] = 0xAB
        call(tuple(None if g is None else g.t for g in gs))
        torch.cuda.synchronize()
        assert all(g is None or g.intact() for g in gs)
        runs.append([None if g is None else g.t.view(torch.uint8).cpu() for g in gs])
    assert all(a is None or torch.equal(a, b) for a, b in zip(*runs))
    return [None if s is None else r.view(s[1]) for r, s in zip(runs[0], specs)]


# ---- patches ---------------------------------------------------------------------------------------------------------------------
def patches_case(N, B, ratios, seed):
    g = torch.Generator().manual_seed(seed)
    ka, kb = rand_keys(g, B, N), rand_keys(g, B, N)
    ka[0, ::2], kb[0, 1::2] = 0, 2 ** 31 - 1          # the smallest and the largest key
    if B > 1:
        ka[1], kb[1] = 7, 7                            # every key equal: the index decides
    m1 = int(N * ratios[0])
    m2 = int(N * ratios[1])
    extra = m2 - (N - m1)
    dka, dkb = ka.to(DEV), kb.to(DEV)
    specs = [((B, N + 1), torch.bool), ((B, N + 1 - m1), torch.int64), ((B, N + 1), torch.bool), ((B, N + 1 - m2), torch.int64)]
    m, ids, vm, vids = twice(lambda out: hip.mask_patches(dka, m1, dkb, extra, out=out), specs)
    want = [MR.patches(ka[b].tolist(), kb[b].tolist(), m1, extra) for b in range(B)]
    wm, wi = MR.pack([w[0] for w in want], N + 1, N + 1 - m1)
    assert torch.equal(m, wm) and torch.equal(ids, wi)
    wm, wi = MR.pack([w[1] for w in want], N + 1, N + 1 - m2)
    assert torch.equal(vm, wm) and torch.equal(vids, wi)
    assert m.sum(1).tolist() == [m1] * B and vm.sum(1).tolist() == [m2] * B and bool((vm | m)[:, 1:].all())
    got = ops.patch_masks(dka, dkb, m1, extra)          # the public route: the same bits, and the CPU route's
    cpu = ops.patch_masks(ka, kb, m1, extra)
    for a, b, c in zip(got, (m, ids, vm, vids), cpu):
        assert torch.equal(a.cpu(), b) and torch.equal(b, c)
    only = twice(lambda out: hip.mask_patches(dka, m1, out=out + (None, None)), specs[:2])   # the first mask alone
    assert torch.equal(only[0], m) and torch.equal(only[1], ids)


@pytest.mark.parametrize("B", [1, 3, 130])
@pytest.mark.parametrize("N", [1, 4, 49, 256, 784])
def test_patches_equal_restatement(N, B):
    patches_case(N, B, (1.0, 1.0) if N == 1 else (0.75, 0.6875), 100 * N + B)


@pytest.mark.parametrize("ratios", [(0.75, 0.25), (0.5, 1.0), (1.0, 0.3)], ids=["extra0", "extra_m1", "m1_N"])
def test_patches_edge_counts(ratios):
    patches_case(16, 3, ratios, 5)


def test_patches_at_the_row_limit():
    patches_case(4096, 2, (0.75, 0.6875), 6)
    with pytest.raises(ValueError):
        ops.patch_masks(torch.zeros(1, 4097, dtype=torch.int32, device=DEV), torch.zeros(1, 4097, dtype=torch.int32, device=DEV), 5, 1)


# ---- words -----------------------------------------------------------------------------------------------------------------------
def words_batch():
    g = torch.Generator().manual_seed(5)
    rows_n = list(range(0, 71)) + [-1, -1]               # captions of 0 ... 70 tokens and two all-pad rows
    L = 71
    tok = word_batch(g, TABLE, rows_n, L)
    tok[40, :40] = torch.tensor([5] + [6] * 39)          # ONE word of 40 tokens (W = 1) running to the caption's end
    tok[41, :3] = torch.tensor([6, 9, 5])                # the first tokens start no word
    tok[42, :42] = 6                                     # W = 0
    tok[43, :43] = torch.tensor(([5] + [6] * 9) * 4 + [7, 6, 6])   # words of 10 tokens: few tokens stay unmasked at p = 0.4
    tok[44, 3] = 4000                                    # a token outside the table starts no word and is never read
    ka, kb = rand_keys(g, len(rows_n), L), rand_keys(g, len(rows_n), L)
    ka[10], kb[10] = 3, 3
    return tok, ka, kb, rows_n


def words_case(tok, ka, kb, p, vl, width):
    B, L = tok.shape
    dtok, dka, dkb, dtab = tok.to(DEV), ka.to(DEV), None if kb is None else kb.to(DEV), TABLE.to(DEV)
    w0, w1 = (L + 1, L + 1) if width is None else width
    specs = [((B, L + 1), torch.bool), ((B, w0), torch.int64), ((B, L + 1), torch.bool) if vl is not None else None,
             ((B, w1), torch.int64) if vl is not None else None, ((2, B), torch.int32)]
    m, ids, vm, vids, counts = twice(lambda out: hip.mask_words(dtok, dtab, dka, p, dkb, vl or 0.0, 1, w0, w1, out=out), specs)
    want = [MR.words(tok[b].tolist(), TABLE.tolist(), ka[b].tolist(), p, None if kb is None else kb[b].tolist(), vl) for b in range(B)]
    wm, wi = MR.pack([w[0] for w in want], L + 1, w0)
    assert torch.equal(m, wm) and torch.equal(ids, wi)
    assert counts[0].tolist() == [len(MR.preserve(w[0])) for w in want]          # the kept counts, not truncated
    if vl is not None:
        wm, wi = MR.pack([w[1] for w in want], L + 1, w1)
        assert torch.equal(vm, wm) and torch.equal(vids, wi)
        assert counts[1].tolist() == [len(MR.preserve(w[1])) for w in want]
    return want, (m, ids, vm, vids)


@pytest.mark.parametrize("p,vl", [(0.15, 0.4), (0.4, None), (1.0, 1.0)])
def test_words_equal_restatement(p, vl):
    tok, ka, kb, rows_n = words_batch()
    want, (m, ids, vm, vids) = words_case(tok, ka, kb if vl is not None else None, p, vl, None)
    if vl == 0.4:   # a row where fewer than k2 tokens are unmasked: the fallback order was exercised
        assert any(int(w[2] * vl) > w[2] - sum(w[0]) for w in want)
    for b, n in enumerate(rows_n):
        n = max(n, 0)
        assert not m[b, 0] and not m[b, n + 1:].any()
    # the public route: width=None cuts both id tensors to the batch maxima; the CPU route gives the same bits
    got = ops.word_masks(tok.to(DEV), TABLE.to(DEV), ka.to(DEV), p, kb.to(DEV) if vl is not None else None, vl)
    cpu = ops.word_masks(tok, TABLE, ka, p, kb if vl is not None else None, vl)
    for a, c in zip(got, cpu):
        assert (a is None and c is None) or (a.device.type == "cuda" and torch.equal(a.cpu(), c))
    assert got[1].shape[1] == max(len(MR.preserve(w[0])) for w in want) and torch.equal(got[1].cpu(), ids[:, :got[1].shape[1]])


def test_words_width_bound_and_overflow():
    """An explicit width is an upper bound without a synchronisation; a row that keeps more positions is truncated to the first `width`
    (nothing is written beyond its row: the guards and the neighbouring rows) and the overflow flag is raised."""
    tok, ka, kb, _ = words_batch()
    tok, ka, kb = tok[:24, :24].contiguous(), ka[:24, :24].contiguous(), kb[:24, :24].contiguous()
    tok[23, 23] = 2
    for width in ((25, 25), (25, 20), (12, 25), (3, 1), (0, 0)):
        words_case(tok, ka, kb, 0.15, 0.4, width)
    d = [t.to(DEV) for t in (tok, TABLE, ka, kb)]
    free = ops.word_masks(d[0], d[1], d[2], 0.15, d[3], 0.4)
    w0, w1 = free[1].shape[1], free[3].shape[1]
    assert not bool(free[4]) and not bool(ops.word_masks(d[0], d[1], d[2], 0.15, d[3], 0.4, width=(w0, w1))[4])
    for width in ((w0 - 1, w1), (w0, w1 - 1)):
        got = ops.word_masks(d[0], d[1], d[2], 0.15, d[3], 0.4, width=width)
        assert bool(got[4]) and got[4].device.type == "cuda"
        assert torch.equal(got[1].cpu(), free[1][:, :width[0]].cpu()) and torch.equal(got[3].cpu(), free[3][:, :width[1]].cpu())


def test_words_strided_rows():
    tok, ka, kb, _ = words_batch()
    wide = torch.full((tok.shape[0], 100), 1, dtype=torch.int64)
    wide[:, :71] = tok
    got = ops.word_masks(wide.to(DEV)[:, :71], TABLE.to(DEV), ka.to(DEV), 0.15, kb.to(DEV), 0.4)
    cpu = ops.word_masks(tok, TABLE, ka, 0.15, kb, 0.4)
    assert all(torch.equal(a.cpu(), c) for a, c in zip(got, cpu))


@pytest.mark.parametrize("p", [0.15, 0.4])
def test_words_float32_ceil(p):
    """k = ceil(float32(W) * p) in the kernel, for every W in 1 ... 512, against torch's statement."""
    want = [int(math.ceil(torch.ones(W, dtype=torch.uint8).float().sum() * p)) for W in range(1, 513)]
    tok = torch.full((512, 513), 1, dtype=torch.int64)
    for W in range(1, 513):
        tok[W - 1, :W], tok[W - 1, W] = 5, 2
    keys = rand_keys(torch.Generator().manual_seed(1), 512, 513)
    m = ops.word_masks(tok.to(DEV), TABLE.to(DEV), keys.to(DEV), p)[0]
    assert m.sum(1).tolist() == want


# ---- blocks ----------------------------------------------------------------------------------------------------------------------
def blocks_case(frames, cen, keys, p, length=5, adjust=0.1):
    B, Tmax = keys.shape
    want = [MR.blocks(t, cen[b].tolist(), keys[b].tolist(), p, length, adjust) for b, t in enumerate(frames)]
    width = max(len(MR.preserve(w[0])) for w in want)
    rows = [[t] + list(MR.block_counts(t, p, length, adjust)) for t in frames]
    dc, dk = cen.to(DEV), keys.to(DEV)
    m, ids = twice(lambda out: hip.mask_blocks(rows, dc, dk, length, width, out=out), [((B, Tmax + 1), torch.bool), ((B, width), torch.int64)])
    wm, wi = MR.pack([w[0] for w in want], Tmax + 1)
    assert torch.equal(m, wm) and torch.equal(ids, wi)
    assert m.sum(1).tolist() == [int(t * p) for t in frames]
    got = ops.block_masks(frames, dc, dk, p, length, adjust)
    cpu = ops.block_masks(frames, cen, keys, p, length, adjust)
    assert all(torch.equal(a.cpu(), b) and torch.equal(b, c) for a, b, c in zip(got, (m, ids), cpu))
    return want


@pytest.mark.parametrize("p", [0.55, 0.45])
def test_blocks_equal_restatement(p):
    g = torch.Generator().manual_seed(int(p * 100))
    frames = BLOCK_T + [50, 50, 50, 50]
    cen, keys = block_inputs(g, frames, p)
    cen[8] = 0                                                # every centre at 0: clamping, duplicates, far under the target
    cen[9] = 49                                               # ... at T - 1
    cen[10, :6] = torch.tensor([2, 7, 12, 17, 22, 27])        # disjoint spans: 30 (25) frames, over both targets
    K, target = MR.block_counts(50, p, 5, 0.1)                # K - 1 disjoint spans from frame 0 on, the last overlapping: n == target
    r = target - 5 * (K - 1)
    assert 1 <= r <= 5
    cen[11, :K - 1] = 2 + 5 * torch.arange(K - 1, dtype=torch.int32)
    cen[11, K - 1] = 5 * (K - 1) + r - 3
    want = blocks_case(frames, cen, keys, p)
    assert {w[1] for w in want} == {"over", "under", "equal"} and want[11][1] == "equal" and want[10][1] == "over" and want[8][1] == "under"


def test_blocks_kept_counts_cross_the_wave_and_workgroup_sizes():
    p, frames = 0.55, []
    for kept in (63, 64, 65, 255, 256, 257):
        frames += [T for T in range(1, 700) if T + 1 - int(T * p) == kept][:1]
    assert len(frames) == 6
    cen, keys = block_inputs(torch.Generator().manual_seed(3), frames, p)
    want = blocks_case(frames, cen, keys, p)
    assert [len(MR.preserve(w[0])) for w in want] == [63, 64, 65, 255, 256, 257]


def test_blocks_at_the_row_limit_and_other_lengths():
    g = torch.Generator().manual_seed(8)
    frames = [4096, 4095, 33]
    for length in (1, 4, 10):
        cen, keys = block_inputs(g, frames, 0.5, length, 0.05)
        blocks_case(frames, cen, keys, 0.5, length, 0.05)
    with pytest.raises(ValueError):
        ops.block_masks([4097], torch.zeros(1, 8, dtype=torch.int32, device=DEV), torch.zeros(1, 4097, dtype=torch.int32, device=DEV), 0.5, 5)


# ---- the reference's recorded cases, bad arguments, the generators -------------------------------------------------------------------
def test_fixture_through_the_device_route():
    run_fixture(torch.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pretrain_masks.pt"), weights_only=False), DEV)


def test_bad_arguments_are_einval_and_launch_nothing():
    L = hip.lib()
    B, N = 2, 16
    keys = torch.zeros(B, N, dtype=torch.int32, device=DEV)
    tok = torch.full((B, N), 5, dtype=torch.int64, device=DEV)
    tab = TABLE.to(DEV)
    mask, ids, counts = Guarded((B, N + 1), torch.bool), Guarded((B, N + 1), torch.int64), Guarded((2, B), torch.int32)
    for g in (mask, ids, counts):
        g.raw[GUARD:GUARD + g.n] = 0xAB
    rows = (ctypes.c_int * 6)(16, 2, 8, 16, 2, 8)
    rows_bad = (ctypes.c_int * 6)(16, 2, 8, 17, 2, 8)
    drows = torch.tensor([16, 2, 8, 16, 2, 8], dtype=torch.int32, device=DEV)
    P, s = hip.ptr, hip.stream()
    calls = {
        "op_mask_patches": [
            lambda: L.op_mask_patches(P(keys), P(keys), B, 4097, 5, 1, P(mask.t), P(ids.t), P(mask.t), P(ids.t), s),     # N over the limit
            lambda: L.op_mask_patches(P(keys), P(keys), B, N, 17, 1, P(mask.t), P(ids.t), P(mask.t), P(ids.t), s),       # m1 > N
            lambda: L.op_mask_patches(P(keys), P(keys), B, N, 12, 13, P(mask.t), P(ids.t), P(mask.t), P(ids.t), s),      # extra > m1
            lambda: L.op_mask_patches(P(keys), P(keys), B, N, 12, -1, P(mask.t), P(ids.t), P(mask.t), P(ids.t), s),      # extra < 0
            lambda: L.op_mask_patches(None, None, B, N, 12, 0, P(mask.t), P(ids.t), None, None, s),                      # null keys
        ],
        "op_mask_words": [
            lambda: L.op_mask_words(P(tok), N, B, 4097, 1, P(tab), tab.numel(), P(keys), None, 0.15, 0.0, P(mask.t), P(ids.t), N + 1, None, None, 0,
                                    P(counts.t), s),                                                                      # L over the limit
            lambda: L.op_mask_words(P(tok), N - 1, B, N, 1, P(tab), tab.numel(), P(keys), None, 0.15, 0.0, P(mask.t), P(ids.t), N + 1, None, None, 0,
                                    P(counts.t), s),                                                                      # ld < L
            lambda: L.op_mask_words(P(tok), N, B, N, 1, P(tab), tab.numel(), P(keys), None, 1.5, 0.0, P(mask.t), P(ids.t), N + 1, None, None, 0,
                                    P(counts.t), s),                                                                      # p > 1
            lambda: L.op_mask_words(P(tok), N, B, N, 1, P(tab), tab.numel(), P(keys), None, 0.15, 0.0, P(mask.t), P(ids.t), N + 2, None, None, 0,
                                    P(counts.t), s),                                                                      # width > L + 1
            lambda: L.op_mask_words(P(tok), N, B, N, 1, P(tab), tab.numel(), P(keys), P(keys), 0.15, 0.4, P(mask.t), P(ids.t), N + 1, None, None, 0,
                                    P(counts.t), s),                                                                      # keys_b without outputs
        ],
        "op_mask_blocks": [
            lambda: L.op_mask_blocks(P(drows), rows, P(keys), 2, P(keys), 4097, B, 5, P(mask.t), P(ids.t), N + 1, s),    # Tmax over the limit
            lambda: L.op_mask_blocks(P(drows), rows_bad, P(keys), 2, P(keys), N, B, 5, P(mask.t), P(ids.t), N + 1, s),   # T > Tmax
            lambda: L.op_mask_blocks(P(drows), rows, P(keys), 1, P(keys), N, B, 5, P(mask.t), P(ids.t), N + 1, s),       # K > Kmax
            lambda: L.op_mask_blocks(P(drows), rows, P(keys), 2, P(keys), N, B, 0, P(mask.t), P(ids.t), N + 1, s),       # length 0
            lambda: L.op_mask_blocks(P(drows), rows, P(keys), 2, P(keys), N, B, 5, P(mask.t), P(ids.t), 8, s),           # width < kept
            lambda: L.op_mask_blocks(P(drows), None, P(keys), 2, P(keys), N, B, 5, P(mask.t), P(ids.t), N + 1, s),       # no host table
        ],
    }
    for name, fns in calls.items():
        for i, fn in enumerate(fns):
            assert fn() == -22, (name, i)
            assert name in L.op_last_error().decode(), (name, i, L.op_last_error())
    torch.cuda.synchronize()
    for g in (mask, ids, counts):
        assert g.intact() and bool((g.raw[GUARD:GUARD + g.n] == 0xAB).all())
    with pytest.raises(ValueError, match="op_mask_blocks"):   # the wrapper turns the entry's EINVAL into a ValueError with its text
        hip.mask_blocks([[16, 2, 8], [17, 2, 8]], keys[:, :2].contiguous(), keys, 5)


def test_generators_feed_the_pretraining_criteria(golden_dir):
    """A batch from each generator goes through the pretraining criterion of the micro model: the loss is finite, and the ids satisfy the
    gather's contract (every id < S or == -1).  The CPU route of the generators gives the device route's bits for the same keys."""
    from one_peace_amd.criterions.pretrain import AudioTextPretrainLossCriterion, ImageTextPretrainLossCriterion
    from tests.test_model_cpu import _build_pretrain
    table = torch.ones(1000, dtype=torch.uint8)
    table[4::3] = 0
    for stage in ("vl", "al"):
        fx = torch.load(os.path.join(golden_dir, "micro_pretrain.pt" if stage == "vl" else "micro_pretrain_al.pt"), weights_only=False)
        base = {k: v for k, v in fx["net_input"].items() if not k.endswith(("_preserve_ids", "_mask_indices"))}
        ni = {k: (v.to(DEV).to(torch.bfloat16) if v.is_floating_point() else v.to(DEV)) for k, v in base.items()}
        gen = ImageTextPretrainMasks(table, patch_image_size=64) if stage == "vl" else AudioTextPretrainMasks(table)
        g = torch.Generator(device=DEV).manual_seed(11)
        batch = gen(ni, generator=g)
        added = sorted(k for k in batch if k not in ni)
        assert len(added) == (8 if stage == "vl" else 6) and all(batch[k].device.type == "cuda" for k in added)
        again = gen(ni, generator=torch.Generator(device=DEV).manual_seed(11))
        assert all(torch.equal(batch[k], again[k]) for k in added)
        for k in added:
            if k.endswith("_preserve_ids"):
                S = batch[k.replace("_preserve_ids", "_mask_indices")].shape[1]
                ids = batch[k]
                assert ids.dtype == torch.int64 and bool(((ids == -1) | ((ids >= 0) & (ids < S))).all()) and bool((ids[:, 0] == 0).all())
        if stage == "vl":
            keys = gen.draw_keys(4, 15, DEV, torch.Generator(device=DEV).manual_seed(11))
            cpu = gen.apply(base, {k: v.cpu() for k, v in keys.items()})
        else:
            frames, Tmax = gen.frames_of(ni)
            keys = gen.draw_keys(4, 15, frames, Tmax, DEV, torch.Generator(device=DEV).manual_seed(11))
            cpu = gen.apply(base, {k: v.cpu() for k, v in keys.items()}, frames)
        assert all(torch.equal(batch[k].cpu(), cpu[k]) for k in added)
        m = _build_pretrain(fx, audio_language=stage == "al").to(DEV).to(torch.bfloat16).eval()
        crit = (ImageTextPretrainLossCriterion(None, 0.5, 1.0, 0.5, 0.5, 2.5, label_smoothing=0.0) if stage == "vl"
                else AudioTextPretrainLossCriterion(None, 1.0, 0.5, 0.5, 2.5, label_smoothing=0.0))
        loss, _, _ = crit(m, {"net_input": batch, "nsentences": 4})
        assert math.isfinite(float(loss.detach()))
