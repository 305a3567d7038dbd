"""Pretraining masks (one_peace_amd/pretrain_masks.py, ops.patch_masks / word_masks / block_masks) on the CPU route.

tests/golden/pretrain_masks.pt holds what the UNMODIFIED reference made (make_pretrain_masks_golden.py), with its recorded random
choices re-expressed as keys and centres; tests/masks_ref.py restates the rules loop by loop.  Every comparison is between integers
and exact."""
import math
import os

import pytest
import torch

from one_peace_amd import ops
from one_peace_amd.pretrain_masks import AudioTextPretrainMasks, ImageTextPretrainMasks, whole_word_table
from tests import masks_ref as MR

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pretrain_masks.pt")


@pytest.fixture(scope="module")
def golden():
    return torch.load(GOLDEN, weights_only=False)


def pad_rows(rows, fill, width=None, dtype=torch.int32):
    width = max(len(r) for r in rows) if width is None else width
    out = torch.full((len(rows), width), fill, dtype=dtype)
    for i, r in enumerate(rows):
        out[i, :len(r)] = torch.as_tensor(r, dtype=dtype)
    return out


# ---- restatement == the reference's recorded outputs -------------------------------------------------------------------------------
def test_restatement_equals_reference_image_text(golden):
    table = golden["table"].tolist()
    for case in golden["image_text"]:
        tr, ir, vtr, vir = case["ratios"]
        N = (case["patch_image_size"] // 16) ** 2
        m1 = int(N * ir)
        extra = int(N * vir) - (N - m1)
        per = {k: [] for k in ("text", "vl_text", "image", "vl_image")}
        for ex, keys in zip(case["samples"], case["keys"]):
            row = ex["source_text"].tolist()
            m, vl, n = MR.words(row, table, keys["text_a"].tolist(), tr, keys["text_b"].tolist(), vtr, pad=golden["pad"])
            im, ivl = MR.patches(keys["image_a"].tolist(), keys["image_b"].tolist(), m1, extra)
            for name, got in (("text", m), ("vl_text", vl), ("image", im), ("vl_image", ivl)):
                assert got == ex[name + "_mask_indices"].tolist(), (case["patch_image_size"], name, row)
                assert MR.preserve(got) == ex[name + "_preserve_ids"].tolist()
                per[name].append(got)
        batch = case["batch"]
        for name, masks in per.items():
            mask, ids = MR.pack(masks, batch[name + "_mask_indices"].shape[1])
            assert torch.equal(mask, batch[name + "_mask_indices"]) and torch.equal(ids, batch[name + "_preserve_ids"]), name


def test_restatement_equals_reference_audio_text(golden):
    table, case = golden["table"].tolist(), golden["audio_text"]
    a = case["args"]
    per = {k: [] for k in ("al_text", "audio", "al_audio")}
    for ex, keys in zip(case["samples"], case["keys"]):
        m, _, _ = MR.words(ex["source_text"].tolist(), table, keys["text_a"].tolist(), a["al_text_mask_ratio"], pad=golden["pad"])
        got = {"al_text": m}
        for name, p in (("audio", a["audio_mask_ratio"]), ("al_audio", a["al_audio_mask_ratio"])):
            got[name], _ = MR.blocks(keys["frames"], keys[name + "_centers"].tolist(), keys[name + "_keys"].tolist(), p,
                                     a["audio_mask_length"], a["audio_mask_prob_adjust"])
        for name, g in got.items():
            assert g == ex[name + "_mask_indices"].tolist(), name
            assert MR.preserve(g) == ex[name + "_preserve_ids"].tolist()
            per[name].append(g)
    for name, masks in per.items():
        mask, ids = MR.pack(masks, case["batch"][name + "_mask_indices"].shape[1])
        assert torch.equal(mask, case["batch"][name + "_mask_indices"]) and torch.equal(ids, case["batch"][name + "_preserve_ids"]), name


def test_restatement_equals_reference_blocks(golden):
    seen = set()
    for c in golden["blocks"]:
        got, case = MR.blocks(c["T"], c["centers"].tolist(), c["keys"].tolist(), c["p"], c["length"], c["adjust"])
        assert got[1:] == c["mask"].tolist(), (c["T"], c["p"])
        seen.add(case)
    assert {c["T"] for c in golden["blocks"]} == {7, 49, 50, 249, 749} and {"over", "under"} <= seen


# ---- the CPU route of ops == restatement, on drawn keys ----------------------------------------------------------------------------
def rand_keys(g, *shape):
    return torch.randint(0, 2 ** 31 - 1, shape, dtype=torch.int32, generator=g)


@pytest.mark.parametrize("N,ratios", [(1, (1.0, 1.0)), (4, (0.75, 0.6875)), (49, (0.75, 0.6875)), (256, (0.75, 0.6875)),
                                      (16, (0.75, 0.25)), (16, (0.5, 1.0)), (16, (1.0, 0.3)), (784, (0.75, 0.6875))])
def test_patch_masks_equal_restatement_and_counts(N, ratios):
    g = torch.Generator().manual_seed(N)
    B = 5
    ka, kb = rand_keys(g, B, N), rand_keys(g, B, N)
    ka[1], kb[1] = 7, 7  # every key equal: the index decides
    ka[2, ::2], kb[2, 1::2] = 0, 2 ** 31 - 2
    m1 = int(N * ratios[0])
    m2 = int(N * ratios[1])
    extra = m2 - (N - m1)
    m, ids, vm, vids = ops.patch_masks(ka, kb, m1, extra)
    want = [MR.patches(ka[b].tolist(), kb[b].tolist(), m1, extra) for b in range(B)]
    for got, got_ids, w, width in ((m, ids, [x[0] for x in want], N + 1 - m1), (vm, vids, [x[1] for x in want], N + 1 - m2)):
        wm, wi = MR.pack(w, N + 1, width)
        assert torch.equal(got, wm) and torch.equal(got_ids, wi)
        assert got_ids.dtype == torch.int64 and got.dtype == torch.bool and tuple(got_ids.shape) == (B, width)
    assert m.sum(1).tolist() == [m1] * B and vm.sum(1).tolist() == [m2] * B           # exact counts
    assert not m[:, 0].any() and not vm[:, 0].any()                                   # CLS
    assert bool((vm | m)[:, 1:].all())                                                # nesting: visible in the image pass -> masked in the vl pass
    assert (ids >= 0).all() and (vids >= 0).all()                                     # full rows: no -1
    if m1:
        assert m[1, 1:1 + m1].all()                                                   # equal keys: the first m1 patches


def word_batch(g, table, rows_n, L, pad=1, eos=2):
    """A batch with the given caption lengths: random tokens from the table's range, eos, pads."""
    tok = torch.full((len(rows_n), L), pad, dtype=torch.int64)
    for b, n in enumerate(rows_n):
        if n >= 0:
            tok[b, :n] = torch.randint(4, table.numel(), (n,), generator=g)
            tok[b, n] = eos
    return tok


TABLE = torch.tensor([1, 1, 1, 1] + [1 if i % 3 else 0 for i in range(4, 60)], dtype=torch.uint8)


def check_words(tok, table, ka, p, kb, vl_ratio, got, width=None, pad=1):
    m, ids, vm, vids, overflow = got
    B, L = tok.shape
    want = [MR.words(tok[b].tolist(), table.tolist(), ka[b].tolist(), p, None if kb is None else kb[b].tolist(), vl_ratio, pad) for b in range(B)]
    widths = (width, width) if not isinstance(width, tuple) else width
    wm, wi = MR.pack([w[0] for w in want], L + 1, widths[0])
    assert torch.equal(m, wm) and torch.equal(ids, wi)
    over = width is not None and any(len(MR.preserve(w[0])) > widths[0] for w in want)
    if kb is not None:
        wm, wi = MR.pack([w[1] for w in want], L + 1, widths[1])
        assert torch.equal(vm, wm) and torch.equal(vids, wi)
        over = over or (width is not None and any(len(MR.preserve(w[1])) > widths[1] for w in want))
    else:
        assert vm is None and vids is None
    assert bool(overflow) == over
    return want


def test_word_masks_equal_restatement():
    g = torch.Generator().manual_seed(5)
    rows_n = list(range(0, 71)) + [-1, -1]  # captions of 0 ... 70 tokens and two all-pad rows
    L = 71
    tok = word_batch(g, TABLE, rows_n, L)
    tok[40, :40] = torch.tensor([5] + [6] * 39)          # ONE word of 40 tokens (W = 1) running to the caption's end
    tok[41, :3] = torch.tensor([6, 9, 5])                # the first tokens start no word
    tok[42, :42] = 6                                     # W = 0
    ka, kb = rand_keys(g, len(rows_n), L), rand_keys(g, len(rows_n), L)
    ka[10], kb[10] = 3, 3
    for p, vl in ((0.15, 0.4), (0.4, None), (1.0, 1.0), (0.0, 0.0)):
        got = ops.word_masks(tok, TABLE, ka, p, kb if vl is not None else None, vl)
        want = check_words(tok, TABLE, ka, p, kb if vl is not None else None, vl, got)
        m, vm = got[0], got[2]
        for b, n in enumerate(rows_n):
            n = max(n, 0)
            assert not m[b, 0] and not m[b, n + 1:].any()                     # CLS, eos and pads
            if vl is not None:
                assert not vm[b, 0] and not vm[b, n + 1:].any()
                unmasked = n - int(m[b].sum())
                k2 = int(n * vl)
                if k2 <= unmasked:                                           # exact count, drawn among the unmasked tokens only
                    assert int(vm[b].sum()) == k2 and not (vm[b] & m[b]).any()
                else:                                                        # the fallback: every unmasked token, then masked ones by index
                    assert int(vm[b].sum()) == k2 and int((vm[b] & ~m[b]).sum()) == unmasked
                    extra = (vm[b] & m[b]).nonzero().flatten().tolist()
                    assert extra == m[b].nonzero().flatten().tolist()[:len(extra)]
        assert not got[0][40].any() or got[0][40, 1:41].all()                # the one word is masked whole or not at all
        assert not got[0][42].any() and not got[0][0].any()                  # W = 0 and n = 0: nothing masked
        assert want[71][0] == [False] and got[1][71].tolist()[0] == 0 and (got[1][71][1:] == -1).all()   # an all-pad row keeps CLS only
    # p = 1 masks every word: a row whose first token starts no word keeps that prefix
    got = ops.word_masks(tok, TABLE, ka, 1.0)
    assert got[0][41, 1:4].tolist() == [False, False, True]


def test_word_masks_width_bound_and_overflow():
    g = torch.Generator().manual_seed(6)
    rows_n = [3, 20, 11, 0]
    L = 24
    tok = word_batch(g, TABLE, rows_n, L)
    ka, kb = rand_keys(g, 4, L), rand_keys(g, 4, L)
    free = ops.word_masks(tok, TABLE, ka, 0.15, kb, 0.4)
    w0, w1 = free[1].shape[1], free[3].shape[1]
    assert w0 == max((free[1] >= 0).sum(1)) and w1 == max((free[3] >= 0).sum(1))          # width=None: the batch maxima
    for width in (L + 1, (w0, w1), (w0 - 1, w1), (w0, w1 - 2), 4, 0):
        got = ops.word_masks(tok, TABLE, ka, 0.15, kb, 0.4, width=width)
        check_words(tok, TABLE, ka, 0.15, kb, 0.4, got, width=width)
    assert not bool(ops.word_masks(tok, TABLE, ka, 0.15, kb, 0.4, width=(w0, w1))[4])
    assert bool(ops.word_masks(tok, TABLE, ka, 0.15, kb, 0.4, width=(w0 - 1, w1))[4])


@pytest.mark.parametrize("p", [0.15, 0.4])
def test_float32_ceil_of_the_word_count(p):
    """k = ceil(float32(W) * p), the product rounded as torch rounds is_word_start.float().sum() * p, for every W in 1 ... 512: the
    restatement's formula and the CPU route's count (one-token words, so the masked tokens are the chosen starts)."""
    Ws = list(range(1, 513))
    want = [int(math.ceil(torch.ones(W, dtype=torch.uint8).float().sum() * p)) for W in Ws]
    assert [MR.words_k(W, p) for W in Ws] == want
    tok = torch.full((512, 513), 1, dtype=torch.int64)
    for W in Ws:
        tok[W - 1, :W], tok[W - 1, W] = 5, 2
    m = ops.word_masks(tok, TABLE, rand_keys(torch.Generator().manual_seed(1), 512, 513), p)[0]
    assert m.sum(1).tolist() == want


BLOCK_T = [1, 7, 49, 50, 749, 249, 0, 12]


def block_inputs(g, frames, p, length=5, adjust=0.1):
    B, Tmax = len(frames), max(frames)
    K = [MR.block_counts(t, p, length, adjust)[0] for t in frames]
    Kmax = max(K + [1])
    cen = torch.zeros(B, Kmax, dtype=torch.int32)
    for b, t in enumerate(frames):
        if t:
            cen[b] = torch.randint(0, t, (Kmax,), generator=g, dtype=torch.int32)
    return cen, rand_keys(g, B, Tmax)


@pytest.mark.parametrize("p", [0.55, 0.45])
def test_block_masks_equal_restatement_and_counts(p):
    g = torch.Generator().manual_seed(int(p * 100))
    frames = BLOCK_T + [50, 50, 50]
    cen, keys = block_inputs(g, frames, p)
    cen[8] = 0                                                # every centre at 0: clamping, duplicates, far under the target
    cen[9] = 49                                               # ... at T - 1
    cen[10, :6] = torch.tensor([2, 7, 12, 17, 22, 27])        # disjoint spans: 30 frames, over both targets
    m, ids = ops.block_masks(frames, cen, keys, p, 5, 0.1)
    want = [MR.blocks(t, cen[b].tolist(), keys[b].tolist(), p, 5, 0.1) for b, t in enumerate(frames)]
    wm, wi = MR.pack([w[0] for w in want], max(frames) + 1)
    assert torch.equal(m, wm) and torch.equal(ids, wi)
    assert {"over", "under"} <= {w[1] for w in want}
    assert m.sum(1).tolist() == [int(t * p) for t in frames]                                   # target_b, exactly
    assert ids.shape[1] == max(t + 1 - int(t * p) for t in frames)
    for b, t in enumerate(frames):
        assert not m[b, 0] and not m[b, t + 1:].any()
        assert (ids[b] >= 0).sum() == t + 1 - int(t * p)


def test_errors():
    g = torch.Generator().manual_seed(0)
    ka, kb = rand_keys(g, 2, 16), rand_keys(g, 2, 16)
    for m1, extra in ((12, -1), (12, 13), (17, 0)):
        with pytest.raises(ValueError):
            ops.patch_masks(ka, kb, m1, extra)
    with pytest.raises(ValueError):
        ops.patch_masks(ka.long(), kb, 12, 4)
    with pytest.raises(ValueError):
        ops.patch_masks(rand_keys(g, 1, 4097), rand_keys(g, 1, 4097), 5, 1)
    with pytest.raises(ValueError):
        ImageTextPretrainMasks(TABLE, image_mask_ratio=0.2, vl_image_mask_ratio=0.5)   # extra < 0
    with pytest.raises(ValueError):
        ImageTextPretrainMasks(TABLE, image_mask_ratio=0.75, vl_image_mask_ratio=1.5)  # extra > m1
    tok = word_batch(g, TABLE, [5, 3], 16)
    with pytest.raises(ValueError):
        ops.word_masks(tok, TABLE, ka, 1.5)
    with pytest.raises(ValueError):
        ops.word_masks(tok, TABLE, ka, 0.15, kb)  # keys_b without vl_ratio
    with pytest.raises(ValueError):
        ops.word_masks(tok, TABLE, ka, 0.15, width=18)
    with pytest.raises(ValueError):
        ops.word_masks(torch.ones(1, 4097, dtype=torch.int64), TABLE, rand_keys(g, 1, 4097), 0.15)
    cen = torch.zeros(2, 3, dtype=torch.int32)
    for kw in ({"non_overlapping": True}, {"expand_adjcent": True}, {"mask_dropout": 0.1}, {"inverse_mask": True}, {"require_same_masks": False}):
        with pytest.raises(NotImplementedError):
            ops.block_masks([16, 9], cen, ka, 0.55, 5, 0.1, **kw)
    with pytest.raises(ValueError):
        ops.block_masks([17, 9], cen, ka, 0.55, 5, 0.1)       # T > Tmax
    with pytest.raises(ValueError):
        ops.block_masks([16, 9], cen[:, :1], ka, 0.55, 5, 0.1)  # K = 2 centres needed, one given
    with pytest.raises(ValueError):
        ops.block_masks([16, 9], cen, ka, 0.55, 5, 0.1, width=5)  # narrower than a row's kept count
    with pytest.raises(ValueError):
        ops.block_masks([16], cen, ka, 0.55, 5, 0.1)


# ---- the two classes -------------------------------------------------------------------------------------------------------------
def test_image_text_class_equals_restatement():
    g = torch.Generator().manual_seed(9)
    tok = word_batch(g, TABLE, [12, 30, 1, 0, 22], 31)
    gen = ImageTextPretrainMasks(TABLE, patch_image_size=112)
    assert (gen.num_patches, gen.mask_patches, gen.vl_extra) == (49, 36, 20)
    net = {"src_tokens": tok, "src_images": torch.zeros(5, 1)}
    out = gen(net, generator=torch.Generator().manual_seed(3))
    keys = gen.draw_keys(5, 31, tok.device, torch.Generator().manual_seed(3))
    again = gen.apply(net, keys)
    names = ["%s_%s" % (a, b) for a in ("text", "image", "vl_text", "vl_image") for b in ("mask_indices", "preserve_ids")]
    assert sorted(out) == sorted(names + ["src_tokens", "src_images"]) and "text_mask_indices" not in net
    assert all(torch.equal(out[k], again[k]) for k in names)
    assert all(k.dtype == torch.int32 and int(k.min()) >= 0 for k in keys.values())
    check_words(tok, TABLE, keys["text_a"], 0.15, keys["text_b"], 0.4,
                (out["text_mask_indices"], out["text_preserve_ids"], out["vl_text_mask_indices"], out["vl_text_preserve_ids"], False))
    want = [MR.patches(keys["image_a"][b].tolist(), keys["image_b"][b].tolist(), 36, 20) for b in range(5)]
    for name, idx, width in (("image", 0, 14), ("vl_image", 1, 17)):
        wm, wi = MR.pack([w[idx] for w in want], 50, width)
        assert torch.equal(out[name + "_mask_indices"], wm) and torch.equal(out[name + "_preserve_ids"], wi)
    other = gen(net, generator=torch.Generator().manual_seed(4))
    assert not torch.equal(other["image_mask_indices"], out["image_mask_indices"])
    bounded = gen(net, generator=torch.Generator().manual_seed(3), width=32)
    assert bounded["text_preserve_ids"].shape[1] == 32 and torch.equal(bounded["text_mask_indices"], out["text_mask_indices"])
    w = out["text_preserve_ids"].shape[1]
    assert torch.equal(bounded["text_preserve_ids"][:, :w], out["text_preserve_ids"]) and (bounded["text_preserve_ids"][:, w:] == -1).all()


def test_audio_text_class_equals_restatement():
    g = torch.Generator().manual_seed(10)
    tok = word_batch(g, TABLE, [12, 30, 1, 7], 31)
    gen = AudioTextPretrainMasks(TABLE)
    assert gen.frame_count(16000) == 49 and gen.frame_count(240000) == 749
    frames = [49, 30, 7, 41]
    pad = torch.arange(50).expand(4, 50) > torch.tensor(frames).view(4, 1)
    net = {"src_tokens": tok, "audio_padding_masks": pad}
    out = gen(net, generator=torch.Generator().manual_seed(3))
    given = gen(net, frames=frames, generator=torch.Generator().manual_seed(3))
    names = ["%s_%s" % (a, b) for a in ("audio", "al_text", "al_audio") for b in ("mask_indices", "preserve_ids")]
    assert sorted(out) == sorted(names + list(net)) and all(torch.equal(out[k], given[k]) for k in names)
    keys = gen.draw_keys(4, 31, frames, 49, tok.device, torch.Generator().manual_seed(3))
    check_words(tok, TABLE, keys["text_a"], 0.4, None, None, (out["al_text_mask_indices"], out["al_text_preserve_ids"], None, None, False))
    for name, p in (("audio", 0.55), ("al_audio", 0.45)):
        cen = keys[name + "_centers"]
        assert all(0 <= c < t for b, t in enumerate(frames) for c in cen[b].tolist())
        want = [MR.blocks(t, cen[b].tolist(), keys[name + "_keys"][b].tolist(), p, 5, 0.1)[0] for b, t in enumerate(frames)]
        wm, wi = MR.pack(want, 50)
        assert torch.equal(out[name + "_mask_indices"], wm) and torch.equal(out[name + "_preserve_ids"], wi)
        assert not (out[name + "_mask_indices"] & pad).any()
    with pytest.raises(ValueError):
        gen({"src_tokens": tok})


def test_whole_word_table_mirrors_the_reference():
    class D:
        nspecial = 4
        symbols = ["<s>", "<pad>", "</s>", "<unk>", "12", "345", "madeupword0001", "zz", "7"]

        def __len__(self):
            return len(self.symbols)

        def __getitem__(self, i):
            return self.symbols[i]

    class Bpe:
        def is_beginning_of_word(self, tok):
            return int(tok) % 2 == 0  # raises ValueError for "zz"
    assert whole_word_table(D(), Bpe()).tolist() == [1, 1, 1, 1, 1, 0, 1, 1, 0]
    assert whole_word_table(D(), Bpe()).dtype == torch.uint8 and whole_word_table(D(), None) is None


def test_fixture_through_the_cpu_route(golden):
    run_fixture(golden, "cpu")


def run_fixture(golden, device):
    """The reference's recorded cases through ops on `device` (shared with the GPU tests)."""
    table = golden["table"].to(device)
    for case in golden["image_text"]:
        tr, ir, vtr, vir = case["ratios"]
        N = (case["patch_image_size"] // 16) ** 2
        m1 = int(N * ir)
        extra = int(N * vir) - (N - m1)
        batch = case["batch"]
        L = batch["src_tokens"].shape[1]
        ka = pad_rows([k["text_a"] for k in case["keys"]], 0, L).to(device)
        kb = pad_rows([k["text_b"] for k in case["keys"]], 0, L).to(device)
        got = ops.word_masks(batch["src_tokens"].to(device), table, ka, tr, kb, vtr, pad=golden["pad"])
        for name, t in zip(("text_mask_indices", "text_preserve_ids", "vl_text_mask_indices", "vl_text_preserve_ids"), got):
            assert torch.equal(t.cpu(), batch[name]), name
        pa = torch.stack([k["image_a"] for k in case["keys"]]).to(device)
        pb = torch.stack([k["image_b"] for k in case["keys"]]).to(device)
        got = ops.patch_masks(pa, pb, m1, extra)
        for name, t in zip(("image_mask_indices", "image_preserve_ids", "vl_image_mask_indices", "vl_image_preserve_ids"), got):
            assert torch.equal(t.cpu(), batch[name]), name
    case = golden["audio_text"]
    a, batch = case["args"], case["batch"]
    L = batch["src_tokens"].shape[1]
    ka = pad_rows([k["text_a"] for k in case["keys"]], 0, L).to(device)
    got = ops.word_masks(batch["src_tokens"].to(device), table, ka, a["al_text_mask_ratio"], pad=golden["pad"])
    assert torch.equal(got[0].cpu(), batch["al_text_mask_indices"]) and torch.equal(got[1].cpu(), batch["al_text_preserve_ids"])
    frames = [k["frames"] for k in case["keys"]]
    for name, p in (("audio", a["audio_mask_ratio"]), ("al_audio", a["al_audio_mask_ratio"])):
        cen = pad_rows([k[name + "_centers"] for k in case["keys"]], 0).to(device)
        keys = torch.stack([k[name + "_keys"] for k in case["keys"]]).to(device)
        m, ids = ops.block_masks(frames, cen, keys, p, a["audio_mask_length"], a["audio_mask_prob_adjust"])
        assert torch.equal(m.cpu(), batch[name + "_mask_indices"]) and torch.equal(ids.cpu(), batch[name + "_preserve_ids"]), name
    for p in (0.55, 0.45):  # compute_block_mask_1d's own cases, as ONE mixed-length batch per ratio
        cs = [c for c in golden["blocks"] if c["p"] == p]
        frames = [c["T"] for c in cs]
        cen = pad_rows([c["centers"] for c in cs], 0, max(max(c["centers"].numel() for c in cs), 1)).to(device)
        keys = pad_rows([c["keys"] for c in cs], 0).to(device)
        m, _ = ops.block_masks(frames, cen, keys, p, 5, 0.1)
        for b, c in enumerate(cs):
            assert m[b, 1:c["T"] + 1].cpu().tolist() == c["mask"].tolist() and not m[b, 0] and not m[b, c["T"] + 1:].any()
