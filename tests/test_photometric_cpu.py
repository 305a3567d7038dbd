"""Photometric train transforms on the CPU: the numpy restatement tests/photometric_ref.py (the arithmetic of csrc/photometric.hip) and
the host-side tables of imageprep against PIL itself, bit for bit; the CPU route of ops.preprocess_images(jitter=, blur=, flips=)
against the hand-written PIL chain; the draws of augment.ColorJitter / GaussianBlur; GroundingTransform's box arithmetic."""
import itertools
import math

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageFilter

from one_peace_amd import augment, imageprep, ops
from tests import photometric_ref as ref

ENHANCERS = {ref.OP_BRIGHTNESS: ImageEnhance.Brightness, ref.OP_CONTRAST: ImageEnhance.Contrast, ref.OP_SATURATION: ImageEnhance.Color}


def make_image(h, w, seed, kind="random"):
    """uint8 [h, w, 3]: random bytes; 'regions' adds saturated (0 and 255) and constant regions."""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "regions":
        a[: h // 3] = 255
        a[h // 3: h // 2, : w // 2] = 0
        a[h // 2:, w // 2:] = (200, 17, 90)
    return a


def pil_chain(a, chain):
    im = Image.fromarray(a)
    for op, f in chain:
        if op:
            im = ENHANCERS[op](im).enhance(f)
    return im


def pil_blur(a, radius):
    return np.asarray(Image.fromarray(a).filter(ImageFilter.GaussianBlur(radius=radius)))


FACTORS = (0.0, 1.0, 0.25, 0.6180339887, 1.4, 2.75)


# ---- ColorJitter -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", sorted(ENHANCERS))
def test_each_enhancer_equals_pil(op):
    rng = np.random.default_rng(op)
    for i, (h, w) in enumerate([(1, 1), (3, 7), (16, 16), (39, 21), (24, 31)]):
        for kind in ("random", "regions"):
            a = make_image(h, w, 10 * op + i, kind)
            for f in FACTORS + (float(rng.uniform(0.6, 1.4)),):
                want = np.asarray(ENHANCERS[op](Image.fromarray(a)).enhance(f))
                assert np.array_equal(ref.enhance(a, op, f), want), (op, h, w, kind, f)


def test_contrast_mean_in_integers_is_pil_rounded_mean():
    from PIL import ImageStat
    for seed in range(20):
        a = make_image(1 + seed, 2 + 3 * seed, seed)
        want = int(ImageStat.Stat(Image.fromarray(a).convert("L")).mean[0] + 0.5)
        assert ref.contrast_mean(a) == want
    assert ref.contrast_mean(np.full((2, 1, 3), 255, np.uint8)) == 255
    half = np.zeros((1, 2, 3), np.uint8)
    half[0, 0] = 1  # L = (0 + 1) / 2: exactly k + 1/2 rounds up
    assert ref.contrast_mean(half) == 1 == int(ImageStat.Stat(Image.fromarray(half).convert("L")).mean[0] + 0.5)


def test_chains_of_three_ops_in_all_six_orders_equal_pil():
    rng = np.random.default_rng(7)
    for n, order in enumerate(itertools.permutations(sorted(ENHANCERS))):
        for kind in ("random", "regions"):
            a = make_image(23, 35, n, kind)
            for fs in ((0.6, 1.4, 1.0), (1.4, 0.0, 0.7), tuple(rng.uniform(0.6, 1.4, 3).tolist())):
                want = np.asarray(pil_chain(a, zip(order, fs)))
                assert np.array_equal(ref.color_jitter(a, order, fs), want), (order, kind, fs)


def test_jitter_table():
    ops_t, f = imageprep.jitter_table([None, [("contrast", 0.5), ("brightness", 1.25)], [(3, 2.0)], ()])
    assert ops_t.dtype == np.int32 and f.dtype == np.float32 and ops_t.shape == f.shape == (4, 3)
    assert ops_t.tolist() == [[0, 0, 0], [2, 1, 0], [3, 0, 0], [0, 0, 0]]
    assert f.tolist() == [[1, 1, 1], [0.5, 1.25, 1], [2, 1, 1], [1, 1, 1]]
    for bad in ([[("hue", 1.0)]], [[(4, 1.0)]], [[(1, -0.1)]], [[(1, float("nan"))]], [[(1, float("inf"))]], [[(1, 1e39)]],
                [[(2, 1.0), (2, 1.0)]], [[(1, 1.0)] * 4]):
        with pytest.raises(ValueError):
            imageprep.jitter_table(bad)


# ---- GaussianBlur ----------------------------------------------------------------------------------------------
def test_gaussian_box_params_and_blur_equal_pil():
    rng = np.random.default_rng(3)
    assert imageprep.gaussian_box_params(0.1)[0] == 0 and imageprep.gaussian_box_params(2.0)[0] == 1
    assert imageprep.gaussian_box_params(33.0)[0] == 32 == imageprep.MAX_BOX_RADIUS
    small = [0.1, 2.0] + rng.uniform(0.1, 2.0, 10).tolist()
    large = [2.5, 33.0] + rng.uniform(2.0, 33.0, 6).tolist()
    for n, r in enumerate(small + large):
        assert imageprep.gaussian_box_params(r) == ref.gaussian_box_params(r)
        R, ww, fw = imageprep.gaussian_box_params(r)
        assert 0 <= R <= 32 and 0 < ww < 1 << 32 and 0 <= fw < 1 << 32
        h, w = (int(v) for v in rng.integers(16, 201, 2))
        for a in (make_image(h, w, n), make_image(h, w, n, "regions"), np.full((h, w, 3), 255, np.uint8)):
            assert np.array_equal(ref.gaussian_blur(a, r), pil_blur(a, r)), (r, h, w)
    for r in small:  # tiny images: every window is clamped on both sides
        for h, w in ((1, 1), (2, 5), (7, 3)):
            a = make_image(h, w, 5)
            assert np.array_equal(ref.gaussian_blur(a, r), pil_blur(a, r)), (r, h, w)


def test_blur_table_and_bad_radii():
    R, ww, fw, on = imageprep.blur_table([None, 0.0, -1.0, 0.1, 2.0])
    assert on.tolist() == [0, 0, 0, 1, 1] and R.tolist() == [0, 0, 0, 0, 1]
    assert (int(R[4]), int(ww[4]), int(fw[4])) == imageprep.gaussian_box_params(2.0)
    assert (R.dtype, ww.dtype, fw.dtype, on.dtype) == (np.int32, np.uint32, np.uint32, np.uint8)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 40.0):
        with pytest.raises(ValueError):
            imageprep.gaussian_box_params(bad)
    with pytest.raises(ValueError):
        imageprep.blur_table([float("nan")])


# ---- order of the chain ----------------------------------------------------------------------------------------
def test_flip_last_equals_pils_compose_order():
    """The reference flips after the distortion and the blur (nlvr2_dataset.py:33-42).  Both commute with the flip, so the device may keep
    the flip in its store: PIL's order equals flip-first, and the restatement applied to the mirrored image equals the mirrored result."""
    a = make_image(32, 48, 11, "regions")
    chain = [(2, 1.3), (3, 0.7), (1, 1.2)]
    compose = np.asarray(pil_chain(a, chain).filter(ImageFilter.GaussianBlur(radius=1.7)).transpose(Image.FLIP_LEFT_RIGHT))
    flipped_first = np.asarray(pil_chain(np.ascontiguousarray(a[:, ::-1]), chain).filter(ImageFilter.GaussianBlur(radius=1.7)))
    assert np.array_equal(compose, flipped_first)
    mine = ref.gaussian_blur(ref.color_jitter(a, *zip(*chain)), 1.7)[:, ::-1]
    assert np.array_equal(mine, compose)


# ---- ops: the CPU routes ---------------------------------------------------------------------------------------
SIZES = [(37, 53), (200, 131), (64, 64), (19, 23), (90, 300)]


def _cases(S):
    imgs = [make_image(h, w, 20 + i, "regions" if i % 2 else "random") for i, (h, w) in enumerate(SIZES)]
    chains = [[(2, 1.3), (1, 0.8), (3, 1.1)], None, [(3, 0.0)], [(1, 1.0), (2, 1.4)], [(1, 1.4)]]
    radii = [0.1, 2.0, None, 1.234, 0.0]
    flips = [True, False, True, True, False]
    return imgs, chains, radii, flips


@pytest.mark.parametrize("S", [16, 48])
def test_cpu_route_of_preprocess_images_equals_the_pil_chain(S):
    imgs, chains, radii, flips = _cases(S)
    got = ops.preprocess_images(imgs, S, jitter=imageprep.jitter_table(chains), blur=radii, flips=flips)
    assert got.shape == (len(imgs), 3, S, S) and got.dtype == torch.float32
    for i, a in enumerate(imgs):
        im = Image.fromarray(a).resize((S, S), Image.BICUBIC)
        im = pil_chain(np.asarray(im), chains[i] or [])
        if radii[i]:
            im = im.filter(ImageFilter.GaussianBlur(radius=radii[i]))
        if flips[i]:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        want = imageprep.to_tensor_normalize(torch.from_numpy(np.array(im)))
        assert torch.equal(got[i], want), i
    only_blur = ops.preprocess_images(imgs, S, blur=radii)
    only_jitter = ops.preprocess_images(imgs, S, jitter=imageprep.jitter_table(chains))
    plain = ops.preprocess_images(imgs, S)
    assert torch.equal(only_blur[2], plain[2]) and torch.equal(only_jitter[1], plain[1])  # the untouched images
    assert not torch.equal(only_blur[1], plain[1]) and not torch.equal(only_jitter[0], plain[0])


def test_preprocess_images_without_the_new_arguments_is_unchanged():
    imgs, _, _, flips = _cases(32)
    for kw in ({}, {"flips": flips}, {"center_crop": True}, {"crops": [(1, 2, 10, 12)] * len(imgs), "flips": flips}):
        pack_kw = dict(kw)
        want = imageprep.to_tensor_normalize(imageprep.apply_packed(imageprep.pack_images(imgs, 32, pin=False, **pack_kw)))
        assert torch.equal(ops.preprocess_images(imgs, 32, **kw), want), kw
        assert torch.equal(ops.preprocess_images(imgs, 32, jitter=None, blur=None, **kw), want), kw


def test_cpu_routes_of_the_three_ops():
    S = 32
    u8 = torch.from_numpy(np.stack([make_image(S, S, 40 + i, "regions" if i == 1 else "random") for i in range(3)]))
    keep = u8.clone()
    ops_t, f = imageprep.jitter_table([[(2, 1.4), (3, 0.5)], None, [(1, 0.0)]])
    got = ops.color_jitter(u8, ops_t, f)
    assert got is u8
    assert np.array_equal(u8[0].numpy(), ref.color_jitter(keep[0].numpy(), ops_t[0], f[0]))
    assert torch.equal(u8[1], keep[1]) and not u8[2].any()
    u8 = keep.clone()
    ops.gaussian_blur(u8, [2.0, None, 0.5])
    assert np.array_equal(u8[0].numpy(), pil_blur(keep[0].numpy(), 2.0)) and torch.equal(u8[1], keep[1])
    assert np.array_equal(u8[2].numpy(), ref.gaussian_blur(keep[2].numpy(), 0.5))
    x = ops.normalize_images(keep, flips=[True, False, False])
    assert torch.equal(x[0], imageprep.to_tensor_normalize(keep[0].flip(1))) and torch.equal(x[1:], imageprep.to_tensor_normalize(keep[1:]))
    assert ops.normalize_images(keep, dtype=torch.bfloat16).dtype == torch.bfloat16


def test_value_errors():
    u8 = torch.zeros(2, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.color_jitter(u8, [[1, 0, 0]], [[1.0, 1.0, 1.0]])                      # one row for two images
    with pytest.raises(ValueError):
        ops.color_jitter(u8, [[5, 0, 0], [0, 0, 0]], np.ones((2, 3)))             # unknown op
    with pytest.raises(ValueError):
        ops.color_jitter(u8, [[1, 0, 0], [0, 0, 0]], [[-1.0, 1, 1], [1, 1, 1]])   # negative factor
    with pytest.raises(ValueError):
        ops.color_jitter(u8.float(), np.zeros((2, 3)), np.ones((2, 3)))           # not uint8
    with pytest.raises(ValueError):
        ops.gaussian_blur(u8, [1.0])
    with pytest.raises(ValueError):
        ops.gaussian_blur(u8, [1.0, 50.0])                                        # box radius above 32
    with pytest.raises(ValueError):
        ops.normalize_images(u8, flips=[True])
    with pytest.raises(ValueError):
        ops.preprocess_images([np.zeros((8, 8, 3), np.uint8)], 16, blur=[1.0, 2.0])
    with pytest.raises(ValueError):
        ops.preprocess_images([np.zeros((8, 8, 3), np.uint8)], 16, jitter=(np.zeros((2, 3)), np.ones((2, 3))))
    with pytest.raises(NotImplementedError):
        augment.ColorJitter(0.4, 0.4, 0.4, hue=0.1)
    with pytest.raises(ValueError):
        augment.ColorJitter(-0.1)
    with pytest.raises(ValueError):
        augment.ColorJitter(0.4, prob=1.5)
    with pytest.raises(ValueError):
        augment.GaussianBlur(p=2.0)
    with pytest.raises(ValueError):
        augment.GaussianBlur(radius_min=0.0)
    with pytest.raises(ValueError):
        augment.GaussianBlur(radius_max=60.0)
    with pytest.raises(ValueError):
        augment.GroundingTransform(50)


# ---- draws -----------------------------------------------------------------------------------------------------
def test_color_jitter_params_ranges_orders_and_probability():
    g = torch.Generator().manual_seed(0)
    cj = augment.ColorJitter(0.4, 0.4, 0.4, prob=0.5, generator=g)   # RandomDistortion(0.4, 0.4, 0.4, 0, 0.5)
    ops_t, f = cj.params(2000)
    assert ops_t.shape == f.shape == (2000, 3) and ops_t.dtype == np.int32 and f.dtype == np.float32
    applied = ops_t.any(axis=1)
    assert 0.45 < applied.mean() < 0.55                                # 0.5 +- 4.5 sigma of 2000 draws
    assert (np.sort(ops_t[applied], axis=1) == [1, 2, 3]).all()      # a permutation of the three ops (hue skipped)
    assert len({tuple(r) for r in ops_t[applied].tolist()}) == 6      # every order occurs
    fa = f[applied]
    assert fa.min() >= np.float32(0.6) and fa.max() <= np.float32(1.4) and fa.min() < 0.62 and fa.max() > 1.38
    assert (f[~applied] == 1).all()
    again = augment.ColorJitter(0.4, 0.4, 0.4, prob=0.5, generator=torch.Generator().manual_seed(0)).params(2000)
    assert np.array_equal(again[0], ops_t) and np.array_equal(again[1], f)
    ops_t, f = augment.ColorJitter(brightness=1.5, saturation=(0.5, 0.5), generator=g).params(300)   # contrast 0: skipped; prob 1
    assert (np.sort(ops_t, axis=1) == [0, 1, 3]).all() and (ops_t[:, 2] == 0).all()
    assert f[ops_t == 1].min() >= 0 and f[ops_t == 1].max() <= 2.5 and f[ops_t == 1].min() < 0.1 and (f[ops_t == 3] == 0.5).all()
    assert not augment.ColorJitter(generator=g).params(5)[0].any()


def test_gaussian_blur_params_range_and_probability():
    g = torch.Generator().manual_seed(1)
    radii = augment.GaussianBlur(generator=g).params(2000)
    drawn = [r for r in radii if r is not None]
    assert 0.45 < len(drawn) / 2000 < 0.55
    assert 0.1 <= min(drawn) < 0.12 and 1.98 < max(drawn) <= 2.0
    assert radii == augment.GaussianBlur(generator=torch.Generator().manual_seed(1)).params(2000)
    assert all(r is not None for r in augment.GaussianBlur(p=1.0, generator=g).params(50))
    assert sum(r is not None for r in augment.GaussianBlur(p=0.0, generator=g).params(500)) <= 1   # u <= 0 only for u == 0


def test_train_image_transform_with_the_photometric_steps():
    imgs, _, _, _ = _cases(32)
    seeded = lambda: torch.Generator().manual_seed(5)
    g = seeded()
    t = augment.TrainImageTransform(32, hflip=0.5, generator=g, color_jitter=augment.ColorJitter(0.4, 0.4, 0.4, prob=0.5, generator=g),
                                    blur=augment.GaussianBlur(generator=g))
    got = t(imgs)
    g = seeded()
    _, flips = augment.TrainImageTransform(32, hflip=0.5, generator=g).params([a.shape[:2] for a in imgs])
    jitter = augment.ColorJitter(0.4, 0.4, 0.4, prob=0.5, generator=g).params(len(imgs))
    radii = augment.GaussianBlur(generator=g).params(len(imgs))
    assert torch.equal(got, ops.preprocess_images(imgs, 32, flips=flips, jitter=jitter, blur=radii))
    plain = augment.TrainImageTransform(32)
    assert plain.color_jitter is None and plain.blur is None and torch.equal(plain(imgs), ops.preprocess_images(imgs, 32))


# ---- RefCOCO ---------------------------------------------------------------------------------------------------
def test_grounding_resize_is_always_square():
    for size in (16, 224, 256, 384, 512):
        for w in (1, 7, size - 1, size, size + 1, 333, 640, 1000, 4000):
            for h in (1, 9, size - 1, size, size + 1, 480, 777, 2500):
                assert augment.GroundingTransform.resized_size(w, h, size, max_size=size) == (size, size), (w, h, size)
    assert augment.GroundingTransform.resized_size(640, 480, 256) == (256, 341)  # without max_size the aspect is kept


def test_grounding_transform_boxes_and_pixels():
    S = 32
    imgs = [make_image(40, 64, 1), make_image(97, 33, 2)]
    boxes = [torch.tensor([[3.0, 5.0, 50.5, 39.0]]), torch.tensor([[0.0, 0.0, 33.0, 97.0], [10.25, 20.5, 30.0, 90.0]])]
    gt = augment.GroundingTransform(S, blur=augment.GaussianBlur(p=1.0, generator=torch.Generator().manual_seed(2)))
    x, targets = gt(imgs, boxes)
    radii = augment.GaussianBlur(p=1.0, generator=torch.Generator().manual_seed(2)).params(2)
    assert torch.equal(x, ops.preprocess_images(imgs, S, blur=radii))
    for a, b, t in zip(imgs, boxes, targets):
        h, w = a.shape[:2]
        ratio_width, ratio_height = float(S) / float(w), float(S) / float(h)       # utils/transforms.py: resize, then Normalize
        want = b * torch.as_tensor([ratio_width, ratio_height, ratio_width, ratio_height])
        want = want / S
        assert t["boxes"].dtype == torch.float32 and torch.equal(t["boxes"], want)
        assert t["size"].tolist() == [S, S]
    assert torch.allclose(targets[1]["boxes"][0], torch.tensor([0.0, 0.0, 1.0, 1.0]), rtol=0, atol=2e-7)  # the whole image: the unit box
    x, _ = augment.GroundingTransform(S)(imgs, boxes)
    assert torch.equal(x, ops.preprocess_images(imgs, S))
    with pytest.raises(ValueError):
        gt(imgs, boxes[:1])
