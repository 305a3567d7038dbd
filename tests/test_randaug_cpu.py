"""RandAugment and RandomErasing on the CPU: the numpy restatement tests/randaug_ref.py (the arithmetic of csrc/randaugment.hip) against
Pillow itself, byte for byte; the host-side tables of imageprep; the draws of augment.RandAugment / RandomErasing; the CPU routes of
ops.rand_augment, ops.erase_images and ops.preprocess_images(randaug=) against the hand-written Pillow / torch statements; the composition
and the refusals of augment.create_transform.  Pillow is the reference throughout: timm is not a dependency of this project."""
import math

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageOps

from one_peace_amd import augment, imageprep, ops
from tests import randaug_ref as ref
from tests.test_photometric_cpu import make_image

FILL = (123, 117, 104)  # min(255, round(255 * CLIP mean))
KINDS = ("random", "regions", "constchan", "two", "const")


def special_image(S, seed, kind):
    """uint8 [S, S, 3]: make_image's 'random' / 'regions', or random with one constant channel, two-valued (0 / 255), constant."""
    if kind in ("random", "regions"):
        return make_image(S, S, seed, kind)
    rng = np.random.default_rng(seed)
    if kind == "constchan":
        a = rng.integers(0, 256, (S, S, 3), dtype=np.uint8)
        a[..., 1] = 77
        return a
    if kind == "two":
        return (rng.integers(0, 2, (S, S, 3)) * 255).astype(np.uint8)
    return np.broadcast_to(np.array([9, 200, 31], np.uint8), (S, S, 3)).copy()


def pil_named(a, item, fill=FILL):
    """uint8 array of one named RandAugment op on array `a`, by the Pillow calls timm's auto_augment.py makes."""
    im = Image.fromarray(a)
    name, v = item[0], (item[1] if len(item) > 1 else None)
    kw = dict(resample=Image.BICUBIC, fillcolor=fill)
    if name == "none":
        out = im
    elif name == "AutoContrast":
        out = ImageOps.autocontrast(im)
    elif name == "Equalize":
        out = ImageOps.equalize(im)
    elif name == "Invert":
        out = ImageOps.invert(im)
    elif name == "Posterize":
        out = im if v >= 8 else ImageOps.posterize(im, int(v))
    elif name == "Solarize":
        out = ImageOps.solarize(im, int(v))
    elif name == "SolarizeAdd":
        lut = [min(255, i + int(v)) if i < 128 else i for i in range(256)]
        out = im.point(lut + lut + lut)
    elif name in ("Color", "Contrast", "Brightness", "Sharpness"):
        out = getattr(ImageEnhance, name)(im).enhance(v)
    elif name == "Rotate":
        out = im.rotate(v, **kw)
    elif name == "ShearX":
        out = im.transform(im.size, Image.AFFINE, (1, v, 0, 0, 1, 0), **kw)
    elif name == "ShearY":
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, v, 1, 0), **kw)
    elif name == "TranslateX":
        out = im.transform(im.size, Image.AFFINE, (1, 0, v, 0, 1, 0), **kw)
    elif name == "TranslateY":
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, v), **kw)
    elif name == "Affine":
        out = im.transform(im.size, Image.AFFINE, tuple(v), **kw)
    else:
        raise ValueError(name)
    return np.asarray(out)


def geometric_items(S):
    """Both signs of shear, translate and rotate at the largest magnitude (10) and at 0."""
    t = 0.45 * S
    return [("ShearX", 0.3), ("ShearX", -0.3), ("ShearY", 0.3), ("ShearY", -0.3), ("TranslateX", t), ("TranslateX", -t), ("TranslateY", t),
            ("TranslateY", -t), ("Rotate", 30.0), ("Rotate", -30.0), ("ShearX", 0.0), ("ShearY", 0.0), ("TranslateX", 0.0),
            ("TranslateY", 0.0), ("Rotate", 0.0), ("Rotate", 11.7), ("ShearX", 0.137)]


POINT_ITEMS = [("Invert",), ("Posterize", 0), ("Posterize", 4), ("Solarize", 0), ("Solarize", 256), ("Solarize", 26), ("SolarizeAdd", 99),
               ("SolarizeAdd", 0)]
HIST_ITEMS = [("AutoContrast",), ("Equalize",)]
SHARP_ITEMS = [("Sharpness", 0.1), ("Sharpness", 1.0), ("Sharpness", 1.9)]
ENHANCE_ITEMS = [("Color", 0.1), ("Color", 1.9), ("Contrast", 0.1), ("Contrast", 1.9), ("Brightness", 0.1), ("Brightness", 1.9),
                 ("Color", 1.0)]


def ref_named(a, item, fill=FILL):
    """The same op through tests/randaug_ref.py, by the code and the fp64 row imageprep.randaug_table gives it."""
    tab_ops, tab_args = imageprep.randaug_table([[item]], a.shape[0])
    return ref.apply_op(a, tab_ops[0, 0], tab_args[0, 0], fill)


# ---- the reference against Pillow ------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [16, 48])
def test_reference_equals_pil_for_every_op_code(S):
    seen = set()
    for items in (POINT_ITEMS, HIST_ITEMS, SHARP_ITEMS, ENHANCE_ITEMS, geometric_items(S), [("none",)]):
        for n, item in enumerate(items):
            for k, kind in enumerate(KINDS):
                a = special_image(S, 1000 + 10 * n + k, kind)
                got, want = ref_named(a, item), pil_named(a, item)
                assert np.array_equal(got, want), (S, item, kind, int((got != want).sum()))
            seen.add(int(imageprep.randaug_table([[item]], S)[0][0, 0]))
    assert seen == set(range(12))  # every op code occurred (Rotate by 0 and ('none',) are code 0)


def test_equalize_takes_both_branches_at_256_pixels():
    """A 16 x 16 channel has 256 pixels: step = (256 - last bin) // 255 is 1 only when the last non-empty bin holds one pixel."""
    S, steps = 16, set()
    for seed in range(40):
        a = make_image(S, S, seed)
        for c in range(3):
            steps.add(ref.equalize_step(np.bincount(a[..., c].reshape(-1), minlength=256)))
        assert np.array_equal(ref.equalize(a), np.asarray(ImageOps.equalize(Image.fromarray(a)))), seed
    assert steps == {0, 1}
    for a in (special_image(S, 1, "const"), special_image(S, 2, "two"), special_image(48, 3, "two"), special_image(48, 4, "regions")):
        assert np.array_equal(ref.equalize(a), np.asarray(ImageOps.equalize(Image.fromarray(a))))
        assert np.array_equal(ref.autocontrast(a), np.asarray(ImageOps.autocontrast(Image.fromarray(a))))


def test_affine_truncates_and_random_matrices_equal_pil():
    rng = np.random.default_rng(5)
    for n in range(12):
        S = (16, 48)[n % 2]
        a = special_image(S, n, KINDS[n % 2])
        co = tuple((np.array([1, 0, 0, 0, 1, 0]) + rng.normal(0, [0.2, 0.2, 4, 0.2, 0.2, 4])).tolist())
        assert np.array_equal(ref.affine(a, co, FILL), pil_named(a, ("Affine", co))), (n, co)
    a = special_image(48, 77, "random")  # rounding instead of truncating would be off on most pixels
    co = imageprep.affine_coeffs("Rotate", 30.0, 48)
    want = pil_named(a, ("Affine", co))
    assert np.array_equal(ref.affine(a, co, FILL), want)


# ---- tables ----------------------------------------------------------------------------------------------------
def test_rotate_matrix_equals_pil_for_20_angles():
    rng = np.random.default_rng(11)
    for n, angle in enumerate([30.0, -30.0, 0.001, 359.5, 45.0, 400.0, -725.25] + rng.uniform(-180, 180, 13).tolist()):
        S = (16, 48, 64)[n % 3]
        a = special_image(S, n, "random")
        co = imageprep.affine_coeffs("Rotate", angle, S)
        want = np.asarray(Image.fromarray(a).rotate(angle, resample=Image.BICUBIC, fillcolor=FILL))
        assert np.array_equal(pil_named(a, ("Affine", co)), want), angle
    for angle in (0, 360.0, -720):
        assert imageprep.affine_coeffs("Rotate", angle, 32) is None
    for angle in (90, 180.0, 270, -90, 450):
        with pytest.raises(ValueError):
            imageprep.affine_coeffs("Rotate", angle, 32)


def test_affine_coeffs_and_randaug_table():
    assert imageprep.affine_coeffs("ShearX", 0.25, 32) == (1, 0.25, 0, 0, 1, 0)
    assert imageprep.affine_coeffs("ShearY", -0.25, 32) == (1, 0, 0, -0.25, 1, 0)
    assert imageprep.affine_coeffs("TranslateX", 3.5, 32) == (1, 0, 3.5, 0, 1, 0)
    assert imageprep.affine_coeffs("TranslateY", -3.5, 32) == (1, 0, 0, 0, 1, -3.5)
    for bad in (("Shear", 0.1), ("ShearX", float("nan")), ("Rotate", float("inf"))):
        with pytest.raises(ValueError):
            imageprep.affine_coeffs(bad[0], bad[1], 32)
    tab_ops, tab_args = imageprep.randaug_table([[("ShearX", 0.21), ("Equalize",)], None, [("Posterize", 8)], [("Rotate", 360.0), ("Solarize", 256)],
                                                 [("Sharpness", 1.5)], [(5, 100)], [("Affine", (1, 0, 2, 0, 1, 3))]], 32)
    assert tab_ops.dtype == np.int32 and tab_args.dtype == np.float64 and tab_ops.shape == (7, 2) and tab_args.shape == (7, 2, 6)
    assert tab_ops.tolist() == [[11, 2], [0, 0], [0, 0], [0, 5], [10, 0], [5, 0], [11, 0]]
    assert tab_args[0, 0].tolist() == [1, 0.21, 0, 0, 1, 0] and not tab_args[0, 1].any() and tab_args[3, 1, 0] == 256
    assert tab_args[4, 0, 0] == 1.5 and tab_args[5, 0, 0] == 100 and tab_args[6, 0].tolist() == [1, 0, 2, 0, 1, 3]
    assert imageprep.randaug_table([])[0].shape == (0, 1)
    for bad in ([[("Hue", 1.0)]], [[(12,)]], [[(-1,)]], [[("Posterize", -1)]], [[("Posterize", 2.5)]], [[("Solarize", 257)]],
                [[("Solarize", float("nan"))]], [[("SolarizeAdd", 256)]], [[("Sharpness", -0.1)]], [[("Color", float("inf"))]],
                [[("Contrast", 1e39)]], [[("Affine", (1, 0, 0, 0, 1))]], [[("Affine", (1, 0, 0, 0, 1, float("nan")))]], [[("Rotate", 90)]],
                [[("Rotate", 180)]], [[("Equalize", 1.0)]], [[("Posterize",)]], [[()]]):
        with pytest.raises(ValueError):
            imageprep.randaug_table(bad, 32)
    with pytest.raises(ValueError):
        imageprep.randaug_table([[("ShearX", 0.1)]])  # no size


def test_check_randaug():
    tab = imageprep.randaug_table([[("ShearX", 0.21), ("Equalize",)], [("Color", 1.2), ("Posterize", 3)]], 32)
    o, a, f = imageprep.check_randaug((torch.from_numpy(tab[0]), tab[1].tolist(), [1, 2, 3]), 2)
    assert np.array_equal(o, tab[0]) and np.array_equal(a, tab[1]) and f == (1, 2, 3)
    o, a, f = imageprep.check_randaug((np.zeros((0, 2)), np.zeros((0, 2, 6)), FILL), 0)
    assert o.shape == (0, 2) and a.shape == (0, 2, 6)
    assert imageprep.check_randaug((np.array([3, 0]), np.zeros((2, 6)), FILL), 2)[0].shape == (2, 1)
    bad_args = tab[1].copy()
    bad_args[1, 1, 0] = 9.5
    for bad in ((tab[0], tab[1], FILL), 3), ((tab[0], tab[1][:, :1], FILL), 2), ((tab[0], tab[1], (1, 2)), 2), ((tab[0], tab[1], (1, 2, 256)), 2), \
            ((tab[0], tab[1], (1, 2, 2.5)), 2), ((tab[0], bad_args, FILL), 2), ((np.array([[12, 0], [0, 0]]), tab[1], FILL), 2), \
            ((np.array([[1.5, 0], [0, 0]]), tab[1], FILL), 2), ((tab[0], tab[1]), 2):
        with pytest.raises(ValueError):
            imageprep.check_randaug(*bad)


# ---- draws -----------------------------------------------------------------------------------------------------
def test_rand_augment_draws():
    size, n = 224, 4000
    ra = augment.RandAugment(magnitude=9, num_layers=2, mstd=0.5, prob=1.0, generator=torch.Generator().manual_seed(1))
    drawn = [item for layers in ra.draw(n // 2, size) for item in layers]
    assert len(drawn) == n and None not in drawn
    names = {"TranslateX": "TranslateXRel", "TranslateY": "TranslateYRel"}
    counts = {name: 0 for name in augment.RAND_INCREASING_OPS}
    signs = {name: [0, 0] for name in augment._SIGNED_OPS}
    for item in drawn:
        name = names.get(item[0], item[0])
        counts[name] += 1
        v = item[1] if len(item) > 1 else None
        if name == "Rotate":
            assert abs(v) <= 30.0
        elif name in ("ShearX", "ShearY"):
            assert abs(v) <= 0.3
        elif name in ("TranslateXRel", "TranslateYRel"):
            assert abs(v) <= 0.45 * size
        elif name in ("Color", "Contrast", "Brightness", "Sharpness"):
            assert 0.1 <= v <= 1.9
            v = v - 1.0
        elif name == "Posterize":
            assert v in (0, 1, 2, 3, 4)
        elif name == "Solarize":
            assert 0 <= v <= 256 and v == int(v)
        elif name == "SolarizeAdd":
            assert 0 <= v <= 110 and v == int(v)
        else:
            assert v is None
        if name in signs and v != 0:
            signs[name][v > 0] += 1
    p = 1.0 / 15
    sigma = math.sqrt(n * p * (1 - p))
    for name, c in counts.items():
        assert abs(c - n * p) <= 5 * sigma, (name, c)
    for name, (neg, pos) in signs.items():
        assert abs(pos - neg) <= 5 * math.sqrt(pos + neg) and min(pos, neg) > 0, (name, neg, pos)
    # the tables: shapes, fill, skipping, a fixed and a uniform magnitude
    tab_ops, tab_args, fill = ra.params(7, 48)
    assert tab_ops.shape == (7, 2) and tab_args.shape == (7, 2, 6) and fill == FILL
    assert ra.params(0, 48)[0].shape == (0, 2)
    none = augment.RandAugment(prob=0.0, generator=torch.Generator().manual_seed(2)).params(50, 48)
    assert not none[0].any()
    half = augment.RandAugment(prob=0.5, num_layers=1, generator=torch.Generator().manual_seed(3)).draw(2000, 48)
    kept = sum(la[0] is not None for la in half)
    assert abs(kept - 1000) <= 5 * math.sqrt(2000 * 0.25)
    fixed = augment.RandAugment(magnitude=10, mstd=0, prob=1.0, num_layers=1, generator=torch.Generator().manual_seed(4)).draw(300, 100)
    for (item,) in fixed:
        if item[0] == "Rotate":
            assert abs(item[1]) == 30.0
        if item[0] == "Solarize":
            assert item[1] == 0
        if item[0] == "Posterize":
            assert item[1] == 0
        if item[0] == "TranslateX":
            assert abs(item[1]) == 0.45 * 100
    uni = augment.RandAugment(magnitude=10, mstd=100, prob=1.0, num_layers=1, generator=torch.Generator().manual_seed(5)).draw(600, 100)
    angles = [abs(item[1]) for (item,) in uni if item[0] == "Rotate"]
    assert len(angles) > 10 and max(angles) <= 30.0 and min(angles) < 10.0 < max(angles)
    a = augment.RandAugment(generator=torch.Generator().manual_seed(9)).params(20, 64)
    b = augment.RandAugment(generator=torch.Generator().manual_seed(9)).params(20, 64)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def test_rand_augment_from_config():
    ra = augment.RandAugment.from_config("rand-m9-mstd0.5-inc1")
    assert (ra.magnitude, ra.num_layers, ra.mstd, ra.prob, ra.fill) == (9.0, 2, 0.5, 0.5, FILL)
    ra = augment.RandAugment.from_config("rand-m7-n3-mstd101-p0.25-inc1", mean=(0.5, 0.5, 1.0))
    assert (ra.magnitude, ra.num_layers, ra.mstd, ra.prob, ra.fill) == (7.0, 3, 101.0, 0.25, (128, 128, 255))
    for bad in ("rand-m9-w0", "rand-m9-mmax20", "rand-m9-inc0", "rand-m9"):
        if bad == "rand-m9":
            assert augment.RandAugment.from_config(bad).magnitude == 9.0
            continue
        with pytest.raises(NotImplementedError):
            augment.RandAugment.from_config(bad)
    with pytest.raises(NotImplementedError):
        augment.RandAugment(increasing=False)
    for bad in ("augmix-m3", "rand-x9", "rand-m", "rand-mstd", "original"):
        with pytest.raises(ValueError):
            augment.RandAugment.from_config(bad)
    for kw in ({"prob": 1.5}, {"num_layers": 0}, {"magnitude": -1}, {"mstd": -0.5}):
        with pytest.raises(ValueError):
            augment.RandAugment(**kw)


def test_random_erasing_params():
    H, W, B = 48, 64, 2000
    re_ = augment.RandomErasing(generator=torch.Generator().manual_seed(6))
    boxes = re_.params(B, H, W)
    assert boxes.shape == (B, 4) and boxes.dtype == np.int32
    erased = boxes[boxes[:, 2] > 0]
    assert abs(len(erased) - 0.25 * B) <= 5 * math.sqrt(B * 0.25 * 0.75)
    assert not boxes[boxes[:, 2] == 0].any()
    top, left, h, w = erased.T
    assert (top >= 0).all() and (left >= 0).all() and (top + h <= H).all() and (left + w <= W).all() and (h < H).all() and (w < W).all()
    # h = round(sqrt(t a)), w = round(sqrt(t / a)) with t / (H W) in [0.02, 1/3] and a in [0.3, 1 / 0.3]: each side within 1/2 of its real value
    t_lo, t_hi, a_lo, a_hi = 0.02 * H * W, H * W / 3.0, 0.3, 1 / 0.3
    assert (h >= math.sqrt(t_lo * a_lo) - 0.5).all() and (h <= math.sqrt(t_hi * a_hi) + 0.5).all()
    assert (w >= math.sqrt(t_lo / a_hi) - 0.5).all() and (w <= math.sqrt(t_hi / a_lo) + 0.5).all()
    hr, wr = np.stack([h - 0.5, h + 0.5]), np.stack([w - 0.5, w + 0.5])
    assert ((hr[1] * wr[1]) >= t_lo).all() and ((hr[0] * wr[0]) <= t_hi).all()          # the area the sides allow meets [t_lo, t_hi]
    assert ((hr[1] / wr[0]) >= a_lo).all() and ((hr[0] / wr[1]) <= a_hi).all()          # ... and the aspect [a_lo, a_hi]
    assert len({tuple(b) for b in erased.tolist()}) > len(erased) // 2
    assert (augment.RandomErasing(1.0, generator=torch.Generator().manual_seed(7)).params(50, 32, 32)[:, 2] > 0).all()
    assert not augment.RandomErasing(0.0).params(50, 32, 32).any()
    for kw in ({"probability": 1.1}, {"min_area": 0.0}, {"min_area": 0.5, "max_area": 0.4}, {"mode": "noise"}, {"min_aspect": 0.0}):
        with pytest.raises(ValueError):
            augment.RandomErasing(**kw)
    with pytest.raises(NotImplementedError):
        augment.RandomErasing(max_count=2)


# ---- CPU routes ------------------------------------------------------------------------------------------------
def test_rand_augment_cpu_route_equals_pil():
    S = 48
    layers = [[("ShearX", 0.21), ("Equalize",)], None, [("Contrast", 1.4), ("Rotate", -17.0)], [("Sharpness", 0.4), ("Solarize", 77)],
              [("Posterize", 8), ("Invert",)], [("none",), ("AutoContrast",)], [("TranslateY", -9.5), ("Brightness", 0.3)]]
    src = torch.from_numpy(np.stack([special_image(S, 40 + i, KINDS[i % 5]) for i in range(len(layers))]))
    tab = imageprep.randaug_table(layers, S)
    got = ops.rand_augment(src.clone(), *tab, FILL)
    for i, la in enumerate(layers):
        want = src[i].numpy()
        for item in la or []:
            want = pil_named(want, item)
        assert np.array_equal(got[i].numpy(), want), i
    assert torch.equal(got[1], src[1])
    with pytest.raises(ValueError):
        ops.rand_augment(src.clone(), tab[0][:3], tab[1][:3], FILL)
    with pytest.raises(ValueError):
        ops.rand_augment(src.float(), *tab, FILL)


def test_erase_images_cpu_route():
    B, H, W = 4, 20, 28
    boxes = [(0, 0, 5, 7), (0, 0, 0, 0), (15, 21, 5, 7), (3, 4, 1, 1)]
    noise = torch.randn(3 * (35 + 35 + 1), generator=torch.Generator().manual_seed(1))
    for dtype in (torch.float32, torch.bfloat16):
        x = torch.randn(B, 3, H, W, generator=torch.Generator().manual_seed(2)).to(dtype)
        want = x.clone()
        want[0, :, 0:5, 0:7] = noise[:105].view(3, 5, 7).to(dtype)
        want[2, :, 15:20, 21:28] = noise[105:210].view(3, 5, 7).to(dtype)
        want[3, :, 3:4, 4:5] = noise[210:].view(3, 1, 1).to(dtype)
        assert torch.equal(ref.erase(x, boxes, noise, [0, 105, 105, 210]), want)
        got = ops.erase_images(x, boxes, noise)
        assert got is x and torch.equal(got, want)
    x = torch.zeros(B, 3, H, W)
    for bad in ([(0, 0, 5, 7)] * 3, [(0, 0, 21, 7)] + boxes[1:], [(-1, 0, 5, 7)] + boxes[1:], [(0, 22, 5, 7)] + boxes[1:], [(0, 0, 5, 0)] + boxes[1:]):
        with pytest.raises(ValueError):
            ops.erase_images(x, bad, noise)
    with pytest.raises(ValueError):
        ops.erase_images(x, boxes, noise[:-1])
    assert torch.equal(ops.erase_images(x, [(0, 0, 0, 0)] * B, None), torch.zeros(B, 3, H, W))
    # RandomErasing: the three modes through the same store
    for mode in ("pixel", "rand", "const"):
        er = augment.RandomErasing(1.0, mode=mode, generator=torch.Generator().manual_seed(3))
        x = torch.full((3, 3, 32, 32), 7.0)
        y = er(x)
        changed = (y != 7.0)
        assert y is x and changed.any(dim=(1, 2, 3)).all() and not changed.all()
        for i in range(3):
            rows, cols = changed[i, 0].any(1).nonzero().view(-1), changed[i, 0].any(0).nonzero().view(-1)
            patch = y[i, :, rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1]
            if mode == "const":
                assert not patch.any()
            elif mode == "rand":
                assert (patch == patch[:, :1, :1]).all() and len(set(patch[:, 0, 0].tolist())) == 3
            else:
                assert patch.unique().numel() > patch.numel() // 2


def test_preprocess_images_with_randaug_cpu_route():
    S = 48
    imgs = [make_image(h, w, 600 + i, "regions" if i % 2 else "random") for i, (h, w) in enumerate([(37, 53), (200, 131), (64, 64), (19, 23), (90, 300)])]
    crops = [(3, 5, 30, 40), (10, 20, 150, 100), (0, 0, 64, 64), (1, 2, 17, 20), (5, 100, 80, 120)]
    flips = [True, False, True, True, False]
    layers = [[("ShearX", 0.21), ("Equalize",)], None, [("Contrast", 1.4), ("Rotate", -17.0)], [("Sharpness", 0.4), ("Solarize", 77)],
              [("TranslateX", 11.0), ("AutoContrast",)]]
    tab = imageprep.randaug_table(layers, S) + (FILL,)
    got = ops.preprocess_images(imgs, S, crops=crops, flips=flips, randaug=tab)
    for i, im in enumerate(imgs):
        top, left, h, w = crops[i]
        pil = Image.fromarray(im).crop((left, top, left + w, top + h)).resize((S, S), Image.BICUBIC)
        if flips[i]:
            pil = pil.transpose(Image.FLIP_LEFT_RIGHT)  # timm's order: the flip comes before RandAugment
        a = np.asarray(pil)
        for item in layers[i] or []:
            a = pil_named(a, item)
        assert torch.equal(got[i], imageprep.to_tensor_normalize(torch.from_numpy(a.copy()))), i
    # randaug=None: the bits of the call without the argument
    for kw in ({}, {"crops": crops, "flips": flips}, {"center_crop": True}, {"jitter": imageprep.jitter_table([[(2, 1.3)]] * 5), "flips": flips}):
        assert torch.equal(ops.preprocess_images(imgs, S, randaug=None, **kw), ops.preprocess_images(imgs, S, **kw))
    for kw in ({"jitter": imageprep.jitter_table([None] * 5)}, {"blur": [None] * 5}):
        with pytest.raises(ValueError):
            ops.preprocess_images(imgs, S, randaug=tab, **kw)
    with pytest.raises(ValueError):
        ops.preprocess_images(imgs[:4], S, randaug=tab)


def test_create_transform_composition_and_refusals():
    S = 32
    t = augment.create_transform(S, True, 0.4, "rand-m9-mstd0.5-inc1", "bicubic", re_prob=0.25, re_mode="pixel", re_count=1)
    tr, er = t.image_transform, t.erasing
    assert isinstance(tr, augment.TrainImageTransform) and tr.scale == (0.08, 1.0) and tr.hflip == 0.5 and not tr.center_crop
    assert isinstance(tr.rand_augment, augment.RandAugment) and tr.color_jitter is None and tr.blur is None  # auto_augment drops the jitter
    assert (tr.rand_augment.magnitude, tr.rand_augment.mstd, tr.rand_augment.num_layers, tr.rand_augment.fill) == (9.0, 0.5, 2, FILL)
    assert isinstance(er, augment.RandomErasing) and (er.probability, er.mode, er.count) == (0.25, "pixel", 1)
    assert (t.mean, t.std) == (imageprep.CLIP_MEAN, imageprep.CLIP_STD)
    t = augment.create_transform(S, True, 0.4)
    assert t.erasing is None and t.image_transform.rand_augment is None
    assert t.image_transform.color_jitter.ranges == augment.ColorJitter(0.4, 0.4, 0.4).ranges
    assert augment.create_transform(S, True, None).image_transform.color_jitter is None
    assert augment.create_transform(S, True, (0.1, 0.2, 0.3)).image_transform.color_jitter.ranges[2] == (0.8, 1.2)
    t = augment.create_transform((3, S, S), False, auto_augment="rand-m9", re_prob=0.25)
    assert t.image_transform.center_crop and t.image_transform.rand_augment is None and t.erasing is None and t.image_transform.hflip == 0.0
    imgs = [make_image(40 + 9 * i, 70 - 5 * i, i) for i in range(4)]
    assert torch.equal(t(imgs), ops.preprocess_images(imgs, S, center_crop=True))
    # the training transform: the same seeded generator gives the composition written out by hand
    make = lambda: augment.create_transform(S, True, 0.4, "rand-m9-mstd0.5-inc1", re_prob=0.5, re_mode="pixel", scale=(0.3, 1.0),
                                            generator=torch.Generator().manual_seed(12))
    got = make()(imgs, torch.float32, "cpu")
    hand = make()
    tr = hand.image_transform
    crops, flips = tr.params([im.shape[:2] for im in imgs])
    x = ops.preprocess_images(imgs, S, crops=crops, flips=flips, randaug=tr.rand_augment.params(4, S))
    boxes = hand.erasing.params(4, S, S)
    x = ops.erase_images(x, boxes, hand.erasing.noise(boxes, x.device))
    assert got.shape == (4, 3, S, S) and torch.equal(got, x)
    assert all(0.3 * h * w - 0.5 * (h + w) <= ch * cw for (h, w), (_, _, ch, cw) in zip([im.shape[:2] for im in imgs], crops))
    assert make()(imgs, torch.bfloat16).dtype == torch.bfloat16
    for kw in ({"interpolation": "bilinear"}, {"interpolation": "random"}, {"input_size": (3, 32, 48)}, {"color_jitter": (0.1, 0.2, 0.3, 0.4)},
               {"scale": (0.5, 1.5)}):
        with pytest.raises(ValueError):
            augment.create_transform(**{"input_size": S, **kw})
    for aa in ("augmix-m5-w4-d2", "original", "v0"):
        with pytest.raises(NotImplementedError):
            augment.create_transform(S, auto_augment=aa)
    with pytest.raises(NotImplementedError):
        augment.create_transform(S, auto_augment="rand-m9-w0")
    with pytest.raises(ValueError):
        augment.TrainImageTransform(S, rand_augment=augment.RandAugment(), color_jitter=augment.ColorJitter(0.4))
    # TrainImageTransform without the new arguments draws and computes what it did
    a = augment.TrainImageTransform(S, min_scale=0.9, hflip=0.5, generator=torch.Generator().manual_seed(3))(imgs)
    b = augment.TrainImageTransform(S, min_scale=(0.9, 1.0), hflip=0.5, generator=torch.Generator().manual_seed(3))(imgs)
    assert torch.equal(a, b)
