"""Training-time image augmentation on the CPU: the crop / centre-crop tables of imageprep.pack_images against PIL
(tests/golden/augment.pt, and PIL itself where it imports), the CPU route of ops.preprocess_images, RandomResizedCrop's box draw,
Mixup's parameter tables, ops.mix_targets and the torch route of ops.mix_images against timm's statements restated here."""
import os
import re

import numpy as np
import pytest
import torch

from one_peace_amd import augment, hip, imageprep, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def source_image(H, W, seed):  # = tests/golden/make_augment_golden.py: source_image
    return torch.randint(0, 256, (H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return torch.load(os.path.join(golden_dir, "augment.pt"), weights_only=False)


def two_pass(packed, i=0):
    """Image i of a packed batch: its tables evaluated with imageprep._pass in the kernels' two-pass order (written out here,
    independently of imageprep.apply_packed)."""
    S, buf = packed.size, packed.host.numpy()
    src_off, H, W, cx_off, kx, cy_off, ky, _, row0, rows, vfirst = (int(v) for v in packed.desc[i])
    coef = buf[packed.coef_off:packed.coef_off + 4 * packed.coef_count].view(np.int32)
    img = torch.from_numpy(buf[src_off:src_off + H * W * 3].reshape(H, W, 3).astype(np.int64))
    rx = coef[cx_off:cx_off + S * (4 + kx)].reshape(S, 4 + kx)
    ry = coef[cy_off:cy_off + S * (4 + ky)].reshape(S, 4 + ky)
    assert not rx[:, 2:4].any() and not ry[:, 2:4].any()
    cx, cy = (rx[:, 0], rx[:, 1], rx[:, 4:]), (ry[:, 0], ry[:, 1], ry[:, 4:])
    # every record stays inside the packed pixels, and the 16 readable bytes behind the last one are there
    assert (cx[0] >= 0).all() and (cx[0] + cx[1] <= W).all() and (cy[0] >= 0).all() and (cy[0] + cy[1] <= H).all()
    assert src_off % 16 == 0 and src_off + H * W * 3 + imageprep.SRC_SLACK <= packed.src_bytes
    assert max(np.abs(rx[:, 4:]).max(), np.abs(ry[:, 4:]).max()) < 1 << 23
    if vfirst:
        assert (row0, rows) == (0, S)
        out = imageprep._pass(imageprep._pass(img, cy, 0), cx, 1)
    else:
        assert row0 == int(cy[0][0]) and row0 + rows == int(cy[0][-1] + cy[1][-1]) <= H
        out = imageprep._pass(imageprep._pass(img[row0:row0 + rows], cx, 1), (cy[0] - row0, cy[1], cy[2]), 0)
    return out.to(torch.uint8), bool(vfirst)


# ---- geometry ---------------------------------------------------------------------------------------------------
def test_fixture_covers_the_shapes_and_boxes(fx):
    crops = fx["crops"].tolist()
    assert {(37, 53, 16), (200, 131, 32), (480, 640, 48), (19, 23, 32)} <= {tuple(r[:3]) for r in crops}
    for H, W, S in [(37, 53, 16), (200, 131, 32), (480, 640, 48), (19, 23, 32)]:
        boxes = [tuple(r[4:]) for r in crops if tuple(r[:3]) == (H, W, S)]
        assert (0, 0, 1, 1) in boxes and (H - 1, W - 1, 1, 1) in boxes and (0, 0, H, W) in boxes          # 1 x 1, the full image
        assert any(t + h == H and l + w == W and (h, w) != (H, W) and h > 1 for t, l, h, w in boxes)      # flush bottom-right
        assert any(h < S and w < S and h > 1 for t, l, h, w in boxes)                                     # upscaling
    vf = [r for r in crops if imageprep.vertical_first(r[6], r[7], r[2])]
    assert len(vf) >= 2 and any(r[4] + r[6] == r[0] and r[5] + r[7] == r[1] for r in vf)
    assert any(imageprep.vertical_first(H, W, int(S * H / W)) for H, W, S, _ in fx["centers"].tolist())
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "augment.pt")) < 1 << 20


def test_crop_tables_equal_pil_crop_resize(fx):
    seen_vfirst = 0
    for (H, W, S, seed, *box), want in zip(fx["crops"].tolist(), fx["crop_outputs"]):
        packed = imageprep.pack_images([source_image(H, W, seed)], S, pin=False, crops=[box])
        got, vfirst = two_pass(packed)
        assert vfirst == imageprep.vertical_first(box[2], box[3], S)  # decided from the BOX
        seen_vfirst += vfirst
        assert torch.equal(got, want), (H, W, S, box)
        assert torch.equal(imageprep.apply_packed(packed)[0], want)
    assert seen_vfirst >= 2


def test_center_crop_tables_equal_pil_resize_window(fx):
    for (H, W, S, seed), want in zip(fx["centers"].tolist(), fx["center_outputs"]):
        packed = imageprep.pack_images([source_image(H, W, seed)], S, pin=False, center_crop=True)
        got, vfirst = two_pass(packed)
        new_h, new_w, top, left = imageprep.center_crop_geometry(H, W, S)
        assert min(new_h, new_w) == S and max(new_h, new_w) == int(S * max(H, W) / min(H, W))
        assert (top, left) == (int(round((new_h - S) / 2.0)), int(round((new_w - S) / 2.0)))
        assert vfirst == (H > 100 * W and new_h < H)  # the whole image and the un-windowed target, as PIL sees them
        assert torch.equal(got, want), (H, W, S)
        assert torch.equal(imageprep.apply_packed(packed)[0], want)


def test_tables_equal_pil_itself_on_random_boxes():
    Image = pytest.importorskip("PIL.Image")
    g = torch.Generator().manual_seed(11)
    for H, W, S in [(37, 53, 16), (200, 131, 32), (480, 640, 48), (19, 23, 32)]:
        img = source_image(H, W, 5)
        pil = Image.fromarray(img.numpy())
        boxes = [imageprep.random_resized_crop_params(H, W, generator=g) for _ in range(8)]
        packed = imageprep.pack_images([img] * 8, S, pin=False, crops=boxes)
        for i, (t, l, h, w) in enumerate(boxes):
            want = np.array(pil.crop((l, t, l + w, t + h)).resize((S, S), Image.BICUBIC))
            assert np.array_equal(two_pass(packed, i)[0].numpy(), want), (H, W, S, boxes[i])
        new_h, new_w, top, left = imageprep.center_crop_geometry(H, W, S)
        want = np.array(pil.resize((new_w, new_h), Image.BICUBIC))[top:top + S, left:left + S]
        assert np.array_equal(two_pass(imageprep.pack_images([img], S, pin=False, center_crop=True))[0].numpy(), want)


def test_pack_images_without_the_new_keywords_is_unchanged_and_flags_are_staged():
    imgs = [source_image(30, 40, 1), source_image(7, 9, 2), source_image(50, 20, 3)]
    plain = imageprep.pack_images(imgs, 32, pin=False)
    assert plain.flip_off is None
    full = imageprep.pack_images(imgs, 32, pin=False, crops=[(0, 0, 30, 40), (0, 0, 7, 9), (0, 0, 50, 20)])
    assert np.array_equal(full.desc, plain.desc) and torch.equal(full.host, plain.host)  # the full-image box is the plain resize
    flagged = imageprep.pack_images(imgs, 32, pin=False, flips=[True, False, True])
    n = plain.host.numel()
    assert torch.equal(flagged.host[:n], plain.host) and flagged.flip_off >= n
    assert flagged.host[flagged.flip_off:flagged.flip_off + 3].tolist() == [1, 0, 1]
    assert torch.equal(imageprep.apply_packed(flagged)[0], imageprep.apply_packed(plain)[0].flip(1))
    assert torch.equal(imageprep.apply_packed(flagged)[1], imageprep.apply_packed(plain)[1])


def test_invalid_boxes_and_arguments_raise_before_any_copy():
    imgs = [source_image(30, 40, 1)]
    for box in [(0, 0, 0, 5), (0, 0, 5, 0), (-1, 0, 5, 5), (0, -1, 5, 5), (26, 0, 5, 5), (0, 36, 5, 5), (0, 0, 31, 40), (0, 0, 30, 41)]:
        with pytest.raises(ValueError, match="box"):
            imageprep.pack_images(imgs, 32, pin=False, crops=[box])
        for dev in ("cpu", "cuda:0"):  # the check comes before the device is touched
            with pytest.raises(ValueError, match="box"):
                ops.preprocess_images(imgs, 32, device=dev, crops=[box])
    with pytest.raises(ValueError, match="one .* per image"):
        imageprep.pack_images(imgs, 32, pin=False, crops=[(0, 0, 5, 5), (0, 0, 5, 5)])
    with pytest.raises(ValueError, match="flag per image"):
        imageprep.pack_images(imgs, 32, pin=False, flips=[True, False])
    with pytest.raises(ValueError, match="mutually exclusive"):
        imageprep.pack_images(imgs, 32, pin=False, crops=[(0, 0, 5, 5)], center_crop=True)
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.preprocess_images(imgs, 32, crops=[(0, 0, 5, 5)], center_crop=True)


def test_cpu_route_of_preprocess_images_equals_the_pil_statement(fx):
    Image = pytest.importorskip("PIL.Image")
    imgs = [source_image(37, 53, 1), source_image(200, 131, 2), source_image(19, 23, 3)]
    pils = [Image.fromarray(i.numpy()) for i in imgs]
    boxes, flips = [(1, 2, 7, 2), (0, 0, 200, 131), (12, 11, 7, 12)], [True, False, True]

    def statement(fn):
        u8 = [fn(p) for p in pils]
        u8 = [p.transpose(Image.FLIP_LEFT_RIGHT) if f else p for p, f in zip(u8, flips)]
        return imageprep.to_tensor_normalize(torch.stack([torch.from_numpy(np.array(p, dtype=np.uint8)) for p in u8]))

    it = iter(boxes)

    def crop(p):
        t, l, h, w = next(it)
        return p.crop((l, t, l + w, t + h)).resize((32, 32), Image.BICUBIC)

    got = ops.preprocess_images(imgs, 32, crops=boxes, flips=flips)
    assert got.dtype == torch.float32 and torch.equal(got, statement(crop))
    assert torch.equal(ops.preprocess_images(pils, 32, crops=boxes, flips=flips), got)  # PIL inputs

    def center(p):
        new_h, new_w, top, left = imageprep.center_crop_geometry(p.size[1], p.size[0], 32)
        return p.resize((new_w, new_h), Image.BICUBIC).crop((left, top, left + 32, top + 32))

    got = ops.preprocess_images(imgs, 32, center_crop=True, flips=flips)
    assert torch.equal(got, statement(center))
    # ... and the tables say the same
    packed = imageprep.pack_images(imgs, 32, pin=False, center_crop=True, flips=flips)
    assert torch.equal(got, imageprep.to_tensor_normalize(imageprep.apply_packed(packed)))
    plain = ops.preprocess_images(imgs, 32)  # today's arguments: unchanged
    assert torch.equal(plain, imageprep.to_tensor_normalize(torch.stack([imageprep.apply_coeffs(i, 32) for i in imgs])))


# ---- RandomResizedCrop's box ------------------------------------------------------------------------------------------
def test_random_resized_crop_params_is_deterministic_and_inside_the_image():
    draw = lambda seed, H, W: [imageprep.random_resized_crop_params(H, W, generator=torch.Generator().manual_seed(seed)) for _ in range(3)]
    assert draw(3, 480, 640) == draw(3, 480, 640) and draw(3, 480, 640) != draw(4, 480, 640)
    for H, W in [(1, 100), (100, 1), (7, 5), (480, 640)]:
        g = torch.Generator().manual_seed(H * 1000 + W)
        seen = set()
        for _ in range(1000):
            top, left, h, w = imageprep.random_resized_crop_params(H, W, generator=g)
            assert all(isinstance(v, int) for v in (top, left, h, w))
            assert 1 <= h <= H and 1 <= w <= W and 0 <= top <= H - h and 0 <= left <= W - w, (H, W, top, left, h, w)
            seen.add((top, left, h, w))
        assert len(seen) > 1 or (H, W) in [(1, 100), (100, 1)]
    assert "NOT checked" in imageprep.random_resized_crop_params.__doc__ and "torchvision" in imageprep.random_resized_crop_params.__doc__


def test_random_resized_crop_params_whole_image_and_central_fallback():
    g = torch.Generator().manual_seed(0)
    assert imageprep.random_resized_crop_params(64, 64, scale=(1.0, 1.0), ratio=(1.0, 1.0), generator=g) == (0, 0, 64, 64)
    # 10 x 100 (in_ratio 10 > 4/3) at scale 1: a box of the whole area and an aspect <= 4/3 is at least sqrt(1000 * 3/4) = 27.4 tall, so
    # all ten tries fail -> h = height, w = int(round(h * 4/3)) = 13, centred with //
    for _ in range(20):
        assert imageprep.random_resized_crop_params(10, 100, scale=(1.0, 1.0), generator=g) == (0, (100 - 13) // 2, 10, 13)
    # 100 x 10 (in_ratio 0.1 < 3/4): w = width, h = int(round(w / (3/4))) = 13
    for _ in range(20):
        assert imageprep.random_resized_crop_params(100, 10, scale=(1.0, 1.0), generator=g) == ((100 - 13) // 2, 0, 13, 10)
    # aspect inside `ratio` but every try too large: scale 4 on a square can never fit -> the whole image
    assert imageprep.random_resized_crop_params(50, 50, scale=(4.0, 4.0), generator=g) == (0, 0, 50, 50)


def test_train_image_transform_is_the_seeded_composition():
    pytest.importorskip("PIL.Image")  # the CPU route is PIL itself
    imgs = [source_image(37, 53, 1), source_image(200, 131, 2), source_image(19, 23, 3), source_image(64, 64, 4)]
    tf = augment.TrainImageTransform(32, min_scale=0.9, hflip=0.5, generator=torch.Generator().manual_seed(5))
    got = tf(imgs)
    g = torch.Generator().manual_seed(5)
    boxes = [imageprep.random_resized_crop_params(i.shape[0], i.shape[1], scale=(0.9, 1.0), generator=g) for i in imgs]
    flips = (torch.rand(4, generator=g) < 0.5).tolist()
    assert any(f for f in flips) and not all(flips) and any((h, w) != tuple(i.shape[:2]) for (t, l, h, w), i in zip(boxes, imgs))
    packed = imageprep.pack_images(imgs, 32, pin=False, crops=boxes, flips=flips)
    want = imageprep.to_tensor_normalize(imageprep.apply_packed(packed))
    assert tuple(got.shape) == (4, 3, 32, 32) and torch.equal(got, want)
    ev = augment.TrainImageTransform(32, center_crop=True)(imgs)
    assert torch.equal(ev, imageprep.to_tensor_normalize(imageprep.apply_packed(imageprep.pack_images(imgs, 32, pin=False, center_crop=True))))
    with pytest.raises(ValueError):
        augment.TrainImageTransform(32, min_scale=0.9, center_crop=True)


# ---- Mixup parameters ---------------------------------------------------------------------------------------------
def test_mixup_params_prob_zero_is_all_copies():
    for mode in ("batch", "elem", "pair"):
        kind, lam, oml, box = augment.Mixup(mixup_alpha=1.0, cutmix_alpha=1.0, prob=0.0, mode=mode).params(8, 16, 16)
        assert kind.dtype == np.int32 and lam.dtype == np.float32 and oml.dtype == np.float32 and box.dtype == np.int32
        assert kind.shape == (8,) and box.shape == (8, 4)
        assert not kind.any() and (lam == 1).all() and (oml == 0).all() and not box.any()


def test_cutmix_box_equals_the_hand_evaluated_formulas():
    m = augment.Mixup(mixup_alpha=0.0, cutmix_alpha=1.0)
    # lambda = 0.75: r = 0.5, cut = 16 x 24 of 32 x 48; centre (3, 40): y 3 -+ 8 -> clip(-5) = 0 ... 11, x 40 -+ 12 -> 28 ... clip(52) = 48
    box, lam = m.cutmix_box(32, 48, 0.75, center=(3, 40))
    assert box == (0, 11, 28, 48) and lam == 1.0 - (11 * 20) / float(32 * 48)
    # lambda = 0.36: r = 0.8, cut = int(16 * 0.8) = 12 x int(24 * 0.8) = 19; centre (8, 12): y 2 ... 14, x 12 -+ 9 -> 3 ... 21
    box, lam = m.cutmix_box(16, 24, 0.36, center=(8, 12))
    assert box == (2, 14, 3, 21) and lam == 1.0 - (12 * 18) / float(16 * 24)
    box, lam = augment.Mixup(mixup_alpha=0.0, cutmix_alpha=1.0, correct_lam=False).cutmix_box(16, 24, 0.36, center=(8, 12))
    assert box == (2, 14, 3, 21) and lam == 0.36  # uncorrected
    # zero-area box: int(H * r) == 0 -> lambda = 1 after correction
    box, lam = m.cutmix_box(16, 16, 1.0 - 1e-4, center=(5, 5))
    assert box == (5, 5, 5, 5) and lam == 1.0
    # cutmix_minmax: cut in [int(size min), int(size max)), origin in [0, size - cut), lambda always corrected
    mm = augment.Mixup(cutmix_minmax=(0.25, 0.75), correct_lam=False)
    assert mm.cutmix_alpha == 1.0
    np.random.seed(3)
    for _ in range(50):
        (yl, yh, xl, xh), lam = mm.cutmix_box(32, 48, 0.5)
        assert 8 <= yh - yl < 24 and 12 <= xh - xl < 36 and 0 <= yl and yh <= 32 and 0 <= xl and xh <= 48
        assert lam == 1.0 - (yh - yl) * (xh - xl) / float(32 * 48)


def test_zero_area_box_leaves_the_image_unchanged():
    m = augment.Mixup(mixup_alpha=0.0, cutmix_alpha=1.0, mode="elem")
    m._draw_elem = lambda n: (np.full(n, 1.0 - 1e-4, dtype=np.float32), np.ones(n, dtype=bool))  # every lambda: int(16 r) == 0
    np.random.seed(0)
    kind, lam, oml, box = m.params(4, 16, 16)
    assert (kind == 2).all() and (lam == 1).all() and (oml == 0).all() and ((box[:, 1] - box[:, 0]) * (box[:, 3] - box[:, 2]) == 0).all()
    x = torch.randn(4, 3, 16, 16, generator=torch.Generator().manual_seed(1))
    assert torch.equal(ops.mix_images(x, (kind, lam, oml, box)), x)


def test_mixup_params_modes():
    np.random.seed(1)
    kind, lam, oml, box = augment.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="pair").params(8, 32, 32)
    assert np.array_equal(kind, kind[::-1]) and np.array_equal(lam, lam[::-1]) and np.array_equal(box, box[::-1])  # mirrored
    assert len(set(lam[:4].tolist())) > 1
    kind, lam, oml, box = augment.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem").params(16, 32, 32)
    assert len(set(lam.tolist())) > 8 and set(kind.tolist()) == {1, 2}  # per-sample values, both kinds drawn
    assert np.array_equal(oml, np.float32(1.0) - lam)                   # elem / pair: fl32(1 - lambda32)
    ck = kind == 2
    assert np.array_equal(lam[ck], (1.0 - (box[ck, 1] - box[ck, 0]) * (box[ck, 3] - box[ck, 2]) / float(32 * 32)).astype(np.float32))
    assert not box[~ck].any()
    kind, lam, oml, box = augment.Mixup(mixup_alpha=0.8, mode="batch").params(6, 32, 32)
    assert (kind == 1).all() and len(set(lam.tolist())) == 1 and len(set(oml.tolist())) == 1
    # batch: lambda stays a double until the tables: fl32(lambda), fl32(1 - lambda)
    m = augment.Mixup(mixup_alpha=0.8, mode="batch")
    l0 = next(v for v in (0.3, 0.1, 0.37, 0.123456789, 0.9) if np.float32(1.0 - v) != np.float32(1.0) - np.float32(v))  # the two differ
    m._draw_batch = lambda: (l0, False)
    kind, lam, oml, box = m.params(2, 8, 8)
    assert lam[0] == np.float32(l0) and oml[0] == np.float32(1.0 - l0) and oml[0] != np.float32(1.0) - np.float32(l0)
    with pytest.raises(AssertionError):
        augment.Mixup()(torch.zeros(3, 3, 8, 8), torch.zeros(3, dtype=torch.long))
    assert "NOT claimed equal to timm" in augment.Mixup.__doc__


# ---- soft targets and the torch route of the mix ------------------------------------------------------------------------
def timm_mixup_target(target, num_classes, lam, smoothing):
    """timm/data/mixup.py: one_hot + mixup_target, restated."""
    off_value = smoothing / num_classes
    on_value = 1.0 - smoothing + off_value

    def one_hot(x):
        x = x.long().view(-1, 1)
        return torch.full((x.size()[0], num_classes), off_value).scatter_(1, x, on_value)

    return one_hot(target) * lam + one_hot(target.flip(0)) * (1.0 - lam)


def test_mix_targets_equals_the_timm_formula():
    t = torch.tensor([3, 0, 9, 9, 1, 4])
    for lam in (1.0, 0.3, 0.6180339887):
        got = ops.mix_targets(t, 10, lam, 0.1)
        assert got.dtype == torch.float32 and torch.equal(got, timm_mixup_target(t, 10, lam, 0.1))
        assert torch.allclose(got.sum(1), torch.ones(6), rtol=0, atol=4 * 2.0 ** -24 * 10)  # rows sum to 1 within fp32 rounding
    lam = torch.tensor([0.25, 1.0, 0.7, 0.7, 1.0, 0.25])
    got = ops.mix_targets(t, 10, lam.numpy(), 0.1)
    assert torch.equal(got, timm_mixup_target(t, 10, lam.unsqueeze(1), 0.1))
    assert torch.equal(ops.mix_targets(t, 10, lam, 0.0), timm_mixup_target(t, 10, lam.unsqueeze(1), 0.0))
    assert torch.allclose(got.sum(1), torch.ones(6), rtol=0, atol=4 * 2.0 ** -24 * 10)


def timm_mix(x, params_mode, tables):
    """timm's _mix_batch / _mix_elem / _mix_pair on a clone of x, with the drawn values taken from `tables` (kind, lam as the mode keeps
    it, box): Python-float lambda and the flipped batch in 'batch' mode, per-sample statements otherwise."""
    kind, lam, box = tables
    x = x.clone()
    B = len(x)
    if params_mode == "batch":
        if kind[0] == 2:
            yl, yh, xl, xh = box[0]
            x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh]
        elif kind[0] == 1:
            x_flipped = x.flip(0).mul_(1.0 - lam)
            x.mul_(lam).add_(x_flipped)
        return x
    x_orig = x.clone()
    for i in range(B):
        j = B - i - 1
        if kind[i] == 2:
            yl, yh, xl, xh = box[i]
            x[i][:, yl:yh, xl:xh] = x_orig[j][:, yl:yh, xl:xh]
        elif kind[i] == 1:
            x[i] = x[i] * lam[i] + x_orig[j] * (1 - lam[i])  # lam[i]: np.float32, as timm's lam_batch
    return x


@pytest.mark.parametrize("mode,B", [("batch", 2), ("batch", 5), ("batch", 8), ("elem", 2), ("elem", 5), ("elem", 8), ("pair", 2), ("pair", 8)])
def test_torch_route_of_mix_images_equals_the_timm_statements(mode, B):
    np.random.seed(10 * B + len(mode))
    g = torch.Generator().manual_seed(B)
    for cutmix_alpha, mixup_alpha in ((0.0, 0.8), (1.0, 0.0), (1.0, 0.8)):
        m = augment.Mixup(mixup_alpha=mixup_alpha, cutmix_alpha=cutmix_alpha, mode=mode)
        for H, W in ((16, 16), (12, 20)):  # (W = 20: a shape the kernel would refuse, the same statement here)
            x = torch.randn(B, 3, H, W, generator=g)
            (kind, lam, oml, box), tlam = m._draw(B, H, W)
            want = timm_mix(x, mode, (kind, tlam, box.tolist()))
            got = ops.mix_images(x, (kind, lam, oml, box))
            assert got is not x and got.dtype == torch.float32 and torch.equal(got, want), (mode, B, H, W)
            xi = x.clone()
            assert ops.mix_images(xi, (kind, lam, oml, box), inplace=True) is xi and torch.equal(xi, want)
            assert torch.equal(ops.mix_images(x, (kind, lam, oml, box), out_dtype=torch.bfloat16), want.to(torch.bfloat16))
            xb = x.to(torch.bfloat16)  # bf16 in: widened, mixed in fp32, rounded once
            assert torch.equal(ops.mix_images(xb, (kind, lam, oml, box)), timm_mix(xb.float(), mode, (kind, tlam, box.tolist())).to(torch.bfloat16))


def test_mixup_call_and_pad_even():
    np.random.seed(4)
    m = augment.Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", label_smoothing=0.1, num_classes=10)
    x = torch.randn(5, 3, 16, 16, generator=torch.Generator().manual_seed(2))
    t = torch.tensor([1, 2, 3, 4, 5])
    xp, tp = augment.Mixup.pad_even(x, t)
    assert xp.shape[0] == 6 and torch.equal(xp[5], x[0]) and tp.tolist() == [1, 2, 3, 4, 5, 1]
    assert augment.Mixup.pad_even(xp, tp)[0] is xp
    state = np.random.get_state()
    (kind, lam, oml, box), tlam = m._draw(6, 16, 16)
    np.random.set_state(state)
    want_x, keep = ops.mix_images(xp, (kind, lam, oml, box)), xp.clone()
    got_x, soft = m(xp, tp)
    assert got_x is xp and torch.equal(got_x, want_x) and not torch.equal(got_x, keep)  # in place
    assert tuple(soft.shape) == (6, 10) and torch.equal(soft, timm_mixup_target(tp, 10, torch.from_numpy(tlam).unsqueeze(1), 0.1))


# ---- the library ------------------------------------------------------------------------------------------------
def test_library_exports_the_new_symbols_and_documents_them():
    lib = hip.lib()
    assert lib.op_abi_version() == 10  # additive
    for name in ("op_image_resize_normalize_flip", "op_mix_images", "op_image_resize_normalize"):
        assert getattr(lib, name) is not None and name in hip.SIGNATURES
    assert len(hip.SIGNATURES["op_image_resize_normalize_flip"][1]) == len(hip.SIGNATURES["op_image_resize_normalize"][1]) + 1
    assert len(hip.SIGNATURES["op_mix_images"][1]) == 13
    text = open(os.path.join(ROOT, "include", "onepeace_hip.h")).read()
    for name, words in (("op_image_resize_normalize_flip", ("image_classify_dataset.py:59", "nlvr2_dataset.py:37", "image_text_pretrain_dataset.py:46-53",
                                                            "image_classify_dataset.py:78-84")),
                        ("op_mix_images", ("image_classify_dataset.py:46-51, 117-130", "OP_ENOTSUP", "B - 1 - i"))):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int %s\(" % name, text, flags=re.S)
        assert m, "%s is not declared behind a comment in include/onepeace_hip.h" % name
        for w in words + ("Additive: op_abi_version() stays 10",):
            assert w in m.group(1), (name, w)
    hub = open(os.path.join(ROOT, "one-peace_amd", "one_peace", "hub_interface.py")).read()
    assert "augment.TrainImageTransform" in hub and "augment.Mixup" in hub
