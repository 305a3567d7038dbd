"""RandAugment and RandomErasing on the device (csrc/randaugment.hip: op_image_randaug_layer, op_image_erase) against Pillow and torch on the
host: zero differing bytes.  Every image buffer sits between guard bytes, and every case runs twice and must give identical bits."""
import ctypes

import numpy as np
import pytest
import torch

from one_peace_amd import augment, hip, imageprep, ops
from tests.test_photometric_cpu import make_image
from tests.test_photometric_gpu import DEV, EINVAL, Guarded, twice
from tests.test_randaug_cpu import (ENHANCE_ITEMS, FILL, HIST_ITEMS, KINDS, POINT_ITEMS, SHARP_ITEMS, geometric_items, pil_named,
                                    special_image)

pytestmark = pytest.mark.gpu
B = 8


def run_family(S, items, seed):
    """Every item on every kind of image, in batches of B images with one untouched image each: zero bytes off Pillow."""
    items = list(items)
    for k in range(-len(items) % (B - 1)):  # whole batches: the first items once more
        items.append(items[k % len(items)])
    for first in range(0, len(items), B - 1):
        for shift in range(len(KINDS)):
            group = items[first:first + B - 1]
            group.insert(shift % B, ("none",))
            src = torch.from_numpy(np.stack([special_image(S, seed + 10 * first + i, KINDS[(i + shift) % len(KINDS)]) for i in range(B)]))
            tab = imageprep.randaug_table([[it] for it in group], S)
            got = twice(lambda t: ops.rand_augment(t, *tab, FILL), src)
            for i, item in enumerate(group):
                want = pil_named(src[i].numpy(), item)
                diff = int((got[i].numpy() != want).sum())
                assert diff == 0, (S, item, KINDS[(i + shift) % len(KINDS)], diff)
            assert torch.equal(got[shift % B], src[shift % B])


@pytest.mark.parametrize("S", [16, 48])
def test_pointwise_ops_equal_pil(S):
    run_family(S, POINT_ITEMS, 100 + S)


@pytest.mark.parametrize("S", [16, 48])
def test_histogram_ops_equal_pil(S):
    run_family(S, HIST_ITEMS * 3 + [("Equalize",)], 200 + S)


@pytest.mark.parametrize("S", [16, 48])
def test_sharpness_equals_pil(S):
    run_family(S, SHARP_ITEMS * 2 + [("Sharpness", 0.55)], 300 + S)


@pytest.mark.parametrize("S", [16, 48])
def test_affine_ops_equal_pil(S):
    run_family(S, geometric_items(S), 400 + S)


@pytest.mark.parametrize("S", [16, 48])
def test_enhance_ops_go_through_color_jitter_and_equal_pil(S):
    run_family(S, ENHANCE_ITEMS, 500 + S)


@pytest.mark.parametrize("S", [16, 48])
def test_two_layers_hand_over_in_both_orders(S):
    """Pairs of a pointwise (P), a histogram (H), a neighbourhood (N) op and an ImageEnhance blend (E, op_image_color_jitter) in both orders."""
    P, H, N, N2, E, E2 = ("Solarize", 100), ("Equalize",), ("Rotate", 17.0), ("Sharpness", 1.7), ("Contrast", 1.4), ("Color", 0.3)
    layers = [[P, H], [H, P], [P, N], [N, P], [H, N], [N, H], [E, N], [N, E], [E, H], [H, E], [P, E], [E2, P], [N2, N], [N, N2],
              [("AutoContrast",), N2], [("ShearX", -0.3), ("Equalize",)], [("none",), H], [N, ("none",)], None, [H, H]]
    src = torch.from_numpy(np.stack([special_image(S, 600 + S + i, KINDS[i % len(KINDS)]) for i in range(len(layers))]))
    tab = imageprep.randaug_table(layers, S)
    assert tab[0].shape == (len(layers), 2)
    got = twice(lambda t: ops.rand_augment(t, *tab, FILL), src)
    for i, la in enumerate(layers):
        want = src[i].numpy()
        for item in la or []:
            want = pil_named(want, item)
        diff = int((got[i].numpy() != want).sum())
        assert diff == 0, (S, la, diff)
    assert torch.equal(got[18], src[18])


def test_largest_image_counters_and_rotate():
    """S = 1024: a bin of the histogram holds up to 2^20 pixels (a constant image: all of them; half 0 / half 255: 2^19 each)."""
    S = 1024
    const = special_image(S, 0, "const")
    halves = np.zeros((S, S, 3), np.uint8)
    halves[S // 2:] = 255
    ramp = np.zeros((S, S, 3), np.uint8)  # 4096 pixels per value in every channel: Equalize's step is 4096
    ramp[..., 0], ramp[..., 1], ramp[..., 2] = np.arange(S)[None, :] // 4, np.arange(S)[:, None] // 4, 255 - np.arange(S)[None, :] // 4
    for a in (const, halves, ramp):
        for item in HIST_ITEMS:
            src = torch.from_numpy(a[None])
            got = twice(lambda t: ops.rand_augment(t, *imageprep.randaug_table([[item]], S), FILL), src)
            diff = int((got[0].numpy() != pil_named(a, item)).sum())
            assert diff == 0, (item, diff)
    a = make_image(S, S, 700, "regions")
    got = twice(lambda t: ops.rand_augment(t, *imageprep.randaug_table([[("Rotate", -30.0)]], S), FILL), torch.from_numpy(a[None]))
    diff = int((got[0].numpy() != pil_named(a, ("Rotate", -30.0))).sum())
    assert diff == 0, diff


# ---- RandomErasing ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [16, 48])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_erase_equals_the_slice_assignment(S, dtype):
    n = 6
    cases = [
        [(0, 0, 3, 5), (0, S - 4, 2, 4), None, (S - 3, 0, 3, 2), (S - 2, S - 5, 2, 5), None],          # the four corners
        [(0, 3, 2, 6), (S - 4, 2, 4, 3), (5, 0, 4, 1), (2, S - 3, 7, 3), (7, 9, 1, 1), (0, 0, S - 1, S - 1)],  # the four edges, 1 x 1, the largest
        [(1, 1, S - 1, S - 1), None, None, (S - 1, S - 1, 1, 1), None, (3, 2, S - 4, 1)],
    ]
    for k, case in enumerate(cases):
        boxes = [(0, 0, 0, 0) if b is None else b for b in case]
        total = sum(3 * h * w for _, _, h, w in boxes)
        noise = torch.randn(total, generator=torch.Generator().manual_seed(k)) * 3
        x = torch.randn(n, 3, S, S, generator=torch.Generator().manual_seed(10 + k)).to(dtype)
        want = ops.erase_images(x.clone(), boxes, noise)
        assert not torch.equal(want, x)
        outs = []
        for _ in range(2):
            g = Guarded((n, 3, S, S), dtype, fill=x)
            assert ops.erase_images(g.t, boxes, noise.to(DEV)) is g.t
            torch.cuda.synchronize()
            assert g.intact()
            outs.append(g.t.cpu())
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], want), (S, dtype, k)
        for i, b in enumerate(case):
            if b is None:
                assert torch.equal(outs[0][i], x[i])
    # RandomErasing itself: the same seeded generator erases the same boxes with the same noise on both routes
    for mode in ("pixel", "rand", "const"):
        x = torch.randn(n, 3, S, S, generator=torch.Generator().manual_seed(20)).to(dtype)
        want = augment.RandomErasing(0.7, mode=mode, generator=torch.Generator().manual_seed(21))(x.clone())
        got = augment.RandomErasing(0.7, mode=mode, generator=torch.Generator().manual_seed(21))(x.to(DEV))
        assert got.is_cuda and torch.equal(got.cpu(), want) and not torch.equal(want, x), mode


# ---- argument checks -------------------------------------------------------------------------------------------
def test_invalid_arguments_return_before_any_launch():
    S, n = 16, 2
    src = torch.from_numpy(np.stack([make_image(S, S, 800 + i) for i in range(n)]))
    g, scratch = Guarded(src.shape, fill=src), Guarded(src.shape, fill=src.flip(0))
    L, st, P = hip.lib(), hip.stream(), ctypes.c_void_p
    tab = torch.zeros(2048, dtype=torch.int32, device=DEV)  # device tables and histograms: never read or written by a rejected call
    d = lambda off=0: P(tab.data_ptr() + off)
    h = lambda a: a.ctypes.data_as(P)
    ops_ok, args_ok, fill = np.array([11, 2], np.int32), np.zeros((n, 6), np.float64), (ctypes.c_ubyte * 3)(*FILL)
    args_ok[0] = (1, 0.1, 0, 0, 1, 0)

    def layer(img=None, B_=n, S_=S, op_h=ops_ok, arg_h=args_ok, op_d=None, arg_d=None, fill_=fill, hist=None, scr=None):
        return L.op_image_randaug_layer(hip.ptr(g.t) if img is None else img, B_, S_, d(0) if op_d is None else op_d,
                                        d(64) if arg_d is None else arg_d, h(op_h), h(arg_h), fill_, d(512) if hist is None else hist,
                                        hip.ptr(scratch.t) if scr is None else scr, st)

    assert layer(S_=8) == EINVAL and layer(S_=24) == EINVAL and layer(S_=1040) == EINVAL and layer(B_=-1) == EINVAL and layer(B_=65536) == EINVAL
    assert layer(img=P(0)) == EINVAL and layer(img=P(g.t.data_ptr() + 4)) == EINVAL
    assert layer(scr=P(0)) == EINVAL and layer(scr=P(scratch.t.data_ptr() + 8)) == EINVAL and layer(scr=hip.ptr(g.t)) == EINVAL
    assert layer(scr=P(g.t.data_ptr() + 16)) == EINVAL  # overlaps the batch
    assert layer(op_d=P(0)) == EINVAL and layer(arg_d=P(0)) == EINVAL and layer(hist=P(0)) == EINVAL and layer(fill_=None) == EINVAL
    assert layer(op_d=d(2)) == EINVAL and layer(arg_d=d(68)) == EINVAL and layer(hist=d(514)) == EINVAL
    for bad in (7, 8, 9, 12, -1):
        assert layer(op_h=np.array([bad, 0], np.int32)) == EINVAL
    assert b"op_image_randaug_layer" in L.op_last_error()

    def with_arg(op, *vals):
        a = np.zeros((n, 6), np.float64)
        a[1, :len(vals)] = vals
        return layer(op_h=np.array([0, op], np.int32), arg_h=a)

    for op, vals in ((4, (8,)), (4, (-1,)), (4, (2.5,)), (5, (257,)), (5, (-1,)), (5, (float("nan"),)), (6, (256,)), (6, (0.5,)), (10, (-0.1,)),
                     (10, (float("inf"),)), (10, (float("nan"),)), (11, (1, 0, float("nan"), 0, 1, 0)), (11, (1, 0, 0, 0, 1, float("inf")))):
        assert with_arg(op, *vals) == EINVAL, (op, vals)
    assert layer(B_=0) == 0 and layer(B_=0, img=P(0), scr=P(0)) == 0
    assert layer(op_h=np.zeros(n, np.int32), arg_h=np.full((n, 6), np.nan)) == 0  # no image has an op: nothing is checked further or launched

    x = Guarded((n, 3, S, S), torch.float32, fill=torch.ones(n, 3, S, S))
    noise = torch.zeros(3 * S * S, device=DEV)
    box_ok = np.array([[1, 2, 3, 4], [0, 0, 0, 0]], np.int32)

    def erase(x_=None, dt=hip.DT_F32, B_=n, S_=S, box_h=box_ok, box_d=None, off=None, noise_=None):
        return L.op_image_erase(hip.ptr(x.t) if x_ is None else x_, dt, B_, S_, d(0) if box_d is None else box_d, h(box_h),
                                hip.ptr(noise) if noise_ is None else noise_, d(64) if off is None else off, st)

    assert erase(dt=2) == EINVAL and erase(S_=0) == EINVAL and erase(S_=16385) == EINVAL and erase(B_=-1) == EINVAL and erase(B_=65536) == EINVAL
    assert erase(x_=P(0)) == EINVAL and erase(x_=P(x.t.data_ptr() + 2)) == EINVAL and erase(box_d=P(0)) == EINVAL and erase(off=P(0)) == EINVAL
    assert erase(box_d=d(2)) == EINVAL and erase(off=d(68)) == EINVAL and erase(noise_=P(0)) == EINVAL and erase(noise_=P(noise.data_ptr() + 2)) == EINVAL
    for bad in ((-1, 0, 2, 2), (0, -1, 2, 2), (0, 0, -1, 2), (0, 0, 2, 0), (15, 0, 2, 2), (0, 13, 2, 4), (0, 0, 17, 1), (0, 0, 1, 17)):
        assert erase(box_h=np.array([bad, (0, 0, 0, 0)], np.int32)) == EINVAL, bad
    assert b"op_image_erase" in L.op_last_error()
    assert erase(B_=0) == 0 and erase(box_h=np.zeros((n, 4), np.int32), noise_=P(0)) == 0  # nothing erased: no launch, no noise needed
    torch.cuda.synchronize()
    assert g.intact() and torch.equal(g.t.cpu(), src) and scratch.intact() and torch.equal(scratch.t.cpu(), src.flip(0))
    assert x.intact() and bool((x.t == 1).all()) and not tab.any()
    tab_ok = imageprep.randaug_table([[("Invert",)], None])
    with pytest.raises(ValueError):
        ops.rand_augment(g.t[:, :, :8], *tab_ok, FILL)  # not square / not contiguous
    with pytest.raises(ValueError):
        ops.erase_images(x.t[:, :, :8], [(0, 0, 1, 1)] * n, torch.zeros(6, device=DEV))  # not square
    with pytest.raises(ValueError):
        ops.erase_images(x.t, [(0, 0, 1, 1)] * n, torch.zeros(6))  # the noise is not on x's device


# ---- the whole chain -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [16, 48])
def test_preprocess_images_with_randaug_equals_its_cpu_route(S):
    imgs = [make_image(h, w, 900 + i, "regions" if i % 2 else "random") for i, (h, w) in enumerate([(37, 53), (200, 131), (64, 64), (19, 23), (90, 300)])]
    crops = [(3, 5, 30, 40), (10, 20, 150, 100), (0, 0, 64, 64), (1, 2, 17, 20), (5, 100, 80, 120)]
    flips = [True, False, True, True, False]
    layers = [[("ShearX", 0.21), ("Equalize",)], None, [("Contrast", 1.4), ("Rotate", -17.0)], [("Sharpness", 0.4), ("Solarize", 77)],
              [("TranslateX", 0.3 * S), ("AutoContrast",)]]
    tab = imageprep.randaug_table(layers, S) + (FILL,)
    for kw in ({"crops": crops, "flips": flips}, {"flips": flips}, {"center_crop": True}, {}):
        want = ops.preprocess_images(imgs, S, randaug=tab, **kw)
        for dtype in (torch.float32, torch.bfloat16):
            got = [ops.preprocess_images(imgs, S, dtype=dtype, device=DEV, randaug=tab, **kw) for _ in range(2)]
            assert torch.equal(got[0], got[1]) and got[0].dtype == dtype
            assert torch.equal(got[0].cpu(), want.to(dtype)), (S, sorted(kw), dtype)
    assert torch.equal(ops.preprocess_images(imgs, S, device=DEV, flips=flips, randaug=None).cpu(), ops.preprocess_images(imgs, S, flips=flips))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_create_transform_equals_its_cpu_route_under_one_seed(dtype):
    S = 48
    imgs = [make_image(h, w, 950 + i, "regions" if i % 2 else "random") for i, (h, w) in enumerate([(37, 53), (200, 131), (64, 64), (59, 83), (90, 300), (48, 48)])]
    for seed in (1, 2):
        make = lambda: augment.create_transform(S, True, 0.4, "rand-m9-mstd0.5-inc1", "bicubic", re_prob=0.6, re_mode="pixel", re_count=1,
                                                generator=torch.Generator().manual_seed(seed))
        want = make()(imgs, dtype, "cpu")
        got = make()(imgs, dtype, DEV)
        assert got.is_cuda and got.dtype == dtype and got.shape == (6, 3, S, S)
        assert torch.equal(got.cpu(), want), (dtype, seed)
    plain = lambda: augment.create_transform(S, True, 0.4, generator=torch.Generator().manual_seed(3))
    assert torch.equal(plain()(imgs, dtype, DEV).cpu(), plain()(imgs, dtype, "cpu"))
    ev = augment.create_transform(S, False)
    assert torch.equal(ev(imgs, dtype, DEV).cpu(), ev(imgs, dtype, "cpu"))
