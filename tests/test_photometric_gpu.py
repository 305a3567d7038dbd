"""Photometric train transforms on the device (csrc/photometric.hip: op_image_color_jitter, op_image_gaussian_blur,
op_image_normalize_flip) against PIL on the host: zero differing bytes.  Every image buffer sits between guard bytes, and every case
runs twice and must give identical bits."""
import ctypes

import numpy as np
import pytest
import torch
from PIL import Image

from one_peace_amd import hip, imageprep, ops
from tests.test_photometric_cpu import make_image, pil_blur, pil_chain

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 256  # bytes in front of and behind every buffer (a multiple of 16: the buffer stays aligned)
EINVAL = -22


class Guarded:
    """A device buffer of `shape` / `dtype` between two guard regions filled with a pattern."""

    def __init__(self, shape, dtype=torch.uint8, fill=None):
        n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
        self.raw = torch.empty(n + 2 * GUARD, dtype=torch.uint8, device=DEV)
        self.pattern = (torch.arange(GUARD, dtype=torch.int32) * 37 % 251 + 1).to(torch.uint8).to(DEV)
        self.raw[:GUARD], self.raw[GUARD + n:] = self.pattern, self.pattern
        self.t = self.raw[GUARD:GUARD + n].view(dtype).view(*shape)
        assert self.t.data_ptr() % 16 == 0 and self.t.is_contiguous()
        if fill is not None:
            self.t.copy_(torch.as_tensor(fill).to(DEV))
        self.n = n

    def intact(self):
        return torch.equal(self.raw[:GUARD], self.pattern) and torch.equal(self.raw[GUARD + self.n:], self.pattern)


def twice(fn, src):
    """fn on two guarded copies of the uint8 batch `src`: the bits of the two runs agree and the guards are intact; the result on the host."""
    outs = []
    for _ in range(2):
        g = Guarded(src.shape, fill=src)
        fn(g.t)
        torch.cuda.synchronize()
        assert g.intact()
        outs.append(g.t.cpu())
    assert torch.equal(outs[0], outs[1])
    return outs[0]


def batch(S, kinds, seed):
    return torch.from_numpy(np.stack([make_image(S, S, seed + i, k) for i, k in enumerate(kinds)]))


# ---- ColorJitter -----------------------------------------------------------------------------------------------
JITTER_CHAINS = [
    [(2, 1.3), (1, 0.8), (3, 1.1)],   # contrast first
    [(3, 0.7), (2, 0.6), (1, 1.2)],   # ... in the middle
    [(1, 1.15), (3, 1.4), (2, 1.4)],  # ... last
    None,                             # no op: untouched
    [(1, 1.0), (2, 1.0), (3, 1.0)],   # factor exactly 1
    [(3, 0.0), (2, 0.0)],             # factor 0: grey, then the mean
    [(1, 1.4), (2, 1.4), (3, 1.4)],   # 1.4 on an image with 0 and 255 bytes
]
JITTER_KINDS = ["random", "regions", "random", "random", "regions", "random", "regions"]


@pytest.mark.parametrize("S", [16, 48])
def test_color_jitter_equals_pil(S):
    src = batch(S, JITTER_KINDS, 100 + S)
    assert (src[6] == 0).any() and (src[6] == 255).any()
    ops_t, f = imageprep.jitter_table(JITTER_CHAINS)
    got = twice(lambda t: ops.color_jitter(t, ops_t, f), src)
    for i, chain in enumerate(JITTER_CHAINS):
        want = np.asarray(pil_chain(src[i].numpy(), chain or []))
        diff = int((got[i].numpy() != want).sum())
        assert diff == 0, (S, i, diff)
    assert torch.equal(got[3], src[3]) and torch.equal(got[4], src[4])


def test_color_jitter_without_contrast_and_without_any_op():
    S = 32
    src = batch(S, ["random", "regions", "random"], 7)
    chains = [[(1, 0.6), (3, 1.4)], None, [(3, 0.3)]]
    got = twice(lambda t: ops.color_jitter(t, *imageprep.jitter_table(chains)), src)
    for i, chain in enumerate(chains):
        assert np.array_equal(got[i].numpy(), np.asarray(pil_chain(src[i].numpy(), chain or []))), i
    assert torch.equal(twice(lambda t: ops.color_jitter(t, *imageprep.jitter_table([None] * 3)), src), src)
    empty = torch.empty(0, 16, 16, 3, dtype=torch.uint8, device=DEV)
    assert ops.color_jitter(empty, np.zeros((0, 3)), np.ones((0, 3))).shape == (0, 16, 16, 3)


# ---- GaussianBlur ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,big", [(16, 9.0), (48, 26.0)])
def test_gaussian_blur_equals_pil(S, big):
    radii = [0.1, 2.0, big, None, 1.234]
    assert [imageprep.gaussian_box_params(r)[0] for r in (0.1, 2.0)] == [0, 1] and imageprep.gaussian_box_params(big)[0] >= S // 2
    src = batch(S, ["random", "regions", "random", "random", "regions"], 200 + S)
    got = twice(lambda t: ops.gaussian_blur(t, radii), src)
    for i, r in enumerate(radii):
        want = src[i].numpy() if r is None else pil_blur(src[i].numpy(), r)
        diff = int((got[i].numpy() != want).sum())
        assert diff == 0, (S, i, r, diff)
    all_white = torch.full((1, S, S, 3), 255, dtype=torch.uint8)
    assert torch.equal(twice(lambda t: ops.gaussian_blur(t, [2.0]), all_white), all_white)
    assert torch.equal(twice(lambda t: ops.gaussian_blur(t, [None] * 5), src), src)


def test_gaussian_blur_at_the_largest_size_and_box_radius():
    """S = 1024 with R = 32: the largest LDS footprint (4-row tiles, 4-pixel column strips) and the cap of the box radius."""
    S, r = 1024, 33.0
    assert imageprep.gaussian_box_params(r)[0] == 32
    src = batch(S, ["regions"], 300)
    got = twice(lambda t: ops.gaussian_blur(t, [r]), src)
    diff = int((got[0].numpy() != pil_blur(src[0].numpy(), r)).sum())
    assert diff == 0, diff


# ---- ToTensor / Normalize / flip -------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [16, 48])
def test_normalize_images_equals_to_tensor_normalize(S):
    src = batch(S, ["random", "regions", "random"], 400 + S)
    g = Guarded(src.shape, fill=src)
    for flips in (None, [True, False, True], torch.tensor([0, 1, 1], dtype=torch.uint8, device=DEV)):
        fl = [False] * 3 if flips is None else [bool(v) for v in (flips.tolist() if torch.is_tensor(flips) else flips)]
        want = imageprep.to_tensor_normalize(torch.stack([s.flip(1) if f else s for s, f in zip(src, fl)]))
        for dtype in (torch.float32, torch.bfloat16):
            outs = [ops.normalize_images(g.t, dtype=dtype, flips=flips) for _ in range(2)]
            torch.cuda.synchronize()
            assert outs[0].dtype == dtype and outs[0].shape == (3, 3, S, S)
            assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0].cpu(), want.to(dtype)), (S, fl, dtype)
    assert g.intact() and torch.equal(g.t.cpu(), src)
    mean, std = (0.5, 0.4, 0.3), (0.2, 0.25, 0.3)
    assert torch.equal(ops.normalize_images(g.t, mean, std).cpu(), imageprep.to_tensor_normalize(src, mean, std))


def test_normalize_flip_output_stays_inside_its_buffer():
    S, B = 32, 3
    src = batch(S, ["random"] * B, 500)
    g_in = Guarded(src.shape, fill=src)
    flip = torch.tensor([1, 0, 1], dtype=torch.uint8, device=DEV)
    mean, std = (ctypes.c_float * 3)(*imageprep.CLIP_MEAN), (ctypes.c_float * 3)(*imageprep.CLIP_STD)
    for dtype, code in ((torch.float32, hip.DT_F32), (torch.bfloat16, hip.DT_BF16)):
        g_out = Guarded((B, 3, S, S), dtype)
        rc = hip.lib().op_image_normalize_flip(hip.ptr(g_in.t), B, S, mean, std, hip.ptr(g_out.t), code, hip.ptr(flip), hip.stream())
        torch.cuda.synchronize()
        assert rc == 0 and g_out.intact() and g_in.intact()
        want = imageprep.to_tensor_normalize(torch.stack([src[0].flip(1), src[1], src[2].flip(1)]))
        assert torch.equal(g_out.t.cpu(), want.to(dtype))


# ---- the whole chain -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [16, 48])
def test_preprocess_images_with_jitter_blur_and_flips_equals_its_cpu_route(S):
    imgs = [make_image(h, w, 600 + i, "regions" if i % 2 else "random") for i, (h, w) in enumerate([(37, 53), (200, 131), (64, 64), (19, 23), (90, 300)])]
    jitter = imageprep.jitter_table([[(2, 1.3), (1, 0.8), (3, 1.1)], None, [(3, 0.0)], [(1, 1.0), (2, 1.4)], [(1, 1.4)]])
    radii, flips = [0.1, 2.0, None, 1.234, 0.0], [True, False, True, True, False]
    for kw in ({"jitter": jitter, "blur": radii, "flips": flips}, {"jitter": jitter}, {"blur": radii, "flips": flips},
               {"jitter": jitter, "blur": radii, "center_crop": True}):
        want = ops.preprocess_images(imgs, S, **kw)
        for dtype in (torch.float32, torch.bfloat16):
            got = [ops.preprocess_images(imgs, S, dtype=dtype, device=DEV, **kw) for _ in range(2)]
            assert torch.equal(got[0], got[1]) and got[0].dtype == dtype
            assert torch.equal(got[0].cpu(), want.to(dtype)), (S, sorted(kw), dtype)
    assert torch.equal(ops.preprocess_images(imgs, S, device=DEV, flips=flips).cpu(), ops.preprocess_images(imgs, S, flips=flips))


# ---- argument checks -------------------------------------------------------------------------------------------
def test_invalid_arguments_return_before_any_launch():
    S, B = 16, 2
    src = batch(S, ["random"] * B, 700)
    g = Guarded(src.shape, fill=src)
    L, st, P = hip.lib(), hip.stream(), ctypes.c_void_p
    tab = torch.zeros(64, dtype=torch.int32, device=DEV)  # device tables: never read by a rejected call
    d = lambda off=0: P(tab.data_ptr() + off)
    h = lambda a: a.ctypes.data_as(P)
    ops_ok, f_ok = np.array([[1, 2, 3], [0, 0, 0]], np.int32), np.full((B, 3), 0.5, np.float32)

    def jitter(img=None, B_=B, S_=S, ops_h=ops_ok, f_h=f_ok, ops_d=None, sums=None):
        return L.op_image_color_jitter(hip.ptr(g.t) if img is None else img, B_, S_, d(0) if ops_d is None else ops_d, d(32), h(ops_h), h(f_h),
                                       d(64) if sums is None else sums, st)

    assert jitter(S_=8) == EINVAL and jitter(S_=24) == EINVAL and jitter(S_=1040) == EINVAL and jitter(B_=-1) == EINVAL
    assert jitter(img=P(0)) == EINVAL and jitter(img=P(g.t.data_ptr() + 4)) == EINVAL
    assert jitter(ops_d=P(0)) == EINVAL and jitter(sums=P(0)) == EINVAL and jitter(ops_d=d(2)) == EINVAL
    assert jitter(ops_h=np.array([[1, 4, 0], [0, 0, 0]], np.int32)) == EINVAL
    assert jitter(ops_h=np.array([[-1, 0, 0], [0, 0, 0]], np.int32)) == EINVAL
    assert jitter(ops_h=np.array([[2, 1, 2], [0, 0, 0]], np.int32)) == EINVAL
    for bad in (-0.5, float("nan"), float("inf")):
        f = f_ok.copy()
        f[1, 2] = bad
        assert jitter(f_h=f) == EINVAL
    assert b"op_image_color_jitter" in L.op_last_error()
    assert jitter(B_=0) == 0 and jitter(B_=0, img=P(0)) == 0

    R_ok, on_ok = np.array([1, 32], np.int32), np.array([1, 1], np.uint8)

    def blur(img=None, B_=B, S_=S, R_h=R_ok, on_h=on_ok, R_d=None):
        return L.op_image_gaussian_blur(hip.ptr(g.t) if img is None else img, B_, S_, d(0) if R_d is None else R_d, d(16), d(32), d(48), h(R_h),
                                        h(on_h), st)

    assert blur(S_=0) == EINVAL and blur(S_=1056) == EINVAL and blur(S_=40) == EINVAL and blur(B_=-3) == EINVAL
    assert blur(img=P(0)) == EINVAL and blur(img=P(g.t.data_ptr() + 8)) == EINVAL and blur(R_d=P(0)) == EINVAL and blur(R_d=d(1)) == EINVAL
    assert blur(R_h=np.array([1, 33], np.int32)) == EINVAL and blur(R_h=np.array([-1, 0], np.int32)) == EINVAL
    assert b"op_image_gaussian_blur" in L.op_last_error()
    assert blur(B_=0) == 0
    assert blur(R_h=np.array([1, 33], np.int32), on_h=np.zeros(2, np.uint8)) == 0  # no image is blurred: nothing is checked or launched

    out = Guarded((B, 3, S, S), torch.float32)
    mean, std = (ctypes.c_float * 3)(*imageprep.CLIP_MEAN), (ctypes.c_float * 3)(*imageprep.CLIP_STD)
    norm = lambda src_=None, S_=S, dt=hip.DT_F32, out_=None, m=mean: L.op_image_normalize_flip(
        hip.ptr(g.t) if src_ is None else src_, B, S_, m, std, hip.ptr(out.t) if out_ is None else out_, dt, None, st)
    assert norm(S_=20) == EINVAL and norm(dt=2) == EINVAL and norm(src_=P(0)) == EINVAL and norm(out_=P(0)) == EINVAL
    assert norm(out_=P(out.t.data_ptr() + 4)) == EINVAL and norm(m=None) == EINVAL and norm(out_=hip.ptr(g.t)) == EINVAL
    torch.cuda.synchronize()
    assert g.intact() and torch.equal(g.t.cpu(), src) and out.intact() and not tab.any()
    with pytest.raises(ValueError):
        ops.gaussian_blur(g.t, [1.0, 40.0])
    with pytest.raises(ValueError):
        ops.color_jitter(g.t[:, :, :8], np.zeros((B, 3)), np.ones((B, 3)))  # not square / not contiguous
