"""numpy restatement of the photometric train transforms (ColorJitter through PIL.ImageEnhance, ImageFilter.GaussianBlur), the
arithmetic csrc/photometric.hip implements.  tests/test_photometric_cpu.py pins every function here to PIL bit for bit; the GPU
tests compare the kernels with PIL itself.  Images are uint8 [H, W, 3] arrays."""
import math

import numpy as np

OP_NONE, OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION = 0, 1, 2, 3


def luma(img):
    """PIL's convert("L") of an RGB image: (19595 R + 38470 G + 7471 B + 0x8000) >> 16."""
    a = img.astype(np.int64)
    return (19595 * a[..., 0] + 38470 * a[..., 1] + 7471 * a[..., 2] + 0x8000) >> 16


def contrast_mean(img):
    """int(ImageStat.Stat(L).mean[0] + 0.5) in integers: (2 sum + count) // (2 count)."""
    L = luma(img)
    return int((2 * int(L.sum()) + L.size) // (2 * L.size))


def blend(degenerate, img, factor):
    """Image.blend(degenerate, image, factor) per byte: t = fadd_rn(d, fmul_rn(f, p - d)) in fp32, truncated for 0 <= f <= 1, clipped
    to 0 ... 255 first otherwise."""
    f = np.float32(factor)
    d = np.broadcast_to(np.asarray(degenerate), img.shape).astype(np.int32)
    p = img.astype(np.int32)
    prod = (f * (p - d).astype(np.float32)).astype(np.float32)
    t = (d.astype(np.float32) + prod).astype(np.float32)
    if np.float32(0) <= f <= np.float32(1):
        return t.astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t)).astype(np.uint8)


def enhance(img, op, factor):
    """One ImageEnhance step: Brightness (degenerate 0), Contrast (the rounded mean of L), Color (L of the pixel)."""
    if op == OP_NONE:
        return img.copy()
    if op == OP_BRIGHTNESS:
        return blend(0, img, factor)
    if op == OP_CONTRAST:
        return blend(contrast_mean(img), img, factor)
    if op == OP_SATURATION:
        return blend(luma(img)[..., None], img, factor)
    raise ValueError("unknown op %r" % (op,))


def color_jitter(img, ops, factors):
    """The ordered chain of enhancers, each on the uint8 result of the one before."""
    for op, f in zip(ops, factors):
        img = enhance(img, int(op), f)
    return img


def gaussian_box_params(radius):
    """(R, ww, fw) of the three extended box blurs ImageFilter.GaussianBlur(radius) runs per axis (BoxBlur.c)."""
    r = np.float32(radius)
    s2 = float(np.float32(np.float32(r * r) / np.float32(3)))
    L = math.sqrt(12.0 * s2 + 1.0)
    l = math.floor((L - 1.0) / 2.0)
    a = (2 * l + 1) * (l * (l + 1) - 3 * s2) / (6 * (s2 - (l + 1) * (l + 1)))
    fr = np.float32(l + a)
    R = int(fr)
    ww = int(np.float32(1 << 24) / np.float32(np.float32(2) * fr + np.float32(1)))
    fw = ((1 << 24) - (2 * R + 1) * ww) // 2
    return R, ww, fw


def box_pass(a, R, ww, fw, axis):
    """One extended box blur along `axis` of a uint8 array: (acc ww + far fw + 2^23) >> 24 in 32-bit unsigned arithmetic, edges
    clamped."""
    n = a.shape[axis]
    src = np.moveaxis(a, axis, 0).astype(np.uint64)
    x = np.arange(n)
    acc = np.zeros_like(src)
    for i in range(-R, R + 1):
        acc += src[np.clip(x + i, 0, n - 1)]
    far = src[np.clip(x - R - 1, 0, n - 1)] + src[np.clip(x + R + 1, 0, n - 1)]
    out = ((acc * np.uint64(ww) + far * np.uint64(fw) + np.uint64(1 << 23)) & np.uint64(0xFFFFFFFF)) >> np.uint64(24)
    return np.moveaxis(out.astype(np.uint8), 0, axis)


def gaussian_blur(img, radius):
    """ImageFilter.GaussianBlur(radius) on an RGB image: three passes along x, then three along y."""
    R, ww, fw = gaussian_box_params(radius)
    for axis in (1, 0):
        for _ in range(3):
            img = box_pass(img, R, ww, fw, axis)
    return img
