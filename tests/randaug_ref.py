"""numpy restatement of the RandAugment ops of timm's auto_augment.py as Pillow defines them (ImageOps.autocontrast / equalize / invert /
posterize / solarize, ImageEnhance.*, Image.transform(AFFINE, BICUBIC), Image.rotate) and of RandomErasing's store: the arithmetic
csrc/randaugment.hip implements.  tests/test_randaug_cpu.py pins every function here to PIL byte for byte; the GPU tests compare the
kernels with PIL itself.  Images are uint8 [H, W, 3] arrays; the op codes are those of imageprep.RANDAUG_OPS."""
import numpy as np

from tests import photometric_ref

(OP_NONE, OP_AUTOCONTRAST, OP_EQUALIZE, OP_INVERT, OP_POSTERIZE, OP_SOLARIZE, OP_SOLARIZE_ADD, OP_COLOR, OP_CONTRAST, OP_BRIGHTNESS,
 OP_SHARPNESS, OP_AFFINE) = range(12)


def autocontrast_lut(h):
    """ImageOps.autocontrast (cutoff 0) of one channel's histogram: two rounded fp64 operations per entry, truncated toward zero."""
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(255, max(0, int(i * scale + offset))) for i in range(256)], dtype=np.uint8)


def equalize_step(h):
    """ImageOps.equalize's step of one channel's histogram: (sum of the non-empty bins - the last of them) // 255; 0 when fewer than two."""
    nz = [int(v) for v in h if v]
    return 0 if len(nz) <= 1 else (sum(nz) - nz[-1]) // 255


def equalize_lut(h):
    step = equalize_step(h)
    if step == 0:
        return np.arange(256, dtype=np.uint8)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(255, n // step))
        n += int(h[i])
    return np.array(lut, dtype=np.uint8)


def _per_channel(img, make_lut):
    out = np.empty_like(img)
    for c in range(3):
        out[..., c] = make_lut(np.bincount(img[..., c].reshape(-1), minlength=256))[img[..., c]]
    return out


def autocontrast(img):
    return _per_channel(img, autocontrast_lut)


def equalize(img):
    return _per_channel(img, equalize_lut)


def invert(img):
    return (255 - img.astype(np.int32)).astype(np.uint8)


def posterize(img, bits):
    return (img.astype(np.int32) & ~(2 ** (8 - int(bits)) - 1) & 255).astype(np.uint8)


def solarize(img, thresh):
    p = img.astype(np.int32)
    return np.where(p < int(thresh), p, 255 - p).astype(np.uint8)


def solarize_add(img, add, thresh=128):
    p = img.astype(np.int32)
    return np.where(p < thresh, np.minimum(255, p + int(add)), p).astype(np.uint8)


def smooth(img):
    """ImageFilter.SMOOTH: the 3 x 3 kernel (1 1 1 / 1 5 1 / 1 1 1) / 13, rounded, in integers; the one-pixel border is copied."""
    a = img.astype(np.int64)
    out = img.copy()
    if a.shape[0] < 3 or a.shape[1] < 3:
        return out
    s = 4 * a[1:-1, 1:-1]
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            s = s + a[dy:a.shape[0] - 2 + dy, dx:a.shape[1] - 2 + dx]
    out[1:-1, 1:-1] = ((2 * s + 13) // 26).astype(np.uint8)
    return out


def sharpness(img, factor):
    """ImageEnhance.Sharpness: Image.blend(SMOOTH of the image, image, factor), the blend of tests/photometric_ref.py."""
    return photometric_ref.blend(smooth(img), img, factor)


def _cub(v1, v2, v3, v4, d):
    p1 = v2
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return p1 + d * (p2 + d * (p3 + d * p4))


def affine(img, coeffs, fill):
    """Image.transform(size, AFFINE, coeffs, resample=BICUBIC, fillcolor=fill) of a square or rectangular RGB image (Geometry.c:
    affine_transform + bicubic_filter32RGB), every operation a rounded fp64 one in the C expression order."""
    H, W = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = (np.float64(v) for v in coeffs)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float64) + 0.5, np.arange(H, dtype=np.float64) + 0.5)
    xin = a0 * xs + a1 * ys + a2
    yin = a3 * xs + a4 * ys + a5
    inside = ~((xin < 0) | (xin >= W) | (yin < 0) | (yin >= H))
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    ix, iy = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = xin - ix, yin - iy
    ix, iy = ix - 1, iy - 1
    src = img.astype(np.float64)
    cols = [np.clip(ix + i, 0, W - 1) for i in range(4)]
    out = np.empty_like(img)
    for c in range(3):
        ch = src[..., c]
        rows = []
        for j in range(4):
            y = iy + j
            ok = (y >= 0) & (y < H)
            yc = np.clip(y, 0, H - 1)
            r = _cub(ch[yc, cols[0]], ch[yc, cols[1]], ch[yc, cols[2]], ch[yc, cols[3]], dx)
            rows.append(r if j == 0 else np.where(ok, r, rows[j - 1]))
        v = _cub(rows[0], rows[1], rows[2], rows[3], dy)
        byte = np.where(v <= 0, 0, np.where(v >= 255, 255, np.trunc(np.clip(v, 0, 255)))).astype(np.uint8)
        out[..., c] = np.where(inside, byte, np.uint8(fill[c]))
    return out


def apply_op(img, code, arg=(0.0,) * 6, fill=(0, 0, 0)):
    """One RandAugment op by its code, arg as the kernel's fp64 [6] row."""
    code = int(code)
    if code == OP_NONE:
        return img.copy()
    if code == OP_AUTOCONTRAST:
        return autocontrast(img)
    if code == OP_EQUALIZE:
        return equalize(img)
    if code == OP_INVERT:
        return invert(img)
    if code == OP_POSTERIZE:
        return posterize(img, arg[0])
    if code == OP_SOLARIZE:
        return solarize(img, arg[0])
    if code == OP_SOLARIZE_ADD:
        return solarize_add(img, arg[0])
    if code == OP_COLOR:
        return photometric_ref.enhance(img, photometric_ref.OP_SATURATION, arg[0])
    if code == OP_CONTRAST:
        return photometric_ref.enhance(img, photometric_ref.OP_CONTRAST, arg[0])
    if code == OP_BRIGHTNESS:
        return photometric_ref.enhance(img, photometric_ref.OP_BRIGHTNESS, arg[0])
    if code == OP_SHARPNESS:
        return sharpness(img, arg[0])
    if code == OP_AFFINE:
        return affine(img, arg, fill)
    raise ValueError("unknown op code %r" % (code,))


def erase(x, boxes, noise, offs):
    """RandomErasing's store on a torch batch x [B, 3, H, W]: x[i, :, top:top+h, left:left+w] = noise_i.view(3, h, w).to(x.dtype)."""
    x = x.clone()
    for i, (top, left, h, w) in enumerate(boxes):
        if h > 0:
            x[i, :, top:top + h, left:left + w] = noise[offs[i]:offs[i] + 3 * h * w].view(3, h, w).to(x.dtype)
    return x
