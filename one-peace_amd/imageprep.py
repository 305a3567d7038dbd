"""Host side of the hub's image transform (one_peace/models/one_peace/hub_interface.py:94-101): ``Resize((S, S), BICUBIC)``
on a PIL RGB image, ``ToTensor``, ``Normalize(CLIP mean / std)`` (data/base_dataset.py:23-24).

The resize is Pillow's ``Image.resize((S, S), Image.BICUBIC)`` for 8-bit images (src/libImaging/Resample.c): a horizontal pass
over the source rows the vertical filter reads, a uint8 intermediate, then the vertical pass, both with 22-bit fixed-point
weights.  ``bicubic_coeffs`` restates Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` so that the device kernel
(csrc/image.hip, op_image_resize_normalize) reproduces PIL bit for bit; ``pack_images`` stages the images and the tables for one
host-to-device copy.  ``apply_coeffs`` is the same arithmetic in torch, the CPU reference of the tests only."""
import math

import numpy as np
import torch

CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)  # data/base_dataset.py:23-24
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)

PRECISION_BITS = 32 - 8 - 2  # Resample.c: 22 fraction bits, so that 255 * sum|w| fits an int32 accumulator
MAX_SIZE = 1024              # S: a multiple of 16 up to this (op_image_resize_normalize)
SRC_SLACK = 16               # readable bytes the kernel needs behind the last image (it reads 16-byte windows)
DESC_FIELDS = 11             # int64 per image in the descriptor table (include/onepeace_hip.h)


def _bicubic(x):
    """Resample.c bicubic_filter, a = -0.5 (float64, evaluated in the C expression order)."""
    a = -0.5
    x = np.abs(x)
    inner = ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    outer = (((x - 5) * x + 8) * x - 4) * a
    return np.where(x < 1.0, inner, np.where(x < 2.0, outer, 0.0))


def bicubic_coeffs(in_size, out_size):
    """(xmin int32 [out], taps int32 [out], weights int32 [out, ksize]) of Pillow's bicubic filter from `in_size` to `out_size`
    samples: support 2 x max(scale, 1), float64 weights normalised by their (sequential) sum, then int(w * 2^22 +- 0.5) toward
    zero.  Output sample o reads input samples xmin[o] ... xmin[o] + taps[o] - 1; weights past taps[o] are zero."""
    if in_size < 1 or out_size < 1:
        raise ValueError("bicubic_coeffs: sizes must be >= 1, got %d -> %d" % (in_size, out_size))
    scale = float(in_size) / out_size
    filterscale = max(scale, 1.0)
    support = 2.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    center = (np.arange(out_size, dtype=np.float64) + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = np.maximum(np.trunc(center - support + 0.5).astype(np.int64), 0)
    xmax = np.minimum(np.trunc(center + support + 0.5).astype(np.int64), in_size) - xmin
    x = np.arange(ksize, dtype=np.int64)
    live = x[None, :] < xmax[:, None]
    w = np.where(live, _bicubic(((x[None, :] + xmin[:, None]).astype(np.float64) - center[:, None] + 0.5) * ss), 0.0)
    ww = np.zeros(out_size, dtype=np.float64)
    for j in range(ksize):  # Pillow sums in tap order; a pairwise sum could round differently
        ww += w[:, j]
    w = np.where(ww[:, None] != 0.0, w / np.where(ww == 0.0, 1.0, ww)[:, None], w)
    fixed = np.trunc(np.where(w < 0, -0.5 + w * (1 << PRECISION_BITS), 0.5 + w * (1 << PRECISION_BITS)))
    return xmin.astype(np.int32), xmax.astype(np.int32), fixed.astype(np.int32)


def vertical_first(H, W, size):
    """Pillow's Image.resize runs the vertical pass first, over all W columns, for an image more than 100 times taller than wide
    that shrinks vertically (PIL/Image.py, resize: `self.size[1] > self.size[0] * 100 and size[1] < self.size[1]`)."""
    return H > W * 100 and size < H


def _clip8(acc):
    return torch.clamp(acc >> PRECISION_BITS, 0, 255).to(torch.uint8)


def _pass(src, coeffs, dim):
    """One fixed-point pass of Resample.c along `dim` of an int64 [H, W, 3] tensor (rows: dim 0, columns: dim 1)."""
    xmin, taps, w = (torch.from_numpy(np.ascontiguousarray(c)).long() for c in coeffs)
    k = torch.arange(w.shape[1])
    idx = (xmin[:, None] + k[None, :]).clamp(max=src.shape[dim] - 1)
    w = torch.where(k[None, :] < taps[:, None], w, torch.zeros_like(w))
    g = src.index_select(dim, idx.reshape(-1))
    if dim == 1:
        g = g.reshape(src.shape[0], *idx.shape, 3)
        acc = (g * w[None, :, :, None]).sum(2)
    else:
        g = g.reshape(*idx.shape, src.shape[1], 3)
        acc = (g * w[:, :, None, None]).sum(1)
    return _clip8(acc + (1 << (PRECISION_BITS - 1))).long()


def apply_coeffs(image, size):
    """uint8 [size, size, 3]: ``Image.resize((size, size), BICUBIC)`` of a uint8 HWC RGB tensor, restated in torch (the CPU
    reference of the tests; the product path is PIL on the host or op_image_resize_normalize on a device).  Horizontal pass over
    the source rows the vertical filter reads, clip to uint8, vertical pass; the other order where vertical_first() says so."""
    img = torch.as_tensor(image)
    H, W = img.shape[0], img.shape[1]
    cx, cy = bicubic_coeffs(W, size), bicubic_coeffs(H, size)
    if vertical_first(H, W, size):
        return _pass(_pass(img.long(), cy, 0), cx, 1).to(torch.uint8)
    row0, row1 = int(cy[0][0]), int(cy[0][-1] + cy[1][-1])
    tmp = _pass(img[row0:row1].long(), cx, 1)
    cy = (cy[0] - row0, cy[1], cy[2])
    return _pass(tmp, cy, 0).to(torch.uint8)


def to_tensor_normalize(u8, mean=CLIP_MEAN, std=CLIP_STD):
    """fp32 [..., 3, S, S] from uint8 [..., S, S, 3] in torchvision's order: ToTensor (u / 255) then Normalize ((x - mean) / std),
    true fp32 divisions (the reference runs them on CPU tensors)."""
    x = torch.as_tensor(u8).movedim(-1, -3).to(torch.float32).div(255)
    m = torch.tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.tensor(std, dtype=torch.float32)[:, None, None]
    return x.sub(m).div(s)


def check_size(size):
    if not (16 <= size <= MAX_SIZE and size % 16 == 0):
        raise ValueError("image size must be a multiple of 16 in [16, %d], got %d" % (MAX_SIZE, size))


class PackedImages:
    """A batch of uint8 HWC RGB images of different sizes and their filter tables, staged for op_image_resize_normalize.

    Layout of the ONE buffer (pinned on the host, copied to the device with one H2D copy): the images back to back (each at a
    16-byte aligned offset) plus SRC_SLACK readable bytes, then the descriptor table int64 [B, DESC_FIELDS], then the coefficient
    records int32.  A record is [xmin, taps, 0, 0, w_0 ... w_{k-1}] with k a multiple of 4 (zero-padded), S records per axis and
    image.  `desc` is the host copy of the table; `workspace_bytes` the size of the uint8 intermediates (rows x S x 3 bytes per image,
    S x W x 3 for an image whose vertical pass goes first)."""

    def __init__(self, host, desc, src_bytes, desc_off, coef_off, coef_count, workspace_bytes, size, sizes):
        self.host, self.desc, self.size, self.sizes = host, desc, size, sizes
        self.src_bytes, self.desc_off, self.coef_off, self.coef_count = src_bytes, desc_off, coef_off, coef_count
        self.workspace_bytes = workspace_bytes

    def __len__(self):
        return self.desc.shape[0]


def as_rgb_array(im):
    """The uint8 [H, W, 3] numpy array of an image array / tensor (H, W >= 1); anything else is a ValueError."""
    a = im.detach().cpu().numpy() if torch.is_tensor(im) else np.asarray(im)
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
        raise ValueError("images must be uint8 [H, W, 3] with H, W >= 1, got %s %s" % (a.dtype, a.shape))
    return np.ascontiguousarray(a)


def _align(n, a=16):
    return (n + a - 1) // a * a


def _record_block(coeffs, size):
    xmin, taps, w = coeffs
    k = _align(w.shape[1], 4)
    rec = np.zeros((size, 4 + k), dtype=np.int32)
    rec[:, 0], rec[:, 1] = xmin, taps
    rec[:, 4:4 + w.shape[1]] = w
    return rec, k


def pack_images(images, size, pin=True):
    """PackedImages of uint8 HWC RGB arrays / tensors (H, W >= 1) for an S x S resize."""
    check_size(size)
    arrs = [as_rgb_array(im) for im in images]
    B = len(arrs)
    desc = np.zeros((B, DESC_FIELDS), dtype=np.int64)
    blocks, src_off, coef_ints, tmp_off = [], 0, 0, 0
    for i, a in enumerate(arrs):
        H, W = a.shape[:2]
        cx, cy = bicubic_coeffs(W, size), bicubic_coeffs(H, size)
        if max(np.abs(cx[2]).max(), np.abs(cy[2]).max()) >= 1 << 23:  # the kernel multiplies on the 24-bit multiplier
            raise ValueError("pack_images: a filter weight of %d x %d -> %d does not fit 24 bits" % (H, W, size))
        rx, kx = _record_block(cx, size)
        ry, ky = _record_block(cy, size)
        vfirst = vertical_first(H, W, size)
        if vfirst:  # intermediate: the S rows of the vertical pass over all W columns
            row0, rows, tmp_bytes = 0, size, size * W * 3
        else:       # intermediate: the source rows the vertical filter reads, each resized to S columns
            row0 = int(cy[0][0])
            rows = int(cy[0][-1] + cy[1][-1]) - row0
            tmp_bytes = rows * size * 3
        desc[i] = (src_off, H, W, coef_ints, kx, coef_ints + rx.size, ky, tmp_off, row0, rows, int(vfirst))
        blocks += [rx.reshape(-1), ry.reshape(-1)]
        src_off = _align(src_off + H * W * 3)
        coef_ints += rx.size + ry.size
        tmp_off += _align(tmp_bytes)
    src_bytes = _align(src_off + SRC_SLACK)
    desc_off = src_bytes
    coef_off = _align(desc_off + desc.nbytes)
    total = coef_off + coef_ints * 4
    host = torch.empty(total, dtype=torch.uint8, pin_memory=pin)
    buf = host.numpy()
    for i, a in enumerate(arrs):
        o = int(desc[i, 0])
        buf[o:o + a.size] = a.reshape(-1)
        buf[o + a.size:_align(o + a.size)] = 0  # alignment gaps and the slack are read (under zero weights): keep them defined
    buf[src_off:src_bytes] = 0
    buf[desc_off:desc_off + desc.nbytes] = desc.view(np.uint8).reshape(-1)
    if blocks:
        buf[coef_off:] = np.concatenate(blocks).view(np.uint8)
    sizes = [(int(a.shape[1]), int(a.shape[0])) for a in arrs]  # (width, height), as PIL's image.size
    return PackedImages(host, desc, src_bytes, desc_off, coef_off, coef_ints, tmp_off, size, sizes)
