"""Host side of the hub's image transform (one_peace/models/one_peace/hub_interface.py:94-101): ``Resize((S, S), BICUBIC)``
on a PIL RGB image, ``ToTensor``, ``Normalize(CLIP mean / std)`` (data/base_dataset.py:23-24).

The resize is Pillow's ``Image.resize((S, S), Image.BICUBIC)`` for 8-bit images (src/libImaging/Resample.c): a horizontal pass
over the source rows the vertical filter reads, a uint8 intermediate, then the vertical pass, both with 22-bit fixed-point
weights.  ``bicubic_coeffs`` restates Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` so that the device kernel
(csrc/image.hip, op_image_resize_normalize) reproduces PIL bit for bit; ``pack_images`` stages the images and the tables for one
host-to-device copy.  ``apply_coeffs`` is the same arithmetic in torch, the CPU reference of the tests only.

The training and evaluation geometry rides on the same two passes (no second resize kernel): ``RandomResizedCrop`` (reference
data/pretrain_data/image_text_pretrain_dataset.py:46-53; boxes from ``random_resized_crop_params``) is the tables of the box with
shifted column starts, ``Resize(S)`` + ``CenterCrop(S)`` (data/vision_data/image_classify_dataset.py:78-84) a window of the tables of
the aspect-preserving resize, and ``RandomHorizontalFlip`` (image_classify_dataset.py:59, nlvr2_dataset.py:37) a per-image flag the
vertical kernel honours when it stores (op_image_resize_normalize_flip).  ``apply_packed`` evaluates a packed batch's tables on the CPU."""
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
    records int32, then (with `flips`) one uint8 flag per image at `flip_off`.  A record is [xmin, taps, 0, 0, w_0 ... w_{k-1}] with k
    a multiple of 4 (zero-padded), S records per axis and image.  `desc` is the host copy of the table; `workspace_bytes` the size of the
    uint8 intermediates (rows x S x 3 bytes per image, S x W x 3 for an image whose vertical pass goes first).  With a crop or a centre
    crop an "image" of the table is the part of the source that was packed (pack_images); `sizes` are those of the whole images."""

    def __init__(self, host, desc, src_bytes, desc_off, coef_off, coef_count, workspace_bytes, size, sizes, flip_off=None):
        self.host, self.desc, self.size, self.sizes = host, desc, size, sizes
        self.src_bytes, self.desc_off, self.coef_off, self.coef_count = src_bytes, desc_off, coef_off, coef_count
        self.workspace_bytes, self.flip_off = workspace_bytes, flip_off

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


def check_crops(crops, sizes):
    """The boxes of `crops` as int tuples (top, left, h, w) -- torchvision's F.resized_crop order -- one per (height, width) of
    `sizes`; a box outside its image or with h or w < 1 is a ValueError."""
    crops = [tuple(int(v) for v in c) for c in crops]
    if len(crops) != len(sizes) or any(len(c) != 4 for c in crops):
        raise ValueError("crops: need one (top, left, h, w) per image, got %d for %d images" % (len(crops), len(sizes)))
    for i, ((top, left, h, w), (H, W)) in enumerate(zip(crops, sizes)):
        if h < 1 or w < 1 or top < 0 or left < 0 or top + h > H or left + w > W:
            raise ValueError("crops: box %d (top %d, left %d, h %d, w %d) is empty or outside its %d x %d image" % (i, top, left, h, w, H, W))
    return crops


def check_flips(flips, count):
    flips = [bool(f) for f in (flips.tolist() if hasattr(flips, "tolist") else flips)]
    if len(flips) != count:
        raise ValueError("flips: need one flag per image, got %d for %d images" % (len(flips), count))
    return flips


def center_crop_geometry(H, W, size):
    """(new_h, new_w, top, left) of torchvision's Resize(size) + CenterCrop(size) on an H x W image: the shorter side goes to `size`, the
    longer to int(size * long / short), and the size x size window starts at int(round((n - size) / 2.0)) of each resized side."""
    if W <= H:
        new_w, new_h = size, int(size * H / W)
    else:
        new_h, new_w = size, int(size * W / H)
    return new_h, new_w, int(round((new_h - size) / 2.0)), int(round((new_w - size) / 2.0))


def _window(coeffs, first, size):
    return tuple(c[first:first + size] for c in coeffs)


def _geometry(a, size, crop, center_crop):
    """(part of `a` to pack, column table, row table, vertical_first) of one image.  The tables index the packed part.
    crop (top, left, h, w): PIL's crop(box).resize((S, S)) is the two passes over the box's rows with the tables of a w x h image, the
    column starts shifted by `left`; a box whose vertical pass goes first (vertical_first of the BOX) is packed as its own narrow image.
    center_crop: Resize(S) + CenterCrop(S) is the S-record window of the tables of the H x W -> new_h x new_w resize, over the source
    rows that window reads; PIL decides the order of the passes from the whole image and the un-windowed target."""
    H, W = a.shape[:2]
    if crop is not None:
        top, left, h, w = crop
        cx, cy = bicubic_coeffs(w, size), bicubic_coeffs(h, size)
        if vertical_first(h, w, size):
            return np.ascontiguousarray(a[top:top + h, left:left + w]), cx, cy, True
        return a[top:top + h], (cx[0] + np.int32(left), cx[1], cx[2]), cy, False
    if center_crop:
        new_h, new_w, oy, ox = center_crop_geometry(H, W, size)
        cx, cy = _window(bicubic_coeffs(W, new_w), ox, size), _window(bicubic_coeffs(H, new_h), oy, size)
        if vertical_first(H, W, new_h):
            return a, cx, cy, True
        r0, r1 = int(cy[0][0]), int(cy[0][-1] + cy[1][-1])
        return a[r0:r1], cx, (cy[0] - np.int32(r0), cy[1], cy[2]), False
    return a, bicubic_coeffs(W, size), bicubic_coeffs(H, size), vertical_first(H, W, size)


def pack_images(images, size, pin=True, crops=None, center_crop=False, flips=None):
    """PackedImages of uint8 HWC RGB arrays / tensors (H, W >= 1) for an S x S resize.  crops: one (top, left, h, w) per image, the
    resize of that box (torchvision's resized_crop); center_crop: torchvision's Resize(S) + CenterCrop(S), exclusive with crops;
    flips: one bool per image, staged behind the tables for the device (the flip itself is the kernel's)."""
    check_size(size)
    arrs = [as_rgb_array(im) for im in images]
    B = len(arrs)
    if crops is not None and center_crop:
        raise ValueError("pack_images: crops and center_crop are mutually exclusive")
    if crops is not None:
        crops = check_crops(crops, [a.shape[:2] for a in arrs])
    if flips is not None:
        flips = check_flips(flips, B)
    sizes = [(int(a.shape[1]), int(a.shape[0])) for a in arrs]  # (width, height), as PIL's image.size
    desc = np.zeros((B, DESC_FIELDS), dtype=np.int64)
    blocks, src_off, coef_ints, tmp_off = [], 0, 0, 0
    for i in range(B):
        a, cx, cy, vfirst = _geometry(arrs[i], size, None if crops is None else crops[i], center_crop)
        arrs[i] = a
        H, W = a.shape[:2]
        if max(np.abs(cx[2]).max(), np.abs(cy[2]).max()) >= 1 << 23:  # the kernel multiplies on the 24-bit multiplier
            raise ValueError("pack_images: a filter weight of %d x %d -> %d does not fit 24 bits" % (H, W, size))
        rx, kx = _record_block(cx, size)
        ry, ky = _record_block(cy, size)
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
    flip_off = None
    if flips is not None:
        flip_off = _align(total)
        total = flip_off + _align(B)
    host = torch.empty(total, dtype=torch.uint8, pin_memory=pin)
    buf = host.numpy()
    for i, a in enumerate(arrs):
        o = int(desc[i, 0])
        buf[o:o + a.size] = a.reshape(-1)
        buf[o + a.size:_align(o + a.size)] = 0  # alignment gaps and the slack are read (under zero weights): keep them defined
    buf[src_off:src_bytes] = 0
    buf[desc_off:desc_off + desc.nbytes] = desc.view(np.uint8).reshape(-1)
    buf[desc_off + desc.nbytes:coef_off] = 0
    if blocks:
        buf[coef_off:coef_off + coef_ints * 4] = np.concatenate(blocks).view(np.uint8)
    if flips is not None:
        buf[coef_off + coef_ints * 4:] = 0
        buf[flip_off:flip_off + B] = np.asarray(flips, dtype=np.uint8)
    return PackedImages(host, desc, src_bytes, desc_off, coef_off, coef_ints, tmp_off, size, sizes, flip_off)


def apply_packed(packed):
    """uint8 [B, S, S, 3]: the tables of a PackedImages batch evaluated on its packed pixels with `_pass`, in the order of the two
    kernels (horizontal pass over rows row0 ... row0 + rows, then the vertical pass; the other order for vfirst), flipped where the
    staged flag says so.  The CPU restatement of op_image_resize_normalize_flip that the tests pin to PIL."""
    S, buf = packed.size, packed.host.numpy()
    coef = buf[packed.coef_off:packed.coef_off + packed.coef_count * 4].view(np.int32)
    out = torch.empty(len(packed), S, S, 3, dtype=torch.uint8)
    for i, (src_off, H, W, cx_off, kx, cy_off, ky, _, row0, rows, vfirst) in enumerate(packed.desc.tolist()):
        img = torch.from_numpy(buf[src_off:src_off + H * W * 3].reshape(H, W, 3).astype(np.int64))
        rx = coef[cx_off:cx_off + S * (4 + kx)].reshape(S, 4 + kx)
        ry = coef[cy_off:cy_off + S * (4 + ky)].reshape(S, 4 + ky)
        cx, cy = (rx[:, 0], rx[:, 1], rx[:, 4:]), (ry[:, 0], ry[:, 1], ry[:, 4:])
        if vfirst:
            res = _pass(_pass(img, cy, 0), cx, 1)
        else:
            res = _pass(_pass(img[row0:row0 + rows], cx, 1), (cy[0] - row0, cy[1], cy[2]), 0)
        if packed.flip_off is not None and buf[packed.flip_off + i]:
            res = res.flip(1)
        out[i] = res.to(torch.uint8)
    return out


# ---- photometric train transforms: the host-side tables of op_image_color_jitter / op_image_gaussian_blur (csrc/photometric.hip) ----
JITTER_OPS = {"none": 0, "brightness": 1, "contrast": 2, "saturation": 3}  # op codes of the ops table (include/onepeace_hip.h)
MAX_BOX_RADIUS = 32  # op_image_gaussian_blur: integer box radius R <= 32 (GaussianBlur radii up to ~33)


def jitter_table(chains):
    """(ops int32 [B, 3], factors float32 [B, 3]) from one chain per image: None / () for an untouched image, else up to three
    (op, factor) pairs in the order they are applied, op a name or code of JITTER_OPS.  Unused slots are (0, 1.0).  ValueError: an unknown
    op, more than three ops or more than one contrast op in an image (torchvision's ColorJitter applies each at most once), a factor that
    is negative or not finite."""
    chains = list(chains)
    ops = np.zeros((len(chains), 3), dtype=np.int32)
    factors = np.ones((len(chains), 3), dtype=np.float32)
    for i, chain in enumerate(chains):
        chain = [] if chain is None else list(chain)
        if len(chain) > 3:
            raise ValueError("jitter_table: image %d has %d ops, at most 3" % (i, len(chain)))
        for k, (op, f) in enumerate(chain):
            code = JITTER_OPS.get(op) if isinstance(op, str) else (int(op) if int(op) in JITTER_OPS.values() else None)
            if code is None:
                raise ValueError("jitter_table: image %d: unknown op %r (need one of %s or 0 ... 3)" % (i, op, sorted(JITTER_OPS)))
            f = float(f)
            if not math.isfinite(f) or f < 0.0 or f > float(np.finfo(np.float32).max):  # (finite as fp32, too)
                raise ValueError("jitter_table: image %d: factor %r must be finite and >= 0" % (i, f))
            ops[i, k], factors[i, k] = code, f
        if int((ops[i] == JITTER_OPS["contrast"]).sum()) > 1:
            raise ValueError("jitter_table: image %d has more than one contrast op" % i)
    return ops, factors


def check_jitter(jitter, count):
    """The (ops, factors) tables of `count` images as (int32 [count, 3], float32 [count, 3]), validated as jitter_table validates."""
    ops, factors = jitter
    ops = np.asarray(ops.cpu() if torch.is_tensor(ops) else ops)
    factors = np.asarray(factors.cpu() if torch.is_tensor(factors) else factors)
    if ops.size != 3 * count or factors.size != 3 * count:
        raise ValueError("jitter: need ops and factors of [%d, 3], got %s and %s" % (count, ops.shape, factors.shape))
    ops, factors = ops.reshape(count, 3), factors.reshape(count, 3)
    return jitter_table([list(zip(o.tolist(), f.tolist())) for o, f in zip(ops, factors)])


def gaussian_box_params(radius):
    """(R, ww, fw) of the three extended box blurs per axis that PIL's ImageFilter.GaussianBlur(radius) runs (src/libImaging/BoxBlur.c):
    with C-float s2 = fl32(fl32(r r) / 3), then in doubles L = sqrt(12 s2 + 1), l = floor((L - 1) / 2),
    a = (2 l + 1)(l (l + 1) - 3 s2) / (6 (s2 - (l + 1)^2)) and fr = fl32(l + a); a line pass uses R = (int)fr, ww = (uint32)(2^24 / (2 fr + 1))
    in fp32 and fw = (2^24 - (2 R + 1) ww) / 2.  ValueError: a radius that is not positive and finite, or R > MAX_BOX_RADIUS."""
    r = float(radius)
    if not math.isfinite(r) or r <= 0.0:
        raise ValueError("gaussian_box_params: radius must be positive and finite, got %r" % (radius,))
    r = np.float32(r)
    s2 = float(np.float32(np.float32(r * r) / np.float32(3)))
    L = math.sqrt(12.0 * s2 + 1.0)
    l = math.floor((L - 1.0) / 2.0)
    a = (2 * l + 1) * (l * (l + 1) - 3 * s2) / (6 * (s2 - (l + 1) * (l + 1)))
    fr = np.float32(l + a)
    R = int(fr)
    if R > MAX_BOX_RADIUS:
        raise ValueError("gaussian_box_params: radius %r gives a box radius of %d, at most %d" % (radius, R, MAX_BOX_RADIUS))
    ww = int(np.float32(1 << 24) / np.float32(np.float32(2) * fr + np.float32(1)))
    fw = ((1 << 24) - (2 * R + 1) * ww) // 2
    return R, ww, fw


def blur_table(radii):
    """(R int32 [B], ww uint32 [B], fw uint32 [B], on uint8 [B]) from one radius per image; None or a radius <= 0 means not blurred."""
    radii = list(radii.tolist() if hasattr(radii, "tolist") else radii)
    B = len(radii)
    R, ww, fw, on = np.zeros(B, np.int32), np.zeros(B, np.uint32), np.zeros(B, np.uint32), np.zeros(B, np.uint8)
    for i, r in enumerate(radii):
        if r is None:
            continue
        if math.isnan(float(r)):
            raise ValueError("blur_table: radius %d is NaN" % i)
        if r > 0:
            R[i], ww[i], fw[i] = gaussian_box_params(r)
            on[i] = 1
    return R, ww, fw, on


# ---- RandAugment: the host-side tables of op_image_randaug_layer (csrc/randaugment.hip) ----
# Op codes of a layer's table (include/onepeace_hip.h).  7 ... 9 are ImageEnhance blends: ops.rand_augment hands them to op_image_color_jitter.
RANDAUG_OPS = {"none": 0, "AutoContrast": 1, "Equalize": 2, "Invert": 3, "Posterize": 4, "Solarize": 5, "SolarizeAdd": 6, "Color": 7,
               "Contrast": 8, "Brightness": 9, "Sharpness": 10, "Affine": 11}
RANDAUG_TO_JITTER = {7: JITTER_OPS["saturation"], 8: JITTER_OPS["contrast"], 9: JITTER_OPS["brightness"]}
AFFINE_NAMES = ("Rotate", "ShearX", "ShearY", "TranslateX", "TranslateY")


def affine_coeffs(name, value, size):
    """The six coefficients of PIL's Image.transform(AFFINE) for timm's geometric RandAugment ops on a size x size image, or None for the
    identity: ShearX (1, v, 0, 0, 1, 0), ShearY (1, 0, 0, v, 1, 0), TranslateX (1, 0, v, 0, 1, 0) and TranslateY (1, 0, 0, 0, 1, v) with v
    in pixels, and Rotate by `value` degrees with Image.rotate's matrix about (size / 2, size / 2): the angle taken modulo 360, cosine and
    sine rounded to 15 decimals, the translation evaluated as PIL evaluates it.  angle % 360 == 0 is the identity (PIL copies the image);
    the other multiples of 90 are a ValueError: there PIL transposes instead of resampling.  ValueError: an unknown name, a value that is
    not finite."""
    v = float(value)
    if name not in AFFINE_NAMES:
        raise ValueError("affine_coeffs: unknown op %r (need one of %s)" % (name, ", ".join(AFFINE_NAMES)))
    if not math.isfinite(v):
        raise ValueError("affine_coeffs: %s: the value must be finite, got %r" % (name, value))
    if name == "ShearX":
        return (1.0, v, 0.0, 0.0, 1.0, 0.0)
    if name == "ShearY":
        return (1.0, 0.0, 0.0, v, 1.0, 0.0)
    if name == "TranslateX":
        return (1.0, 0.0, v, 0.0, 1.0, 0.0)
    if name == "TranslateY":
        return (1.0, 0.0, 0.0, 0.0, 1.0, v)
    angle = v % 360.0
    if angle == 0:
        return None
    if angle in (90, 180, 270):
        raise ValueError("affine_coeffs: Rotate by %r degrees is a transpose in PIL, not a resampling (not provided)" % (value,))
    cx = cy = size / 2
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return tuple(m)


def _randaug_row(i, name, vals, size):
    """(code, the six fp64 arguments) of one op of image i."""
    zero = (0.0,) * 6
    if name in AFFINE_NAMES:
        if len(vals) != 1:
            raise ValueError("randaug_table: image %d: %s takes one value" % (i, name))
        if size is None:
            raise ValueError("randaug_table: image %d: %s needs the image size" % (i, name))
        co = affine_coeffs(name, vals[0], size)
        return (0, zero) if co is None else (RANDAUG_OPS["Affine"], co)
    code = RANDAUG_OPS.get(name) if isinstance(name, str) else (int(name) if int(name) in RANDAUG_OPS.values() else None)
    if code is None:
        raise ValueError("randaug_table: image %d: unknown op %r (need one of %s, %s or a code 0 ... 11)" % (
            i, name, ", ".join(sorted(RANDAUG_OPS)), ", ".join(AFFINE_NAMES)))
    want = 6 if code == 11 else (0 if code <= 3 else 1)
    if len(vals) != want and not (want == 0 and len(vals) == 6):
        raise ValueError("randaug_table: image %d: op %r takes %d value(s), got %d" % (i, name, want, len(vals)))
    vals = tuple(float(v) for v in vals)
    if not all(math.isfinite(v) for v in vals):
        raise ValueError("randaug_table: image %d: op %r has an argument that is not finite" % (i, name))
    if code in (4, 5, 6):
        lo, hi = {4: (0, None), 5: (0, 256), 6: (0, 255)}[code]
        v = vals[0]
        if v != math.floor(v) or v < lo or (hi is not None and v > hi):
            raise ValueError("randaug_table: image %d: op %r: %r is not an integer in its range" % (i, name, v))
        if code == 4 and v >= 8:  # timm's posterize returns the image for bits >= 8
            return 0, zero
    if code in (7, 8, 9, 10) and (vals[0] < 0.0 or vals[0] > float(np.finfo(np.float32).max)):
        raise ValueError("randaug_table: image %d: op %r: the factor %r must be >= 0 (and finite as fp32)" % (i, name, vals[0]))
    if code <= 3:
        return code, zero
    return code, (vals + zero)[:6]


def randaug_table(layers_per_image, size=None):
    """(ops int32 [B, L], args fp64 [B, L, 6]) from one list of ops per image, in the order they are applied, e.g.
    [("ShearX", 0.21), ("Equalize",)]: a name of RANDAUG_OPS with its argument (Posterize bits, Solarize thresh, SolarizeAdd add, the factor
    of Color / Contrast / Brightness / Sharpness, the six coefficients of Affine), or Rotate (degrees), ShearX / ShearY, TranslateX / TranslateY
    (pixels), which become Affine through affine_coeffs (they need `size`).  L = the longest list (at least 1); missing layers are op 0.
    Posterize with bits >= 8 and Rotate by a multiple of 360 are op 0.  ValueError: an unknown name, a wrong number of arguments, an argument
    that is not finite, bits / thresh / add not an integer in 0 ... / 0 ... 256 / 0 ... 255, a negative factor, Rotate by 90, 180 or 270."""
    layers = [[] if la is None else list(la) for la in layers_per_image]
    L = max([1] + [len(la) for la in layers])
    ops = np.zeros((len(layers), L), dtype=np.int32)
    args = np.zeros((len(layers), L, 6), dtype=np.float64)
    for i, la in enumerate(layers):
        for k, item in enumerate(la):
            item = tuple(item) if isinstance(item, (tuple, list)) else (item,)
            if not item:
                raise ValueError("randaug_table: image %d: an empty op" % i)
            vals = item[1:]
            if len(vals) == 1 and isinstance(vals[0], (tuple, list, np.ndarray)):
                vals = tuple(vals[0])
            ops[i, k], args[i, k] = _randaug_row(i, item[0], vals, size)
    return ops, args


def check_randaug(randaug, count):
    """The (ops, args, fill) of `count` images as (int32 [count, L], fp64 [count, L, 6], three ints 0 ... 255), validated as randaug_table
    validates op codes and arguments."""
    if len(randaug) != 3:
        raise ValueError("randaug: need (ops, args, fill)")
    ops, args, fill = randaug
    ops = np.asarray(ops.cpu() if torch.is_tensor(ops) else ops)
    args = np.asarray(args.cpu() if torch.is_tensor(args) else args, dtype=np.float64)
    if ops.ndim == 1:
        ops = ops.reshape(-1, 1)
    if ops.ndim != 2 or ops.shape[0] != count or args.size != ops.size * 6:
        raise ValueError("randaug: need ops [%d, L] and args [%d, L, 6], got %s and %s" % (count, count, ops.shape, args.shape))
    args = args.reshape(ops.shape + (6,))
    fill = tuple(fill)
    if len(fill) != 3 or any(int(v) != v or not 0 <= v <= 255 for v in fill):
        raise ValueError("randaug: fill must be three integers in 0 ... 255, got %r" % (fill,))
    fill = tuple(int(v) for v in fill)
    if ops.size == 0:
        return np.zeros(ops.shape, np.int32), np.zeros(ops.shape + (6,), np.float64), fill
    if (ops != ops.astype(np.int64)).any():
        raise ValueError("randaug: op codes must be integers")
    rows = [[(int(o),) + ((tuple(a.tolist()),) if int(o) == 11 else (() if 0 <= int(o) <= 3 else (float(a[0]),))) for o, a in zip(orow, arow)]
            for orow, arow in zip(ops, args)]
    tab_ops, tab_args = randaug_table(rows)
    return tab_ops, tab_args, fill


def random_resized_crop_params(height, width, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    """(top, left, h, w) of torchvision's RandomResizedCrop.get_params for a height x width image, restated with torch's RNG
    (`generator`): up to 10 tries of area * U(scale), exp(U(log ratio)), w = int(round(sqrt(a r))), h = int(round(sqrt(a / r))), the
    first with 0 < w <= width and 0 < h <= height placed at randint(0, height - h + 1), randint(0, width - w + 1); else the central
    crop whose aspect is clamped into `ratio`.  torchvision is not a dependency of this project: the ALGORITHM and the pixel path of
    the boxes are checked by the tests, equality of the random stream with torchvision's is NOT checked."""
    if height < 1 or width < 1:
        raise ValueError("random_resized_crop_params: need height, width >= 1, got %d x %d" % (height, width))
    area = height * width
    log_ratio = (math.log(ratio[0]), math.log(ratio[1]))

    def uniform(lo, hi):
        return float(torch.empty(1).uniform_(lo, hi, generator=generator))

    def randint(n):
        return int(torch.randint(0, n, (1,), generator=generator))

    for _ in range(10):
        target_area = area * uniform(scale[0], scale[1])
        aspect = math.exp(uniform(log_ratio[0], log_ratio[1]))
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= width and 0 < h <= height:
            return randint(height - h + 1), randint(width - w + 1), h, w
    in_ratio = float(width) / float(height)
    if in_ratio < min(ratio):
        w = width
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = height
        w = int(round(h * max(ratio)))
    else:
        w, h = width, height
    return (height - h) // 2, (width - w) // 2, h, w
