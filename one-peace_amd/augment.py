"""Training-time image augmentation on the device: the train / evaluation transforms of the reference's datasets and timm's Mixup /
CutMix as its image-classification collater uses it.

``TrainImageTransform`` takes a list of decoded images to the model's [B, 3, S, S] input: ``RandomResizedCrop(S, scale=(min_scale, 1.0),
BICUBIC)`` (data/pretrain_data/image_text_pretrain_dataset.py:46-53), ``Resize(S)`` + ``CenterCrop(S)``
(data/vision_data/image_classify_dataset.py:78-84) or the plain ``Resize((S, S))``, ``RandomHorizontalFlip``
(image_classify_dataset.py:59, nlvr2_dataset.py:37), ToTensor and Normalize -- all inside ops.preprocess_images, i.e. one H2D copy
and the two kernels of csrc/image.hip on a device, PIL itself on the CPU.

``Mixup`` has timm's constructor and call (image_classify_dataset.py:46-51, 117-130).  The parameters are drawn on the host
(``params``), the pixels are mixed by ops.mix_images (op_mix_images, csrc/augment.hip: one pass, in place) and the soft targets built
by ops.mix_targets; they are what ops.classify_loss takes on its soft route.

``ColorJitter`` (the reference's ``RandomDistortion``, utils/transforms.py:144-157) and ``GaussianBlur`` (utils/transforms.py:160-188) draw
the per-image tables of the photometric steps; ops.preprocess_images runs them between the resize and ToTensor (csrc/photometric.hip on
a device, PIL on the CPU).  ``GroundingTransform`` is the RefCOCO train transform with its box arithmetic
(data/vl_data/refcoco_dataset.py:31-36).

``RandAugment``, ``RandomErasing`` and ``create_transform`` are timm's, as the default image-classification train transform calls them
(data/vision_data/image_classify_dataset.py:65-77: create_transform(auto_augment='rand-m9-mstd0.5-inc1', interpolation='bicubic',
re_prob=0.25, re_mode='pixel', re_count=1)): RandomResizedCrop, RandomHorizontalFlip, RandAugment on the uint8 image, ToTensor, Normalize,
RandomErasing.  The procedure is restated from timm's auto_augment.py, random_erasing.py and transforms_factory.py; timm is not a
dependency of this project, so parity is claimed with the Pillow calls those files make (which the tests check byte for byte), not with
an installed timm, and the random stream is torch's.

Not provided (out of scope): the reference's own RandomAugment (utils/randaugment.py, defined by OpenCV's warpAffine / filter2D; NLVR2 and
raw_transform stay complete up to it), RandAugment's BILINEAR / NEAREST / random resampling, weighted op choice (`w`), `mmax`, the
non-increasing op set, AugMix / AutoAugment policies, more than one erased box per image, hue jitter (every use in the reference passes
hue = 0), polygon targets and BPE tokenisation."""
import math
import re

import numpy as np
import torch

from . import imageprep, ops


class TrainImageTransform:
    """images (uint8 [H, W, 3] arrays / tensors or PIL images) -> [B, 3, size, size] on `device`.

    min_scale: RandomResizedCrop(size, scale=(min_scale, 1.0), ratio=(3/4, 4/3), BICUBIC), or a (lo, hi) pair for scale=(lo, hi); with
    min_scale=0.9 this is the pretraining transform.  center_crop: Resize(size) + CenterCrop(size) (exclusive with min_scale).  Neither: Resize((size, size)).
    hflip: probability of RandomHorizontalFlip, applied last.  color_jitter / blur: a ColorJitter / GaussianBlur of this module, applied
    to the resized uint8 image in that order, before the flip (the reference's Compose order); None: the step is absent.  generator: the torch.Generator of the crop boxes and flips (None:
    torch's global one).  The random stream is torch's, not torchvision's: see imageprep.random_resized_crop_params.
    rand_augment: a RandAugment of this module, applied AFTER the flip (timm's create_transform order); exclusive with color_jitter / blur."""

    def __init__(self, size, min_scale=None, center_crop=False, hflip=0.0, generator=None, color_jitter=None, blur=None, rand_augment=None):
        imageprep.check_size(size)
        if min_scale is not None and center_crop:
            raise ValueError("TrainImageTransform: min_scale (RandomResizedCrop) and center_crop are mutually exclusive")
        self.scale = None
        if min_scale is not None:
            self.scale = (float(min_scale), 1.0) if isinstance(min_scale, (int, float)) else tuple(float(v) for v in min_scale)
            if len(self.scale) != 2 or not 0.0 < self.scale[0] <= self.scale[1] <= 1.0:
                raise ValueError("TrainImageTransform: min_scale must be in (0, 1] or a pair 0 < lo <= hi <= 1, got %r" % (min_scale,))
        if not 0.0 <= hflip <= 1.0:
            raise ValueError("TrainImageTransform: hflip is a probability, got %r" % (hflip,))
        if rand_augment is not None and (color_jitter is not None or blur is not None):
            raise ValueError("TrainImageTransform: rand_augment excludes color_jitter and blur (the flip sits on the other side of them)")
        self.size, self.min_scale, self.center_crop, self.hflip, self.generator = size, min_scale, center_crop, hflip, generator
        self.color_jitter, self.blur, self.rand_augment = color_jitter, blur, rand_augment

    def params(self, sizes):
        """(crops or None, flips or None) for images of the given (height, width)."""
        crops = flips = None
        if self.min_scale is not None:
            crops = [imageprep.random_resized_crop_params(h, w, scale=self.scale, generator=self.generator) for h, w in sizes]
        if self.hflip > 0.0:
            flips = (torch.rand(len(sizes), generator=self.generator) < self.hflip).tolist()
        return crops, flips

    def __call__(self, images, dtype=torch.float32, device="cpu", mean=None, std=None):
        images = list(images)
        sizes = [(im.size[1], im.size[0]) if ops._is_pil(im) else tuple(im.shape[:2]) for im in images]
        crops, flips = self.params(sizes)
        if self.rand_augment is not None:
            return ops.preprocess_images(images, self.size, mean, std, dtype, device, crops=crops, center_crop=self.center_crop, flips=flips,
                                         randaug=self.rand_augment.params(len(images), self.size))
        if self.color_jitter is None and self.blur is None:
            return ops.preprocess_images(images, self.size, mean, std, dtype, device, crops=crops, center_crop=self.center_crop, flips=flips)
        jitter = None if self.color_jitter is None else self.color_jitter.params(len(images))
        blur = None if self.blur is None else self.blur.params(len(images))
        return ops.preprocess_images(images, self.size, mean, std, dtype, device, crops=crops, center_crop=self.center_crop, flips=flips,
                                     jitter=jitter, blur=blur)


def _jitter_range(value, name):
    """torchvision's ColorJitter._check_input for brightness / contrast / saturation: a number v >= 0 is [max(0, 1 - v), 1 + v], a pair is
    taken as it is; None when the range is [1, 1] (the op is skipped)."""
    if isinstance(value, (int, float)):
        if value < 0:
            raise ValueError("ColorJitter: %s must be non-negative, got %r" % (name, value))
        lo, hi = max(0.0, 1.0 - float(value)), 1.0 + float(value)
    else:
        lo, hi = (float(v) for v in value)
        if not 0.0 <= lo <= hi or hi == float("inf"):
            raise ValueError("ColorJitter: %s range must be 0 <= min <= max < inf, got %r" % (name, value))
    return None if lo == hi == 1.0 else (lo, hi)


class ColorJitter:
    """torchvision's ColorJitter(brightness, contrast, saturation) applied with probability `prob`: the reference's
    RandomDistortion(b, c, s, 0, prob) (utils/transforms.py:144-157) is ColorJitter(b, c, s, prob=prob); NLVR2 and the raw_transform of the
    image classification use RandomDistortion(0.4, 0.4, 0.4, 0, 0.5) = ColorJitter(0.4, 0.4, 0.4, prob=0.5).

    Per image: a permutation of (brightness, contrast, saturation, hue) gives the order of the ops, each factor is uniform in
    [max(0, 1 - v), 1 + v]; an op whose v is 0 is skipped.  hue != 0 raises NotImplementedError (not provided; the reference passes 0).
    The draws use torch's random stream (`generator`); it is NOT claimed equal to torchvision's, only the procedure is restated."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0, prob=1.0, generator=None):
        if (hue != 0) if isinstance(hue, (int, float)) else (tuple(hue) != (0, 0)):
            raise NotImplementedError("ColorJitter: hue jitter is not provided (every use in the reference passes hue = 0)")
        if not 0.0 <= prob <= 1.0:
            raise ValueError("ColorJitter: prob is a probability, got %r" % (prob,))
        self.ranges = {1: _jitter_range(brightness, "brightness"), 2: _jitter_range(contrast, "contrast"),
                       3: _jitter_range(saturation, "saturation")}
        self.prob, self.generator = prob, generator

    def params(self, B):
        """(ops int32 [B, 3], factors float32 [B, 3]): the tables of ops.color_jitter / ops.preprocess_images(jitter = ...)."""
        chains = []
        for _ in range(B):
            chain = []
            if float(torch.rand(1, generator=self.generator)) < self.prob:
                for fn in torch.randperm(4, generator=self.generator).tolist():  # 0 brightness, 1 contrast, 2 saturation, 3 hue
                    rng = self.ranges.get(fn + 1)
                    if rng is not None:
                        chain.append((fn + 1, float(torch.empty(1).uniform_(rng[0], rng[1], generator=self.generator))))
            chains.append(chain)
        return imageprep.jitter_table(chains)


class GaussianBlur:
    """The reference's GaussianBlur(p, radius_min, radius_max) (utils/transforms.py:160-188): with a draw u ~ U[0, 1), the image is blurred
    when u <= p, by ImageFilter.GaussianBlur(radius ~ U(radius_min, radius_max)).  torch's random stream (`generator`)."""

    def __init__(self, p=0.5, radius_min=0.1, radius_max=2.0, generator=None):
        if not 0.0 <= p <= 1.0:
            raise ValueError("GaussianBlur: p is a probability, got %r" % (p,))
        if not 0.0 < radius_min <= radius_max:
            raise ValueError("GaussianBlur: need 0 < radius_min <= radius_max, got %r, %r" % (radius_min, radius_max))
        imageprep.gaussian_box_params(radius_max)  # (a ValueError when the device kernel cannot take the largest radius)
        self.prob, self.radius_min, self.radius_max, self.generator = p, radius_min, radius_max, generator

    def params(self, B):
        """One entry per image: the radius, or None for an image that is not blurred (ops.gaussian_blur's `radii`)."""
        radii = []
        for _ in range(B):
            do_it = float(torch.rand(1, generator=self.generator)) <= self.prob
            radii.append(float(torch.empty(1).uniform_(self.radius_min, self.radius_max, generator=self.generator)) if do_it else None)
        return radii


# timm's _RAND_INCREASING_TRANSFORMS, in its order
RAND_INCREASING_OPS = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness",
                       "Sharpness", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
_SIGNED_OPS = ("Rotate", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel", "Color", "Contrast", "Brightness", "Sharpness")


class RandAugment:
    """timm's RandAugment over its increasing op set (timm/data/auto_augment.py: rand_augment_transform('rand-m9-mstd0.5-inc1')), as the
    reference's image classification uses it.  ``params(B, size)`` draws the (ops, args, fill) tables of ops.rand_augment /
    ops.preprocess_images(randaug=) for B images of size x size.

    Per image and layer: an op drawn uniformly, with replacement, from RAND_INCREASING_OPS; skipped (op 0) when a uniform draw exceeds
    `prob`; the magnitude m = clamp(gauss(magnitude, mstd), 0, 10) (mstd >= 100: uniform in [0, magnitude]; mstd = 0: m = magnitude), mapped
    to the op's argument:
      Rotate +- m / 10 * 30 degrees; ShearX / ShearY +- m / 10 * 0.3; TranslateXRel / YRel +- m / 10 * translate_pct * size pixels;
      Color / Contrast / Brightness / Sharpness max(0.1, 1 +- m / 10 * 0.9); Posterize bits = 4 - int(m / 10 * 4);
      Solarize thresh = 256 - int(m / 10 * 256); SolarizeAdd add = min(128, int(m / 10 * 110)); the signs flipped with probability 0.5.
    The geometric ops resample with BICUBIC and fill with fill = min(255, round(255 mean)) per channel.  increasing=False (timm's
    non-increasing forms), weighted choice and magnitude_max are not provided (NotImplementedError).  The draws use torch's random stream
    (`generator`); it is NOT claimed equal to timm's, only the procedure is restated."""

    def __init__(self, magnitude=9, num_layers=2, mstd=0.5, prob=0.5, increasing=True, translate_pct=0.45, mean=imageprep.CLIP_MEAN,
                 generator=None):
        if not increasing:
            raise NotImplementedError("RandAugment: only the increasing op set ('inc1') is provided")
        if not (math.isfinite(magnitude) and 0 <= magnitude):
            raise ValueError("RandAugment: magnitude must be finite and >= 0, got %r" % (magnitude,))
        if int(num_layers) != num_layers or num_layers < 1:
            raise ValueError("RandAugment: num_layers must be an integer >= 1, got %r" % (num_layers,))
        if not 0.0 <= prob <= 1.0:
            raise ValueError("RandAugment: prob is a probability, got %r" % (prob,))
        if not mstd >= 0:
            raise ValueError("RandAugment: mstd must be >= 0, got %r" % (mstd,))
        self.magnitude, self.num_layers, self.mstd, self.prob = float(magnitude), int(num_layers), float(mstd), float(prob)
        self.translate_pct, self.generator = float(translate_pct), generator
        self.fill = tuple(min(255, round(255 * x)) for x in mean)
        if len(self.fill) != 3 or min(self.fill) < 0:
            raise ValueError("RandAugment: mean must be three values in [0, 1], got %r" % (mean,))

    @classmethod
    def from_config(cls, config, **kwargs):
        """RandAugment from timm's config string, e.g. 'rand-m9-mstd0.5-inc1': sections m (magnitude), n (layers), mstd, p (probability),
        inc (increasing set).  w (weighted choice) and mmax raise NotImplementedError; anything else is a ValueError."""
        parts = str(config).split("-")
        if parts[0] != "rand":
            raise ValueError("RandAugment.from_config: %r does not start with 'rand'" % (config,))
        for part in parts[1:]:
            m = re.fullmatch(r"([a-z]+)(\d+(?:\.\d*)?|\.\d+)", part)
            if m is None:
                raise ValueError("RandAugment.from_config: cannot parse section %r of %r" % (part, config))
            key, val = m.group(1), m.group(2)
            if key in ("w", "mmax"):
                raise NotImplementedError("RandAugment.from_config: section %r (%s) is not provided" % (
                    part, "weighted op choice" if key == "w" else "magnitude_max"))
            if key == "m":
                kwargs["magnitude"] = float(val)
            elif key == "n":
                kwargs["num_layers"] = int(val)
            elif key == "mstd":
                kwargs["mstd"] = float(val)
            elif key == "p":
                kwargs["prob"] = float(val)
            elif key == "inc":
                kwargs["increasing"] = bool(int(val))
            else:
                raise ValueError("RandAugment.from_config: unknown section %r of %r" % (part, config))
        return cls(**kwargs)

    def _level(self, name, m, negate, size):
        """(the name imageprep.randaug_table knows, its value) of op `name` at magnitude m."""
        sign = -1.0 if negate else 1.0
        if name == "Rotate":
            return "Rotate", sign * (m / 10.0) * 30.0
        if name in ("ShearX", "ShearY"):
            return name, sign * (m / 10.0) * 0.3
        if name in ("TranslateXRel", "TranslateYRel"):
            return name[:-3], sign * (m / 10.0) * self.translate_pct * size
        if name in ("Color", "Contrast", "Brightness", "Sharpness"):
            return name, max(0.1, 1.0 + sign * (m / 10.0) * 0.9)
        if name == "Posterize":
            return name, max(0, 4 - int((m / 10.0) * 4))
        if name == "Solarize":
            return name, max(0, 256 - int((m / 10.0) * 256))
        if name == "SolarizeAdd":
            return name, min(128, int((m / 10.0) * 110))
        return name, None

    def draw(self, B, size):
        """The drawn layers as lists: per image `num_layers` entries, None (skipped) or (name, value) / (name,)."""
        g = self.generator
        out = []
        for _ in range(B):
            layers = []
            for _ in range(self.num_layers):
                name = RAND_INCREASING_OPS[int(torch.randint(0, len(RAND_INCREASING_OPS), (1,), generator=g))]
                if float(torch.rand(1, generator=g)) > self.prob:
                    layers.append(None)
                    continue
                if self.mstd >= 100.0:
                    m = float(torch.rand(1, generator=g)) * self.magnitude
                elif self.mstd > 0.0:
                    m = self.magnitude + self.mstd * float(torch.randn(1, generator=g))
                else:
                    m = self.magnitude
                m = max(0.0, min(m, 10.0))
                negate = name in _SIGNED_OPS and float(torch.rand(1, generator=g)) > 0.5
                name, value = self._level(name, m, negate, size)
                layers.append((name,) if value is None else (name, value))
            out.append(layers)
        return out

    def params(self, B, size):
        """(ops int32 [B, num_layers], args fp64 [B, num_layers, 6], fill): the tables of ops.rand_augment for B images of size x size."""
        rows = [[("none",) if la is None else la for la in layers] for layers in self.draw(B, size)]
        tab_ops, tab_args = imageprep.randaug_table(rows, size)
        if tab_ops.shape[1] != self.num_layers:  # (B == 0)
            tab_ops, tab_args = np.zeros((B, self.num_layers), np.int32), np.zeros((B, self.num_layers, 6), np.float64)
        return tab_ops, tab_args, self.fill


class RandomErasing:
    """timm's RandomErasing (timm/data/random_erasing.py) on a normalised batch x [B, 3, H, W], in place, one box per image.

    Per image: skipped when a uniform draw exceeds `probability`; else up to 10 attempts of target = U(min_area, max_area) * H W / count,
    aspect = exp(U(log min_aspect, log max_aspect)), h = int(round(sqrt(target * aspect))), w = int(round(sqrt(target / aspect))), the
    first with w < W and h < H placed at top = randint(0, H - h), left = randint(0, W - w), both ends included.  max_aspect defaults to
    1 / min_aspect.  mode 'pixel': one normal value per erased element; 'rand': one per channel; 'const': zeros.  The noise is drawn in fp32
    with torch.randn, for the erased areas only -- on x's device, or with `generator` on the generator's device -- and cast to x's dtype
    by the store (ops.erase_images: op_image_erase on a device).  min_count = max_count = 1 only (the reference's re_count=1); other
    counts raise NotImplementedError.  torch's random stream, not timm's."""

    def __init__(self, probability=0.25, min_area=0.02, max_area=1 / 3, min_aspect=0.3, max_aspect=None, mode="pixel", min_count=1,
                 max_count=None, generator=None):
        if not 0.0 <= probability <= 1.0:
            raise ValueError("RandomErasing: probability is a probability, got %r" % (probability,))
        if not 0.0 < min_area <= max_area <= 1.0:
            raise ValueError("RandomErasing: need 0 < min_area <= max_area <= 1, got %r, %r" % (min_area, max_area))
        if not min_aspect > 0.0:
            raise ValueError("RandomErasing: min_aspect must be > 0, got %r" % (min_aspect,))
        max_aspect = max_aspect or 1.0 / min_aspect
        if not min_aspect <= max_aspect:
            raise ValueError("RandomErasing: need 0 < min_aspect <= max_aspect, got %r, %r" % (min_aspect, max_aspect))
        mode = mode.lower()
        if mode not in ("pixel", "const", "rand"):
            raise ValueError("RandomErasing: mode must be 'pixel', 'const' or 'rand', got %r" % (mode,))
        max_count = max_count or min_count
        if (min_count, max_count) != (1, 1):
            raise NotImplementedError("RandomErasing: one box per image only (min_count = max_count = 1)")
        self.probability, self.min_area, self.max_area, self.mode, self.generator = probability, min_area, max_area, mode, generator
        self.log_aspect = (math.log(min_aspect), math.log(max_aspect))
        self.min_aspect, self.max_aspect, self.count = min_aspect, max_aspect, 1

    def params(self, B, H, W):
        """int32 [B, 4]: (top, left, h, w) per image; h = 0 for an image that is not erased."""
        g = self.generator
        uniform = lambda lo, hi: float(torch.empty(1).uniform_(lo, hi, generator=g)) if lo < hi else float(lo)
        boxes = np.zeros((B, 4), dtype=np.int32)
        for i in range(B):
            if float(torch.rand(1, generator=g)) > self.probability:
                continue
            for _ in range(10):
                target = uniform(self.min_area, self.max_area) * (H * W) / self.count
                aspect = math.exp(uniform(*self.log_aspect))
                h, w = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
                if w < W and h < H:
                    top = int(torch.randint(0, H - h + 1, (1,), generator=g))
                    left = int(torch.randint(0, W - w + 1, (1,), generator=g))
                    if h > 0 and w > 0:  # (an empty box erases nothing)
                        boxes[i] = (top, left, h, w)
                    break
        return boxes

    def noise(self, boxes, device):
        """The packed fp32 noise of ops.erase_images for `boxes` on `device`: 3 h w values per erased image."""
        g = self.generator
        draw_on = device if g is None else g.device
        sizes = [(int(h), int(w)) for _, _, h, w in boxes if h > 0]
        total = sum(3 * h * w for h, w in sizes)
        if self.mode == "const":
            return torch.zeros(total, dtype=torch.float32, device=device)
        if self.mode == "pixel":
            return torch.randn(total, dtype=torch.float32, device=draw_on, generator=g).to(device)
        per_channel = torch.randn(len(sizes), 3, dtype=torch.float32, device=draw_on, generator=g).to(device)
        parts = [per_channel[k].view(3, 1).expand(3, h * w).reshape(-1) for k, (h, w) in enumerate(sizes)]
        return torch.cat(parts) if parts else torch.zeros(0, dtype=torch.float32, device=device)

    def __call__(self, x):
        B, _, H, W = x.shape
        boxes = self.params(B, H, W)
        return ops.erase_images(x, boxes, self.noise(boxes, x.device))


class _CreatedTransform:
    """What create_transform returns: (images, dtype, device) -> [B, 3, S, S].  image_transform: the TrainImageTransform (crop, flip,
    ColorJitter or RandAugment, ToTensor, Normalize); erasing: the RandomErasing behind it, or None."""

    def __init__(self, image_transform, erasing, mean, std):
        self.image_transform, self.erasing, self.mean, self.std = image_transform, erasing, mean, std

    def __call__(self, images, dtype=torch.float32, device="cpu"):
        x = self.image_transform(images, dtype=dtype, device=device, mean=self.mean, std=self.std)
        return x if self.erasing is None else self.erasing(x)


def create_transform(input_size, is_training=True, color_jitter=0.4, auto_augment=None, interpolation="bicubic", re_prob=0.0, re_mode="const",
                     re_count=1, mean=imageprep.CLIP_MEAN, std=imageprep.CLIP_STD, scale=(0.08, 1.0), hflip=0.5, generator=None):
    """timm.data.create_transform (timm/data/transforms_factory.py) for batches: a callable (images, dtype, device) -> [B, 3, S, S].
    The reference's default image-classification train transform (image_classify_dataset.py:65-77) is
    create_transform(S, True, color_jitter, 'rand-m9-mstd0.5-inc1', 'bicubic', re_prob=0.25, re_mode='pixel', re_count=1).

    is_training: RandomResizedCrop(S, scale, ratio=(3/4, 4/3)), RandomHorizontalFlip(hflip), then RandAugment.from_config(auto_augment)
    -- or, without auto_augment, ColorJitter(c, c, c) for color_jitter = c (a triple gives the three strengths; None or 0: none; timm drops
    the jitter when auto_augment is set) -- ToTensor, Normalize(mean, std) and, for re_prob > 0, RandomErasing(re_prob, mode=re_mode,
    max_count=re_count).  not is_training: the project's evaluation transform, Resize(S) + CenterCrop(S), ToTensor, Normalize.
    ValueError: an interpolation other than 'bicubic' (the device kernels resample with BICUBIC only).  NotImplementedError: an
    auto_augment policy that is not 'rand-...' (AugMix / AutoAugment).  All draws come from `generator` (torch's stream, not timm's)."""
    if interpolation != "bicubic":
        raise ValueError("create_transform: interpolation must be 'bicubic', got %r" % (interpolation,))
    size = input_size[-1] if isinstance(input_size, (tuple, list)) else input_size
    if isinstance(input_size, (tuple, list)) and input_size[-1] != input_size[-2]:
        raise ValueError("create_transform: input_size must be square, got %r" % (input_size,))
    mean, std = tuple(mean), tuple(std)
    if not is_training:
        return _CreatedTransform(TrainImageTransform(size, center_crop=True), None, mean, std)
    rand_augment = jitter = None
    if auto_augment:
        if not str(auto_augment).startswith("rand"):
            raise NotImplementedError("create_transform: auto_augment %r: only RandAugment ('rand-...') is provided" % (auto_augment,))
        rand_augment = RandAugment.from_config(auto_augment, mean=mean, generator=generator)
    elif color_jitter is not None:
        cj = (float(color_jitter),) * 3 if isinstance(color_jitter, (int, float)) else tuple(color_jitter)
        if len(cj) != 3:
            raise ValueError("create_transform: color_jitter must be a number or three (hue is not provided), got %r" % (color_jitter,))
        if any(cj):
            jitter = ColorJitter(*cj, generator=generator)
    transform = TrainImageTransform(size, min_scale=tuple(scale), hflip=hflip, generator=generator, color_jitter=jitter, rand_augment=rand_augment)
    erasing = RandomErasing(re_prob, mode=re_mode, max_count=re_count, generator=generator) if re_prob > 0.0 else None
    return _CreatedTransform(transform, erasing, mean, std)


class GroundingTransform:
    """The RefCOCO train transform (data/vl_data/refcoco_dataset.py:31-36): RandomResize([size], max_size=size), GaussianBlur, ToTensor and
    Normalize(max_image_size=size) with the box arithmetic of utils/transforms.py (resize: 53-60, Normalize: 113-116).

    The resize is always to (size, size): get_size_with_aspect_ratio(image_size, size, max_size=size) puts the shorter side at `size` and
    the longer at int(size * long / short) >= size, then clips both to max_size = size (``resized_size``; the early exit for a shorter
    side that already equals `size` clips the same way).  So the aspect ratio is not kept and the ratios are rw = float(size) / float(w),
    rh = float(size) / float(h).  Boxes (x0, y0, x1, y1 in pixels) become boxes * fp32[rw, rh, rw, rh] / size, in torch's fp32 arithmetic
    as the reference runs it; target["size"] = [size, size].  blur: a GaussianBlur of this module or None.  Polygons are not handled (the
    dataset never passes them)."""

    def __init__(self, size, blur=None):
        imageprep.check_size(size)
        self.size, self.blur = size, blur

    @staticmethod
    def resized_size(w, h, size, max_size=None):
        """(oh, ow) of the reference's get_size_with_aspect_ratio((w, h), size, max_size), restated."""
        if (w <= h and w == size) or (h <= w and h == size):
            if max_size is not None:
                h, w = min(h, int(max_size)), min(w, int(max_size))
            return h, w
        if w < h:
            ow, oh = size, int(size * h / w)
        else:
            oh, ow = size, int(size * w / h)
        if max_size is not None:
            oh, ow = min(oh, int(max_size)), min(ow, int(max_size))
        return oh, ow

    def boxes(self, boxes, w, h):
        """fp32 boxes of a w x h image after the resize to (size, size) and Normalize's division by max_image_size = size."""
        ratio_width, ratio_height = float(self.size) / float(w), float(self.size) / float(h)
        scaled = torch.as_tensor(boxes, dtype=torch.float32) * torch.as_tensor([ratio_width, ratio_height, ratio_width, ratio_height])
        return scaled / self.size

    def __call__(self, images, boxes, dtype=torch.float32, device="cpu", mean=None, std=None):
        """(x [B, 3, size, size] on `device`, targets): boxes[i] = the [n_i, 4] (or [4]) boxes of image i in pixels; targets[i] =
        {"boxes": fp32 of the same shape on the CPU, "size": tensor([size, size])}."""
        images = list(images)
        if len(boxes) != len(images):
            raise ValueError("GroundingTransform: need the boxes of every image, got %d for %d images" % (len(boxes), len(images)))
        sizes = [(im.size[1], im.size[0]) if ops._is_pil(im) else tuple(im.shape[:2]) for im in images]
        targets = [{"boxes": self.boxes(b, w, h), "size": torch.tensor([self.size, self.size])} for b, (h, w) in zip(boxes, sizes)]
        blur = None if self.blur is None else self.blur.params(len(images))
        return ops.preprocess_images(images, self.size, mean, std, dtype, device, blur=blur), targets


class Mixup:
    """timm's Mixup (timm/data/mixup.py) with its constructor and ``__call__(x, target) -> (x, soft_target)``, the even-batch assertion
    included; x [B, C, H, W] is mixed IN PLACE with the flipped batch (sample i with sample B - 1 - i).

    mode 'batch': one lambda ~ Beta(alpha, alpha) for the batch, applied with probability `prob`; CutMix instead of Mixup with
    probability `switch_prob` when both alphas are > 0.  'elem': the same per sample.  'pair': B / 2 draws, mirrored over the batch.
    CutMix box: r = sqrt(1 - lambda), cut = int(H r), int(W r), centre randint(0, H), randint(0, W), edges clip(c -+ cut // 2, 0, size);
    with cutmix_minmax: cut = randint(int(size min), int(size max)), origin randint(0, size - cut).  lambda becomes
    1 - area / (H W) when correct_lam is set or cutmix_minmax is used.

    How lambda reaches fp32 (it decides the last bit of every mixed pixel, and is what timm's own arithmetic does): 'batch' keeps a
    Python double, so the kernel gets lam = fl32(lambda) and one_minus_lam = fl32(1 - lambda); 'elem' and 'pair' keep a float32
    lambda, so lam = lambda32 and one_minus_lam = fl32(1 - lambda32).  The draws use np.random as timm's do, but timm is not a
    dependency of this project: the random stream is NOT claimed equal to timm's, only the formulas are restated and tested."""

    def __init__(self, mixup_alpha=1.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode="batch", correct_lam=True,
                 label_smoothing=0.1, num_classes=1000):
        self.mixup_alpha, self.cutmix_alpha, self.cutmix_minmax = mixup_alpha, cutmix_alpha, cutmix_minmax
        if cutmix_minmax is not None:
            assert len(cutmix_minmax) == 2
            self.cutmix_alpha = 1.0  # (timm: force cutmix alpha == 1.0 when minmax active to keep logic simple & safe)
        if mode not in ("batch", "elem", "pair"):
            raise ValueError("Mixup: mode must be 'batch', 'elem' or 'pair', got %r" % (mode,))
        self.mix_prob, self.switch_prob, self.mode, self.correct_lam = prob, switch_prob, mode, correct_lam
        self.label_smoothing, self.num_classes = label_smoothing, num_classes
        self.mixup_enabled = True

    # ---- the CutMix box ------------------------------------------------------------------------------------------
    def cutmix_box(self, H, W, lam, center=None):
        """((yl, yh, xl, xh), lambda) of timm's cutmix_bbox_and_lam for an H x W image.  center = (cy, cx) fixes the centre of the
        normal case (tests); None draws it."""
        if self.cutmix_minmax is not None:
            lo, hi = self.cutmix_minmax
            cut_h = int(np.random.randint(int(H * lo), int(H * hi)))
            cut_w = int(np.random.randint(int(W * lo), int(W * hi)))
            yl = int(np.random.randint(0, H - cut_h))
            xl = int(np.random.randint(0, W - cut_w))
            yh, xh = yl + cut_h, xl + cut_w
        else:
            ratio = np.sqrt(1 - lam)
            cut_h, cut_w = int(H * ratio), int(W * ratio)
            cy, cx = (int(np.random.randint(0, H)), int(np.random.randint(0, W))) if center is None else center
            yl, yh = int(np.clip(cy - cut_h // 2, 0, H)), int(np.clip(cy + cut_h // 2, 0, H))
            xl, xh = int(np.clip(cx - cut_w // 2, 0, W)), int(np.clip(cx + cut_w // 2, 0, W))
        if self.correct_lam or self.cutmix_minmax is not None:
            lam = 1.0 - (yh - yl) * (xh - xl) / float(H * W)
        return (yl, yh, xl, xh), lam

    # ---- draws ---------------------------------------------------------------------------------------------------
    def _draw_elem(self, n):
        lam = np.ones(n, dtype=np.float32)
        use_cutmix = np.zeros(n, dtype=bool)
        if self.mixup_enabled:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = np.random.rand(n) < self.switch_prob
                lam_mix = np.where(use_cutmix, np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n),
                                   np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n))
            elif self.mixup_alpha > 0.0:
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha, size=n)
            elif self.cutmix_alpha > 0.0:
                use_cutmix = np.ones(n, dtype=bool)
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha, size=n)
            else:
                raise ValueError("One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true.")
            lam = np.where(np.random.rand(n) < self.mix_prob, lam_mix.astype(np.float32), lam)
        return lam, use_cutmix

    def _draw_batch(self):
        lam, use_cutmix = 1.0, False
        if self.mixup_enabled and np.random.rand() < self.mix_prob:
            if self.mixup_alpha > 0.0 and self.cutmix_alpha > 0.0:
                use_cutmix = bool(np.random.rand() < self.switch_prob)
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha) if use_cutmix else np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.mixup_alpha > 0.0:
                lam_mix = np.random.beta(self.mixup_alpha, self.mixup_alpha)
            elif self.cutmix_alpha > 0.0:
                use_cutmix = True
                lam_mix = np.random.beta(self.cutmix_alpha, self.cutmix_alpha)
            else:
                raise ValueError("One of mixup_alpha > 0., cutmix_alpha > 0., cutmix_minmax not None should be true.")
            lam = float(lam_mix)
        return lam, use_cutmix

    def _draw(self, B, H, W):
        """(the four tables, the lambda of the soft targets: a Python float in 'batch' mode, float32 [B] otherwise)."""
        kind = np.zeros(B, dtype=np.int32)
        lam_t = np.ones(B, dtype=np.float32)
        oml_t = np.zeros(B, dtype=np.float32)
        box = np.zeros((B, 4), dtype=np.int32)
        if self.mode == "batch":
            lam, use_cutmix = self._draw_batch()
            if lam != 1.0:
                if use_cutmix:
                    b, lam = self.cutmix_box(H, W, lam)
                    kind[:], box[:] = 2, b
                else:
                    kind[:] = 1
                lam_t[:], oml_t[:] = np.float32(lam), np.float32(1.0 - lam)  # a double until here: fl32(lambda), fl32(1 - lambda)
            return (kind, lam_t, oml_t, box), lam
        n = B if self.mode == "elem" else B // 2
        lam_n, use_cutmix = self._draw_elem(n)
        for i in range(n):
            lam = lam_n[i]
            if lam != 1.0:
                if use_cutmix[i]:
                    b, lam = self.cutmix_box(H, W, lam)
                    kind[i], box[i] = 2, b
                    lam_n[i] = lam  # (float32 again)
                else:
                    kind[i] = 1
        lam_t[:n] = lam_n
        if self.mode == "pair":  # the partner B - 1 - i gets sample i's draw
            kind[B - n:], box[B - n:], lam_t[B - n:] = kind[:n][::-1], box[:n][::-1], lam_n[::-1]
        oml_t[:] = np.float32(1.0) - lam_t  # float32 arithmetic: fl32(1 - lambda32)
        return (kind, lam_t, oml_t, box), lam_t.copy()

    def params(self, B, H, W):
        """One draw for a batch of B images of H x W: kind int32 [B] (0 copy, 1 Mixup, 2 CutMix), lam fp32 [B], one_minus_lam fp32 [B]
        and box int32 [B, 4] (yl, yh, xl, xh), numpy arrays on the host -- the tables of ops.mix_images.  Where kind is 0, lam is 1."""
        return self._draw(B, H, W)[0]

    @staticmethod
    def pad_even(x, target):
        """An odd batch gets its sample 0 appended, as the reference's collater does (image_classify_dataset.py:122-126)."""
        if len(x) % 2 != 0:
            x, target = torch.cat([x, x[:1]], dim=0), torch.cat([target, target[:1]], dim=0)
        return x, target

    def __call__(self, x, target):
        assert len(x) % 2 == 0, "Batch size should be even when using this"
        B, _, H, W = x.shape
        tables, lam = self._draw(B, H, W)
        x = ops.mix_images(x, tables, inplace=True)
        return x, ops.mix_targets(target, self.num_classes, lam, self.label_smoothing)
