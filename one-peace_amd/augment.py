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

Not provided (out of scope): RandAugment (the reference's utils/randaugment.py is defined by OpenCV's warpAffine / filter2D), RandomErasing,
timm's create_transform, hue jitter (every use in the reference passes hue = 0), polygon targets and BPE tokenisation."""
import numpy as np
import torch

from . import imageprep, ops


class TrainImageTransform:
    """images (uint8 [H, W, 3] arrays / tensors or PIL images) -> [B, 3, size, size] on `device`.

    min_scale: RandomResizedCrop(size, scale=(min_scale, 1.0), ratio=(3/4, 4/3), BICUBIC); with min_scale=0.9 this is the pretraining
    transform.  center_crop: Resize(size) + CenterCrop(size) (exclusive with min_scale).  Neither: Resize((size, size)).
    hflip: probability of RandomHorizontalFlip, applied last.  color_jitter / blur: a ColorJitter / GaussianBlur of this module, applied
    to the resized uint8 image in that order, before the flip (the reference's Compose order); None: the step is absent.  generator: the torch.Generator of the crop boxes and flips (None:
    torch's global one).  The random stream is torch's, not torchvision's: see imageprep.random_resized_crop_params."""

    def __init__(self, size, min_scale=None, center_crop=False, hflip=0.0, generator=None, color_jitter=None, blur=None):
        imageprep.check_size(size)
        if min_scale is not None and center_crop:
            raise ValueError("TrainImageTransform: min_scale (RandomResizedCrop) and center_crop are mutually exclusive")
        if min_scale is not None and not 0.0 < min_scale <= 1.0:
            raise ValueError("TrainImageTransform: min_scale must be in (0, 1], got %r" % (min_scale,))
        if not 0.0 <= hflip <= 1.0:
            raise ValueError("TrainImageTransform: hflip is a probability, got %r" % (hflip,))
        self.size, self.min_scale, self.center_crop, self.hflip, self.generator = size, min_scale, center_crop, hflip, generator
        self.color_jitter, self.blur = color_jitter, blur

    def params(self, sizes):
        """(crops or None, flips or None) for images of the given (height, width)."""
        crops = flips = None
        if self.min_scale is not None:
            crops = [imageprep.random_resized_crop_params(h, w, scale=(self.min_scale, 1.0), generator=self.generator) for h, w in sizes]
        if self.hflip > 0.0:
            flips = (torch.rand(len(sizes), generator=self.generator) < self.hflip).tolist()
        return crops, flips

    def __call__(self, images, dtype=torch.float32, device="cpu", mean=None, std=None):
        images = list(images)
        sizes = [(im.size[1], im.size[0]) if ops._is_pil(im) else tuple(im.shape[:2]) for im in images]
        crops, flips = self.params(sizes)
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
