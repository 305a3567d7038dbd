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

Not provided (out of scope): RandAugment, RandomDistortion / ColorJitter, GaussianBlur, RandomErasing, timm's create_transform, the
RefCOCO box transforms and BPE tokenisation."""
import numpy as np
import torch

from . import imageprep, ops


class TrainImageTransform:
    """images (uint8 [H, W, 3] arrays / tensors or PIL images) -> [B, 3, size, size] on `device`.

    min_scale: RandomResizedCrop(size, scale=(min_scale, 1.0), ratio=(3/4, 4/3), BICUBIC); with min_scale=0.9 this is the pretraining
    transform.  center_crop: Resize(size) + CenterCrop(size) (exclusive with min_scale).  Neither: Resize((size, size)).
    hflip: probability of RandomHorizontalFlip, applied last.  generator: the torch.Generator of the crop boxes and flips (None:
    torch's global one).  The random stream is torch's, not torchvision's: see imageprep.random_resized_crop_params."""

    def __init__(self, size, min_scale=None, center_crop=False, hflip=0.0, generator=None):
        imageprep.check_size(size)
        if min_scale is not None and center_crop:
            raise ValueError("TrainImageTransform: min_scale (RandomResizedCrop) and center_crop are mutually exclusive")
        if min_scale is not None and not 0.0 < min_scale <= 1.0:
            raise ValueError("TrainImageTransform: min_scale must be in (0, 1], got %r" % (min_scale,))
        if not 0.0 <= hflip <= 1.0:
            raise ValueError("TrainImageTransform: hflip is a probability, got %r" % (hflip,))
        self.size, self.min_scale, self.center_crop, self.hflip, self.generator = size, min_scale, center_crop, hflip, generator

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
        return ops.preprocess_images(images, self.size, mean, std, dtype, device, crops=crops, center_crop=self.center_crop, flips=flips)


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
