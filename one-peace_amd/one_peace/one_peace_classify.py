"""Fine-tuning model (registry name ``one_peace_classify``): the shared encoder under a classification head.

API parity target: one_peace/models/one_peace/one_peace_classify.py:49-207 -- the constructor ``(cfg, src_dict, head_type,
num_classes, use_two_images)``, ``build_model(cfg, task)``, ``forward(src_tokens, src_images, src_images_2, src_audios,
audio_padding_masks)`` returning the logits, the text -> image -> audio precedence of the pooled stream with ``use_image_features``,
``freeze_finetune_updates`` with ``set_num_updates``, the same parameter names (``encoder_wrapper.*``, ``classify_head.*``) and the same
checkpoint upgrade rules.  Every shipped fine-tuning script (vqa, nlvr2, visual grounding, vggsound, fsd50k, aqa, image classification)
builds this model with ``attn_pooling: true``; the head's pooling is ops.attention_pool (csrc/attnpool.hip)."""
import contextlib
import logging
from dataclasses import dataclass
from typing import Optional

import torch

from ..registry import register_model
from ..unify_model_config import UnifyModelConfig
from .one_peace_base import ModelWrapper, OnePeaceBaseModel, OnePeaceClassifyHead, init_one_peace_params

logger = logging.getLogger(__name__)

_HEAD_USES = {"text": ("text",), "image": ("image",), "audio": ("audio",), "vl": ("text", "image"), "al": ("text", "audio")}
_MODALITIES = ("text", "image", "audio")


@dataclass
class OnePeaceClassifyConfig(UnifyModelConfig):
    head_scale_ratio: int = 1
    use_pooler: bool = False
    pooler_dropout: float = 0.0
    attn_pooling: bool = False
    use_image_features: bool = False
    freeze_finetune_updates: int = 0


@register_model("one_peace_classify", dataclass=OnePeaceClassifyConfig)
class OnePeaceClassifyModel(OnePeaceBaseModel):
    def __init__(self, cfg, src_dict, head_type, num_classes=None, use_two_images=False):
        super().__init__(cfg, src_dict)
        if head_type not in _HEAD_USES:
            raise NotImplementedError("one_peace_classify: head_type %r (one of %s)" % (head_type, ", ".join(_HEAD_USES)))
        enc = cfg.encoder
        self.head_type = head_type
        self.classify_head = OnePeaceClassifyHead(
            attn_pooling=cfg.attn_pooling, use_pooler=cfg.use_pooler, pooler_dropout=cfg.pooler_dropout, input_dim=enc.embed_dim,
            num_heads=enc.attention_heads, head_scale_ratio=cfg.head_scale_ratio, num_classes=num_classes, use_two_images=use_two_images)
        used = _HEAD_USES[head_type]
        for m in _MODALITIES:
            setattr(enc, "use_%s_moe" % m, m in used)
        self.encoder_wrapper = ModelWrapper(enc, src_dict, use_text_norm="text" in used, use_image_norm="image" in used,
                                            use_audio_norm="audio" in used, num_layers=enc.layers)
        self.apply(init_one_peace_params)
        # (the reference wraps every layer in fsdp_wrap(checkpoint_wrapper(...)) here; the fused HIP layer implements both activation
        # policies itself, see one_peace_retrieval.py)

    @classmethod
    def build_model(cls, cfg, task):
        cfg.encoder.image_adapter.rel_bucket_size = task.cfg.patch_image_size // 16
        return cls(cfg, task.source_dictionary, head_type=task.cfg.head_type, num_classes=task.cfg.num_classes,
                   use_two_images=task.cfg.use_two_images)

    def set_num_updates(self, num_updates):
        super().set_num_updates(num_updates)
        self.num_updates = num_updates

    def forward(self, src_tokens: Optional[torch.Tensor] = None, src_images: Optional[torch.Tensor] = None,
                src_images_2: Optional[torch.Tensor] = None, src_audios: Optional[torch.Tensor] = None,
                audio_padding_masks: Optional[torch.Tensor] = None):
        encoder_type = self.head_type
        # the encoder trains once freeze_finetune_updates updates have passed (always, when no trainer ever set the count)
        ft = self.cfg.freeze_finetune_updates <= self.num_updates if hasattr(self, "num_updates") else True
        with torch.no_grad() if not ft else contextlib.ExitStack():
            text, image, audio, text_pad, image_pad, audio_pad = self.encoder_wrapper(
                src_tokens=src_tokens, src_images=src_images, src_audios=src_audios, audio_padding_masks=audio_padding_masks,
                encoder_type=encoder_type, return_padding_mask=True)
        text_2 = image_2 = audio_2 = None
        if src_images_2 is not None:  # (as the reference: outside the no_grad block, with the padding mask the first pass returned)
            text_2, image_2, audio_2 = self.encoder_wrapper(
                src_tokens=src_tokens, src_images=src_images_2, is_second_image=True, src_audios=src_audios,
                audio_padding_masks=audio_pad, encoder_type=encoder_type)
        if text is not None and not self.cfg.use_image_features:
            return self.classify_head(text, text_2, text_pad)
        if image is not None:
            return self.classify_head(image, image_2, image_pad)
        if audio is not None:
            return self.classify_head(audio, audio_2, audio_pad)
        raise NotImplementedError

    # ---- checkpoints ------------------------------------------------------------------------------------------------
    def upgrade_state_dict_named(self, state_dict, name):
        super().upgrade_state_dict_named(state_dict, name)
        self.remove_pretraining_modules(state_dict)
        prefix = name + "." if name != "" else ""
        for key, value in self.state_dict().items():
            if prefix + key not in state_dict:  # the head of a pretraining checkpoint: freshly initialised
                logger.info("%s not exists, re-initialized", prefix + key)
                state_dict[prefix + key] = value

    def remove_pretraining_modules(self, state_dict):
        """one_peace_classify.py:178-207: the final norms this model does not have, the contrastive projections, and every entry of
        a tower the head type does not use."""
        own = self.state_dict()
        for m in _MODALITIES:
            for leaf in ("weight", "bias"):
                key = "encoder_wrapper.fusion_model.%s_layer_norm.%s" % (m, leaf)
                if key not in own:
                    state_dict.pop(key, None)
                state_dict.pop("%s_proj.%s" % (m, leaf), None)
        unused = [m + "_" for m in _MODALITIES if m not in _HEAD_USES[self.head_type]]
        for key in [k for k in state_dict if any(tag in k for tag in unused)]:
            del state_dict[key]
