"""Vision-branch classifier: mirror of one_peace_vision/classification/models_vit.py (OnePeaceViT, one_piece_g_256 / _384 / _448 /
_512 -- the reference's spelling), with convert_to_vision.py:11-25, main_ft.py:285-294 and utils/lr_decay.py as functions.

The model is COMPOSED of the project's ImageAdapter, TransformerEncoder and TransformerEncoderLayer (image FFN only, sub-LN attention,
LayerNorm inside the FFN, layer scale, one shared relative-position table): no second implementation of the layer.  On bf16 device
tensors the encoder's fused HIP path runs (head_dim 64, as in the four g factories), and with ``global_pool`` the head is
``ops.token_mean_norm`` (csrc/tokenpool.hip: mean over the patch tokens + fc_norm, the gradient of the activations written once)
followed by the head's GEMM.  With ``global_pool=False`` the head reads the CLS row of the encoder's final norm in torch.

State-dict contract: ``state_dict()`` keys, ``named_parameters()`` names and ``load_state_dict`` are the REFERENCE's --
``image_adapter.{embed_images.*, cls_embedding, pos_embed, rel_pos_table.weight, rp_bucket}``, ``encoder.layers.N.*``,
``encoder.layer_norm.*`` (without global_pool), ``fc_norm.*``, ``head.*`` -- so a checkpoint of main_ft.py loads with strict=True.  The
composed modules keep three tensors under other names (rel_pos_table_list.0, image_layer_norm) and two buffers the reference does not
have (position_idx, version); hooks on this module map them both ways.  The hooks follow the module into a wrapper (a container's or
DDP's ``state_dict()`` / ``load_state_dict`` use the reference's keys under the wrapper's prefix); the ``named_parameters()`` override does
NOT: a wrapper walks the sub-modules itself and yields ``image_adapter.rel_pos_table_list.0.weight`` and ``encoder.image_layer_norm.*``,
and strict-load error messages name those too.  Build parameter groups on the bare model (``param_groups_lrd(model.module, ...)``);
``vision_param_groups`` accepts either spelling of a name without a wrapper's prefix.

Deviations, stated:
  * stochastic depth is the encoder's own draw (one Bernoulli draw for the whole stack, per sample and branch): the reference's
    distribution, not its random stream.
  * ``rp_bias=True`` (a table inside every layer) is not built: the four factories use the shared table.  NotImplementedError.
  * ``use_checkpoint=True`` turns on the encoder's own activation recompute (cfg.checkpoint_activations of the fused layers).
  * images whose side is not 16 * bucket_size go through ImageAdapter's bicubic resize of the position table.  The reference's branch
    for that case (models_vit.py:145-153) reshapes bucket^2 rows into window^2 and cannot run: no parity is claimed for it.
  * cls_embedding and pos_embed start as the reference's scaled normal draws and the head as trunc_normal_(std=.02) * init_scale;
    every Linear inside the composed modules keeps the project's initialisation (checkpoints overwrite both).  head.bias starts at
    exactly 0 (the project's Linear), where the reference has nn.Linear's uniform bias times init_scale."""
import logging
from collections import OrderedDict

import torch
import torch.nn as nn

from .. import ops
from ..adapter.image import ImageAdapter
from ..components import LayerNorm, Linear
from ..transformer.transformer_encoder import TransformerEncoder
from ..unify_model_config import AdjustEncDecConfig, ImageAdapterConfig

logger = logging.getLogger(__name__)

# (name inside the composed modules, the reference's name), both relative to this module
_RENAMES = (("image_adapter.rel_pos_table_list.0.weight", "image_adapter.rel_pos_table.weight"),
            ("encoder.image_layer_norm.", "encoder.layer_norm."))
_OWN_BUFFERS = ("image_adapter.position_idx", "encoder.version")  # buffers of the composed modules the reference does not have


def _to_reference(key):
    for own, ref in _RENAMES:
        if key.startswith(own):
            return ref + key[len(own):]
    return key


def _from_reference(key):
    for own, ref in _RENAMES:
        if key.startswith(ref):
            return own + key[len(ref):]
    return key


class OnePeaceViT(nn.Module):
    def __init__(self, activation_dropout=0.0, attention_dropout=0.0, attention_heads=24, bucket_size=16, dropout=0.0,
                 drop_path_rate=0.0, embed_dim=1536, ffn_embed_dim=6144, global_pool=True, init_scale=0.001, layers=40,
                 layer_scale_init_value=1e-2, num_classes=1000, rp_bias=False, shared_rp_bias=True, use_checkpoint=False):
        super().__init__()
        if rp_bias:
            raise NotImplementedError("OnePeaceViT: rp_bias=True (a relative-position table in every layer) is not built; the "
                                      "one_piece_g_* factories use shared_rp_bias")
        adapter_cfg = ImageAdapterConfig(bucket_size=bucket_size, rel_bucket_size=bucket_size, vision_encoder_type="hmlp", dropout=dropout,
                                         use_attn_bias=shared_rp_bias)
        cfg = AdjustEncDecConfig(
            embed_dim=embed_dim, ffn_embed_dim=ffn_embed_dim, layers=layers, attention_heads=attention_heads, normalize_before=True,
            learned_pos=True, drop_path_rate=drop_path_rate, use_text_moe=False, use_image_moe=True, use_audio_moe=False,
            attention_dropout=attention_dropout, activation_dropout=activation_dropout, dropout=dropout, magneto_scale_attn=True,
            scale_attn=False, scale_fc=True, scale_heads=False, use_layer_scale=True, layer_scale_init_value=layer_scale_init_value,
            checkpoint_activations=use_checkpoint, image_adapter=adapter_cfg)
        self.cfg = cfg
        self.image_adapter = ImageAdapter(adapter_cfg, embed_dim, attention_heads, num_layers=1)
        self.encoder = TransformerEncoder(cfg, None, use_text_norm=False, use_image_norm=not global_pool, use_audio_norm=False)
        self.global_pool = global_pool
        self.fc_norm = LayerNorm(embed_dim) if global_pool else nn.Identity()
        self.head = Linear(embed_dim, num_classes)
        with torch.no_grad():
            scale = embed_dim ** -0.5
            self.image_adapter.cls_embedding.copy_(scale * torch.randn(1, 1, embed_dim))       # models_vit.py:123-127
            self.image_adapter.pos_embed.copy_(scale * torch.randn(bucket_size ** 2 + 1, embed_dim))
            nn.init.trunc_normal_(self.head.weight, std=.02)  # timm's trunc_normal_: cut at +-2 in absolute terms (models_vit.py:412-417)
            self.head.weight.mul_(init_scale)
            self.head.bias.mul_(init_scale)
        self._register_state_dict_hook(self._reference_keys)
        self._register_load_state_dict_pre_hook(self._own_keys)

    # ---- the reference's names ------------------------------------------------------------------------------------------
    @staticmethod
    def _reference_keys(module, state_dict, prefix, local_metadata):
        """state_dict(): the reference's keys, in the composed modules' order."""
        items = list(state_dict.items())
        if not any(k.startswith(prefix) and (_to_reference(k[len(prefix):]) != k[len(prefix):] or k[len(prefix):] in _OWN_BUFFERS)
                   for k, _ in items):
            return state_dict
        state_dict.clear()
        for k, v in items:
            if k.startswith(prefix):
                rest = k[len(prefix):]
                if rest in _OWN_BUFFERS:
                    continue
                k = prefix + _to_reference(rest)
            state_dict[k] = v
        return state_dict

    def _own_keys(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys, error_msgs):
        """load_state_dict(): reference keys -> the composed modules' keys; their own two buffers are filled in."""
        for k in [k for k in state_dict if k.startswith(prefix)]:
            own = prefix + _from_reference(k[len(prefix):])
            if own != k:
                state_dict[own] = state_dict.pop(k)
        for name in _OWN_BUFFERS:
            mod, leaf = name.split(".")
            state_dict.setdefault(prefix + name, getattr(getattr(self, mod), leaf))

    def named_parameters(self, prefix="", recurse=True, remove_duplicate=True):
        for name, p in super().named_parameters(prefix=prefix, recurse=recurse, remove_duplicate=remove_duplicate):
            lead = prefix + "." if prefix else ""
            yield (lead + _to_reference(name[len(lead):]) if name.startswith(lead) else name), p

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"image_adapter.pos_embed", "image_adapter.cls_embedding"}

    # ---- forward --------------------------------------------------------------------------------------------------------
    def forward_features(self, src_images):
        """-> the encoder's output, T x B x C as in the reference (a view of the batch-major activations on the HIP path)."""
        out = self.encoder(None, self.image_adapter(src_images), None, encoder_type="image")
        return out["encoder_out"][0]

    def forward_head(self, x):
        """x: [B, S, H] (row 0 is CLS) -> logits [B, num_classes]."""
        if self.global_pool:
            x = ops.token_mean_norm(x, self.fc_norm.weight, self.fc_norm.bias, self.fc_norm.eps)
        else:
            x = x[:, 0]
        return self.head(x)

    def forward(self, src_images):
        return self.forward_head(self.forward_features(src_images).transpose(0, 1))


def one_piece_g_256(**kwargs):
    return OnePeaceViT(bucket_size=16, rp_bias=False, shared_rp_bias=True, **kwargs)


def one_piece_g_384(**kwargs):
    return OnePeaceViT(bucket_size=24, rp_bias=False, shared_rp_bias=True, **kwargs)


def one_piece_g_448(**kwargs):
    return OnePeaceViT(bucket_size=28, rp_bias=False, shared_rp_bias=True, **kwargs)


def one_piece_g_512(**kwargs):
    return OnePeaceViT(bucket_size=32, rp_bias=False, shared_rp_bias=True, **kwargs)


# --------------------------------------------------------------------------------------------------------------
# checkpoints
# --------------------------------------------------------------------------------------------------------------
_DROPPED = ("image_proj.weight", "image_proj.bias", "encoder_wrapper.fusion_model.image_layer_norm.weight",
            "encoder_wrapper.fusion_model.image_layer_norm.bias")
_OTHER_BRANCHES = ("text", "audio", "decoder", "mask", "logit_scale", "version")


def convert_to_vision(state_dict):
    """convert_to_vision.py:11-25 on a one_peace_pretrain / one_peace_retrieval state dict: the image projection and the image branch's
    final norm are dropped, every key that names another branch (text, audio, decoder, mask tokens, logit scales, version) likewise,
    ``encoder_wrapper.fusion_model.`` becomes ``encoder.`` and the adapter moves to the top level.  Returns a new dict of detached
    tensors; the argument is left as it is (the script empties its own).  No file is read or written."""
    out = OrderedDict()
    for k, v in state_dict.items():
        if k in _DROPPED or any(tag in k for tag in _OTHER_BRANCHES):
            continue
        new = k.replace("encoder_wrapper", "encoder").replace("fusion_model.", "")
        if "image_adapter" in new:
            new = new.replace("encoder.", "")
        out[new] = v.detach()
    return out


def load_pretrained(model, state_dict):
    """main_ft.py:285-294: load a converted checkpoint into `model` non-strictly.  ``image_adapter.rp_bucket`` is dropped (the model's
    own bucket matrix stands), the shared table is taken from ``image_adapter.rel_pos_table_list.0.weight`` or
    ``image_adapter.rel_pos_table.weight``, and both position tables go through ImageAdapter.upgrade_state_dict_named, which resizes
    them when the model's bucket size is larger.  Returns load_state_dict's (missing_keys, unexpected_keys) under the reference's
    names: ``fc_norm.*`` and ``head.*`` are missing by design.
    Known limit: a larger RELATIVE-position table is resampled with scipy.interpolate.interp2d, which SciPy 1.14 removed -- loading a
    16-bucket checkpoint into a 24 / 28 / 32-bucket model raises there."""
    sd = OrderedDict(state_dict)
    sd.pop("image_adapter.rp_bucket", None)
    if getattr(model.image_adapter, "rp_bucket", None) is not None:
        sd["image_adapter.rp_bucket"] = model.image_adapter.rp_bucket  # (so that it is not reported missing)
    ref_table, own_table = "image_adapter.rel_pos_table.weight", "image_adapter.rel_pos_table_list.0.weight"
    if own_table in sd:
        sd[ref_table] = sd.pop(own_table).clone()
    adapter = {k[len("image_adapter."):]: v for k, v in sd.items() if k in (ref_table, "image_adapter.pos_embed")}
    before = set(adapter)
    model.image_adapter.upgrade_state_dict_named(adapter, "")  # renames the table, resizes both, fills in what is absent
    for k in (ref_table, "image_adapter.pos_embed"):
        leaf = _from_reference(k)[len("image_adapter."):]
        if k[len("image_adapter."):] in before:
            sd[k] = adapter[leaf]
    result = model.load_state_dict(sd, strict=False)
    return [_to_reference(k) for k in result.missing_keys], list(result.unexpected_keys)


# --------------------------------------------------------------------------------------------------------------
# parameter groups (utils/lr_decay.py)
# --------------------------------------------------------------------------------------------------------------
def get_layer_id_for_vit(name, num_layers):
    """utils/lr_decay.py:63-69: the adapter is layer 0, encoder layer k is k + 1, everything else (fc_norm, head, the encoder's final
    norm) is `num_layers`."""
    if name.startswith("image_adapter"):
        return 0
    if name.startswith("encoder.layers"):
        return int(name.split(".")[2]) + 1
    return num_layers


def _layer_scales(model, layer_decay):
    num_layers = len(model.encoder.layers) + 1
    return num_layers, [layer_decay ** (num_layers - i) for i in range(num_layers + 1)]


def param_groups_lrd(model, weight_decay=0.05, no_weight_decay_list=(), layer_decay=.75):
    """utils/lr_decay.py:17-60: groups ``{lr_scale, weight_decay, params}`` in the order their first parameter appears.  Every 1-D
    parameter and every listed name goes without weight decay; layer id i trains at layer_decay ** (num_layers - i) with
    num_layers = len(encoder.layers) + 1, i.e. num_layers + 1 ids -- NOT the multimodal trainer's rule as written
    (optim.reference_param_groups: num_layers + 2 ids and the exponent num_layers + 1 - i with num_layers = len(layers): the same scale
    per encoder layer, but the adapter's relative-position table in layer 1; here it is in layer 0)."""
    num_layers, scales = _layer_scales(model, layer_decay)
    groups = OrderedDict()
    for n, p in model.named_parameters():
        if not p.requires_grad:
            continue
        decays = not (p.ndim == 1 or n in no_weight_decay_list)
        layer_id = get_layer_id_for_vit(n, num_layers) if layer_decay < 1 else 0
        name = "layer_%d_%s" % (layer_id, "decay" if decays else "no_decay")
        if name not in groups:
            groups[name] = {"lr_scale": scales[layer_id], "weight_decay": weight_decay if decays else 0., "params": []}
        groups[name]["params"].append(p)
    return list(groups.values())


def vision_param_groups(model, no_weight_decay_list=None, layer_decay=.75):
    """(no_decay(name, p), lr_scale(name, p)): the rule of param_groups_lrd as the two callables distributed.FlatParameters and
    FusedAdamW take (the counterpart of optim.reference_param_groups for this model)."""
    skip = set(model.no_weight_decay() if no_weight_decay_list is None else no_weight_decay_list)
    num_layers, scales = _layer_scales(model, layer_decay)

    def no_decay(name, p):
        return p.ndim == 1 or _to_reference(name) in skip

    def lr_scale(name, p):
        return scales[get_layer_id_for_vit(_to_reference(name), num_layers) if layer_decay < 1 else 0]
    return no_decay, lr_scale
