"""Video branch (action recognition): mirror of one_peace_vision/video/mmaction_custom/models/backbones/onepeace.py -- Adapter (:21-39),
the layer with its three bottleneck adapters and the temporal pass through the SAME attention weights (:254-352), ImageAdaptor's
temporal embedding (:198-201), the backbone OnePeaceViT (:423-691, here OnePeaceVideoViT) -- with the checkpoint loading of :526-609 +
:630 and the freezing rule of video/train.py:187-190 as functions.

The layer SUBCLASSES the project's TransformerEncoderLayer (same parameters under the reference's names: self_attn.*,
self_attn_layer_norm, image_ffn.{0.wi_0, 0.wi_1, 2, 3}, final_layer_norm, gamma_1, gamma_2) and adds T_Adapter, S_Adapter, MLP_Adapter
(and T_Adapter_in with num_tadapter == 2); the adapter subclasses ImageAdapter.  Activations stay in the project's batch-major rows
[B * T, N, D] (frame-major inside a video) all the way: every op of the temporal path but the attention core is row-wise, and the core
(ops.temporal_attention over csrc/frameattn.hip) reads the packed q|k|v rows where they lie, so the reference's two rearranges of the
whole activation matrix per layer (:331, :337) do not exist here.

The fused route runs on bf16 device tensors when head_dim is 64, num_frames <= 32, attention and activation dropout are inactive and
dropout is inactive or the model is in eval mode: LayerNorms through ops.layer_norm, q|k|v as one packed GEMM (ops.packed_qkv), the
temporal core through ops.temporal_attention, the spatial core through ops.spatial_attention (the project's attention kernels with the
shared relative-position handle), adapters through ops.linear with GELU in between, the GeGLU term through ops.ffn_branch.  Otherwise
the same statements run as torch ops.  ``use_checkpoint`` wraps each layer in torch.utils.checkpoint (non-reentrant).

State-dict contract: ``state_dict()`` keys and ``load_state_dict`` are the REFERENCE's -- ``image_adapter.{embed_images.*,
cls_embedding, pos_embed, temporal_embedding, rel_pos_table.weight, rp_bucket}``, ``encoder.layers.N.*``,
``encoder.image_layer_norm.*`` -- through the hook technique of models_vit.py: the composed ImageAdapter keeps the table as
rel_pos_table_list.0 and owns one buffer the reference does not have (position_idx).  As there, ``named_parameters()`` of the bare model
yields the reference's names; a wrapper's does not.

Deviations, stated:
  * stochastic depth is drawn per frame (the reference's batch axis is b * t), three independent draws per layer (temporal term,
    gamma_1 term, MLP_Adapter term) as in :338, :344, :350: the reference's distribution, not its random stream.
  * ``rp_bias=True`` (a table inside every layer) is not built.  NotImplementedError, as in models_vit.py.
  * the temporal core keeps scores and probabilities in fp32 (include/onepeace_hip.h); the reference's bf16 run rounds them.
  * the fused spatial core (ops.spatial_attention) takes the relative-position bias as a CONSTANT: the reference's fine-tuning state
    freezes the table (freeze_for_adapters).  While the table requires a gradient, that one product (scores + bias, softmax, values) of
    each layer runs as torch ops on the packed q|k|v rows and the table's gradient comes from autograd; everything else stays fused.
  * the encoder is this module's own small container (layers + image_layer_norm): it has no ``version`` buffer.
  * every Linear keeps the project's initialisation until init_weights() (trunc_normal_ std .02, zero biases, unit LayerNorms, zero
    D_fc2 of every adapter, :611-665); ``pretrained`` file loading (:621-634, a pickle) is not mirrored: load_pretrained takes a state
    dict and reads no file.
  * VideoRecognizer states what the reference's config binds (Recognizer3D + I3DHead with spatial_type='avg', dropout_ratio=0.5,
    average_clips='prob'): mmaction itself is not mirrored."""
import logging
from collections import OrderedDict

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint

from .. import ops
from ..adapter.image import ImageAdapter
from ..components import LayerNorm, Linear
from ..transformer.transformer_layer import TransformerEncoderLayer
from ..unify_model_config import AdjustEncDecConfig, ImageAdapterConfig

logger = logging.getLogger(__name__)

_RENAMES = (("image_adapter.rel_pos_table_list.0.weight", "image_adapter.rel_pos_table.weight"),)
_OWN_BUFFERS = ("image_adapter.position_idx",)  # a buffer of the composed adapter the reference does not have
_TRAINABLE_TAGS = ("temporal_embedding", "image_layer_norm", "cls_head", "Adapter")  # video/train.py:189


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


def _drop_path_rows(x, drop_prob, training):
    """onepeace.py:61-77 on batch-major rows: one draw per frame (the reference's batch axis b * t).  x: [B * T, N, D]."""
    if drop_prob == 0.0 or not training:
        return x
    keep = 1.0 - drop_prob
    mask = torch.empty(x.shape[0], 1, 1, dtype=x.dtype, device=x.device).bernoulli_(keep)
    return x.div(keep) * mask


class Adapter(nn.Module):
    """onepeace.py:21-39: D_fc1, GELU, D_fc2, optional skip connection."""

    def __init__(self, D_features, mlp_ratio=0.25, skip_connect=True):
        super().__init__()
        self.skip_connect = skip_connect
        self.act = nn.GELU()
        self.D_fc1 = Linear(D_features, int(D_features * mlp_ratio))
        self.D_fc2 = Linear(int(D_features * mlp_ratio), D_features)

    def forward(self, x):
        xs = self.D_fc2(self.act(self.D_fc1(x)))
        return x + xs if self.skip_connect else xs


class VideoEncoderLayer(TransformerEncoderLayer):
    """onepeace.py:254-352 on batch-major rows x [B * T, N, D]."""

    def __init__(self, cfg, drop_path_rate=0.0, num_tadapter=1, num_frames=8, scale=1.0):
        super().__init__(cfg, drop_path_rate)
        self.MLP_Adapter = Adapter(self.embed_dim, skip_connect=False)
        self.S_Adapter = Adapter(self.embed_dim)
        self.scale = scale
        self.T_Adapter = Adapter(self.embed_dim, skip_connect=False)
        if num_tadapter == 2:
            self.T_Adapter_in = Adapter(self.embed_dim)
        self.num_tadapter, self.num_frames = num_tadapter, num_frames

    def video_fused_supported(self):
        a = self.self_attn
        return (a.head_dim == 64 and self.num_frames <= 32 and a.c_attn is None and self.attn_ln is None
                and not (self.training and (a.dropout_p > 0.0 or float(self.cfg.activation_dropout) > 0.0 or self.dropout_prob > 0.0)))

    # ---- the attention module, temporal (bias None, sequences over t) or spatial (sequences over n) --------------------------------
    def _attend_torch(self, h, temporal, bias):
        a = self.self_attn
        BT, N, D = h.shape
        T = self.num_frames
        B, heads, hd = BT // T, a.num_heads, a.head_dim
        qkv = torch.cat([a.q_proj(h), a.k_proj(h), a.v_proj(h)], dim=-1).reshape(BT * N, 3 * D)
        drop = self.training and a.dropout_p > 0.0
        if temporal and not drop:
            core = ops.temporal_attention(qkv, B, T, N, heads, a.scaling)
        else:
            x = qkv.view(B, T, N, 3, heads, hd)
            x = x.permute(3, 0, 2, 4, 1, 5) if temporal else x.permute(3, 0, 1, 4, 2, 5)  # [3, B, N | T, heads, T | N, hd]
            q, k, v = x.unbind(0)
            w = torch.matmul(q * a.scaling, k.transpose(-1, -2))
            if bias is not None:
                w = w + bias
            p = a.dropout_module(F.softmax(w, dim=-1, dtype=torch.promote_types(w.dtype, torch.float32)).to(w.dtype))
            core = torch.matmul(p, v)
            core = core.permute(0, 3, 1, 2, 4) if temporal else core.permute(0, 1, 3, 2, 4)  # -> [B, T, N, heads, hd]
            core = core.reshape(BT * N, D)
        return a.out_proj(a.ln(core) if a.ln is not None else core).view(BT, N, D)

    def _attend_fused(self, h2, temporal, bias, BT, N):
        a = self.self_attn
        qkv = ops.packed_qkv(h2, a.q_proj.weight, a.q_proj.bias, a.k_proj.weight, a.v_proj.weight, a.v_proj.bias)
        if temporal:
            core = ops.temporal_attention(qkv, BT // self.num_frames, self.num_frames, N, a.num_heads, a.scaling)
        elif bias is None or isinstance(bias, ops.RelPosBias):
            core = ops.spatial_attention(qkv, bias, BT, N, a.num_heads, a.scaling)
        else:  # a dense bias [heads, N, N] that carries the table's gradient: this one product as torch ops on the packed rows
            q, k, v = qkv.view(BT, N, 3, a.num_heads, a.head_dim).permute(2, 0, 3, 1, 4).unbind(0)
            w = torch.matmul(q * a.scaling, k.transpose(-1, -2)) + bias
            core = torch.matmul(F.softmax(w, dim=-1, dtype=torch.float32).to(w.dtype), v).permute(0, 2, 1, 3).reshape(BT * N, -1)
        if a.ln is not None:
            core = ops.layer_norm(core, a.ln.weight, a.ln.bias, a.ln.eps)
        return ops.linear(core, a.out_proj.weight, a.out_proj.bias)

    def forward(self, x, bias=None, fused=False):
        """x: [B * T, N, D].  bias: an ops.RelPosBias handle (fused, frozen table), the dense shared bias [heads, N, N] (torch ops; fused
        while the table is being trained), or None."""
        BT, N, D = x.shape
        if BT % self.num_frames:
            raise ValueError("VideoEncoderLayer: %d frames are not a multiple of num_frames = %d" % (BT, self.num_frames))
        ln1, dp = self.self_attn_layer_norm, self.drop_path_prob
        if fused:
            x = x.contiguous()
            norm1 = lambda t: ops.layer_norm(t.reshape(BT * N, D), ln1.weight, ln1.bias, ln1.eps)  # noqa: E731
            attend = lambda h, temporal: self._attend_fused(h, temporal, bias, BT, N).view(BT, N, D)  # noqa: E731
        else:
            norm1 = ln1
            attend = lambda h, temporal: self._attend_torch(h, temporal, None if temporal else bias)  # noqa: E731
        # temporal adaptation (:331-338): its result only feeds the spatial attention's input
        h = norm1(x)
        if self.num_tadapter == 2:
            h = self.T_Adapter_in(h)
        xt = self.T_Adapter(attend(h, True))
        xs = x + _drop_path_rows(xt, dp, self.training)
        # spatial adaptation (:343-344): the residual is the LAYER INPUT
        ys = self.S_Adapter(attend(norm1(xs), False))
        x = x + _drop_path_rows(self.gamma_1 * ys if self.gamma_1 is not None else ys, dp, self.training)
        # joint adaptation (:346-350)
        fln = self.final_layer_norm
        if fused:
            xn = ops.layer_norm(x, fln.weight, fln.bias, fln.eps)
            x = ops.ffn_branch(x.contiguous(), None, self.ffn_params("image"), True)
        else:
            xn = fln(x)
            y = self.dropout_module(self.image_ffn(xn))
            x = x + (self.gamma_2 * y if self.gamma_2 is not None else y)
        return x + _drop_path_rows(self.scale * self.MLP_Adapter(xn), dp, self.training)


class VideoImageAdapter(ImageAdapter):
    """ImageAdapter + onepeace.py:158 and :198-201: a learned embedding per frame, added at every token position."""

    def __init__(self, cfg, embed_dim, attention_heads, num_frames):
        super().__init__(cfg, embed_dim, attention_heads, num_layers=1)
        self.num_frames = num_frames
        self.temporal_embedding = nn.Parameter(torch.zeros(1, num_frames, embed_dim))

    def forward(self, src_images):
        """src_images: [B * T, C, R, R] -> x [B * T, N, D], the shared bias spec (relpos.RelPosSpec) or None."""
        x, _, biases = super().forward(src_images)
        BT, N, D = x.shape
        if BT % self.num_frames:
            raise ValueError("VideoImageAdapter: %d frames are not a multiple of num_frames = %d" % (BT, self.num_frames))
        x = (x.view(-1, self.num_frames, N, D) + self.temporal_embedding.unsqueeze(2)).view(BT, N, D)
        return x, (biases[0] if biases else None)


class VideoEncoder(nn.Module):
    """onepeace.py:355-420: the layers (stochastic depth rising linearly) and image_layer_norm."""

    def __init__(self, cfg, num_tadapter, num_frames, scale, use_checkpoint):
        super().__init__()
        rates = [r.item() for r in torch.linspace(0, cfg.drop_path_rate, cfg.layers)]
        self.layers = nn.ModuleList(VideoEncoderLayer(cfg, rates[i], num_tadapter, num_frames, scale) for i in range(cfg.layers))
        self.image_layer_norm = LayerNorm(cfg.embed_dim)
        self.use_checkpoint = use_checkpoint

    def forward(self, x, spec):
        fused = ops.hip_eligible(x) and all(layer.video_fused_supported() for layer in self.layers)
        bias = None
        if spec is not None:  # the kernels take the bias as a constant: a table that is being trained goes through the torch product
            constant = not (spec.table.requires_grad and torch.is_grad_enabled())
            bias = spec.handle() if fused and constant else spec.dense(1)[0].to(x.dtype)
        for layer in self.layers:
            if self.use_checkpoint and torch.is_grad_enabled():
                x = checkpoint.checkpoint(layer, x, bias, fused, use_reentrant=False)
            else:
                x = layer(x, bias, fused)
        return self.image_layer_norm(x)


class OnePeaceVideoViT(nn.Module):
    def __init__(self, activation_dropout=0.0, attention_dropout=0.0, attention_heads=12, adapter_scale=0.5, bucket_size=16,
                 num_tadapter=1, num_frames=32, dropout=0.1, drop_path_rate=0.0, embed_dim=1536, ffn_embed_dim=6144, layers=40,
                 layer_scale_init_value=1e-2, rp_bias=False, shared_rp_bias=True, use_checkpoint=False, pretrained=None):
        super().__init__()
        if rp_bias:
            raise NotImplementedError("OnePeaceVideoViT: rp_bias=True (a relative-position table in every layer) is not built; the "
                                      "reference's video configs use shared_rp_bias")
        if pretrained is not None:
            raise NotImplementedError("OnePeaceVideoViT: `pretrained` (a pickle path) is not read here; use load_pretrained(model, "
                                      "state_dict) on a convert_to_vision state dict")
        self.pretrained = None
        adapter_cfg = ImageAdapterConfig(bucket_size=bucket_size, rel_bucket_size=bucket_size, vision_encoder_type="hmlp", dropout=dropout,
                                         use_attn_bias=shared_rp_bias)
        cfg = AdjustEncDecConfig(
            embed_dim=embed_dim, ffn_embed_dim=ffn_embed_dim, layers=layers, attention_heads=attention_heads, normalize_before=True,
            learned_pos=True, drop_path_rate=drop_path_rate, use_text_moe=False, use_image_moe=True, use_audio_moe=False,
            attention_dropout=attention_dropout, activation_dropout=activation_dropout, dropout=dropout, magneto_scale_attn=True,
            scale_attn=False, scale_fc=True, scale_heads=False, use_layer_scale=True, layer_scale_init_value=layer_scale_init_value,
            checkpoint_activations=False, image_adapter=adapter_cfg)
        self.cfg = cfg
        self.image_adapter = VideoImageAdapter(adapter_cfg, embed_dim, attention_heads, num_frames)
        self.encoder = VideoEncoder(cfg, num_tadapter, num_frames, adapter_scale, use_checkpoint)
        self.rp_bias, self.shared_rp_bias, self.num_frames = rp_bias, shared_rp_bias, num_frames
        with torch.no_grad():
            scale = embed_dim ** -0.5
            self.image_adapter.cls_embedding.copy_(scale * torch.randn(1, 1, embed_dim))  # onepeace.py:152-157
            self.image_adapter.pos_embed.copy_(scale * torch.randn(bucket_size ** 2 + 1, embed_dim))
        self._register_state_dict_hook(self._reference_keys)
        self._register_load_state_dict_pre_hook(self._own_keys)

    # ---- the reference's names ------------------------------------------------------------------------------------------
    @staticmethod
    def _reference_keys(module, state_dict, prefix, local_metadata):
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

    def init_weights(self, pretrained=None):
        """onepeace.py:611-665 without the file: trunc_normal_(std=.02) Linears with zero biases, unit LayerNorms, then every adapter's
        D_fc2 zeroed, so that a freshly adapted model computes what the image model computes (temporal_embedding starts at zero)."""
        if pretrained is not None:
            raise NotImplementedError("init_weights: `pretrained` is not read here; use load_pretrained(model, state_dict)")

        def _init(m):
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=.02)  # timm's: cut at +-2 in absolute terms
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)
        self.apply(_init)
        for n, m in self.encoder.named_modules():
            if isinstance(m, Adapter):
                nn.init.constant_(m.D_fc2.weight, 0)
                nn.init.constant_(m.D_fc2.bias, 0)

    @torch.jit.ignore
    def no_weight_decay(self):
        return {"image_adapter.pos_embed", "image_adapter.cls_embedding", "image_adapter.temporal_embedding"}

    def get_num_layers(self):
        return len(self.encoder.layers)

    # ---- forward --------------------------------------------------------------------------------------------------------
    def forward_features(self, x):
        """x: [B, C, T, H, W] -> the encoder's output N x (B * T) x D as in the reference (a view of the batch-major activations)."""
        B, C, T, H, W = x.shape
        frames = x.permute(0, 2, 1, 3, 4).reshape(B * T, C, H, W)
        h, spec = self.image_adapter(frames)
        return self.encoder(h, spec).transpose(0, 1)

    def forward(self, x):
        """x: [B, C, T, H, W] -> [B, D, T, 1, 1]: the CLS rows of image_layer_norm (onepeace.py:684-691), the layout an I3D head takes."""
        B, T = x.shape[0], x.shape[2]
        cls = self.forward_features(x).transpose(0, 1)[:, 0]
        return cls.reshape(B, T, -1).permute(0, 2, 1).unsqueeze(-1).unsqueeze(-1)


def load_pretrained(model, state_dict):
    """onepeace.py:526-609 + :630 on a convert_to_vision state dict (models_vit.convert_to_vision), non-strict, no file read:
    ``image_adapter.rp_bucket`` is dropped (the model's own bucket matrix stands), the shared table is taken from
    ``image_adapter.rel_pos_table_list.0.weight`` or ``image_adapter.rel_pos_table.weight``, and both position tables go through
    ImageAdapter.upgrade_state_dict_named, which resizes them when the model's bucket size is larger (the SciPy interp2d limit of
    models_vit.load_pretrained applies: INTEGRATION.md).  Returns (missing_keys, unexpected_keys) under the reference's names: every
    adapter's parameters and ``image_adapter.temporal_embedding`` are missing BY DESIGN (init_weights() decides them), and so is
    ``encoder.image_layer_norm.*`` when the dict comes from convert_to_vision, which drops the pretraining model's final norm."""
    sd = OrderedDict(state_dict["state_dict"] if "state_dict" in state_dict else state_dict)  # (:565-568)
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


def freeze_for_adapters(model):
    """video/train.py:187-190: only parameters whose name contains ``temporal_embedding``, ``image_layer_norm``, ``cls_head`` or
    ``Adapter`` stay trainable.  `model` may be the backbone or a VideoRecognizer.  On the fused route a frozen weight costs no
    weight-gradient GEMM (every autograd function asks ctx.needs_input_grad).  Returns the names left trainable."""
    kept = []
    for name, p in model.named_parameters():
        p.requires_grad = any(tag in name for tag in _TRAINABLE_TAGS)
        if p.requires_grad:
            kept.append(name)
    return kept


class VideoRecognizer(nn.Module):
    """What the reference's Kinetics-400 configs bind around the backbone, stated, not mirrored (mmaction is not part of this project):
    Recognizer3D + I3DHead(spatial_type='avg', dropout_ratio=0.5), test_cfg average_clips='prob'.  The backbone's [B, D, T, 1, 1] is
    averaged over T (the head's adaptive average pool), dropout, then the ``cls_head`` Linear (I3DHead.fc_cls, init std 0.01)."""

    def __init__(self, backbone, num_classes, dropout_ratio=0.5, init_std=0.01):
        super().__init__()
        self.backbone = backbone
        self.dropout = nn.Dropout(dropout_ratio) if dropout_ratio > 0 else nn.Identity()
        self.cls_head = Linear(backbone.cfg.embed_dim, num_classes)
        nn.init.normal_(self.cls_head.weight, std=init_std)

    def forward(self, x):
        """x: [B, C, T, H, W] -> class scores [B, num_classes]."""
        feat = self.backbone(x).flatten(2).mean(dim=2)
        return self.cls_head(self.dropout(feat))

    @torch.no_grad()
    def forward_test(self, x):
        """x: [B, V, C, T, H, W], V views (clips x crops) per video -> [B, num_classes]: the views' class PROBABILITIES averaged
        (average_clips='prob')."""
        B, V = x.shape[:2]
        scores = self.forward(x.flatten(0, 1))
        return F.softmax(scores.float(), dim=-1).view(B, V, -1).mean(dim=1)
