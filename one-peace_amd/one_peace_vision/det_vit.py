"""Detection branch (ViTDet backbone): mirror of one_peace_vision/det/models/onepeace.py -- ImageAdaptor without a CLS token and with the
window bucket (:78-157), MultiheadAttention with the decomposed relative positions (:160-216), the layer with window partition
(:219-331), the encoder (:334-409), the backbone OnePeace (:412-629, here OnePeaceDetViT) -- with the checkpoint loading of :472-483 as
load_pretrained_det and get_onepeace_lr_decay_rate (:632-653).

Modules and parameters carry the reference's names, so ``state_dict()`` keys are the reference's and a state dict of the reference model
loads with ``strict=True``.  Activations stay in the project's batch-major rows of the [B, Hg, Wg, D] map all the way: the attention core
of a window block (ops.window_attention over csrc/windowattn.hip) reads the packed q|k|v rows where they lie, so window_partition,
window_unpartition, the expanded window bias [B * windows * heads, 256, 256] (:398-401) and the score tensors of add_decomposed_rel_pos
do not exist here.

A window block takes the fused route when the tensors are bf16 device tensors, head_dim is 64, the window is 16, the grid is a multiple
of 16 and dropout is inactive: ops.layer_norm, ops.packed_qkv, ops.window_attention, the sub-LayerNorm, ops.linear, ops.ffn_branch
(the row-wise ones need embed_dim and ffn_embed_dim to be multiples of 128; a narrower model keeps the kernels for the window core alone).
Otherwise the same statements run as torch ops (ops.window_attention_torch on the packed rows, which pads as detectron2 does: the padded
positions take the projection of a zero row, q_proj.bias | 0 | v_proj.bias).  GLOBAL blocks always run the torch statement of the
attention core on the packed rows (one window of bucket_size x bucket_size; their decomposed indices are detectron2's get_rel_pos for
q_size == k_size, ops.decomposed_rel_index); the row-wise ops around it are fused under the same conditions.
``use_checkpoint`` wraps each layer in torch.utils.checkpoint (non-reentrant).

Not built, stated:
  * ``rp_bias=True`` (a table inside every layer) raises NotImplementedError: its checkpoint path (:596-611) needs
    scipy.interpolate.interp2d, which current SciPy no longer has.
  * SimpleFeaturePyramid, the Cascade R-CNN heads and soft-NMS of det/configs/onepeace/cascade_mask_rcnn_vitdet_50ep.py: those are
    detectron2, not this backbone (INTEGRATION.md says how a config binds OnePeaceDetViT).
  * the reference's random stream for stochastic depth: one draw per sample and residual term, the reference's distribution.
  * ``pretrained`` file loading (:472-477, a pickle): load_pretrained_det takes a state dict and reads no file.
  * the grid must be bucket_size x bucket_size (the reference's pos_embed reshape and global bias need the same); the attention
    module's ``dropout_module`` is never applied in the reference's forward (:194-216) and is not applied here."""
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint

from .. import ops
from ..transformer.transformer_layer import sample_path_scale


def make_bucket_position(size):
    """[size^2, size^2] int64: entry (i, j) = (iy - jy + size - 1) * (2 size - 1) + (ix - jx + size - 1), the rows [1:, 1:] of the
    reference's make_image_bucket_position (:23-39; the CLS entries do not exist here)."""
    c = torch.arange(size)
    yy, xx = c.repeat_interleave(size), c.repeat(size)
    return (yy[:, None] - yy[None, :] + size - 1) * (2 * size - 1) + (xx[:, None] - xx[None, :] + size - 1)


class LayerNorm2D(nn.Module):
    def __init__(self, embed_dim):
        super().__init__()
        self.layer_norm = nn.LayerNorm(embed_dim)

    def forward(self, x):
        return self.layer_norm(x.permute(0, 2, 3, 1)).permute(0, 3, 1, 2)


class GeGLU(nn.Module):
    def __init__(self, embed_dim, ffn_dim):
        super().__init__()
        self.wi_0 = nn.Linear(embed_dim, ffn_dim, bias=False)
        self.wi_1 = nn.Linear(embed_dim, ffn_dim, bias=False)
        self.act = nn.GELU()

    def forward(self, x):
        return self.act(self.wi_0(x)) * self.wi_1(x)


class ImageAdaptor(nn.Module):
    """onepeace.py:78-157: hMLP stem, pos_embed[1:] (no CLS token), the shared table with rp_bucket and rp_bucket_window."""

    def __init__(self, attention_heads=24, bucket_size=64, embed_dim=1536, dropout=0.1, pretrain_bucket_size=16, shared_rp_bias=True,
                 window_size=0):
        super().__init__()
        self.dropout = nn.Dropout(dropout)
        self.embed_images = nn.Sequential(
            nn.Conv2d(3, embed_dim // 4, kernel_size=4, stride=4), LayerNorm2D(embed_dim // 4), nn.GELU(),
            nn.Conv2d(embed_dim // 4, embed_dim // 4, kernel_size=2, stride=2), LayerNorm2D(embed_dim // 4), nn.GELU(),
            nn.Conv2d(embed_dim // 4, embed_dim, kernel_size=2, stride=2))
        self.pretrain_bucket_size, self.bucket_size, self.window_size = pretrain_bucket_size, bucket_size, window_size
        self.pos_embed = nn.Parameter(embed_dim ** -0.5 * torch.randn(bucket_size ** 2 + 1, embed_dim))
        self.shared_rp_bias = shared_rp_bias
        if shared_rp_bias:
            self.rel_pos_table = nn.Embedding((2 * pretrain_bucket_size - 1) ** 2 + 3, attention_heads)
            nn.init.constant_(self.rel_pos_table.weight, 0)
            self.register_buffer("rp_bucket", make_bucket_position(bucket_size))
            self.register_buffer("rp_bucket_window", make_bucket_position(window_size))

    def get_rel_pos_bias(self, window=False):
        """[heads, L, L], L = window^2 or bucket^2: F.embedding of the table through the bucket matrix; the table is resized with a
        bicubic F.interpolate first when its size differs (:123-144)."""
        src = 2 * self.pretrain_bucket_size - 1
        dst = 2 * self.window_size - 1 if window else 2 * self.bucket_size - 1
        table = self.rel_pos_table.weight
        if src != dst:
            grid = F.interpolate(table[:-3].view(1, src, src, -1).permute(0, 3, 1, 2), size=(dst, dst), mode="bicubic")
            table = torch.cat((grid.permute(0, 2, 3, 1).reshape(dst ** 2, -1), table[-3:]), dim=0)
        return F.embedding(self.rp_bucket_window if window else self.rp_bucket, table).permute(2, 0, 1).contiguous()

    def forward(self, x):
        x = self.embed_images(x).permute(0, 2, 3, 1)
        h, w = x.shape[1:3]
        if h * w != self.bucket_size ** 2:
            raise ValueError("ImageAdaptor: a %d x %d grid does not match bucket_size = %d" % (h, w, self.bucket_size))
        x = self.dropout(x + self.pos_embed[1:].unsqueeze(0).reshape(1, h, w, -1))
        if not self.shared_rp_bias:
            return x, None, None
        return x, self.get_rel_pos_bias(), self.get_rel_pos_bias(True)


class MultiheadAttention(nn.Module):
    """onepeace.py:160-216; forward lives in the layer (the packed projection belongs to the route)."""

    def __init__(self, embed_dim, num_heads, dropout=0.0, use_decomposed_rel_pos=False, input_size=None):
        super().__init__()
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.dropout_module = nn.Dropout(dropout)
        self.head_dim = embed_dim // num_heads
        assert self.head_dim * num_heads == embed_dim, "embed_dim must be divisible by num_heads"
        self.scaling = self.head_dim ** -0.5
        self.ln = nn.LayerNorm(embed_dim)
        self.k_proj = nn.Linear(embed_dim, embed_dim, bias=False)
        self.v_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        self.q_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=True)
        self.use_decomposed_rel_pos = use_decomposed_rel_pos
        if use_decomposed_rel_pos:
            self.rel_pos_h = nn.Parameter(torch.zeros(2 * input_size[0] - 1, self.head_dim))
            self.rel_pos_w = nn.Parameter(torch.zeros(2 * input_size[1] - 1, self.head_dim))


def _drop_path(x, ps):
    """x [B, ...] times the per-sample multipliers ps (fp32 [B]) or unchanged."""
    return x if ps is None else x * ps.to(x.dtype).view(-1, *([1] * (x.dim() - 1)))


class TransformerEncoderLayer(nn.Module):
    """onepeace.py:219-331 on the batch-major map x [B, Hg, Wg, D]."""

    def __init__(self, activation_dropout=0.0, attention_dropout=0.0, attention_heads=24, bucket_size=64, pretrain_bucket_size=16,
                 dropout=0.0, drop_path_rate=0.0, embed_dim=1536, ffn_embed_dim=6144, layer_scale_init_value=1e-2, rp_bias=False,
                 use_decomposed_rel_pos=False, window_size=0):
        super().__init__()
        self.embed_dim, self.ffn_embed_dim, self.rp_bias = embed_dim, ffn_embed_dim, rp_bias
        size = window_size if window_size > 0 else bucket_size
        self.self_attn = MultiheadAttention(embed_dim, attention_heads, dropout=attention_dropout,
                                            use_decomposed_rel_pos=use_decomposed_rel_pos, input_size=(size, size))
        self.self_attn_layer_norm = nn.LayerNorm(embed_dim)
        self.dropout = nn.Dropout(dropout)
        self.activation_dropout = nn.Dropout(float(activation_dropout))
        self.image_ffn = nn.Sequential(GeGLU(embed_dim, ffn_embed_dim), self.activation_dropout, nn.LayerNorm(ffn_embed_dim),
                                       nn.Linear(ffn_embed_dim, embed_dim))
        self.final_layer_norm = nn.LayerNorm(embed_dim)
        self.drop_path_prob = float(drop_path_rate)
        self.gamma_1 = nn.Parameter(layer_scale_init_value * torch.ones(embed_dim))
        self.gamma_2 = nn.Parameter(layer_scale_init_value * torch.ones(embed_dim))
        self.window_size = window_size
        self.bucket_size = size

    def fused_supported(self, x):
        """The row-wise ops of the layer as HIP ops: bf16 device tensors, head_dim 64, inactive dropout, and widths the packed
        projection and the FFN branch take (multiples of 128).  A narrower model still runs its window core through the kernels
        (ops.window_attention decides that by itself), with torch ops around it."""
        drop = self.training and (self.dropout.p > 0.0 or self.activation_dropout.p > 0.0)
        return (ops.hip_eligible(x) and self.self_attn.head_dim == 64 and not drop and self.embed_dim % 128 == 0
                and self.ffn_embed_dim % 128 == 0)

    def ffn_params(self):
        ffn, fln = self.image_ffn, self.final_layer_norm
        return (fln.weight, fln.bias, ffn[0].wi_0.weight, ffn[0].wi_1.weight, ffn[2].weight, ffn[2].bias, ffn[3].weight, ffn[3].bias,
                self.gamma_2)

    def _core(self, qkv, bias, B, Hg, Wg):
        """The attention core on the packed rows [B * Hg * Wg, 3 D] (:204-213 with the partition of :310 and :325 in a window block)."""
        a = self.self_attn
        rel_h, rel_w = (a.rel_pos_h, a.rel_pos_w) if a.use_decomposed_rel_pos else (None, None)
        if self.window_size > 0:
            pad_row = torch.cat([a.q_proj.bias, torch.zeros_like(a.q_proj.bias), a.v_proj.bias]).to(qkv.dtype)
            return ops.window_attention(qkv, bias, rel_h, rel_w, B, Hg, Wg, a.num_heads, self.window_size, a.scaling, pad_row)
        if Hg != Wg or Hg != self.bucket_size:
            raise ValueError("a global block needs a %d x %d grid, got %d x %d" % (self.bucket_size, self.bucket_size, Hg, Wg))
        return ops.window_attention_torch(qkv, bias, rel_h, rel_w, B, Hg, Wg, a.num_heads, Hg, a.scaling)

    def forward(self, x, attn_bias=None, attn_bias_window=None):
        B, Hg, Wg, D = x.shape
        a, ln1 = self.self_attn, self.self_attn_layer_norm
        bias = attn_bias_window if self.window_size > 0 else attn_bias
        ps1 = sample_path_scale(B, self.drop_path_prob, self.training, x.device)
        ps2 = sample_path_scale(B, self.drop_path_prob, self.training, x.device)
        if self.fused_supported(x):
            x = x.contiguous()
            h = ops.layer_norm(x.view(B * Hg * Wg, D), ln1.weight, ln1.bias, ln1.eps)
            qkv = ops.packed_qkv(h, a.q_proj.weight, a.q_proj.bias, a.k_proj.weight, a.v_proj.weight, a.v_proj.bias)
            core = self._core(qkv, bias, B, Hg, Wg)
            y = ops.linear(ops.layer_norm(core, a.ln.weight, a.ln.bias, a.ln.eps), a.out_proj.weight, a.out_proj.bias)
            x = x + _drop_path(self.gamma_1 * y.view(B, Hg, Wg, D), ps1)
            return ops.ffn_branch(x.view(B, Hg * Wg, D), ps2, self.ffn_params(), True).view(B, Hg, Wg, D)
        h = ln1(x).reshape(B * Hg * Wg, D)
        qkv = torch.cat([a.q_proj(h), a.k_proj(h), a.v_proj(h)], dim=-1)
        y = a.out_proj(a.ln(self._core(qkv, bias, B, Hg, Wg))).view(B, Hg, Wg, D)
        x = x + _drop_path(self.gamma_1 * self.dropout(y), ps1)
        return x + _drop_path(self.gamma_2 * self.dropout(self.image_ffn(self.final_layer_norm(x))), ps2)


class TransformerEncoder(nn.Module):
    """onepeace.py:334-409: the layers (stochastic depth rising linearly), no final LayerNorm."""

    def __init__(self, layers=40, drop_path_rate=0.0, window_size=0, window_block_indexes=(), use_checkpoint=False, **layer_args):
        super().__init__()
        rates = [r.item() for r in torch.linspace(0, drop_path_rate, layers)]
        self.attention_heads, self.window_size = layer_args["attention_heads"], window_size
        self.layers = nn.ModuleList(TransformerEncoderLayer(drop_path_rate=rates[i], window_size=window_size if i in window_block_indexes else 0,
                                                            **layer_args) for i in range(layers))
        self.num_layers = len(self.layers)
        self.use_checkpoint = use_checkpoint

    def forward(self, image_info):
        x, bias, bias_window = image_info
        if bias is not None:   # (:391-401: the reference adds them into zeros of x's dtype and expands them; here they stay [heads, L, L])
            bias, bias_window = bias.to(x.dtype), bias_window.to(x.dtype)
        for layer in self.layers:
            if self.use_checkpoint and torch.is_grad_enabled():
                x = checkpoint.checkpoint(layer, x, bias, bias_window, use_reentrant=False)
            else:
                x = layer(x, bias, bias_window)
        return x


class OnePeaceDetViT(nn.Module):
    def __init__(self, activation_dropout=0.0, attention_dropout=0.0, attention_heads=24, bucket_size=64, pretrain_bucket_size=16,
                 dropout=0.0, embed_dim=1536, drop_path_rate=0.0, ffn_embed_dim=6144, layers=40, layer_scale_init_value=1e-2,
                 out_feature="last_feat", rp_bias=False, use_decomposed_rel_pos=False, shared_rp_bias=True, use_checkpoint=False,
                 window_size=0, window_block_indexes=(), pretrained=None):
        super().__init__()
        if rp_bias:
            raise NotImplementedError("OnePeaceDetViT: rp_bias=True (a relative-position table in every layer) is not built; the "
                                      "reference's detection config uses shared_rp_bias")
        if pretrained is not None:
            raise NotImplementedError("OnePeaceDetViT: `pretrained` (a path) is not read here; use load_pretrained_det(model, state_dict)")
        # (the reference does not hand pretrain_bucket_size to its adapter either: :436-443, the table keeps the default 16)
        self.image_adapter = ImageAdaptor(attention_heads=attention_heads, bucket_size=bucket_size, embed_dim=embed_dim, dropout=dropout,
                                          shared_rp_bias=shared_rp_bias, window_size=window_size)
        self.encoder = TransformerEncoder(
            layers=layers, drop_path_rate=drop_path_rate, window_size=window_size, window_block_indexes=tuple(window_block_indexes),
            use_checkpoint=use_checkpoint, activation_dropout=activation_dropout, attention_dropout=attention_dropout,
            attention_heads=attention_heads, bucket_size=bucket_size, pretrain_bucket_size=pretrain_bucket_size, dropout=dropout,
            embed_dim=embed_dim, ffn_embed_dim=ffn_embed_dim, layer_scale_init_value=layer_scale_init_value, rp_bias=rp_bias,
            use_decomposed_rel_pos=use_decomposed_rel_pos)
        self.rp_bias, self.shared_rp_bias = rp_bias, shared_rp_bias
        self._out_feature_channels = {out_feature: embed_dim}
        self._out_feature_strides = {out_feature: 16}
        self._out_features = [out_feature]
        self.apply(self._init_weights)

    @staticmethod
    def _init_weights(m):
        if isinstance(m, nn.Linear):
            nn.init.trunc_normal_(m.weight, std=0.02)
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        elif isinstance(m, nn.LayerNorm):
            nn.init.constant_(m.bias, 0)
            nn.init.constant_(m.weight, 1.0)

    def forward(self, x):
        """x: [B, 3, 16 * bucket_size, 16 * bucket_size] -> {out_feature: [B, D, Hg, Wg]}."""
        x = self.encoder(self.image_adapter(x))
        return {self._out_features[0]: x.permute(0, 3, 1, 2).contiguous()}


def resize_abs_pos_embed(model, state_dict):
    """onepeace.py:535-558: the checkpoint's pos_embed (CLS row + a square grid) resized to the model's grid, bicubic, in place."""
    pos = state_dict["image_adapter.pos_embed"]
    new = model.image_adapter.bucket_size
    extra = model.image_adapter.pos_embed.shape[-2] - new ** 2
    old = int((pos.shape[-2] - extra) ** 0.5)
    if old != new:
        grid = pos[extra:].reshape(-1, old, old, pos.shape[-1]).permute(0, 3, 1, 2)
        grid = F.interpolate(grid.float(), size=(new, new), mode="bicubic", align_corners=False).to(pos.dtype)
        state_dict["image_adapter.pos_embed"] = torch.cat((pos[:extra], grid.permute(0, 2, 3, 1).flatten(0, 2)), dim=0)


def load_pretrained_det(model, state_dict):
    """onepeace.py:472-483 on a state dict (a ``model`` entry is unwrapped), no file read: resize_abs_pos_embed, every
    ``image_adapter.rp_bucket*`` dropped (the model's own matrices stand), ``image_adapter.rel_pos_table_list.0.weight`` copied to
    ``image_adapter.rel_pos_table.weight`` (:586-587; the table keeps its pretraining size, get_rel_pos_bias resizes it per forward),
    loaded non-strictly.  Returns (missing_keys, unexpected_keys): rel_pos_h / rel_pos_w of every layer and the two bucket matrices are
    missing BY DESIGN, and the pretraining name of the table is reported unexpected, as in the reference's printout."""
    sd = dict(state_dict["model"] if "model" in state_dict else state_dict)
    resize_abs_pos_embed(model, sd)
    listed = "image_adapter.rel_pos_table_list.0.weight"
    if model.shared_rp_bias and listed in sd:
        sd["image_adapter.rel_pos_table.weight"] = sd[listed]
    for k in [k for k in sd if "image_adapter.rp_bucket" in k]:
        sd.pop(k)
    result = model.load_state_dict(sd, strict=False)
    return list(result.missing_keys), list(result.unexpected_keys)


def get_onepeace_lr_decay_rate(name, lr_decay_rate=0.9, num_layers=40):
    """onepeace.py:632-653 without the print: lr_decay_rate ^ (num_layers + 1 - layer_id), layer_id 0 for ``backbone...image_adapter``,
    n + 1 for ``backbone...layers.n.`` (not under ``.residual.``), num_layers + 1 for everything else."""
    layer_id = num_layers + 1
    if name.startswith("backbone"):
        if ".image_adapter" in name:
            layer_id = 0
        elif ".layers." in name and ".residual." not in name:
            layer_id = int(name[name.find(".layers."):].split(".")[2]) + 1
    return lr_decay_rate ** (num_layers + 1 - layer_id)
