"""Generate tests/golden/det.pt from the UNMODIFIED reference detection backbone (one_peace_vision/det/models/onepeace.py: OnePeace), run
on the CPU through oracle/ref_shim.py's loader.

    python tests/golden/make_det_golden.py        # needs the reference tree; writes tests/golden/det.pt

detectron2, fairscale and timm are not installed, and the reference file imports from all three at module level; this script puts stub
modules of its own into sys.modules: Backbone is nn.Module, get_rank returns 0, checkpoint_wrapper is the identity, trunc_normal_ is
ref_shim's stub, DropPath is timm's arithmetic (unused: drop_path_rate = 0 makes the reference take nn.Identity).  window_partition,
window_unpartition and add_decomposed_rel_pos (with get_rel_pos) are THIS SCRIPT'S OWN RESTATEMENT of detectron2's published arithmetic
(detectron2/modeling/backbone/utils.py), written out below: the fixture is the reference file's output OVER THOSE THREE STAND-INS, not
over detectron2's own code.

OnePeace(attention_heads=1, embed_dim=64, ffn_embed_dim=64, bucket_size=32, pretrain_bucket_size=16, window_size=16, layers=2,
window_block_indexes=(0,), use_decomposed_rel_pos=True, shared_rp_bias=True, layer_scale_init_value=0.1, dropout=0) -- head_dim 64, one
window block (four windows) and one global block; with embed_dim=128 and two heads the file does not fit under 1 MiB -- from seed 0,
B = 1, input 512 x 512, eval mode.  rel_pos_table, rel_pos_h and
rel_pos_w start at zero and get seeded normal draws of std 0.02.  Weights and inputs are rounded to bf16-representable values first.
The input is stored as a bf16 [1, 3, 64, 64] tensor that this script and the tests expand 8 x per axis by repeat_interleave (the full
input alone would exceed the size limit); the cotangent likewise as [1, 64, 8, 8], expanded 4 x.  Stored: the state dict in bf16
(exact) WITHOUT its two integer buffers image_adapter.rp_bucket [1024, 1024] and image_adapter.rp_bucket_window [256, 256] (8.5 MB as
int64) -- "state_dict_keys" lists every key of the reference's state dict, "bucket_rows" holds rows 0, 1 and the last of both matrices
and "bucket_sums" their element sums, which pin the index arithmetic; the fp32 output [1, 64, 32, 32], the fp32 gradients of
sum(cotangent * output) for GRADS, and, from the reference's own .bfloat16() run on the CPU, only its relative Frobenius errors per
tensor, as plain numbers.  Tensors, names and plain numbers only."""
import os
import sys
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim as R  # noqa: E402

ARGS = dict(attention_heads=1, embed_dim=64, ffn_embed_dim=64, bucket_size=32, pretrain_bucket_size=16, window_size=16, layers=2,
            window_block_indexes=(0,), use_decomposed_rel_pos=True, shared_rp_bias=True, layer_scale_init_value=0.1, dropout=0.0)
GRADS = ("encoder.layers.0.self_attn.rel_pos_h", "encoder.layers.0.self_attn.rel_pos_w", "encoder.layers.1.self_attn.rel_pos_h",
         "encoder.layers.1.self_attn.rel_pos_w", "image_adapter.rel_pos_table.weight", "image_adapter.pos_embed",
         "encoder.layers.0.self_attn.q_proj.bias", "encoder.layers.0.self_attn.v_proj.bias", "encoder.layers.0.gamma_1",
         "encoder.layers.1.gamma_1", "encoder.layers.0.self_attn.k_proj.weight")
SMALL, UP = 64, 8
COT_SMALL, COT_UP = 8, 4
BUCKETS = ("image_adapter.rp_bucket", "image_adapter.rp_bucket_window")


# ---- the three stand-ins: detectron2/modeling/backbone/utils.py restated ---------------------------------------------------------------
def window_partition(x, window_size):
    B, H, W, C = x.shape
    pad_h = (window_size - H % window_size) % window_size
    pad_w = (window_size - W % window_size) % window_size
    if pad_h > 0 or pad_w > 0:
        x = F.pad(x, (0, 0, 0, pad_w, 0, pad_h))
    Hp, Wp = H + pad_h, W + pad_w
    x = x.view(B, Hp // window_size, window_size, Wp // window_size, window_size, C)
    windows = x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, window_size, window_size, C)
    return windows, (Hp, Wp)


def window_unpartition(windows, window_size, pad_hw, hw):
    Hp, Wp = pad_hw
    H, W = hw
    B = windows.shape[0] // (Hp * Wp // window_size // window_size)
    x = windows.view(B, Hp // window_size, Wp // window_size, window_size, window_size, -1)
    x = x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, Hp, Wp, -1)
    if Hp > H or Wp > W:
        x = x[:, :H, :W, :].contiguous()
    return x


def get_rel_pos(q_size, k_size, rel_pos):
    max_rel_dist = int(2 * max(q_size, k_size) - 1)
    if rel_pos.shape[0] != max_rel_dist:
        rel_pos_resized = F.interpolate(rel_pos.reshape(1, rel_pos.shape[0], -1).permute(0, 2, 1), size=max_rel_dist, mode="linear")
        rel_pos_resized = rel_pos_resized.reshape(-1, max_rel_dist).permute(1, 0)
    else:
        rel_pos_resized = rel_pos
    q_coords = torch.arange(q_size)[:, None] * max(k_size / q_size, 1.0)
    k_coords = torch.arange(k_size)[None, :] * max(q_size / k_size, 1.0)
    relative_coords = (q_coords - k_coords) + (k_size - 1) * max(q_size / k_size, 1.0)
    return rel_pos_resized[relative_coords.long()]


def add_decomposed_rel_pos(attn, q, rel_pos_h, rel_pos_w, q_size, k_size):
    q_h, q_w = q_size
    k_h, k_w = k_size
    Rh = get_rel_pos(q_h, k_h, rel_pos_h)
    Rw = get_rel_pos(q_w, k_w, rel_pos_w)
    B, _, dim = q.shape
    r_q = q.reshape(B, q_h, q_w, dim)
    rel_h = torch.einsum("bhwc,hkc->bhwk", r_q, Rh)
    rel_w = torch.einsum("bhwc,wkc->bhwk", r_q, Rw)
    attn = (attn.view(B, q_h, q_w, k_h, k_w) + rel_h[:, :, :, :, None] + rel_w[:, :, :, None, :]).view(B, q_h * q_w, k_h * k_w)
    return attn


class DropPath(nn.Module):
    def __init__(self, drop_prob=0.0):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        if self.drop_prob == 0.0 or not self.training:
            return x
        keep = 1 - self.drop_prob
        return x.div(keep) * x.new_empty((x.shape[0],) + (1,) * (x.ndim - 1)).bernoulli_(keep)


def _stubs():
    def mod(name, **attrs):
        m = sys.modules.get(name)
        if m is None:
            m = types.ModuleType(name)
            m.__path__ = []
            sys.modules[name] = m
        for k, v in attrs.items():
            setattr(m, k, v)
        return m

    mod("fairscale")
    mod("fairscale.nn")
    mod("fairscale.nn.checkpoint", checkpoint_wrapper=lambda m, *a, **k: m)
    mod("timm.models.layers", DropPath=DropPath)
    mod("detectron2")
    mod("detectron2.modeling", Backbone=nn.Module)
    mod("detectron2.modeling.backbone")
    mod("detectron2.modeling.backbone.utils", window_partition=window_partition, window_unpartition=window_unpartition,
        add_decomposed_rel_pos=add_decomposed_rel_pos)
    mod("detectron2.utils")
    mod("detectron2.utils.comm", get_rank=lambda: 0)


def bf(t):
    return t.to(torch.bfloat16).float() if t.is_floating_point() else t


def expand(small):
    """[1, 3, 64, 64] -> [1, 3, 512, 512]: every pixel repeated 8 x 8."""
    return small.repeat_interleave(UP, dim=2).repeat_interleave(UP, dim=3)


def expand_cot(small):
    """[1, D, 8, 8] -> [1, D, 32, 32]."""
    return small.repeat_interleave(COT_UP, dim=2).repeat_interleave(COT_UP, dim=3)


def build(ref):
    torch.manual_seed(0)
    m = ref.OnePeace(**ARGS)
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n, p in sorted(m.named_parameters()):
            if "rel_pos" in n:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
        for p in m.parameters():
            p.copy_(bf(p))
    return m.eval()


def run(m, image, cot, dtype):
    m = m.to(dtype)
    out = m(image.to(dtype))["last_feat"]
    assert out.dtype == dtype and tuple(out.shape) == (1, ARGS["embed_dim"], 32, 32)
    (out * cot.to(dtype)).sum().backward()
    params = dict(m.named_parameters())
    return out.detach().clone(), {n: params[n].grad.detach().clone() for n in GRADS}


def relerr(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    R.install()
    _stubs()
    ref = R._load_file("_ref_det_onepeace", os.path.join(R.REFERENCE_ROOT, "one_peace_vision", "det", "models", "onepeace.py"))
    g = torch.Generator().manual_seed(7)
    small = bf(torch.randn(1, 3, SMALL, SMALL, generator=g))
    cot_small = bf(torch.randn(1, ARGS["embed_dim"], COT_SMALL, COT_SMALL, generator=g))
    cot = expand_cot(cot_small)
    out, grads = run(build(ref), expand(small), cot, torch.float32)
    bout, bgrads = run(build(ref), expand(small), cot, torch.bfloat16)
    full = build(ref).state_dict()
    sd = {k: v.to(torch.bfloat16) for k, v in full.items() if k not in BUCKETS}
    assert all(v.is_floating_point() for v in sd.values()) and all(k in full for k in BUCKETS)
    rows = {k: {i: full[k][i].to(torch.int16) for i in (0, 1, full[k].shape[0] - 1)} for k in BUCKETS}
    sums = {k: int(full[k].sum()) for k in BUCKETS}
    ref_bf16 = {"output": relerr(bout, out)}
    ref_bf16.update({n: relerr(bgrads[n], grads[n]) for n in GRADS})
    fx = {"args": ARGS, "image_small": small.to(torch.bfloat16), "upsample": UP, "cotangent_small": cot_small.to(torch.bfloat16), "cotangent_upsample": COT_UP,
          "state_dict": sd, "state_dict_keys": list(full.keys()), "bucket_rows": rows, "bucket_sums": sums,
          "output": out, "grads": grads, "grad_names": list(GRADS), "ref_bf16_relerr": ref_bf16}
    for k, v in ref_bf16.items():
        print("%-48s the reference's bf16 run off by %.3e (rel. Frobenius)" % (k, v))
    path = os.path.join(HERE, "det.pt")
    torch.save(fx, path)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
