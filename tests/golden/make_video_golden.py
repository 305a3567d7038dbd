"""Generate tests/golden/video.pt from the UNMODIFIED reference video backbone
(one_peace_vision/video/mmaction_custom/models/backbones/onepeace.py: OnePeaceViT), run on the CPU through oracle/ref_shim.py's loader.

    python tests/golden/make_video_golden.py        # needs the reference tree; writes tests/golden/video.pt

The reference file imports mmcv.runner.get_dist_info, mmaction.utils.get_root_logger and mmaction.models.builder.BACKBONES at module
level; this script puts stub modules of its own into sys.modules for the three (rank 0 of 1, the logging module's logger, a registry
whose register_module() returns the class unchanged).  einops, scipy and timm's trunc_normal_ (ref_shim's stub) are what is installed.

OnePeaceViT(attention_heads=2, embed_dim=128, ffn_embed_dim=128, bucket_size=4, num_frames=4, layers=2, layer_scale_init_value=0.1,
dropout=0) -- head_dim 64 -- from seed 0, input [2, 3, 4, 64, 64], eval mode.  After init_weights() (which zeroes every adapter's D_fc2;
the table and temporal_embedding start at zero too) every adapter's D_fc2 (weight and bias), rel_pos_table and temporal_embedding get
seeded normal draws of std 0.02, so that every path carries values.  Weights and inputs are rounded to bf16-representable values first,
so that the fp32 run, the reference's own bf16 run and a bf16 device run start from the same numbers; the fixture stores them as bf16
(exact).  Case "tadapter1" stores the whole state dict, the fp32 output [2, 128, 4, 1, 1] and the gradients of sum(cotangent * output)
for GRADS, and the same from the reference after .bfloat16() on the CPU (what bf16 arithmetic costs the reference itself).  Case
"tadapter2" (num_tadapter=2) takes every key it shares with case one from case one and stores only ITS EXTRA keys (T_Adapter_in.*;
"base" names the case that holds the rest -- asserted equal here), its outputs and gradients.  Tensors, names and plain
numbers only."""
import logging
import os
import sys
import types

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim as R  # noqa: E402

ARGS = dict(attention_heads=2, embed_dim=128, ffn_embed_dim=128, bucket_size=4, num_frames=4, layers=2, layer_scale_init_value=0.1,
            dropout=0.0)
GRADS = ("encoder.layers.0.T_Adapter.D_fc1.weight", "encoder.layers.1.T_Adapter.D_fc2.bias", "encoder.layers.0.S_Adapter.D_fc1.bias",
         "encoder.layers.1.S_Adapter.D_fc2.bias", "encoder.layers.0.MLP_Adapter.D_fc1.bias", "encoder.layers.1.MLP_Adapter.D_fc2.weight",
         "encoder.layers.0.T_Adapter_in.D_fc1.bias", "encoder.layers.1.T_Adapter_in.D_fc2.bias",
         "image_adapter.temporal_embedding", "encoder.image_layer_norm.weight", "encoder.layers.0.gamma_1",
         "encoder.layers.0.self_attn.q_proj.bias", "encoder.layers.0.self_attn.v_proj.bias", "image_adapter.pos_embed",
         "image_adapter.rel_pos_table.weight")  # (few weight matrices: the file stays under 1 MiB)
B, RES = 2, 64


def _stubs():
    def mod(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
        return m

    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    mod("mmcv")
    mod("mmcv.runner", get_dist_info=lambda: (0, 1))
    mod("mmaction")
    mod("mmaction.utils", get_root_logger=lambda *a, **k: logging.getLogger("mmaction"))
    mod("mmaction.models")
    mod("mmaction.models.builder", BACKBONES=_Registry())


def bf(t):
    return t.to(torch.bfloat16).float() if t.is_floating_point() else t


def build(ref, num_tadapter, base=None):
    torch.manual_seed(0)
    m = ref.OnePeaceViT(num_tadapter=num_tadapter, **ARGS)
    m.init_weights()
    if base is not None:  # the keys the first case has are the first case's: the second differs by T_Adapter_in alone
        missing = m.load_state_dict({k: v.float() if v.is_floating_point() else v for k, v in base.items()}, strict=False).missing_keys
        assert missing and all("T_Adapter_in" in k for k in missing), missing
    g = torch.Generator().manual_seed(11)
    with torch.no_grad():
        for n, p in sorted(m.named_parameters()):   # by name: the draws of the shared keys do not depend on num_tadapter
            if "T_Adapter_in" in n:
                continue
            if ("Adapter" in n and "D_fc2" in n) or "rel_pos_table" in n or "temporal_embedding" in n:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
        for n, p in sorted(m.named_parameters()):
            if "T_Adapter_in" in n and "D_fc2" in n:
                p.copy_(0.02 * torch.randn(p.shape, generator=g))
        for p in m.parameters():
            p.copy_(bf(p))
    return m.eval()


def run(m, video, cot, dtype):
    m = m.to(dtype)
    out = m(video.to(dtype))
    assert out.dtype == dtype and tuple(out.shape) == (B, ARGS["embed_dim"], ARGS["num_frames"], 1, 1)
    (out * cot.to(dtype)).sum().backward()
    params = dict(m.named_parameters())
    return out.detach().clone(), {n: params[n].grad.detach().clone() for n in GRADS if n in params}


def main():
    R.install()
    _stubs()
    ref = R._load_file("_ref_video_onepeace", os.path.join(R.REFERENCE_ROOT, "one_peace_vision", "video", "mmaction_custom", "models",
                                                           "backbones", "onepeace.py"))
    g = torch.Generator().manual_seed(7)
    video = bf(torch.randn(B, 3, ARGS["num_frames"], RES, RES, generator=g))
    cot = bf(torch.randn(B, ARGS["embed_dim"], ARGS["num_frames"], 1, 1, generator=g))
    fx = {"args": ARGS, "video": video.to(torch.bfloat16), "cotangent": cot.to(torch.bfloat16), "cases": {}}
    full = None
    for name, num_tadapter in (("tadapter1", 1), ("tadapter2", 2)):
        runs = {dtype: run(build(ref, num_tadapter, full), video, cot, dtype) for dtype in (torch.float32, torch.bfloat16)}
        sd = {k: (v.to(torch.bfloat16) if v.is_floating_point() else v.clone())
              for k, v in build(ref, num_tadapter, full).state_dict().items()}
        if full is None:
            full = sd
        else:  # only the extra keys are stored; the rest IS case one's
            extra = {k: v for k, v in sd.items() if k not in full}
            assert all("T_Adapter_in" in k for k in extra) and all(torch.equal(sd[k], full[k]) for k in full)
            sd = extra
        fx["cases"][name] = {"num_tadapter": num_tadapter, "state_dict": sd, "base": None if sd is full else "tadapter1",
                             "output": runs[torch.float32][0], "grads": runs[torch.float32][1],
                             "bf16_output": runs[torch.bfloat16][0], "bf16_grads": runs[torch.bfloat16][1]}
        want = runs[torch.float32][0]
        e = (runs[torch.bfloat16][0].float() - want).norm() / want.norm()
        print("%-10s output |.| %.3e, the reference's bf16 run off by %.2e (rel. Frobenius)" % (name, want.norm(), e))
    path = os.path.join(HERE, "video.pt")
    torch.save(fx, path)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
