"""Generate tests/golden/vision.pt from the UNMODIFIED reference OnePeaceViT (one_peace_vision/classification/models_vit.py) and
utils/lr_decay.py, run on the CPU through oracle/ref_shim.py (which stubs timm.models.layers.trunc_normal_).

    python tests/golden/make_vision_golden.py        # needs the reference tree; writes tests/golden/vision.pt

OnePeaceViT(bucket_size=4, embed_dim=64, ffn_embed_dim=128, attention_heads=4, layers=2, num_classes=5, layer_scale_init_value=0.1)
from seed 0, once with global_pool=True and once with False, in eval mode.  The relative-position table, which the reference starts at
zero, gets a seeded normal draw (std 0.02) so that the bias path carries values.  Weights and images are rounded to bf16-representable
values first, so that the fp32 run, the reference's own bf16 run and a bf16 device run all start from the same numbers; the fixture
stores them as bf16 (exact).  Per case: the state dict, the fp32 logits, the gradients of sum(cotangent * logits) with respect to
head.weight, fc_norm.weight (global_pool only), image_adapter.pos_embed and encoder.layers.0.gamma_1, the same from the reference
after .bfloat16() on the CPU (bf16_logits, bf16_grads: what bf16 arithmetic costs the reference itself), and the groups of
param_groups_lrd(weight_decay=0.05, no_weight_decay_list=model.no_weight_decay(), layer_decay=0.75) as lists of names with their
lr_scale and weight_decay.  Tensors, names and plain numbers only."""
import contextlib
import io
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim as R  # noqa: E402

ARGS = dict(bucket_size=4, embed_dim=64, ffn_embed_dim=128, attention_heads=4, layers=2, num_classes=5, layer_scale_init_value=0.1)
GRADS = ("head.weight", "fc_norm.weight", "image_adapter.pos_embed", "encoder.layers.0.gamma_1")
B, RES = 2, 64


def bf(t):
    return t.to(torch.bfloat16).float() if t.is_floating_point() else t


def build(vit, global_pool):
    torch.manual_seed(0)
    m = vit.OnePeaceViT(global_pool=global_pool, **ARGS)
    with torch.no_grad():
        m.image_adapter.rel_pos_table.weight.normal_(std=0.02)
        for p in m.parameters():
            p.copy_(bf(p))
    return m.eval()


def run(m, images, cot, dtype):
    m = m.to(dtype)
    logits = m(images.to(dtype))
    assert logits.dtype == dtype and tuple(logits.shape) == (B, ARGS["num_classes"])
    (logits * cot.to(dtype)).sum().backward()
    params = dict(m.named_parameters())
    return logits.detach().clone(), {n: params[n].grad.detach().clone() for n in GRADS if n in params}


def main():
    R.install()
    root = os.path.join(R.REFERENCE_ROOT, "one_peace_vision", "classification")
    vit = R._load_file("_ref_vision_models_vit", os.path.join(root, "models_vit.py"))
    lrd = R._load_file("_ref_vision_lr_decay", os.path.join(root, "utils", "lr_decay.py"))
    g = torch.Generator().manual_seed(7)
    images = bf(torch.randn(B, 3, RES, RES, generator=g))
    cot = bf(torch.randn(B, ARGS["num_classes"], generator=g))
    fx = {"args": ARGS, "images": images.to(torch.bfloat16), "cotangent": cot.to(torch.bfloat16), "cases": {}}
    for name, global_pool in (("global_pool", True), ("cls_token", False)):
        runs = {dtype: run(build(vit, global_pool), images, cot, dtype) for dtype in (torch.float32, torch.bfloat16)}
        m = build(vit, global_pool)
        names = {id(p): n for n, p in m.named_parameters()}
        with contextlib.redirect_stdout(io.StringIO()):  # (the function prints its groups)
            groups = lrd.param_groups_lrd(m, 0.05, no_weight_decay_list=m.no_weight_decay(), layer_decay=0.75)
        fx["cases"][name] = {
            "global_pool": global_pool,
            "state_dict": {k: (v.to(torch.bfloat16) if v.is_floating_point() else v.clone()) for k, v in m.state_dict().items()},
            "logits": runs[torch.float32][0], "grads": runs[torch.float32][1],
            "bf16_logits": runs[torch.bfloat16][0], "bf16_grads": runs[torch.bfloat16][1],
            "groups": [{"lr_scale": float(gr["lr_scale"]), "weight_decay": float(gr["weight_decay"]),
                        "params": [names[id(p)] for p in gr["params"]]} for gr in groups]}
        want = runs[torch.float32][0]
        e = (runs[torch.bfloat16][0].float() - want).norm() / want.norm()
        print("%-12s logits |.| %.3e, the reference's bf16 run off by %.2e (rel. Frobenius)" % (name, want.norm(), e))
    path = os.path.join(HERE, "vision.pt")
    torch.save(fx, path)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("wrote", path, size, "bytes")


if __name__ == "__main__":
    main()
