"""Generate tests/golden/classify.pt from the UNMODIFIED reference OnePeaceClassifyModel, run on the CPU through oracle/ref_shim.py.

    python tests/golden/make_classify_golden.py        # needs the reference tree; writes tests/golden/classify.pt

Micro models (H = 128, 2 layers, 2 heads, 64 x 64 images, 9 tokens, 1 s of audio) with the deterministic weights of oracle/synth.py.
Weights and floating-point inputs are rounded to bf16-representable values first, so that the fp32 run, the reference's own bf16 run
and a bf16 device run all start from the same numbers.  The file holds the inputs once (floating-point ones as bf16: exact) and per case the names of those it passes, the
`shapes` of the state dict, the fp32 logits, the gradients under a fixed random cotangent of every classify_head.* parameter and of a
few encoder parameters, and the same outputs of the reference after .bfloat16() on the CPU -- what bf16 arithmetic costs the reference
itself, the yardstick of tests/test_classify_gpu.py.  A gradient of more than 4096 elements is stored as its first 16 rows plus its
Frobenius norm (name#rows16, name#norm): the fixture stays far below 1 MiB.  Tensors and plain numbers only."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim as R  # noqa: E402
from oracle import synth  # noqa: E402

MICRO = dict(embed_dim=128, ffn_embed_dim=256, layers=2, attention_heads=2, image_rel_bucket_size=4, text_bucket_size=256,
             audio_bucket_size=512)
VOCAB, B, NUM_CLASSES = 1000, 3, 7
OPTS = dict(attn_pooling=True, use_pooler=False, pooler_dropout=0.0, head_scale_ratio=1, use_image_features=False,
            freeze_finetune_updates=0, use_two_images=False, add_type_embedding=False)
CASES = [   # name, head type, options that differ from OPTS
    ("vl_two_images", "vl", dict(use_two_images=True, add_type_embedding=True, use_pooler=True)),
    ("image", "image", {}),
    ("audio", "audio", {}),
    ("al", "al", {}),
    ("image_cls_token", "image", dict(attn_pooling=False)),
]
ENCODER_GRADS = {"text": ("encoder_wrapper.text_adapter.cls_embedding", "encoder_wrapper.fusion_model.text_layer_norm.weight"),
                 "image": ("encoder_wrapper.image_adapter.cls_embedding", "encoder_wrapper.fusion_model.image_layer_norm.weight"),
                 "audio": ("encoder_wrapper.audio_adapter.cls_embedding", "encoder_wrapper.fusion_model.audio_layer_norm.weight")}
COMMON_GRADS = ("encoder_wrapper.fusion_model.layers.0.self_attn.q_proj.weight", "encoder_wrapper.fusion_model.layers.1.self_attn.out_proj.bias")
USES = {"vl": ("text", "image"), "image": ("image",), "audio": ("audio",), "al": ("text", "audio")}


def bf(t):
    return t.to(torch.bfloat16).float() if t.is_floating_point() else t


def kept_grads(model, head_type):
    names = set(COMMON_GRADS)
    for m in USES[head_type]:
        names.update(ENCODER_GRADS[m])
    out = {}
    for n, p in model.named_parameters():
        if not (n.startswith("classify_head.") or n in names):
            continue
        if p.grad is None:   # (classify_head.norm without attention pooling: built, never used)
            continue
        g = p.grad.detach().clone()
        if g.numel() <= 4096:
            out[n] = g
        else:
            out[n + "#rows16"] = g[:16].clone()
            out[n + "#norm"] = g.double().norm().float()
    return out


def build(head_type, opts):
    mod = R.ref("one_peace.models.one_peace.one_peace_classify")
    cfg = R.make_cfg(**MICRO)
    for k in ("attn_pooling", "use_pooler", "pooler_dropout", "head_scale_ratio", "use_image_features", "freeze_finetune_updates"):
        setattr(cfg, k, opts[k])
    cfg.encoder.text_adapter.add_type_embedding = cfg.encoder.image_adapter.add_type_embedding = opts["add_type_embedding"]
    torch.manual_seed(0)
    m = mod.OnePeaceClassifyModel(cfg, R.TinyDictionary(VOCAB), head_type, num_classes=NUM_CLASSES, use_two_images=opts["use_two_images"])
    shapes = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    sd = {k: bf(v) for k, v in synth.synth_state_dict(shapes).items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.split(".")[-1] in synth.NON_SYNTH for k in missing), (missing, unexpected)
    return m.eval(), shapes


def main():
    base = synth.synth_inputs(B, text_len=9, image_res=64, audio_samples=16000, vocab=VOCAB)
    base = {k: bf(v) for k, v in base.items()}
    images_2 = bf(synth.synth_tensor("inputs/src_images_2", base["src_images"].shape) * 2.0)   # (synth_tensor scales unnamed kinds by 0.5)
    base["src_images_2"] = images_2
    # the inputs once, shared by the cases (each case lists the names it passes to the model)
    fx = {"cfg": MICRO, "vocab": VOCAB, "num_classes": NUM_CLASSES, "cases": {},
          "inputs": {k: (v.to(torch.bfloat16) if v.is_floating_point() else v) for k, v in base.items()}}
    for name, head_type, delta in CASES:
        opts = dict(OPTS, **delta)
        inp = {}
        if "text" in USES[head_type]:
            inp["src_tokens"] = base["src_tokens"]
        if "image" in USES[head_type]:
            inp["src_images"] = base["src_images"]
            if opts["use_two_images"]:
                inp["src_images_2"] = images_2
        if "audio" in USES[head_type]:
            inp["src_audios"], inp["audio_padding_masks"] = base["src_audios"], base["audio_padding_masks"]
        cot = bf(synth.synth_tensor("cotangent/" + name, (B, NUM_CLASSES), seed=11))
        runs = {}
        for dtype in (torch.float32, torch.bfloat16):
            m, shapes = build(head_type, opts)
            m = m.to(dtype)
            args = {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in inp.items()}
            logits = m(**args)
            assert logits.dtype == dtype and tuple(logits.shape) == (B, NUM_CLASSES)
            logits.backward(cot.to(dtype))
            runs[dtype] = {"logits": logits.detach().clone(), "grads": kept_grads(m, head_type)}
        fx["cases"][name] = {
            "head_type": head_type, "opts": opts, "shapes": shapes, "cotangent": cot.to(torch.bfloat16),
            "inputs": sorted(inp),
            "logits": runs[torch.float32]["logits"], "grads": runs[torch.float32]["grads"],
            "bf16_logits": runs[torch.bfloat16]["logits"], "bf16_grads": runs[torch.bfloat16]["grads"]}
        e = (runs[torch.bfloat16]["logits"].float() - runs[torch.float32]["logits"]).norm() / runs[torch.float32]["logits"].norm()
        print("%-16s logits |.| %.4f, the reference's bf16 run off by %.2e (rel. Frobenius)" % (name, runs[torch.float32]["logits"].norm(), e))
    path = os.path.join(HERE, "classify.pt")
    torch.save(fx, path)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
