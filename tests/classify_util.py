"""Shared by tests/test_classify_cpu.py and tests/test_classify_gpu.py: the fixture tests/golden/classify.pt
(tests/golden/make_classify_golden.py), the mirror model built with the fixture's configuration and the bf16-rounded synthetic weights,
and the comparison of stored gradients."""
import os
from types import SimpleNamespace

import torch

from oracle import synth
from tests.model_util import TinyDictionary

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "classify.pt")
CASE_NAMES = ("vl_two_images", "image", "audio", "al", "image_cls_token")
_fx = None


def fixture():
    global _fx
    if _fx is None:
        _fx = torch.load(GOLDEN, map_location="cpu", weights_only=False)
    return _fx


def make_cfg(fx, opts):
    from one_peace_amd.unify_model_config import one_peace_encoder_config
    enc = one_peace_encoder_config(drop_path_rate=0.0, layer_scale_init_value=1e-2, **fx["cfg"])
    enc.text_adapter.add_type_embedding = enc.image_adapter.add_type_embedding = opts["add_type_embedding"]
    return SimpleNamespace(encoder=enc, **{k: opts[k] for k in ("attn_pooling", "use_pooler", "pooler_dropout", "head_scale_ratio",
                                                                 "use_image_features", "freeze_finetune_updates")})


def build(fx, case, check_shapes=True):
    """The mirror of the case's model with the generator's weights (synthetic, rounded to bf16 values), in eval mode as the generator."""
    from one_peace_amd.one_peace.one_peace_classify import OnePeaceClassifyModel
    opts = case["opts"]
    torch.manual_seed(0)
    m = OnePeaceClassifyModel(make_cfg(fx, opts), TinyDictionary(fx["vocab"]), case["head_type"], num_classes=fx["num_classes"],
                              use_two_images=opts["use_two_images"])
    own = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    if check_shapes:
        assert own == {k: tuple(v) for k, v in case["shapes"].items()}, sorted(set(own) ^ set(case["shapes"]))
    sd = {k: v.to(torch.bfloat16).float() for k, v in synth.synth_state_dict(own).items()}
    missing, unexpected = m.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.split(".")[-1] in synth.NON_SYNTH for k in missing), (missing, unexpected)
    return m.eval()


def inputs(fx, case, device="cpu", dtype=torch.float32):
    return {k: (fx["inputs"][k].to(device=device, dtype=dtype) if fx["inputs"][k].is_floating_point() else fx["inputs"][k].to(device))
            for k in case["inputs"]}


def stored_grads(model, stored):
    """(name, the model's gradient cut the way the fixture stores it, the stored tensor) for every stored entry but the norms."""
    params = dict(model.named_parameters())
    for key, want in stored.items():
        if key.endswith("#norm"):
            continue
        name = key.split("#")[0]
        g = params[name].grad
        assert g is not None, "no gradient for %s" % name
        yield key, (g[:16] if key.endswith("#rows16") else g), want


def rel_fro(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm())
