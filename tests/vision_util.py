"""Shared by tests/test_vision_cpu.py and tests/test_vision_gpu.py: the fixture tests/golden/vision.pt
(tests/golden/make_vision_golden.py) and the mirror OnePeaceViT built with the fixture's arguments and weights."""
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "vision.pt")
CASE_NAMES = ("global_pool", "cls_token")
_fx = None


def fixture():
    global _fx
    if _fx is None:
        _fx = torch.load(GOLDEN, map_location="cpu", weights_only=False)
    return _fx


def build(fx, case, **extra):
    """The mirror of the case's model with the fixture's weights (strict), in eval mode as the generator, fp32 on the CPU."""
    from one_peace_amd.one_peace_vision import OnePeaceViT
    m = OnePeaceViT(global_pool=case["global_pool"], **dict(fx["args"], **extra))
    m.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in case["state_dict"].items()}, strict=True)
    return m.eval()


def run(m, fx, device="cpu", dtype=torch.float32):
    """Logits and the gradients of sum(cotangent * logits), by the reference's parameter names."""
    logits = m(fx["images"].to(device=device, dtype=dtype))
    (logits * fx["cotangent"].to(device=device, dtype=dtype)).sum().backward()
    return logits.detach(), {n: p.grad for n, p in m.named_parameters() if p.grad is not None}


def rel_fro(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm())
