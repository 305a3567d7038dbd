"""Shared by tests/test_video_cpu.py and tests/test_video_gpu.py: the fixture tests/golden/video.pt
(tests/golden/make_video_golden.py) and the mirror OnePeaceVideoViT built with the fixture's arguments and weights."""
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "video.pt")
CASE_NAMES = ("tadapter1", "tadapter2")
_fx = None


def fixture():
    global _fx
    if _fx is None:
        _fx = torch.load(GOLDEN, map_location="cpu", weights_only=False)
    return _fx


def state_dict(fx, case):
    """The case's whole state dict in fp32: its own keys on top of the case it names as its base."""
    sd = dict(fx["cases"][case["base"]]["state_dict"]) if case["base"] else {}
    sd.update(case["state_dict"])
    return {k: (v.float() if v.is_floating_point() else v) for k, v in sd.items()}


def build(fx, case, **extra):
    """The mirror of the case's model with the fixture's weights (strict), in eval mode as the generator, fp32 on the CPU."""
    from one_peace_amd.one_peace_vision import OnePeaceVideoViT
    m = OnePeaceVideoViT(num_tadapter=case["num_tadapter"], **dict(fx["args"], **extra))
    m.load_state_dict(state_dict(fx, case), strict=True)
    return m.eval()


def run(m, fx, device="cpu", dtype=torch.float32):
    """The output [B, D, T, 1, 1] and the gradients of sum(cotangent * output), by the reference's parameter names."""
    out = m(fx["video"].to(device=device, dtype=dtype))
    (out * fx["cotangent"].to(device=device, dtype=dtype)).sum().backward()
    return out.detach(), {n: p.grad for n, p in m.named_parameters() if p.grad is not None}


def rel_fro(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm())
