"""Shared by tests/test_det_cpu.py and tests/test_det_gpu.py: the fixture tests/golden/det.pt (tests/golden/make_det_golden.py) and
the mirror OnePeaceDetViT built with the fixture's arguments and weights."""
import os

import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "det.pt")
BUCKETS = ("image_adapter.rp_bucket", "image_adapter.rp_bucket_window")
_fx = None


def fixture():
    global _fx
    if _fx is None:
        _fx = torch.load(GOLDEN, map_location="cpu", weights_only=False)
    return _fx


def image(fx):
    up = fx["upsample"]
    return fx["image_small"].repeat_interleave(up, dim=2).repeat_interleave(up, dim=3)


def cotangent(fx):
    up = fx["cotangent_upsample"]
    return fx["cotangent_small"].repeat_interleave(up, dim=2).repeat_interleave(up, dim=3)


def state_dict(fx, model):
    """The reference's state dict in fp32.  The fixture leaves out the two integer bucket matrices (8.5 MB); they are the model's own
    here, after the fixture's rows and sums of them were compared (tests/test_det_cpu.py does that on its own too)."""
    sd = {k: v.float() for k, v in fx["state_dict"].items()}
    for k in BUCKETS:
        own = model.state_dict()[k]
        for i, row in fx["bucket_rows"][k].items():
            assert torch.equal(own[i], row.long()), (k, i)
        assert int(own.sum()) == fx["bucket_sums"][k], k
        sd[k] = own
    return sd


def build(fx, **extra):
    """The mirror with the fixture's weights (strict), in eval mode as the generator, fp32 on the CPU."""
    from one_peace_amd.one_peace_vision import OnePeaceDetViT
    m = OnePeaceDetViT(**dict(fx["args"], **extra))
    m.load_state_dict(state_dict(fx, m), strict=True)
    return m.eval()


def run(m, fx, device="cpu", dtype=torch.float32):
    """The output [B, D, Hg, Wg] and the gradients of sum(cotangent * output), by parameter name."""
    out = m(image(fx).to(device=device, dtype=dtype))["last_feat"]
    (out * cotangent(fx).to(device=device, dtype=dtype)).sum().backward()
    return out.detach(), {n: p.grad for n, p in m.named_parameters() if p.grad is not None}


def rel_fro(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm())
