"""OnePeaceViT in bf16 on the MI355X against tests/golden/vision.pt, gated per tensor by the reference's OWN bf16 error on the CPU (both
sides of the gate come from the fixture), the project's standing gate of tests/test_classify_gpu.py:

    rel_fro(HIP path, fp32 fixture)  <=  2.5 x rel_fro(reference in bf16, fp32 fixture)

The mean-pool kernels must actually have run (a spy on hip.token_mean_ln_fwd / hip.token_mean_ln_bwd); one training-mode step with
stochastic depth gives finite gradients for every parameter.  Both errors of every row go to vision_parity_report.txt in the tests' output
directory (tests/util.py: OUT)."""
import os

import pytest
import torch

from tests import vision_util as V
from tests.util import OUT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 2.5
REPORT = os.path.join(OUT, "vision_parity_report.txt")
_report_started = []


class _Spy:
    def __init__(self):
        from one_peace_amd import hip
        self.hip, self.calls = hip, []
        self.fwd, self.bwd = hip.token_mean_ln_fwd, hip.token_mean_ln_bwd

    def __enter__(self):
        self.hip.token_mean_ln_fwd = lambda *a, **k: self.calls.append("fwd") or self.fwd(*a, **k)
        self.hip.token_mean_ln_bwd = lambda *a, **k: self.calls.append("bwd") or self.bwd(*a, **k)
        return self

    def __exit__(self, *exc):
        self.hip.token_mean_ln_fwd, self.hip.token_mean_ln_bwd = self.fwd, self.bwd


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_hip_path_is_within_the_references_own_bf16_error(name):
    fx = V.fixture()
    case = fx["cases"][name]
    m = V.build(fx, case).to(DEV).to(torch.bfloat16)
    with _Spy() as spy:
        logits, grads = V.run(m, fx, DEV, torch.bfloat16)
        torch.cuda.synchronize()
    assert spy.calls == (["fwd", "bwd"] if case["global_pool"] else []), spy.calls
    rows = [("logits", V.rel_fro(logits, case["logits"]), V.rel_fro(case["bf16_logits"], case["logits"]))]
    for key, want in case["grads"].items():
        rows.append((key, V.rel_fro(grads[key], want), V.rel_fro(case["bf16_grads"][key], want)))
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    fails = []
    with open(REPORT, "a" if _report_started else "w") as f:   # one report per session
        _report_started.append(True)
        for what, mine, theirs in rows:
            line = "%-12s %-28s hip %.3e  reference bf16 %.3e  ratio %.2f" % (name, what, mine, theirs, mine / theirs)
            print(line)
            f.write(line + "\n")
            if not mine <= MARGIN * theirs:
                fails.append((what, mine, theirs))
    assert len(rows) == (5 if case["global_pool"] else 4) and not fails, fails


@pytest.mark.parametrize("use_checkpoint", [False, True], ids=["keep", "recompute"])
def test_head_dim_64_runs_the_encoders_fused_layers(use_checkpoint):
    """The four g factories have head_dim 64: there the encoder's fused HIP layers run (the fixture's head_dim is 16, which takes the
    layers' torch ops).  A 2-layer model of that head size against ITSELF in fp32 on the CPU; 5e-2 is the smoke bound of
    tests/test_classify_gpu.py for one bf16 pass (2^-8 per rounding, a few dozen roundings deep), the gate of the head is the test above.
    use_checkpoint=True: the same forward + backward through the fused layers' activation recompute, under the same bound."""
    from one_peace_amd.one_peace_vision import OnePeaceViT
    from one_peace_amd.transformer.transformer_layer import TransformerEncoderLayer
    fx = V.fixture()
    torch.manual_seed(5)
    m = OnePeaceViT(**dict(fx["args"], embed_dim=128, ffn_embed_dim=256, attention_heads=2, init_scale=1.0, use_checkpoint=use_checkpoint)).eval()
    with torch.no_grad():
        m.image_adapter.rel_pos_table_list[0].weight.normal_(std=0.02)
        for p in m.parameters():
            p.copy_(p.to(torch.bfloat16).float())
    want, want_grads = V.run(m, fx)
    want_grads = {n: g.clone() for n, g in want_grads.items()}
    m.zero_grad(set_to_none=True)
    m = m.to(DEV).to(torch.bfloat16)
    ran, fused = [], TransformerEncoderLayer.forward_fused
    TransformerEncoderLayer.forward_fused = lambda self, *a, **k: ran.append(1) or fused(self, *a, **k)
    try:
        with _Spy() as spy:
            got, grads = V.run(m, fx, DEV, torch.bfloat16)
            torch.cuda.synchronize()
    finally:
        TransformerEncoderLayer.forward_fused = fused
    assert len(ran) == 2 and spy.calls == ["fwd", "bwd"]
    assert V.rel_fro(got, want) <= 5e-2, V.rel_fro(got, want)
    for n in ("head.weight", "fc_norm.weight", "image_adapter.pos_embed"):
        assert V.rel_fro(grads[n], want_grads[n]) <= 5e-2, (n, V.rel_fro(grads[n], want_grads[n]))


def test_training_step_with_stochastic_depth_gives_finite_gradients():
    fx = V.fixture()
    case = fx["cases"]["global_pool"]
    m = V.build(fx, case, drop_path_rate=0.2).to(DEV).to(torch.bfloat16).train()
    torch.manual_seed(0)
    with _Spy() as spy:
        logits = m(fx["images"].to(DEV, torch.bfloat16))
        loss = torch.nn.functional.cross_entropy(logits.float(), torch.tensor([1, 3], device=DEV))
        loss.backward()
        torch.cuda.synchronize()
    assert spy.calls == ["fwd", "bwd"]
    assert bool(torch.isfinite(loss))
    for n, p in m.named_parameters():
        assert p.grad is not None, n
        assert bool(torch.isfinite(p.grad.float()).all()), n
