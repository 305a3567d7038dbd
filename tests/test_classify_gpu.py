"""one_peace_classify in bf16 on the MI355X against tests/golden/classify.pt: logits and head gradients of every fixture case, gated
per tensor by the reference's OWN bf16 error on the CPU (both sides of the gate come from the fixture):

    rel_fro(HIP path, fp32 fixture)  <=  2.5 x rel_fro(reference in bf16, fp32 fixture)

2.5 is the project's standing margin over a measured error (README, round 6).  The attention-pooling kernels must actually have run
(a spy on hip.attn_pool_fwd / hip.attn_pool_bwd); one classify_criterion backward and one hub extract_vl_features call run end to end."""
import dataclasses

import pytest
import torch

from tests import classify_util as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 2.5


class _Spy:
    def __init__(self):
        from one_peace_amd import hip
        self.hip, self.calls = hip, []
        self.fwd, self.bwd = hip.attn_pool_fwd, hip.attn_pool_bwd

    def __enter__(self):
        self.hip.attn_pool_fwd = lambda *a, **k: self.calls.append("fwd") or self.fwd(*a, **k)
        self.hip.attn_pool_bwd = lambda *a, **k: self.calls.append("bwd") or self.bwd(*a, **k)
        return self

    def __exit__(self, *exc):
        self.hip.attn_pool_fwd, self.hip.attn_pool_bwd = self.fwd, self.bwd


def _device_model(fx, case):
    return U.build(fx, case).to(DEV).to(torch.bfloat16).train()   # (every dropout of the fixture's configuration is 0)


@pytest.mark.parametrize("name", U.CASE_NAMES)
def test_hip_path_is_within_the_references_own_bf16_error(name):
    fx = U.fixture()
    case = fx["cases"][name]
    m = _device_model(fx, case)
    with _Spy() as spy:
        logits = m(**U.inputs(fx, case, DEV, torch.bfloat16))
        logits.backward(case["cotangent"].to(DEV))
        torch.cuda.synchronize()
    passes = (2 if case["opts"]["use_two_images"] else 1) if case["opts"]["attn_pooling"] else 0
    assert spy.calls.count("fwd") == passes and spy.calls.count("bwd") == passes, spy.calls
    rows = [("logits", U.rel_fro(logits, case["logits"]), U.rel_fro(case["bf16_logits"], case["logits"]))]
    for key, got, want in U.stored_grads(m, case["grads"]):
        if key.startswith("classify_head."):
            rows.append((key, U.rel_fro(got, want), U.rel_fro(case["bf16_grads"][key], want)))
    fails = []
    for what, mine, theirs in rows:
        print("%s %-58s hip %.3e  reference bf16 %.3e  ratio %.2f" % (name, what, mine, theirs, mine / theirs))
        if not mine <= MARGIN * theirs:
            fails.append((what, mine, theirs))
    assert len(rows) >= 7 and not fails, fails


def test_classify_criterion_backward_on_the_device():
    from one_peace_amd.criterions.finetune import ClassifyCriterion
    fx = U.fixture()
    case = fx["cases"]["al"]
    m = _device_model(fx, case)
    target = torch.tensor([1, 6, 3], device=DEV)
    sample = {"net_input": U.inputs(fx, case, DEV, torch.bfloat16), "target": target, "nsentences": 3}
    with _Spy() as spy:
        loss, sample_size, log = ClassifyCriterion(None, label_smoothing=0.1)(m, sample)
        loss.backward()
        torch.cuda.synchronize()
    assert spy.calls == ["fwd", "bwd"]
    want = torch.nn.functional.cross_entropy(case["logits"], target.cpu(), label_smoothing=0.1, reduction="sum")
    assert abs(float(loss.detach()) - float(want)) <= 5e-2 * float(want), (float(loss.detach()), float(want))
    q = m.classify_head.attn_pooling_func.q.grad
    assert q is not None and bool(torch.isfinite(q).all()) and float(q.float().abs().sum()) > 0


def test_hub_extract_vl_features_on_the_device(tmp_path):
    from one_peace_amd.one_peace import hub_interface as H
    fx = U.fixture()
    case = fx["cases"]["vl_two_images"]
    one = dict(case, opts=dict(case["opts"], use_two_images=False))   # extract_vl_features passes one image
    m = U.build(fx, one, check_shapes=False)
    path = tmp_path / "vl.pt"
    torch.save({"cfg": {"model": dict(encoder=dataclasses.asdict(m.cfg.encoder), attn_pooling=True, use_pooler=True)}, "model": m.state_dict()}, path)
    hub = H.from_pretrained(str(path), model_type="one_peace_classify", device=DEV, dtype="bf16", head_type="vl",
                            num_classes=fx["num_classes"], patch_image_size=64)
    inp = U.inputs(fx, one, DEV, torch.bfloat16)
    with torch.no_grad():
        want = m(src_tokens=inp["src_tokens"].cpu(), src_images=inp["src_images"].float().cpu())
    with _Spy() as spy:
        got = hub.extract_vl_features(inp["src_images"], inp["src_tokens"])
        torch.cuda.synchronize()
    assert spy.calls == ["fwd"] and got.dtype == torch.bfloat16 and tuple(got.shape) == (3, fx["num_classes"])
    assert U.rel_fro(got, want) <= 5e-2, U.rel_fro(got, want)   # (a smoke bound: the gate of this path is the test above)
