"""OnePeaceVideoViT in bf16 on the MI355X against tests/golden/video.pt, gated per tensor by the reference's OWN bf16 error on the CPU
(both sides of the gate come from the fixture), the standing gate of tests/test_vision_gpu.py:

    rel_fro(HIP path, fp32 fixture)  <=  2.5 x rel_fro(reference in bf16, fp32 fixture)

The temporal attention kernels must actually have run, once per layer each (a spy on hip.attn_frames_fwd / hip.attn_frames_bwd), next
to the project's attention kernels for the spatial pass (with a frozen table: they take the bias as a constant); one training-mode
step with stochastic depth after freeze_for_adapters gives finite gradients for every trainable parameter and allocates none for a
frozen one.  Both errors of every row go to video_parity_report.txt in the tests' output directory (tests/util.py: OUT)."""
import os

import pytest
import torch

from tests import video_util as V
from tests.util import OUT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MARGIN = 2.5
REPORT = os.path.join(OUT, "video_parity_report.txt")
_report_started = []


class _Spy:
    NAMES = ("attn_frames_fwd", "attn_frames_bwd", "attn_fwd", "attn_bwd_launch")

    def __init__(self):
        from one_peace_amd import hip
        self.hip, self.calls = hip, []
        self.real = {n: getattr(hip, n) for n in self.NAMES}

    def _wrap(self, name):
        return lambda *a, **k: self.calls.append(name) or self.real[name](*a, **k)

    def __enter__(self):
        for n in self.NAMES:
            setattr(self.hip, n, self._wrap(n))
        return self

    def __exit__(self, *exc):
        for n in self.NAMES:
            setattr(self.hip, n, self.real[n])

    def count(self, name):
        return sum(c == name for c in self.calls)


TABLE = "image_adapter.rel_pos_table.weight"


@pytest.mark.parametrize("table", ["trained", "frozen"])
@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_hip_path_is_within_the_references_own_bf16_error(name, table):
    """table = "trained": the fixture's state, every parameter trainable -- the spatial scores + bias product of each layer then runs as
    torch ops (the kernels take the bias as a constant) and the table's gradient is gated like the rest.  table = "frozen": the
    reference's fine-tuning state for that tensor -- the project's attention kernels run the spatial pass; the same gates without the
    table's row."""
    fx = V.fixture()
    case = fx["cases"][name]
    layers = fx["args"]["layers"]
    m = V.build(fx, case).to(DEV).to(torch.bfloat16)
    if table == "frozen":
        m.image_adapter.rel_pos_table_list[0].weight.requires_grad = False
    with _Spy() as spy:
        out, grads = V.run(m, fx, DEV, torch.bfloat16)
        torch.cuda.synchronize()
    spatial = layers if table == "frozen" else 0
    assert [spy.count(n) for n in _Spy.NAMES] == [layers, layers, spatial, spatial], spy.calls   # each kernel pair once per layer
    want_grads = {k: v for k, v in case["grads"].items() if not (table == "frozen" and k == TABLE)}
    assert TABLE in case["grads"] and (TABLE in grads) == (table == "trained")
    rows = [("output", V.rel_fro(out, case["output"]), V.rel_fro(case["bf16_output"], case["output"]))]
    for key, want in want_grads.items():
        rows.append((key, V.rel_fro(grads[key], want), V.rel_fro(case["bf16_grads"][key], want)))
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    fails = []
    with open(REPORT, "a" if _report_started else "w") as f:   # one report per session
        _report_started.append(True)
        for what, mine, theirs in rows:
            line = "%-10s %-8s %-44s hip %.3e  reference bf16 %.3e  ratio %.2f" % (name, table, what, mine, theirs, mine / theirs)
            print(line)
            f.write(line + "\n")
            if not mine <= MARGIN * theirs:
                fails.append((what, mine, theirs))
    assert len(rows) == 1 + len(want_grads) and len(rows) >= 12 and not fails, fails


def test_training_step_after_freezing_trains_the_adapters_only():
    from one_peace_amd.one_peace_vision import VideoRecognizer, freeze_for_adapters
    fx = V.fixture()
    case = fx["cases"]["tadapter2"]
    layers = fx["args"]["layers"]
    rec = VideoRecognizer(V.build(fx, case, drop_path_rate=0.2), num_classes=5).to(DEV).to(torch.bfloat16).train()
    kept = set(freeze_for_adapters(rec))
    torch.manual_seed(0)
    with _Spy() as spy:
        scores = rec(fx["video"].to(DEV, torch.bfloat16))
        loss = torch.nn.functional.cross_entropy(scores.float(), torch.tensor([1, 3], device=DEV))
        loss.backward()
        torch.cuda.synchronize()
    assert [spy.count(n) for n in _Spy.NAMES] == [layers] * 4, spy.calls
    assert bool(torch.isfinite(loss))
    for n, p in rec.named_parameters():
        if n in kept:
            assert p.grad is not None, n
            assert bool(torch.isfinite(p.grad.float()).all()), n
        else:
            assert p.grad is None, n
    assert any("T_Adapter_in" in n for n in kept) and any(float(p.grad.float().abs().max()) > 0 for n, p in rec.named_parameters()
                                                           if "T_Adapter." in n)
