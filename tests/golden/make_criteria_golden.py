"""Generate tests/golden/criteria.pt from the UNMODIFIED reference criteria (one_peace/criterions/classify_loss.py: ClassifyCriterion,
one_peace/criterions/hinge_loss.py: HingeLoss), run on CPU through oracle/ref_shim.py.

    python tests/golden/make_criteria_golden.py      # needs the reference tree; writes criteria.pt

The model is a stub that returns a leaf logits tensor, so `logits.grad` after `loss.backward()` is the reference's gradient.  The
shim's fairseq.utils has no `item` (only reduce_metrics reads it, which is not run here).  one_peace/criterions/refcoco_loss.py
imports torchvision, which this environment does not have: RefCOCOCriterion gets NO reference fixture, and the box loss is pinned in
the tests to an fp64 statement of the published formula instead.

Cases (each: inputs, loss, n_correct, sample_size, the logging keys, logits.grad; tensors and plain numbers only).
  hard_eps0_f32, hard_eps01_f32, hard_eps0_bf16, hard_eps01_bf16: class targets [B] with one -100 (ignore_index), label smoothing 0 / 0.1.
  soft_f32: soft targets [B, C] whose rows sum to 0, 0.3, 2.5 and to arbitrary values (VQA scores do not sum to 1).
  multi_f32: multi-label 0 / 1 targets.
  hinge_m1, hinge_m3: logits [B, 4] on a grid of 1/4, so that 1 + x_k - x_target is exactly 0 for some k (0.5 subgradients) and some
    maxima tie.  hinge_m3 is the reference constructed with margin = 3.0: it records the same numbers as hinge_m1, which shows the
    reference ignoring its `margin` option.
"""
import importlib
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim as R  # noqa: E402


class Stub(torch.nn.Module):
    """Returns its leaf logits whatever it is called with; records the keyword arguments."""

    def __init__(self, logits):
        super().__init__()
        self.logits = logits.clone().requires_grad_(True)
        self.seen = None

    def forward(self, **kw):
        self.seen = kw
        return self.logits


def run(criterion, logits, sample):
    model = Stub(logits)
    loss, sample_size, log = criterion(model, sample)
    loss.backward()
    assert sorted(log) == ["loss", "n_correct", "nsentences", "sample_size"]
    assert float(log["loss"]) == float(loss.detach()) and log["nsentences"] == sample["nsentences"] and log["sample_size"] == sample_size
    return model, {"logits": logits, "target": sample["target"], "nsentences": sample["nsentences"], "loss": loss.detach(),
                   "n_correct": log["n_correct"].detach(), "sample_size": sample_size, "grad": model.logits.grad.clone()}


def main():
    R.install()
    ClassifyCriterion = importlib.import_module("one_peace.criterions.classify_loss").ClassifyCriterion
    HingeLoss = importlib.import_module("one_peace.criterions.hinge_loss").HingeLoss
    g = torch.Generator().manual_seed(31)
    out = {}

    B, C = 13, 37
    logits = (torch.randn(B, C, generator=g) * 3).to(torch.bfloat16).float()  # bf16-representable: the bf16 cases see the same values
    hard = torch.randint(0, C, (B,), generator=g)
    hard[:6] = logits[:6].argmax(1)
    hard[4] = -100
    for eps, ename in ((0.0, "eps0"), (0.1, "eps01")):
        for dt, dname in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
            crit = ClassifyCriterion(None, use_multi_label=False, label_smoothing=eps)
            _, case = run(crit, logits.to(dt), {"net_input": {"src_tokens": torch.zeros(B, 1)}, "target": hard, "nsentences": B})
            case["label_smoothing"] = eps
            out["hard_%s_%s" % (ename, dname)] = case
            assert float(case["grad"][4].abs().sum()) == 0.0

    soft = torch.rand(B, C, generator=g) * (torch.rand(B, C, generator=g) < 0.2)
    soft[0] = 0.0
    soft[1] = 0.0
    soft[1, 3], soft[1, 20] = 0.25, 0.05
    soft[2] = 0.0
    soft[2, 0], soft[2, 7], soft[2, 36] = 1.0, 1.0, 0.5
    assert float(soft[0].sum()) == 0.0 and abs(float(soft[1].sum()) - 0.3) < 1e-6 and float(soft[2].sum()) == 2.5
    _, out["soft_f32"] = run(ClassifyCriterion(None), logits, {"net_input": {}, "target": soft, "nsentences": B})

    multi = (torch.rand(B, C, generator=g) < 0.15).float()
    _, out["multi_f32"] = run(ClassifyCriterion(None, use_multi_label=True), logits, {"net_input": {}, "target": multi, "nsentences": B})

    nb, K = 11, 4
    hl = torch.randint(-8, 9, (nb, K), generator=g).float() / 4
    ht = torch.randint(0, K, (nb,), generator=g)
    hl[0] = torch.tensor([0.5, 1.5, 1.5, -0.25])   # 1 + x_0 - x_t = 0 for t = 1: a 0.5 subgradient; tied maxima, the lower index wins
    ht[0] = 1
    hl[1] = torch.tensor([2.0, 1.0, 2.0, 1.0])     # t = 2: arg-max is 0 (tie), so not counted; two exact zeros
    ht[1] = 2
    hl[2] = torch.tensor([-1.0, 0.0, -2.0, -1.0])  # t = 1 is the arg-max; 1 + x_k - x_t = 0 for k = 0 and k = 3
    ht[2] = 1
    ni = {"src_tokens": torch.zeros(nb * K, 3, dtype=torch.long), "src_audios": torch.arange(nb * 5.0).view(nb, 5),
          "audio_padding_masks": torch.zeros(nb, 5, dtype=torch.bool)}
    for margin, name in ((1.0, "hinge_m1"), (3.0, "hinge_m3")):
        model, case = run(HingeLoss(None, margin=margin, num_choices=K), hl.view(-1, 1), {"net_input": ni, "target": ht, "nsentences": nb})
        assert model.seen["src_audios"].shape == (nb * K, 5) and torch.equal(model.seen["src_audios"][K], ni["src_audios"][1])
        case["net_input"], case["margin"], case["num_choices"] = ni, margin, K
        out[name] = case
    assert torch.equal(out["hinge_m1"]["loss"], out["hinge_m3"]["loss"]) and torch.equal(out["hinge_m1"]["grad"], out["hinge_m3"]["grad"])
    assert float((out["hinge_m1"]["grad"] == 0.5).sum()) >= 3  # the exact zeros are there

    torch.save(out, os.path.join(HERE, "criteria.pt"))
    for k, v in out.items():
        print(k, "loss", float(v["loss"]), "n_correct", float(v["n_correct"]), "sample_size", v["sample_size"])


if __name__ == "__main__":
    main()
