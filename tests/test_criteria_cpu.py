"""The fine-tuning criteria on the torch path (CPU): ClassifyCriterion / HingeLoss against the UNMODIFIED reference's recorded results
(tests/golden/criteria.pt, made by tests/golden/make_criteria_golden.py), RefCOCOCriterion / ops.box_loss against an fp64 statement of
the published formula (the reference's refcoco_loss.py needs torchvision, which is not available: no fixture), the refusals of
op_row_loss / op_box_loss before any launch, and the static checks of csrc/losses.hip.

Where the torch route is the same sequence of torch calls as the reference (every classify mode, hinge at margin 1) the results are
compared bitwise.  The fp64 statements and the error units of this file are shared with tests/test_criteria_gpu.py.

Error units.  u = 2^-24 (half an fp32 ulp at 1) times a scale:
  a row loss: the sum of the absolute values of the terms summed for that row -- for a cross-entropy sum_c |t_c| (|lse| + |x_c|) with t the
    (smoothed) target row, for the multi-label loss sum_c max(x, 0) + |x t| + log1p(exp(-|x|)), for the hinge sum_k |margin| + |x_k| + |x_t|;
  a gradient entry: max(1, sum_c |t_c|) for the cross-entropies (entries are p_c sum t - t_c), 1 for the multi-label loss (sigmoid - t);
  the boxes: |loss| for the loss, the case's largest |fp64 gradient| for a gradient entry.
A row loss's unit also has the absolute floor C 2^-126 (see `units`)."""
import math
import os
import shutil
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "criteria.pt")
U = 2.0 ** -24
HARD, SOFT, MULTI, HINGE = 0, 1, 2, 3


class Stub(torch.nn.Module):
    """A model that returns its leaf logits whatever it is called with."""

    def __init__(self, logits):
        super().__init__()
        self.logits = logits.clone().requires_grad_(True)
        self.seen = None

    def forward(self, **kw):
        self.seen = kw
        return self.logits


# ---- fp64 statements of the formulae (host), with the scales of the error units ------------------------------------------------
def smoothed_targets(targets, C, eps):
    """[B, C] fp64: (1 - eps) one-hot + eps / C (torch's label smoothing); a zero row for ignore_index -100."""
    keep = targets != -100
    t = torch.zeros(targets.shape[0], C, dtype=torch.float64)
    t[keep] = eps / C
    t[keep, targets[keep]] += 1.0 - eps
    return t


def rows_fp64(mode, x, targets, eps=0.0, margin=1.0):
    """x [B, C] (any float dtype, taken as the values it holds), targets as the mode wants them.  Returns fp64 tensors
    (row_loss [B], row_correct [B], grad [B, C], loss_scale [B], grad_scale [B])."""
    x = x.detach().double().requires_grad_(True)
    B, C = x.shape
    first_max = x.detach().argmax(1)  # torch: the lowest index among equal maxima
    if mode in (HARD, SOFT):
        t = smoothed_targets(targets, C, eps) if mode == HARD else targets.double()
        lse = torch.logsumexp(x, dim=1, keepdim=True)
        loss = (t * (lse - x)).sum(1)
        correct = (first_max == targets).double() if mode == HARD else ((x - lse).exp() * t).sum(1).detach()
        lscale = (t.abs() * (lse.abs() + x.abs())).sum(1).detach()
        gscale = t.abs().sum(1).clamp(min=1.0)
    elif mode == MULTI:
        t = targets.double()
        soft = torch.log1p(torch.exp(-x.abs()))
        loss = (torch.logaddexp(x, torch.zeros_like(x)) - x * t).sum(1)  # = max(x, 0) + log1p(exp(-|x|)) - x t, smooth at 0 for autograd
        correct = t.gather(1, first_max[:, None])[:, 0]
        lscale = (x.clamp(min=0) + (x * t).abs() + soft).sum(1).detach()
        gscale = torch.ones(B, dtype=torch.float64)
    else:
        xt = x.gather(1, targets[:, None])
        loss = torch.max(torch.zeros((), dtype=torch.float64), margin + x - xt).sum(1)  # torch.max(tensor, tensor): 0.5 / 0.5 at a tie
        correct = (first_max == targets).double()
        lscale = (abs(margin) + x.abs() + xt.abs()).sum(1).detach()
        gscale = torch.ones(B, dtype=torch.float64)
    (grad,) = torch.autograd.grad(loss.sum(), x)
    return loss.detach(), correct, grad, lscale, gscale


def rows_reference_fp32(mode, x, targets, eps=0.0, margin=1.0):
    """The reference's own fp32 arithmetic on the host, per row: (row_loss, row_correct, grad), fp32."""
    x = x.detach().float().requires_grad_(True)
    if mode == HARD:
        loss = F.cross_entropy(x, targets, label_smoothing=eps, reduction="none")
        correct = x.detach().argmax(1).eq(targets).float()
    elif mode == SOFT:
        lp = F.log_softmax(x, dim=-1, dtype=torch.float32)  # fairseq's utils.log_softmax
        loss = (-targets.float() * lp).sum(1)
        correct = (lp.exp() * targets.float()).sum(1).detach()
    elif mode == MULTI:
        loss = F.binary_cross_entropy_with_logits(x, targets.float(), reduction="none").sum(1)
        correct = targets.float().gather(1, x.detach().argmax(1, keepdim=True))[:, 0]
    else:
        loss = torch.max(torch.tensor(0.0), margin + x - x.gather(1, targets[:, None])).sum(1)
        correct = x.detach().argmax(1).eq(targets).float()
    (grad,) = torch.autograd.grad(loss.sum(), x)
    return loss.detach(), correct, grad


def units(got, want, scale, terms=1):
    """The worst |got - want| in units of 2^-24 scale + terms 2^-126 (entries whose scale is 0 must be exact).  The second part is the
    floor of the format: each of the `terms` summed for an entry may be below fp32's smallest normal number, 2^-126, where fp32 has no
    relative precision left (exp(-|x|) at |x| > 87); it only matters for saturated rows whose whole loss is of that size."""
    err = (got.double() - want.double()).abs()
    scale = scale.double().expand_as(err) if scale.dim() == err.dim() else scale.double()[:, None].expand_as(err)
    zero = scale == 0
    assert bool((err[zero] == 0).all()), "an entry whose scale is 0 must be exact"
    if bool(zero.all()):
        return 0.0
    return float((err[~zero] / (U * scale[~zero] + terms * 2.0 ** -126)).max())


def box_loss_fp64(logits, targets):
    """refcoco_loss.py:36-46 with torchvision's generalized_box_iou written out for the diagonal, in fp64.  Returns (loss, valid rows,
    d loss / d logits); with no valid row the loss is NaN and the gradient is that of the L1 term."""
    x = logits.detach().double().requires_grad_(True)
    t = targets.double()
    o = x.sigmoid()
    l1 = (o - t).abs().sum() / x.shape[0]
    valid = (o[:, :2] < o[:, 2:]).all(1)
    a, b = o[valid], t[valid]
    area1 = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1])
    area2 = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(a[:, 2:], b[:, 2:]) - torch.max(a[:, :2], b[:, :2])).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]
    union = area1 + area2 - inter
    whi = (torch.max(a[:, 2:], b[:, 2:]) - torch.min(a[:, :2], b[:, :2])).clamp(min=0)
    areai = whi[:, 0] * whi[:, 1]
    giou = inter / union - (areai - union) / areai
    nv = int(valid.sum())
    loss = l1 + (1 - giou).mean()
    (grad,) = torch.autograd.grad(loss if nv else l1, x)
    return loss.detach(), nv, grad


def box_case(B, seed, dtype=torch.float32):
    """(logits [B, 4] holding values `dtype` represents, targets fp32 [B, 4]): every side of every box >= 0.05; about a third of the
    predicted boxes have x1 > x2 or y1 > y2 (invalid rows); row 0 (B >= 5) ties the target's corner exactly (sigmoid(0) = 0.5)."""
    g = torch.Generator().manual_seed(seed)

    def boxes(n):
        lo = 0.05 + 0.55 * torch.rand(n, 2, generator=g)
        side = 0.05 + 0.3 * torch.rand(n, 2, generator=g)
        return torch.cat([lo, lo + side], 1)
    o, t = boxes(B), boxes(B)
    if B > 1:
        flip = torch.rand(B, generator=g) < 0.33
        flip[1] = True
        o[flip] = o[flip][:, [2, 1, 0, 3]]  # x1 > x2 by the same side
    logits = torch.log(o / (1 - o)).to(dtype).float()
    if B >= 5:
        logits[0] = torch.tensor([0.0, 0.0, 2.0, 1.0])
        t[0] = torch.tensor([0.5, 0.5, 0.9, 0.7])
    return logits.to(dtype), t


# ---- the tests ------------------------------------------------------------------------------------------------------------------
def test_the_three_criteria_are_registered():
    from one_peace_amd import criterions, registry  # noqa: F401
    from one_peace_amd.criterions import finetune
    assert registry.CRITERION_REGISTRY["classify_criterion"] is finetune.ClassifyCriterion
    assert registry.CRITERION_REGISTRY["hinge_loss"] is finetune.HingeLoss
    assert registry.CRITERION_REGISTRY["refcoco_criterion"] is finetune.RefCOCOCriterion
    for cls in (finetune.ClassifyCriterion, finetune.HingeLoss, finetune.RefCOCOCriterion):
        assert cls.logging_outputs_can_be_summed() is True
        cls.reduce_metrics([{"loss": 1.0, "nsentences": 2, "sample_size": 2, "n_correct": 1}])  # a no-op without fairseq.metrics


CLASSIFY_CASES = ["hard_eps0_f32", "hard_eps0_bf16", "hard_eps01_f32", "hard_eps01_bf16", "soft_f32", "multi_f32"]


@pytest.mark.parametrize("name", CLASSIFY_CASES)
def test_classify_criterion_torch_route_reproduces_the_reference_bitwise(name):
    from one_peace_amd import ops
    from one_peace_amd.criterions.finetune import ClassifyCriterion
    case = torch.load(GOLDEN)[name]
    crit = ClassifyCriterion(None, use_multi_label=name.startswith("multi"), label_smoothing=case.get("label_smoothing", 0.0))
    model = Stub(case["logits"])
    loss, sample_size, log = crit(model, {"net_input": {"src_tokens": torch.zeros(1)}, "target": case["target"], "nsentences": case["nsentences"]})
    loss.backward()
    assert sorted(log) == ["loss", "n_correct", "nsentences", "sample_size"]
    assert sample_size == case["sample_size"] == log["sample_size"] == log["nsentences"] == 13
    assert loss.dtype == case["loss"].dtype and torch.equal(loss.detach(), case["loss"]) and torch.equal(log["loss"], case["loss"])
    assert log["n_correct"].dtype == case["n_correct"].dtype and torch.equal(log["n_correct"], case["n_correct"])
    assert torch.equal(model.logits.grad, case["grad"])  # the same sequence of torch calls
    # and the recorded numbers are the formula: fp64 on the same values
    mode = MULTI if name.startswith("multi") else (SOFT if name.startswith("soft") else HARD)
    l64, c64, g64, lscale, gscale = rows_fp64(mode, case["logits"], case["target"], eps=case.get("label_smoothing", 0.0))
    if case["logits"].dtype == torch.float32:
        assert abs(float(case["loss"]) - float(l64.sum())) <= 8 * U * float(lscale.sum())
        assert units(case["grad"], g64, gscale) <= 8
        assert abs(float(case["n_correct"]) - float(c64.sum())) <= 8 * U * max(1.0, float(c64.sum()))
    l2, c2 = ops.classify_loss(case["logits"], case["target"], name.startswith("multi"), case.get("label_smoothing", 0.0))
    assert torch.equal(l2, case["loss"]) and torch.equal(c2, case["n_correct"])


def test_hinge_loss_equals_the_reference_at_margin_1_and_honours_margin_3():
    from one_peace_amd.criterions.finetune import HingeLoss
    fx = torch.load(GOLDEN)
    m1, m3 = fx["hinge_m1"], fx["hinge_m3"]
    assert m3["margin"] == 3.0 and torch.equal(m1["loss"], m3["loss"]) and torch.equal(m1["grad"], m3["grad"])  # the reference ignores it
    K = m1["num_choices"]
    sample = {"net_input": m1["net_input"], "target": m1["target"], "nsentences": m1["nsentences"]}
    model = Stub(m1["logits"])
    loss, sample_size, log = HingeLoss(None, margin=1.0, num_choices=K)(model, sample)
    loss.backward()
    assert sorted(log) == ["loss", "n_correct", "nsentences", "sample_size"] and sample_size == m1["sample_size"] == 11
    assert torch.equal(loss.detach(), m1["loss"]) and torch.equal(log["n_correct"], m1["n_correct"])
    assert torch.equal(model.logits.grad, m1["grad"]) and float((model.logits.grad == 0.5).sum()) >= 3
    # repeat_interleave of the audio inputs, the tokens as they are
    assert sorted(model.seen) == ["audio_padding_masks", "src_audios", "src_tokens"]
    assert torch.equal(model.seen["src_audios"], m1["net_input"]["src_audios"].repeat_interleave(K, 0))
    assert torch.equal(model.seen["audio_padding_masks"], m1["net_input"]["audio_padding_masks"].repeat_interleave(K, 0))
    assert model.seen["src_tokens"] is m1["net_input"]["src_tokens"]
    # margin 3: the fp64 statement with 3 (logits on a grid of 1/4: every sum is exact in fp32)
    x = m1["logits"].view(-1, K)
    l64, c64, g64, _, _ = rows_fp64(HINGE, x, m1["target"], margin=3.0)
    model = Stub(m1["logits"])
    loss3, _, log3 = HingeLoss(None, margin=3.0, num_choices=K)(model, sample)
    loss3.backward()
    assert float(loss3.detach()) == float(l64.sum()) and float(loss3.detach()) != float(m1["loss"])
    assert torch.equal(model.logits.grad.view(-1, K).double(), g64) and float(log3["n_correct"]) == float(c64.sum())


@pytest.mark.parametrize("B", [1, 5, 67])
def test_box_loss_torch_route_against_fp64_autograd(B):
    from one_peace_amd import ops
    from one_peace_amd.criterions.finetune import RefCOCOCriterion
    logits, targets = box_case(B, seed=100 + B)
    want, nv, g64 = box_loss_fp64(logits, targets)
    assert nv == B if B == 1 else 0 < nv < B
    model = Stub(logits)
    loss, sample_size, log = RefCOCOCriterion(None)(model, {"net_input": {"src_tokens": torch.zeros(1)}, "target": targets, "nsentences": B})
    loss.backward()
    assert sample_size == 1 and sorted(log) == ["loss", "nsentences", "sample_size"] and log["sample_size"] == 1 and log["nsentences"] == B
    assert torch.equal(log["loss"], loss.detach()) and torch.equal(loss.detach(), ops.box_loss(logits, targets))
    # fp32 against fp64: a few units of 2^-24 |loss| per operation of a short chain, and of the largest gradient
    assert abs(float(loss.detach()) - float(want)) <= 16 * U * abs(float(want))
    assert float((model.logits.grad.double() - g64).abs().max()) <= 16 * U * float(g64.abs().max())


def test_box_loss_without_a_valid_row_is_nan_with_the_l1_gradient_and_zero_at_equality():
    from one_peace_amd import ops
    logits = torch.tensor([[1.0, 0.0, -1.0, 2.0], [0.5, 1.0, 0.25, -1.0]], requires_grad=True)  # x1 > x2; y1 > y2
    targets = torch.tensor([[0.1, 0.2, 0.6, 0.7], [0.3, 0.1, 0.9, 0.5]])
    loss = ops.box_loss(logits, targets)
    assert math.isnan(float(loss))
    want, nv, g64 = box_loss_fp64(logits, targets)
    assert nv == 0 and math.isnan(float(want))
    o = logits.detach().sigmoid()
    l1 = ((logits.sigmoid() - targets).abs().sum() / 2)
    (g,) = torch.autograd.grad(l1, logits)
    assert float((g.double() - g64).abs().max()) <= 4 * U and float(g.abs().min()) > 0
    assert torch.equal(g, torch.sign(o - targets) * o * (1 - o) / 2)
    # o == t: sign(0) = 0
    x = torch.zeros(1, 4, requires_grad=True)
    loss = ops.box_loss(x, torch.full((1, 4), 0.5))
    assert math.isnan(float(loss))  # a degenerate box is not a valid row
    _, _, g64 = box_loss_fp64(x, torch.full((1, 4), 0.5))
    assert float(g64.abs().max()) == 0.0
    with pytest.raises(ValueError, match=r"\[B, 4\]"):
        ops.box_loss(torch.zeros(3, 5), torch.zeros(3, 5))


def test_refcoco_criterion_divides_the_l1_term_by_nsentences():
    from one_peace_amd import ops
    from one_peace_amd.criterions.finetune import RefCOCOCriterion
    logits, targets = box_case(5, seed=3)
    loss, _, _ = RefCOCOCriterion(None)(Stub(logits), {"net_input": {}, "target": targets, "nsentences": 10})
    l1 = float((logits.sigmoid() - targets).abs().sum())
    assert abs(float(loss) - (float(ops.box_loss(logits, targets)) - l1 / 5 + l1 / 10)) <= 1e-6


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("onepeace_build", os.path.join(ROOT, "one-peace_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from one_peace_amd import hip
    return hip.lib()


def test_loss_entry_points_reject_bad_arguments_before_any_launch(lib):
    fake = 1 << 20  # never dereferenced: validation comes first

    def row(logits=fake, dtype=0, ld=7, targets=fake, tdt=1, ldt=7, B=5, C=7, mode=0, eps=0.0, margin=1.0, loss=fake, correct=fake,
            dlogits=fake, sums=fake):
        return lib.op_row_loss(logits, dtype, ld, targets, tdt, ldt, B, C, mode, eps, margin, 1.0, loss, correct, dlogits, sums, None)
    for kw, msg in (({"mode": 4}, b"mode"), ({"mode": -1}, b"mode"), ({"dtype": 2}, b"dtype"), ({"mode": 1, "tdt": 3}, b"target_dtype"),
                    ({"B": -1}, b"B ="), ({"C": 0}, b"C ="), ({"ld": 6}, b"ld ="), ({"mode": 2, "ldt": 6}, b"ld_targets"),
                    ({"eps": 1.0}, b"label_smoothing"), ({"eps": -0.1}, b"label_smoothing"), ({"eps": float("nan")}, b"label_smoothing"),
                    ({"logits": None}, b"non-null"), ({"targets": None}, b"non-null"), ({"loss": None}, b"non-null"),
                    ({"correct": None}, b"non-null"), ({"logits": fake + 1}, b"aligned"), ({"dtype": 1, "logits": fake + 2}, b"aligned"),
                    ({"targets": fake + 4}, b"aligned"), ({"dlogits": fake + 2}, b"aligned")):
        assert row(**kw) == -22, kw
        err = lib.op_last_error()
        assert err.startswith(b"op_row_loss") and msg in err, (kw, err)
    assert row(B=0) == 0 and row(B=0, dlogits=None, sums=None) == 0  # nothing to do: no launch, so no device is needed

    def box(logits=fake, dtype=0, targets=fake, B=5, out=fake, dlogits=fake):
        return lib.op_box_loss(logits, dtype, targets, B, 1.0, out, dlogits, None)
    for kw, msg in (({"dtype": 2}, b"dtype"), ({"B": -1}, b"B ="), ({"B": 1 << 24}, b"B ="), ({"logits": None}, b"non-null"),
                    ({"targets": None}, b"non-null"), ({"out": None}, b"non-null"), ({"logits": fake + 4}, b"aligned"),
                    ({"dtype": 1, "logits": fake + 8}, b"aligned"), ({"targets": fake + 8}, b"aligned"), ({"dlogits": fake + 4}, b"aligned")):
        assert box(**kw) == -22, kw
        err = lib.op_last_error()
        assert err.startswith(b"op_box_loss") and msg in err, (kw, err)
    assert box(B=0) == 0
    assert lib.op_abi_version() == 10


def test_hip_route_is_not_taken_without_a_device_and_refuses_other_inputs():
    from one_peace_amd import hip, ops
    x = torch.randn(4, 6)
    assert not ops.loss_hip_eligible(x) and not ops.loss_hip_eligible(x.to(torch.bfloat16))
    if not torch.cuda.is_available():
        with pytest.raises((RuntimeError, AssertionError)):
            hip.row_loss(x, torch.zeros(4, dtype=torch.int64), hip.ROW_LOSS_HARD)
        with pytest.raises((RuntimeError, AssertionError)):
            hip.box_loss(x[:, :4].contiguous(), x[:, :4].contiguous())


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None, reason="needs hipcc")
def test_loss_kernels_compile_without_scratch_and_without_float_atomics(tmp_path):
    sys.path.insert(0, ROOT)
    from tools import check_mfma_hazards as C
    isa = C.compile_isa(str(tmp_path), "losses")
    usage = C.resource_usage(isa)
    for kernel, count in (("row_loss_kernel", 4), ("sum_rows_kernel", 1), ("box_loss_kernel", 2)):
        assert sum(kernel in n for n in usage) == count, (kernel, sorted(usage))
    assert len(usage) == 7 and all(u.get("ScratchSize", 1) == 0 for u in usage.values()), usage
    text = open(isa).read()
    assert "atomic" not in text and "ds_add_f" not in text and "ds_add_rtn_f" not in text
    assert "global_load_dwordx4" in text  # 16-byte row loads
