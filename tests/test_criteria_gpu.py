"""op_row_loss / op_box_loss (csrc/losses.hip) and the fine-tuning criteria on the device, through the C-ABI wrappers (hip.row_loss,
hip.box_loss) and through ops / the criteria.  Reference: the same formula in fp64 torch on the host, on the same input values
(tests/test_criteria_cpu.py: rows_fp64, box_loss_fp64, with the error units defined there).

Gates.  For every case the test also runs the reference's own fp32 arithmetic on the host (F.cross_entropy, fp32 log_softmax then
multiply and sum, F.binary_cross_entropy_with_logits, the torch box formula) and measures its worst error in units; the kernel's gate
is 2 x that + 2 units (2: the other summation order -- a wave tree against a sequential sum -- and the device exponential; + 2: a case
where the reference happens to be exact does not demand exactness), and no case may need more than 16 units.  Both worst values are
printed per case.  The hinge gradient holds multiples of 1/2 only and is compared exactly.  loss_sum: the sum of the row gates plus
(1 + ceil(log2 B)) 2^-24 sum |L_r| for the fp32 sum over the rows.  n_correct: exact in the hard, multi-label and hinge modes; in the
soft mode the row-loss style gate with scale sum_c |t_c|."""
import math
import os

import pytest
import torch

from tests.test_criteria_cpu import (GOLDEN, HARD, HINGE, MULTI, SOFT, U, Stub, box_case, box_loss_fp64, rows_fp64, rows_reference_fp32,
                                     units)

pytestmark = pytest.mark.gpu
DEV = "cuda"
CAP_UNITS = 16.0


def mods():
    from one_peace_amd import hip, ops
    return hip, ops


def make_logits(B, C, amp, seed):
    """bf16-representable fp32 values.  B >= 5: row 1 = +-3e4 (overflows an exponential taken without the maximum), row 2 all equal,
    row 3 dyadic with tied maxima (the first of them not at index 0 when C > 2)."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(B, C, generator=g) * amp).to(torch.bfloat16).float()
    if B >= 5:
        x[1] = torch.where(torch.arange(C) % 2 == 0, 3e4, -3e4).to(torch.bfloat16).float()
        x[2] = 1.25
        x[3] = torch.randint(-8, 9, (C,), generator=g).float() / 4
        top = float(x[3].max()) + 0.25
        x[3, C // 2] = top
        x[3, C - 1] = top
    return x


def make_targets(mode, x, seed):
    B, C = x.shape
    g = torch.Generator().manual_seed(seed + 1)
    if mode in (HARD, HINGE):
        t = torch.randint(0, C, (B,), generator=g)
        half = torch.rand(B, generator=g) < 0.5
        t[half] = x.argmax(1)[half]
        if B >= 5:
            t[3] = C - 1          # a tied maximum that is not the lowest index: not a hit
            t[0] = x[0].argmax()  # a hit
            if mode == HARD:
                t[4] = -100
        return t
    if mode == SOFT:
        t = torch.rand(B, C, generator=g) * (torch.rand(B, C, generator=g) < 0.2) * 2.0
        if B >= 5:
            t[0] = 0.0            # a row that sums to 0
        return t
    return (torch.rand(B, C, generator=g) < 0.15).float()


def check_rows(mode, x, targets, eps=0.0, margin=1.0, what="", dtype=torch.float32, wide=0):
    """x: host fp32 [B, C] of bf16-representable values; runs the kernel on `dtype` logits (`wide` > 0: as a column slice, starting at
    an odd column, of a matrix `wide` columns wider), checks rows, sums, gradient and the ops route, returns the kernel's outputs."""
    hip, ops = mods()
    B, C = x.shape
    l64, c64, g64, lscale, gscale = rows_fp64(mode, x, targets, eps, margin)
    lref, cref, gref = rows_reference_fp32(mode, x, targets, eps, margin)
    xd = x.to(DEV, dtype)
    if wide:
        big = torch.full((B, C + wide), 7.0, dtype=dtype, device=DEV)
        big[:, 3:3 + C] = xd
        xd = big[:, 3:3 + C]
        assert xd.stride(0) == C + wide and not xd.is_contiguous() or B == 1
    td = targets.to(DEV)
    sums, loss, correct, dlogits = hip.row_loss(xd, td, mode, eps, margin)
    torch.cuda.synchronize()
    loss, correct, dlogits, sums = loss.cpu(), correct.cpu(), dlogits.cpu(), sums.cpu()

    ref_l, got_l = units(lref[:, None], l64[:, None], lscale, C), units(loss[:, None], l64[:, None], lscale, C)
    gate_l = 2 * ref_l + 2
    if mode == HINGE:
        ref_g = got_g = gate_g = 0.0
        assert torch.equal(dlogits.double(), g64), what
    else:
        ref_g, got_g = units(gref, g64, gscale), units(dlogits, g64, gscale)
        gate_g = 2 * ref_g + 2
    print("%s B=%d C=%d %s: row loss units reference %.2f kernel %.2f (gate %.2f); gradient units reference %.2f kernel %.2f (gate %.2f)"
          % (what, B, C, str(dtype).replace("torch.", ""), ref_l, got_l, gate_l, ref_g, got_g, gate_g))
    assert got_l <= gate_l and got_l <= CAP_UNITS, (what, got_l, gate_l)
    assert got_g <= gate_g and got_g <= CAP_UNITS, (what, got_g, gate_g)

    if mode == SOFT:
        tsum = targets.double().abs().sum(1)
        ref_c, got_c = units(cref[:, None], c64[:, None], tsum), units(correct[:, None], c64[:, None], tsum)
        assert got_c <= 2 * ref_c + 2 and got_c <= CAP_UNITS, (what, got_c, ref_c)
        gate_c = (2 * ref_c + 2) * U * float(tsum.sum()) + (1 + math.ceil(math.log2(B))) * U * float(c64.abs().sum())
        assert abs(float(sums[1]) - float(c64.sum())) <= gate_c, (what, float(sums[1]), float(c64.sum()))
    else:
        assert torch.equal(correct.double(), c64), (what, correct, c64)
        assert float(sums[1]) == float(c64.sum()), what
    gate_sum = gate_l * (U * float(lscale.sum()) + B * C * 2.0 ** -126) + (1 + math.ceil(math.log2(B))) * U * float(l64.abs().sum())
    assert abs(float(sums[0]) - float(l64.sum())) <= gate_sum, (what, float(sums[0]), float(l64.sum()), gate_sum)

    # the autograd route: the same kernel, the gradient times the incoming one and cast to the logits' dtype
    leaf = xd.detach().clone().requires_grad_(True) if not wide else None
    if leaf is not None:
        if mode == HINGE:
            ls, nc = ops.hinge_loss(leaf, td, margin)
        else:
            ls, nc = ops.classify_loss(leaf, td, use_multi_label=mode == MULTI, label_smoothing=eps)
        assert ls.dtype == torch.float32 and not nc.requires_grad and ls.requires_grad
        (2.0 * ls).backward()
        assert torch.equal(ls.detach().cpu(), sums[0]) and torch.equal(nc.cpu(), sums[1])
        assert leaf.grad.dtype == dtype and torch.equal(leaf.grad.cpu(), (dlogits * 2.0).to(dtype))
    return sums, loss, correct, dlogits


SHAPES = [(B, C) for B in (1, 5, 67) for C in (2, 7, 200, 309, 1000, 3129)]
MODES = [("hard_eps0", HARD, 0.0), ("hard_eps01", HARD, 0.1), ("soft", SOFT, 0.0), ("multi", MULTI, 0.0)]


@pytest.mark.parametrize("B,C", SHAPES)
@pytest.mark.parametrize("name,mode,eps", MODES)
def test_row_loss_against_fp64(name, mode, eps, B, C):
    for amp in (1.0, 8.0, 60.0):
        x = make_logits(B, C, amp, seed=1000 * B + C + int(amp))
        t = make_targets(mode, x, seed=B + C)
        for dtype in (torch.bfloat16, torch.float32):
            check_rows(mode, x, t, eps=eps, what="%s amp=%g" % (name, amp), dtype=dtype)


@pytest.mark.parametrize("name,mode,eps", MODES)
def test_row_loss_on_a_column_slice_and_past_the_staged_columns(name, mode, eps):
    """ld > C with rows that start at an odd element (never 16-byte aligned for bf16, one row in four for fp32), and C = 4173 > the
    4096 columns staged in LDS (the later columns are read again in the second and third pass)."""
    for B, C, wide in ((5, 309, 24), (5, 200, 9), (3, 4173, 0), (5, 4173, 5)):
        x = make_logits(B, C, 8.0, seed=C + wide)
        t = make_targets(mode, x, seed=C)
        for dtype in (torch.bfloat16, torch.float32):
            check_rows(mode, x, t, eps=eps, what="%s wide=%d" % (name, wide), dtype=dtype, wide=wide)


@pytest.mark.parametrize("B", [1, 5, 67])
def test_hinge_against_fp64_with_exact_gradients(B):
    hip, _ = mods()
    for amp in (1.0, 8.0, 60.0):
        for margin in (1.0, 3.0, 0.0):
            x = make_logits(B, 4, amp, seed=B + int(amp))
            if B >= 5:
                x[0] = torch.tensor([0.5, 1.5, 1.5, -0.25])  # target 1 (the arg-max of the tie): margin + x_0 - x_t = 0 at margin 1
            t = make_targets(HINGE, x, seed=B)
            for dtype in (torch.bfloat16, torch.float32):
                _, _, _, dl = check_rows(HINGE, x, t, margin=margin, what="hinge amp=%g margin=%g" % (amp, margin), dtype=dtype)
                if B >= 5 and margin == 1.0:
                    assert int(t[0]) == 1 and dl[0].tolist() == [0.5, -1.5, 1.0, 0.0]  # 0.5 at the exact zero; the target: 1 - (0.5 + 1 + 1)
                if margin == 0.0:  # every k = target term is an exact zero: 0.5 of its own, minus the sum of all of them
                    assert bool((dl.gather(1, t[:, None])[:, 0] <= 0.0).all())


def test_two_runs_are_bit_identical():
    hip, _ = mods()
    for mode, eps in ((HARD, 0.1), (SOFT, 0.0), (MULTI, 0.0), (HINGE, 0.0)):
        x = make_logits(67, 4 if mode == HINGE else 3129, 8.0, seed=5).to(DEV, torch.bfloat16)
        t = make_targets(mode, x.float().cpu(), seed=6).to(DEV)
        a = hip.row_loss(x, t, mode, eps, 1.0)
        b = hip.row_loss(x, t, mode, eps, 1.0)
        for u, v in zip(a, b):
            assert torch.equal(u.view(torch.int32), v.view(torch.int32))  # bits: NaN-safe
    lg, tg = box_case(67, seed=9)
    a = hip.box_loss(lg.to(DEV), tg.to(DEV))
    b = hip.box_loss(lg.to(DEV), tg.to(DEV))
    for u, v in zip(a, b):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32))


def test_ignored_out_of_range_and_nan_rows():
    hip, _ = mods()
    B, C = 6, 309
    x = make_logits(B, C, 8.0, seed=77)
    t = make_targets(HARD, x, seed=78)
    t[4] = 5
    clean = [o.cpu() for o in hip.row_loss(x.to(DEV), t.to(DEV), HARD, 0.1, 1.0)]
    t2 = t.clone()
    t2[0], t2[2], t2[5] = -100, C, -1
    sums, loss, correct, dl = [o.cpu() for o in hip.row_loss(x.to(DEV), t2.to(DEV), HARD, 0.1, 1.0)]
    assert float(loss[0]) == 0.0 and float(correct[0]) == 0.0 and float(dl[0].abs().max()) == 0.0          # ignore_index
    for r in (2, 5):                                                                                        # out of range
        assert math.isnan(float(loss[r])) and float(correct[r]) == 0.0 and float(dl[r].abs().max()) == 0.0
    for r in (1, 3, 4):                                                                                     # the other rows: untouched
        assert torch.equal(loss[r], clean[1][r]) and torch.equal(correct[r], clean[2][r]) and torch.equal(dl[r], clean[3][r])
    assert math.isnan(float(sums[0])) and float(sums[1]) == float(correct.sum())
    # hinge has no ignore_index: -100 is out of range there
    xh = make_logits(5, 4, 1.0, seed=3)
    th = torch.tensor([0, -100, 4, 3, 1])
    _, lh, ch, dh = [o.cpu() for o in hip.row_loss(xh.to(DEV), th.to(DEV), HINGE, 0.0, 1.0)]
    assert [math.isnan(v) for v in lh.tolist()] == [False, True, True, False, False] and float(dh[1:3].abs().max()) == 0.0
    # a NaN logit: that row's loss is NaN in every mode, the other rows keep their bits
    for mode, eps in ((HARD, 0.0), (HARD, 0.1), (SOFT, 0.0), (MULTI, 0.0), (HINGE, 0.0)):
        xm = make_logits(B, 4 if mode == HINGE else C, 8.0, seed=79)
        tm = make_targets(mode, xm, seed=80)
        if mode == HARD:
            tm[4] = 1
        if mode == HINGE:
            tm[1] = 0       # the NaN is not at the target: a max(0, .) that drops NaNs would hide it
        base = [o.cpu() for o in hip.row_loss(xm.to(DEV), tm.to(DEV), mode, eps, 1.0)]
        xn = xm.clone()
        xn[1, 3 if mode == HINGE else 201] = float("nan")
        got = [o.cpu() for o in hip.row_loss(xn.to(DEV), tm.to(DEV), mode, eps, 1.0)]
        assert math.isnan(float(got[1][1])) and math.isnan(float(got[0][0])), (mode, eps)
        keep = [r for r in range(B) if r != 1]
        assert torch.equal(got[1][keep], base[1][keep]) and torch.equal(got[3][keep], base[3][keep]), (mode, eps)


@pytest.mark.parametrize("B", [1, 5, 67])
def test_box_loss_against_fp64(B):
    hip, ops = mods()
    from one_peace_amd.ops import box_loss_torch
    for dtype in (torch.bfloat16, torch.float32):
        logits, targets = box_case(B, seed=100 + B, dtype=dtype)
        want, nv, g64 = box_loss_fp64(logits.float(), targets)
        assert nv == B if B == 1 else 0 < nv < B
        leaf = logits.float().clone().requires_grad_(True)
        ref = box_loss_torch(leaf, targets)  # the torch formula in fp32 on the host
        (gref,) = torch.autograd.grad(ref, leaf)
        ref = ref.detach()
        out, dl = hip.box_loss(logits.to(DEV), targets.to(DEV))
        out, dl = out.cpu(), dl.cpu()
        gmax = float(g64.abs().max())
        ref_l, got_l = abs(float(ref) - float(want)) / (U * abs(float(want))), abs(float(out[0]) - float(want)) / (U * abs(float(want)))
        ref_g, got_g = float((gref.double() - g64).abs().max()) / (U * gmax), float((dl.double() - g64).abs().max()) / (U * gmax)
        print("box B=%d %s: loss units reference %.2f kernel %.2f; gradient units reference %.2f kernel %.2f"
              % (B, str(dtype).replace("torch.", ""), ref_l, got_l, ref_g, got_g))
        assert float(out[1]) == nv
        assert got_l <= 2 * ref_l + 2 and got_l <= CAP_UNITS and got_g <= 2 * ref_g + 2 and got_g <= CAP_UNITS
        x = logits.to(DEV).requires_grad_(True)
        loss = ops.box_loss(x, targets.to(DEV))
        (3.0 * loss).backward()
        assert loss.dtype == torch.float32 and torch.equal(loss.detach().cpu(), out[0])
        assert x.grad.dtype == dtype and torch.equal(x.grad.cpu(), (dl * 3.0).to(dtype))


def test_box_loss_without_a_valid_row_and_at_equality():
    hip, _ = mods()
    from one_peace_amd.ops import box_loss_torch
    logits = torch.tensor([[1.0, 0.0, -1.0, 2.0], [0.5, 1.0, 0.25, -1.0]])
    targets = torch.tensor([[0.1, 0.2, 0.6, 0.7], [0.3, 0.1, 0.9, 0.5]])
    out, dl = [o.cpu() for o in hip.box_loss(logits.to(DEV), targets.to(DEV))]
    _, nv, g64 = box_loss_fp64(logits, targets)
    assert nv == 0 and math.isnan(float(out[0])) and float(out[1]) == 0.0
    assert float((dl.double() - g64).abs().max()) <= 4 * U * float(g64.abs().max()) and float(dl.abs().min()) > 0  # the L1 term alone
    out, dl = [o.cpu() for o in hip.box_loss(torch.zeros(1, 4, device=DEV), torch.full((1, 4), 0.5, device=DEV))]
    assert math.isnan(float(out[0])) and float(dl.abs().max()) == 0.0  # o == t: sign(0) = 0
    # a valid row that ties the target's corner: max / min give 1/2 to each side, as fp64 autograd does (sigmoid(0) = 0.5 exactly)
    lg = torch.tensor([[0.0, 0.0, 2.0, 1.0]])
    tg = torch.tensor([[0.5, 0.5, 0.9, 0.7]])
    out, dl = [o.cpu() for o in hip.box_loss(lg.to(DEV), tg.to(DEV))]
    want, nv, g64 = box_loss_fp64(lg, tg)
    leaf = lg.clone().requires_grad_(True)
    ref = box_loss_torch(leaf, tg)  # the gate: 2 x the error of the torch formula in fp32 on the host + 2 units
    (gref,) = torch.autograd.grad(ref, leaf)
    ref = ref.detach()
    assert nv == 1 and abs(float(out[0]) - float(want)) <= 2 * abs(float(ref) - float(want)) + 2 * U * float(want)
    assert float((dl.double() - g64).abs().max()) <= 2 * float((gref.double() - g64).abs().max()) + 2 * U * float(g64.abs().max())
    assert abs(float(out[0]) - float(want)) <= CAP_UNITS * U * float(want)
    _, _, shifted = box_loss_fp64(torch.tensor([[1e-3, 1e-3, 2.0, 1.0]]), tg)
    assert float((g64[0, :2] - shifted[0, :2]).abs().min()) > 1e-2  # the tie matters: just off it the gradient is another one


def _criterion_case(name, fx):
    from one_peace_amd.criterions.finetune import ClassifyCriterion, HingeLoss
    case = fx[name]
    if name.startswith("hinge"):
        K = case["num_choices"]
        crit = HingeLoss(None, margin=1.0, num_choices=K)  # what the reference computed, whatever margin it was built with
        ni = {k: v.to(DEV) for k, v in case["net_input"].items()}
        return crit, ni, HINGE, case["logits"].view(-1, K), 0.0
    mode = MULTI if name.startswith("multi") else (SOFT if name.startswith("soft") else HARD)
    crit = ClassifyCriterion(None, use_multi_label=mode == MULTI, label_smoothing=case.get("label_smoothing", 0.0))
    return crit, {"src_tokens": torch.zeros(1, device=DEV)}, mode, case["logits"], case.get("label_smoothing", 0.0)


@pytest.mark.parametrize("name", ["hard_eps0_f32", "hard_eps0_bf16", "hard_eps01_f32", "hard_eps01_bf16", "soft_f32", "multi_f32", "hinge_m1",
                                  "hinge_m3"])
def test_criteria_on_the_device_against_the_reference_fixture(name):
    """forward and backward through a stub model that returns device logits.  The recorded numbers are the reference's fp32 (for the
    bf16 cases: bf16) arithmetic; the logits are bf16-representable, so the bf16 cases are compared with the fp32 records of the same
    values.  Device loss within the loss_sum gate of fp64, and within that plus the record's own distance to fp64 of the record;
    gradient entries likewise (a bf16 gradient is the fp32 one rounded to 8 significant bits: + 2^-8 |g|); counters equal (soft: within its gate)."""
    fx = torch.load(GOLDEN)
    case, rec = fx[name], fx[name.replace("bf16", "f32")]
    crit, ni, mode, x2d, eps = _criterion_case(name, fx)
    assert torch.equal(case["logits"].float(), rec["logits"])
    B = x2d.shape[0]
    l64, c64, g64, lscale, gscale = rows_fp64(mode, x2d, case["target"], eps, 1.0)
    lref, cref, gref = rows_reference_fp32(mode, x2d, case["target"], eps, 1.0)
    gate_units = min(2 * units(lref[:, None], l64[:, None], lscale) + 2, CAP_UNITS)
    gate_sum = gate_units * U * float(lscale.sum()) + (1 + math.ceil(math.log2(B))) * U * float(l64.abs().sum())
    model = Stub(case["logits"].to(DEV))
    loss, sample_size, log = crit(model, {"net_input": ni, "target": case["target"].to(DEV), "nsentences": case["nsentences"]})
    loss.backward()
    assert sample_size == case["sample_size"] and sorted(log) == ["loss", "n_correct", "nsentences", "sample_size"]
    assert loss.dtype == torch.float32 and torch.equal(log["loss"], loss.detach())
    assert abs(float(loss) - float(l64.sum())) <= gate_sum, (float(loss), float(l64.sum()), gate_sum)
    assert abs(float(loss) - float(rec["loss"])) <= gate_sum + abs(float(rec["loss"]) - float(l64.sum()))
    grad = model.logits.grad.cpu().view(B, -1)
    assert model.logits.grad.dtype == case["logits"].dtype
    if mode == HINGE:
        assert torch.equal(grad, rec["grad"].view(B, -1))
    else:
        gate_g = min(2 * units(gref, g64, gscale) + 2, CAP_UNITS) * U * gscale[:, None] + (
            2.0 ** -8 * g64.abs() if grad.dtype == torch.bfloat16 else 0.0)
        assert bool(((grad.double() - g64).abs() <= gate_g).all())
        assert bool(((grad.double() - rec["grad"].double()).abs() <= gate_g + (rec["grad"].double() - g64).abs()).all())
    if mode == SOFT:
        tsum = case["target"].double().abs().sum()
        assert abs(float(log["n_correct"]) - float(c64.sum())) <= (gate_units * U * float(tsum)
                                                                 + (1 + math.ceil(math.log2(B))) * U * float(c64.abs().sum()))
    else:
        assert float(log["n_correct"]) == float(rec["n_correct"]) == float(c64.sum())


def test_refcoco_criterion_on_the_device():
    from one_peace_amd.criterions.finetune import RefCOCOCriterion
    from one_peace_amd.ops import box_loss_torch
    logits, targets = box_case(67, seed=11)
    want, nv, g64 = box_loss_fp64(logits, targets)
    leaf = logits.clone().requires_grad_(True)
    ref = box_loss_torch(leaf, targets)
    (gref,) = torch.autograd.grad(ref, leaf)
    ref = ref.detach()
    gate_l = min(2 * abs(float(ref) - float(want)) + 2 * U * float(want), CAP_UNITS * U * float(want))
    gate_g = min(2 * float((gref.double() - g64).abs().max()) + 2 * U * float(g64.abs().max()), CAP_UNITS * U * float(g64.abs().max()))
    model = Stub(logits.to(DEV))
    loss, sample_size, log = RefCOCOCriterion(None)(model, {"net_input": {"src_tokens": torch.zeros(1, device=DEV)},
                                                            "target": targets.to(DEV), "nsentences": 67})
    loss.backward()
    assert sample_size == 1 and sorted(log) == ["loss", "nsentences", "sample_size"] and log["nsentences"] == 67
    assert abs(float(loss.detach()) - float(want)) <= gate_l
    assert float((model.logits.grad.cpu().double() - g64).abs().max()) <= gate_g
