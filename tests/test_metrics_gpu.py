"""op_average_precision (csrc/metrics.hip) and the Accuracy / IouAcc / MAP mirrors on the device.  The kernel is checked against the
exact value -- integer counts from a numpy sort and searchsorted on the host, the quotients summed with math.fsum -- with the gate
(P_c + 2) 2^-53 derived in tests/test_metrics_cpu.py; then bit-identity of runs and of a column computed alone, the refusals before a
launch, the mirrors against the reference's eval logs (tests/golden/classify_metrics.pt), and an end-to-end run from hub features."""
import ctypes
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests.model_util import build_retrieval, load_synth
from tests.test_metrics_cpu import ACC_KEYS, IOU_KEYS, MAP_KEYS, ap_gate, exact_counts, run_metric, sklearn_gate

pytestmark = pytest.mark.gpu
DEV = "cuda"


def hipmod():
    from one_peace_amd import hip
    return hip


def exact_ap(tp, cnt):
    return math.fsum(int(t) / int(n) for t, n in zip(tp, cnt)) / len(tp) if len(tp) else 0.0


def check_against_exact(scores, targets, ap, npos, what=""):
    """scores fp32 [N, C] and targets uint8 [N, C] on the host; ap fp64 [C] and npos [C] as the kernel returned them."""
    counts = exact_counts(scores.numpy(), targets.numpy() != 0)
    ap, npos = ap.cpu(), npos.cpu()
    worst = Fraction(0)
    for c, (tp, cnt) in enumerate(counts):
        assert int(npos[c]) == len(tp), (what, c, int(npos[c]), len(tp))
        err = abs(Fraction(float(ap[c])) - Fraction(exact_ap(tp, cnt)))
        worst = max(worst, err / ap_gate(len(tp)))
        assert err <= ap_gate(len(tp)), (what, c, float(ap[c]), exact_ap(tp, cnt), len(tp))
    print("%s: worst |ap - exact| / gate = %.3f over %d classes" % (what, float(worst), len(counts)))


def sparse_case(N, C, seed, mean_positives=3.0):
    g = torch.Generator().manual_seed(seed)
    scores = torch.sigmoid(torch.randn(N, C, generator=g) * 4)  # confident scores: some saturate to equal fp32 values
    targets = (torch.rand(N, C, generator=g) < mean_positives / C).to(torch.uint8)
    return scores, targets


def _cases():
    g = torch.Generator().manual_seed(7)
    inf = float("inf")
    special = torch.tensor([[0.0, inf, -inf, 1.0], [-0.0, -inf, -inf, 1.0], [1.0, 0.0, inf, 1.0], [-1.0, inf, 0.0, 1.0], [0.0, -0.0, 5.0, 1.0]])
    special_y = torch.tensor([[1, 0, 1, 1], [0, 1, 0, 1], [0, 1, 1, 0], [1, 0, 0, 1], [1, 1, 1, 0]], dtype=torch.uint8)
    edge = torch.rand(300, 5, generator=g)
    edge_y = (torch.rand(300, 5, generator=g) < 0.2).to(torch.uint8)
    edge_y[:, 1] = 0   # a column without positives
    edge_y[:, 3] = 1   # a column with only positives
    half_y = (torch.rand(4096, 64, generator=g) < 0.5).to(torch.uint8)
    return {
        "one_positive": (torch.tensor([[0.3]]), torch.tensor([[1]], dtype=torch.uint8)),
        "one_negative": (torch.tensor([[0.3]]), torch.tensor([[0]], dtype=torch.uint8)),
        "7x3": (torch.randn(7, 3, generator=g), (torch.rand(7, 3, generator=g) < 0.5).to(torch.uint8)),
        "fsd50k_10231x200": sparse_case(10231, 200, 1),
        "audioset_20000x527": sparse_case(20000, 527, 2),
        "dense_4096x64": (torch.randn(4096, 64, generator=g), half_y),
        "four_levels": (torch.randint(0, 4, (1000, 9), generator=g).float() / 3, (torch.rand(1000, 9, generator=g) < 0.3).to(torch.uint8)),
        "all_equal": (torch.full((513, 3), 0.25), (torch.rand(513, 3, generator=g) < 0.4).to(torch.uint8)),
        "inf_and_signed_zero": (special, special_y),
        "empty_and_full_columns": (edge, edge_y),
    }


CASES = _cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_average_precision_kernel_against_the_exact_value(name):
    hip = hipmod()
    scores, targets = CASES[name]
    ap, npos = hip.average_precision(scores.to(DEV), targets.to(DEV))
    torch.cuda.synchronize()
    assert ap.dtype == torch.float64 and npos.dtype == torch.int32 and ap.shape == (scores.shape[1],)
    check_against_exact(scores, targets, ap, npos, name)
    if name == "empty_and_full_columns":
        assert float(ap[1]) == 0.0 and int(npos[1]) == 0 and float(ap[3]) == 1.0 and int(npos[3]) == 300
    if name == "all_equal":  # one threshold: every positive sees TP = P, CNT = N
        assert all(abs(float(a) - int(p) / 513) <= float(ap_gate(int(p))) for a, p in zip(ap.cpu(), npos.cpu()))


def test_average_precision_kernel_takes_row_strides():
    """Columns 3 ... 12 of wider buffers (ld 29 for the scores, 17 for the targets): the values of the contiguous copy, bit for bit."""
    hip = hipmod()
    g = torch.Generator().manual_seed(9)
    wide_s = torch.randn(700, 29, generator=g).to(DEV)
    wide_y = (torch.rand(700, 17, generator=g) < 0.3).to(torch.uint8).to(DEV)
    s, y = wide_s[:, 3:13], wide_y[:, 3:13]
    assert s.stride() == (29, 1) and y.stride() == (17, 1)
    ap, npos = hip.average_precision(s, y)
    ap2, npos2 = hip.average_precision(s.contiguous(), y.contiguous())
    torch.cuda.synchronize()
    assert torch.equal(ap.view(torch.int64), ap2.view(torch.int64)) and torch.equal(npos, npos2)
    check_against_exact(s.cpu().contiguous(), y.cpu().contiguous(), ap, npos, "strided")


def test_average_precision_runs_and_single_columns_are_bit_identical():
    hip = hipmod()
    for name in ("fsd50k_10231x200", "dense_4096x64", "four_levels"):
        scores, targets = (t.to(DEV) for t in CASES[name])
        ap1, n1 = hip.average_precision(scores, targets)
        ap2, n2 = hip.average_precision(scores, targets)
        torch.cuda.synchronize()
        assert torch.equal(ap1.view(torch.int64), ap2.view(torch.int64)) and torch.equal(n1, n2), name
        for c in (0, scores.shape[1] // 2, scores.shape[1] - 1):
            alone, n_alone = hip.average_precision(scores[:, c:c + 1].contiguous(), targets[:, c:c + 1].contiguous())
            view, _ = hip.average_precision(scores[:, c:c + 1], targets[:, c:c + 1])  # the same column at the batch's row stride
            assert torch.equal(alone.view(torch.int64), ap1[c:c + 1].view(torch.int64)) and int(n_alone) == int(n1[c]), (name, c)
            assert torch.equal(view.view(torch.int64), ap1[c:c + 1].view(torch.int64)), (name, c)


def _raw_call(scores, targets, N, C, ap, npos, ws, ws_bytes=None, ld_scores=None, ld_targets=None, ws_offset=0):
    hip = hipmod()
    rc = hip.lib().op_average_precision(hip.ptr(scores), scores.stride(0) if ld_scores is None else ld_scores, hip.ptr(targets),
                                        targets.stride(0) if ld_targets is None else ld_targets, N, C, hip.ptr(ap), hip.ptr(npos),
                                        ctypes.c_void_p(ws.data_ptr() + ws_offset), ws.numel() - ws_offset if ws_bytes is None else ws_bytes,
                                        hip.stream())
    torch.cuda.synchronize()
    return rc, hip.lib().op_last_error().decode()


def test_invalid_arguments_are_refused_without_a_launch():
    hip = hipmod()
    scores, targets = (t.to(DEV) for t in CASES["four_levels"])
    N, C = scores.shape
    need = hip.lib().op_average_precision_workspace_bytes(N, C)
    assert need == 4 * N * C + 16 * C * ((N + 63) // 64)
    ws = torch.empty(need + 64, dtype=torch.uint8, device=DEV)
    ap = torch.full((C,), 7.0, dtype=torch.float64, device=DEV)
    npos = torch.full((C,), -7, dtype=torch.int32, device=DEV)
    rc, _ = _raw_call(scores, targets, N, C, ap, npos, ws, ws_bytes=need)
    assert rc == 0 and bool((ap != 7.0).all()) and bool((npos >= 0).all())  # the valid call runs, in exactly `need` bytes
    bad = [(dict(N=0), "N ="), (dict(N=1 << 31), "N ="), (dict(C=0), "C ="), (dict(C=65536), "C ="),
           (dict(ld_scores=C - 1), "ld_scores"), (dict(ld_targets=C - 1), "ld_targets"),
           (dict(ws_bytes=need - 1), "workspace"), (dict(ws_offset=8), "workspace"), (dict(ws_offset=4), "workspace")]
    for kw, msg in bad:
        ap.fill_(7.0)
        npos.fill_(-7)
        args = dict(N=N, C=C)
        args.update(kw)
        rc, err = _raw_call(scores, targets, args.pop("N"), args.pop("C"), ap, npos, ws, **args)
        assert rc == -22 and err.startswith("op_average_precision") and msg in err, (kw, rc, err)
        assert bool((ap == 7.0).all()) and bool((npos == -7).all()), kw  # nothing was launched
    with pytest.raises(ValueError):
        hip.average_precision(scores[:0], targets[:0])


def test_accuracy_and_iou_acc_on_device_equal_the_reference_eval_logs(golden_dir):
    from one_peace_amd.metrics import Accuracy, IouAcc
    fx = torch.load(os.path.join(golden_dir, "classify_metrics.pt"))
    for name in ("accuracy_hard", "accuracy_soft"):
        m = run_metric(Accuracy(), fx[name], ACC_KEYS, device=DEV)
        assert m.score_sum.is_cuda and m.hyps.is_cuda
        assert m.merge_results(output_predict=True) == fx[name]["eval_log"], name
    m = run_metric(IouAcc(), fx["iou_acc"], IOU_KEYS, device=DEV)
    assert m.score_sum.is_cuda and m.hyps.is_cuda
    assert m.merge_results(output_predict=True) == fx["iou_acc"]["eval_log"]


def test_map_on_device_logits(golden_dir):
    """Per class against the exact value of the device's OWN fp32 sigmoid output (device and host sigmoid may differ in the last bit,
    and so may their ties).  Against the fixture's sklearn values and `map` only when the two sigmoid outputs are bit-equal: then the
    gates of the CPU test hold; otherwise the difference is printed, not gated."""
    from one_peace_amd import ops
    from one_peace_amd.metrics import MAP
    case = torch.load(os.path.join(golden_dir, "classify_metrics.pt"))["map"]
    m = run_metric(MAP(), case, MAP_KEYS, device=DEV)
    assert m.logits.is_cuda and m.targets.is_cuda
    log = m.merge_results(output_predict=True)
    sig = torch.sigmoid(case["logits"].to(DEV))
    ap, npos = ops.average_precision(sig, case["targets"].to(DEV))
    assert ap.is_cuda and npos.dtype == torch.int64 and torch.equal(npos.cpu(), case["npos"])
    check_against_exact(sig.cpu(), case["targets"].to(torch.uint8), ap, npos, "map fixture, device sigmoid")
    assert log["map"] == ap.mean().item() and log["map_cnt"] == 37
    assert log["predict_results"] == dict(zip(case["ids"].tolist(), sig.cpu().tolist()))
    same = torch.equal(sig.cpu().view(torch.int32), case["sigmoid"].view(torch.int32))
    diff = abs(Fraction(log["map"]) - Fraction(case["eval_log"]["map"]))
    print("device sigmoid bit-equal to the host's: %s; |map - reference map| = %.3e" % (same, float(diff)))
    if same:
        gates = [sklearn_gate(int(P)) for P in npos.cpu()]
        for c in range(ap.numel()):
            assert abs(Fraction(float(ap[c])) - Fraction(float(case["ap"][c]))) <= gates[c], c
        assert diff <= max(gates) + Fraction(1, 2 ** 52)
        assert log["predict_results"] == case["eval_log"]["predict_results"]


def test_accuracy_and_map_end_to_end_from_hub_features(golden_dir):
    """Zero-shot classification with the micro retrieval model: hub features of synthetic clips and of class token sequences give
    logits on the device; Accuracy on them equals the CPU route on the same logits, and every class's average precision -- device
    kernel and CPU route alike -- is within the gate of the exact value of the scores it ranked, so the two `map` values are within
    two gates plus the rounding of their means."""
    from one_peace_amd import ops
    from one_peace_amd.metrics import MAP, Accuracy
    from one_peace_amd.one_peace.hub_interface import OnePeaceHubInterface
    mfx = torch.load(os.path.join(golden_dir, "micro_retrieval.pt"), weights_only=False)
    hub = OnePeaceHubInterface(load_synth(build_retrieval(mfx["cfg"], mfx["vocab"]), mfx["shapes"]), device=DEV, dtype="bf16")
    g = torch.Generator().manual_seed(31)
    n_clip, n_cls = 12, 5
    clips = [torch.randn(16000 + 700 * i, generator=g) * 0.1 for i in range(n_clip)]
    prompts = [torch.cat([torch.tensor([0]), torch.randint(4, mfx["vocab"], (3 + c,), generator=g), torch.tensor([2])]) for c in range(n_cls)]
    wavs, masks = hub.process_audio(clips)
    audio = hub.extract_audio_features(wavs, masks)
    text = hub.extract_text_features(hub.process_text(prompts))
    logits = 20.0 * audio.float() @ text.float().t()
    assert logits.is_cuda and logits.shape == (n_clip, n_cls)
    ids = torch.arange(n_clip, device=DEV)
    labels = torch.randint(0, n_cls, (n_clip,), generator=g).to(DEV)
    labels[::2] = logits.argmax(1)[::2]
    multi = (torch.rand(n_clip, n_cls, generator=g) < 0.4).float().to(DEV)

    def run(device):
        acc, mp_ = Accuracy(), MAP()
        acc.initialize()
        mp_.initialize()
        for sl in (slice(0, 5), slice(5, n_clip)):
            acc.compute(ids[sl].to(device), logits[sl].to(device), labels[sl].to(device))
            mp_.compute(ids[sl].to(device), logits[sl].to(device), multi[sl].to(device))
        return acc.merge_results(output_predict=True), mp_.merge_results(output_predict=True)

    acc_dev, map_dev = run(DEV)
    acc_cpu, map_cpu = run("cpu")
    assert acc_dev == acc_cpu and acc_dev["score_cnt"] == n_clip and acc_dev["score_sum"] >= n_clip / 2
    gate = Fraction(0)
    for device in (DEV, "cpu"):
        sig = torch.sigmoid(logits.to(device))
        ap, npos = ops.average_precision(sig, multi.to(device))
        check_against_exact(sig.cpu(), multi.cpu().to(torch.uint8), ap, npos, "hub logits on " + device)
        gate = max(gate, max(ap_gate(int(P)) for P in npos.cpu()))
    print("map on the device %.17g, on the CPU %.17g" % (map_dev["map"], map_cpu["map"]))
    assert map_dev["map_cnt"] == map_cpu["map_cnt"] == n_clip
    assert abs(Fraction(map_dev["map"]) - Fraction(map_cpu["map"])) <= 2 * gate + Fraction(1, 2 ** 52)
