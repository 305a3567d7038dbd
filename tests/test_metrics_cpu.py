"""The classification metrics on the torch path (CPU): the Accuracy / IouAcc / MAP mirrors against the reference's own eval logs
(tests/golden/classify_metrics.pt, made by tests/golden/make_metrics_golden.py from one_peace/metrics/{accuracy,iou_acc,map}.py with
sklearn 1.7.2), ops.average_precision against the exact rational value, a world-2 gloo run with uneven shards, the ValueError cases,
and the static checks of csrc/metrics.hip (argument validation before any launch, ScratchSize 0).

Gates.  u = 2^-53.  ops.average_precision forms P_c correctly rounded quotients in [0, 1], adds P_c non-negative terms (in any order:
at most (P_c - 1) u relative), divides once and AP <= 1: |ap - exact| <= (P_c + 2) 2^-53.  Against sklearn's own fp64 value the gate
is (P_c + 4) 2^-52, that bound plus sklearn's measured distance to the exact value (the generator asserts sklearn is within half of
it); `map`, a mean of the classes, is within the largest per-class gate plus 2^-52."""
import os
import shutil
import sys
import tempfile
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "classify_metrics.pt")


def exact_counts(scores, positive):
    """Per class the integer pairs (TP(i), CNT(i)) of every positive i in sample order, by definition: scores fp32 [N, C] (numpy), order
    by value.  CNT(i) = #{j : s_j >= s_i}, TP(i) = #{positive j : s_j >= s_i}, from a sort and searchsorted."""
    out = []
    for c in range(scores.shape[1]):
        s = scores[:, c].astype(np.float64)  # exact, and -0 == +0 as values
        y = positive[:, c].astype(bool)
        all_sorted, pos_sorted = np.sort(s), np.sort(s[y])
        cnt = len(s) - np.searchsorted(all_sorted, s[y], side="left")
        tp = len(pos_sorted) - np.searchsorted(pos_sorted, s[y], side="left")
        out.append((tp.astype(np.int64), cnt.astype(np.int64)))
    return out


def exact_ap_fraction(tp, cnt):
    if len(tp) == 0:
        return Fraction(0)
    return sum((Fraction(int(t), int(n)) for t, n in zip(tp, cnt)), Fraction(0)) / len(tp)


def ap_gate(P):
    return Fraction(P + 2, 2 ** 53)


def sklearn_gate(P):
    return Fraction(P + 4, 2 ** 52)


def run_metric(metric, case, keys, chunks=None, device=None):
    """initialize, compute over the fixture's two batches (or `chunks`), return the metric."""
    n = case[keys[0]].shape[0]
    chunks = chunks or (slice(0, case["split"]), slice(case["split"], n))
    metric.initialize()
    for c in chunks:
        args = [case[k][c] for k in keys]
        metric.compute(*[a.to(device) for a in args] if device else args)
    return metric


ACC_KEYS, IOU_KEYS, MAP_KEYS = ("ids", "logits", "targets"), ("ids", "hyps", "refs"), ("ids", "logits", "targets")


def test_accuracy_and_iou_acc_reproduce_the_reference_eval_logs():
    from one_peace_amd.metrics import Accuracy, IouAcc
    fx = torch.load(GOLDEN)
    assert fx["sklearn_version"] == "1.7.2"
    for name in ("accuracy_hard", "accuracy_soft"):
        log = run_metric(Accuracy(), fx[name], ACC_KEYS).merge_results(output_predict=True)
        assert log == fx[name]["eval_log"], name  # counts, predictions, and `accuracy` as the same float
        assert sorted(log) == ["accuracy", "predict_results", "score_cnt", "score_sum"] and log["score_cnt"] == 19
        assert 0 < log["accuracy"] < 1 and len(log["predict_results"]) == 19
        assert run_metric(Accuracy(), fx[name], ACC_KEYS).merge_results()["predict_results"] == {}
    assert fx["accuracy_soft"]["targets"].dim() == 2 and fx["accuracy_soft"]["eval_log"]["score_sum"] != round(fx["accuracy_soft"]["eval_log"]["score_sum"])
    log = run_metric(IouAcc(), fx["iou_acc"], IOU_KEYS).merge_results(output_predict=True)
    assert log == fx["iou_acc"]["eval_log"]
    assert sorted(log) == ["iou_acc", "predict_results", "score_cnt", "score_sum"]
    # rows 5, 6, 7 and 9 count; row 0 (disjoint, IoU "1" from a negative width times a negative height) does not
    assert log["score_sum"] == 4.0 and log["score_cnt"] == 11 and log["iou_acc"] == 4.0 / 11
    assert run_metric(IouAcc(), fx["iou_acc"], IOU_KEYS).merge_results()["predict_results"] == {}


def test_map_reproduces_the_reference_eval_log_within_the_gate():
    from one_peace_amd import ops
    from one_peace_amd.metrics import MAP
    case = torch.load(GOLDEN)["map"]
    want = case["eval_log"]
    log = run_metric(MAP(), case, MAP_KEYS).merge_results(output_predict=True)
    assert sorted(log) == ["map", "map_cnt", "predict_results"]
    assert log["map_cnt"] == want["map_cnt"] == 37 and log["predict_results"] == want["predict_results"]
    sig = torch.sigmoid(case["logits"])
    assert torch.equal(sig, case["sigmoid"])  # the same CPU sigmoid as the generator's
    ap, npos = ops.average_precision(sig, case["targets"])
    assert ap.dtype == torch.float64 and npos.dtype == torch.int64 and torch.equal(npos, case["npos"])
    gates = [sklearn_gate(int(P)) for P in npos]
    for c in range(ap.numel()):
        assert abs(Fraction(float(ap[c])) - Fraction(float(case["ap"][c]))) <= gates[c], (c, float(ap[c]), float(case["ap"][c]))
    assert float(ap[2]) == 0.0 and int(npos[2]) == 0 and float(ap[4]) == 1.0 and int(npos[4]) == 37
    assert abs(Fraction(log["map"]) - Fraction(want["map"])) <= max(gates) + Fraction(1, 2 ** 52)
    assert run_metric(MAP(), case, MAP_KEYS).merge_results()["predict_results"] == {}


def quantised_case(N, C, levels, rate, seed):
    g = torch.Generator().manual_seed(seed)
    scores = (torch.randint(0, levels, (N, C), generator=g).float() - levels // 2) / 7.0  # not dyadic: the fp32 values are what is ranked
    targets = torch.rand(N, C, generator=g) < rate
    return scores, targets


@pytest.mark.parametrize("levels", [2, 5, 50, 10 ** 5])
@pytest.mark.parametrize("rate", [0.02, 0.3, 0.9])
def test_average_precision_torch_path_against_the_exact_rational_value(levels, rate):
    from one_peace_amd import ops
    scores, targets = quantised_case(211, 5, levels, rate, seed=levels + int(rate * 100))
    ap, npos = ops.average_precision(scores, targets)
    counts = exact_counts(scores.numpy(), targets.numpy())
    for c, (tp, cnt) in enumerate(counts):
        assert int(npos[c]) == len(tp) == int(targets[:, c].sum())
        assert abs(Fraction(float(ap[c])) - exact_ap_fraction(tp, cnt)) <= ap_gate(len(tp)), (c, float(ap[c]))
    # the same values from bf16 / fp16 scores (cast to fp32 first) and integer / float targets
    half = scores.to(torch.bfloat16)
    a1, n1 = ops.average_precision(half, targets.long())
    a2, n2 = ops.average_precision(half.float(), targets.float())
    assert torch.equal(a1, a2) and torch.equal(n1, n2) and torch.equal(n1, npos)


def test_average_precision_special_values_and_empty_classes():
    from one_peace_amd import ops
    inf = float("inf")
    scores = torch.tensor([[0.0, inf, 1.0, 0.5], [-0.0, -inf, 1.0, 0.5], [1.0, 0.0, 1.0, 0.25], [-1.0, inf, 1.0, 0.75]])
    targets = torch.tensor([[1, 0, 1, 0], [0, 1, 1, 0], [0, 1, 0, 0], [1, 0, 1, 0]])
    ap, npos = ops.average_precision(scores, targets)
    # class 0: +0 ties with -0 -> positive 0 sees {1, 0, -0}: 1 / 3; positive 3 sees all four: 2 / 4.  class 1: -inf sees 4 (2 positives),
    # 0.0 sees {inf, inf, 0}: 1 / 3.  class 2: all tied, 3 of 4 positive.  class 3: no positives.
    want = [(Fraction(1, 3) + Fraction(2, 4)) / 2, (Fraction(2, 4) + Fraction(1, 3)) / 2, Fraction(3, 4), Fraction(0)]
    assert npos.tolist() == [2, 2, 3, 0]
    for c in range(4):
        assert abs(Fraction(float(ap[c])) - want[c]) <= ap_gate(int(npos[c]))
    assert float(ap[3]) == 0.0
    ones, _ = ops.average_precision(scores, torch.ones(4, 4, dtype=torch.bool))
    assert ones.tolist() == [1.0] * 4


def test_average_precision_value_errors():
    from one_peace_amd import ops
    s = torch.rand(6, 3)
    y = torch.rand(6, 3) < 0.5
    with pytest.raises(ValueError, match="shape"):
        ops.average_precision(s, y[:5])
    with pytest.raises(ValueError, match="shape"):
        ops.average_precision(s[:, 0], y[:, 0])
    bad = s.clone()
    bad[2, 1] = float("nan")
    with pytest.raises(ValueError, match="NaN"):
        ops.average_precision(bad, y)
    with pytest.raises(ValueError, match="0 or 1"):
        ops.average_precision(s, y.float() * 0.5)
    with pytest.raises(ValueError):
        ops.average_precision(s[:0], y[:0])
    ops.average_precision(s, y.float())  # 0.0 / 1.0 floats are fine


def _worker(rank, world, initfile, outdir):
    sys.path.insert(0, ROOT)
    dist.init_process_group("gloo", init_method="file://" + initfile, rank=rank, world_size=world)
    try:
        from one_peace_amd.metrics import MAP, Accuracy, IouAcc
        fx = torch.load(GOLDEN)
        logs = {}
        for name, cls, keys, shards in (("accuracy_hard", Accuracy, ACC_KEYS, (slice(0, 5), slice(5, 19))),
                                        ("accuracy_soft", Accuracy, ACC_KEYS, (slice(0, 12), slice(12, 19))),
                                        ("iou_acc", IouAcc, IOU_KEYS, (slice(0, 3), slice(3, 11))),
                                        ("map", MAP, MAP_KEYS, (slice(0, 9), slice(9, 37)))):
            sh = shards[rank]
            mid = sh.start + (sh.stop - sh.start) // 2
            logs[name] = run_metric(cls(), fx[name], keys, chunks=(slice(sh.start, mid), slice(mid, sh.stop))).merge_results(
                output_predict=True)
        torch.save(logs, os.path.join(outdir, "r%d.pt" % rank))
    finally:
        dist.destroy_process_group()


def test_metrics_world2_gloo_equal_the_single_process_results():
    from one_peace_amd.metrics import MAP, Accuracy, IouAcc
    fx = torch.load(GOLDEN)
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(2, os.path.join(d, "init"), d), nprocs=2, join=True)
        logs = [torch.load(os.path.join(d, "r%d.pt" % r)) for r in range(2)]
    for name, cls, keys in (("accuracy_hard", Accuracy, ACC_KEYS), ("accuracy_soft", Accuracy, ACC_KEYS), ("iou_acc", IouAcc, IOU_KEYS),
                            ("map", MAP, MAP_KEYS)):
        single = run_metric(cls(), fx[name], keys).merge_results(output_predict=True)
        assert logs[0][name] == single and logs[1][name] == single, name
        assert len(single["predict_results"]) == fx[name]["ids"].shape[0]


@pytest.fixture(scope="module")
def lib():
    import importlib.util
    spec = importlib.util.spec_from_file_location("onepeace_build", os.path.join(ROOT, "one-peace_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build(verbose=False)
    from one_peace_amd import hip
    return hip.lib()


def test_average_precision_entry_point_rejects_bad_arguments(lib):
    fake = 1 << 20  # never dereferenced: validation comes first
    need = lib.op_average_precision_workspace_bytes(100, 7)
    assert need == 4 * 100 * 7 + 16 * 7 * 2
    assert lib.op_average_precision_workspace_bytes(10231, 200) == 4 * 10231 * 200 + 16 * 200 * 160
    for N, C, lds, ldt, ws, ws_bytes, msg in ((0, 7, 7, 7, fake, need, b"N ="), (1 << 31, 7, 7, 7, fake, 1 << 40, b"N ="),
                                               (100, 0, 7, 7, fake, need, b"C ="), (100, 65536, 65536, 65536, fake, 1 << 40, b"C ="),
                                               (100, 7, 6, 7, fake, need, b"ld_scores"), (100, 7, 7, 5, fake, need, b"ld_targets"),
                                               (100, 7, 7, 7, fake, need - 1, b"workspace"), (100, 7, 7, 7, fake + 8, need, b"workspace"),
                                               (100, 7, 7, 7, None, need, b"workspace")):
        rc = lib.op_average_precision(fake, lds, fake, ldt, N, C, fake, fake, ws, ws_bytes, None)
        assert rc == -22, (N, C, lds, ldt)
        err = lib.op_last_error()
        assert err.startswith(b"op_average_precision") and msg in err, err
    assert lib.op_average_precision(None, 7, fake, 7, 100, 7, fake, fake, fake, need, None) == -22
    assert lib.op_abi_version() == 10


@pytest.mark.skipif(shutil.which(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")) is None, reason="needs hipcc")
def test_metrics_kernels_compile_without_scratch_and_without_float_atomics(tmp_path):
    sys.path.insert(0, ROOT)
    from tools import check_mfma_hazards as C
    isa = C.compile_isa(str(tmp_path), "metrics")
    usage = C.resource_usage(isa)
    for kernel in ("ap_prepare_kernel", "ap_count_kernel", "ap_finish_kernel"):
        assert any(kernel in n for n in usage), (kernel, sorted(usage))
    assert len(usage) == 3 and all(u.get("ScratchSize", 1) == 0 for u in usage.values()), usage
    text = open(isa).read()
    assert "v_div_scale_f64" in text               # IEEE fp64 division, not a reciprocal approximation
    assert "atomic" not in text and "ds_add_f" not in text and "ds_add_rtn_f" not in text
