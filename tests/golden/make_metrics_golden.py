"""Generate tests/golden/classify_metrics.pt from the UNMODIFIED reference metrics (one_peace/metrics/accuracy.py, iou_acc.py, map.py:
classes Accuracy, IouAcc, MAP), run on CPU through oracle/ref_shim.py, with sklearn 1.7.2 behind MAP.

    python tests/golden/make_metrics_golden.py      # needs the reference tree and scikit-learn; writes classify_metrics.pt

The three modules import all_gather from ..utils.data_utils, which they only call under torch.distributed; that one name is stubbed
here, and torch.Tensor.cuda is the identity for the duration of the script (their initialize() calls .cuda() on the empty state).

Cases.  Accuracy: 1-D class targets and 2-D soft-label targets (VQA style; the soft scores are multiples of 1/4, so that the fp32 score_sum is
exact however the rows are split over batches and ranks), no tied maxima, two batches each.  IouAcc: disjoint boxes
(whose "intersection" has negative width AND height, hence a positive area: the w > 0 & h > 0 condition decides), touching boxes,
nested boxes on both sides of 0.5, boxes that overlap by exactly 0.5, all as exact small integers.  MAP: logits [37, 6] in batches of
23 and 14 rows on a grid of 1/4 (ties), with saturated entries (|x| > 20: their fp32 sigmoid is exactly 1.0, or distinct tiny values), a
class without positives and a class with only positives; the fp32 sigmoid outputs are stored next to the logits, with sklearn's
per-class values.  For every MAP class the script asserts that sklearn's value lies within half of the tests' gate,
(P_c + 4) 2^-52, of the exact rational value.  The file holds tensors, plain numbers and the sklearn version string only.
"""
import importlib
import os
import sys
import types
import warnings
from fractions import Fraction

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import ref_shim as R  # noqa: E402

SKLEARN = "1.7.2"


def reference_metrics():
    R.install()
    op_root = os.path.join(R.REFERENCE_ROOT, "one_peace")
    for name, path in (("one_peace.metrics", os.path.join(op_root, "metrics")), ("one_peace.utils", os.path.join(op_root, "utils"))):
        if name not in sys.modules:
            m = types.ModuleType(name)
            m.__path__ = [path]
            m.__package__ = name
            sys.modules[name] = m
    stub = types.ModuleType("one_peace.utils.data_utils")

    def all_gather(q, exclude_self=False):
        raise RuntimeError("not reached: the fixture runs without torch.distributed")

    stub.all_gather = all_gather
    sys.modules["one_peace.utils.data_utils"] = stub
    return (importlib.import_module("one_peace.metrics.accuracy").Accuracy, importlib.import_module("one_peace.metrics.iou_acc").IouAcc,
            importlib.import_module("one_peace.metrics.map").MAP)


def accuracy_data():
    g = torch.Generator().manual_seed(11)
    B, C = 19, 7
    logits = torch.randperm(B * C, generator=g).float().view(B, C) / 8 - 5  # all entries distinct: no tied maxima
    ids = 500 + 7 * torch.arange(B)
    hard = torch.randint(0, C, (B,), generator=g)
    hard[:9] = logits[:9].argmax(1)  # some right, some wrong
    soft = torch.tensor([0.0, 0.25, 0.5, 1.0])[torch.randint(0, 4, (B, C), generator=g)]  # dyadic: fp32 sums exact in any order
    return ids, logits, hard, soft


def iou_data():
    hyps = torch.tensor([[0, 0, 1, 1],    # disjoint: w = h = -1, "area" +1, IoU 1 -- only w > 0 & h > 0 rejects it
                         [0, 0, 2, 2],    # disjoint along x only
                         [0, 0, 1, 1],    # touching along an edge: w = 0
                         [0, 0, 2, 2],    # touching at a corner
                         [1, 1, 3, 3],    # nested, IoU 4 / 16
                         [0, 0, 4, 3],    # nested, IoU 12 / 16
                         [0, 0, 2, 1],    # IoU exactly 1 / 2
                         [0, 0, 3, 2],    # IoU exactly 1 / 2 (3 / 6)
                         [0, 0, 5, 2],    # IoU 4 / 10
                         [2, 3, 7, 9],    # equal boxes
                         [1, 0, 6, 4]],   # partial overlap, IoU 9 / 27
                        dtype=torch.float32)
    refs = torch.tensor([[2, 2, 3, 3], [3, 0, 5, 2], [1, 0, 2, 1], [2, 2, 4, 4], [0, 0, 4, 4], [0, 0, 4, 4], [0, 0, 1, 1], [0, 0, 3, 1],
                         [0, 0, 2, 2], [2, 3, 7, 9], [3, 1, 7, 5]], dtype=torch.float32)
    ids = 40 + torch.arange(hyps.shape[0])
    return ids, hyps, refs


def map_data():
    g = torch.Generator().manual_seed(23)
    N, C = 37, 6
    logits = torch.randint(-12, 13, (N, C), generator=g).float() / 4  # a grid of 1 / 4: many exact ties
    sat = torch.tensor([25.0, 30.0, 22.5, -25.0, -40.0, -21.0, 88.0, -104.0])  # fp32 sigmoid: 1.0 three times, tiny distinct values, 1.0, 0.0
    where = torch.randperm(N * C, generator=g)[:24]
    logits.view(-1)[where] = sat[torch.randint(0, len(sat), (24,), generator=g)]
    targets = (torch.rand(N, C, generator=g) < 0.3).float()
    targets[:, 2] = 0.0  # a class without positives
    targets[:, 4] = 1.0  # a class with only positives
    ids = 9000 + torch.arange(N)
    return ids, logits, targets


def exact_ap(scores, y):
    """The exact rational average precision of one class: scores as the fp32 values they are, counts by definition."""
    s = [Fraction(float(v)) for v in scores.tolist()]
    pos = [i for i, t in enumerate(y.tolist()) if t]
    if not pos:
        return Fraction(0), 0
    total = Fraction(0)
    for i in pos:
        cnt = sum(1 for v in s if v >= s[i])
        tp = sum(1 for j in pos if s[j] >= s[i])
        total += Fraction(tp, cnt)
    return total / len(pos), len(pos)


def main():
    import sklearn
    from sklearn.metrics import average_precision_score
    assert sklearn.__version__ == SKLEARN, "this fixture records sklearn %s, found %s" % (SKLEARN, sklearn.__version__)
    saved_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        Accuracy, IouAcc, MAP = reference_metrics()
        out = {"sklearn_version": sklearn.__version__}

        ids, logits, hard, soft = accuracy_data()
        for name, tg in (("hard", hard), ("soft", soft)):
            m = Accuracy()
            m.initialize()
            m.compute(ids[:8], logits[:8], tg[:8])
            m.compute(ids[8:], logits[8:], tg[8:])
            out["accuracy_" + name] = {"ids": ids, "logits": logits, "targets": tg, "split": 8, "eval_log": m.merge_results(output_predict=True)}

        ids, hyps, refs = iou_data()
        m = IouAcc()
        m.initialize()
        m.compute(ids[:4], hyps[:4], refs[:4])
        m.compute(ids[4:], hyps[4:], refs[4:])
        out["iou_acc"] = {"ids": ids, "hyps": hyps, "refs": refs, "split": 4, "eval_log": m.merge_results(output_predict=True)}

        ids, logits, targets = map_data()
        m = MAP()
        m.initialize()
        m.compute(ids[:23], logits[:23], targets[:23])
        m.compute(ids[23:], logits[23:], targets[23:])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # "No positive class found in y_true" for the empty class: the value is 0.0
            log = m.merge_results(output_predict=True)
            sig = torch.sigmoid(logits)
            ap = torch.from_numpy(average_precision_score(targets.numpy(), sig.numpy(), average=None))
        assert ap.dtype == torch.float64 and float(ap.mean()) == float(log["map"])
        assert float((sig == 1.0).sum()) >= 2 and float(sig[:, 2].min()) >= 0.0
        npos = []
        for c in range(targets.shape[1]):
            want, P = exact_ap(sig[:, c], targets[:, c])
            npos.append(P)
            gate = Fraction(P + 4, 2 ** 52)
            assert abs(Fraction(float(ap[c])) - want) <= gate / 2, (c, float(ap[c]), float(want))
        assert npos[2] == 0 and float(ap[2]) == 0.0 and npos[4] == targets.shape[0] and float(ap[4]) == 1.0
        log["map"] = float(log["map"])
        out["map"] = {"ids": ids, "logits": logits, "targets": targets, "sigmoid": sig, "split": 23, "ap": ap,
                      "npos": torch.tensor(npos), "eval_log": log}
    finally:
        torch.Tensor.cuda = saved_cuda
    torch.save(out, os.path.join(HERE, "classify_metrics.pt"))
    for k in ("accuracy_hard", "accuracy_soft", "iou_acc", "map"):
        print(k, {a: b for a, b in out[k]["eval_log"].items() if a != "predict_results"})
    print("ap", out["map"]["ap"].tolist(), "npos", npos)


if __name__ == "__main__":
    main()
