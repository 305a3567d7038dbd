"""The GEMM kernels of csrc/gemm.hip and csrc/gemm_epilogue_v.h against fp64 on the SAME bf16 inputs, PER ELEMENT, on every route the
launch planner can take (tests/gemm_ref.py: exact results, budget, families, guards, route mirror, case list).

Every test allocates every operand and every output inside guarded buffers (NaN around the inputs, a sentinel bit pattern around C,
h0, h1 with ld = N + 8), launches twice and requires identical bits, gates every output element with

    |got - exact|  <=  R + C_ACC * 2^-24 * T

(R: the one documented rounding of that output, T: the magnitude sum; no norms), checks the guards, and appends the case's largest
|err| / (2^-24 T) and |err| / R to gemm_fp64_errors.jsonl in the tests' output directory (tests/util.py: out_dir()).  C_ACC and
C_GELU are to be measured from that record (committed as profiles/gemm_fp64_errors_mi355x.jsonl).  OUTSTANDING: this file has not yet
run on an MI355X, no record is committed, and the constants are the CPU stand-in's (tests/gemm_ref.py: MEASURED_ON_MI355X = False) -- a
GeGLU case may miss the gate on the device's erf until C_GELU is measured there.  In the `integer` family every fp32 operation is
exact: every output but the GeGLU product must EQUAL the exact value (rounded once where it is stored as bf16).

NT case ids carry the route the case was written for, and the test asserts route(case) -- built from op_gemm_plan, the four-wave rule
and the TUNE fields -- returns it:

  nt128 / nt128_regstaged    128 x 128 kernel, LDS-DMA / register staging: all epilogues; 1-3 segments of 128 with null biases; GeGLU
                             at F = 8, 72 with and without h0 / h1; residual with / without gamma and rowscale, in place, rows_per_sample = 7,
                             row tables with dropped rows; N % 16 == 8 (the partial half-stores)
  g256_bk32 g256b g256v      256 x 256 kernels (tile_mode = 2; fullline = 0, 1, 3 + sched = 3): all epilogues, segments of 256, alpha;
  g256p                      the persistent kernel on a single problem (sched = 6): bias and residual; row tables on g256v / g256p
  ...+splitk_reduce          K = 448 split in 2 (4 + 3 K-tiles) and 3 (3 + 3 + 1) without a bias: the fp32 slabs are read back from the
                             scratch and gated with R = 0; 256 x 256 slabs at the smallest problem the planner splits (5632 x 768 x 4096)
  ...+fold                   bias, residual and residual-with-row-table epilogues in splitk_fold_epilogue_kernel
  ...+tail256                tail-rows split under tile_mode = 2 (M = 257, 384, 529; rows_per_sample = 100 straddles the split: m_off)
  g256p+tail128+fold         default tiles: the one leftover row of 5633 as a 128 x 128 launch that splits K and folds on its own
  grouped_p / grouped_v      gemm_nt_grouped, persistent and sched = 7: one to three problems of 1, 257, 300 rows, row tables
  batched                    gemm_nt_batched, G = 3, overlapping row patches
  tn8w / tn4w (+splitk_reduceN | +resid)   gemm_tn, both flavours, fresh and accumulating, K = 64 and 2112 (66 k-steps: 18 + 18 + 18 + 12)
  wgrad, tn_grouped          ops.wgrad at 96 * 5 + 7 rows; gemm_tn_grouped with three K, mixed accumulate flags and the side product

Misaligned leading dimensions are not launched (the entry points refuse them: tests/test_gemm_ref_cpu.py)."""
import json
import os
import time

import pytest
import torch

from tests import gemm_ref as R
from tests.util import out_dir

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32


def hipmod():
    from one_peace_amd import hip
    return hip


def g(t, dtype=BF, **kw):
    return R.guarded_from(t, dtype, device=DEV, **kw)


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


def record(rec, t0):
    rec["seconds"] = round(time.time() - t0, 3)
    with open(os.path.join(out_dir(), "gemm_fp64_errors.jsonl"), "a") as f:
        f.write(json.dumps(rec) + "\n")
    print(json.dumps(rec))


class Figures:
    """Collects the gate's failures and the largest figures of a case."""

    def __init__(self, family):
        self.family, self.fails, self.fig = family, [], {}

    def gate(self, got, exact, T, rounding, what, G=None, equal_ok=True, key=None):
        """key: the record's name of |err| / (2^-24 T); "acc_f32" (what C_ACC is measured from) for an fp32 output, "acc" for a bf16 one."""
        fails, fig = R.gate(got, exact, T, rounding, G=G, what=what)
        self.fails += fails
        key = key or ("acc_f32" if rounding == "f32" else "acc")
        for k, v in fig.items():
            k = key if k == "acc" else k
            self.fig[k] = max(self.fig.get(k, 0.0), v)
        if self.family == "integer" and equal_ok:   # every partial sum and every epilogue operation is exact
            want = exact if rounding == "f32" else R.bf(exact)
            if not torch.equal(got.double(), want):
                self.fails.append("%s: not equal to the exact value in the integer family (%d elements)" % (what, int((got.double() != want).sum())))

    def guard(self, view, what):
        n = R.check_guard(view)
        if n:
            self.fails.append("%s: %d guard elements overwritten" % (what, n))


# ----------------------------------------------------------------------------------------------------------------------
# op_gemm_nt
# ----------------------------------------------------------------------------------------------------------------------
class NtDevice:
    """The guarded device operands of an NT case and one launch of it."""

    def __init__(self, case, op):
        self.case, self.op = case, op
        self.A, self.Ws = g(op["A"]), [g(w) for w in op["Ws"]]
        self.biases = [g(b) for b in op["biases"]]
        self.resid0 = op.get("resid")
        self.gamma = g(op.get("gamma"))
        self.rowscale = g(op.get("rowscale"), F32)
        self.rows = g(op.get("rows"), torch.int32)
        self.alpha = torch.tensor([op["alpha"]], dtype=F32, device=DEV) if "alpha" in op else None
        M, N = case.M, case.N
        self.rows_total = self.resid0.shape[0] if self.resid0 is not None else M
        self.resid = g(self.resid0) if self.resid0 is not None else None
        self.C = self.resid if case.alias else R.guarded((self.rows_total, N), F32 if case.epi == R.EPI_F32 else BF, device=DEV)
        self.h0 = R.guarded((M, N), BF, device=DEV) if case.h else None
        self.h1 = R.guarded((M, N), BF, device=DEV) if case.h and case.epi == R.EPI_GEGLU else None
        self.C_before = None

    def launch(self):
        hip, case = hipmod(), self.case
        if self.resid is not None:
            self.resid.copy_(self.resid0.to(DEV))
        if not case.alias:
            self.C.fill_(3.0 if case.rows else float("nan"))   # row table: the rows no entry names must stay as they are
        for h in (self.h0, self.h1):
            if h is not None:
                h.fill_(float("nan"))
        self.C_before = self.C.clone()
        geglu = case.epi == R.EPI_GEGLU
        hip.gemm_nt(self.A, self.Ws, None if geglu else self.biases, out=self.C, epilogue=case.epi, n_seg=0 if geglu else case.N // case.nseg,
                    h0=self.h0, h1=self.h1, resid=self.resid, gamma=self.gamma, rowscale=self.rowscale, rows_per_sample=case.rps,
                    alpha=self.alpha, N=None if geglu else case.N, splitk=case.splitk, resid_rows=self.rows)
        torch.cuda.synchronize()
        return [t.clone() if t is not None else None for t in (self.C, self.h0, self.h1)]


@pytest.mark.parametrize("case", R.NT_CASES, ids=[c.id for c in R.NT_CASES])
def test_gemm_nt_against_fp64(case):
    hip = hipmod()
    t0 = time.time()
    assert R.route(case, hip) == case.route
    op = R.make_nt_operands(case)
    d = NtDevice(case, op)
    try:
        R.apply_tune(hip, case.tune)
        first = d.launch()
        slabs = None
        if case.slabs:
            ranges = R.split_ranges(case.K, case.tune["force_splits"])
            ws = hip.workspace(1, torch.device(DEV, torch.cuda.current_device()), "gemm_splitk").view(F32)
            slabs = [ws[z * case.M * case.N:(z + 1) * case.M * case.N].view(case.M, case.N).clone() for z in range(len(ranges))]
        again = d.launch()
    finally:
        hip.TUNE.reset()
    same = all(a is None or torch.equal(bits(a), bits(b)) for a, b in zip(first, again))
    C, h0, h1 = first
    opd = R.op_to(op, DEV)
    ex = R.nt_ref(opd)
    F = Figures(case.family)
    rounding = "f32" if case.epi == R.EPI_F32 else "bf16"
    if case.rows:
        rows = opd["rows"].long()
        keep = rows >= 0
        F.gate(C[rows[keep]], ex["C"][keep], ex["T"]["C"][keep], rounding, "C")
        untouched = torch.ones(d.rows_total, dtype=torch.bool, device=DEV)
        untouched[rows[keep]] = False
        if not torch.equal(bits(C[untouched]), bits(d.C_before[untouched])):
            F.fails.append("C: a row that the row table does not name was written")
    else:
        F.gate(C, ex["C"], ex["T"]["C"], rounding, "C", G=ex.get("G"), equal_ok=case.epi != R.EPI_GEGLU)
    if h0 is not None:
        F.gate(h0, ex["h0"], ex["T"]["h0"], "bf16", "h0")
    if h1 is not None:
        F.gate(h1, ex["h1"], ex["T"]["h1"], "bf16", "h1")
    if slabs is not None:
        A, W = opd["A"], torch.cat(opd["Ws"], 0)
        for z, (k0, k1) in enumerate(ranges):
            F.gate(slabs[z], A[:, k0:k1] @ W[:, k0:k1].t(), A[:, k0:k1].abs() @ W[:, k0:k1].abs().t(), "f32", "slab%d" % z)
    for name, t in (("C", d.C), ("h0", d.h0), ("h1", d.h1)):
        if t is not None:
            F.guard(t, name)
    record({"case": case.id, "op": "gemm_nt", "route": case.route, "family": case.family, "fig": F.fig, "repeat_same_bits": same,
            "gate_failures": len(F.fails)}, t0)
    assert same, "a repeated launch returned different bits"
    assert not F.fails, "\n".join(F.fails)


# ----------------------------------------------------------------------------------------------------------------------
# op_gemm_nt_grouped
# ----------------------------------------------------------------------------------------------------------------------
GROUPED = [(n, K, epi, sched, rows, fam)
           for n in (1, 2, 3) for K in (128, 192) for epi in (R.EPI_BIAS, R.EPI_RESID) for sched in (0, 7)
           for rows in ((False, True) if epi == R.EPI_RESID else (False,)) for fam in (("unit", "cancel") if K == 192 else ("unit",))]
GROUPED += [(3, 192, R.EPI_RESID, sched, rows, fam) for sched in (0, 7) for rows in (False, True) for fam in R.FAMILIES if fam not in ("unit", "cancel")]


@pytest.mark.parametrize("n,K,epi,sched,rows,family", GROUPED,
                         ids=["grouped_%s-%s-n%d-K%d-%s%s" % ("v" if s == 7 else "p", R.EPI_NAMES[e], n, K, f, "-rows" if r else "") for n, K, e, s, r, f in GROUPED])
def test_gemm_nt_grouped_against_fp64(n, K, epi, sched, rows, family):
    """Problems of 1, 257 and 300 rows (N = 256) in ONE launch: per-problem weights, biases (the middle one null), gamma, rowscale and
    rows_per_sample (7, 100, 1), the branch output h0; with row tables all problems write their rows of ONE full matrix."""
    hip = hipmod()
    t0 = time.time()
    Ms, N, rps = (1, 257, 300)[:n], 256, (7, 100, 1)
    cases = [R.NtCase("grouped", "grouped", epi, Ms[i], N, K, family, bias=(i != 1,), h=epi == R.EPI_RESID, rps=rps[i]) for i in range(n)]
    ops = [R.make_nt_operands(c, seed=i) for i, c in enumerate(cases)]
    total = sum(Ms) + 9
    table = R.make_row_table(sum(Ms), total, 5) if rows else None
    off = [sum(Ms[:i]) for i in range(n)]
    As, Ws = [g(o["A"]) for o in ops], [g(o["Ws"][0]) for o in ops]
    bs = [g(o["biases"][0]) for o in ops]
    resid = gammas = rowscales = h0s = tabs = None
    full0 = None
    if epi == R.EPI_RESID:
        gammas, rowscales = [g(o["gamma"]) for o in ops], [g(o["rowscale"], F32) for o in ops]
        h0s = [R.guarded((m, N), BF, device=DEV) for m in Ms]
        if rows:
            full0 = R.make_vec(family, (total, N), 31, "resid")
            tabs = [g(table[off[i]:off[i] + Ms[i]], torch.int32) for i in range(n)]
            for i, o in enumerate(ops):
                o["resid"], o["rows"] = full0, table[off[i]:off[i] + Ms[i]]
    full = R.guarded((total, N), BF, device=DEV) if rows else None
    outs = [full] * n if rows else [R.guarded((m, N), BF, device=DEV) for m in Ms]

    def launch():
        if rows:
            full.copy_(full0.to(DEV))
            res = [full] * n
        else:
            for o in outs:
                o.fill_(float("nan"))
            res = [g(o["resid"]) for o in ops] if epi == R.EPI_RESID else None
        for h in h0s or ():
            h.fill_(float("nan"))
        got = hip.gemm_nt_grouped(As, Ws, biases=bs, outs=outs, epilogue=epi, h0s=h0s, resids=res, gammas=gammas, rowscales=rowscales,
                                  rows_per_sample=list(rps[:n]), resid_rows=tabs)
        assert got is not None, "the grouped launch refused the shape"
        torch.cuda.synchronize()
        return [o.clone() for o in (outs[:1] if rows else outs)] + [h.clone() for h in h0s or ()]

    try:
        R.apply_tune(hip, dict(sched=sched))
        first = launch()
        again = launch()
    finally:
        hip.TUNE.reset()
    same = all(torch.equal(bits(a), bits(b)) for a, b in zip(first, again))
    F = Figures(family)
    named = torch.zeros(total, dtype=torch.bool, device=DEV)
    for i, o in enumerate(ops):
        opd = R.op_to(o, DEV)
        ex = R.nt_ref(opd)
        if rows:
            r = opd["rows"].long()
            keep = r >= 0
            named[r[keep]] = True
            F.gate(first[0][r[keep]], ex["C"][keep], ex["T"]["C"][keep], "bf16", "C%d" % i)
        else:
            F.gate(first[i], ex["C"], ex["T"]["C"], "bf16", "C%d" % i)
            F.guard(outs[i], "C%d" % i)
        if h0s:
            F.gate(h0s[i], ex["h0"], ex["T"]["h0"], "bf16", "h0_%d" % i)
            F.guard(h0s[i], "h0_%d" % i)
    if rows:
        F.guard(full, "C")
        if not torch.equal(bits(first[0][~named]), bits(full0.to(DEV).to(BF)[~named])):
            F.fails.append("C: a row that no row table names was written")
    record({"case": "grouped_%s-%s-n%d-K%d-%s%s" % ("v" if sched == 7 else "p", R.EPI_NAMES[epi], n, K, family, "-rows" if rows else ""),
            "op": "gemm_nt_grouped", "route": "grouped_v" if sched == 7 else "grouped_p", "family": family, "fig": F.fig,
            "repeat_same_bits": same, "gate_failures": len(F.fails)}, t0)
    assert same, "a repeated launch returned different bits"
    assert not F.fails, "\n".join(F.fails)


# ----------------------------------------------------------------------------------------------------------------------
# op_gemm_nt_batched
# ----------------------------------------------------------------------------------------------------------------------
BATCHED = [(rows, N, K, True, fam) for rows, N, K in ((70, 136, 128), (129, 8, 192)) for fam in ("unit", "offset", "integer", "nonfinite")]
BATCHED += [(129, 136, 192, False, fam) for fam in R.FAMILIES]


@pytest.mark.parametrize("use_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("rows,N,K,overlap,family", BATCHED, ids=["%d-%d-%d-%s-%s" % (r, n, k, "overlap" if o else "apart", f) for r, n, k, o, f in BATCHED])
def test_gemm_nt_batched_against_fp64(rows, N, K, overlap, family, use_bias):
    """G = 3 problems in one launch.  overlap: the A rows are K-wide patches of ONE flat vector, 72 elements apart (lda < K), the batches
    16 elements apart (stride_a < rows * lda).  Rows that share their elements cannot carry a per-row structure: `cancel`, `wide` and
    `basis` run on the second layout (apart: a [G * rows, K] matrix with lda = K + 8, every batch with operands of its own), where every
    family does; the overlapping one takes what a flat vector can hold (unit, offset, integer, a NaN among them).
    The binding takes contiguous W [G, N, K], bias [G, N] and C [G, rows, N] (ldb = K, ldc = N): those three are guarded by rows above
    and below, not by columns."""
    hip = hipmod()
    t0 = time.time()
    G = 3
    if overlap:
        lda, stride_a = 72, 16
        L = (G - 1) * stride_a + (rows - 1) * lda + K
        flat, W = R.make_ab("unit" if family == "nonfinite" else family, 1, G * N, max(L, K))
        flat = flat[0, :L].contiguous()
        W = W[:, :K].contiguous()
        if family == "nonfinite":
            flat[L // 2], W[N // 2, K // 3] = float("nan"), float("inf")
        fd = g(flat)
        A = fd.as_strided((G, rows, K), (stride_a, lda, 1))
    else:
        ab = [R.make_ab(family, rows, N, K, seed=z) for z in range(G)]
        W = torch.cat([w for _, w in ab], 0)
        Ag = g(torch.cat([a for a, _ in ab], 0))
        A = Ag.as_strided((G, rows, K), (rows * Ag.stride(0), Ag.stride(0), 1))
    bias = R.make_vec(family, (G, N), 3, "bias") if use_bias else None
    Wd = g(W, ld_extra=0).view(G, N, K)
    bd = g(bias, ld_extra=0) if use_bias else None
    out = R.guarded((G * rows, N), BF, ld_extra=0, device=DEV)

    def launch():
        out.fill_(float("nan"))
        hip.gemm_nt_batched(A, Wd, bd, out.view(G, rows, N), rows, K)
        torch.cuda.synchronize()
        return out.clone()

    first, again = launch(), launch()
    Ad = A.double()
    F = Figures(family)
    for z in range(G):
        exact, T = Ad[z] @ Wd[z].double().t(), Ad[z].abs() @ Wd[z].double().abs().t()
        if use_bias:
            exact, T = exact + bd[z].double(), T + bd[z].double().abs()
        F.gate(first[z * rows:(z + 1) * rows], exact, T, "bf16", "C%d" % z)
    F.guard(out, "C")
    same = torch.equal(bits(first), bits(again))
    record({"case": "batched-%d-%d-%d-%s-%s-%s" % (rows, N, K, "overlap" if overlap else "apart", "bias" if use_bias else "nobias", family),
            "op": "gemm_nt_batched", "route": "batched", "family": family, "fig": F.fig, "repeat_same_bits": same, "gate_failures": len(F.fails)}, t0)
    assert same, "a repeated launch returned different bits"
    assert not F.fails, "\n".join(F.fails)


# ----------------------------------------------------------------------------------------------------------------------
# op_gemm_tn, ops.wgrad, op_gemm_tn_grouped
# ----------------------------------------------------------------------------------------------------------------------
def _tn_cases():
    c = []
    for fam in ("unit", "cancel"):
        for fl in (1, 3):
            for M, N in ((8, 8), (136, 264), (264, 136), (264, 264), (8, 264), (136, 8)):
                for K in (64, 2112):
                    for splitk in ((True, False) if K > 64 else (False,)):
                        for acc in (False, True):
                            c.append((fam, fl, M, N, K, splitk, acc))
    for fam in R.FAMILIES:
        if fam not in ("unit", "cancel"):
            for fl in (1, 3):
                for K, splitk in ((2112, True), (192, False)):
                    for acc in (False, True):
                        c.append((fam, fl, 264, 136, K, splitk, acc))
    return c


TN_CASES = _tn_cases()


def _tn_id(fam, fl, M, N, K, splitk, acc):
    return "%s-M%d-N%d-K%d-%s%s%s" % (R.tn_route(M, N, K, splitk, acc, fl)[0], M, N, K, fam, "" if splitk else "-nosplit", "-acc" if acc else "")


def _tn_operands(fam, M, N, K, seed=0):
    """A_km [K, M], B_kn [K, N] (the families of make_ab run along K: a = A_km^T, w = B_kn^T) and a base [M, N]."""
    a, w = R.make_ab(fam, M, N, K, seed)
    return a.t().contiguous(), w.t().contiguous(), R.make_vec(fam, (M, N), 40 + seed, "resid")


@pytest.mark.parametrize("fam,fl,M,N,K,splitk,acc", TN_CASES, ids=[_tn_id(*c) for c in TN_CASES])
def test_gemm_tn_against_fp64(fam, fl, M, N, K, splitk, acc):
    """Strided operands (lda = M + 8, ldb = N + 8, ldc = N + 8).  An accumulating launch rounds base + product ONCE on both routes (the
    split-K reduce adds the slabs to the bf16 base in fp32; the unsplit launch goes through the residual epilogue).
    The route in the id is asserted through the scratch: it is filled with NaN before the launch; a route named +splitk_reduceN must
    leave N fp32 slabs there that pass the gate with R = 0 against fp64 over THEIR K-range, any other route must leave it untouched."""
    hip = hipmod()
    t0 = time.time()
    A, B, base = _tn_operands(fam, M, N, K)
    Ad, Bd = g(A), g(B)
    out = R.guarded((M, N), BF, device=DEV)
    name, ranges = R.tn_route(M, N, K, splitk, acc, fl)
    probe = 4 * M * N        # floats: room for four slabs, the most any case here splits into
    assert len(ranges) <= 4
    ws = hip.workspace(hip.SPLITK_WS_BYTES, Ad.device, "gemm_splitk").view(F32)

    def launch():
        out.copy_(base.to(DEV)) if acc else out.fill_(float("nan"))
        ws[:probe].fill_(float("nan"))
        hip.gemm_tn(Ad, Bd, out=out, accumulate=acc, splitk=splitk)
        torch.cuda.synchronize()
        return out.clone()

    try:
        R.apply_tune(hip, dict(fullline=fl))
        first, again = launch(), launch()
    finally:
        hip.TUNE.reset()
    D, X = A.to(DEV).double(), B.to(DEV).double()
    exact, T = R.tn_ref(D, X, base.to(DEV).double() if acc else None)
    F = Figures(fam)
    F.gate(first, exact, T, "bf16", "C")
    F.guard(out, "C")
    for z, (k0, k1) in enumerate(ranges):
        ex_z, T_z = R.tn_ref(D[k0:k1], X[k0:k1])
        F.gate(ws[z * M * N:(z + 1) * M * N].view(M, N), ex_z, T_z, "f32", "slab%d" % z)
    rest = ws[len(ranges) * M * N:probe]
    if not bool(torch.isnan(rest).all()):
        F.fails.append("the split-K scratch was written beyond the %d slabs of %s" % (len(ranges), name))
    same = torch.equal(bits(first), bits(again))
    record({"case": _tn_id(fam, fl, M, N, K, splitk, acc), "op": "gemm_tn", "route": name,
            "family": fam, "fig": F.fig, "repeat_same_bits": same, "gate_failures": len(F.fails)}, t0)
    assert same, "a repeated launch returned different bits"
    assert not F.fails, "\n".join(F.fails)


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("acc", [False, True], ids=["fresh", "acc"])
@pytest.mark.parametrize("M,N", [(136, 264), (256, 384)])
def test_wgrad_with_leftover_rows_against_fp64(M, N, acc, fam):
    """ops.wgrad at 96 * 5 + 7 = 487 rows: the 448 rows the transpose-read kernel takes, then the 39 leftover rows as a second,
    accumulating launch over a zero-padded copy.  TWO documented roundings: bf16 after the main launch, bf16 after the second."""
    from one_peace_amd import ops
    t0 = time.time()
    rows = 96 * 5 + 7
    dy, x, base = _tn_operands(fam, M, N, rows)
    dyd, xd = g(dy), g(x)
    out = R.guarded((M, N), BF, device=DEV)

    def launch():
        out.copy_(base.to(DEV)) if acc else out.fill_(float("nan"))
        ops.wgrad(dyd, xd, out=out, accumulate=acc)
        torch.cuda.synchronize()
        return out.clone()

    first, again = launch(), launch()
    K0 = rows - rows % 64
    D, X = dy.to(DEV).double(), x.to(DEV).double()
    first_stage, T0 = R.tn_ref(D[:K0], X[:K0], base.to(DEV).double() if acc else None)
    tail, T1 = R.tn_ref(D[K0:], X[K0:])
    exact, T = first_stage + tail, T0 + T1
    fin = torch.isfinite(exact) & torch.isfinite(T)       # (`nonfinite`: got must be non-finite exactly where exact is)
    fails = ["%d elements differ from the exact result in finiteness" % int((fin != torch.isfinite(first)).sum())] if not torch.equal(fin, torch.isfinite(first)) else []
    z = torch.zeros_like(exact)
    exact, T, first_stage, got = (torch.where(fin, t, z) for t in (exact, T, first_stage, first.double()))
    _, f32 = R.budget(exact, T, "bf16")
    err = (got - exact).abs()
    R0 = R.half_ulp_bf16(first_stage.abs() + f32)
    bound = R0 + R.half_ulp_bf16(exact.abs() + R0 + f32) + f32    # (the second rounding happens within R0 + f32 of the exact value)
    bad = ~(err <= bound)
    if bool(bad.any()):
        fails.append("%d of %d elements outside two roundings + the fp32 allowance (worst %.3e > %.3e)" % (
            int(bad.sum()), bad.numel(), float(err[bad].max()), float(bound[bad].max())))
    if fam == "integer" and not torch.equal(first.double(), R.bf(R.bf(first_stage) + tail)):
        fails.append("not equal to the twice-rounded exact value in the integer family")
    if R.check_guard(out):
        fails.append("guard overwritten")
    same = torch.equal(bits(first), bits(again))
    record({"case": "wgrad-M%d-N%d-K%d-%s-%s" % (M, N, rows, fam, "acc" if acc else "fresh"), "op": "wgrad", "route": "wgrad", "family": fam,
            "fig": {"acc": float((err / (R.U32 * T).clamp_min(1e-300)).max()), "R": float((err / (bound - f32)).max())}, "repeat_same_bits": same,
            "gate_failures": len(fails)}, t0)
    assert same, "a repeated launch returned different bits"
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fam", R.FAMILIES)
@pytest.mark.parametrize("nwg", [0, 5])
def test_gemm_tn_grouped_against_fp64(nwg, fam):
    """Four problems of different K in one persistent launch, accumulate flags mixed, the side product on two of them (rowdot from the
    launch's own fp32 product: R = 0; with rscale the gradient receives rscale[m] * product, rounded once with its base)."""
    hip = hipmod()
    t0 = time.time()
    specs = [(128, 256, 256, True, "side+rscale"), (192, 264, 136, False, None), (448, 512, 256, True, "side"), (64, 8, 8, True, None)]
    host, probs = [], []
    for i, (K, M, N, acc, side) in enumerate(specs):
        A, B, base = _tn_operands(fam, M, N, K, seed=i)
        Wm = R.make_vec(fam, (M, N), 60 + i, "resid") if side else None
        rs = R.make_vec(fam, M, 70 + i, "gamma") if side == "side+rscale" else None
        host.append((A, B, base, Wm, rs))
        out = R.guarded((M, N), BF, device=DEV)
        sd = None
        if side:
            rd = R.guarded((N // 128, M), F32, ld_extra=0, device=DEV)
            sd = (g(Wm), rd) + ((g(rs),) if rs is not None else ())
        probs.append((g(A), g(B), out, acc, sd))

    def launch():
        for (A, B, base, Wm, rs), q in zip(host, probs):
            q[2].copy_(base.to(DEV)) if q[3] else q[2].fill_(float("nan"))
            if q[4] is not None:
                q[4][1].fill_(float("nan"))
        assert hip.gemm_tn_grouped(probs, tune=nwg), "the grouped launch refused a problem"
        torch.cuda.synchronize()
        return [q[2].clone() for q in probs] + [q[4][1].clone() for q in probs if q[4] is not None]

    first, again = launch(), launch()
    F = Figures(fam)
    for i, ((A, B, base, Wm, rs), q) in enumerate(zip(host, probs)):
        Ad, Bd = A.to(DEV).double(), B.to(DEV).double()
        exact, T = R.tn_ref(Ad, Bd, base.to(DEV).double() if q[3] else None, rscale=rs.to(DEV).double() if rs is not None else None)
        F.gate(first[i], exact, T, "bf16", "C%d" % i)
        F.guard(q[2], "C%d" % i)
        if q[4] is not None:
            ex, Ts = R.tn_side_ref(Ad, Bd, Wm.to(DEV).double())
            F.gate(q[4][1], ex, Ts, "f32", "rowdot%d" % i, key="acc_rowdot")
            F.guard(q[4][1], "rowdot%d" % i)
    same = all(torch.equal(bits(a), bits(b)) for a, b in zip(first, again))
    record({"case": "tn_grouped-nwg%d-%s" % (nwg, fam), "op": "gemm_tn_grouped", "route": "tn_grouped", "family": fam, "fig": F.fig,
            "repeat_same_bits": same, "gate_failures": len(F.fails)}, t0)
    assert same, "a repeated launch returned different bits"
    assert not F.fails, "\n".join(F.fails)
