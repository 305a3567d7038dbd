"""tests/gemm_ref.py checked on the CPU: the exact formulas against autograd and the oracle, the rounding model and an fp32 stand-in
(torch's fp32 matmul of the same operands + the epilogue in fp32) inside the per-element budget on every family and shape class,
every mutant of the fp64 computation REJECTED with the committed constants, the committed constants equal to the maxima of
profiles/gemm_fp64_errors_mi355x.jsonl once that record of an MI355X run is committed (until then, and so today: equal to the CPU
stand-in's figures, with gemm_ref.MEASURED_ON_MI355X false), every declared route of the GPU cases equal to route(case) from the host-only op_gemm_plan,
and the entry points' refusal of a bf16 output with ldc % 8 == 4."""
import ctypes
import json
import math
import os

import pytest
import torch

from oracle import onepeace_oracle as O
from tests import gemm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROFILE = os.path.join(ROOT, "profiles", "gemm_fp64_errors_mi355x.jsonl")


@pytest.fixture(scope="module")
def lib_path():
    import importlib.util
    spec = importlib.util.spec_from_file_location("onepeace_build", os.path.join(ROOT, "one-peace_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.build(verbose=False)


def case_of(epi, M, N, K, family, **kw):
    return R.NtCase("cpu", "cpu", epi, M, N, K, family, **kw)


def exact_of(case, seed=0):
    op = R.op_to(R.make_nt_operands(case, seed), "cpu")
    return op, R.nt_ref(op)


def gate_all(got, ex, epi, c_acc=None):
    """Failures of every output of an NT launch."""
    fails = []
    for name in ("C", "h0", "h1"):
        if name in got and name in ex:
            rounding = "f32" if (epi == R.EPI_F32 and name == "C") else "bf16"
            fails += R.gate(got[name], ex[name], ex["T"][name], rounding, G=ex.get("G") if name == "C" else None, what=name, c_acc=c_acc)[0]
    return fails


def standin(op):
    """What a kernel with fp32 accumulators computes, on the CPU: fp32 matmul, the epilogue in fp32, one rounding."""
    f = lambda t: None if t is None else t.float()  # noqa: E731
    A, epi = f(op["A"]), op["epi"]
    if epi == R.EPI_GEGLU:
        h0, h1 = A @ f(op["Ws"][0]).t(), A @ f(op["Ws"][1]).t()
        return {"C": R.bf(0.5 * h0 * (1.0 + torch.erf(h0 * (1.0 / math.sqrt(2.0)))) * h1), "h0": R.bf(h0), "h1": R.bf(h1)}
    acc = A @ torch.cat([f(w) for w in op["Ws"]], 0).t()
    bias = torch.cat([f(b) if b is not None else torch.zeros(w.shape[0]) for w, b in zip(op["Ws"], op["biases"])])
    if epi == R.EPI_BIAS:
        return {"C": R.bf(acc + bias)}
    if epi == R.EPI_F32:
        return {"C": op.get("alpha", 1.0) * acc + bias}
    y = acc + bias
    M, N = y.shape
    s = torch.ones(M, 1)
    if op.get("rowscale") is not None:
        s = f(op["rowscale"])[torch.arange(M) // max(op.get("rps", 0), 1)][:, None]
    if op.get("gamma") is not None:
        s = s * f(op["gamma"])[None, :]
    resid = f(op["resid"])
    if op.get("rows") is not None:
        resid = resid[op["rows"].clamp_min(0).long()]
    return {"C": R.bf(torch.addcmul(resid, s.expand(M, N), y)), "h0": R.bf(y)}


EPI_KW = {R.EPI_BIAS: {}, R.EPI_F32: dict(alpha=0.5), R.EPI_GEGLU: dict(h=True), R.EPI_RESID: dict(h=True, rps=7)}


def test_exact_formulas_match_autograd_and_the_oracle():
    x = torch.linspace(-12, 12, 4801, dtype=torch.float64, requires_grad=True)
    want = O.gelu_erf(x)
    assert float((R.gelu_erf(x) - want).detach().abs().max()) < 4e-15    # (two ulps of 12 between 1 + erf and erfc)
    (grad,) = torch.autograd.grad(want.sum(), x)
    assert float((R.gelu_erf_grad(x.detach()) - grad).abs().max()) < 1e-14
    # the residual formula of tests/test_ops_gpu.py::test_gemm_residual_epilogue, and the branch output
    B, S = 5, 37
    case = case_of(R.EPI_RESID, B * S, 256, 512, "unit", h=True, rps=S)
    op, ex = exact_of(case)
    y = op["A"] @ op["Ws"][0].t() + op["biases"][0]
    ref = op["resid"] + op["rowscale"].repeat_interleave(S)[:, None] * op["gamma"] * y
    assert torch.equal(ex["h0"], y) and float((ex["C"] - ref).abs().max()) < 1e-13
    op2 = dict(op, rowscale=None)
    want = O.residual_scale(y.view(B, S, -1), op["gamma"], op["resid"].view(B, S, -1)).view(B * S, -1)
    assert float((R.nt_ref(op2)["C"] - want).abs().max()) < 1e-13
    # magnitude sums dominate their outputs, whatever the signs
    for name in ("C", "h0"):
        assert bool((ex["T"][name] >= ex[name].abs() * (1 - 1e-12)).all())
    # a tail-rows remainder: m_off shifts the rowscale lookup
    rem = dict(op, A=op["A"][128:], resid=op["resid"][128:], m_off=128)
    assert torch.equal(R.nt_ref(rem)["C"], ex["C"][128:])
    # the transpose-read product and the side product
    a, b = torch.randn(64, 16, dtype=torch.float64), torch.randn(64, 256, dtype=torch.float64)
    w, base = torch.randn(16, 256, dtype=torch.float64), torch.randn(16, 256, dtype=torch.float64)
    assert float((R.tn_ref(a, b, base)[0] - (base + a.t() @ b)).abs().max()) < 1e-13
    rd, Trd = R.tn_side_ref(a, b, w)
    assert rd.shape == (2, 16) and float((rd[1] - (w * (a.t() @ b))[:, 128:].sum(1)).abs().max()) < 1e-12 and bool((Trd >= rd.abs()).all())


def test_half_ulp_and_guards():
    x = torch.tensor([1.0, 1.5, 1.9999, 2.0, 0.75, 0.0, 3e-39, -260.0], dtype=torch.float64)
    want = torch.tensor([2.0 ** -8, 2.0 ** -8, 2.0 ** -8, 2.0 ** -7, 2.0 ** -9, 2.0 ** -134, 2.0 ** -134, 1.0], dtype=torch.float64)
    assert torch.equal(R.half_ulp_bf16(x), want)
    # bf() rounds ONCE: 1 + 2^-8 + 2^-40 lies above the tie between 1 and 1 + 2^-7 (through fp32 it would land on the tie and go to even)
    t = torch.tensor([1 + 2.0 ** -8 + 2.0 ** -40, -(1 + 2.0 ** -8 + 2.0 ** -40), 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8 - 2.0 ** -40], dtype=torch.float64)
    assert R.bf(t).tolist() == [1 + 2.0 ** -7, -(1 + 2.0 ** -7), 1.0, 1 + 2.0 ** -7]
    for dtype in (torch.bfloat16, torch.float32):
        v = R.guarded((5, 24), dtype)
        buf = v._guard[0]
        assert buf.shape == (9, 32) and v.stride(0) == 32 and v.storage_offset() % 8 == 0 and bool(torch.isnan(buf.float()).all())
        v.fill_(1.0)
        assert R.check_guard(v) == 0
        buf[2, 24] = 0.5        # one element past column N of the first row
        buf[7, 0] = 0.5         # one row past M
        assert R.check_guard(v) == 2
    vec = R.guarded((40,), torch.bfloat16)
    vec.fill_(0.0)
    assert vec.storage_offset() % 8 == 0 and R.check_guard(vec) == 0
    vec._guard[0][vec.storage_offset() + 40] = 0.0
    assert R.check_guard(vec) == 1


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("epi", sorted(EPI_KW), ids=[R.EPI_NAMES[e] for e in sorted(EPI_KW)])
def test_rounding_model_is_inside_the_budget(epi, family):
    """fp64, then the one documented rounding: inside R alone (c_acc = 0; an fp32 output: its storage rounding, c_acc = 1)."""
    case = case_of(epi, 129, 72 if epi == R.EPI_GEGLU else 136, 192, family, **EPI_KW[epi])
    op, ex = exact_of(case)
    fails = gate_all(R.nt_ref(op, model=True), ex, epi, c_acc=1.0 if epi == R.EPI_F32 else 0.0)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("K", [64, 1536, 6144])
@pytest.mark.parametrize("epi", sorted(EPI_KW), ids=[R.EPI_NAMES[e] for e in sorted(EPI_KW)])
def test_fp32_stand_in_is_inside_the_budget(epi, K, family):
    case = case_of(epi, 70, 72 if epi == R.EPI_GEGLU else 136, K, family, **EPI_KW[epi])
    op, ex = exact_of(case)
    got = standin(op)
    fails = gate_all(got, ex, epi)
    assert not fails, "\n".join(fails)
    if family == "integer":
        for name, t in got.items():
            if not (epi == R.EPI_GEGLU and name == "C"):
                assert torch.equal(t.double(), ex[name] if epi == R.EPI_F32 else R.bf(ex[name])), name


def _store(view, value, past_n=False):
    """What the kernel's stores do to a guarded output; past_n: the second 8-column half-store of the last column block is issued
    although N % 16 == 8 (it lands behind column N)."""
    view.copy_(value)
    if past_n:
        buf = view._guard[0]
        r0 = view.storage_offset() // buf.stride(0)
        buf[r0:r0 + view.shape[0], view.shape[1]:view.shape[1] + 8] = value[:, -8:].to(buf.dtype)


MUTANT_CASES = {   # mutant -> (family, case): the designated family of the issue, at the smallest shape that shows the bug
    "drop_last_kstep": ("basis", case_of(R.EPI_BIAS, 129, 136, 192, "basis")),
    "bias_twice_in_fold": ("unit", case_of(R.EPI_BIAS, 129, 136, 448, "unit")),
    "y_rounded_before_layer_scale": ("unit", case_of(R.EPI_RESID, 257, 256, 512, "unit", h=True, rps=7)),
    "slab_rounded_bf16": ("cancel", case_of(R.EPI_BIAS, 129, 136, 448, "cancel", bias=(False,))),
    "geglu_halves_swapped": ("unit", case_of(R.EPI_GEGLU, 129, 72, 192, "unit", h=True)),
    "tail_rowscale_without_m_off": ("unit", case_of(R.EPI_RESID, 529, 256, 192, "unit", rps=100)),
    "segment_bias_of_neighbour": ("unit", case_of(R.EPI_BIAS, 129, 384, 128, "unit", nseg=3, bias=(True, False, True))),
}


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_every_mutant_fails(mutant):
    """Each with the committed C_ACC / C_GELU; the unmutated model passes the same gate on the same case."""
    if mutant == "accumulate_double_round":
        a, w = R.make_ab("unit", 136, 264, 192)
        A, B, base = a.t().double(), w.t().double(), R.make_vec("unit", (136, 264), 40, "resid").double()
        exact, T = R.tn_ref(A, B, base)
        assert not R.gate(R.tn_ref(A, B, base, model=True)[0], exact, T, "bf16")[0]
        assert R.gate(R.tn_ref(A, B, base, model=True, mutant=mutant)[0], exact, T, "bf16")[0]
        return
    if mutant == "second_half_store_past_N":   # caught by the guard, not by the gate
        case = case_of(R.EPI_BIAS, 17, 72, 128, "unit")
        op, ex = exact_of(case)
        good, bad = R.guarded((17, 72), torch.bfloat16), R.guarded((17, 72), torch.bfloat16)
        _store(good, R.nt_ref(op, model=True)["C"])
        _store(bad, R.nt_ref(op, model=True)["C"], past_n=True)
        assert R.check_guard(good) == 0 and R.check_guard(bad) == 17 * 8
        assert not R.gate(bad, ex["C"], ex["T"]["C"], "bf16")[0]    # the values themselves are right: only the guard sees it
        return
    family, case = MUTANT_CASES[mutant]
    op, ex = exact_of(case)
    if mutant == "slab_rounded_bf16":
        op["splits"] = R.split_ranges(case.K, 3)
    assert not gate_all(R.nt_ref(op, model=True), ex, case.epi)
    fails = gate_all(R.nt_ref(op, model=True, mutant=mutant), ex, case.epi)
    assert fails, "%s passes the gate" % mutant


def test_constants():
    """C_ACC <= 16 is a condition.  At 16 the fp32 allowance of the `unit` family at K = 1536 is below 2 % of the bf16 half ulp on the
    typical element: a kernel that is one ulp off cannot hide in it.  With the record of the MI355X run committed, the constants
    are its maxima; without it (MEASURED_ON_MI355X false) they are the CPU stand-in's figures, measured again here."""
    assert R.C_ACC == R.MARGIN * R.MEASURED_MAX_RATIO["acc"] <= 16.0 and R.MARGIN == 2.0
    assert R.C_GELU == R.MARGIN * R.MEASURED_MAX_RATIO["gelu"]
    op, ex = exact_of(case_of(R.EPI_BIAS, 129, 136, 1536, "unit"))
    Rr, f32 = R.budget(ex["C"], ex["T"]["C"], "bf16", c_acc=16.0)
    assert float((f32 / Rr).median()) < 0.02
    assert R.MEASURED_ON_MI355X == os.path.exists(PROFILE), "the record and the flag that says the constants come from it go together"
    if R.MEASURED_ON_MI355X:
        recs = [json.loads(l) for l in open(PROFILE) if l.strip()]
        acc = max(r["fig"]["acc_f32"] for r in recs if "acc_f32" in r["fig"])
        gelu = max(r["fig"]["gelu"] for r in recs if "gelu" in r["fig"] and r["family"] in ("integer", "basis"))
        assert abs(acc - R.MEASURED_MAX_RATIO["acc"]) <= 5e-4 * acc and abs(gelu - R.MEASURED_MAX_RATIO["gelu"]) <= 5e-4 * gelu
        assert all(r["gate_failures"] == 0 and r["repeat_same_bits"] for r in recs)
        return
    # NO record of an MI355X run is committed: the constants are the CPU stand-in's figures, measured here the way the GPU test
    # measures them (the largest ratio, rounded up to the committed digits)
    acc = gelu = 0.0
    for family in R.FAMILIES:
        for K in (64, 1536, 6144):
            op, ex = exact_of(case_of(R.EPI_F32, 70, 136, K, family, alpha=0.5))
            acc = max(acc, R.gate(standin(op)["C"], ex["C"], ex["T"]["C"], "f32")[1]["acc"])
            if family in ("integer", "basis"):   # exact accumulators: the error of the fp32 product BEFORE its rounding is the epilogue's
                op, ex = exact_of(case_of(R.EPI_GEGLU, 70, 72, K, family, h=True))
                h0, h1 = (op["A"].float() @ op["Ws"][i].float().t() for i in (0, 1))
                c32 = 0.5 * h0 * (1.0 + torch.erf(h0 * (1.0 / math.sqrt(2.0)))) * h1
                gelu = max(gelu, float(((c32.double() - ex["C"]).abs() / (R.U32 * ex["G"]).clamp_min(1e-300)).max()))
    print("CPU stand-in: acc %.4f gelu %.4f" % (acc, gelu))
    assert 0.5 * R.MEASURED_MAX_RATIO["acc"] <= acc <= R.MEASURED_MAX_RATIO["acc"]
    assert 0.5 * R.MEASURED_MAX_RATIO["gelu"] <= gelu <= R.MEASURED_MAX_RATIO["gelu"]


def test_every_gpu_case_declares_the_route_the_planner_takes(lib_path):
    from one_peace_amd import hip
    wrong = [(c.id, R.route(c, hip)) for c in R.NT_CASES if R.route(c, hip) != c.route]
    assert not wrong, wrong[:5]
    names = " ".join(c.id for c in R.NT_CASES)
    for r in ("nt128-", "nt128_regstaged-", "g256_bk32-", "g256b-", "g256v-", "g256p-", "+splitk_reduce", "+fold", "+tail128", "+tail256",
              "g256_bk32+splitk_reduce"):
        assert r in names, r
    # the restated planner of op_gemm_tn (the GPU test checks it against the scratch the launch leaves): the split the ids promise
    assert R.tn_route(264, 264, 2112, True, False, 1) == ("tn8w+splitk_reduce4", [(0, 576), (576, 1152), (1152, 1728), (1728, 2112)])
    assert R.tn_route(264, 264, 2112, False, True, 3) == ("tn4w+resid", []) and R.tn_route(8, 8, 64, True, False, 1) == ("tn8w", [])
    assert R.split_ranges(448, 2) == [(0, 256), (256, 448)] and R.split_ranges(448, 3) == [(0, 192), (192, 384), (384, 448)]


def test_bf16_outputs_need_ldc_multiple_of_8(lib_path):
    """Every kernel stores an output row in 16-byte pieces at m * ldc + 8 j: a bf16 output at ldc % 8 == 4 would be misaligned on every
    odd row.  The entry points refuse it before anything is launched (no GPU needed; the pointers are never followed)."""
    from one_peace_amd import hip
    lib = hip.lib()
    p = ctypes.c_void_p(4096)
    null = ctypes.c_void_p(None)

    def nt(ldc, epi):   # M = 0: the entry point returns 0 right after its argument checks -- nothing can ever be launched from here
        return lib.op_gemm_nt(p, 64, p, null, null, 64, 0, null, null, null, p, ldc, null, null, p, 16, null, null, 0, null, 0, 8, 64, epi,
                              null, 0, 0, null, 0, null)

    for epi in (R.EPI_BIAS, R.EPI_GEGLU, R.EPI_RESID):
        assert nt(12, epi) == -22 and b"ldc" in lib.op_last_error()
        assert nt(16, epi) == 0
    assert nt(10, R.EPI_F32) == -22 and b"ldc" in lib.op_last_error()
    assert nt(12, R.EPI_F32) == 0
    batched = lambda ldc, stride_c: lib.op_gemm_nt_batched(p, 64, 64, p, 64, 512, null, 0, p, ldc, stride_c, 0, 8, 64, 2, null)  # noqa: E731
    assert batched(12, 48) == -22 and batched(16, 44) == -22 and batched(16, 48) == 0
    # op_gemm_tn has no early return to hide behind: its refusal (-95, the caller falls back) is visible through the host-side twin
    # the callers ask first, and ops.wgrad hands the output's leading dimension to it
    assert not hip.gemm_tn_supported(64, 8, 8, 8, 8, 12) and hip.gemm_tn_supported(64, 8, 8, 8, 8, 16)
