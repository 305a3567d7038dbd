"""tests/rows_ref.py checked without a GPU: the closed forms against fp64 autograd through the oracle's formulas, the fp32 re-statement
of every kernel inside every budget (the largest share is printed), every mutant of the computation failing the gate on a case that
the test names, the numbers of the dispatch mirror at the listed sizes, and the condition that the fp32 allowance stays a quarter of
the bf16 rounding on the `unit` family."""
import pytest
import torch

from oracle import onepeace_oracle as O
from tests import rows_ref as R

BF, F32 = R.BF, R.F32


def rd(dtype):
    return "bf16" if dtype == BF else "f32"


def close(a, b, what):
    err, ref = float((a - b).abs().max()), float(b.abs().max())
    assert err <= 1e-12 * max(ref, 1e-300) or err == 0, "%s: %.3e against max %.3e" % (what, err, ref)


# ---- 1. closed forms against autograd ---------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["unit", "offset", "dropped"])
@pytest.mark.parametrize("rps", [1, 3])
def test_resid_closed_forms_against_autograd(family, rps):
    """out = resid + ps gamma y (transformer_layer.py:70-88, the oracle's residual_scale) with y = z + bias; rows are sample-major."""
    B, N = 4, 16
    r = R.make_rows(family, B * rps, N, rps)
    dout, z, gamma, ps, bias = (t.double() for t in (r.dout, r.y, r.gamma, r.rowscale, r.mul))
    za, ga, ba = (t.clone().requires_grad_() for t in (z, gamma, bias))
    y = za + ba
    out = O.residual_scale(y.view(B, rps, N).transpose(0, 1), ga, torch.zeros(rps, B, N, dtype=torch.float64), ps).transpose(0, 1).reshape(B * rps, N)
    (out * dout).sum().backward()
    ref = R.resid_bwd_ref(dout, y.detach(), gamma, ps, rps, dgamma=True, dbias=True)
    close(ref["dbranch"][0], za.grad, "dbranch")
    close(ref["dgamma"][0], ga.grad, "dgamma")
    close(ref["dbias"][0], ba.grad, "dbias")
    close(R.scale_rows_ref(dout, gamma, ps, rps)[0], za.grad, "scale_rows")
    # the g0 route: dbranch without gamma, dgamma = sum_s rowdot + bias g0 with rowdot the row dots of the un-gamma-scaled gradient and z
    g0 = R.resid_bwd_ref(dout, None, gamma, ps, rps, dbias=True, g0=True)
    close(g0["dbranch"][0] * gamma, za.grad, "dbranch (g0 route) times gamma")
    close(g0["dbias"][0], ba.grad, "dbias (g0 route)")
    rowdot = (g0["dbranch"][0] * z).view(B, rps, N).sum(1)
    close(R.gamma_grad_finish_ref(rowdot, [(bias, g0["g0"][0])])[0], ga.grad, "gamma_grad_finish")
    close(R.colsum_ref(dout, y.detach(), ps, rps)[0], ga.grad, "colsum(x, y, rowscale)")
    close(R.colsum_ref(dout, None, ps, rps, mul=gamma)[0], ba.grad, "colsum(x, rowscale, mul)")
    segs = R.colsum_segments_ref(dout, 2, N // 2)
    close(torch.cat([s[0] for s in segs]), dout.sum(0), "colsum_segments")


def test_geglu_closed_form_against_autograd():
    dg, h0, h1 = (t.double() for t in R.make_geglu("nonfinite", 8 * 40))
    dg = torch.nan_to_num(dg, nan=0.5, posinf=2.0)
    a, b = h0.clone().requires_grad_(), h1.clone().requires_grad_()
    (O.gelu_erf(a) * b * dg).sum().backward()
    (r0, _), (r1, _) = R.geglu_bwd_ref(dg, h0, h1)
    close(r0, a.grad, "dh0")
    close(r1, b.grad, "dh1")


# ---- 2. the emulations inside the budget; 3. the mutants outside it -----------------------------------------------------------
def colsum_fails(case, mutant=None, combos=None):
    """(failures, largest share) of emulate_colsum over the case's combinations."""
    r = R.make_rows(case.family, case.M, case.N, case.rps)
    fails, share = [], 0.0
    for combo in combos or case.combos():
        kw, dt = R.colsum_kwargs(r, combo), (F32 if combo[3] else BF)
        exact, E = R.colsum_ref(r.dout.double(), budget=case.family != "integer", **R.to64(kw))
        got = R.emulate_colsum(r.dout, dtype=dt, mutant=mutant, **kw)
        f, s, _ = R.gate(got, exact, E, rd(dt), "%s[%s] out" % (case.id, R.combo_name(combo)))
        fails, share = fails + f, max(share, s)
    return fails, share


def resid_fails(case, mutant=None, combos=None):
    r = R.make_rows(case.family, case.M, case.N, case.rps)
    fails, share = [], 0.0
    for combo in combos or case.combos():
        dout, kw = R.resid_kwargs(r, combo)
        ref = R.resid_bwd_ref(dout.double(), budget=case.family != "integer", **R.to64(kw))
        got = R.emulate_resid_bwd(dout, mutant=mutant, **kw)
        assert set(ref) == set(got)
        for k, (exact, E) in ref.items():
            f, s, _ = R.gate(got[k], exact, E, "f32" if k == "g0" else "bf16", "%s[%s] %s" % (case.id, R.combo_name(combo), k))
            fails, share = fails + f, max(share, s)
    return fails, share


def finish_fails(case, mutant=None):
    slots, N, npairs, family = case
    rowdot, pairs, base = R.make_finish(family, slots, N)
    pairs = [(None if (i == 1 and npairs == 3) else b, g) for i, (b, g) in enumerate(pairs[:npairs])]
    fails, share = [], 0.0
    for acc in (False, True):
        exact, E = R.gamma_grad_finish_ref(rowdot.double(), R.to64(pairs), base.double() if acc else None, budget=family != "integer")
        got = R.emulate_gamma_grad_finish(rowdot, pairs, base if acc else None, mutant)
        f, s, _ = R.gate(got, exact, E, "bf16", "finish-%dx%d-p%d-%s acc=%d" % (slots, N, npairs, family, acc))
        fails, share = fails + f, max(share, s)
    return fails, share


def scale_fails(case, mutant=None):
    M, N, family, ga, rs = case
    rps = R.scale_rps(M)
    r = R.make_rows(family, M, N, rps)
    kw = dict(gamma=r.gamma if ga else None, rowscale=r.rowscale if rs else None, rps=rps)
    exact, E = R.scale_rows_ref(r.dout.double(), budget=family != "integer", **R.to64(kw))
    return R.gate(R.emulate_scale_rows(r.dout, mutant=mutant, **kw), exact, E, "bf16", "scale_rows-%dx%d-%s" % (M, N, family))[:2]


def geglu_fails(case, mutant=None):
    numel, family = case
    dg, h0, h1 = R.make_geglu(family, numel)
    (r0, e0), (r1, e1) = R.geglu_bwd_ref(dg.double(), h0.double(), h1.double())
    g0, g1 = R.emulate_geglu_bwd(dg, h0, h1, mutant)
    f0, s0, _ = R.gate(g0, r0, e0, "bf16", "geglu-%d-%s dh0" % (numel, family))
    f1, s1, _ = R.gate(g1, r1, e1, "bf16", "geglu-%d-%s dh1" % (numel, family))
    return f0 + f1, max(s0, s1)


def segments_fails(case, mutant=None):
    n_seg, seg_cols, M, null, family = case
    r = R.make_rows(family, M, n_seg * seg_cols)
    fails, share = [], 0.0
    for acc in (False, True):
        bases = [r.base0[:seg_cols], r.base1[:seg_cols], r.mul[:seg_cols]][:n_seg] if acc else None
        ref = R.colsum_segments_ref(r.dout.double(), n_seg, seg_cols, R.to64(bases), budget=family != "integer")
        got = R.emulate_colsum_segments(r.dout, n_seg, seg_cols, bases, mutant)
        for i in range(n_seg):
            f, s, _ = R.gate(got[i], ref[i][0], ref[i][1], "bf16", "segments-%dx%dx%d-%s out%d acc=%d" % (M, n_seg, seg_cols, family, i, acc))
            fails, share = fails + f, max(share, s)
    return fails, share


def transpose_fails(shape, mutant=None):
    rows, cols = shape[:2]
    x, scale = R.make_transpose(rows, cols)
    fails = []
    for sc in (None, scale):
        got, ref = R.emulate_transpose(x, sc, mutant), R.transpose_ref(x, sc)
        if not torch.equal(got.view(torch.int16), ref.view(torch.int16)):
            fails.append("transpose-%dx%d scale=%d" % (rows, cols, sc is not None))
    return fails, 0.0


RUNNERS = {"colsum": (colsum_fails, R.COLSUM_CASES), "resid_bwd": (resid_fails, R.RESID_CASES), "gamma_grad_finish": (finish_fails, R.FINISH_CASES),
           "scale_rows": (scale_fails, R.SCALE_CASES), "geglu_bwd": (geglu_fails, R.GEGLU_CASES), "segments": (segments_fails, R.SEGMENT_CASES),
           "transpose": (transpose_fails, R.TRANSPOSE_SHAPES)}


@pytest.mark.parametrize("op", sorted(RUNNERS))
def test_emulations_stay_inside_the_budget(op):
    run, cases = RUNNERS[op]
    worst = (0.0, None)
    for case in cases:
        fails, share = run(case)
        assert not fails, "\n".join(fails[:8])
        worst = max(worst, (share, getattr(case, "id", case)), key=lambda t: t[0])
    print("%s: largest share %.4f at %s over %d cases" % (op, worst[0], worst[1], len(cases)))
    assert worst[0] <= 1


def test_resid_combinations_all_launched():
    """The round-robin of RowsCase.combos reaches every combination that op_resid_bwd's argument checks admit, and does so past the clamp."""
    for cases, allc in ((R.RESID_CASES, R.RESID_COMBOS), (R.COLSUM_CASES, R.COLSUM_COMBOS)):
        assert {c for case in cases for c in case.combos()} == set(allc)
        big = {c for case in cases if case.M > 16384 for c in case.combos()}
        assert {c[2] for c in big} == {c[2] for c in allc} and {c[-1] for c in big} == {False, True}
    assert [c.id for c in R.RESID_PRODUCT[:len(R.RESID_CASES)]] == [c.id for c in R.RESID_CASES]      # (the GPU list begins with the CPU list)
    assert {c[4] for c in R.SEGMENT_CASES} == set(R.FAMILIES) and sum(c[3] is not None for c in R.SEGMENT_CASES) == 1
    shapes = {(M, N) for M in R.M_SMALL for N in R.N_SMALL} | {(M, N) for M in R.M_BIG for N in R.N_BIG}
    for cases in (R.RESID_PRODUCT, R.COLSUM_PRODUCT):     # the product, less `unit` past M = 257 and `nonfinite` below five rows
        have = {(c.M, c.N, c.family) for c in cases}
        assert have == {(M, N, f) for M, N in shapes for f in R.FAMILIES if not (f == "unit" and M > 257) and not (f == "nonfinite" and M < 5)}
        assert {c.rps for c in cases} >= {1, 3, 7, 64, 16384} and all(c.M % c.rps == 0 for c in cases)
    assert len(R.RESID_COMBOS) == 80 and all(not ("dgamma" in c[2] and "g0" in c[2]) for c in R.RESID_COMBOS)


# (mutants that only some combinations can show: the combination is given, so the search below stays short)
G, RS, T = True, True, True
MUTANT_COMBOS = {
    ("colsum", "rowscale_by_row"): [(False, RS, False, False, False)],
    ("colsum", "odd_tail_dropped"): [(False, False, False, False, False)],
    ("colsum", "base_after_rounding"): [(True, RS, True, False, True)],
    ("resid_bwd", "rowscale_by_row"): [(G, RS, ("dgamma", "dbias"), False, False)],
    ("resid_bwd", "pair_second_scale"): [(G, RS, ("dgamma", "dbias"), False, False)],
    ("resid_bwd", "base_after_rounding"): [(G, RS, ("dgamma", "dbias"), True, False)],
    ("resid_bwd", "gamma_missing_dbias"): [(G, RS, ("dbias",), False, False)],
    ("resid_bwd", "gamma_in_dbranch_g0"): [(G, RS, ("g0", "dbias"), False, False)],
    ("resid_bwd", "neg_entry_reads_row0"): [(G, RS, ("dgamma", "dbias"), False, T)],
    ("resid_bwd", "y_through_table"): [(G, RS, ("dgamma", "dbias"), False, T)],
}
ALL_MUTANTS = [(op, m) for op in sorted(R.MUTANTS) for m in R.MUTANTS[op]]


@pytest.mark.parametrize("op,mutant", ALL_MUTANTS, ids=["%s-%s" % t for t in ALL_MUTANTS])
def test_every_mutant_fails_the_gate(op, mutant):
    run, cases = RUNNERS[op]
    combos = MUTANT_COMBOS.get((op, mutant)) or ([(G, RS, ("dgamma", "dbias"), False, False)] if op == "resid_bwd" else
                                                   [(False, False, False, False, False), (True, RS, True, False, False)] if op == "colsum" else None)
    for case in cases:
        fails, _ = run(case, mutant, combos) if combos else run(case, mutant)
        if fails:
            print("%s / %s is caught by %s" % (op, mutant, fails[0]))
            return
    pytest.fail("no case of %s catches the mutant %s" % (op, mutant))


def test_segments_share_the_colsum_mutants():
    for mutant in ("odd_tail_dropped", "last_col_block_dropped", "partials_bf16", "base_after_rounding"):
        assert any(segments_fails(case, mutant)[0] for case in R.SEGMENT_CASES), mutant


# ---- 4. the mirror's numbers at the listed sizes ------------------------------------------------------------------------------
def test_mirror_numbers():
    want = {1: (1, 1), 3: (1, 1), 4: (1, 1), 5: (1, 2), 63: (1, 16), 64: (1, 16), 65: (2, 9), 257: (5, 13), 4100: (65, 16), 16384: (256, 16),
            16385: (256, 17), 16384 + 2 * 1024 + 5: (256, 19)}
    for M, (parts, rpw) in want.items():
        assert (R.cs_parts(M), R.cs_rows_per_wave(M)) == (parts, rpw), M
    # past the clamp both unrolled loops take full trips and an odd tail: 17 = 4 * 4 + 1 = 2 * 8 + 1, 19 = 4 * 4 + 3 = 2 * 9 + 1
    assert all(R.cs_rows_per_wave(M) % 2 == 1 and R.cs_rows_per_wave(M) % 4 != 0 and R.cs_rows_per_wave(M) > 4 for M in R.M_BIG[1:])
    assert R.cs_depth(16385) == 17 + 3 + 32 + 8
    assert R.ew_grid(4194304 // 8) == 2048 and [R.ew_trips(n // 8) for n in R.GEGLU_NUMEL] == [1, 1, 1, 2]
    assert [R.ew_trips(M * (N // 8)) for M, N in R.SCALE_SHAPES] == [1, 1, 1, 2, 2] and 2730 * 192 <= 2048 * 256 < 2731 * 192
    # the slot loop: which counts take unrolled trips, a tail, or both
    shape = {s: (max(len(a[1]) for a, _ in R.finish_chains(s)), max(len(t) for _, t in R.finish_chains(s))) for s in R.FINISH_SLOTS}
    assert shape == {1: (0, 1), 3: (0, 1), 4: (0, 1), 5: (0, 2), 12: (0, 3), 13: (1, 3), 16: (1, 0), 17: (1, 1), 29: (2, 3), 144: (9, 0)}
    for s in R.FINISH_SLOTS:     # every slot is added exactly once
        assert sorted(x for a, _ in R.finish_chains(s) for c in a for x in c) == list(range(s))
    assert R.finish_depth(144) == 9 + 4 and R.finish_depth(1) == 1 + 4
    assert any(N % 512 and N > 512 for N in R.N_SMALL) and all(n in R.neg_entries(16385) for n in (0, 1023, 1024, 16384))


# ---- 5. the condition: the fp32 allowance is a quarter of the bf16 rounding ---------------------------------------------------
def test_allowance_is_a_quarter_of_the_rounding_on_unit():
    worst = (0.0, None)

    def ratio(exact, E, what):
        nonlocal worst
        Rr = R.half_ulp_bf16(exact.abs() + E)
        m = float((E / Rr).flatten().median())
        worst = max(worst, (m, what), key=lambda t: t[0])
        assert m <= 0.25, "%s: median E / R = %.3f" % (what, m)
    for case in R.COLSUM_CASES:
        if case.family == "unit":
            r = R.make_rows("unit", case.M, case.N, case.rps)
            for combo in R.COLSUM_COMBOS:
                if not combo[3]:
                    ratio(*R.colsum_ref(r.dout.double(), **R.to64(R.colsum_kwargs(r, combo))), "%s[%s]" % (case.id, R.combo_name(combo)))
    for case in R.RESID_CASES:
        if case.family == "unit":
            r = R.make_rows("unit", case.M, case.N, case.rps)
            for combo in R.RESID_COMBOS:
                dout, kw = R.resid_kwargs(r, combo)
                for k, (exact, E) in R.resid_bwd_ref(dout.double(), **R.to64(kw)).items():
                    if k != "g0":
                        ratio(exact, E, "%s[%s] %s" % (case.id, R.combo_name(combo), k))
    for slots, N, npairs, family in R.FINISH_CASES:
        if family == "unit":
            rowdot, pairs, base = R.make_finish(family, slots, N)
            ratio(*R.gamma_grad_finish_ref(rowdot.double(), R.to64(pairs[:npairs]), base.double()), "finish-%dx%d" % (slots, N))
    dg, h0, h1 = (t.double() for t in R.make_geglu("nonfinite", 8 * 257))
    ok = torch.isfinite(dg)
    for (exact, E), what in zip(R.geglu_bwd_ref(dg[ok], h0[ok], h1[ok]), ("geglu dh0", "geglu dh1")):
        ratio(exact, E, what)
    print("largest median E / R on `unit`: %.4f at %s" % worst)
