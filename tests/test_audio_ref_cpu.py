"""tests/audio_ref.py on the CPU: the fp64 re-statement of the kernel's fp32 convolution chain is sound, the `exact` family needs no chain,
the near-midpoint allowance of the rounded dx is rare (condition 1) and a single missing row lies far above the dW0 gate (condition 2),
the fp32 re-statement of both kernels passes the gate in every family and each of its mutants fails it, the mirror of a_grid gives the
hand-computed values, and the case list has no duplicates and covers what it claims."""
import os

import pytest
import torch

from tests import audio_ref as A
from tests import ln_ref

EPS = A.EPS


def fwd64(r, chain=True):
    return A.fwd_ref(A.to64(r.wav), A.to64(r.w0), A.to64(r.b0), A.to64(r.lnw), A.to64(r.lnb), r.rows, r.stride, EPS, chain=chain)


def bwd64(r, f, accumulate=False):
    mean, rstd = f["mean"].float(), f["rstd"].float()     # the reference's statistics as the fp32 numbers the kernel is given
    ref = A.bwd_ref(A.to64(r.dy), f["S"], f["v"], A.to64(r.lnw), A.to64(r.lnb), mean.double(), rstd.double(), r.b0 is not None,
                    A.to64(r.base) if accumulate else None)
    return mean, rstd, ref


def gate_fwd(got, f):
    y, mean, rstd = got
    fails, shares = [], {}
    assert torch.equal(torch.isfinite(f["y"]).all(1), ~A.touched_rows(f["S"])) and torch.equal(torch.isfinite(f["y"]).any(1), ~A.touched_rows(f["S"]))
    for k, g, kind in (("y", y, "bf16"), ("mean", mean, "f32"), ("rstd", rstd, "f32")):
        fl, s, _ = A.gate(g, f[k], f["E_" + k], kind, k)
        fails, shares[k] = fails + fl, s
        if not torch.equal(torch.isfinite(g.double()), torch.isfinite(f[k])):
            fails.append("%s: finite where the reference is not, or the reverse" % k)
    return fails, shares


def gate_bwd(got, ref):
    fails, shares = [], {}
    for k, g in got.items():
        exact, E = ref[k]
        fl, s, _ = A.gate(g, exact, E, "bf16", k)
        fails, shares[k] = fails + fl, s
        if not torch.equal(torch.isfinite(g.double()), torch.isfinite(exact)):
            fails.append("%s: finite where the reference is not, or the reverse" % k)
    return fails, shares


# ---- the chain -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,bias", [(64, True), (512, False), (512, True)])
def test_chain_is_sound(C, bias):
    r = A.make_inputs("unit", 2000, C, 5, bias)
    S, w0, b0 = A.patches(A.to64(r.wav), r.rows, 5), A.to64(r.w0), A.to64(r.b0)
    chain = A.conv_chain(S, w0, b0)
    exact, e_a = A.conv_exact(S, w0, b0)
    assert torch.equal(chain, chain.float().double())
    assert bool(((chain - exact).abs() <= e_a).all()), float(((chain - exact).abs() / e_a).max())
    far = (A.half_ulp_bf16(exact) - (exact - A.bf(exact)).abs()) > e_a
    assert bool((A.bf(chain) == A.bf(exact))[far].all())
    assert float((~far).double().mean()) < 1e-2 and float((A.bf(chain) != A.bf(exact)).double().mean()) < 1e-4     # (a few in a million differ)
    # the fp64 re-statement IS the fp32 fused multiply-add: against an exact rational evaluation of one step on awkward operands
    from fractions import Fraction
    g = torch.Generator().manual_seed(5)
    a = torch.randn(4000, generator=g).float() * torch.ldexp(torch.ones(4000), torch.randint(-40, 41, (4000,), generator=g))
    w, s = (A._b(torch.randn(4000, generator=g)) for _ in range(2))
    step = (a.double() + w.double() * s.double()).float()
    for i in range(0, 4000, 7):
        t = Fraction(float(a[i])) + Fraction(float(w[i])) * Fraction(float(s[i]))
        lo = torch.nextafter(step[i], torch.tensor(-float("inf"))).item()
        hi = torch.nextafter(step[i], torch.tensor(float("inf"))).item()
        d = abs(Fraction(float(step[i])) - t)
        assert d <= abs(Fraction(lo) - t) and d <= abs(Fraction(hi) - t), i


@pytest.mark.parametrize("C,stride", [(8, 5), (64, 1), (512, 16)])
def test_exact_family_needs_no_chain(C, stride):
    r = A.make_inputs("exact", 300, C, stride, True)
    S, w0, b0 = A.patches(A.to64(r.wav), r.rows, stride), A.to64(r.w0), A.to64(r.b0)
    exact, _ = A.conv_exact(S, w0, b0)
    assert torch.equal(A.conv_chain(S, w0, b0), exact) and torch.equal(A.bf(exact), exact)
    f = fwd64(r, chain=False)
    y, mean, rstd = A.emulate_conv1_fwd(r, EPS)
    assert torch.equal(mean.double(), f["mean"]), "the mean of the exact family is exact at a power-of-two C"
    assert not gate_fwd((y, mean, rstd), f)[0]


# ---- the two conditions ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", [f for f in A.FAMILIES if f != "nonfinite"])
@pytest.mark.parametrize("C", [64, 264, 512])
def test_condition_1_few_elements_near_a_midpoint(family, C):
    r = A.make_inputs(family, 1030, C, 5, C != 264)
    _, _, ref = bwd64(r, fwd64(r))
    share = float((ref["dx"][3] != 0).double().mean())
    print("E_q != 0 on %.2f %% of dx (%s, C = %d)" % (100 * share, family, C))
    assert share <= 0.05


@pytest.mark.parametrize("rows,C", [(8195, 64), (1030, 512)])
def test_condition_2_one_missing_row_is_far_above_the_gate(rows, C):
    r = A.make_inputs("unit", rows, C, 5, True)
    f = fwd64(r)
    _, _, ref = bwd64(r, f)
    med = float(A.single_row_ratio(ref, f["S"]).median())
    print("median (largest single-row term) / (R + E) of dW0 at %d x %d: %.1f" % (rows, C, med))
    assert med >= 8


# ---- the emulation passes, every mutant fails --------------------------------------------------------------------------------
@pytest.mark.parametrize("family", A.FAMILIES)
@pytest.mark.parametrize("rows,C,stride,bias,affine", [(4100, 64, 5, True, "both"), (1030, 264, 5, False, "lnb_null"), (37, 8, 5, True, "none"),
                                                       (700, 512, 5, False, "dlnb_null")])
def test_emulation_passes_the_gate(family, rows, C, stride, bias, affine):
    r = A.make_inputs(family, rows, C, stride, bias, affine)
    f = fwd64(r, chain=family != "exact")
    fails, shares = gate_fwd(A.emulate_conv1_fwd(r, EPS), f)
    assert not fails, fails[:4]
    for acc in (False, True):
        mean, rstd, ref = bwd64(r, f, acc)
        got = A.emulate_conv1_bwd(r, mean, rstd, acc)
        assert set(got) == set(A.wanted(bias, affine))
        fails, shares = gate_bwd(got, ref)
        assert not fails, fails[:4]
    if family == "silence" and not bias:
        sil = A.silent_rows(f["S"])
        assert int(sil.sum()) > 0 and bool((f["v"][sil] == 0).all())
        want = A.bf(A.gelu_erf(torch.zeros(C, dtype=torch.float64) if r.lnb is None else A.to64(r.lnb)))
        assert torch.equal(A.emulate_conv1_fwd(r, EPS)[0][sil].double(), want.expand(int(sil.sum()), C))
    if family == "nonfinite":
        assert int(A.touched_rows(f["S"]).sum()) == 4     # each of the two samples touches exactly two rows at stride 5


@pytest.mark.parametrize("mutant", sorted(A.MUTANTS))
def test_every_mutant_fails_the_gate(mutant):
    kinds, family, rows, C = A.MUTANTS[mutant]
    r = A.make_inputs(family, rows, C, 5, True, "both")
    f = fwd64(r, chain=family != "exact")
    caught = {}
    if "fwd" in kinds:
        assert not gate_fwd(A.emulate_conv1_fwd(r, EPS), f)[0]
        caught["fwd"] = bool(gate_fwd(A.emulate_conv1_fwd(r, EPS, mutant), f)[0])
    if "bwd" in kinds:
        mean, rstd, ref = bwd64(r, f, True)
        assert not gate_bwd(A.emulate_conv1_bwd(r, mean, rstd, True), ref)[0]
        caught["bwd"] = bool(gate_bwd(A.emulate_conv1_bwd(r, mean, rstd, True, mutant), ref)[0])
    assert all(caught.values()), (mutant, caught)


# ---- the mirror and the case list ------------------------------------------------------------------------------------------
def test_mirror_of_a_grid_by_hand():
    # rows: (grid, trips, Dw = trips + 3 + ceil(grid / 8) + 8)
    for rows, want in {1: (1, 1, 13), 3: (1, 1, 13), 4: (1, 1, 13), 5: (2, 1, 13), 4096: (1024, 1, 140), 4097: (1024, 2, 141),
                       8192: (1024, 2, 141), 8195: (1024, 3, 142), 2496: (624, 1, 90), 2048000: (1024, 500, 639)}.items():
        assert (A.a_grid(rows), A.trips(rows), A.wgrad_depth(rows)) == want, rows
    assert A.wav_len(1, 5) == 10 and A.wav_len(832, 5) == 4165 and A.wav_len(3, 16) == 42
    assert ln_ref.depth(8) == ln_ref.depth(512) == 15


def test_case_list():
    ids = [c.id for c in A.CASES]
    assert len(set(ids)) == len(ids) and 100 <= len(ids) <= 400
    plain = [c for c in A.CASES if not c.chained]
    assert {c.rows for c in plain} == set(A.ROWS) and {c.C for c in plain} == set(A.CS)
    assert {(c.rows, c.C) for c in plain} == {(r, c) for r in A.ROWS for c in A.CS}
    for fam in A.FAMILIES:
        mine = [c for c in plain if c.family == fam]
        assert {c.C for c in mine} == set(A.CS), fam
        assert {c.rows for c in mine} >= {5, 4096, 4097, 8195}, fam
        assert {c.accumulate for c in mine} == {0, 1} and {c.bias for c in mine} == {False, True}, fam
        assert {c.affine for c in mine} == set(A.AFFINE), fam
        assert [c for c in A.CASES if c.chained and c.family == fam], fam
    assert {c.stride for c in plain} == set(A.STRIDES)
    assert len({(c.bias, c.affine, c.accumulate) for c in plain}) == 16
    assert len({(c.bias, c.affine, c.accumulate) for c in plain if c.rows == 8195}) >= 8     # (also where the row loop takes three trips)
    assert all(c.stride == 5 and c.rows >= 5 for c in A.CASES if c.family == "nonfinite")
    assert max(c.rows * c.C for c in A.CASES) == 8195 * 512
    for c in plain:     # the trips the row list is there for
        assert A.trips(c.rows) == {1: 1, 3: 1, 5: 1, 4096: 1, 4097: 2, 8195: 3}[c.rows]


def test_record_matches_the_committed_file():
    """The maxima quoted in tests/audio_ref.py are those of profiles/audio_fp64_errors_mi355x.txt."""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "audio_fp64_errors_mi355x.txt")
    assert os.path.exists(path) and A.RECORD is not None
    best = {}
    lines = [ln for ln in open(path).read().splitlines() if ln.strip()]
    for ln in lines:
        for tok in ln.split(" shares ")[1].split():
            if "=" not in tok:     # ("(bit for bit)": the wrapper and rows = 0 lines)
                continue
            k, v = tok.split("=")
            s, o = (float(x) for x in v.split("/"))
            best[k] = (max(best.get(k, (0, 0))[0], s), max(best.get(k, (0, 0))[1], o))
    assert all(s <= 1 for s, _ in best.values())
    assert {k: (round(s, 2), round(o, 2)) for k, (s, o) in best.items()} == A.RECORD
    assert {ln.split()[0] for ln in lines} >= {c.id for c in A.CASES}
