"""tests/ln_ref.py checked without a GPU: the closed forms against fp64 autograd through the oracle's formulas, the fp32 re-statement
of every kernel inside every budget (the largest share is printed), every mutant of the computation failing a gate on the family
meant to catch it, and the coverage the case lists claim, proved from the route mirror."""
import pytest
import torch

from oracle import onepeace_oracle as O
from tests import ln_ref as L

BF, F32 = L.BF, L.F32
SMALL = {(1, 1): 72, (2, 1): 520, (3, 1): 1096, (4, 1): 1544, (2, 4): 2056, (3, 4): 4104, (4, 4): 6152}   # one cols per (CH, NW) class


def d(t):
    return None if t is None else t.double()


def operands(family, rows, cols, dtype=BF, seed=0, wide=False, dyfam="normal"):
    x = L.make_x(family, rows, cols, dtype, seed)
    w, b = L.make_wb(family, cols, dtype, seed, wide)
    return x, w, b, L.make_dy(dyfam, rows, cols, dtype, seed)


def close(a, b, what):
    err = float((a - b).abs().max())
    ref = float(b.abs().max())
    assert err <= 1e-12 * max(ref, 1e-300) or err == 0, "%s: %.3e against max %.3e" % (what, err, ref)


# ---- 1. closed forms against autograd ---------------------------------------------------------------------------------
@pytest.mark.parametrize("family", L.FAMILIES)
@pytest.mark.parametrize("gelu", [False, True])
def test_closed_forms_against_autograd(family, gelu):
    rows, cols = 7, 40
    x, w, b, dy = (d(t) for t in operands(family, rows, cols))
    add = d(L.make_x("normal", rows, cols, BF, 5))
    eps = 1e-5
    xa, wa, ba = (t.clone().requires_grad_() for t in (x, w, b))
    t = O.layer_norm(xa, wa, ba, eps)
    ya = O.gelu_erf(t) if gelu else t
    y, mean, rstd = L.ln_fwd_ref(x, w, b, eps, gelu)
    close(y, ya.detach(), "y")
    close(mean, x.mean(1), "mean")
    close(rstd, (x.var(1, unbiased=False) + eps).rsqrt(), "rstd")
    gx, gw_, gb = torch.autograd.grad(ya, (xa, wa, ba), dy)
    dx, dw, db = L.ln_bwd_ref(dy, x, w, b, mean, rstd, gelu, add=add)
    # (relative to the largest of the terms that cancel in dx, rstd |dy w|: the sums of the `offset` family are large against their result)
    scale = float((rstd[:, None] * (dy * w).abs()).max())
    assert float((dx - (gx + add)).abs().max()) <= 1e-12 * max(scale, float(dx.abs().max()))
    close(dw, gw_, "dw")
    close(db, gb, "db")
    base = (d(L.make_wb("normal", cols, BF, 9)[0]), d(L.make_wb("normal", cols, BF, 9)[1]))
    _, dw2, db2 = L.ln_bwd_ref(dy, x, w, b, mean, rstd, gelu, base=base)
    close(dw2, gw_ + base[0], "dw + base")
    close(db2, gb + base[1], "db + base")


def test_closed_forms_row_table():
    rows, total, cols = 9, 14, 24
    X, w, b, dy = (d(t) for t in operands("normal", total, cols))
    dy = dy[:rows]
    add = d(L.make_x("normal", total, cols, BF, 5))
    tab = L.make_row_table(rows, total)
    assert bool((tab < 0).any()) and bool((tab >= 0).any())
    xg = L.gather_rows(X, tab)
    assert bool((xg[tab < 0] == 0).all())
    y, mean, rstd = L.ln_fwd_ref(X, w, b, 1e-5, False, x_rows=tab)
    y2, _, _ = L.ln_fwd_ref(xg, w, b, 1e-5, False)
    assert torch.equal(y, y2)
    assert torch.equal(y[tab < 0], b.expand(int((tab < 0).sum()), cols))
    dx, dw, db = L.ln_bwd_ref(dy, X, w, b, mean, rstd, False, add=add, x_rows=tab)
    dxp, dwp, dbp = L.ln_bwd_ref(dy, xg, w, b, mean, rstd, False, add=L.gather_rows(add, tab))
    assert torch.equal(dx, dxp) and torch.equal(dw, dwp) and torch.equal(db, dbp)
    full = L.scatter_rows(add, dx, tab)
    named = torch.zeros(total, dtype=torch.bool)
    named[tab[tab >= 0].long()] = True
    assert torch.equal(full[~named], add[~named]) and torch.equal(full[tab[tab >= 0].long()], dx[tab >= 0])


@pytest.mark.parametrize("family", L.FAMILIES)
def test_geglu_closed_forms_against_autograd(family):
    rows, cols = 6, 32
    h0, h1 = (d(t) for t in L.make_h(family, rows, cols))
    w, b = (d(t) for t in L.make_wb(family, cols))
    dy = d(L.make_dy("normal", rows, cols))
    g, e_g0 = L.geglu_product(h0, h1)
    assert torch.equal(g, L.bf(O.gelu_erf(h0) * h1)) or float((g - L.bf(O.gelu_erf(h0) * h1)).abs().max()) <= float(e_g0.max())
    y, mean, rstd = L.ln_geglu_fwd_ref(h0, h1, w, b, 1e-5)
    close(y, O.layer_norm(g, w, b, 1e-5), "y")
    # backward: autograd through LayerNorm at the ROUNDED product, then through the unrounded GeGLU (what the kernel's formulas state)
    ga = g.clone().requires_grad_()
    wa = w.clone().requires_grad_()
    dg, dw_ = torch.autograd.grad(O.layer_norm(ga, wa, b, 1e-5), (ga, wa), dy)
    h0a, h1a = h0.clone().requires_grad_(), h1.clone().requires_grad_()
    g0, g1 = torch.autograd.grad(O.gelu_erf(h0a) * h1a, (h0a, h1a), dg)
    dh0, dh1, dw, db = L.ln_geglu_bwd_ref(dy, h0, h1, w, mean, rstd)
    scale = float((rstd[:, None] * (dy * w).abs()).max())      # (the largest of the terms that cancel in dg)
    assert float((dh0 - g0).abs().max()) <= 1e-12 * scale * max(1.0, float((h1 * L.gelu_erf_grad(h0)).abs().max()))
    assert float((dh1 - g1).abs().max()) <= 1e-12 * scale * max(1.0, float(h0.abs().max()))
    close(dw, dw_, "dw")
    close(db, dy.sum(0), "db")


# ---- 2. the fp32 re-statement inside every budget ------------------------------------------------------------------
def ln_shares(family, rows, cols, dtype, gelu, mutant=None, wide=False, dyfam="normal", eps=1e-5, table=False, accumulate=False):
    """Gate the emulation (or a mutant of it) of one forward + backward; returns (failures, {output: share})."""
    total = rows + 5 if table else rows
    x, w, b, dy = operands(family, total, cols, dtype, wide=wide, dyfam=dyfam)
    dy = dy[:rows]
    tab = L.make_row_table(rows, total) if table else None
    add = L.make_x("normal", total, cols, dtype, 5)
    base = tuple(L._store(0.5 * t, dtype) for t in L.make_wb("normal", cols, dtype, 9)) if accumulate else None
    rnd = "bf16" if dtype == BF else "f32"
    fails, sh = [], {}

    def gate(got, exact, E, rounding, what):
        f, s, _ = L.gate(got, exact, E, rounding, what)
        fails.extend(f)
        sh[what] = s

    y, mean, rstd = L.emulate_ln_fwd(x, w, b, eps, gelu, dtype, x_rows=tab, mutant=mutant)
    ye, me, re_ = L.ln_fwd_ref(d(x), d(w), d(b), eps, gelu, x_rows=tab)
    e_y, e_m, e_r = L.fwd_budget(d(x), d(w), d(b), eps, gelu, x_rows=tab)
    gate(y, ye, e_y, rnd, "y")
    gate(mean, me, e_m, "f32", "mean")
    gate(rstd, re_, e_r, "f32", "rstd")
    # the backward takes the statistics of an UNMUTATED forward (every gate looks at one kernel)
    _, mean, rstd = L.emulate_ln_fwd(x, w, b, eps, gelu, dtype, x_rows=tab)
    dx, dw, db = L.emulate_ln_bwd(dy, x, w, b, mean, rstd, gelu, dtype, add=add, x_rows=tab, dx_full=add, base=base, mutant=mutant)
    args = (d(dy), d(x), d(w), d(b), d(mean), d(rstd), gelu)
    kw = dict(add=d(add), x_rows=tab, base=None if base is None else (d(base[0]), d(base[1])))
    dxe, dwe, dbe = L.ln_bwd_ref(*args, **kw)
    e_dx, e_dw, e_db, _ = L.bwd_budget("bwd", *args, out_dtype=dtype, **kw)
    if tab is not None:      # rows no entry names keep `add`; the rows of dropped entries are not gated (nothing is stored)
        keep = tab >= 0
        full = L.scatter_rows(d(add), dxe, tab)
        E = L.scatter_rows(torch.zeros_like(full), torch.where(keep[:, None], e_dx, torch.zeros_like(e_dx)), tab)
        gate(dx, full, E, rnd, "dx")
    else:
        gate(dx, dxe, e_dx, rnd, "dx")
    gate(dw, dwe, e_dw, rnd, "dw")
    gate(db, dbe, e_db, rnd, "db")
    return fails, sh


def geglu_shares(family, rows, cols, mutant=None, accumulate=False, dyfam="normal"):
    h0, h1 = L.make_h(family, rows, cols)
    w, b = L.make_wb(family, cols)
    dy = L.make_dy(dyfam, rows, cols)
    base = tuple(L._store(0.5 * t, BF) for t in L.make_wb("normal", cols, BF, 9)) if accumulate else None
    fails, sh = [], {}

    def gate(got, exact, E, rounding, what):
        f, s, _ = L.gate(got, exact, E, rounding, what)
        fails.extend(f)
        sh[what] = s

    y, mean, rstd = L.emulate_ln_geglu_fwd(h0, h1, w, b, 1e-5, mutant=mutant)
    ye, me, re_ = L.ln_geglu_fwd_ref(d(h0), d(h1), d(w), d(b), 1e-5)
    e_y, e_m, e_r = L.geglu_fwd_budget(d(h0), d(h1), d(w), d(b), 1e-5)
    gate(y, ye, e_y, "bf16", "y")
    gate(mean, me, e_m, "f32", "mean")
    gate(rstd, re_, e_r, "f32", "rstd")
    _, mean, rstd = L.emulate_ln_geglu_fwd(h0, h1, w, b, 1e-5)
    o0, o1, dw, db = L.emulate_ln_geglu_bwd(dy, h0, h1, w, mean, rstd, base=base, mutant=mutant)
    args = (d(dy), d(h0), d(h1), d(w), d(mean), d(rstd))
    bb = None if base is None else (d(base[0]), d(base[1]))
    r0, r1, dwe, dbe = L.ln_geglu_bwd_ref(*args, base=bb)
    e0, e1, e_dw, e_db = L.geglu_bwd_budget(*args, base=bb)
    gate(o0, r0, e0, "bf16", "dh0")
    gate(o1, r1, e1, "bf16", "dh1")
    gate(dw, dwe, e_dw, "bf16", "dw")
    gate(db, dbe, e_db, "bf16", "db")
    return fails, sh


@pytest.mark.parametrize("chnw", sorted(SMALL))
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "f32"])
def test_emulation_inside_budget_per_class(chnw, dtype):
    cols = SMALL[chnw]
    assert L.ch_nw(cols) == chnw
    for gelu in (False, True):
        fails, sh = ln_shares("normal", 11, cols, dtype, gelu, table=gelu, accumulate=not gelu)
        print("CH %d NW %d %s gelu %d largest shares %s" % (chnw + (dtype, gelu, {k: round(v, 3) for k, v in sh.items()})))
        assert not fails and max(sh.values()) < 1, fails
    if dtype == BF:
        fails, sh = geglu_shares("normal", 11, cols, accumulate=True)
        print("CH %d NW %d geglu largest shares %s" % (chnw + ({k: round(v, 3) for k, v in sh.items()},)))
        assert not fails and max(sh.values()) < 1, fails


@pytest.mark.parametrize("family", L.FAMILIES)
def test_emulation_inside_budget_per_family(family):
    for dtype in (BF, F32):
        for gelu, wide, dyfam in ((False, False, "rowscale"), (True, True, "normal")):
            fails, sh = ln_shares(family, 23, 264, dtype, gelu, wide=wide, dyfam=dyfam, eps=1e-6 if wide else 1e-5)
            print("%s %s gelu %d largest shares %s" % (family, dtype, gelu, {k: round(v, 3) for k, v in sh.items()}))
            assert not fails and max(sh.values()) < 1, fails
    fails, sh = geglu_shares(family, 23, 264, dyfam="rowscale")
    print("%s geglu largest shares %s" % (family, {k: round(v, 3) for k, v in sh.items()}))
    assert not fails and max(sh.values()) < 1, fails


# ---- 3. the mutants fail ---------------------------------------------------------------------------------------------
# (mutant, which emulation, family, dtype, the outputs of which at least one must miss its gate)
MUTANT_CASES = [
    ("var_one_pass", "ln", "offset", BF, ("rstd",)),
    ("var_one_pass", "ln", "offset", F32, ("rstd", "y")),
    ("var_unbiased", "ln", "normal", BF, ("rstd",)),
    ("var_unbiased", "geglu", "normal", BF, ("rstd",)),
    ("eps_outside_root", "ln", "tiny", BF, ("rstd", "y")),
    ("eps_outside_root", "ln", "constant", BF, ("rstd",)),
    ("dx_without_c2", "ln", "normal", BF, ("dx",)),
    ("dx_without_c2", "geglu", "normal", BF, ("dh0", "dh1")),
    ("dx_without_w", "ln", "normal", BF, ("dx",)),
    ("dx_without_w", "geglu", "normal", BF, ("dh0",)),
    ("tanh_gelu", "ln_gelu", "gelu_tails", BF, ("y",)),
    ("tanh_gelu", "ln_gelu", "gelu_tails", F32, ("y", "dx")),
    ("tanh_gelu", "geglu", "gelu_tails", BF, ("mean", "dh1")),
    ("stats_of_unrounded_product", "geglu", "normal", BF, ("mean",)),
    ("chunk_unwritten", "ln", "normal", BF, ("y",)),
    ("chunk_unwritten", "ln", "outlier", BF, ("dx",)),
    ("chunk_unwritten", "geglu", "normal", BF, ("y", "dh0")),
    ("stale_prefetch", "ln", "normal", BF, ("y",)),
    ("stale_prefetch", "ln", "rowscale", BF, ("mean", "dx")),
    ("stale_prefetch", "geglu", "normal", BF, ("y", "dh0")),
    ("add_on_unmapped_row", "ln_table", "normal", BF, ("dx",)),
    ("accumulate_ignored", "ln_acc", "normal", BF, ("dw", "db")),
    ("accumulate_ignored", "geglu_acc", "normal", BF, ("dw", "db")),
]


def test_every_mutant_listed():
    assert {m[0] for m in MUTANT_CASES} == set(L.MUTANTS)


@pytest.mark.parametrize("mutant,which,family,dtype,outputs", MUTANT_CASES, ids=["%s-%s-%s-%s" % (m[0], m[1], m[2], "bf16" if m[3] == BF else "f32") for m in MUTANT_CASES])
def test_mutant_fails(mutant, which, family, dtype, outputs):
    rows, cols = 23, 264
    if which.startswith("geglu"):
        run = lambda m: geglu_shares(family, rows, cols, mutant=m, accumulate=which.endswith("acc"))  # noqa: E731
    else:
        run = lambda m: ln_shares(family, rows, cols, dtype, which == "ln_gelu", mutant=m, table=which == "ln_table", accumulate=which == "ln_acc")  # noqa: E731
    fails, sh = run(None)
    assert not fails and max(sh.values()) < 1, fails      # the unmutated emulation passes the same gates on the same inputs
    fails, sh = run(mutant)
    for o in outputs:
        assert sh[o] > 1, "%s passes the %s gate on %s (share %.3f)" % (mutant, o, family, sh[o])
    print("%s on %s: %s" % (mutant, family, "; ".join(fails)[:400]))


# ---- 4. coverage of the case lists, from the route mirror ---------------------------------------------------------
def test_route_mirror():
    assert L.route("fwd", 4101, 72) == (1, 1, False, 3, False)
    assert L.route("bwd", 1029, 8192, F32) == (4, 4, False, 3, False)
    assert L.route("fwd", 2049, 64) == (1, 1, False, 2, False)    # 513 workgroups capped to 512: 2048 row groups, one takes a second row
    assert L.route("fwd", 5, 1544) == (4, 1, False, 1, True)
    assert L.route("geglu_fwd", 8197, 2048) == (4, 1, True, 2, False)
    # (under the forward's cap of 2048 workgroups the listed 8197 / 2053 rows take two trips; 16389 / 4101 rows take three)
    assert L.route("geglu_fwd", 2053, 6144)[3] == 2 and L.route("geglu_fwd", 16389, 2048)[3] == 3 and L.route("geglu_fwd", 4101, 8192)[3] == 3
    assert L.route("geglu_bwd", 4101, 520) == (2, 1, True, 3, False)
    assert L.route("fwd", 16384, 2048) == (4, 1, True, 8, False) and L.route("fwd", 16383, 2048)[2] is False
    assert L.route("fwd", 16384, 2048, stats=False)[2] is False and L.route("fwd_q8", 16384, 2048)[2] is False
    assert L.route("bwd", 4096, 8192)[:3] == (4, 4, True) and L.route("bwd", 4095, 8192)[2] is False
    assert L.route("bwd", 2048, 8192, F32)[:3] == (4, 4, True) and L.route("bwd", 2047, 8192, F32)[2] is False
    assert L.wgrad_depth("bwd", 4101, 72) == 3 + 3 + 64 + 8 and L.wgrad_depth("bwd", 1029, 4104) == 3 + 64 + 8


def test_case_lists_cover_every_route():
    classes = sorted(SMALL)
    seen = {}
    for c in L.CASES:
        for kind in c.kinds():
            CH, NW, nt, trips, idle = L.route(kind, c.rows, c.cols, c.dtype)
            seen.setdefault((kind, CH, NW), []).append((trips, idle, c))
    for kind in ("fwd", "bwd", "geglu_fwd", "geglu_bwd"):
        for CH, NW in classes:
            got = seen.get((kind, CH, NW), [])
            trips = {t for t, _, _ in got}
            assert 1 in trips, (kind, CH, NW, "one trip")
            assert max(trips) >= 3, (kind, CH, NW, trips)
        assert any(t >= 3 for (k, _, nw), v in seen.items() if k == kind and nw == 1 for t, _, _ in v)
        assert any(t >= 3 for (k, _, nw), v in seen.items() if k == kind and nw == 4 for t, _, _ in v)
        assert any(idle for (k, _, _), v in seen.items() if k == kind for _, idle, _ in v), (kind, "idle row group")
        assert any(c.cols % (64 * nw * 8) != 0 and c.cols > 64 * nw * 8 for (k, _, nw), v in seen.items() if k == kind for _, _, c in v), (kind, "ragged last chunk")
    for kind in ("fwd", "bwd"):
        for nw in (1, 4):
            assert any(c.dtype == F32 for (k, _, n), v in seen.items() if k == kind and n == nw for _, _, c in v)
            fam = {c.family for (k, _, n), v in seen.items() if k == kind and n == nw for _, _, c in v}
            assert fam == set(L.FAMILIES), (kind, nw, set(L.FAMILIES) - fam)
    # both cache policies: the default one above, the non-temporal one in the three large cases
    for rows, cols, dtype in L.NT_CASES:
        assert L.route("fwd", rows, cols, dtype)[2] and L.route("bwd", rows, cols, dtype)[2]
        assert not L.route("fwd", rows - 1, cols, dtype)[2] and not L.route("bwd", rows - 1, cols, dtype)[2]
    assert not any(L.route(k, c.rows, c.cols, c.dtype)[2] for c in L.CASES if c.kind == "ln" for k in c.kinds())
    assert {c.dyfam for c in L.CASES} == {"normal", "rowscale"} and any(c.wide for c in L.CASES)


def test_issue_case_table():
    ids = {(c.kind, c.rows, c.cols, c.dtype, c.gelu) for c in L.CASES}
    for cols in L.A_COLS:
        assert ("ln", 4101, cols, BF, False) in ids and ("ln", 4101, cols, BF, True) in ids
        assert ("geglu_fwd", 8197, cols, BF, False) in ids and ("geglu_bwd", 4101, cols, BF, False) in ids
    for cols in L.B_COLS:
        assert ("ln", 1029, cols, BF, False) in ids and ("geglu_bwd", 1029, cols, BF, False) in ids
    for k in (("ln", 4101, 520, F32, False), ("ln", 4101, 2048, F32, False), ("ln", 1029, 2056, F32, False), ("ln", 1029, 6144, BF, True),
              ("geglu_fwd", 2053, 2056, BF, False), ("geglu_fwd", 2053, 6144, BF, False)):
        assert k in ids, k
    assert any(c.rows == 1029 and c.cols == 8192 and c.dtype == F32 for c in L.CASES)
    for rows in (1, 3, 5, 2049):
        for cols in (8, 64, 1544):
            assert any(c.kind == "ln" and c.rows == rows and c.cols == cols for c in L.CASES)
    assert any(not c.halves for c in L.by_group("D", "geglu_fwd")) and any(not c.halves for c in L.by_group("D", "geglu_bwd"))


def test_no_case_above_36m_elements():
    assert max(c.elements() for c in L.CASES) <= 36_000_000
    assert max(r * c for r, c, _ in L.NT_CASES) <= 36_000_000
