"""The LayerNorm kernels of csrc/layernorm.hip against fp64 on the SAME inputs, PER ELEMENT, on every route of the dispatch
(tests/ln_ref.py: closed forms, budget, families, route mirror, case lists; checked on the CPU by tests/test_ln_ref_cpu.py).

Every output lives in a guarded buffer (a sentinel bit pattern around it, checked after every launch), every input is compared bit
for bit with its host copy afterwards, and every gate is  |got - exact| <= R + E  with the derived E of tests/ln_ref.py: y, mean, rstd
of the forward (mean and rstd as the fp32 numbers they are), dx, dw, db of the backward -- which is handed the kernel's OWN forward
statistics, as is the reference.  The references are evaluated in fp64 on the device.  Each case appends one line to
ln_fp64_report.txt in the tests' output directory: its id, its route (CH, NW, nt, trips, idle) and per output the largest share of the
budget |err| / (R + E), followed after the slash by the largest (|err| - R) / E (the fp32 allowance used beyond the output's rounding)."""
import os

import pytest
import torch

from tests import ln_ref as L
from tests.gemm_ref import SENTINEL
from tests.util import out_dir

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = L.BF, L.F32


def hipmod():
    from one_peace_amd import hip
    return hip


def bits(t):
    return t.contiguous().view({BF: torch.int16, F32: torch.int32, torch.uint8: torch.uint8, torch.int32: torch.int32}[t.dtype])


def same(a, b):
    return torch.equal(bits(a), bits(b))


def D(t):
    return None if t is None else t.to(DEV).double()


class Run:
    """The guarded device tensors of one test, its failures and its largest shares."""
    reported = False      # the first case of a session starts ln_fp64_report.txt afresh: one line per case

    def __init__(self, cid, routes):
        self.cid, self.routes, self.fails, self.sh, self.over = cid, routes, [], {}, {}
        self.inputs, self.outputs = [], []

    def inp(self, host, dtype):
        """A guarded device copy of a host tensor (NaN sentinels around it); compared with the host copy at the end."""
        if host is None:
            return None
        host = host.to(dtype)
        v = L.guarded_from(host, dtype, device=DEV, ld_extra=0 if host.dim() == 2 else 8)
        self.inputs.append((v, host))
        return v

    def out(self, shape, dtype, fill=None):
        v = L.guarded(tuple(shape), dtype, ld_extra=0 if len(shape) == 2 else 8, device=DEV)
        if fill is not None:
            v.copy_(fill.to(DEV))
        self.outputs.append(v)
        return v

    def gate(self, got, exact, E, dtype, what, key=None):
        f, s, over = L.gate(got, exact, E, "bf16" if dtype == BF else "f32", what)
        self.fails += f
        key = key or what
        self.sh[key] = max(self.sh.get(key, 0.0), s)
        self.over[key] = max(self.over.get(key, 0.0), over)

    def require(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def finish(self):
        torch.cuda.synchronize()
        for v in self.outputs + [v for v, _ in self.inputs]:
            n = L.check_guard(v)
            self.require(n == 0, "%d guard elements overwritten around a %s buffer" % (n, tuple(v.shape)))
        for v, host in self.inputs:
            self.require(torch.equal(bits(v.cpu()), bits(host)), "an input of shape %s changed" % (tuple(v.shape),))
        line = "%s route %s shares %s" % (self.cid, self.routes, " ".join("%s=%.4f/%.3f" % (k, v, self.over[k]) for k, v in sorted(self.sh.items())))
        with open(os.path.join(out_dir(), "ln_fp64_report.txt"), "a" if Run.reported else "w") as f:   # (a fresh report per session)
            f.write(line + "\n")
        Run.reported = True
        print(line)
        assert not self.fails, "\n".join(self.fails[:12])
        assert all(s <= 1 for s in self.sh.values()), self.sh


# ---- launches through the C ABI, every output given by the caller -------------------------------------------------------
def fwd(x, w, b, y, mean, rstd, rows, eps, gelu, x_rows=None):
    hip = hipmod()
    hip._check(hip.lib().op_layernorm_fwd(hip.ptr(x), hip.ptr(w), hip.ptr(b), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), rows, x.shape[1], eps,
                                          int(gelu), hip._dt(x), hip.ptr(x_rows), hip.stream()), "op_layernorm_fwd")


def bwd(dy, x, w, b, mean, rstd, add, dx, dw, db, rows, gelu, accumulate=False, x_rows=None):
    hip = hipmod()
    cols = x.shape[1]
    ws = hip.workspace(hip.lib().op_layernorm_bwd_workspace_bytes(rows, cols), x.device, "ln") if dw is not None else None
    hip._check(hip.lib().op_layernorm_bwd(hip.ptr(dy), hip.ptr(x), hip.ptr(w), hip.ptr(b), hip.ptr(mean), hip.ptr(rstd), hip.ptr(add), hip.ptr(dx),
                                          hip.ptr(dw), hip.ptr(db), hip.ptr(ws), rows, cols, int(gelu), int(accumulate), hip._dt(x), hip.ptr(x_rows),
                                          hip.stream()), "op_layernorm_bwd")


def base_pair(cols, dtype):
    return tuple(L._store(0.5 * t, dtype) for t in L.make_wb("normal", cols, dtype, 9))


def routes_of(case):
    return " ".join("%s=%s" % (k, L.route(k, case.rows, case.cols, case.dtype)) for k in case.kinds())


LN_CASES = [c for c in L.CASES if c.kind == "ln"]


@pytest.mark.parametrize("case", LN_CASES, ids=[c.id for c in LN_CASES])
def test_ln_fwd_bwd(case):
    rows, cols, dt, gelu, eps = case.rows, case.cols, case.dtype, case.gelu, case.eps
    run = Run(case.id, routes_of(case))
    hx = L.make_x(case.family, rows, cols, dt)
    hw, hb = L.make_wb(case.family, cols, dt, wide=case.wide)
    hdy = L.make_dy(case.dyfam, rows, cols, dt)
    hadd = L.make_x("normal", rows, cols, dt, 5)
    x, w, b, dy, add = (run.inp(t, dt) for t in (hx, hw, hb, hdy, hadd))
    # ---- forward
    y, mean, rstd = run.out((rows, cols), dt), run.out((rows,), F32), run.out((rows,), F32)
    fwd(x, w, b, y, mean, rstd, rows, eps, gelu)
    ye, me, re_ = L.ln_fwd_ref(D(hx), D(hw), D(hb), eps, gelu)
    e_y, e_m, e_r = L.fwd_budget(D(hx), D(hw), D(hb), eps, gelu)
    run.gate(y, ye, e_y, dt, "y")
    run.gate(mean, me, e_m, F32, "mean")
    run.gate(rstd, re_, e_r, F32, "rstd")
    y2 = run.out((rows, cols), dt)
    fwd(x, w, b, y2, None, None, rows, eps, gelu)
    run.require(same(y, y2), "want_stats=False changes y")
    del ye, e_y, y2
    # ---- backward on the kernel's own statistics: out of place with `add`, fresh dw / db
    dx, dw, db = run.out((rows, cols), dt), run.out((cols,), dt), run.out((cols,), dt)
    bwd(dy, x, w, b, mean, rstd, add, dx, dw, db, rows, gelu)
    args = (D(hdy), D(hx), D(hw), D(hb), mean.double(), rstd.double(), gelu)
    dxe, dwe, dbe = L.ln_bwd_ref(*args, add=D(hadd))
    e_dx, e_dw, e_db, _ = L.bwd_budget("bwd", *args, add=D(hadd), out_dtype=dt)
    run.gate(dx, dxe, e_dx, dt, "dx")
    run.gate(dw, dwe, e_dw, dt, "dw")
    run.gate(db, dbe, e_db, dt, "db")
    del dxe, e_dx
    # ---- the same launch again: dw / db reproducible; without the weight gradient: the same dx
    dx2, dw2, db2 = run.out((rows, cols), dt), run.out((cols,), dt), run.out((cols,), dt)
    bwd(dy, x, w, b, mean, rstd, add, dx2, dw2, db2, rows, gelu)
    run.require(same(dx, dx2) and same(dw, dw2) and same(db, db2), "two identical launches differ")
    dx2.fill_(0)
    bwd(dy, x, w, b, mean, rstd, add, dx2, None, None, rows, gelu)
    run.require(same(dx, dx2), "need_wgrad=False changes dx")
    # ---- in place (dx is add)
    dx3 = run.out((rows, cols), dt, fill=hadd.to(dt))
    bwd(dy, x, w, b, mean, rstd, dx3, dx3, None, None, rows, gelu)
    run.require(same(dx, dx3), "dx = add in place differs from out of place")
    # ---- without `add`
    bwd(dy, x, w, b, mean, rstd, None, dx2, None, None, rows, gelu)
    dx0, _, _ = L.ln_bwd_ref(*args)
    e0, _, _, _ = L.bwd_budget("bwd", *args, out_dtype=dt)
    run.gate(dx2, dx0, e0, dt, "dx(no add)", key="dx")
    del dx0, e0
    # ---- accumulate onto a stored base, twice; then a fresh launch into the dirty buffers
    hbase = base_pair(cols, dt)
    dwa, dba = run.out((cols,), dt, fill=hbase[0].to(dt)), run.out((cols,), dt, fill=hbase[1].to(dt))
    for _ in range(2):
        before = (dwa.double().clone(), dba.double().clone())
        bwd(dy, x, w, b, mean, rstd, None, dx2, dwa, dba, rows, gelu, accumulate=True)
        _, dwe, dbe = L.ln_bwd_ref(*args, base=before)
        _, e_dw, e_db, _ = L.bwd_budget("bwd", *args, base=before, out_dtype=dt)
        run.gate(dwa, dwe, e_dw, dt, "dw(accumulate)", key="dw")
        run.gate(dba, dbe, e_db, dt, "db(accumulate)", key="db")
    bwd(dy, x, w, b, mean, rstd, None, dx2, dwa, dba, rows, gelu, accumulate=False)
    run.require(same(dwa, dw) and same(dba, db), "accumulate=False adds to what the buffers held")
    run.finish()


# ---- the row table ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(L.A_ROWS, 520), (L.B_ROWS, 4104)])
def test_x_rows_against_fp64(rows, cols):
    dt, eps, total = BF, 1e-5, rows + 37
    run = Run("x_rows-%dx%d" % (rows, cols), "fwd=%s bwd=%s" % (L.route("fwd", rows, cols), L.route("bwd", rows, cols)))
    hx = L.make_x("normal", total, cols, dt)
    hw, hb = L.make_wb("normal", cols, dt)
    hdy = L.make_dy("rowscale", rows, cols, dt)
    hadd = L.make_x("normal", total, cols, dt, 5)
    htab = L.make_row_table(rows, total)
    assert int((htab < 0).sum()) > 10 and bool((htab[1:] < htab[:-1]).any())
    x, w, b, dy, add, tab = [run.inp(t, dt) for t in (hx, hw, hb, hdy, hadd)] + [run.inp(htab, torch.int32)]
    dtab = htab.to(DEV)
    y, mean, rstd = run.out((rows, cols), dt), run.out((rows,), F32), run.out((rows,), F32)
    fwd(x, w, b, y, mean, rstd, rows, eps, False, x_rows=tab)
    ye, me, re_ = L.ln_fwd_ref(D(hx), D(hw), D(hb), eps, False, x_rows=dtab)
    e_y, e_m, e_r = L.fwd_budget(D(hx), D(hw), D(hb), eps, False, x_rows=dtab)
    run.gate(y, ye, e_y, dt, "y")
    run.gate(mean, me, e_m, F32, "mean")
    run.gate(rstd, re_, e_r, F32, "rstd")
    # backward: dx is a larger matrix that holds other bits before
    hprev = L.make_x("rowscale", total, cols, dt, 6)
    dx, dw, db = run.out((total, cols), dt, fill=hprev.to(dt)), run.out((cols,), dt), run.out((cols,), dt)
    bwd(dy, x, w, b, mean, rstd, add, dx, dw, db, rows, False, x_rows=tab)
    args = (D(hdy), D(hx), D(hw), D(hb), mean.double(), rstd.double(), False)
    dxe, dwe, dbe = L.ln_bwd_ref(*args, add=D(hadd), x_rows=dtab)
    e_dx, e_dw, e_db, _ = L.bwd_budget("bwd", *args, add=D(hadd), x_rows=dtab, out_dtype=dt)
    keep = dtab >= 0
    full = L.scatter_rows(D(hprev), dxe, dtab)
    E = L.scatter_rows(torch.zeros_like(full), torch.where(keep[:, None], e_dx, torch.zeros_like(e_dx)), dtab)
    run.gate(dx, full, E, dt, "dx")
    run.gate(dw, dwe, e_dw, dt, "dw")
    run.gate(db, dbe, e_db, dt, "db")
    named = torch.zeros(total, dtype=torch.bool, device=DEV)
    named[dtab[keep].long()] = True
    run.require(int((~named).sum()) > 37, "the table names too many rows")
    run.require(same(dx[~named], hprev.to(dt).to(DEV)[~named]), "a row of dx that no entry names changed")
    # in place: the rows no entry names keep `add`
    dxi = run.out((total, cols), dt, fill=hadd.to(dt))
    bwd(dy, x, w, b, mean, rstd, dxi, dxi, None, None, rows, False, x_rows=tab)
    run.require(same(dxi[named], dx[named]), "in place differs from out of place on the mapped rows")
    run.require(same(dxi[~named], hadd.to(dt).to(DEV)[~named]), "in place: a row that no entry names changed")
    run.finish()


# ---- GeGLU --------------------------------------------------------------------------------------------------------------
def halves_in(run, h0, h1, halves):
    """h0 / h1 as the halves of one guarded [rows, 2 cols] matrix (row stride 2 cols + 8), or two contiguous tensors."""
    if not halves:
        return run.inp(h0, BF), run.inp(h1, BF)
    host = torch.cat([h0, h1], 1).to(BF)
    H = L.guarded_from(host, BF, device=DEV)
    run.inputs.append((H, host))
    cols = h0.shape[1]
    return H[:, :cols], H[:, cols:]


GAP = 8


def halves_out(run, rows, cols, halves):
    """dh0 / dh1 as column blocks of one guarded matrix with GAP sentinel columns between them; returns (dh0, dh1, check)."""
    if not halves:
        return run.out((rows, cols), BF), run.out((rows, cols), BF), lambda: True
    M = L.guarded((rows, 2 * cols + GAP), BF, device=DEV)
    it, pat = SENTINEL[BF]
    gap = M.view(it)[:, cols:cols + GAP]
    gap.fill_(pat)
    run.outputs.append(M)
    return M[:, :cols], M[:, cols + GAP:], lambda: bool((gap == pat).all())


GF_CASES = L.by_group("D", "geglu_fwd")
GB_CASES = L.by_group("D", "geglu_bwd")


@pytest.mark.parametrize("case", GF_CASES, ids=[c.id for c in GF_CASES])
def test_ln_geglu_fwd(case):
    hip = hipmod()
    rows, cols = case.rows, case.cols
    run = Run(case.id, routes_of(case))
    hh0, hh1 = L.make_h(case.family, rows, cols)
    hw, hb = L.make_wb(case.family, cols, BF, wide=case.wide)
    h0, h1 = halves_in(run, hh0, hh1, case.halves)
    w, b = run.inp(hw, BF), run.inp(hb, BF)
    y, mean, rstd = run.out((rows, cols), BF), run.out((rows,), F32), run.out((rows,), F32)
    hip.ln_geglu_fwd(h0, h1, w, b, eps=case.eps, out=y, mean=mean, rstd=rstd)
    ye, me, re_ = L.ln_geglu_fwd_ref(D(hh0), D(hh1), D(hw), D(hb), case.eps)
    e_y, e_m, e_r = L.geglu_fwd_budget(D(hh0), D(hh1), D(hw), D(hb), case.eps)
    run.gate(y, ye, e_y, BF, "y")
    run.gate(mean, me, e_m, F32, "mean")
    run.gate(rstd, re_, e_r, F32, "rstd")
    y2 = run.out((rows, cols), BF)
    hip.ln_geglu_fwd(h0, h1, w, b, eps=case.eps, want_stats=False, out=y2)
    run.require(same(y, y2), "want_stats=False changes y")
    run.finish()


@pytest.mark.parametrize("case", GB_CASES, ids=[c.id for c in GB_CASES])
def test_ln_geglu_bwd(case):
    hip = hipmod()
    rows, cols = case.rows, case.cols
    run = Run(case.id, routes_of(case))
    hh0, hh1 = L.make_h(case.family, rows, cols)
    hw, hb = L.make_wb(case.family, cols, BF, wide=case.wide)
    hdy = L.make_dy(case.dyfam, rows, cols, BF)
    h0, h1 = halves_in(run, hh0, hh1, case.halves)
    w, b, dy = run.inp(hw, BF), run.inp(hb, BF), run.inp(hdy, BF)
    mean, rstd = run.out((rows,), F32), run.out((rows,), F32)
    hip.ln_geglu_fwd(h0, h1, w, b, eps=case.eps, out=run.out((rows, cols), BF), mean=mean, rstd=rstd)
    dh0, dh1, gap_ok = halves_out(run, rows, cols, case.halves)
    dw, db = run.out((cols,), BF), run.out((cols,), BF)
    hip.ln_geglu_bwd(dy, h0, h1, w, mean, rstd, dw=dw, db=db, accumulate=False, dh0=dh0, dh1=dh1)
    run.require(gap_ok(), "written between the halves of the gradient matrix")
    args = (D(hdy), D(hh0), D(hh1), D(hw), mean.double(), rstd.double())
    r0, r1, dwe, dbe = L.ln_geglu_bwd_ref(*args)
    e0, e1, e_dw, e_db = L.geglu_bwd_budget(*args)
    run.gate(dh0, r0, e0, BF, "dh0")
    run.gate(dh1, r1, e1, BF, "dh1")
    run.gate(dw, dwe, e_dw, BF, "dw")
    run.gate(db, dbe, e_db, BF, "db")
    del r0, r1, e0, e1
    # reproducible; the same dh0 / dh1 without the weight gradient; accumulation onto a stored base
    c0, c1, gap2 = halves_out(run, rows, cols, case.halves)
    dw2, db2 = run.out((cols,), BF), run.out((cols,), BF)
    hip.ln_geglu_bwd(dy, h0, h1, w, mean, rstd, dw=dw2, db=db2, accumulate=False, dh0=c0, dh1=c1)
    run.require(same(c0, dh0) and same(c1, dh1) and same(dw, dw2) and same(db, db2) and gap2(), "two identical launches differ")
    c0.fill_(0), c1.fill_(0)
    hip.ln_geglu_bwd(dy, h0, h1, w, mean, rstd, need_wgrad=False, dh0=c0, dh1=c1)
    run.require(same(c0, dh0) and same(c1, dh1) and gap2(), "need_wgrad=False changes dh0 / dh1")
    hbase = base_pair(cols, BF)
    dwa, dba = run.out((cols,), BF, fill=hbase[0].to(BF)), run.out((cols,), BF, fill=hbase[1].to(BF))
    for _ in range(2):
        before = (dwa.double().clone(), dba.double().clone())
        hip.ln_geglu_bwd(dy, h0, h1, w, mean, rstd, dw=dwa, db=dba, accumulate=True, dh0=c0, dh1=c1)
        _, _, dwe, dbe = L.ln_geglu_bwd_ref(*args, base=before)
        _, _, e_dw, e_db = L.geglu_bwd_budget(*args, base=before)
        run.gate(dwa, dwe, e_dw, BF, "dw(accumulate)", key="dw")
        run.gate(dba, dbe, e_db, BF, "db(accumulate)", key="db")
    run.require(same(c0, dh0) and same(c1, dh1) and gap2(), "accumulate=True changes dh0 / dh1 or writes between the halves")
    run.finish()


# ---- the fp8 copies at three trips, and one trip at the widest row of every (CH, NW) class ---------------------------------
Q8_WIDEST = [(5, cols) for cols in (512, 1024, 1536, 2048, 4096, 6144, 8192)]


@pytest.mark.parametrize("rows,cols", [(L.A_ROWS, 520), (L.B_ROWS, 4104)] + Q8_WIDEST)
def test_layernorm_q8(rows, cols):
    hip = hipmod()
    run = Run("q8-ln-%dx%d" % (rows, cols), "fwd_q8=%s" % (L.route("fwd_q8", rows, cols),))
    hx = L.make_x("rowscale", rows, cols, BF)
    hw, hb = L.make_wb("normal", cols, BF)
    x, w, b = run.inp(hx, BF), run.inp(hw, BF), run.inp(hb, BF)
    y, mean, rstd = run.out((rows, cols), BF), run.out((rows,), F32), run.out((rows,), F32)
    q = torch.full((rows + 4, cols), 0xA5, dtype=torch.uint8, device=DEV)      # (two guard rows above and below the fp8 matrix)
    qs = run.out((rows,), F32)
    qv = q[2:2 + rows]
    hip._check(hip.lib().op_layernorm_fwd_q8(hip.ptr(x), hip.ptr(w), hip.ptr(b), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), hip.ptr(qv), hip.ptr(qs),
                                             rows, cols, 1e-5, hip.stream()), "op_layernorm_fwd_q8")
    run.require(bool((q[:2] == 0xA5).all()) and bool((q[2 + rows:] == 0xA5).all()), "written outside the fp8 matrix")
    q_ref, s_ref = hip.quant_fp8_rows(y)
    run.require(torch.equal(qv, q_ref) and same(qs, s_ref), "the fp8 copy is not quant_fp8_rows(y)")
    ye, me, re_ = L.ln_fwd_ref(D(hx), D(hw), D(hb), 1e-5, False)
    e_y, e_m, e_r = L.fwd_budget(D(hx), D(hw), D(hb), 1e-5, False)
    run.gate(y, ye, e_y, BF, "y")
    run.gate(mean, me, e_m, F32, "mean")
    run.gate(rstd, re_, e_r, F32, "rstd")
    run.finish()


@pytest.mark.parametrize("rows,cols", [(8197, 520), (2053, 2056), (16389, 72), (4101, 2056), (16389, 2048)] + Q8_WIDEST)
def test_ln_geglu_q8(rows, cols):
    hip = hipmod()
    run = Run("q8-geglu-%dx%d" % (rows, cols), "geglu_fwd_q8=%s" % (L.route("geglu_fwd_q8", rows, cols),))
    hh0, hh1 = L.make_h("normal", rows, cols)
    hw, hb = L.make_wb("normal", cols, BF)
    h0, h1 = halves_in(run, hh0, hh1, True)
    w, b = run.inp(hw, BF), run.inp(hb, BF)
    y, mean, rstd, qs = run.out((rows, cols), BF), run.out((rows,), F32), run.out((rows,), F32), run.out((rows,), F32)
    q = torch.full((rows + 4, cols), 0xA5, dtype=torch.uint8, device=DEV)
    qv = q[2:2 + rows]
    hip.ln_geglu_fwd(h0, h1, w, b, out=y, mean=mean, rstd=rstd, q8=(qv, qs))
    run.require(bool((q[:2] == 0xA5).all()) and bool((q[2 + rows:] == 0xA5).all()), "written outside the fp8 matrix")
    q_ref, s_ref = hip.quant_fp8_rows(y)
    run.require(torch.equal(qv, q_ref) and same(qs, s_ref), "the fp8 copy is not quant_fp8_rows(y)")
    ye, me, re_ = L.ln_geglu_fwd_ref(D(hh0), D(hh1), D(hw), D(hb), 1e-5)
    e_y, e_m, e_r = L.geglu_fwd_budget(D(hh0), D(hh1), D(hw), D(hb), 1e-5)
    run.gate(y, ye, e_y, BF, "y")
    run.gate(mean, me, e_m, F32, "mean")
    run.gate(rstd, re_, e_r, F32, "rstd")
    run.finish()


# ---- the non-temporal variants (>= 64 MiB) against fp64, and against the default-policy kernel one row below the threshold -------
@pytest.mark.parametrize("rows,cols,dt", L.NT_CASES, ids=["%dx%d-%s" % (r, c, "bf16" if t == BF else "f32") for r, c, t in L.NT_CASES])
def test_nontemporal_variants(rows, cols, dt):
    assert L.route("fwd", rows, cols, dt)[2] and L.route("bwd", rows, cols, dt)[2] and not L.route("fwd", rows - 1, cols, dt)[2]
    run = Run("nt-%dx%d-%s" % (rows, cols, "bf16" if dt == BF else "f32"), "fwd=%s bwd=%s" % (L.route("fwd", rows, cols, dt), L.route("bwd", rows, cols, dt)))
    gelu = dt == F32
    hx = L.make_x("offset" if dt == BF else "normal", rows, cols, dt)
    hw, hb = L.make_wb("normal", cols, dt)
    hdy = L.make_dy("normal", rows, cols, dt)
    x, w, b, dy = (run.inp(t, dt) for t in (hx, hw, hb, hdy))
    y, mean, rstd = run.out((rows, cols), dt), run.out((rows,), F32), run.out((rows,), F32)
    fwd(x, w, b, y, mean, rstd, rows, 1e-5, gelu)
    dx, dw, db = run.out((rows, cols), dt), run.out((cols,), dt), run.out((cols,), dt)
    bwd(dy, x, w, b, mean, rstd, None, dx, dw, db, rows, gelu)
    xd, wd, bd = x.double(), w.double(), b.double()
    ye, me, re_ = L.ln_fwd_ref(xd, wd, bd, 1e-5, gelu)
    e_y, e_m, e_r = L.fwd_budget(xd, wd, bd, 1e-5, gelu)
    run.gate(y, ye, e_y, dt, "y")
    run.gate(mean, me, e_m, F32, "mean")
    run.gate(rstd, re_, e_r, F32, "rstd")
    del ye, e_y
    args = (dy.double(), xd, wd, bd, mean.double(), rstd.double(), gelu)
    dxe, dwe, dbe = L.ln_bwd_ref(*args)
    e_dx, e_dw, e_db, _ = L.bwd_budget("bwd", *args, out_dtype=dt)
    run.gate(dx, dxe, e_dx, dt, "dx")
    run.gate(dw, dwe, e_dw, dt, "dw")
    run.gate(db, dbe, e_db, dt, "db")
    del dxe, e_dx, args, xd
    # the first rows - 1 rows: below the threshold, the default-policy kernel
    r1 = rows - 1
    y2, mean2, rstd2, dx2 = run.out((r1, cols), dt), run.out((r1,), F32), run.out((r1,), F32), run.out((r1, cols), dt)
    fwd(x, w, b, y2, mean2, rstd2, r1, 1e-5, gelu)
    bwd(dy, x, w, b, mean, rstd, None, dx2, None, None, r1, gelu)
    run.require(same(y[:r1], y2) and same(mean[:r1], mean2) and same(rstd[:r1], rstd2), "the non-temporal forward differs from the default one")
    run.require(same(dx[:r1], dx2), "the non-temporal backward differs from the default one")
    run.finish()


# ---- non-finite rows ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols", [(L.A_ROWS, 520), (L.B_ROWS, 4104)])
def test_nonfinite_rows_stay_in_their_rows(rows, cols):
    run = Run("nonfinite-%dx%d" % (rows, cols), "fwd=%s" % (L.route("fwd", rows, cols),))
    hx = L.make_x("normal", rows, cols, BF)
    hw, hb = L.make_wb("normal", cols, BF)
    r_nan, r_inf = rows // 2 + 1, rows - 2        # (rows of a second and a third trip)
    hbad = hx.clone()
    hbad[r_nan, cols // 3] = float("nan")
    hbad[r_inf, 5], hbad[r_inf, cols - 1] = float("inf"), float("-inf")
    x, xb, w, b = run.inp(hx, BF), run.inp(hbad, BF), run.inp(hw, BF), run.inp(hb, BF)
    outs = []
    for src in (x, xb):
        y, mean, rstd = run.out((rows, cols), BF), run.out((rows,), F32), run.out((rows,), F32)
        fwd(src, w, b, y, mean, rstd, rows, 1e-5, False)
        outs.append((y, mean, rstd))
    (y, mean, rstd), (yb, meanb, rstdb) = outs
    ok = torch.ones(rows, dtype=torch.bool, device=DEV)
    ok[r_nan] = ok[r_inf] = False
    run.require(not bool(torch.isfinite(yb[~ok]).any()), "a row holding NaN / inf has finite outputs")
    run.require(same(yb[ok], y[ok]) and same(meanb[ok], mean[ok]) and same(rstdb[ok], rstd[ok]), "a non-finite row changed another row")
    run.require(bool(torch.isfinite(y).all()), "the finite run is not finite")
    run.finish()


# ---- paths that return before any launch --------------------------------------------------------------------------------
def test_zero_rows_and_refused_arguments():
    """rows = 0 with real buffers returns cleanly and writes nothing; cols % 8 != 0 and cols > 8192 are refused with an error code.
    A zero-row TENSOR has a null address, and every entry point checks its pointers before it looks at rows: the wrappers raise on
    an empty input instead of returning empty outputs (asserted below as the behaviour of today).  No caller reaches it: a residual
    branch in which a segment keeps no sample falls back to the multiplier form (TransformerEncoder._draw_kept_plans), and a batch
    has at least one row."""
    hip = hipmod()
    run = Run("rows0", "-")
    rows, cols = 3, 64
    hx = L.make_x("normal", rows, cols, BF)
    hw, hb = L.make_wb("normal", cols, BF)
    x, w, b = run.inp(hx, BF), run.inp(hw, BF), run.inp(hb, BF)
    hkeep = L.make_x("normal", rows, cols, BF, 3)
    keep2, keep1 = hkeep.to(BF).to(DEV), hkeep[0].to(BF).to(DEV)
    y, dx, d1 = (run.out((rows, cols), BF, fill=hkeep) for _ in range(3))
    mean, rstd = run.out((rows,), F32, fill=hkeep[0, :rows]), run.out((rows,), F32, fill=hkeep[0, :rows])
    dw, db = run.out((cols,), BF, fill=hkeep[0]), run.out((cols,), BF, fill=hkeep[0])
    fwd(x, w, b, y, mean, rstd, 0, 1e-5, False)
    bwd(x, x, w, b, mean, rstd, None, dx, dw, db, 0, False)
    hip._check(hip.lib().op_ln_geglu_fwd(hip.ptr(x), hip.ptr(x), cols, hip.ptr(w), hip.ptr(b), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), 0, cols, 1e-5,
                                         hip.stream()), "op_ln_geglu_fwd")
    ws = hip.workspace(hip.lib().op_layernorm_bwd_workspace_bytes(0, cols), x.device, "ln")
    hip._check(hip.lib().op_ln_geglu_bwd(hip.ptr(x), hip.ptr(x), hip.ptr(x), hip.ptr(w), hip.ptr(mean), hip.ptr(rstd), hip.ptr(dx), hip.ptr(d1), cols, cols,
                                         hip.ptr(dw), hip.ptr(db), hip.ptr(ws), 0, cols, 0, hip.stream()), "op_ln_geglu_bwd")
    torch.cuda.synchronize()
    run.require(same(y, keep2) and same(dx, keep2) and same(d1, keep2), "a launch of no rows wrote a row")
    run.require(same(dw, keep1) and same(db, keep1), "a launch of no rows wrote dw / db")
    run.require(same(mean, hkeep[0, :rows].to(DEV)) and same(rstd, hkeep[0, :rows].to(DEV)), "a launch of no rows wrote statistics")
    empty = torch.empty(0, cols, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError, match="null"):
        hip.layernorm_fwd(empty, w, b)
    with pytest.raises(RuntimeError, match="null"):
        hip.ln_geglu_fwd(empty, empty, w, b)
    bad = torch.zeros(2, 12, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):
        hip.layernorm_fwd(bad, None, None)
    wide = torch.zeros(2, 8200, dtype=BF, device=DEV)
    with pytest.raises(RuntimeError):
        hip.layernorm_fwd(wide, None, None)
    with pytest.raises(RuntimeError):
        hip.ln_geglu_fwd(wide, wide, None, None)
    run.finish()
