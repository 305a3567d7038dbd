"""The row-wise backward kernels of csrc/elementwise.hip -- op_colsum, op_colsum_segments, op_resid_bwd, op_gamma_grad_finish,
op_scale_rows, op_geglu_bwd, op_transpose_scaled, op_transpose_batched -- against fp64 on the SAME inputs, PER ELEMENT, on every route of
the dispatch (tests/rows_ref.py: closed forms, derived budget, families, dispatch mirror, case lists; checked on the CPU by
tests/test_rows_ref_cpu.py).

Launches go through the C ABI, so that every output is the caller's: every output and every input lives in a guarded buffer (a sentinel
bit pattern around it, checked after the launches; the transposes' guarded operands also give the odd leading dimensions), every
input is compared bit for bit with its host copy afterwards, and the workspace is filled with the fp32 NaN sentinel before every launch
that takes one -- a fold that reads a slot its first pass did not write shows as NaN.  Every gate is |got - exact| <= R + E with the E
of tests/rows_ref.py; the references are evaluated in fp64 on the device.  Each case appends one line to rows_fp64_report.txt in the
tests' output directory: its id, the mirrored route and per output the largest share |err| / (R + E), followed after the slash by the
largest (|err| - R) / E.  The Python wrappers are checked once per op to return the bits of the C-ABI launch, and M = 0 is pinned."""
import os

import pytest
import torch

from tests import rows_ref as R
from tests.gemm_ref import SENTINEL
from tests.util import out_dir

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32, I32 = R.BF, R.F32, torch.int32


def hipmod():
    from one_peace_amd import hip
    return hip


def bits(t):
    return t.contiguous().view({BF: torch.int16, F32: torch.int32, I32: torch.int32, torch.uint8: torch.uint8}[t.dtype])


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def D(t):
    return R.to64(t, DEV)


def nan_ws(nbytes, tag):
    """The cached workspace of the wrappers, every word of it the fp32 NaN sentinel."""
    hip = hipmod()
    ws = hip.workspace(nbytes, torch.device(DEV, torch.cuda.current_device()), tag)
    ws.view(torch.int32).fill_(SENTINEL[F32][1])
    return ws


class Run:
    """The guarded device tensors of one test, its failures and its largest shares."""
    reported = False      # the first case of a session starts rows_fp64_report.txt afresh: one line per case

    def __init__(self, cid, route):
        self.cid, self.route, self.fails, self.sh, self.over = cid, route, [], {}, {}
        self.inputs, self.outputs = [], []

    def inp(self, host, dtype, ld=None):
        """A guarded device copy of a host tensor; compared with the host copy at the end.  ld: a 2-D operand's leading dimension."""
        if host is None:
            return None
        host = host.to(dtype)
        if host.dim() == 2:
            v = R.guarded_ld(tuple(host.shape), dtype, ld or host.shape[1], device=DEV)
            v.copy_(host.to(DEV))
        else:
            v = R.guarded_from(host, dtype, device=DEV)
        self.inputs.append((v, host))
        return v

    def out(self, shape, dtype, fill=None, ld=None):
        v = R.guarded_ld(tuple(shape), dtype, ld or shape[1], device=DEV) if len(shape) == 2 else R.guarded(tuple(shape), dtype, device=DEV)
        if fill is not None:
            v.copy_(fill.to(DEV))
        self.outputs.append(v)
        return v

    def gate(self, got, exact, E, dtype, what, key, exact_f32=False):
        f, s, over = R.gate(got, exact, E, "bf16" if dtype == BF else "f32", "%s %s" % (what, key))
        self.fails += f
        self.sh[key] = max(self.sh.get(key, 0.0), s)
        self.over[key] = max(self.over.get(key, 0.0), over)
        if exact_f32 and dtype == F32:
            self.require(torch.equal(got.double(), exact), "%s %s: an fp32 output of the integer family is not exact" % (what, key))

    def require(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def finish(self):
        torch.cuda.synchronize()
        for v in self.outputs + [v for v, _ in self.inputs]:
            n = R.check_guard(v)
            self.require(n == 0, "%d guard elements overwritten around a %s buffer" % (n, tuple(v.shape)))
        for v, host in self.inputs:
            self.require(torch.equal(bits(v.cpu()), bits(host)), "an input of shape %s changed" % (tuple(v.shape),))
        line = "%s route %s shares %s" % (self.cid, self.route, " ".join("%s=%.4f/%.3f" % (k, v, self.over[k]) for k, v in sorted(self.sh.items())) or "(bit for bit)")
        with open(os.path.join(out_dir(), "rows_fp64_report.txt"), "a" if Run.reported else "w") as f:   # (a fresh report per session)
            f.write(line + "\n")
        Run.reported = True
        print(line)
        assert not self.fails, "\n".join(self.fails[:12])
        assert all(s <= 1 for s in self.sh.values()), self.sh


# ---- launches through the C ABI, every output given by the caller -------------------------------------------------------
def c_colsum(x, y, rowscale, rps, mul, out, M, N, accumulate):
    hip = hipmod()
    ws = nan_ws(hip.lib().op_colsum_workspace_bytes(N), "colsum")
    hip._check(hip.lib().op_colsum(hip.ptr(x), hip.ptr(y), hip.ptr(rowscale), rps, hip.ptr(mul), hip.ptr(out), hip.ptr(ws), M, N, int(accumulate),
                                   hip._dt(out), hip.stream()), "op_colsum")


def c_segments(x, outs, M, n_seg, seg_cols, accumulate):
    hip = hipmod()
    ws = nan_ws(hip.lib().op_colsum_workspace_bytes(n_seg * seg_cols), "colsum")
    o = list(outs) + [None] * (3 - len(outs))
    hip._check(hip.lib().op_colsum_segments(hip.ptr(x), hip.ptr(o[0]), hip.ptr(o[1]), hip.ptr(o[2]), hip.ptr(ws), M, n_seg, seg_cols, int(accumulate),
                                            hip.stream()), "op_colsum_segments")


def c_resid(dout, y, gamma, rowscale, rps, dbranch, dgamma, dbias, g0, M, N, accumulate, table):
    hip = hipmod()
    ws = nan_ws(hip.lib().op_resid_bwd_workspace_bytes(N), "resid")
    hip._check(hip.lib().op_resid_bwd(hip.ptr(dout), hip.ptr(y), hip.ptr(gamma), hip.ptr(rowscale), rps, hip.ptr(dbranch), hip.ptr(dgamma), hip.ptr(dbias),
                                      hip.ptr(g0), hip.ptr(ws), M, N, int(accumulate), hip.ptr(table), hip.stream()), "op_resid_bwd")


def c_finish(rowdot, pairs, dgamma, accumulate):
    hip = hipmod()
    flat = []
    for b, g in list(pairs) + [(None, None)] * (3 - len(pairs)):
        flat += [hip.ptr(b), hip.ptr(g)]
    hip._check(hip.lib().op_gamma_grad_finish(hip.ptr(rowdot), rowdot.shape[0], *flat, hip.ptr(dgamma), rowdot.shape[1], int(accumulate), hip.stream()),
               "op_gamma_grad_finish")


def c_geglu(dg, h0, h1, dh0, dh1):
    hip = hipmod()
    hip._check(hip.lib().op_geglu_bwd(hip.ptr(dg), hip.ptr(h0), hip.ptr(h1), hip.ptr(dh0), hip.ptr(dh1), dg.numel(), hip.stream()), "op_geglu_bwd")


def c_scale_rows(dout, gamma, rowscale, rps, out, M, N):
    hip = hipmod()
    hip._check(hip.lib().op_scale_rows(hip.ptr(dout), hip.ptr(gamma), hip.ptr(rowscale), rps, hip.ptr(out), M, N, hip.stream()), "op_scale_rows")


def c_transpose(x, out, scale):
    hip = hipmod()
    rows, cols = x.shape
    hip._check(hip.lib().op_transpose_scaled(hip.ptr(x), hip.ptr(out), rows, cols, x.stride(0), out.stride(0), hip.ptr(scale), hip.stream()),
               "op_transpose_scaled")


class DevRows:
    """The guarded device copies of a RowsIn."""

    def __init__(self, run, r):
        self.dout, self.full, self.y = run.inp(r.dout, BF), run.inp(r.full, BF), run.inp(r.y, BF)
        self.gamma, self.mul, self.rowscale, self.table = run.inp(r.gamma, BF), run.inp(r.mul, BF), run.inp(r.rowscale, F32), run.inp(r.table, I32)


# ---- op_colsum ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.COLSUM_PRODUCT, ids=[c.id for c in R.COLSUM_PRODUCT])
def test_colsum(case):
    M, N = case.M, case.N
    r = R.make_rows(case.family, M, N, case.rps)
    run = Run(case.id, R.route_cs(M, N))
    d = DevRows(run, r)
    for combo in case.combos():
        y, rs, mul, f32, acc = combo
        dt, what = (F32 if f32 else BF), R.combo_name(combo)
        out = run.out((N,), dt, fill=r.base0 if acc else None)
        c_colsum(d.dout, d.y if y else None, d.rowscale if rs else None, case.rps, d.mul if mul else None, out, M, N, acc)
        exact, E = R.colsum_ref(D(r.dout), budget=case.family != "integer", **D(R.colsum_kwargs(r, combo)))
        run.gate(out, exact, E, dt, what, "out", exact_f32=case.family == "integer")
    run.finish()


# ---- op_colsum_segments -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SEGMENT_CASES, ids=["segments-%dx%d-M%d-null%s-%s" % c for c in R.SEGMENT_CASES])
def test_colsum_segments(case):
    n_seg, seg_cols, M, null, family = case
    r = R.make_rows(family, M, n_seg * seg_cols)
    run = Run("segments-%dx%d-M%d-null%s-%s" % case, R.route_cs(M, seg_cols))
    x = run.inp(r.dout, BF)
    hbases = [r.base0[:seg_cols], r.base1[:seg_cols], r.mul[:seg_cols]][:n_seg]
    for acc in (False, True):
        outs = [None if i == null else run.out((seg_cols,), BF, fill=hbases[i]) for i in range(n_seg)]
        c_segments(x, outs, M, n_seg, seg_cols, acc)
        ref = R.colsum_segments_ref(D(r.dout), n_seg, seg_cols, D(hbases) if acc else None, budget=family != "integer")
        for i in range(n_seg):
            if outs[i] is not None:
                run.gate(outs[i], ref[i][0], ref[i][1], BF, "acc=%d" % acc, "out%d" % i)
    run.finish()


# ---- op_resid_bwd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.RESID_PRODUCT, ids=[c.id for c in R.RESID_PRODUCT])
def test_resid_bwd(case):
    M, N = case.M, case.N
    r = R.make_rows(case.family, M, N, case.rps)
    run = Run(case.id, R.route_cs(M, N))
    d = DevRows(run, r)
    budget = case.family != "integer"
    for combo in case.combos():
        ga, rs, sums, acc, tab = combo
        what = R.combo_name(combo)
        dbranch = run.out((M, N), BF)
        got = {"dbranch": dbranch}
        for k, hbase in (("dgamma", r.base0), ("dbias", r.base1)):
            if k in sums:
                got[k] = run.out((N,), BF, fill=hbase if acc else None)
        if "g0" in sums:
            got["g0"] = run.out((N,), F32)
        # (y is handed over also when no dgamma is asked for: it must then be ignored)
        c_resid(d.full if tab else d.dout, d.y, d.gamma if ga else None, d.rowscale if rs else None, case.rps, dbranch, got.get("dgamma"),
                got.get("dbias"), got.get("g0"), M, N, acc, d.table if tab else None)
        hd, kw = R.resid_kwargs(r, combo)
        ref = R.resid_bwd_ref(D(hd), budget=budget, **D(kw))
        assert set(ref) == set(got)
        for k, (exact, E) in ref.items():
            run.gate(got[k], exact, E, F32 if k == "g0" else BF, what, k, exact_f32=not budget)
        del ref
    run.finish()


# ---- op_gamma_grad_finish -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.FINISH_CASES, ids=["finish-%dx%d-p%d-%s" % c for c in R.FINISH_CASES])
def test_gamma_grad_finish(case):
    slots, N, npairs, family = case
    hrow, hpairs, hbase = R.make_finish(family, slots, N)
    hpairs = [(None if (i == 1 and npairs == 3) else b, g) for i, (b, g) in enumerate(hpairs[:npairs])]      # (a null bias once)
    run = Run("finish-%dx%d-p%d-%s" % case, "depth=%d" % R.finish_depth(slots))
    rowdot = run.inp(hrow, F32)
    pairs = [(run.inp(b, BF), run.inp(g, F32)) for b, g in hpairs]
    for acc in (False, True):
        out = run.out((N,), BF, fill=hbase)
        c_finish(rowdot, pairs, out, acc)
        exact, E = R.gamma_grad_finish_ref(D(hrow), D(hpairs), D(hbase) if acc else None, budget=family != "integer")
        run.gate(out, exact, E, BF, "acc=%d" % acc, "dgamma")
    run.finish()


# ---- op_geglu_bwd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.GEGLU_CASES, ids=["geglu-%d-%s" % c for c in R.GEGLU_CASES])
def test_geglu_bwd(case):
    numel, family = case
    hdg, hh0, hh1 = R.make_geglu(family, numel)
    run = Run("geglu-%d-%s" % case, "grid=%d trips=%d" % (R.ew_grid(numel // 8), R.ew_trips(numel // 8)))
    dg, h0, h1 = run.inp(hdg, BF), run.inp(hh0, BF), run.inp(hh1, BF)
    dh0, dh1 = run.out((numel,), BF), run.out((numel,), BF)
    c_geglu(dg, h0, h1, dh0, dh1)
    (r0, e0), (r1, e1) = R.geglu_bwd_ref(D(hdg), D(hh0), D(hh1))
    run.gate(dh0, r0, e0, BF, "", "dh0")
    run.gate(dh1, r1, e1, BF, "", "dh1")
    run.finish()


# ---- op_scale_rows ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SCALE_CASES, ids=["scale_rows-%dx%d-%s-g%d-r%d" % c for c in R.SCALE_CASES])
def test_scale_rows(case):
    M, N, family, ga, rs = case
    rps = R.scale_rps(M)
    r = R.make_rows(family, M, N, rps)
    run = Run("scale_rows-%dx%d-%s-g%d-r%d" % case, "rps=%d grid=%d trips=%d" % (rps, R.ew_grid(M * (N // 8)), R.ew_trips(M * (N // 8))))
    dout, gamma, rowscale = run.inp(r.dout, BF), run.inp(r.gamma if ga else None, BF), run.inp(r.rowscale if rs else None, F32)
    out = run.out((M, N), BF)
    c_scale_rows(dout, gamma, rowscale, rps, out, M, N)
    exact, E = R.scale_rows_ref(D(r.dout), D(r.gamma) if ga else None, D(r.rowscale) if rs else None, rps, budget=family != "integer")
    run.gate(out, exact, E, BF, "", "dbranch")
    run.finish()


# ---- the transposes -----------------------------------------------------------------------------------------------------
def transpose_operands(run, shape, scaled):
    rows, cols, ld_in, ld_out = shape
    hx, hscale = R.make_transpose(rows, cols)
    x = run.inp(hx, BF, ld=ld_in)
    scale = run.inp(hscale, BF) if scaled else None
    return hx, (hscale if scaled else None), x, scale, run.out((cols, rows), BF, ld=ld_out)


@pytest.mark.parametrize("shape", R.TRANSPOSE_SHAPES, ids=["%dx%d-ld%s-%s" % s for s in R.TRANSPOSE_SHAPES])
def test_transpose_scaled(shape):
    run = Run("transpose-%dx%d-ld%s-%s" % shape, "tiles=%dx%d" % (R.cdiv(shape[1], 64), R.cdiv(shape[0], 64)))
    for scaled in (False, True):
        hx, hscale, x, scale, out = transpose_operands(run, shape, scaled)
        c_transpose(x, out, scale)
        run.require(same(out, R.transpose_ref(hx, hscale).to(DEV)), "scaled=%d: the transpose is not bf(scale * in) bit for bit" % scaled)
    run.finish()


@pytest.mark.parametrize("which", R.TRANSPOSE_TABLES, ids=["table%d" % len(t) for t in R.TRANSPOSE_TABLES])
def test_transpose_batched(which):
    hip = hipmod()
    run = Run("transpose_batched-%d" % len(which), "descriptors=%s" % (which,))
    jobs, refs, singles = [], [], []
    for j, i in enumerate(which):
        hx, hscale, x, scale, out = transpose_operands(run, R.TRANSPOSE_SHAPES[i], scaled=j % 2 == 1 or len(which) == 1)
        jobs.append((x, out, scale))
        refs.append(R.transpose_ref(hx, hscale).to(DEV))
        one = run.out(tuple(out.shape), BF, ld=out.stride(0))
        c_transpose(x, one, scale)
        singles.append(one)
    table, total = hip.transpose_table(jobs, torch.device(DEV))
    hip._check(hip.lib().op_transpose_batched(hip.ptr(table), len(jobs), total, hip.stream()), "op_transpose_batched")
    for (x, out, scale), ref, one in zip(jobs, refs, singles):
        run.require(same(out, ref), "descriptor of %s: not bf(scale * in) bit for bit" % (tuple(x.shape),))
        run.require(same(out, one), "descriptor of %s: differs from the single launch" % (tuple(x.shape),))
    run.finish()


# ---- the Python wrappers return the bits of the C-ABI launch ------------------------------------------------------------
def test_wrappers_return_the_c_abi_bits():
    hip = hipmod()
    M, N, rps = 63, 520, 7
    r = R.make_rows("unit", M, N, rps)
    run = Run("wrappers", R.route_cs(M, N))
    d = DevRows(run, r)
    dout, y, gamma, mul, rowscale, table, full = (t.contiguous() if t is not None else None for t in (d.dout, d.y, d.gamma, d.mul, d.rowscale, d.table, d.full))
    # colsum
    out = run.out((N,), BF)
    c_colsum(d.dout, d.y, d.rowscale, rps, d.mul, out, M, N, False)
    run.require(same(hip.colsum(dout, y, rowscale, rps, mul), out), "hip.colsum")
    outf = run.out((N,), F32)
    c_colsum(d.dout, None, None, 0, None, outf, M, N, False)
    run.require(same(hip.colsum(dout, out_dtype=F32), outf), "hip.colsum (fp32)")
    # colsum_segments (three segments of 192 columns of another matrix, the middle output null)
    xs = R.make_rows("unit", 77, 3 * 192).dout.to(BF).to(DEV)
    souts = [run.out((192,), BF), None, run.out((192,), BF)]
    c_segments(xs, souts, 77, 3, 192, False)
    w = hip.colsum_segments(xs, 192, outs=[torch.empty(192, dtype=BF, device=DEV), None, torch.empty(192, dtype=BF, device=DEV)])
    run.require(same(w[0], souts[0]) and w[1] is None and same(w[2], souts[2]), "hip.colsum_segments")
    w = hip.colsum_segments(xs, 192)
    run.require(same(w[0], souts[0]) and same(w[2], souts[2]), "hip.colsum_segments (allocating)")
    # resid_bwd with True and with given targets, with g0 and through the row table
    br, dga, dbi = run.out((M, N), BF), run.out((N,), BF), run.out((N,), BF)
    c_resid(d.dout, d.y, d.gamma, d.rowscale, rps, br, dga, dbi, None, M, N, False, None)
    w = hip.resid_bwd(dout, y, gamma, rowscale, rps, dgamma=True, dbias=True)
    run.require(same(w[0], br) and same(w[1], dga) and same(w[2], dbi), "hip.resid_bwd (True)")
    hb = (r.base0.to(BF).to(DEV), r.base1.to(BF).to(DEV))
    dga2, dbi2 = run.out((N,), BF, fill=r.base0), run.out((N,), BF, fill=r.base1)
    c_resid(d.dout, d.y, d.gamma, d.rowscale, rps, br, dga2, dbi2, None, M, N, True, None)
    w = hip.resid_bwd(dout, y, gamma, rowscale, rps, dgamma=hb[0], dbias=hb[1], accumulate=True)
    run.require(same(w[1], dga2) and same(w[2], dbi2) and w[1] is hb[0], "hip.resid_bwd (given targets, accumulate)")
    g0, br0, dbi3 = run.out((N,), F32), run.out((M, N), BF), run.out((N,), BF)
    c_resid(d.full, None, d.gamma, d.rowscale, rps, br0, None, dbi3, g0, M, N, False, d.table)
    wg0 = torch.empty(N, dtype=F32, device=DEV)
    w = hip.resid_bwd(full, None, gamma, rowscale, rps, dbias=True, g0=wg0, dout_rows=table)
    run.require(same(w[0], br0) and same(w[2], dbi3) and same(wg0, g0) and w[1] is None, "hip.resid_bwd (g0, row table)")
    # gamma_grad_finish
    hrow, hpairs, hbase = R.make_finish("unit", 29, 200)
    rowdot = hrow.to(DEV)
    pairs = [(b.to(BF).to(DEV), g.to(DEV)) for b, g in hpairs[:2]]
    fo = run.out((200,), BF, fill=hbase)
    c_finish(rowdot, pairs, fo, True)
    run.require(same(hip.gamma_grad_finish(rowdot, pairs, hbase.to(BF).to(DEV), True), fo), "hip.gamma_grad_finish")
    # geglu_bwd, scale_rows
    hdg, hh0, hh1 = (t.to(BF).to(DEV) for t in R.make_geglu("sweep", 8 * 257))
    o0, o1 = run.out((8 * 257,), BF), run.out((8 * 257,), BF)
    c_geglu(hdg, hh0, hh1, o0, o1)
    w = hip.geglu_bwd(hdg, hh0, hh1)
    run.require(same(w[0], o0) and same(w[1], o1), "hip.geglu_bwd")
    so = run.out((M, N), BF)
    c_scale_rows(d.dout, d.gamma, d.rowscale, rps, so, M, N)
    run.require(same(hip.scale_rows(dout, gamma, rowscale, rps), so), "hip.scale_rows")
    # transpose, transpose_table + transpose_batched
    hx, hscale, x, scale, to = transpose_operands(run, (65, 67, 72, None), True)
    c_transpose(x, to, scale)
    run.require(same(hip.transpose(x, scale=scale), to), "hip.transpose")
    tb = torch.zeros(67, 65, dtype=BF, device=DEV)
    table_, total = hip.transpose_table([(x, tb, scale)], torch.device(DEV))
    hip.transpose_batched(table_, 1, total)
    run.require(same(tb, to), "hip.transpose_table + hip.transpose_batched")
    run.finish()


# ---- M = 0 --------------------------------------------------------------------------------------------------------------
def test_zero_rows():
    """The sum over no rows is zero: non-accumulating outputs come back as zeros, accumulating ones untouched, g0 zero, nothing is written
    elsewhere -- at the C ABI with valid pointers and M = 0, and through the wrappers with empty tensors (whose address is null)."""
    hip = hipmod()
    N, rows = 64, 3
    r = R.make_rows("unit", rows, N)
    run = Run("rows0", "-")
    d = DevRows(run, r)
    keep1, zero1 = r.base0.to(BF).to(DEV), torch.zeros(N, dtype=BF, device=DEV)
    keep2 = r.y.to(BF).to(DEV)
    for acc in (False, True):
        want = keep1 if acc else zero1
        out, outf = run.out((N,), BF, fill=r.base0), run.out((N,), F32, fill=r.base0)
        c_colsum(d.dout, d.y, d.rowscale, 1, d.mul, out, 0, N, acc)
        c_colsum(d.dout, None, None, 0, None, outf, 0, N, acc)
        run.require(same(out, want) and same(outf, want.float()), "op_colsum, M = 0, accumulate=%d" % acc)
        s0, s2 = run.out((32,), BF, fill=r.base0[:32]), run.out((32,), BF, fill=r.base0[:32])
        c_segments(d.dout, [s0, None], 0, 2, 32, acc)
        c_segments(d.dout, [None, s2], 0, 2, 32, acc)
        run.require(same(s0, want[:32]) and same(s2, want[:32]), "op_colsum_segments, M = 0, accumulate=%d" % acc)
        br, dga, dbi = run.out((rows, N), BF, fill=r.y), run.out((N,), BF, fill=r.base0), run.out((N,), BF, fill=r.base0)
        c_resid(d.dout, d.y, d.gamma, d.rowscale, 1, br, dga, dbi, None, 0, N, acc, None)
        run.require(same(dga, want) and same(dbi, want) and same(br, keep2), "op_resid_bwd (dgamma, dbias), M = 0, accumulate=%d" % acc)
        g0, dbi2 = run.out((N,), F32, fill=r.base0), run.out((N,), BF, fill=r.base0)
        c_resid(d.full, None, d.gamma, d.rowscale, 1, br, None, dbi2, g0, 0, N, acc, d.table)
        run.require(same(g0, zero1.float()) and same(dbi2, want) and same(br, keep2), "op_resid_bwd (g0, dbias, row table), M = 0, accumulate=%d" % acc)
        c_resid(d.dout, None, d.gamma, None, 0, br, None, None, None, 0, N, acc, None)
        run.require(same(br, keep2), "op_resid_bwd (no sums), M = 0: dbranch written")
    # the wrappers, on empty tensors
    e2, e1, et = torch.empty(0, N, dtype=BF, device=DEV), torch.empty(0, dtype=F32, device=DEV), torch.empty(0, dtype=I32, device=DEV)
    gamma = d.gamma.contiguous()
    run.require(same(hip.colsum(e2, e2, e1, 1, gamma), zero1) and same(hip.colsum(e2, out_dtype=F32), zero1.float()), "hip.colsum on an empty tensor")
    acc_out = keep1.clone()
    run.require(hip.colsum(e2, out=acc_out, accumulate=True) is acc_out and same(acc_out, keep1), "hip.colsum on an empty tensor, accumulate")
    w = hip.colsum_segments(e2, 32)
    run.require(len(w) == 2 and all(same(t, zero1[:32]) for t in w), "hip.colsum_segments on an empty tensor")
    w = hip.resid_bwd(e2, e2, gamma, e1, 1, dgamma=True, dbias=True)
    run.require(tuple(w[0].shape) == (0, N) and same(w[1], zero1) and same(w[2], zero1), "hip.resid_bwd on an empty tensor")
    a0, a1, g0 = keep1.clone(), keep1.clone(), torch.full((N,), 3.0, dtype=F32, device=DEV)
    hip.resid_bwd(e2, e2, gamma, e1, 1, dgamma=a0, dbias=a1, accumulate=True)
    run.require(same(a0, keep1) and same(a1, keep1), "hip.resid_bwd on an empty tensor, accumulate")
    w = hip.resid_bwd(d.full.contiguous(), None, gamma, e1, 1, dbias=True, g0=g0, dout_rows=et)
    run.require(tuple(w[0].shape) == (0, N) and same(w[2], zero1) and same(g0, zero1.float()), "hip.resid_bwd with an empty row table")
    run.require(tuple(hip.resid_bwd(e2)[0].shape) == (0, N), "hip.resid_bwd on an empty tensor, no sums")
    run.finish()
