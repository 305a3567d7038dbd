"""The row kernels that leave out the rows of samples stochastic depth dropped (ops.SKIP_ZERO_ROWS): op_ln_geglu_fwd_skip,
op_ln_geglu_bwd_skip, op_layernorm_bwd_skip and op_resid_bwd_skip against the PLAIN entry points on the inputs of the dense step.

A row r belongs to sample r / rps; where ps[sample] == 0 the row is dropped.  The dense step has an exact-zero gradient row there (and
zeros or real activations in the forward operands), so the reference is the plain entry on such inputs.  The launch under test gets
the same inputs with every dropped row -- operands AND statistics -- overwritten with NaN: an output that is finite everywhere
proves that nothing of those rows was read.  Asserted per case:
  * kept rows are the reference's, bit for bit; so are the fp32 column partials every workgroup leaves in the workspace (read back
    after both launches) and the column sums (dw / db, dgamma / dbias / g0) after their fold;
  * dropped rows of the output are +0 -- or, where the LayerNorm backward adds a residual gradient, the bits of that row;
  * the guards around every buffer are intact and no input changed;
  * with a null ps the new entry gives the plain entry's bits.
Launches go through the C ABI into guarded, sentinel-filled buffers (tests/gemm_ref.py); the workspace holds the fp32 NaN sentinel
before every launch.  mean / rstd of a dropped row need not be written by the forward: only the kept rows' statistics are compared.

Shapes: 5 samples of 1, 3 and 64 rows (5 and 15 rows are no multiple of 4: one workgroup of the wave-per-row route holds kept and
dropped rows), every mask below, per-sample multipliers (rps = S) and the per-row vector (rps = 1), one width per route of the
dispatch, and per kernel one row count past its grid cap, so that the walk of a wave / workgroup crosses kept-dropped boundaries from
one trip to the next."""
import pytest
import torch

from tests import rows_ref as R
from tests.gemm_ref import SENTINEL

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = torch.bfloat16, torch.float32

# MIRROR of the dispatch (csrc/layernorm.hip: LN_ROUTES, OP_LN_GEGLU_BLOCKS_FWD / _BWD, g_ln_blocks_bwd; csrc/elementwise.hip:
# CS_MAX_PARTS, four rows per part and two rows per wave and trip): the rows one trip of the whole grid covers
WAVE_ROUTE_MAX_COLS = 2048


def rows_per_trip(kernel, cols):
    if kernel == "resid_bwd":
        return R.CS_MAX_PARTS * 4 * 2
    cap = 2048 if kernel == "ln_geglu_fwd" else 512
    return cap * (4 if cols <= WAVE_ROUTE_MAX_COLS else 1)


def ln_bwd_grid(rows, cols):
    """Workgroups of ln_bwd_kernel / ln_geglu_bwd_kernel (ln_grid with the cap 512): each writes one [2][cols] fp32 slot of partials."""
    return max(1, min(512, R.cdiv(rows, 4) if cols <= WAVE_ROUTE_MAX_COLS else rows))


def partials(ws, count):
    """The first `count` fp32 words of a workspace as the launches left them (the fold only reads them), on the host."""
    return ws.view(torch.int32)[:count].clone().cpu()


MASKS = ("kept", "dropped", "first", "last", "alternating")


def make_ps(mask, B, seed):
    g = torch.Generator().manual_seed(900 + seed)
    ps = 1.0 / (0.6 + 0.4 * torch.rand(B, generator=g))
    i = torch.arange(B)
    drop = {"kept": i < 0, "dropped": i >= 0, "first": i == 0, "last": i == B - 1, "alternating": i % 2 == 0}[mask]
    return torch.where(drop, torch.zeros(B), ps).float()


def hipmod():
    from one_peace_amd import hip
    return hip


def bits(t):
    return t.contiguous().view({BF: torch.int16, F32: torch.int32}[t.dtype])


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def nan_ws(nbytes, tag):
    hip = hipmod()
    ws = hip.workspace(nbytes, torch.device(DEV, torch.cuda.current_device()), tag)
    ws.view(torch.int32).fill_(SENTINEL[F32][1])
    return ws


class Bufs:
    """The guarded device buffers of one launch: inputs (compared with their host copies afterwards) and outputs."""

    def __init__(self):
        self.inputs, self.outputs = [], []

    def inp(self, host, dtype):
        if host is None:
            return None
        host = host.to(dtype)
        v = R.guarded_ld(tuple(host.shape), dtype, host.shape[1], device=DEV) if host.dim() == 2 else R.guarded_from(host, dtype, device=DEV)
        v.copy_(host.to(DEV))
        self.inputs.append((v, host))
        return v

    def out(self, shape, dtype, fill=None):
        v = R.guarded_ld(tuple(shape), dtype, shape[1], device=DEV) if len(shape) == 2 else R.guarded(tuple(shape), dtype, device=DEV)
        if fill is not None:
            v.copy_(fill.to(dtype).to(DEV))
        self.outputs.append(v)
        return v

    def check(self, what):
        torch.cuda.synchronize()
        for v in self.outputs + [v for v, _ in self.inputs]:
            assert R.check_guard(v) == 0, "%s: guard elements overwritten around a %s buffer" % (what, tuple(v.shape))
        for v, host in self.inputs:
            assert torch.equal(bits(v.cpu()), bits(host)), "%s: an input of shape %s changed" % (what, tuple(v.shape))


def nan_rows(t, dropped):
    """A copy of t ([rows, ...] or [rows]) whose dropped rows hold NaN."""
    t = t.clone()
    t[dropped] = float("nan")
    return t


def is_pos_zero(t):
    return bool((bits(t) == 0).all())


def small_cases():
    """(B, S, mask, rps is S): 5 samples of 1, 3 and 64 rows under every mask, per-sample multipliers and the per-row vector."""
    return [(5, S, mask, per_sample) for S in (1, 3, 64) for mask in MASKS for per_sample in (True, False)]


def past_cap(kernel, cols):
    """A number of 3-row samples that puts some 450 rows on the second trip of the grid."""
    return rows_per_trip(kernel, cols) // 3 + 150


def rand_bf(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn(*shape, generator=g)).to(BF).float()


def ps_args(ps, S, per_sample):
    """(device vector, rows per sample, dropped-row mask on the host)."""
    rows = ps.repeat_interleave(S)
    vec = ps if per_sample else rows
    return vec.to(DEV), (S if per_sample else 1), rows == 0


# ---- launches ------------------------------------------------------------------------------------------------------------
def c_geglu_fwd(h0, h1, w, b, y, mean, rstd, rows, cols, ps=None, rps=1, plain=False):
    hip = hipmod()
    L = hip.lib()
    if plain:
        hip._check(L.op_ln_geglu_fwd(hip.ptr(h0), hip.ptr(h1), h0.stride(0), hip.ptr(w), hip.ptr(b), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd), rows,
                                     cols, 1e-5, hip.stream()), "op_ln_geglu_fwd")
    else:
        hip._check(L.op_ln_geglu_fwd_skip(hip.ptr(h0), hip.ptr(h1), h0.stride(0), hip.ptr(w), hip.ptr(b), hip.ptr(y), hip.ptr(mean), hip.ptr(rstd),
                                          rows, cols, 1e-5, hip.ptr(ps), rps, hip.stream()), "op_ln_geglu_fwd_skip")


def c_geglu_bwd(dy, h0, h1, w, mean, rstd, dh0, dh1, dw, db, rows, cols, ps=None, rps=1, plain=False):
    hip = hipmod()
    L = hip.lib()
    ws = nan_ws(L.op_layernorm_bwd_workspace_bytes(rows, cols), "ln")
    head = (hip.ptr(dy), hip.ptr(h0), hip.ptr(h1), hip.ptr(w), hip.ptr(mean), hip.ptr(rstd), hip.ptr(dh0), hip.ptr(dh1), dh0.stride(0), h0.stride(0),
            hip.ptr(dw), hip.ptr(db), hip.ptr(ws), rows, cols, 0)
    if plain:
        hip._check(L.op_ln_geglu_bwd(*head, hip.stream()), "op_ln_geglu_bwd")
    else:
        hip._check(L.op_ln_geglu_bwd_skip(*head, hip.ptr(ps), rps, hip.stream()), "op_ln_geglu_bwd_skip")
    return partials(ws, ln_bwd_grid(rows, cols) * 2 * cols)


def c_ln_bwd(dy, x, w, mean, rstd, add, dx, dw, db, rows, cols, ps=None, rps=1, plain=False):
    hip = hipmod()
    L = hip.lib()
    ws = nan_ws(L.op_layernorm_bwd_workspace_bytes(rows, cols), "ln")
    if plain:
        hip._check(L.op_layernorm_bwd(hip.ptr(dy), hip.ptr(x), hip.ptr(w), None, hip.ptr(mean), hip.ptr(rstd), hip.ptr(add), hip.ptr(dx), hip.ptr(dw),
                                      hip.ptr(db), hip.ptr(ws), rows, cols, 0, 0, hip.DT_BF16, None, hip.stream()), "op_layernorm_bwd")
    else:
        hip._check(L.op_layernorm_bwd_skip(hip.ptr(dy), hip.ptr(x), hip.ptr(w), hip.ptr(mean), hip.ptr(rstd), hip.ptr(add), hip.ptr(dx), hip.ptr(dw),
                                           hip.ptr(db), hip.ptr(ws), rows, cols, 0, hip.ptr(ps), rps, hip.stream()), "op_layernorm_bwd_skip")
    return partials(ws, ln_bwd_grid(rows, cols) * 2 * cols)


def c_resid(dout, y, gamma, rowscale, rps, dbranch, dgamma, dbias, g0, M, N, skip):
    hip = hipmod()
    L = hip.lib()
    ws = nan_ws(L.op_resid_bwd_workspace_bytes(N), "resid")
    fn = L.op_resid_bwd_skip if skip else L.op_resid_bwd
    hip._check(fn(hip.ptr(dout), hip.ptr(y), hip.ptr(gamma), hip.ptr(rowscale), rps, hip.ptr(dbranch), hip.ptr(dgamma), hip.ptr(dbias), hip.ptr(g0),
                  hip.ptr(ws), M, N, 0, None, hip.stream()), "op_resid_bwd")
    return partials(ws, 2 * R.cs_parts(M) * N)     # (part[pass][parts][N]; a pass that was not asked for leaves the sentinel)


# ---- LayerNorm_F(GeGLU): forward and backward share their operands, and the backward needs the forward's statistics ------
def geglu_case(cols, B, S, mask, per_sample, seed):
    rows = B * S
    ps = make_ps(mask, B, seed)
    vec, rps, dropped = ps_args(ps, S, per_sample)
    kept = ~dropped
    w, b = rand_bf((cols,), seed + 1) * 0.5 + 1.0, rand_bf((cols,), seed + 2)
    hh = rand_bf((rows, 2 * cols), seed + 3, 1.5)
    hh[dropped] = 0.0     # (what the forward fill wrote into the rows no window covers; a real row serves as well: the mask `last` keeps one)
    if mask == "last":
        hh[dropped] = rand_bf((int(dropped.sum()), 2 * cols), seed + 4)
    dy = rand_bf((rows, cols), seed + 5)
    dy[dropped] = 0.0     # (the dense step: the input gradient of a zero row)
    what = "geglu %dx%d S=%d %s rps=%d" % (rows, cols, S, mask, rps)

    def forward(hh_host, plain, pvec):
        bu = Bufs()
        hhd = bu.inp(hh_host, BF)
        wd, bd = bu.inp(w, BF), bu.inp(b, BF)
        y, mean, rstd = bu.out((rows, cols), BF), bu.out((rows,), F32), bu.out((rows,), F32)
        c_geglu_fwd(hhd[:, :cols], hhd[:, cols:], wd, bd, y, mean, rstd, rows, cols, pvec, rps, plain)
        bu.check(what + " forward")
        return y.cpu(), mean.cpu(), rstd.cpu()

    ref = forward(hh, True, None)
    null = forward(hh, False, None)
    assert all(same(a, b_) for a, b_ in zip(ref, null)), what + ": a null ps does not give op_ln_geglu_fwd's bits"
    got = forward(nan_rows(hh, dropped), False, vec)
    assert bool(torch.isfinite(got[0].float()).all()), what + ": y is not finite (a dropped row was read)"
    for g_, r_, name in zip(got, ref, ("y", "mean", "rstd")):
        assert same(g_[kept], r_[kept]), "%s: kept rows of %s differ" % (what, name)
    assert is_pos_zero(got[0][dropped]), what + ": y of a dropped row is not +0"

    def backward(hh_host, dy_host, mean_host, rstd_host, plain, pvec):
        bu = Bufs()
        hhd, dyd, wd = bu.inp(hh_host, BF), bu.inp(dy_host, BF), bu.inp(w, BF)
        md, rd = bu.inp(mean_host, F32), bu.inp(rstd_host, F32)
        dh = bu.out((rows, 2 * cols), BF)
        dw, db = bu.out((cols,), BF), bu.out((cols,), BF)
        part = c_geglu_bwd(dyd, hhd[:, :cols], hhd[:, cols:], wd, md, rd, dh[:, :cols], dh[:, cols:], dw, db, rows, cols, pvec, rps, plain)
        bu.check(what + " backward")
        return dh.cpu(), dw.cpu(), db.cpu(), part

    mean, rstd = ref[1], ref[2]
    bref = backward(hh, dy, mean, rstd, True, None)
    bnull = backward(hh, dy, mean, rstd, False, None)
    assert all(same(a, b_) for a, b_ in zip(bref[:3], bnull[:3])) and torch.equal(bref[3], bnull[3]), what + ": a null ps does not give op_ln_geglu_bwd's bits"
    bgot = backward(nan_rows(hh, dropped), nan_rows(dy, dropped), nan_rows(mean, dropped), nan_rows(rstd, dropped), False, vec)
    assert all(bool(torch.isfinite(t.float()).all()) for t in bgot[:3]), what + ": a backward output is not finite (a dropped row was read)"
    assert same(bgot[0][kept], bref[0][kept]), what + ": kept rows of dh0 | dh1 differ"
    assert is_pos_zero(bgot[0][dropped]), what + ": dh0 | dh1 of a dropped row is not +0"
    assert same(bgot[1], bref[1]) and same(bgot[2], bref[2]), what + ": dw / db differ"
    assert torch.equal(bgot[3], bref[3]), what + ": the fp32 partials of dw / db differ"


@pytest.mark.parametrize("cols", [256, 1536, 6144])
def test_ln_geglu_pair_leaves_out_dropped_rows(cols):
    for i, (B, S, mask, per_sample) in enumerate(small_cases()):
        geglu_case(cols, B, S, mask, per_sample, 10 * i)


@pytest.mark.parametrize("cols", [256, 2056])
def test_ln_geglu_pair_past_the_grid_cap(cols):
    """Forward: 2048 workgroups, backward 512 (four rows each on the wave-per-row route): both walks take a second trip."""
    B = past_cap("ln_geglu_fwd", cols)
    assert B * 3 > rows_per_trip("ln_geglu_fwd", cols) > rows_per_trip("ln_geglu_bwd", cols)
    geglu_case(cols, B, 3, "alternating", True, 7)
    geglu_case(cols, B, 3, "first", False, 8)


# ---- LayerNorm backward ------------------------------------------------------------------------------------------------
def ln_bwd_case(cols, B, S, mask, per_sample, add_mode, seed):
    rows = B * S
    ps = make_ps(mask, B, seed)
    vec, rps, dropped = ps_args(ps, S, per_sample)
    kept = ~dropped
    w = rand_bf((cols,), seed + 1) * 0.5 + 1.0
    x = rand_bf((rows, cols), seed + 2, 2.0) + 0.5     # (real activations in every row: the forward LayerNorms stay dense)
    xd = x.double()
    mean = xd.mean(1).float()
    rstd = (1.0 / torch.sqrt(xd.var(1, unbiased=False) + 1e-5)).float()
    dy = rand_bf((rows, cols), seed + 3)
    dy[dropped] = 0.0
    add = rand_bf((rows, cols), seed + 4) if add_mode != "none" else None
    if add is not None:
        add[0, :8] = torch.tensor([-0.0, 0.0, 1.0, -1.0, -0.0, 0.0, 2.0, -2.0])     # (the copy keeps the sign of a zero)
    what = "ln_bwd %dx%d S=%d %s rps=%d add=%s" % (rows, cols, S, mask, rps, add_mode)

    def run(x_host, dy_host, mean_host, rstd_host, plain, pvec):
        bu = Bufs()
        xdv, dyd, wd = bu.inp(x_host, BF), bu.inp(dy_host, BF), bu.inp(w, BF)
        md, rd = bu.inp(mean_host, F32), bu.inp(rstd_host, F32)
        if add_mode == "inplace":
            dx = bu.out((rows, cols), BF, fill=add)
            addd = dx
        else:
            addd, dx = bu.inp(add, BF), bu.out((rows, cols), BF)
        dw, db = bu.out((cols,), BF), bu.out((cols,), BF)
        part = c_ln_bwd(dyd, xdv, wd, md, rd, addd, dx, dw, db, rows, cols, pvec, rps, plain)
        bu.check(what)
        return dx.cpu(), dw.cpu(), db.cpu(), part

    ref = run(x, dy, mean, rstd, True, None)
    null = run(x, dy, mean, rstd, False, None)
    assert all(same(a, b_) for a, b_ in zip(ref[:3], null[:3])) and torch.equal(ref[3], null[3]), what + ": a null ps does not give op_layernorm_bwd's bits"
    got = run(nan_rows(x, dropped), nan_rows(dy, dropped), nan_rows(mean, dropped), nan_rows(rstd, dropped), False, vec)
    assert all(bool(torch.isfinite(t.float()).all()) for t in got[:3]), what + ": an output is not finite (a dropped row was read)"
    assert same(got[0][kept], ref[0][kept]), what + ": kept rows of dx differ"
    if add is None:
        assert is_pos_zero(got[0][dropped]), what + ": dx of a dropped row is not +0"
    else:
        assert same(got[0][dropped], add.to(BF)[dropped]), what + ": dx of a dropped row is not the residual gradient's row"
        assert torch.equal(got[0][dropped].float(), ref[0][dropped].float()), what + ": dx of a dropped row is not the dense value"
    assert same(got[1], ref[1]) and same(got[2], ref[2]), what + ": dw / db differ"
    assert torch.equal(got[3], ref[3]), what + ": the fp32 partials of dw / db differ"


@pytest.mark.parametrize("cols", [256, 1536, 2056])
def test_layernorm_bwd_leaves_out_dropped_rows(cols):
    for i, (B, S, mask, per_sample) in enumerate(small_cases()):
        ln_bwd_case(cols, B, S, mask, per_sample, ("none", "add", "inplace")[i % 3], 10 * i)


@pytest.mark.parametrize("cols", [256, 2056])
def test_layernorm_bwd_past_the_grid_cap(cols):
    B = past_cap("ln_bwd", cols)
    assert B * 3 > rows_per_trip("ln_bwd", cols)
    ln_bwd_case(cols, B, 3, "alternating", True, "add", 5)
    ln_bwd_case(cols, B, 3, "last", False, "none", 6)


# ---- op_resid_bwd ------------------------------------------------------------------------------------------------------
def resid_case(N, B, S, mask, per_sample, sums, seed):
    M = B * S
    ps = make_ps(mask, B, seed)
    vec, rps, dropped = ps_args(ps, S, per_sample)
    kept = ~dropped
    dout, y = rand_bf((M, N), seed + 1), rand_bf((M, N), seed + 2)     # (real gradients in every row: the dense kernel multiplies by 0)
    gamma = rand_bf((N,), seed + 3) * 0.1
    what = "resid_bwd %dx%d S=%d %s rps=%d %s" % (M, N, S, mask, rps, "+".join(sums))

    def run(dout_host, y_host, skip):
        bu = Bufs()
        dd, gd = bu.inp(dout_host, BF), bu.inp(gamma, BF)
        yd = bu.inp(y_host, BF) if "dgamma" in sums else None
        scale = bu.inp(vec.cpu(), F32)
        dbranch = bu.out((M, N), BF)
        dgamma = bu.out((N,), BF) if "dgamma" in sums else None
        dbias = bu.out((N,), BF) if "dbias" in sums else None
        g0 = bu.out((N,), F32) if "g0" in sums else None
        part = c_resid(dd, yd, gd, scale, rps, dbranch, dgamma, dbias, g0, M, N, skip)
        bu.check(what)
        return [t.cpu() if t is not None else None for t in (dbranch, dgamma, dbias, g0)] + [part]

    ref = run(dout, y, False)
    got = run(nan_rows(dout, dropped), nan_rows(y, dropped), True)
    assert all(t is None or bool(torch.isfinite(t.float()).all()) for t in got[:4]), what + ": an output is not finite (a dropped row was read)"
    assert same(got[0][kept], ref[0][kept]), what + ": kept rows of dbranch differ"
    assert is_pos_zero(got[0][dropped]), what + ": dbranch of a dropped row is not +0"
    for g_, r_, name in zip(got[1:4], ref[1:4], ("dgamma", "dbias", "g0")):
        assert (g_ is None and r_ is None) or same(g_, r_), "%s: %s differs" % (what, name)
    assert torch.equal(got[4], ref[4]), what + ": the fp32 part slots of the column sums differ"
    if sums:
        n = R.cs_parts(M) * N
        assert bool(torch.isfinite(got[4][n:].view(F32)).all()), what + ": a part slot of the plain sum was not written"


SUMS = (("dgamma", "dbias"), ("g0", "dbias"), (), ("g0",))


@pytest.mark.parametrize("N", [256, 520, 1536])
def test_resid_bwd_leaves_out_dropped_rows(N):
    for i, (B, S, mask, per_sample) in enumerate(small_cases()):
        resid_case(N, B, S, mask, per_sample, SUMS[i % 4], 10 * i)


def test_resid_bwd_past_the_grid_cap():
    B = past_cap("resid_bwd", 256)
    assert B * 3 > rows_per_trip("resid_bwd", 256)
    resid_case(256, B, 3, "alternating", True, ("g0", "dbias"), 3)
    resid_case(256, B, 3, "first", False, ("dgamma", "dbias"), 4)


def test_resid_bwd_skip_without_multipliers_is_the_plain_entry():
    M, N = 15, 256
    dout = rand_bf((M, N), 1)
    outs = []
    for skip in (False, True):
        bu = Bufs()
        dd = bu.inp(dout, BF)
        dbranch = bu.out((M, N), BF)
        c_resid(dd, None, None, None, 0, dbranch, None, None, None, M, N, skip)
        bu.check("resid_bwd without rowscale")
        outs.append(dbranch.cpu())
    assert same(outs[0], outs[1])
