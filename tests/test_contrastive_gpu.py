"""The contrastive head on the device against float64 torch: op_infonce_rows, op_l2norm_fwd/_bwd in both output dtypes,
ops.info_nce (ITC/ATC) and ops.dcl_loss (the four masked-token terms), at the shapes training runs them.

References are plain torch ops in float64 on the same bf16-rounded inputs the kernels get: on the device for the large
shapes, on the CPU for the small ones.  Every tolerance is stated next to its assertion."""
import math

import pytest
import torch
import torch.nn.functional as F

from oracle import onepeace_oracle as O
from tests.util import BF16_FRO, BF16_MAX, assert_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
U32 = 2.0 ** -24  # fp32 unit roundoff


def hipmod():
    from one_peace_amd import hip
    return hip


def opsmod():
    from one_peace_amd import ops
    return ops


def dgen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def ref_device(numel):
    return DEV if numel > (1 << 16) else "cpu"


# ------------------------------------------------------------------------------------------------------------------
# op_infonce_rows
# ------------------------------------------------------------------------------------------------------------------
def nce_ref(sim, t0, eps, gscale):
    """fp64 row losses (smoothed NLL of log_softmax, eps/(n-1) as in adjust_label_smoothed_nll_loss), gscale * their autograd
    gradient, <grad, sim> and sum |grad * sim| per row, and first-index argmax hits."""
    s64 = sim.to(ref_device(sim.numel()), torch.float64, copy=True).requires_grad_(True)
    rows, n = s64.shape
    tgt = torch.arange(rows, device=s64.device) + t0
    lp = F.log_softmax(s64, dim=-1)
    loss = -lp.gather(1, tgt[:, None]).squeeze(1)
    if eps:
        e = eps / (n - 1)
        loss = (1 - eps - e) * loss - e * lp.sum(-1)
    (loss.sum() * gscale).backward()
    g = s64.grad
    s = s64.detach()
    return loss.detach(), g, (g * s).sum(1), (g * s).abs().sum(1), (s.argmax(1) == tgt).double()


def nce_check(sim_in, t0, eps, gscale, what):
    """Runs op_infonce_rows on a copy of sim_in and checks everything it writes against nce_ref."""
    hip = hipmod()
    rows, n = sim_in.shape
    s = sim_in.clone()
    loss, hit, dot = hip.infonce_rows(s, t0, eps, gscale=gscale, write_grad=True)
    rl, rg, rdot, rabs, rhit = nce_ref(sim_in, t0, eps, gscale)
    dev = rl.device
    smax = float(sim_in.abs().max())
    mag = smax + math.log(n) + 1.0  # size of the fp32 terms lse, s_t, mean(s) whose difference is the loss
    # loss: a difference of fp32 quantities of size <= mag, each within a few ulps, plus (smoothing) eps/(n-1) times the
    # n-term fp32 sum of the row, whose error is ~(n/256 + 8) ulps of n * smax.  32 ulps of mag covers both
    # (measured: <= 4.0 ulps of mag).
    el = float((loss.to(dev).double() - rl).abs().max())
    assert el <= 32 * U32 * mag, "%s: loss err %.3e > %.3e" % (what, el, 32 * U32 * mag)
    # gradient: gscale * (p_k * c - e - [k == t] * w).  p_k = exp(s_k - lse) carries a relative error of a few ulps of
    # |s_k - lse| <= 2 smax + log n (argument rounding of the fast exp and of the subtraction), so the absolute error is
    # bounded by gscale * p_k * (few ulps) * mag2; 4 ulps of gscale * mag2 bounds every entry (measured: <= 0.32).
    mag2 = 2 * smax + math.log(n) + 1.0
    eg = float((s.to(dev).double() - rg).abs().max())
    assert eg <= 4 * U32 * gscale * mag2, "%s: grad err %.3e > %.3e" % (what, eg, 4 * U32 * gscale * mag2)
    # <grad, sim>: the gradient error above times |s| <= smax (the p_k sum to one), plus the fp32 sum of n products:
    # ~(n/256 + 8) ulps of sum |g s| (measured: <= 0.13 of the bound)
    ed = (dot.to(dev).double() - rdot).abs()
    bound = 4 * U32 * gscale * mag2 * (smax + 1) + 4 * (n / 256 + 8) * U32 * rabs
    assert bool((ed <= bound).all()), "%s: dot err %.3e (bound %.3e)" % (what, float(ed.max()), float(bound.max()))
    # hits: the kernel reads the same fp32 values, so the argmax (first index on ties) is exact
    assert torch.equal(hit.to(dev).double(), rhit), what
    return s, loss, hit, dot


def nce_sims(rows, n, t0, scale, seed):
    """scale * cos with cos uniform in [-1, 1); every second row has its target at cos = 1 (a clear hit, and a row loss
    near zero at scale 100 -- the cancellation case of lse - s_t)."""
    g = dgen(seed)
    cos = torch.rand(rows, n, device=DEV, generator=g) * 2 - 1
    r = torch.arange(0, rows, 2, device=DEV)
    cos[r, r + t0] = 1.0
    return (scale * cos).float().contiguous()


@pytest.mark.parametrize("n", [2, 63, 256, 257, 1000, 2048, 16387])
@pytest.mark.parametrize("eps", [0.0, 0.1])
def test_infonce_rows_fp64(n, eps):
    """Sizes from one column trip to 64 (DCL), targets at the start, the middle and the end of the row, logit scales
    1, 2.5 (DCL) and 100 (the clamp of logit_scale.exp())."""
    for rows in (1, 37, 256):
        if rows > n:
            continue
        for t0 in sorted({0, (n - rows) // 2, n - rows}):
            for scale in (1.0, 2.5, 100.0):
                sim = nce_sims(rows, n, t0, scale, seed=n * 7 + rows + t0)
                nce_check(sim, t0, eps, 0.37, "n=%d rows=%d t0=%d eps=%g scale=%g" % (n, rows, t0, eps, scale))


@pytest.mark.parametrize("n", [1000, 16387])
def test_infonce_rows_ld_and_no_grad(n):
    """A view into a wider buffer (ld > n) gives the bits of the contiguous run and leaves the columns past n alone;
    write_grad=False leaves sim bit-unchanged, writes dot = 0 and the same loss and hits."""
    hip = hipmod()
    rows, t0, ld = 37, 5, n + 40
    sim = nce_sims(rows, n, t0, 100.0, seed=3)
    buf = torch.randn(rows, ld, device=DEV, generator=dgen(4))
    buf[:, :n] = sim
    before = buf.clone()
    view = buf[:, :n]
    assert view.stride(0) == ld
    lv, hv, dv = hip.infonce_rows(view, t0, 0.1, gscale=0.5, write_grad=True)
    s, lc, hc, dc = nce_check(sim, t0, 0.1, 0.5, "ld n=%d" % n)
    assert torch.equal(buf[:, n:], before[:, n:])
    assert torch.equal(view, s) and torch.equal(lv, lc) and torch.equal(hv, hc) and torch.equal(dv, dc)
    s2 = sim.clone()
    l2, h2, d2 = hip.infonce_rows(s2, t0, 0.1, gscale=0.5, write_grad=False)
    assert torch.equal(s2, sim)
    assert torch.equal(d2, torch.zeros_like(d2))
    assert torch.equal(l2, lc) and torch.equal(h2, hc)


@pytest.mark.parametrize("n,t0", [(300, 0), (2048, 0), (2048, 2048 - 256), (16387, 9000)])
def test_infonce_rows_argmax_ties(n, t0):
    """Exact ties for the maximum, placed so that the first maximal column falls in another lane of the same wave, another
    wave, a later loop trip of the same thread, or anywhere (2- and 3-way ties).  hit = 1 exactly when the target is the
    FIRST maximal column, as torch.argmax returns."""
    rows = 256
    g = torch.Generator().manual_seed(n + t0)
    cos = torch.rand(rows, n, generator=g) * 0.5
    trips = (n + 255) // 256
    for r in range(rows):
        t = t0 + r
        kind = r % 4
        if kind == 0:  # same wave, other lane, same trip
            base = t - t % 64
            others = [base + int(torch.randint(0, 64, (1,), generator=g))]
        elif kind == 1:  # same thread, other trip
            others = [t % 256 + 256 * int(torch.randint(0, trips, (1,), generator=g))]
        elif kind == 2:  # anywhere
            others = [int(torch.randint(0, n, (1,), generator=g))]
        else:  # three-way
            others = [int(v) for v in torch.randint(0, n, (2,), generator=g)]
        others = [o for o in others if o != t and o < n] or [(t + 64) % n]
        cos[r, t] = 0.75
        cos[r, others] = 0.75
    sim = (100.0 * cos).float().to(DEV)
    _, _, hit, _ = nce_check(sim, t0, 0.0, 1.0, "ties n=%d t0=%d" % (n, t0))
    first = torch.tensor([int(torch.nonzero(sim[r].cpu() == sim[r].max().cpu())[0]) for r in range(rows)])
    assert torch.equal(hit.cpu(), (first == torch.arange(rows) + t0).float())
    assert 0 < float(hit.sum()) < rows  # both outcomes occur


def test_infonce_rows_nan_row():
    """A NaN in one row makes that row's loss, gradient and dot NaN; every other row keeps the bits of a clean run."""
    hip = hipmod()
    rows, n, t0, bad = 37, 1000, 100, 11
    sim = nce_sims(rows, n, t0, 100.0, seed=9)
    clean, dirty = sim.clone(), sim.clone()
    dirty[bad, 517] = float("nan")
    lc, hc, dc = hip.infonce_rows(clean, t0, 0.1, gscale=0.25)
    ld, hd, dd = hip.infonce_rows(dirty, t0, 0.1, gscale=0.25)
    ok = torch.arange(rows, device=DEV) != bad
    assert torch.equal(ld[ok], lc[ok]) and torch.equal(hd[ok], hc[ok]) and torch.equal(dd[ok], dc[ok])
    assert torch.equal(dirty[ok], clean[ok])
    assert bool(torch.isnan(ld[bad])) and bool(torch.isnan(dd[bad])) and bool(torch.isnan(dirty[bad]).all())


# ------------------------------------------------------------------------------------------------------------------
# op_l2norm_fwd / op_l2norm_bwd
# ------------------------------------------------------------------------------------------------------------------
def l2_inputs(rows, cols, seed, dy_dtype):
    """Rows of norms 0.1 .. 100; with rows >= 3, row 1 is zero and row 2 has norm 0.5e-12 < eps with dy along x (where
    the projection term a kernel must drop would otherwise remove most of dy)."""
    g = dgen(seed)
    x = torch.randn(rows, cols, device=DEV, generator=g, dtype=torch.float64)
    x = x * torch.pow(10.0, torch.rand(rows, 1, device=DEV, generator=g, dtype=torch.float64) * 3 - 1) / math.sqrt(cols)
    dy = torch.randn(rows, cols, device=DEV, generator=g, dtype=torch.float64)
    edges = []
    if rows >= 3:
        x[1] = 0
        x[2] = x[2] / x[2].norm() * 0.5e-12
        dy[2] = x[2] / x[2].norm() * math.sqrt(cols) + 0.1 * dy[2]
        edges = [1, 2]
    return x.to(torch.bfloat16), dy.to(dy_dtype), edges


@pytest.mark.parametrize("cols", [8, 64, 512, 520, 768, 1536, 8200])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
def test_l2norm_fp64(cols, out_dtype):
    """bf16 y: forward and backward exactly as L2NormalizeFn runs them (bf16 dy, the backward reads the bf16 y).  fp32 y:
    the op pair with fp32 dy.  Widths with a partial last 512-column pass (520, 768, 8200) and a zero row and a row with
    0 < ||x|| < eps, where F.normalize's gradient is dy / eps (clamp_min passes none)."""
    hip, ops = hipmod(), opsmod()
    for rows in (1, 3, 5, 257, 12288):
        what = "rows=%d cols=%d %s" % (rows, cols, out_dtype)
        x, dy, edges = l2_inputs(rows, cols, seed=rows + cols, dy_dtype=out_dtype)
        rdev = ref_device(x.numel())
        x64 = x.double().to(rdev).requires_grad_(True)
        y64 = F.normalize(x64, dim=1)
        y64.backward(dy.double().to(rdev))
        r64, dx64 = y64.detach(), x64.grad
        if out_dtype == torch.bfloat16:
            xin = x.clone().requires_grad_(True)
            y = ops.l2_normalize(xin)
            y.backward(dy)
            dx = xin.grad
            _, inv = hip.l2norm_fwd(x)
        else:
            y, inv = hip.l2norm_fwd(x, out_dtype=torch.float32)
            dx = hip.l2norm_bwd(dy, y, inv)
        assert y.dtype == out_dtype and dx.dtype == torch.bfloat16
        y, dx = y.detach().to(rdev).double(), dx.to(rdev).double()
        nrm = x64.detach().norm(dim=1)
        keep = torch.ones(rows, dtype=torch.bool, device=rdev)
        keep[edges] = False
        # y: bf16 -- one rounding of a unit vector (util.BF16_*); fp32 -- a few ulps (as test_ops_gpu.test_l2norm)
        # (measured: bf16 rel-fro 1.9e-3, max-rel 3.4e-3; fp32 8.3e-8, 1.9e-7)
        tol = {} if out_dtype == torch.bfloat16 else dict(fro=1e-6, mx=1e-5)
        assert_close(y[keep], r64[keep], what=what + " y", **tol)
        # dx row-wise relative: rows of norm 0.1 .. 100 give gradients 1e-1 .. 1e1 times apart, so each row is scaled by
        # its norm first.  One bf16 rounding of dx, plus bf16 y / dy in the projection (util.BF16_*; measured: rel-fro
        # 2.3e-3, max-rel 3.6e-3)
        s = nrm[keep, None]
        assert_close(dx[keep] * s, dx64[keep] * s, what=what + " dx")
        # inv_norm = 1 / max(||x||, eps): fp32 sum of squares, a few ulps
        inv = inv.to(rdev).double()
        assert_close(inv[keep], 1.0 / nrm[keep], fro=1e-6, mx=1e-6, what=what + " inv")
        for r in edges:
            # zero row: y = 0 exactly; tiny row: y = x / eps.  Both: dx = dy / eps (same tolerances)
            if r == 1:
                assert float(y[r].abs().max()) == 0.0
            else:
                assert_close(y[r], r64[r], what=what + " tiny y", **tol)
            assert_close(dx[r], dx64[r], what=what + " edge %d dx" % r)
        for r in edges:  # inv_norm = -1 / eps marks the clamp
            assert abs(float(inv[r]) + 1e12) <= 1e-6 * 1e12, what


# ------------------------------------------------------------------------------------------------------------------
# ops.info_nce (InfoNCEFn) against fp64 autograd of O.itc_loss
# ------------------------------------------------------------------------------------------------------------------
def unit_rows(x):
    return F.normalize(x.double(), dim=1).to(torch.bfloat16)


def itc_inputs(b, H, world, rank, seed):
    """L2-normalised bf16 embeddings: b_local[i] = normalise(a_local[i] + sigma_i * noise) with sigma_i in [1, 20]
    (cosines 0.05 .. 0.7: hits and misses at every size), the other ranks' rows independent."""
    g = dgen(seed)
    a = torch.randn(b, H, device=DEV, generator=g, dtype=torch.float64) / math.sqrt(H)
    sig = 1 + 19 * torch.rand(b, 1, device=DEV, generator=g, dtype=torch.float64)
    t = a + sig * torch.randn(b, H, device=DEV, generator=g, dtype=torch.float64) / math.sqrt(H)
    a_l, b_l = unit_rows(a), unit_rows(t)
    a_all = unit_rows(torch.randn(world * b, H, device=DEV, generator=g))
    b_all = unit_rows(torch.randn(world * b, H, device=DEV, generator=g))
    a_all[rank * b:(rank + 1) * b] = a_l
    b_all[rank * b:(rank + 1) * b] = b_l
    return a_l, b_l, a_all, b_all


def itc_run(a_l, b_l, a_all, b_all, scale, rank, ls):
    """(HIP loss, hits, grads) and (fp64 oracle loss, hits, grads)."""
    ops = opsmod()
    al, bl = a_l.clone().requires_grad_(True), b_l.clone().requires_grad_(True)
    sc = torch.tensor(scale, dtype=torch.float32, device=DEV, requires_grad=True)
    loss, ha, hb = ops.info_nce(al, bl, a_all, b_all, sc, rank, ls)
    loss.backward()
    a64, b64 = a_l.double().requires_grad_(True), b_l.double().requires_grad_(True)
    s64 = torch.tensor(scale, dtype=torch.float64, device=DEV, requires_grad=True)
    rl, rha, rhb = O.itc_loss(a64, b64, a_all.double(), b_all.double(), s64, rank, ls)
    rl.backward()
    return (loss.detach(), ha, hb, al.grad, bl.grad, sc.grad), (rl.detach(), rha, rhb, a64.grad, b64.grad, s64.grad)


def dscale_mag(local, allv, scale, rank, ls):
    """sum over rows and columns of |dsim| (|sim| + 1) / scale in fp64: the size of the terms d scale is summed from."""
    b = local.shape[0]
    sim = scale * local.double() @ allv.double().t()
    g = nce_ref(sim, rank * b, ls, 0.5 / b)[1]
    return float((g.abs() * (sim.to(g.device).abs() + 1)).sum()) / scale


def clear_hits(local, allv, scale, rank):
    """(hits over the rows whose fp64 top-2 gap exceeds the fp32 GEMM's error bound, number of rows that do not).  The
    kernel's sims are fp32 sums of H exact bf16 products of unit vectors: |error| <= H * u32 * scale on each side."""
    b, H = local.shape
    sim = scale * local.double() @ allv.double().t()
    top = sim.topk(2, dim=1).values
    clear = (top[:, 0] - top[:, 1]) > 2 * H * U32 * scale
    tgt = torch.arange(b, device=DEV) + rank * b
    hit = sim.argmax(1) == tgt
    return float((hit & clear).sum()), int((~clear).sum())


@pytest.mark.parametrize("b,H", [(4, 768), (37, 520), (37, 1536), (128, 768), (256, 1536), (256, 520)])
@pytest.mark.parametrize("world,rank", [(1, 0), (2, 0), (2, 1), (8, 0), (8, 7)])
def test_info_nce_fp64(b, H, world, rank):
    """Loss, d a_local, d b_local and d scale against fp64 autograd of O.itc_loss, and the hit counts on clear rows.
    b = 37 with H = 520 runs both padding branches of gemm_any (K to 576, N = 37 world to a multiple of 8)."""
    a_l, b_l, a_all, b_all = itc_inputs(b, H, world, rank, seed=b * 131 + H + world * 7 + rank)
    n = world * b
    for ls in (0.0, 0.1):
        for scale in (1.0, 100.0):
            what = "b=%d H=%d world=%d rank=%d ls=%g scale=%g" % (b, H, world, rank, ls, scale)
            (loss, ha, hb, da, db, dsc), (rl, rha, rhb, rda, rdb, rdsc) = itc_run(a_l, b_l, a_all, b_all, scale, rank, ls)
            # loss: the fp32 sims differ from fp64 by <= ~sqrt(H) u32 scale (random-signed sums of H products), the
            # row loss moves by at most that, plus the op's own 32 ulps of (scale + log n) (measured: <= 0.04 of the bound)
            el = abs(float(loss) - float(rl))
            bl = 4 * math.sqrt(H) * U32 * scale + 32 * U32 * (scale + math.log(n) + 1)
            assert el <= bl, "%s: loss %.3e > %.3e" % (what, el, bl)
            # d a / d b: dsim rounded to bf16 before the backward GEMM, the result rounded to bf16: two bf16 roundings
            # (util.BF16_*, which holds one rounding with room for two at RMS 1.1e-3 each; measured: rel-fro <= 3.0e-3)
            assert_close(da, rda, what=what + " da")
            assert_close(db, rdb, what=what + " db")
            # d scale = sum(dsim * sim) / scale from the kernel's fp32 row dots.  The fp32 sims are off by ~sqrt(H) u32
            # scale, which moves each p_k by that relative amount and each sim by that absolute amount; the terms can
            # cancel between rows, so the bound is relative to their size sum |dsim| (|sim| + 1) / scale (measured: <= 0.23
            # of the bound, at b = 4 and scale 100)
            mag = dscale_mag(a_l, b_all, scale, rank, ls) + dscale_mag(b_l, a_all, scale, rank, ls)
            es = abs(float(dsc) - float(rdsc))
            bs = 8 * math.sqrt(H) * U32 * (scale + 1) * mag
            assert es <= bs, "%s: dscale err %.3e > %.3e (got %.6e ref %.6e)" % (what, es, bs, float(dsc), float(rdsc))
            # hits: exact on rows whose top-2 gap is clear of the fp32 rounding; rows that are not may go either way
            for got, loc, allv in ((ha, a_l, b_all), (hb, b_l, a_all)):
                want, unclear = clear_hits(loc, allv, scale, rank)
                assert want <= float(got) <= want + unclear, \
                    "%s: hits %g, clear %g, unclear %d" % (what, float(got), want, unclear)


@pytest.mark.parametrize("rank", [0, 1])
def test_info_nce_tied_hits(rank):
    """Exact ties built by construction: the other rank holds bit copies of some local rows.  The copies tie with the
    target; on rank 0 they come after it (hit), on rank 1 before it (miss), exactly as torch.argmax's first index."""
    b, H, world = 37, 520, 2
    g = dgen(77)
    a = torch.randn(b, H, device=DEV, generator=g, dtype=torch.float64)
    a_l = unit_rows(a)
    b_l = unit_rows(a + 0.3 * torch.randn(b, H, device=DEV, generator=g, dtype=torch.float64))  # cos ~ 0.96: target wins
    a_all = unit_rows(torch.randn(world * b, H, device=DEV, generator=g))
    b_all = unit_rows(torch.randn(world * b, H, device=DEV, generator=g))
    a_all[rank * b:(rank + 1) * b] = a_l
    b_all[rank * b:(rank + 1) * b] = b_l
    other = (1 - rank) * b
    dup = torch.arange(0, b, 3, device=DEV)  # rows whose target gets a bit copy on the other rank
    b_all[other + dup] = b_l[dup]
    a_all[other + dup] = a_l[dup]
    ops = opsmod()
    for loc, allv in ((a_l, b_all), (b_l, a_all)):  # premise: the GEMM gives equal columns bit-equal values
        sim = ops.gemm_any(loc, allv, out_f32=True, alpha=torch.full((1,), 100.0, device=DEV))
        assert torch.equal(sim[dup, rank * b + dup], sim[dup, other + dup])
    (_, ha, hb, *_), (_, rha, rhb, *_) = itc_run(a_l, b_l, a_all, b_all, 100.0, rank, 0.0)
    expect = b if rank == 0 else b - dup.numel()
    assert float(rha) == expect and float(rhb) == expect  # the fp64 oracle's argmax agrees with the construction
    assert float(ha) == expect and float(hb) == expect


# ------------------------------------------------------------------------------------------------------------------
# ops.dcl_loss (DclFn) against O.dcl_loss
# ------------------------------------------------------------------------------------------------------------------
def dcl_features(m, n, H, seed):
    """Raw (not normalised) bf16 features: teacher [n, H]; the m masked student rows predict the first m teacher rows
    (student = teacher + noise, cos ~ 0.45), so the softmax is far from uniform."""
    g = dgen(seed)
    t = torch.randn(n, H, device=DEV, generator=g, dtype=torch.float64)
    s = t[:m] + 2 * torch.randn(m, H, device=DEV, generator=g, dtype=torch.float64)
    return s.to(torch.bfloat16), t.to(torch.bfloat16)


def dcl_oracle(s, t, scale, ls):
    """O.dcl_loss in fp64 on [1, 1 + n, H] features: position 0 is the CLS token, positions 1 .. m are masked (targets
    0 .. m-1).  Returns (loss, d s)."""
    m, H = s.shape
    n = t.shape[0]
    stu = torch.zeros(1, 1 + n, H, dtype=torch.float64, device=s.device)
    stu[0, 1:1 + m] = s.double()
    stu.requires_grad_(True)
    tea = torch.zeros(1, 1 + n, H, dtype=torch.float64, device=s.device)
    tea[0, 1:] = t.double()
    mask = torch.zeros(1, 1 + n, dtype=torch.bool, device=s.device)
    mask[0, 1:1 + m] = True
    loss = O.dcl_loss(stu, tea, mask, scale, ls)
    loss.backward()
    return loss.detach(), stu.grad[0, 1:1 + m]


def dcl_hip(s, t, scale, ls, block):
    """compute_dcl_loss's HIP branch on rows already in target order: l2_normalize -> dcl_loss.  Returns (loss, d s) and
    DclFn's own inputs and (loss, d s_n)."""
    ops = opsmod()
    si = s.clone().requires_grad_(True)
    s_n, t_n = ops.l2_normalize(si), ops.l2_normalize(t)
    s_n.retain_grad()
    loss = ops.dcl_loss(s_n, t_n, scale, ls, block)
    loss.backward()
    return (loss.detach(), si.grad), (s_n.detach(), t_n, s_n.grad)


def dcl_fn_ref(s_n, t_n, scale, ls):
    """What DclFn computes, in fp64 on the bf16 unit vectors it is given: the smoothed NLL of log_softmax(scale s_n t_n^T)
    with target(i) = i, and its gradient in s_n."""
    s64 = s_n.double().requires_grad_(True)
    sim = scale * s64 @ t_n.double().t()
    loss = O.smoothed_nll(F.log_softmax(sim, dim=-1), torch.arange(s_n.shape[0], device=sim.device), ls)
    loss.backward()
    return loss.detach(), s64.grad


def dcl_loss_bound(scale, H, m, n):
    """The kernels see bf16-rounded unit vectors (<= 2^-9 relative per entry, random-signed): each sim moves by
    ~scale 2^-8 / sqrt(H), each row loss by a few of those, and the mean over m independent rows by 1/sqrt(m) of that;
    plus the op's own 32 ulps of (scale + log n)."""
    return 4 * scale * 2.0 ** -8 / math.sqrt(H * m) + 32 * U32 * (scale + math.log(n) + 1)


def dcl_compare(s, t, scale, ls, block, what):
    """DclFn on its own inputs against dcl_fn_ref, and l2_normalize -> DclFn against O.dcl_loss on the raw features."""
    (loss, ds), (s_n, t_n, ds_n) = dcl_hip(s, t, scale, ls, block)
    rdev = ref_device(t.numel())
    m, H = s.shape
    n = t.shape[0]
    fl, fds = dcl_fn_ref(s_n.to(rdev), t_n.to(rdev), scale, ls)
    # DclFn loss: fp32 sims of bf16 unit vectors (~sqrt(H) u32 scale each) and the row op's 32 ulps of (scale + log n)
    # (measured: <= 0.03 of the bound)
    e1 = abs(float(loss) - float(fl))
    b1 = 4 * math.sqrt(H) * U32 * scale + 32 * U32 * (scale + math.log(n) + 1)
    assert e1 <= b1, "%s: DclFn loss err %.3e > %.3e" % (what, e1, b1)
    # d s_n: dsim rounded to bf16 before the GEMM, d s_n rounded to bf16 (util.BF16_*; measured: rel-fro <= 2.7e-3,
    # max-rel <= 5.4e-3)
    assert_close(ds_n, fds, what=what + " DclFn d s_n")
    rl, rds = dcl_oracle(s.to(rdev), t.to(rdev), scale, ls)
    el = abs(float(loss) - float(rl))
    bl = dcl_loss_bound(scale, H, m, n)
    assert el <= bl, "%s: loss err %.3e > %.3e" % (what, el, bl)  # (measured: <= 0.21 of the bound)
    # d s through the chain: five bf16 roundings (s_n, t_n, dsim, d s_n, the l2norm backward's dx) at RMS ~1.1e-3 each;
    # twice util.BF16_* (measured: rel-fro <= 3.9e-3, max-rel <= 8.2e-3)
    assert_close(ds, rds, fro=2 * BF16_FRO, mx=2 * BF16_MAX, what=what + " d student")


@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("block", [1, 7, 64])
@pytest.mark.parametrize("m,n,H", [(13, 61, 520), (61, 61, 768), (1, 61, 768), (1, 2, 64), (70, 203, 1536)])
def test_dcl_small_blocks(m, n, H, block, ls):
    """Several blocks with a short last one, targets offset by r0, n not a multiple of 8 (both GEMMs through the padding
    branches of gemm_any), m = n and m = 1."""
    s, t = dcl_features(m, n, H, seed=m * 1000 + n + H)
    dcl_compare(s, t, 2.5, ls, block, "m=%d n=%d H=%d block=%d ls=%g" % (m, n, H, block, ls))


@pytest.mark.parametrize("ls", [0.0, 0.1])
def test_dcl_one_full_block_and_one_row(ls):
    """m = 4097 at the default block: a full block of 4096 rows, then a 1-row block whose target is column 4096."""
    s, t = dcl_features(4097, 4100, 768, seed=4097)
    dcl_compare(s, t, 2.5, ls, 4096, "m=4097 n=4100 ls=%g" % ls)


def test_dcl_bench_shape():
    """bench.py --objective pretrain-vl's image term at b = 64: m = 12288, n = 16384, H = 1536, default block.  Against the
    fp64 oracle; the peak memory of DclFn stays at one block of sims (fp32 + its bf16 copy) plus d student and the
    transposed teacher, far below the m x n fp32 matrix; and blocks of 4096 / 1000 / m give the same gradient bits."""
    ops = opsmod()
    m, n, H = 12288, 16384, 1536
    s, t = dcl_features(m, n, H, seed=5)
    dcl_compare(s, t, 2.5, 0.0, 4096, "bench shape")
    s_n, t_n = ops.l2_normalize(s), ops.l2_normalize(t)
    sn = s_n.clone().requires_grad_(True)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = ops.dcl_loss(sn, t_n, 2.5, 0.0)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    full = m * n * 4
    block = 4096
    bound = block * n * (4 + 2) + m * H * 4 + n * H * 2 + block * H * (4 + 2) + (16 << 20)
    # (measured: 528 MiB of a 556 MiB bound; 632 MiB when the previous block's sims were still alive)
    assert grow <= bound < 0.75 * full, \
        "DclFn peak growth %.1f MiB (bound %.1f MiB, m x n fp32 %.1f MiB)" % (grow / 2**20, bound / 2**20, full / 2**20)
    (g0,) = torch.autograd.grad(loss, sn)
    for blk in (1000, m):
        sb = s_n.clone().requires_grad_(True)
        lb = ops.dcl_loss(sb, t_n, 2.5, 0.0, blk)
        (gb,) = torch.autograd.grad(lb, sb)
        # the row losses are summed in another grouping: a few fp32 ulps of the total (measured: 0 for 1000, 1 ulp for m)
        assert abs(float(lb.detach()) - float(loss.detach())) <= 64 * U32 * abs(float(loss.detach()))
        # each row's gradient comes from its own row op and GEMM rows that do not depend on the block: bit-identical
        assert torch.equal(gb, g0), "block %d" % blk


@pytest.mark.parametrize("ls", [0.0, 0.1])
@pytest.mark.parametrize("pad", [False, True])
def test_compute_dcl_loss_hip_branch(pad, ls):
    """criterions/pretrain.compute_dcl_loss on bf16 device features (HIP branch: masked rows gathered, the teacher permuted
    to [indices, rest]) against O.dcl_loss in fp64 with the same padding masks."""
    from one_peace_amd.criterions.pretrain import compute_dcl_loss
    B, L, H = 4, 58, 768
    g = dgen(31)
    tea = torch.randn(B, L, H, device=DEV, generator=g, dtype=torch.float64)
    stu = (tea + 2 * torch.randn(B, L, H, device=DEV, generator=g, dtype=torch.float64)).to(torch.bfloat16)
    tea = tea.to(torch.bfloat16)
    mask = torch.rand(B, L, device=DEV, generator=g) < 0.4
    mask[:, 0] = False
    pads = None
    if pad:
        lens = torch.tensor([57, 40, 23, 51], device=DEV)
        pads = torch.arange(L - 1, device=DEV)[None, :] >= lens[:, None]
        mask[:, 1:] &= ~pads
    si = stu.clone().requires_grad_(True)
    loss = compute_dcl_loss(si, tea, mask, 2.5, ls, pads)
    loss.backward()
    s64 = stu.double().requires_grad_(True)
    rl = O.dcl_loss(s64, tea.double(), mask, 2.5, ls, pads)
    rl.backward()
    n = int((~pads).sum()) if pad else B * (L - 1)  # 171 / 228 teacher tokens: not multiples of 8
    el = abs(float(loss.detach()) - float(rl.detach()))
    bl = dcl_loss_bound(2.5, H, int(mask.sum()), n)  # as dcl_compare
    assert el <= bl, "loss err %.3e > %.3e" % (el, bl)  # (measured: <= 0.36 of the bound)
    assert torch.equal(si.grad[~mask], torch.zeros_like(si.grad[~mask]))  # CLS, unmasked and padded tokens get none
    # as dcl_compare (measured: rel-fro 3.5e-3, max-rel 8.1e-3)
    assert_close(si.grad[mask], s64.grad[mask], fro=2 * BF16_FRO, mx=2 * BF16_MAX, what="compute_dcl_loss d student")
