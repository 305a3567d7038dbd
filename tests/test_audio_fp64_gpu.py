"""The fused first block of the audio feature extractor (csrc/audio.hip: op_audio_conv1_ln_gelu_fwd / _bwd) against fp64 on the SAME
inputs, PER ELEMENT, on every route of its row walk (tests/audio_ref.py: closed forms, derived budget, families, the mirror of a_grid,
the case list; checked on the CPU by tests/test_audio_ref_cpu.py).

Launches go through the C ABI, so that every output is the caller's: every input and output lives in a guarded buffer (the waveform holds
exactly stride (rows - 1) + 10 elements between NaN guards), every input is compared bit for bit with its host copy afterwards, and the
backward's workspace is filled with the fp32 NaN sentinel before every launch.  Every gate is |got - exact| <= R + E with the E of
tests/audio_ref.py; the reference is evaluated in fp64 on the device.  Each case is launched twice and must return the same bits
(neither kernel uses atomics).  Backward cases run on the reference's statistics rounded to fp32, so that the backward is tested on its
own; one chained case per family runs it on the forward kernel's.  Each case appends one line to audio_fp64_report.txt in the tests'
output directory: its id, grid, trips and per output the largest share |err| / (R + E), followed after the slash by the largest
(|err| - R) / E.  The Python wrappers are checked to return the bits of the C-ABI launch, rows = 0 is pinned both ways, and the audio
stem of one_peace_amd/audio_ops.py is checked, bit for bit, to keep the samples of a batch independent of each other."""
import os

import pytest
import torch

from tests import audio_ref as A
from tests.gemm_ref import SENTINEL
from tests.util import out_dir

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF, F32 = A.BF, A.F32
EPS = A.EPS


def hipmod():
    from one_peace_amd import hip
    return hip


def bits(t):
    return t.contiguous().view({BF: torch.int16, F32: torch.int32}[t.dtype])


def same(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def D(t):
    return A.to64(t, DEV)


def nan_ws(C):
    """The cached workspace of the wrappers, every word of it the fp32 NaN sentinel."""
    hip = hipmod()
    ws = hip.workspace(hip.lib().op_audio_conv1_ln_gelu_bwd_workspace_bytes(C), torch.device(DEV, torch.cuda.current_device()), "audio_conv1")
    ws.view(torch.int32).fill_(SENTINEL[F32][1])
    return ws


class Run:
    """The guarded device tensors of one test, its failures and its largest shares."""
    reported = False      # the first case of a session starts audio_fp64_report.txt afresh: one line per case

    def __init__(self, cid, route):
        self.cid, self.route, self.fails, self.sh, self.over = cid, route, [], {}, {}
        self.inputs, self.outputs = [], []

    def inp(self, host, dtype=BF):
        """A guarded (flat) device copy of a host tensor; compared with the host copy at the end."""
        if host is None:
            return None
        host = host.to(dtype).reshape(-1)
        v = A.guarded_from(host, dtype, device=DEV)
        self.inputs.append((v, host))
        return v

    def out(self, n, dtype, fill=None):
        v = A.guarded((n,), dtype, device=DEV)
        if fill is not None:
            v.copy_(fill.reshape(-1).to(DEV))
        self.outputs.append(v)
        return v

    def gate(self, got, exact, E, dtype, key):
        f, s, over = A.gate(got.view(exact.shape), exact, E, "bf16" if dtype == BF else "f32", key)
        self.fails += f
        self.sh[key] = max(self.sh.get(key, 0.0), s)
        self.over[key] = max(self.over.get(key, 0.0), over)
        # got must be non-finite exactly where the reference is
        self.require(torch.equal(torch.isfinite(got.view(exact.shape)), torch.isfinite(exact)), "%s: finite where the reference is not, or the reverse" % key)

    def require(self, ok, msg):
        if not ok:
            self.fails.append(msg)

    def finish(self):
        torch.cuda.synchronize()
        for v in self.outputs + [v for v, _ in self.inputs]:
            n = A.check_guard(v)
            self.require(n == 0, "%d guard elements overwritten around a buffer of %d" % (n, v.numel()))
        for v, host in self.inputs:
            self.require(torch.equal(bits(v.cpu()), bits(host)), "an input of %d elements changed" % v.numel())
        line = "%s route %s shares %s" % (self.cid, self.route, " ".join("%s=%.4f/%.3f" % (k, v, self.over[k]) for k, v in sorted(self.sh.items())) or "(bit for bit)")
        with open(os.path.join(out_dir(), "audio_fp64_report.txt"), "a" if Run.reported else "w") as f:   # (a fresh report per session)
            f.write(line + "\n")
        Run.reported = True
        print(line)
        assert not self.fails, "\n".join(self.fails[:12])
        assert all(s <= 1 for s in self.sh.values()), self.sh


class Dev:
    """The guarded device copies of an Inputs."""

    def __init__(self, run, r):
        self.wav, self.w0, self.b0, self.lnw, self.lnb, self.dy = (run.inp(t) for t in (r.wav, r.w0, r.b0, r.lnw, r.lnb, r.dy))


# ---- launches through the C ABI, every output given by the caller -------------------------------------------------------
def c_fwd(d, stride, y, mean, rstd, rows, C):
    hip = hipmod()
    hip._check(hip.lib().op_audio_conv1_ln_gelu_fwd(hip.ptr(d.wav), stride, hip.ptr(d.w0), hip.ptr(d.b0), hip.ptr(d.lnw), hip.ptr(d.lnb), hip.ptr(y),
                                                    hip.ptr(mean), hip.ptr(rstd), rows, C, EPS, hip.stream()), "op_audio_conv1_ln_gelu_fwd")


def c_bwd(d, stride, mean, rstd, outs, rows, C, accumulate):
    hip = hipmod()
    ws = nan_ws(C)
    hip._check(hip.lib().op_audio_conv1_ln_gelu_bwd(hip.ptr(d.dy), hip.ptr(d.wav), stride, hip.ptr(d.w0), hip.ptr(d.b0), hip.ptr(d.lnw), hip.ptr(d.lnb),
                                                    hip.ptr(mean), hip.ptr(rstd), hip.ptr(outs.get("dW0")), hip.ptr(outs.get("db0")),
                                                    hip.ptr(outs.get("dlnw")), hip.ptr(outs.get("dlnb")), hip.ptr(ws), rows, C, int(accumulate),
                                                    hip.stream()), "op_audio_conv1_ln_gelu_bwd")


def grad_outs(run, r):
    """The gradients the launch asks for, each holding its base (an overwriting launch must not let it through)."""
    return {k: run.out(r.base[k].numel(), BF, fill=r.base[k]) for k in r.wants}


def launch_fwd_twice(run, d, r):
    rows, C = r.rows, r.C
    got = []
    for _ in range(2):
        y, mean, rstd = run.out(rows * C, BF), run.out(rows, F32), run.out(rows, F32)
        c_fwd(d, r.stride, y, mean, rstd, rows, C)
        got.append((y, mean, rstd))
    run.require(all(same(a, b) for a, b in zip(*got)), "two forward launches differ")
    return got[0]


def launch_bwd_twice(run, d, r, mean, rstd, accumulate):
    got = []
    for _ in range(2):
        outs = grad_outs(run, r)
        c_bwd(d, r.stride, mean, rstd, outs, r.rows, r.C, accumulate)
        got.append(outs)
    run.require(all(same(got[0][k], got[1][k]) for k in r.wants), "two backward launches differ")
    return got[0]


# ---- every case: forward, then backward ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", A.CASES, ids=[c.id for c in A.CASES])
def test_audio_first_block(case):
    r = case.inputs()
    rows, C = r.rows, r.C
    run = Run(case.id, "grid=%d trips=%d" % (A.a_grid(rows), A.trips(rows)))
    d = Dev(run, r)
    y, mean, rstd = launch_fwd_twice(run, d, r)
    f = A.fwd_ref(D(r.wav), D(r.w0), D(r.b0), D(r.lnw), D(r.lnb), rows, r.stride, EPS, chain=case.family != "exact")
    run.gate(y, f["y"], f["E_y"], BF, "y")
    run.gate(mean, f["mean"], f["E_mean"], F32, "mean")
    run.gate(rstd, f["rstd"], f["E_rstd"], F32, "rstd")
    if case.family == "exact" and C & (C - 1) == 0:
        run.require(torch.equal(mean.double(), f["mean"]), "the mean of the exact family is not exact")
    if case.family == "nonfinite":
        touched = A.touched_rows(f["S"])
        run.require(int(touched.sum()) == 4 and torch.equal(~torch.isfinite(y.view(rows, C)).any(1), touched), "non-finite rows: not exactly the four touched")
    if case.family == "silence" and not case.bias:
        sil = A.silent_rows(f["S"])
        want = A.bf(A.gelu_erf(torch.zeros(C, dtype=torch.float64, device=DEV) if r.lnb is None else D(r.lnb)))
        run.require(int(sil.sum()) > 0 and torch.equal(y.view(rows, C)[sil].double(), want.expand(int(sil.sum()), C)), "silent rows: y != bf(gelu(lnb))")
    # backward: on the reference's statistics as fp32 numbers, or (chained) on the forward kernel's own
    if case.chained:
        mean_in, rstd_in = mean, rstd
    else:
        mean_in, rstd_in = run.inp(f["mean"].float().cpu(), F32), run.inp(f["rstd"].float().cpu(), F32)
    ref = A.bwd_ref(D(r.dy), f["S"], f["v"], D(r.lnw), D(r.lnb), mean_in.double(), rstd_in.double(), case.bias, D(r.base) if case.accumulate else None)
    got = launch_bwd_twice(run, d, r, mean_in, rstd_in, case.accumulate)
    assert set(got) == set(A.wanted(case.bias, case.affine))
    for k, g in got.items():
        run.gate(g, ref[k][0], ref[k][1], BF, k)
    run.finish()


# ---- the Python wrappers return the bits of the C-ABI launch ------------------------------------------------------------
def test_wrappers_return_the_c_abi_bits():
    hip = hipmod()
    run = Run("wrappers", "-")
    for bias, affine in ((True, "both"), (False, "none")):
        r = A.make_inputs("unit", 1030, 264, 5, bias, affine)
        rows, C = r.rows, r.C
        d = Dev(run, r)
        t = {k: (None if getattr(r, k) is None else getattr(r, k).to(BF).to(DEV)) for k in ("wav", "w0", "b0", "lnw", "lnb", "dy")}
        y, mean, rstd = launch_fwd_twice(run, d, r)
        wy, wmean, wrstd = hip.audio_conv1_ln_gelu_fwd(t["wav"], 5, t["w0"], t["b0"], t["lnw"], t["lnb"], rows, EPS, slack_rows=2)
        run.require(tuple(wy.shape) == (rows + 2, C) and same(wy[:rows].reshape(-1), y) and same(wmean, mean) and same(wrstd, rstd), "hip.audio_conv1_ln_gelu_fwd")
        run.require(bool((bits(wy[rows:]) == 0).all()), "slack_rows: the rows after the last are not zero")
        wy0 = hip.audio_conv1_ln_gelu_fwd(t["wav"], 5, t["w0"], t["b0"], t["lnw"], t["lnb"], rows, EPS)[0]
        run.require(tuple(wy0.shape) == (rows, C) and same(wy0.reshape(-1), y), "hip.audio_conv1_ln_gelu_fwd without slack rows")
        for acc in (False, True):
            got = launch_bwd_twice(run, d, r, mean, rstd, acc)
            if acc:
                mine = tuple(r.base[k].to(BF).to(DEV) if k in r.wants else None for k in A.OUTPUTS)
                w = hip.audio_conv1_ln_gelu_bwd(t["dy"].view(rows, C), t["wav"], 5, t["w0"], t["b0"], t["lnw"], t["lnb"], wmean, wrstd, accumulate=True, out=mine)
                run.require(all(a is b for a, b in zip(w, mine)), "hip.audio_conv1_ln_gelu_bwd: out= tensors not returned")
            else:
                w = hip.audio_conv1_ln_gelu_bwd(t["dy"].view(rows, C), t["wav"], 5, t["w0"], t["b0"], t["lnw"], t["lnb"], wmean, wrstd)
            for k, wt in zip(A.OUTPUTS, w):
                run.require((wt is None) == (k not in r.wants), "hip.audio_conv1_ln_gelu_bwd: %s given / missing" % k)
                if wt is not None:
                    run.require(same(wt.reshape(-1), got[k]), "hip.audio_conv1_ln_gelu_bwd (accumulate=%d): %s" % (acc, k))
    run.finish()


# ---- rows = 0 -------------------------------------------------------------------------------------------------------------
def test_zero_rows():
    """No rows: the forward writes nothing, the backward's sums are zero -- non-accumulating gradients come back as zeros, accumulating ones
    untouched -- at the C ABI with valid pointers, and through the wrappers with empty tensors (whose address is null)."""
    hip = hipmod()
    r = A.make_inputs("unit", 3, 64, 5, True, "both")
    C = r.C
    run = Run("rows0", "-")
    d = Dev(run, r)
    y, mean, rstd = run.out(3 * C, BF, fill=r.dy), run.out(3, F32, fill=r.base["db0"][:3]), run.out(3, F32, fill=r.base["db0"][:3])
    c_fwd(d, 5, y, mean, rstd, 0, C)
    run.require(same(y, r.dy.to(BF).to(DEV).reshape(-1)) and same(mean, r.base["db0"][:3].to(DEV)) and same(rstd, mean), "op_audio_conv1_ln_gelu_fwd, rows = 0: wrote")
    for acc in (False, True):
        outs = grad_outs(run, r)
        c_bwd(d, 5, mean, rstd, outs, 0, C, acc)
        for k, g in outs.items():
            want = r.base[k].to(BF).to(DEV).reshape(-1) if acc else torch.zeros(g.numel(), dtype=BF, device=DEV)
            run.require(same(g, want), "op_audio_conv1_ln_gelu_bwd, rows = 0, accumulate=%d: %s" % (acc, k))
        some = {k: v for k, v in grad_outs(run, r).items() if k in ("dW0", "dlnw")}      # (null db0 / dlnb)
        c_bwd(d, 5, mean, rstd, some, 0, C, acc)
        run.require(all(same(g, r.base[k].to(BF).to(DEV).reshape(-1) if acc else torch.zeros_like(g)) for k, g in some.items()), "rows = 0 with null outputs")
    # the wrappers, on empty tensors
    t = {k: getattr(r, k).to(BF).to(DEV) for k in ("wav", "w0", "b0", "lnw", "lnb")}
    wy, wmean, wrstd = hip.audio_conv1_ln_gelu_fwd(t["wav"], 5, t["w0"], t["b0"], t["lnw"], t["lnb"], 0, EPS, slack_rows=2)
    run.require(tuple(wy.shape) == (2, C) and bool((bits(wy) == 0).all()) and wmean.numel() == 0 and wrstd.numel() == 0, "hip.audio_conv1_ln_gelu_fwd, rows = 0")
    wy, _, _ = hip.audio_conv1_ln_gelu_fwd(t["wav"][:0], 5, t["w0"], None, None, None, 0, EPS)
    run.require(tuple(wy.shape) == (0, C), "hip.audio_conv1_ln_gelu_fwd on an empty waveform")
    e2 = torch.empty(0, C, dtype=BF, device=DEV)
    w = hip.audio_conv1_ln_gelu_bwd(e2, t["wav"], 5, t["w0"], t["b0"], t["lnw"], t["lnb"], wmean, wrstd)
    run.require(tuple(w[0].shape) == (C, 10) and all(bool((bits(g) == 0).all()) for g in w), "hip.audio_conv1_ln_gelu_bwd on an empty dy")
    mine = tuple(r.base[k].to(BF).to(DEV) for k in A.OUTPUTS)
    hip.audio_conv1_ln_gelu_bwd(e2, t["wav"][:0], 5, t["w0"], t["b0"], t["lnw"], t["lnb"], wmean, wrstd, accumulate=True, out=mine)
    run.require(all(same(g, r.base[k].to(BF).to(DEV)) for k, g in zip(A.OUTPUTS, mine)), "hip.audio_conv1_ln_gelu_bwd on an empty dy, accumulate")
    run.finish()


# ---- the stem keeps the samples of a batch apart (one_peace_amd/audio_ops.py: the "garbage rows") ---------------------------
def _extractor(m, wv, grad=True):
    from one_peace_amd import audio_ops
    m.zero_grad()
    with torch.enable_grad() if grad else torch.no_grad():
        o = audio_ops.feature_extractor(wv, m.conv_layers)
        if grad:
            o[0].float().square().sum().backward()     # a loss that touches sample 0's frames only
    return o.detach().clone(), ({n: p.grad.detach().clone() for n, p in m.named_parameters()} if grad else None)


def test_feature_extractor_keeps_samples_independent():
    """The last slots of a sample are computed from its neighbour; no valid frame may read them and they must get zero gradient.  Bit
    comparisons: replacing sample 1's waveform leaves the frames of samples 0 and 2, and every parameter gradient of a loss on sample 0,
    as they were; a NaN waveform in sample 1 leaves them finite and unchanged."""
    from one_peace_amd.adapter.audio import ConvFeatureExtractionModel
    torch.manual_seed(0)
    spec = [(64, 10, 5)] + [(64, 3, 2)] * 4 + [(64, 2, 2)] * 2
    m = ConvFeatureExtractionModel(spec).to(DEV).to(BF)
    g = torch.Generator().manual_seed(11)
    wv = torch.randn(3, 4000, generator=g).to(BF).to(DEV)
    wv[2] *= 0.25     # (different valid content per sample)
    other, nan = wv.clone(), wv.clone()
    other[1] = (3 * torch.randn(4000, generator=g)).to(BF).to(DEV)
    nan[1] = float("nan")
    o, grads = _extractor(m, wv)
    assert o.shape[0] == 3 and bool(torch.isfinite(o.float()).all())
    o_again, grads_again = _extractor(m, wv)
    assert same(o, o_again) and all(same(grads[n], grads_again[n]) for n in grads), "the extractor is not reproducible on the same input"
    o2, grads2 = _extractor(m, other)
    assert not same(o[1], o2[1])
    for b in (0, 2):
        assert same(o[b], o2[b]), "sample %d's frames changed with sample 1's waveform" % b
    for n in grads:
        assert bool(torch.isfinite(grads[n].float()).all()) and float(grads[n].float().abs().max()) > 0, n
        assert same(grads[n], grads2[n]), "the gradient of %s (loss on sample 0) changed with sample 1's waveform" % n
    o3, _ = _extractor(m, nan, grad=False)
    for b in (0, 2):
        assert bool(torch.isfinite(o3[b].float()).all()) and same(o[b], o3[b]), "sample %d's frames changed with a NaN waveform in sample 1" % b


@pytest.mark.parametrize("T", [46, 37])
def test_grouped_conv_keeps_samples_independent(T):
    from one_peace_amd import audio_ops
    B, C, G, k = 3, 128, 4, 19
    g = torch.Generator().manual_seed(12 + T)
    rn = lambda *s: torch.randn(*s, generator=g).to(BF).to(DEV)  # noqa: E731
    x, dy, w, b = rn(B, T, C), rn(B, T, C), (rn(C, C // G, k) * (C // G * k) ** -0.5).to(BF), rn(C)
    res = []
    for variant in ("base", "base", "other", "nan"):
        xv, dyv = x.clone(), dy.clone()
        if variant == "other":
            xv[1], dyv[1] = rn(T, C), rn(T, C)
        elif variant == "nan":
            xv[1], dyv[1] = float("nan"), float("nan")
        xv.requires_grad_(True)
        y = audio_ops.grouped_conv1d_same(xv, w, b, G)
        y.backward(dyv)
        res.append((y.detach().clone(), xv.grad.detach().clone()))
    (y0, dx0), (y1, dx1) = res[0], res[1]
    assert same(y0, y1) and same(dx0, dx1), "grouped_conv1d_same is not reproducible on the same input"
    assert bool(torch.isfinite(y0.float()).all()) and bool(torch.isfinite(dx0.float()).all())
    for variant, (y2, dx2) in zip(("other", "nan"), res[2:]):
        assert not same(y0[1], y2[1])
        for s in (0, 2):
            assert same(y0[s], y2[s]), "%s: sample %d's output rows changed with sample 1" % (variant, s)
            assert same(dx0[s], dx2[s]), "%s: sample %d's dx changed with sample 1" % (variant, s)
