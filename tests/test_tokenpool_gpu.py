"""op_token_mean_ln_fwd / op_token_mean_ln_bwd (csrc/tokenpool.hip) on the MI355X against the fp64 restatement and the derived
per-element budget of tests/tokenpool_ref.py: every output of every shape, dense and as a strided view; the CLS row never read and
written as zeros; guard elements untouched; two runs and two batch sizes bit for bit; NULL arguments; the limits; the autograd route
of ops.token_mean_norm.  The largest observed / allowed ratio per output goes to tokenpool_fp64_report.txt in the tests' output
directory (tests/util.py: OUT).

MEASURED on the MI355X (profiles/tokenpool_fp64_report.txt, one line per case of the first test): largest ratio 0.998 for y and dx (bf16
outputs: a rounding next to a midpoint), 0.60 for dw_part, 0.02 for rstd, 0.07 for pooled, 0.002 for mean, below 0.001 for db_part."""
import ctypes
import os

import pytest
import torch

from tests import tokenpool_ref as T
from tests.util import OUT

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 1e-5
REPORT = os.path.join(OUT, "tokenpool_fp64_report.txt")
# (B, S, H): a single patch token; H no multiple of the 64-lane footprint; two splits' worth at the model's H; every split in use;
# the last split partly filled; more than one round of 16 staged samples in the dw / db kernel with the last round partly filled;
# two column passes per lane with the second partly filled (H = 2056 > 2048); all four column passes (H = 8192)
SHAPES = [(1, 2, 8), (3, 17, 72), (2, 257, 1536), (2, 1025, 1536), (5, 130, 264), (37, 3, 72), (1, 3, 2056), (2, 5, 8192)]
_cache = {}
_report_started = []


def _hip():
    from one_peace_amd import hip
    return hip


def _case(shape):
    """Inputs and fp64 references of a shape, computed once and left unchanged."""
    if shape not in _cache:
        B, S, H = shape
        x, dy, w, b = T.make_inputs(B, S, H)
        _cache[shape] = dict(x=x, dy=dy, w=w, b=b, fwd=T.forward_ref(x, w, b, EPS))
    return _cache[shape]


def _dev(t, dtype=torch.bfloat16):
    return None if t is None else t.to(dtype).to(DEV)


def _x_on_device(x, strided):
    if not strided:
        return _dev(x).contiguous(), None, None
    B, S, H = x.shape
    view, whole, mask = T.guarded3(B, S, H, torch.bfloat16, DEV)
    view.copy_(_dev(x))
    return view, whole, mask


def _report(lines):
    os.makedirs(os.path.dirname(REPORT), exist_ok=True)
    with open(REPORT, "a" if _report_started else "w") as f:   # one report per session, not one per suite run ever made
        _report_started.append(True)
        for line in lines:
            f.write(line + "\n")


def _run(shape, strided, x=None, w="case", b="case", dx_fill=None):
    """Forward and backward of one case through the ctypes wrappers.  Returns the outputs (device tensors) and the dx guard."""
    hip = _hip()
    c = _case(shape)
    B, S, H = shape
    xd, whole, mask = _x_on_device(c["x"] if x is None else x, strided)
    wd = _dev(c["w"]) if isinstance(w, str) else w
    bd = _dev(c["b"]) if isinstance(b, str) else b
    y, pooled, mean, rstd = hip.token_mean_ln_fwd(xd, wd, bd, EPS)
    if strided:
        dx, dwhole, dmask = T.guarded3(B, S, H, torch.bfloat16, DEV)
    else:
        dx, dwhole, dmask = torch.empty(B, S, H, dtype=torch.bfloat16, device=DEV), None, None
    if dx_fill is not None:
        dx.fill_(dx_fill)
    _, dw, db = hip.token_mean_ln_bwd(_dev(c["dy"]), pooled, wd, mean, rstd, S, dx=dx)
    torch.cuda.synchronize()
    guards = (T.guard_touched(whole, mask) if strided else 0, T.guard_touched(dwhole, dmask) if strided else 0)
    return dict(y=y, pooled=pooled, mean=mean, rstd=rstd, dx=dx, dw_part=dw, db_part=db), guards


@pytest.mark.parametrize("strided", [False, True], ids=["dense", "view"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_output_is_within_the_derived_budget_of_fp64(shape, strided):
    c = _case(shape)
    out, guards = _run(shape, strided, dx_fill=float("nan"))
    # the backward's reference starts from the STORED fp32 pooled / mean / rstd: they are inputs of that entry
    bwd = T.backward_ref(c["dy"], out["pooled"].double().cpu(), c["w"], out["mean"].double().cpu(), out["rstd"].double().cpu(), shape[1])
    refs = dict(c["fwd"], **bwd)
    shares = {k: T.share(out[k], refs[k]) for k in ("y", "pooled", "mean", "rstd", "dx", "dw_part", "db_part")}
    line = "%-14s %-5s " % ("x".join(map(str, shape)), "view" if strided else "dense") + "  ".join("%s %.3f" % kv for kv in shares.items())
    print(line)
    _report([line])
    assert all(v <= 1.0 for v in shares.values()), shares
    assert guards == (0, 0), "guard elements of x / dx changed: %s" % (guards,)
    dx = out["dx"]
    assert not bool(torch.isnan(dx.float()).any()), "a pre-filled NaN survived inside dx"
    assert bool((dx[:, 0, :].view(torch.int16) == 0).all()), "the CLS row of dx must be +0"
    assert bool((dx[:, 1:, :] == dx[:, 1:2, :]).all()), "every token row of dx holds the same value"


@pytest.mark.parametrize("shape", [(3, 17, 72), (2, 257, 1536)], ids=lambda s: "x".join(map(str, s)))
def test_the_cls_row_is_never_read(shape):
    c = _case(shape)
    clean, _ = _run(shape, False)
    poisoned = c["x"].clone()
    poisoned[:, 0, :] = float("nan")
    got, _ = _run(shape, False, x=poisoned)
    for k in clean:
        assert bool(torch.isfinite(got[k].float()).all()), k
        assert torch.equal(got[k].view(torch.int16 if got[k].dtype == torch.bfloat16 else torch.int32),
                           clean[k].view(torch.int16 if clean[k].dtype == torch.bfloat16 else torch.int32)), k


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize("shape", [(2, 1025, 1536), (37, 3, 72)], ids=lambda s: "x".join(map(str, s)))
def test_two_runs_give_identical_bits(shape):
    a, _ = _run(shape, True)
    b, _ = _run(shape, True)
    for k in a:
        assert torch.equal(_bits(a[k]), _bits(b[k])), k


def test_parts_alone_without_dx():
    """dx NULL: the entry computes dw_part / db_part only, with the bits of the full call."""
    hip = _hip()
    shape = (37, 3, 72)
    c = _case(shape)
    full, _ = _run(shape, False)
    dy, w = _dev(c["dy"]), _dev(c["w"])
    dx, dw, db = hip.token_mean_ln_bwd(dy, full["pooled"], w, full["mean"], full["rstd"], shape[1], want_dx=False)
    torch.cuda.synchronize()
    assert dx is None
    assert torch.equal(_bits(dw), _bits(full["dw_part"])) and torch.equal(_bits(db), _bits(full["db_part"]))


def test_a_samples_bits_do_not_depend_on_the_batch():
    hip = _hip()
    shape = (5, 130, 264)
    c = _case(shape)
    full, _ = _run(shape, False)
    x0, dy0 = _dev(c["x"][:1]).contiguous(), _dev(c["dy"][:1]).contiguous()
    w, b = _dev(c["w"]), _dev(c["b"])
    y, pooled, mean, rstd = hip.token_mean_ln_fwd(x0, w, b, EPS)
    dx, _, _ = hip.token_mean_ln_bwd(dy0, pooled, w, mean, rstd, shape[1], want_parts=False)
    torch.cuda.synchronize()
    for k, v in (("y", y), ("pooled", pooled), ("mean", mean), ("rstd", rstd), ("dx", dx)):
        assert torch.equal(_bits(v), _bits(full[k][:1])), k


def test_null_weight_bias_and_parts():
    hip = _hip()
    shape = (3, 17, 72)
    c = _case(shape)
    B, S, H = shape
    x = _dev(c["x"]).contiguous()
    y, pooled, mean, rstd = hip.token_mean_ln_fwd(x, None, None, EPS)
    dx, dw, db = hip.token_mean_ln_bwd(_dev(c["dy"]), pooled, None, mean, rstd, S, want_parts=False)
    torch.cuda.synchronize()
    assert dw is None and db is None
    fwd = T.forward_ref(c["x"], None, None, EPS)
    bwd = T.backward_ref(c["dy"], pooled.double().cpu(), None, mean.double().cpu(), rstd.double().cpu(), S)
    shares = {"y": T.share(y, fwd["y"]), "pooled": T.share(pooled, fwd["pooled"]), "dx": T.share(dx, bwd["dx"])}
    assert all(v <= 1.0 for v in shares.values()), shares
    # the weight alone, and one of the two parts alone
    y2, pooled2, mean2, rstd2 = hip.token_mean_ln_fwd(x, _dev(c["w"]), None, EPS)
    only_db = torch.empty(H, dtype=torch.float32, device=DEV)
    L = hip.lib()
    dx2 = torch.empty(B, S, H, dtype=torch.bfloat16, device=DEV)
    dy_d, w_d = _dev(c["dy"]), _dev(c["w"])   # (named: a raw pointer keeps no tensor alive)
    rc = L.op_token_mean_ln_bwd(hip.ptr(dy_d), hip.ptr(pooled2), hip.ptr(w_d), hip.ptr(mean2), hip.ptr(rstd2), hip.ptr(dx2),
                                H, S * H, None, hip.ptr(only_db), B, S, H, hip.stream())
    torch.cuda.synchronize()
    assert rc == 0
    bwd2 = T.backward_ref(c["dy"], pooled2.double().cpu(), c["w"], mean2.double().cpu(), rstd2.double().cpu(), S)
    assert T.share(only_db, bwd2["db_part"]) <= 1.0 and T.share(dx2, bwd2["dx"]) <= 1.0
    assert T.share(y2, T.forward_ref(c["x"], c["w"], None, EPS)["y"]) <= 1.0


def test_limit_violations_return_einval_and_touch_nothing():
    hip = _hip()
    L = hip.lib()
    B, S, H = 2, 9, 64
    x = torch.zeros(B, S, H + 8, dtype=torch.bfloat16, device=DEV)
    w = torch.ones(H + 8, dtype=torch.bfloat16, device=DEV)
    f32 = lambda *s: torch.full(s, 7.0, dtype=torch.float32, device=DEV)  # noqa: E731
    y = torch.full((B, H), 7.0, dtype=torch.bfloat16, device=DEV)
    pooled, mean, rstd, part = f32(B, H), f32(B), f32(B), f32(B * 16 * H)
    dx = torch.full((B, S, H + 8), 7.0, dtype=torch.bfloat16, device=DEV)
    dwp, dbp = f32(H), f32(H)
    P, off = hip.ptr, lambda t, n: ctypes.c_void_p(t.data_ptr() + n)  # noqa: E731

    def fwd(x_=None, ld=H + 8, bs=S * (H + 8), w_=None, S_=S, H_=H, B_=B, eps=EPS):
        return L.op_token_mean_ln_fwd(x_ or P(x), ld, bs, w_ or P(w), P(w), eps, P(y), P(pooled), P(mean), P(rstd), P(part), B_, S_, H_,
                                      hip.stream())

    def bwd(ldg=H + 8, bsg=S * (H + 8), dx_=None, S_=S, H_=H, B_=B):
        return L.op_token_mean_ln_bwd(P(y), P(pooled), P(w), P(mean), P(rstd), dx_ or P(dx), ldg, bsg, P(dwp), P(dbp), B_, S_, H_,
                                      hip.stream())

    bad = [fwd(H_=60), fwd(H_=0), fwd(H_=8200, ld=8200), fwd(S_=1), fwd(S_=65537), fwd(ld=H - 8), fwd(ld=H + 4), fwd(bs=S * (H + 8) + 4),
           fwd(bs=-8), fwd(x_=off(x, 2)), fwd(w_=off(w, 2)), fwd(B_=-1), fwd(eps=-1.0),
           bwd(H_=60), bwd(S_=1), bwd(ldg=H - 8), bwd(ldg=H + 4), bwd(bsg=(S - 1) * (H + 8)), bwd(dx_=off(dx, 2)), bwd(B_=-1)]
    torch.cuda.synchronize()
    assert all(rc == -22 for rc in bad), bad
    assert L.op_last_error()
    for t in (y, pooled, mean, rstd, dx, dwp, dbp):
        assert bool((t == 7.0).all()), "an output was written by a refused call"
    assert fwd(B_=0) == 0 and bwd(B_=0) == 0  # returns without a launch
    torch.cuda.synchronize()
    assert bool((y == 7.0).all()) and bool((dx == 7.0).all())


@pytest.mark.parametrize("shape", [(3, 17, 72), (2, 257, 1536)], ids=lambda s: "x".join(map(str, s)))
def test_autograd_route_matches_the_torch_statement(shape):
    from one_peace_amd import ops
    hip = _hip()
    c = _case(shape)
    B, S, H = shape
    calls = []
    fwd, bwd = hip.token_mean_ln_fwd, hip.token_mean_ln_bwd
    hip.token_mean_ln_fwd = lambda *a, **k: calls.append("fwd") or fwd(*a, **k)
    hip.token_mean_ln_bwd = lambda *a, **k: calls.append("bwd") or bwd(*a, **k)
    try:
        x = _dev(c["x"]).requires_grad_(True)
        w, b = _dev(c["w"]).requires_grad_(True), _dev(c["b"]).requires_grad_(True)
        y = ops.token_mean_norm(x, w, b, EPS)
        y.backward(_dev(c["dy"]))
        torch.cuda.synchronize()
    finally:
        hip.token_mean_ln_fwd, hip.token_mean_ln_bwd = fwd, bwd
    assert calls == ["fwd", "bwd"]
    # the torch statement in fp64 on the same bf16 values
    x64, w64, b64 = (t.clone().requires_grad_(True) for t in (c["x"], c["w"], c["b"]))
    ops.token_mean_norm_torch(x64, w64, b64, EPS).backward(c["dy"])
    f = c["fwd"]
    err = (f["pooled"][2], f["mean"][2], f["rstd"][2])
    ref = T.backward_ref(c["dy"], f["pooled"][0], c["w"], f["mean"][0], f["rstd"][0], S, fwd_err=err)
    assert float((ref["dx"][0] - x64.grad).abs().max()) <= 1e-12 and float((ref["dw_part"][0] - w64.grad).abs().max()) <= 1e-10
    dw_exact, _, E_dw = ref["dw_part"]
    db_exact, _, E_db = ref["db_part"]
    shares = {"y": T.share(y, f["y"]), "dx": T.share(x.grad, ref["dx"]),
              "dweight": T.share(w.grad, (dw_exact, T.half_ulp_bf16(dw_exact.abs() + E_dw), E_dw)),
              "dbias": T.share(b.grad, (db_exact, T.half_ulp_bf16(db_exact.abs() + E_db), E_db))}
    print(shape, shares)
    assert all(v <= 1.0 for v in shares.values()), shares
    assert w.grad.dtype == torch.bfloat16 and b.grad.dtype == torch.bfloat16


def test_fp32_input_takes_the_torch_route():
    from one_peace_amd import ops
    hip = _hip()
    x = torch.randn(2, 9, 64, device=DEV, requires_grad=True)
    w, b = torch.ones(64, device=DEV), torch.zeros(64, device=DEV)
    fwd = hip.token_mean_ln_fwd
    hip.token_mean_ln_fwd = lambda *a, **k: (_ for _ in ()).throw(AssertionError("the HIP route ran for fp32"))
    try:
        y = ops.token_mean_norm(x, w, b, EPS)
        odd = ops.token_mean_norm(torch.randn(2, 9, 60, device=DEV, dtype=torch.bfloat16), None, None, EPS)   # H % 8 != 0
    finally:
        hip.token_mean_ln_fwd = fwd
    assert y.dtype == torch.float32 and torch.equal(y, ops.token_mean_norm_torch(x, w, b, EPS)) and tuple(odd.shape) == (2, 60)
