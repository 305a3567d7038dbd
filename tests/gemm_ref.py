"""Shared by tests/test_gemm_ref_cpu.py and tests/test_gemm_fp64_gpu.py: the GEMM family of csrc/gemm.hip in fp64 (every epilogue,
the transpose-read weight gradient with and without accumulation, the grouped launch's side product), the per-element error budget,
the seeded input families, guarded buffers, the mirror of the launch routes, the NT case list, and mutants of the fp64 computation
(one per class of subtle kernel bug).  Nothing here needs a GPU: everything runs on whatever device its inputs live on.

Every input holds bf16 VALUES (built in fp32, rounded to bf16, upcast), so the reference and a kernel see the same numbers.

The gate is per element, no norms:

    |got - exact|  <=  R + C_ACC * 2^-24 * T        (+ C_GELU * 2^-24 * max(|h0|, |gelu(h0)|) * |h1| for the GeGLU product)

exact: the output in fp64.  T: its MAGNITUDE SUM, the same formula with every term replaced by its absolute value (sum |a||w| +
|bias| for the bias epilogue; |resid| + |rowscale * gamma| * T_y for the residual one; through |gelu'| for the GeGLU product) --
what an fp32 ulp of the kernel's running sums is measured against.  R: the ONE rounding the kernel documents for that output --
half a bf16 ulp at |exact| for a bf16 output (at |exact| + the fp32 allowance: the neighbouring binade at a binade edge), nothing
for an fp32 output or a split-K slab.  The residual output is rounded once (y stays fp32 into the layer scale), h0 / h1 have their
own half ulp, an accumulating weight gradient rounds base + product once on both of its routes."""
import math

import torch

U32 = 2.0 ** -24   # fp32 unit roundoff
EPI_BIAS, EPI_F32, EPI_GEGLU, EPI_RESID = 0, 1, 2, 3
EPI_NAMES = {EPI_BIAS: "bias", EPI_F32: "f32", EPI_GEGLU: "geglu", EPI_RESID: "resid"}

# C_ACC / C_GELU = MARGIN x the largest ratio measured on the MI355X (profiles/gemm_fp64_errors_mi355x.jsonl, one line per case of
# tests/test_gemm_fp64_gpu.py); the factor 2 covers the order of the fp32 sums, which changes with the route and the CU count.
#   "acc":  max |got - exact| / (2^-24 T) over every fp32 output: the EPI_F32 cases and the split-K slabs read back from the scratch.
#   "gelu": max (|got - exact| - R) / (2^-24 max(|h0|, |gelu(h0)|) |h1|) over the GeGLU products of the `integer` and `basis`
#           families, whose accumulators are exact: what exceeds the output rounding there is the device's erf alone (csrc/common.h:
#           Abramowitz-Stegun 7.1.26, |error| <= 1.5e-7 = 2.5 x 2^-24 on erfc, plus __expf and the reciprocal).  The excess shows
#           where the fp32 value crosses a bf16 rounding midpoint: a few dozen of the ~10^6 elements of those cases.
# CONDITION (not a measurement): C_ACC <= 16.  At 16 the fp32 allowance of the `unit` family at K <= 1536 is below 2 % of the bf16
# half ulp: an error of one ulp cannot pass.  tests/test_gemm_ref_cpu.py checks the condition and that every mutant below fails.
#
# UNMEASURED: no MI355X run of tests/test_gemm_fp64_gpu.py has been made, and profiles/gemm_fp64_errors_mi355x.jsonl does not exist yet.
# Both figures below are the CPU STAND-IN's (torch's fp32 matmul of the same operands, the epilogue and torch.erf in fp32; measured by
# tests/test_gemm_ref_cpu.py::test_constants): "acc" 1.54 at K = 64 (0.17 - 0.52 at K = 1536, 6144); "gelu" 2.09 = the error of the
# stand-in's fp32 GeGLU product before its rounding, over 2^-24 max(|h0|, |gelu(h0)|) |h1|, on `integer` and `basis`.  The device's
# erf is an approximation with a larger error than torch.erf: GeGLU cases may miss the gate until "gelu" is measured on the device.
# The MI355X run replaces both with the record's maxima, commits the record and sets MEASURED_ON_MI355X (test_constants then requires
# the equality).
MEASURED_ON_MI355X = False
MEASURED_MAX_RATIO = {"acc": 1.54, "gelu": 2.09}
MARGIN = 2.0
C_ACC = MARGIN * MEASURED_MAX_RATIO["acc"]
C_GELU = MARGIN * MEASURED_MAX_RATIO["gelu"]


def bf(x):
    """Round to bf16 and back: ONE round-to-nearest-even, also from fp64 (torch converts fp64 through fp32: a value that fp32 rounds
    onto a bf16 tie would be rounded twice -- such an fp32 value is moved one ulp back towards x first)."""
    if x.dtype != torch.float64:
        return x.to(torch.bfloat16).to(x.dtype)
    f = x.float()
    b = f.view(torch.int32)
    d = x - f.double()
    tie = ((b & 0xFFFF) == 0x8000) & (d != 0) & torch.isfinite(f)
    away = (d > 0) == (f > 0)
    b = b + (tie & away).int() - (tie & ~away).int()
    return b.view(torch.float32).to(torch.bfloat16).double()


def cdiv(a, b):
    return (a + b - 1) // b


def gelu_erf(x):
    """x Phi(x) through erfc (no cancellation at very negative x)."""
    return 0.5 * x * torch.special.erfc(-x * (1.0 / math.sqrt(2.0)))


def gelu_erf_grad(x):
    return 0.5 * torch.special.erfc(-x * (1.0 / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) * (1.0 / math.sqrt(2.0 * math.pi))


# ----------------------------------------------------------------------------------------------------------------------
# exact results (fp64) with their magnitude sums; the rounding model; the mutants
# ----------------------------------------------------------------------------------------------------------------------
MUTANTS = ("drop_last_kstep", "bias_twice_in_fold", "y_rounded_before_layer_scale", "slab_rounded_bf16", "accumulate_double_round",
           "geglu_halves_swapped", "tail_rowscale_without_m_off", "second_half_store_past_N", "segment_bias_of_neighbour")


def _acc(A, W, mutant=None, splits=None):
    """A W^T and |A| |W|^T in fp64.  splits: [(k0, k1)] K-ranges of split-K slabs."""
    acc = A @ W.t()
    if mutant == "drop_last_kstep":   # the last 32-deep k-step missing in one 16 x 16 block of accumulators
        K = A.shape[1]
        acc = acc.clone()
        acc[:16, :16] -= A[:16, K - 32:] @ W[:16, K - 32:].t()
    if mutant == "slab_rounded_bf16":
        acc = sum(bf(A[:, k0:k1] @ W[:, k0:k1].t()) for k0, k1 in splits)
    return acc, A.abs() @ W.abs().t()


def nt_ref(op, model=False, mutant=None):
    """One NT launch.  op: dict with A [M, K], Ws (1-3 [n_seg, K] weights; GeGLU: [W0, W1]), biases (list, entries may be None), epi,
    and where they apply alpha (float), resid [M, N] ([rows_total, N] with a row table), gamma [N] | None, rowscale (fp32 values)
    | None, rps (rows per sample), m_off, rows (int row table, < 0 = dropped) | None, splits ([(k0, k1)]).  All tensors fp64.
    Returns name -> fp64 tensor for C, h0, h1 (h0 alone: the residual epilogue's y); model=False adds "T" (name -> magnitude sum)
    and, for GeGLU, "G" = max(|h0|, |gelu(h0)|) |h1|.  model=True applies the one documented rounding per output.  With a row
    table C has the launch's M rows: row m belongs to row rows[m] of the full matrix."""
    assert mutant is None or mutant in MUTANTS, mutant
    A, epi = op["A"], op["epi"]
    rnd = bf if model else (lambda t: t)
    out, T = {}, {}
    if epi == EPI_GEGLU:
        W0, W1 = op["Ws"]
        if mutant == "geglu_halves_swapped":
            W0, W1 = W1, W0
        h0, T0 = _acc(A, W0, mutant)
        h1, T1 = _acc(A, W1)
        out["C"], out["h0"], out["h1"] = rnd(gelu_erf(h0) * h1), rnd(h0), rnd(h1)
        T["C"] = gelu_erf_grad(h0).abs() * T0 * h1.abs() + gelu_erf(h0).abs() * T1
        T["h0"], T["h1"] = T0, T1
        if not model:
            out["T"], out["G"] = T, torch.maximum(h0.abs(), gelu_erf(h0).abs()) * h1.abs()
        return out
    W = torch.cat(list(op["Ws"]), 0)
    N = W.shape[0]
    acc, Ta = _acc(A, W, mutant, op.get("splits"))
    nseg = len(op["Ws"])
    bl = list(op.get("biases") or []) + [None] * 3
    if mutant == "segment_bias_of_neighbour":
        bl = [bl[(i + 1) % nseg] for i in range(nseg)]
    bias = torch.cat([b if b is not None else torch.zeros(w.shape[0], dtype=A.dtype, device=A.device) for w, b in zip(op["Ws"], bl)])
    if mutant == "bias_twice_in_fold":
        bias = 2 * bias
    if epi == EPI_BIAS:
        out["C"], T["C"] = rnd(acc + bias), Ta + bias.abs()
    elif epi == EPI_F32:
        alpha = op.get("alpha", 1.0)
        out["C"], T["C"] = acc * alpha + bias, Ta * abs(alpha) + bias.abs()
        if model:
            out["C"] = out["C"].float().double()
    else:
        M = A.shape[0]
        y, Ty = acc + bias, Ta + bias.abs()
        m = torch.arange(M, device=A.device)
        s = torch.ones(M, 1, dtype=A.dtype, device=A.device)
        if op.get("rowscale") is not None:
            m_off, rps = op.get("m_off", 0), max(op.get("rps", 0), 1)
            idx = (m + m_off) // rps
            if mutant == "tail_rowscale_without_m_off":   # the remainder launch of a tail-rows split counts its rows from 0
                m_main = M - (M % 256)
                idx = torch.where(m >= m_main, (m - m_main + m_off) // rps, idx)
            s = op["rowscale"][idx][:, None]
        if op.get("gamma") is not None:
            s = s * op["gamma"][None, :]
        else:
            s = s.expand(M, N)
        resid = op["resid"]
        if op.get("rows") is not None:
            resid = resid[op["rows"].clamp_min(0).long()]
        yy = bf(y) if mutant == "y_rounded_before_layer_scale" else y
        out["C"], out["h0"] = rnd(resid + s * yy), rnd(y)
        T["C"], T["h0"] = resid.abs() + s.abs() * Ty, Ty
    if not model:
        out["T"] = T
    return out


def tn_ref(A_km, B_kn, base=None, model=False, mutant=None, rscale=None):
    """C = (base +) (rscale[:, None] *) A_km^T B_kn in fp64, and its magnitude sum."""
    P, TP = A_km.t() @ B_kn, A_km.abs().t() @ B_kn.abs()
    if rscale is not None:
        P, TP = rscale[:, None] * P, rscale.abs()[:, None] * TP
    if mutant == "accumulate_double_round":
        P = bf(P)
    C, T = (P, TP) if base is None else (base + P, base.abs() + TP)
    return (bf(C) if model else C), T


def tn_side_ref(A_km, B_kn, W):
    """rowdot [N / 128, M] of hip.gemm_tn_grouped: rowdot[s][m] = sum over the 128 columns n of slot s of W[m][n] * (A_km^T B_kn)[m][n]
    (the launch's own fp32 product, unscaled), and its magnitude sum."""
    P, TP = A_km.t() @ B_kn, A_km.abs().t() @ B_kn.abs()
    M, N = P.shape
    return ((W * P).view(M, N // 128, 128).sum(2).t().contiguous(), (W.abs() * TP).view(M, N // 128, 128).sum(2).t().contiguous())


# ----------------------------------------------------------------------------------------------------------------------
# the gate
# ----------------------------------------------------------------------------------------------------------------------
def half_ulp_bf16(x):
    """Half a bf16 ulp at |x| (fp64 tensor); below the smallest normal number the subnormal spacing."""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -126))    # |x| = m 2^e, m in [0.5, 1): the binade is 2^(e - 1)
    return torch.ldexp(torch.ones_like(x), e - 9)


def budget(exact, T, rounding, G=None, c_acc=None, c_gelu=None):
    """(R, fp32 allowance) per element.  rounding: "bf16" | "f32"."""
    f32 = (C_ACC if c_acc is None else c_acc) * U32 * T
    if G is not None:
        f32 = f32 + (C_GELU if c_gelu is None else c_gelu) * U32 * G
    R = half_ulp_bf16(exact.abs() + f32) if rounding == "bf16" else torch.zeros_like(exact)
    return R, f32


def gate(got, exact, T, rounding, G=None, what="C", c_acc=None, c_gelu=None):
    """Per-element check of one output.  Returns (failures, figures): failures = strings; figures = the largest |err| / (2^-24 T),
    |err| / R (bf16 outputs) and (|err| - R) / (2^-24 G) (GeGLU product) over the elements whose exact value is finite.  Where the
    exact value is not finite, got must not be finite either -- and nowhere else."""
    got, fails, fig = got.double(), [], {}
    fin = torch.isfinite(exact) & torch.isfinite(T)
    wrong = fin != torch.isfinite(got)
    if bool(wrong.any()):
        i = tuple(wrong.nonzero()[0].tolist())
        fails.append("%s%s: got %r where exact is %r (%d elements differ in finiteness)" % (what, list(i), float(got[i]), float(exact[i]), int(wrong.sum())))
    z = torch.zeros_like(exact)
    err = torch.where(fin, (got - exact).abs(), z)
    err = torch.where(torch.isfinite(err), err, z)
    ex, Tm = torch.where(fin, exact, z), torch.where(fin, T, z)
    Gm = torch.where(fin, G, z) if G is not None else None
    R, f32 = budget(ex, Tm, rounding, Gm, c_acc, c_gelu)
    bad = err > R + f32
    if bool(bad.any()):
        i = tuple(bad.nonzero()[0].tolist())
        fails.append("%s%s: |%.9g - %.9g| = %.3e > R %.3e + fp32 %.3e (T %.3e; %d of %d elements)" % (
            what, list(i), float(got[i]), float(exact[i]), float(err[i]), float(R[i]), float(f32[i]), float(Tm[i]), int(bad.sum()), bad.numel()))
    tiny = 1e-300
    fig["acc"] = float((err / (U32 * Tm).clamp_min(tiny)).max()) if err.numel() else 0.0
    if rounding == "bf16":
        fig["R"] = float((err / R).max()) if err.numel() else 0.0
    if G is not None:
        fig["gelu"] = float(((err - R).clamp_min(0) / (U32 * Gm).clamp_min(tiny)).max())
    return fails, fig


# ----------------------------------------------------------------------------------------------------------------------
# input families
# ----------------------------------------------------------------------------------------------------------------------
FAMILIES = ("unit", "offset", "cancel", "wide", "integer", "basis", "nonfinite")


def _gen(family, seed):
    return torch.Generator().manual_seed(1000 * FAMILIES.index(family) + seed)


def make_ab(family, M, N, K, seed=0, span=40, inf_row=None):
    """A [M, K], W [N, K] as fp32 tensors holding bf16 values (CPU, seeded).
    unit: A ~ N(0, 1), W ~ N(0, 1 / K).  offset: A + 8 (large accumulators, moderate results).
    cancel: the second half of K mirrors the first with the opposite sign in W, A scaled by 1 + 2^-6 there (T >> |exact|).
    wide: rows of A and of W scaled by powers of two from 2^-span to 2^span.  integer: entries in {-2 ... 2} (every partial sum exact).
    basis: row m of A is one-hot at k = (K - 1 - m) mod K, so C[m, n] = W[n, k] (W ~ N(0, 1) here).
    nonfinite: one NaN in row M // 2 of A, one +Inf in row inf_row (default N // 2) of W."""
    g = _gen(family, seed)
    A = torch.randn(M, K, generator=g)
    W = torch.randn(N, K, generator=g) * K ** -0.5
    if family == "offset":
        A = A + 8.0
    elif family == "cancel":
        h = K // 2
        A, W = A.to(torch.bfloat16).float(), W.to(torch.bfloat16).float()
        A[:, h:2 * h] = A[:, :h] * (1.0 + 2.0 ** -6)
        W[:, h:2 * h] = -W[:, :h]
    elif family == "wide":
        ea = torch.randint(-span, span + 1, (M,), generator=g)
        ew = torch.randint(-span, span + 1, (N,), generator=g)
        ea[0], ew[0], ea[M - 1], ew[N - 1] = -span, span, span, -span
        A, W = torch.ldexp(A, ea[:, None]), torch.ldexp(W, ew[:, None])
    elif family == "integer":
        A = torch.randint(-2, 3, (M, K), generator=g).float()
        W = torch.randint(-2, 3, (N, K), generator=g).float()
    elif family == "basis":
        W = W * K ** 0.5      # N(0, 1): the outputs ARE weight entries, and a GeGLU launch sees gelu over its whole working range
        A = torch.zeros(M, K)
        A[torch.arange(M), (K - 1 - torch.arange(M)) % K] = 1.0
    elif family == "nonfinite":
        A[M // 2, K // 3] = float("nan")
        W[N // 2 if inf_row is None else inf_row, (2 * K) // 3] = float("inf")
    elif family != "unit":
        raise ValueError(family)
    return A.to(torch.bfloat16).float(), W.to(torch.bfloat16).float()


def make_vec(family, n, seed, kind):
    """bias / gamma / rowscale / a residual or base matrix row block (n may be a shape).  In the `integer` family every one of them is
    a small integer or a power of two, so that every fp32 operation of every epilogue is exact."""
    g = _gen(family, 7919 + seed)
    shape = n if isinstance(n, tuple) else (n,)
    if family == "integer":
        if kind in ("bias", "resid"):
            v = torch.randint(-2, 3, shape, generator=g).float()
        else:   # gamma, rowscale: +-(0.5, 1, 2)
            v = torch.ldexp(torch.ones(shape), torch.randint(-1, 2, shape, generator=g)) * (1 - 2 * torch.randint(0, 2, shape, generator=g)).float()
            v = v.abs() if kind == "rowscale" else v
    elif kind == "gamma":
        v = 0.1 + torch.rand(shape, generator=g)
        v[::5] = -v[::5]
    elif kind == "rowscale":   # drop-path: 0 or 1 / keep
        v = torch.where(torch.rand(shape, generator=g) < 0.3, torch.zeros(shape), torch.full(shape, 1.25))
    else:
        v = torch.randn(shape, generator=g)
    return v if kind == "rowscale" else v.to(torch.bfloat16).float()


# ----------------------------------------------------------------------------------------------------------------------
# guards
# ----------------------------------------------------------------------------------------------------------------------
SENTINEL = {torch.bfloat16: (torch.int16, 0x7FA5), torch.float32: (torch.int32, 0x7FC5A5A5), torch.int32: (torch.int32, -0x5A5A5A5B)}
# (both floating-point patterns are NaNs: around an INPUT, anything read from outside the operand that reaches a valid output shows)


def guarded(shape, dtype, ld_extra=8, pad_rows=2, device="cpu"):
    """A view of `shape` (1-D or 2-D) inside a larger buffer filled with a sentinel bit pattern: ld = cols + ld_extra, pad_rows rows
    above and below (a vector: 8 * pad_rows elements in front and ld_extra + 8 * pad_rows behind); the view starts a multiple of 8
    elements into the buffer.  check_guard(view) compares everything outside the view with the sentinel, as integers."""
    it, pat = SENTINEL[dtype]
    if len(shape) == 1:
        front = 8 * pad_rows
        buf = torch.full((front + shape[0] + ld_extra + front,), pat, dtype=it, device=device).view(dtype)
        view = buf[front:front + shape[0]]
        mask = torch.ones(buf.shape, dtype=torch.bool, device=device)
        mask[front:front + shape[0]] = False
    else:
        rows, cols = shape
        ld = cols + ld_extra
        assert ld % 8 == 0, "leading dimensions stay multiples of 8 elements"
        buf = torch.full((rows + 2 * pad_rows, ld), pat, dtype=it, device=device).view(dtype)
        view = buf[pad_rows:pad_rows + rows, :cols]
        mask = torch.ones(buf.shape, dtype=torch.bool, device=device)
        mask[pad_rows:pad_rows + rows, :cols] = False
    view._guard = (buf, mask)
    return view


def guarded_from(src, dtype=None, device=None, **kw):
    """A guarded copy of `src` (None stays None)."""
    if src is None:
        return None
    dtype = dtype or src.dtype
    v = guarded(tuple(src.shape), dtype, device=device or src.device, **kw)
    v.copy_(src.to(v.device))
    return v


def check_guard(view):
    """Number of guard elements around `view` that no longer hold the sentinel (0 = untouched)."""
    buf, mask = view._guard
    it, pat = SENTINEL[buf.dtype]
    return int(((buf.view(it) != pat) & mask).sum())


# ----------------------------------------------------------------------------------------------------------------------
# the route mirror of op_gemm_nt
# ----------------------------------------------------------------------------------------------------------------------
class NtCase:
    """One NT launch of the GPU test.  route: the name the case was WRITTEN for (route(case) must return it).  M, N, K: the launch
    (GeGLU: N = F); nseg weight segments of N / nseg rows; bias: per segment, present or not; h: with the h0 (/ h1) outputs;
    rows: "table" = residual epilogue through a row table with dropped rows; alias: resid is C; tune: TUNE fields."""

    def __init__(self, group, route, epi, M, N, K, family="unit", nseg=1, bias=(True, True, True), h=False, gamma=True, rowscale=True,
                 rps=0, alias=False, rows=None, alpha=None, splitk=True, slabs=False, **tune):
        self.group, self.route, self.epi, self.M, self.N, self.K, self.family = group, route, epi, M, N, K, family
        self.nseg, self.bias, self.h, self.gamma, self.rowscale, self.rps = nseg, tuple(bias)[:nseg], h, gamma, rowscale, rps
        self.alias, self.rows, self.alpha, self.splitk, self.slabs, self.tune = alias, rows, alpha, splitk, slabs, tune
        if epi == EPI_GEGLU:
            self.bias = (False,)
        opts = "".join(("-seg%d" % nseg if nseg > 1 else "", "-b" + "".join("1" if b else "0" for b in self.bias) if epi != EPI_GEGLU else "",
                        "-h" if h else "", "" if epi != EPI_RESID else "-g%d%d" % (gamma, rowscale), "-rps%d" % rps if rps else "",
                        "-alias" if alias else "", "-rows" if rows else "", "-alpha" if alpha is not None else "",
                        "" if splitk else "-nosplit"))
        kn = "".join("-%s%d" % (k, v) for k, v in sorted(tune.items()))
        self.id = "%s-%s-%s-M%d-N%d-K%d-%s%s%s" % (group, route, EPI_NAMES[epi], M, N, K, family, opts, kn)


def apply_tune(hip, tune):
    hip.TUNE.reset()
    for k, v in tune.items():
        assert hasattr(hip.TUNE, k), k
        setattr(hip.TUNE, k, v)


def four_wave_256(hip, M, N, K, splits):
    """csrc/gemm.hip: four_wave_256 (does launch256 take gemm256v / gemm256p?)."""
    fl = hip.TUNE.fullline
    fills = cdiv(M, 256) * cdiv(N, 256) >= 256 and splits == 1
    return (fl == 3 or (fl == 2 and fills)) and splits == 1 and N % 256 == 0 and K % 64 == 0 and K >= 128


def _kernel_name(hip, tile, splits, fold, M, N, K, epi, rows, m_off):
    """The kernel of ONE launch (launch / launch256 of csrc/gemm.hip) under the current hip.TUNE."""
    T = hip.TUNE
    if tile == 128 or (rows and splits == 1 and not four_wave_256(hip, M, N, K, splits)):   # (a K-split launch writes fp32 slabs: no row table in the kernel)
        name = "nt128" if T.glds else "nt128_regstaged"
    else:
        e = EPI_F32 if splits > 1 else epi
        nq = 128 if e == EPI_GEGLU else 256
        fills = cdiv(M, 256) * cdiv(N, nq) >= 256 and splits == 1
        if (T.fullline == 3 or (T.fullline == 2 and fills and e != EPI_GEGLU)) and splits == 1 and N % nq == 0 and K % 64 == 0 and K >= 128:
            short_k = e in (EPI_BIAS, EPI_RESID) and m_off == 0 and K <= 2048
            sched = T.sched if T.sched else (6 if short_k else 3)
            name = "g256p" if (e in (EPI_BIAS, EPI_RESID) and sched == 6 and m_off == 0) else "g256v"
        elif (T.fullline == 1 or (T.fullline == 2 and fills)) and N % nq == 0 and K % 64 == 0:
            name = "g256b"
        else:
            name = "g256_bk32"
    if splits > 1:
        name += "+fold" if fold else "+splitk_reduce"
    return name


def ws_bytes_of(case):
    """The split-K scratch hip.gemm_nt hands to the library (0 = none)."""
    if case.splitk and case.epi in (EPI_BIAS, EPI_RESID) and (case.K >= 2048 or case.M <= 1024):
        return max(32 * case.M * case.N, 1 << 20)
    return 0


def route(case, hip):
    """Name of the kernels op_gemm_nt runs for `case`, from hip.gemm_plan (host-only), the four-wave rule and the case's TUNE fields:
    nt128 | nt128_regstaged | g256_bk32 | g256b | g256v | g256p, + "+splitk_reduce" | "+fold" for a K-split launch, + "+tail128" |
    "+tail256" (and the remainder's own "+fold" / "+splitk_reduce") when the rows of M % 256 run as a second launch.  (With
    tile_mode = 2 the remainder is forced onto the 256 x 256 kernels as well, and -- having a row offset -- never onto gemm256p.)"""
    tune = dict(case.tune)
    seg = case.N // case.nseg
    if case.epi != EPI_GEGLU and case.nseg > 1 and seg % 256 != 0:
        tune["tile_mode"] = 1     # (seg_ok of gemm_nt_impl: segments that are no multiple of 256 keep the 128 x 128 kernel)
    try:
        apply_tune(hip, tune)
        ws = ws_bytes_of(case)
        has_bias = bool(case.bias[0]) and case.epi != EPI_GEGLU
        tile, splits, fold, tail = hip.gemm_plan(case.M, case.N, case.K, case.epi, has_bias, ws)
        rows = bool(case.rows)
        name = _kernel_name(hip, tile, splits, fold, case.M - tail, case.N, case.K, case.epi, rows, 0)
        if tail:
            t2, s2, f2, tail2 = hip.gemm_plan(tail, case.N, case.K, case.epi, has_bias, ws)
            assert tail2 == 0
            rem = _kernel_name(hip, t2, s2, f2, tail, case.N, case.K, case.epi, rows, case.M - tail)
            name += "+tail128" if rem.startswith("nt128") else "+tail256"
            if s2 > 1:
                name += rem[rem.index("+"):]
        return name
    finally:
        hip.TUNE.reset()


def split_ranges(K, forced):
    """K-ranges of the slabs of a forced split on the 128 x 128 kernel (plan_gemm: 64-deep K-tiles, ceil(nk / s) per slab)."""
    nk = K // 64
    kps = cdiv(nk, forced)
    return [(z * kps * 64, min(nk, (z + 1) * kps) * 64) for z in range(cdiv(nk, kps))]


def tn_route(M, N, K, splitk, accumulate, fullline):
    """op_gemm_tn's choice, restated: (name, K-ranges of the split-K slabs).  name: tn8w | tn4w, + "+splitk_reduceN" | "+resid" (in-place
    accumulation) | "".  The GPU test does not take this on trust: it fills the scratch with NaN before the launch and gates every slab
    the name promises against fp64 -- and requires the scratch untouched where the name promises no split."""
    nk, tiles = K // 32, cdiv(M, 256) * cdiv(N, 256)
    best_s, best_t, best_kps = 1, 1e300, nk
    for s in range(1, 17):
        if s > 1 and (not splitk or nk // s < 16):
            break
        kps = cdiv(nk, s)
        kps += kps & 1
        eff = cdiv(nk, kps)
        t = float((tiles * eff + 255) // 256) * kps * (256.0 * 256 / 1040.0) * 32
        if eff > 1:
            t += eff * M * N * 8.0 / 4.0e3 + 1.0e4
        if t < best_t:
            best_t, best_s, best_kps = t, eff, kps
    four = fullline == 3 or (fullline == 2 and tiles <= 108 and K >= 16384)
    name = ("tn4w" if four else "tn8w") + ("+splitk_reduce%d" % best_s if best_s > 1 else "+resid" if accumulate else "")
    ranges = [(z * best_kps * 32, min(nk, (z + 1) * best_kps) * 32) for z in range(best_s)] if best_s > 1 else []
    return name, ranges


# ----------------------------------------------------------------------------------------------------------------------
# operands of an NT case
# ----------------------------------------------------------------------------------------------------------------------
def make_row_table(M, rows_total, seed):
    """int32 [M]: distinct rows of a [rows_total, N] matrix in a scrambled order, about one in seven dropped (-1, -7)."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randperm(rows_total, generator=g)[:M].to(torch.int32)
    drop = torch.rand(M, generator=g) < 0.15
    if M > 3:
        drop[1] = True
    t[drop] = -1
    t[drop & (torch.arange(M) % 2 == 0)] = -7
    return t


def make_nt_operands(case, seed=0):
    """CPU fp32 tensors (bf16 values) of `case`: dict with A, Ws, biases, and by epilogue alpha, resid, gamma, rowscale, rps, rows."""
    fam, M, N, K = case.family, case.M, case.N, case.K
    geglu = case.epi == EPI_GEGLU
    nrow = 2 * N if geglu else N
    span = 20 if geglu else 40    # (GeGLU multiplies two products: 2^80 x 2^80 leaves bf16)
    A, W = make_ab(fam, M, nrow, K, seed, span=span, inf_row=(N + N // 2) if geglu else None)
    op = {"epi": case.epi, "A": A}
    if geglu:
        op["Ws"], op["biases"] = [W[:N].contiguous(), W[N:].contiguous()], [None, None]
        return op
    seg = N // case.nseg
    op["Ws"] = [W[i * seg:(i + 1) * seg].contiguous() for i in range(case.nseg)]
    op["biases"] = [make_vec(fam, seg, 10 + i, "bias") if case.bias[i] else None for i in range(case.nseg)]
    if case.epi == EPI_F32 and case.alpha is not None:
        op["alpha"] = case.alpha
    if case.epi == EPI_RESID:
        rows_total = M + 9 if case.rows else M
        op["resid"] = make_vec(fam, (rows_total, N), 20, "resid")
        op["gamma"] = make_vec(fam, N, 21, "gamma") if case.gamma else None
        op["rps"] = case.rps
        op["rowscale"] = make_vec(fam, cdiv(M, max(case.rps, 1)), 22, "rowscale") if case.rowscale else None
        op["rows"] = make_row_table(M, rows_total, 23) if case.rows else None
    return op


def op_to(op, device, dtype=torch.float64):
    """The operand dict with every tensor on `device` as `dtype` (the row table stays an integer tensor)."""
    def cv(v):
        if isinstance(v, torch.Tensor):
            return v.to(device) if not v.is_floating_point() else v.to(device=device, dtype=dtype)
        if isinstance(v, list):
            return [cv(x) for x in v]
        return v
    return {k: cv(v) for k, v in op.items()}


# ----------------------------------------------------------------------------------------------------------------------
# the NT cases (shared: the CPU test checks every declared route against route(case) without a GPU)
# ----------------------------------------------------------------------------------------------------------------------
SWEEP_M = (1, 17, 127, 129, 255, 257)
SWEEP_K = (64, 128, 192, 448, 1536)
T256 = dict(tile_mode=2)
FLAVOURS = (   # name at K >= 128, TUNE fields, the epilogues the kernel has
    ("g256_bk32", dict(tile_mode=2, fullline=0), (EPI_BIAS, EPI_F32, EPI_GEGLU, EPI_RESID)),
    ("g256b", dict(tile_mode=2, fullline=1), (EPI_BIAS, EPI_F32, EPI_GEGLU, EPI_RESID)),
    ("g256v", dict(tile_mode=2, fullline=3, sched=3), (EPI_BIAS, EPI_F32, EPI_GEGLU, EPI_RESID)),
    ("g256p", dict(tile_mode=2, fullline=3, sched=6), (EPI_BIAS, EPI_RESID)),
)


def _nt_cases():
    c = []
    add = lambda *a, **k: c.append(NtCase(*a, **k))  # noqa: E731
    # ---- every family on every route and epilogue, at one shape per route (M = 257: two M-tiles of 128, a one-row last tile of 256)
    for fam in FAMILIES:
        for glds in (1, 0):
            r = "nt128" if glds else "nt128_regstaged"
            t = dict(tile_mode=1, glds=glds)
            add("families", r, EPI_BIAS, 257, 136, 192, fam, **t)
            add("families", r, EPI_F32, 257, 136, 192, fam, alpha=0.5, **t)
            add("families", r, EPI_GEGLU, 257, 72, 192, fam, h=True, **t)
            add("families", r, EPI_RESID, 257, 136, 192, fam, h=True, rps=7, **t)
        for name, t, epis in FLAVOURS:
            for epi in epis:
                extra = dict(alpha=0.5) if epi == EPI_F32 else dict(h=True, rps=7) if epi == EPI_RESID else dict(h=True) if epi == EPI_GEGLU else {}
                add("families", name, epi, 257, 256, 192, fam, **extra, **t)
        add("families", "nt128+splitk_reduce", EPI_BIAS, 129, 136, 448, fam, bias=(False,), force_splits=3, tile_mode=1, slabs=True)
        add("families", "nt128+fold", EPI_RESID, 129, 136, 448, fam, h=True, rps=7, force_splits=2, tile_mode=1)
        add("families", "g256v+tail256", EPI_RESID, 529, 256, 192, fam, h=True, rps=100, tail_rows=3, tile_mode=2, fullline=3, sched=3)
        add("families", "nt128_regstaged+fold", EPI_RESID, 129, 136, 448, fam, alias=True, gamma=False, force_splits=3, tile_mode=1, glds=0)
        # the remainder's own K-split and fold: default tiles, a launch of more than 512 128 x 128 tiles whose leftover row splits K
        add("families", "g256p+tail128+fold", EPI_RESID, 5633, 1536, 2048, fam, h=True, rps=257, tail_rows=3, fullline=3)
        # 256 x 256 slabs: the smallest problem for which the planner reports (256, s > 1) -- it needs more than 256 128 x 128 tiles
        add("families", "g256_bk32+splitk_reduce", EPI_BIAS, 5632, 768, 4096, fam, bias=(False,))
        add("families", "g256b+splitk_reduce", EPI_BIAS, 5632, 768, 4096, fam, bias=(False,), fullline=1)
    # ---- the M, N, K sweep on `unit` and `cancel`
    for fam in ("unit", "cancel"):
        for i, M in enumerate(SWEEP_M):
            for j, K in enumerate(SWEEP_K):
                if (i + j) % 2:      # a checkerboard of the M x K product per kernel; the other colour on the second staging form
                    continue
                N = (8, 72, 136, 264)[(i + j // 2) % 4]
                add("sweep", "nt128", EPI_BIAS, M, N, K, fam, splitk=False, tile_mode=1)   # (no scratch: the planner would split K = 1536)
                add("sweep", "nt128_regstaged", EPI_RESID, M, N, K, fam, h=True, rps=7, splitk=False, tile_mode=1, glds=0)
            for j, K in enumerate(SWEEP_K):
                if (i + j) % 2 == 0:
                    continue
                N = (8, 72, 136, 264)[(i + j // 2) % 4]
                add("sweep", "nt128_regstaged", EPI_BIAS, M, N, K, fam, splitk=False, tile_mode=1, glds=0)
                add("sweep", "nt128", EPI_RESID, M, N, K, fam, h=True, rps=7, splitk=False, tile_mode=1)
                add("sweep", "nt128", EPI_GEGLU, M, (8, 72)[j % 2], K, fam, h=bool(i % 2), tile_mode=1)
                add("sweep", "nt128", EPI_F32, M, N, K, fam, alpha=-1.5, bias=(bool(i % 2),), tile_mode=1)
        for name, t, epis in FLAVOURS:
            for i, M in enumerate(SWEEP_M):
                for j, K in enumerate(SWEEP_K):
                    if (i + j) % 2 or (K == 64 and name in ("g256v", "g256p")):   # K = 64: the four-wave flavours fall back to the BK = 32 kernel
                        continue
                    N = (256, 512)[(i + j // 2) % 2]
                    epi = epis[(i + j // 2) % len(epis)]
                    extra = dict(alpha=-1.5) if epi == EPI_F32 else dict(h=bool(i % 2), rps=7) if epi == EPI_RESID else dict(h=bool(i % 2)) if epi == EPI_GEGLU else {}
                    add("sweep", name, epi, M, N, K, fam, **extra, **t)
            if name == "g256_bk32":   # N % 256 != 0: the half-store guards of the 256 x 256 kernel
                add("sweep", "g256_bk32", EPI_BIAS, 129, 264, 192, fam, **t)
                add("sweep", "g256_bk32", EPI_RESID, 257, 136, 448, fam, h=True, rps=7, **t)
            elif name != "g256b":
                add("sweep", "g256_bk32", epis[-1], 129, 256, 64, fam, h=epis[-1] == EPI_RESID, **t)
    # ---- nt128: segments, GeGLU outputs, residual forms
    for glds in (1, 0):
        r = "nt128" if glds else "nt128_regstaged"
        t = dict(tile_mode=1, glds=glds)
        add("forms", r, EPI_BIAS, 129, 128, 128, "unit", nseg=1, **t)
        add("forms", r, EPI_BIAS, 129, 256, 128, "unit", nseg=2, bias=(True, False), **t)
        add("forms", r, EPI_BIAS, 129, 384, 128, "unit", nseg=3, bias=(True, False, True), **t)
        add("forms", r, EPI_BIAS, 129, 384, 128, "unit", nseg=3, bias=(False, False, False), **t)
        add("forms", r, EPI_F32, 129, 384, 128, "unit", nseg=3, bias=(True, False, True), alpha=0.75, **t)
        add("forms", r, EPI_GEGLU, 129, 72, 128, "unit", h=False, **t)
        add("forms", r, EPI_GEGLU, 129, 72, 128, "unit", h=True, **t)
        add("forms", r, EPI_GEGLU, 192, 264, 192, "basis", h=True, **t)     # (exact accumulators: what C_GELU is measured on)
        for gamma, rowscale in ((False, False), (True, False), (False, True), (True, True)):
            add("forms", r, EPI_RESID, 129, 136, 128, "unit", gamma=gamma, rowscale=rowscale, rps=7, **t)
        add("forms", r, EPI_RESID, 129, 136, 128, "unit", alias=True, rps=7, **t)
        add("forms", r, EPI_RESID, 129, 136, 128, "unit", rows="table", h=True, rps=7, **t)
        add("forms", r, EPI_RESID, 129, 136, 128, "unit", rows="table", alias=True, rps=7, **t)
    # ---- 256 x 256 kernels: segments of 256, EPI_F32 with alpha and bias, row tables on the four-wave kernels
    for name, t, epis in FLAVOURS:
        add("forms", name, EPI_BIAS, 257, 768, 128, "unit", nseg=3, bias=(True, False, True), **t)
        add("forms", name, EPI_RESID, 257, 512, 128, "unit", nseg=2, bias=(False, True), alias=True, rps=7, **t)
        if EPI_F32 in epis:
            add("forms", name, EPI_F32, 257, 512, 128, "unit", nseg=2, bias=(True, False), alpha=0.75, **t)
            add("forms", name, EPI_GEGLU, 192, 512, 192, "basis", h=True, **t)
        if name in ("g256v", "g256p"):
            add("forms", name, EPI_RESID, 257, 256, 128, "unit", rows="table", h=True, rps=7, **t)
            add("forms", name, EPI_RESID, 257, 256, 128, "cancel", rows="table", alias=True, gamma=False, rps=7, **t)
        else:   # the eight-wave kernels have no row-table epilogue: the launch goes to the 128 x 128 kernel
            add("forms", "nt128", EPI_RESID, 257, 256, 128, "unit", rows="table", h=True, rps=7, **t)
    # ---- split-K on the 128 x 128 kernel, K = 448 (7 K-tiles: 4 + 3, and 3 + 3 + 1)
    for fam in ("unit", "cancel"):
        for s in (2, 3):
            for M, N in ((17, 8), (257, 264)):
                t = dict(force_splits=s, tile_mode=1)
                add("splitk", "nt128+splitk_reduce", EPI_BIAS, M, N, 448, fam, bias=(False,), slabs=True, **t)
                add("splitk", "nt128+fold", EPI_BIAS, M, N, 448, fam, **t)
                add("splitk", "nt128+fold", EPI_RESID, M, N, 448, fam, h=True, rps=7, **t)
                add("splitk", "nt128+fold", EPI_RESID, M, N, 448, fam, rows="table", h=True, rps=7, **t)
            add("splitk", "nt128+fold", EPI_BIAS, 257, 384, 448, fam, nseg=3, bias=(True, False, True), force_splits=s, tile_mode=1)
            add("splitk", "nt128_regstaged+fold", EPI_RESID, 129, 136, 448, fam, alias=True, gamma=False, force_splits=s, tile_mode=1, glds=0)
    # ---- tail-rows split (tail_rows = 3: always): the rows of M % 256 as a second launch with a row offset
    for name, t, epis in FLAVOURS:
        main = name
        for M in (257, 384, 529):
            tt = dict(t, tail_rows=3)
            # rows_per_sample = 100 straddles the split at 256 / 512 (samples 2 and 5 lie on both sides): m_off
            add("tail", main + "+tail256", EPI_RESID, M, 256, 192, "unit", h=True, rps=100, **tt)
            add("tail", main + "+tail256", EPI_BIAS, M, 512, 128, "cancel", **tt)
        if name in ("g256v", "g256p"):
            add("tail", main + "+tail256", EPI_RESID, 529, 256, 192, "cancel", rows="table", h=True, rps=100, **dict(t, tail_rows=3))
        if EPI_F32 in epis:
            add("tail", main + "+tail256", EPI_F32, 384, 256, 192, "unit", alpha=0.75, **dict(t, tail_rows=3))
            add("tail", main + "+tail256", EPI_GEGLU, 529, 128, 192, "unit", h=True, **dict(t, tail_rows=3))
    add("tail", "g256p+tail128+fold", EPI_RESID, 5633, 1536, 2048, "cancel", rows="table", rps=257, tail_rows=3, fullline=3)
    ids = [x.id for x in c]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1][:3]
    return c


NT_CASES = _nt_cases()
