"""Autograd layer over the C-ABI HIP kernels (``hip.py``).

Each ``torch.autograd.Function`` here is what the host-side mirrors of the reference modules call when their
input is a bf16 tensor on an MI355X.  Forward and backward enqueue HIP kernels on the current stream; PyTorch
only owns the memory.  An encoder layer is two functions -- ``AttnBranchFn`` (LN, fused QKV GEMM, attention, sub-LN,
out-proj + layer-scale/drop-path residual) and ``FfnBranchMultiFn`` (LN, GeGLU GEMM, LN(F), down GEMM + residual) -- so that
joint text+image / text+audio streams can route each modality's rows to its own FFN.  With ``save_acts=False`` a branch
keeps only its input and recomputes the intermediates in backward -- the reference's ``checkpoint_activations: true``
(pretrain_vl_3B.yaml:93, one_peace_pretrain.py:78-96); with ``save_acts=True`` (``checkpoint_activations: false``) it
keeps them, which 288 GB of HBM affords even for the 4B model at batch 64.
"""
import math
import os
import weakref

import torch
import torch.nn.functional as F

from . import hip

# --------------------------------------------------------------------------------------------------------------
# derived-buffer cache: transposed weights for the dgrad GEMMs (never parameters, rebuilt when the weight changes)
# --------------------------------------------------------------------------------------------------------------
_wt_cache = {}
_cache_epoch = 0


_refresh_plan = None  # (key set, device table, n, total tiles, [cache keys]) of the batched refresh


def invalidate_weight_cache():
    """Call after parameters were updated through raw pointers (the fused AdamW kernel does not bump _version)."""
    global _cache_epoch
    _cache_epoch += 1


def refresh_weight_cache():
    """After an optimiser step: rebuild EVERY cached transposed weight in one batched launch (520 matrices at 4B; lazily,
    one launch per matrix plus a concatenation per q/k/v triple, they cost 14 ms per step) and mark them current."""
    global _cache_epoch, _refresh_plan
    _cache_epoch += 1
    # fp8 copies of the FFN weights (opt-in variant): re-quantised IN PLACE into the same buffers -- a replayed TrainStepGraph keeps
    # reading these addresses, and an eager step must not pay a cache miss per weight either
    if not FP8_FFN and (_fp8_cache or _fp8_derived_cache):  # the opt-in variant was switched off: nothing reads these copies any more
        _fp8_cache.clear()
        _fp8_pairs.clear()
        _fp8_derived_cache.clear()
    for k, (ref, _, qs) in list(_fp8_cache.items()):
        w = ref()
        if w is None:
            del _fp8_cache[k]
            continue
        hip.quant_fp8_rows(w.detach(), out=qs)
        _fp8_cache[k] = (ref, (w._version, w.data_ptr(), _cache_epoch), qs)
    live = [(k, v) for k, v in _wt_cache.items() if all(r() is not None for r in v[0]) and (v[3] is None or v[3]() is not None)]
    if not live:
        return
    sig = tuple((k, tuple(r().data_ptr() for r in v[0]), v[2].data_ptr(), v[3]().data_ptr() if v[3] is not None else 0) for k, v in live)
    if _refresh_plan is None or _refresh_plan[0] != sig:
        jobs = []
        for k, v in live:
            off = 0
            for r in v[0]:
                w = r().detach()
                # segment i fills columns [off, off + out_i) of [in, sum out]; a scaled entry (one weight) carries its row scales
                jobs.append((w, v[2][:, off:off + w.shape[0]], v[3]().detach() if v[3] is not None else None))
                off += w.shape[0]
        table, tiles = hip.transpose_table(jobs, live[0][1][2].device)
        _refresh_plan = (sig, table, len(jobs), tiles)
    hip.transpose_batched(_refresh_plan[1], _refresh_plan[2], _refresh_plan[3])
    torch.autograd.graph.increment_version([v[2] for _, v in live])
    for k, v in live:
        _wt_cache[k] = (v[0], _wt_version(tuple(r() for r in v[0]), v[3]() if v[3] is not None else None), v[2], v[3])
    for k, (_, qs, tref) in list(_fp8_derived_cache.items()):  # fp8 copies of the transposed weights (opt-in fp8 input-gradient GEMMs)
        t = tref()
        if t is None:
            del _fp8_derived_cache[k]
            continue
        hip.quant_fp8_rows(t, out=qs)
        _fp8_derived_cache[k] = ((_cache_epoch, t._version), qs, tref)


def _wt_version(ws, scale):
    return (tuple(w._version for w in ws), tuple(w.data_ptr() for w in ws), _cache_epoch,
            (scale._version, scale.data_ptr()) if scale is not None else None)


def _transposed(ws, scale=None):
    """[sum(out_i), in] -> cached bf16 [in, sum(out_i)] (ws: one weight or a tuple that is concatenated on dim 0).
    scale (bf16 [out], one weight only): column j of the copy is scale[j] * W[j, :] -- the last Linear of a residual branch with the
    layer scale folded in, the operand of  dx = (rowscale * dout) . (gamma o W)  when the branch gradient is kept un-scaled.

    Entries are keyed by the identity of the parameter objects and validated through weak references (a freed
    parameter's address can be handed to a different tensor by the allocator) plus (_version, epoch)."""
    ws = ws if isinstance(ws, (tuple, list)) else (ws,)
    assert scale is None or len(ws) == 1
    key = tuple(id(w) for w in ws) + ((id(scale),) if scale is not None else ())
    ver = _wt_version(ws, scale)
    hit = _wt_cache.get(key)
    if hit is not None and all(r() is w for r, w in zip(hit[0], ws)) and (scale is None or (hit[3] is not None and hit[3]() is scale)):
        if hit[1] == ver:
            return hit[2]
        out = hit[2]
    else:
        out = None
        if len(_wt_cache) > 4096:  # drop entries of parameters that no longer exist
            for k in [k for k, v in _wt_cache.items() if any(r() is None for r in v[0]) or (v[3] is not None and v[3]() is None)]:
                del _wt_cache[k]
    src = ws[0] if len(ws) == 1 else torch.cat([w.detach() for w in ws], dim=0)
    t = hip.transpose(src.detach(), out, scale=scale.detach() if scale is not None else None)
    if out is not None:  # rebuilt in place through a raw pointer: tell the copies derived from it (_fp8_derived) by its version
        torch.autograd.graph.increment_version(t)
    _wt_cache[key] = (tuple(weakref.ref(w) for w in ws), ver, t, weakref.ref(scale) if scale is not None else None)
    return t


# --------------------------------------------------------------------------------------------------------------
# fp8 (e4m3) variant of the forward FFN GEMMs -- BASELINE configs[4], explicit opt-in (bench.py --config 4 --fp8)
# --------------------------------------------------------------------------------------------------------------
FP8_FFN = False
_fp8_cache = {}


FP8_FFN_DGRAD = os.environ.get("ONEPEACE_FP8_DGRAD", "1") != "0"


def set_fp8_ffn(on, dgrad=None):
    """Opt in / out of running the FFN GEMMs on fp8 e4m3 operands with per-row scales (csrc/fp8.hip): the forward up- and
    down-projection and (round 6; dgrad=False or ONEPEACE_FP8_DGRAD=0 keeps them in bf16) the two INPUT-gradient GEMMs of the backward
    -- d LN_F(g) = dy W2 and d LN2(x) = dh [W0 | W1] -- whose operands are quantised row by row (the gradient rows by op_quant_fp8_rows,
    the transposed weight copies once per optimiser step).  The WEIGHT gradients stay on the bf16 kernels and the bf16 activations."""
    global FP8_FFN, FP8_FFN_DGRAD
    old, FP8_FFN = FP8_FFN, bool(on)
    if dgrad is not None:
        FP8_FFN_DGRAD = bool(dgrad)
    return old


_fp8_derived_cache = {}


def _fp8_derived(t):
    """(fp8 bytes, row scales) of a DERIVED bf16 matrix that keeps its address across optimiser steps (a cached transposed weight copy,
    _transposed).  Quantised on first use; refresh_weight_cache re-quantises every entry IN PLACE right behind the transposes it rebuilds
    (eagerly, outside any captured graph: a replayed TrainStepGraph keeps reading these addresses and must find this step's weights);
    after invalidate_weight_cache (lazy mode) or an in-place rebuild of t (its _version: _transposed bumps it) the next use re-quantises
    into the same buffers."""
    key = (t.data_ptr(), tuple(t.shape))
    ver = (_cache_epoch, t._version)
    hit = _fp8_derived_cache.get(key)
    if hit is not None and hit[2]() is t:
        if hit[0] != ver:
            hip.quant_fp8_rows(t, out=hit[1])
            _fp8_derived_cache[key] = (ver, hit[1], hit[2])
        return hit[1]
    if hit is None and len(_fp8_derived_cache) > 4096:  # drop the entries of copies that no longer exist; live ones keep their buffers
        for k in [k for k, v in _fp8_derived_cache.items() if v[2]() is None]:
            del _fp8_derived_cache[k]
    qs = hip.quant_fp8_rows(t, out=hit[1] if hit is not None else None)
    _fp8_derived_cache[key] = (ver, qs, weakref.ref(t))
    return qs


# --------------------------------------------------------------------------------------------------------------
# memory level between "keep every activation" and the reference's checkpoint_activations
# --------------------------------------------------------------------------------------------------------------
RECOMPUTE_CHEAP = os.environ.get("ONEPEACE_RECOMPUTE_CHEAP", "0") == "1"


def set_recompute_cheap(on):
    """With save_acts=True, do NOT keep the four row matrices a LayerNorm-type pass can re-create from tensors that are kept anyway:
    LN1(x), the attention sub-LayerNorm's output, LN2(x_mid) and LN_F(gelu(h0) * h1) -- they are read only by the weight-gradient
    GEMMs.  Backward re-runs the same kernels on the same inputs (bit-identical operands, so bit-identical gradients): 14 H of the
    46 H bytes kept per token and layer = 63 GB at the headline batch (128 tuples x 571 tokens x 40 layers) for 3 LayerNorm + 1
    LN-GeGLU forward passes per layer in backward (+33 ms of a 700 ms step).  bench.py switches it on instead of halving the per-GPU
    batch when RCCL's buffers leave too little room on a multi-GPU node (pretrain_vl_3B.yaml:93 checkpoint_activations is the
    reference's only level)."""
    global RECOMPUTE_CHEAP
    old, RECOMPUTE_CHEAP = RECOMPUTE_CHEAP, bool(on)
    return old


def _fp8_weight(w):
    """(fp8 bytes, row scales) of a weight [out, in]; a derived buffer like the transposed dgrad copies, re-quantised IN PLACE when
    the weight changes (parameter version / optimiser epoch): the buffers keep their addresses."""
    key = id(w)
    ver = (w._version, w.data_ptr(), _cache_epoch)
    hit = _fp8_cache.get(key)
    if hit is not None and hit[0]() is w:
        if hit[1] != ver:
            hip.quant_fp8_rows(w.detach(), out=hit[2])
            _fp8_cache[key] = (hit[0], ver, hit[2])
        return hit[2]
    if len(_fp8_cache) > 4096:
        for k in [k for k, v in _fp8_cache.items() if v[0]() is None]:
            del _fp8_cache[k]
    qs = hip.quant_fp8_rows(w.detach())
    _fp8_cache[key] = (weakref.ref(w), ver, qs)
    return qs


_fp8_pairs = {}


def _fp8_weight_pair(w0, w1):
    """wi_0 | wi_1 as ONE fp8 matrix [2F, H] + scales [2F] (the plain N = 2F up-projection of the training forward): the two weights'
    cache entries are views of the halves, so the per-weight refresh keeps the pair current in place."""
    key = (id(w0), id(w1))
    hit = _fp8_pairs.get(key)
    if hit is None or hit[0]() is not w0 or hit[1]() is not w1:
        F0, K = w0.shape
        q = torch.empty(F0 + w1.shape[0], K, dtype=torch.uint8, device=w0.device)
        sc = torch.empty(F0 + w1.shape[0], dtype=torch.float32, device=w0.device)
        for w, lo, hi in ((w0, 0, F0), (w1, F0, q.shape[0])):
            view = (q[lo:hi], sc[lo:hi])
            hip.quant_fp8_rows(w.detach(), out=view)
            _fp8_cache[id(w)] = (weakref.ref(w), (w._version, w.data_ptr(), _cache_epoch), view)
        if len(_fp8_pairs) > 1024:
            for k in [k for k, v in _fp8_pairs.items() if v[0]() is None or v[1]() is None]:
                del _fp8_pairs[k]
        hit = _fp8_pairs[key] = (weakref.ref(w0), weakref.ref(w1), (q, sc))
    else:
        _fp8_weight(w0)
        _fp8_weight(w1)
    return hit[2]


def _round_up(n, m):
    return ((n + m - 1) // m) * m


def _t_pad(x2d):
    """[M, C] -> [C, Mpad] (Mpad = M rounded up to 64, zero tail): the K-contiguous operand of a weight-gradient GEMM."""
    M, C = x2d.shape
    Mp = _round_up(M, 64)
    out = torch.empty(C, Mp, dtype=x2d.dtype, device=x2d.device)
    if Mp != M:
        out[:, M:].zero_()
    hip.transpose(x2d, out)
    return out


_tail_pads = {}


def _tail_pad(t, rows0, operand):
    """The last len(t) - rows0 (< 64) rows of `t` as a 64-row matrix whose other rows are zero.  The buffer is cached per
    (device, stream, operand, row count, width): it is zeroed once and only its first rows are ever overwritten."""
    r, cols = t.shape[0] - rows0, t.shape[1]
    key = (t.device, torch.cuda.current_stream(t.device).cuda_stream, operand, r, cols)
    buf = _tail_pads.get(key)
    if buf is None:
        if len(_tail_pads) > 64:
            _tail_pads.clear()
        buf = _tail_pads[key] = torch.zeros(64, cols, dtype=t.dtype, device=t.device)
    buf[:r].copy_(t[rows0:])
    return buf


def wgrad_tn_rows(K):
    """Rows of a weight-gradient GEMM the transpose-read kernel takes in its main launch (it consumes 64 rows per step)."""
    return K - K % 64


def wgrad(dy, x, out=None, accumulate=False):
    """dW[out, in] (+)= dy[rows, out]^T x[rows, in].  Transpose-read GEMM straight from the row-major activations; a row count
    that is not a multiple of 64 (16 x 257 image tokens) is split into the multiple-of-64 part and a second, one-step launch
    over a zero-padded copy of the < 64 leftover rows, accumulated into the same output.  Shapes the kernel does not take
    at all (fewer than 64 rows, widths that are not multiples of 8): two transposed K-padded copies + the NT kernel."""
    K, M = dy.shape
    N = x.shape[1]
    K0 = wgrad_tn_rows(K)
    if K0 >= 64 and hip.gemm_tn_supported(K0, M, N, dy.stride(0), x.stride(0), out.stride(0) if out is not None else 0):
        out = hip.gemm_tn(dy[:K0], x[:K0], out, accumulate)
        if K0 != K:
            hip.gemm_tn(_tail_pad(dy, K0, 0), _tail_pad(x, K0, 1), out, True)
        return out
    if out is not None and accumulate:
        return out.add_(hip.gemm_nt(_t_pad(dy), [_t_pad(x)]))
    return hip.gemm_nt(_t_pad(dy), [_t_pad(x)], out=out)


# --------------------------------------------------------------------------------------------------------------
# deferred weight gradients: all dW GEMMs of an encoder layer as ONE grouped launch (csrc/gemm.hip: gemm256w_tn_grouped_kernel)
# --------------------------------------------------------------------------------------------------------------
GROUPED_WGRAD = os.environ.get("ONEPEACE_GROUPED_WGRAD", "1") != "0"
# The multiplier form of stochastic depth (the default; NOT skip_dropped_branches) sends every sample through every branch and
# multiplies a dropped sample's branch output by ps = 0; in backward that zero is the INPUT: op_resid_bwd writes ps * dout, so the rows
# of a dropped sample are zero in every gradient matrix of the branch.  "1": the weight gradients (whose K dimension is the token rows)
# run only the 64-row K-tiles that hold a row of a kept sample (hip.live_ktiles, one tiny launch per branch, the masks never leave
# the device) -- the same bits, since a +-0 product leaves an fp32 accumulator what it was; the one exception is a non-finite
# activation in a dropped sample's row (0 * inf = NaN is skipped, as with skip_dropped_branches).  "0": every tile runs (A/B, tests).
SKIP_ZERO_BACKWARD = os.environ.get("ONEPEACE_SKIP_ZERO_BACKWARD", "1") != "0"


def _live_ktiles(segs, probs, device):
    """Per problem of `probs` ([(row0, rows)]) its live K-tile list for the grouped weight-gradient launch, or None when the lists do
    not apply: switched off, no multipliers, or a row range the 64-row tiles / the samples do not tile exactly (padded segments)."""
    if not (SKIP_ZERO_BACKWARD and GROUPED_WGRAD) or all(q[0] is None for q in segs):
        return [None] * len(probs)
    if any(rows % 64 != 0 or rows < 64 for _, rows in probs) or len(segs) > 4 or len(probs) > 8:
        return [None] * len(probs)
    if any(ps is not None and (ps.dtype != torch.float32 or not ps.is_contiguous() or ps.numel() < B) for ps, _, _, B in segs):
        return [None] * len(probs)
    return hip.live_ktiles(segs, probs, device)


# The INPUT gradients of such a branch (dy W^T: the token rows are the M dimension) multiply those zero rows into zero rows.  "1": they
# run only the 256-row windows hip.live_mwindows lists (windows that start at a kept sample's first row where a sample nearly fills
# them, aligned tiles with a kept row elsewhere -- hip.mwindow_rule), one tiny launch per branch builds the lists and writes +0 into the
# rows no window covers; the last rows of S % 256 == 1 samples form strided windows of the same launch.  The same bits: a
# listed row is the dense launch's row (same operands, same K order), a dense row of zeros is +0; a non-finite gradient in a dropped
# sample's row gives 0 where the dense launch gives NaN.  "0": the dense launches (A/B, tests).
SKIP_ZERO_DGRAD = os.environ.get("ONEPEACE_SKIP_ZERO_DGRAD", "1") != "0"
_dense_dgrad_plans = {}


def _dense_dgrad_sums_k_in_one_piece(M, N, K, device):
    """Does hip.gemm_nt run this input gradient without a K-split (main launch and tail rows)?  Only then a listed window, which never
    splits, has the dense launch's bits.  (Training shapes: yes -- the planner splits K for launches of a few M-tiles.)  The scratch is
    the one that launch would get, at its size of this moment."""
    scratch = hip.splitk_scratch(M, N, K, hip.EPI_BIAS, device)
    ws = scratch.numel() if scratch is not None else 0
    key = (M, N, K, ws, hip.TUNE.gemm())
    if key not in _dense_dgrad_plans:
        _, splits, _, tail = hip.gemm_plan(M, N, K, hip.EPI_BIAS, False, ws)
        _dense_dgrad_plans[key] = splits == 1 and (tail == 0 or hip.gemm_plan(tail, N, K, hip.EPI_BIAS, False, ws)[1] == 1)
    return _dense_dgrad_plans[key]


def _dgrad_windows(segs, lists, outs, dense, unread=()):
    """hip.live_mwindows' lists for the input gradients of a branch, or None when they do not apply: switched off, no multipliers, a
    shape the persistent kernel does not take, or a dense launch ([(M, N, K)], the per-problem launches the lists replace) that would
    split K.  segs: [(ps, row0, S, B, ps stride)].  unread: outputs whose ONLY reader leaves out the rows of dropped samples when the
    lists apply and SKIP_ZERO_ROWS is on (the caller passes it ps) -- they get no +0 rows then; with the switch off they are filled
    like `outs`."""
    outs = list(outs) + ([] if SKIP_ZERO_ROWS else list(unread))
    every = outs + (list(unread) if SKIP_ZERO_ROWS else [])
    if not SKIP_ZERO_DGRAD or all(q[0] is None for q in segs) or len(segs) > 4 or len(lists) > 4 or len(every) > 4:
        return None
    if any(N % 256 != 0 or K % 64 != 0 or K < 128 or not _dense_dgrad_sums_k_in_one_piece(M, N, K, every[0].device) for M, N, K in dense):
        return None
    if any(ps is not None and (ps.dtype != torch.float32 or not ps.is_contiguous() or ps.numel() <= (B - 1) * st) for ps, _, _, B, st in segs):
        return None
    if any(o.dtype != torch.bfloat16 or o.stride(0) % 8 != 0 or o.shape[1] % 8 != 0 for o in every):
        return None
    return hip.live_mwindows(segs, lists, outs)


def _bwd_fills(pairs):
    """(outs, unread) of _dgrad_windows from [(output or None, does its ONLY reader take the multipliers?)]: an output whose reader
    skips the rows of dropped samples needs no +0 rows (DESIGN.md section 4.4 has the readers).
    Attention branch: d subLN(attn) -- the sub-LayerNorm's backward skips; without a sub-LayerNorm the dense attention backward reads
    it --, d LN1(x) -- LN1's backward skips.  FFN branch: d LN_F(g) -- op_ln_geglu_bwd skips; without LN_F the dense op_geglu_bwd
    reads it --, d LN2(x) -- LN2's backward runs over ALL rows with one (ps, rows per sample) pair: it skips in a one-segment branch."""
    pairs = [(o, skips) for o, skips in pairs if o is not None]
    return [o for o, skips in pairs if not skips], [o for o, skips in pairs if skips]


def _dgrad_listed(As, Ws, outs, windows, segs):
    """outs[p] = As[p] Ws[p]^T over a window list built for `segs`.  False: nothing launched (the caller runs the dense launch)."""
    return hip.gemm_nt_windows(As, Ws, outs, windows, max([sg.S for sg in segs if hip.mwindow_rule(sg.S)[1]] or [1]))


# The FORWARD GEMMs of such a branch (q|k|v, out-proj + residual; wi_0|wi_1, down-projection + residual) multiply every row of a dropped
# sample, and the epilogue or a later kernel multiplies the result by ps = 0.  "1": they run over the same kind of window lists
# (hip.live_mwindows_fwd: one launch per branch builds the list and FILLS the rows no window covers -- +0 in q|k|v and h0|h1, a copy of
# the residual input in the branch output, which is what fma(0, y, res) gives).  A listed row is the dense launch's row (same operands,
# same K order, same epilogue); a -0 element of a dropped sample's residual stays -0 where the dense epilogue can give +0, and a non-finite
# y in a dropped row no longer becomes NaN: equal as numbers, as the backward lists.  Attention and the forward LayerNorms stay dense and
# read zeros or real rows for a dropped sample; the other row kernels: SKIP_ZERO_ROWS below.  "0": the dense launches (A/B, tests).  Independent of SKIP_ZERO_DGRAD / SKIP_ZERO_BACKWARD.
SKIP_ZERO_FWD = os.environ.get("ONEPEACE_SKIP_ZERO_FWD", "1") != "0"
_dense_fwd_plans = {}
# The ROW kernels between those GEMMs (LayerNorm_F(GeGLU) forward and backward, the LayerNorm backwards, op_resid_bwd) ran over every row:
# a dropped sample's rows were zeros a fill had written for them to read, or values a later kernel multiplies by exact zeros.  "1":
# where the window lists of a branch and direction apply, those kernels get the multipliers and read NOTHING of a dropped sample's
# row (hip.ln_geglu_fwd / ln_geglu_bwd / layernorm_bwd: ps; hip.resid_bwd: skip_zero_rows) -- they store what the dense kernel makes of
# the exact-zero row it would have read (+0; the residual gradient where a LayerNorm backward adds one; LN_F(GeGLU) forward +0 instead
# of its bias row, which every reader multiplies by zero) -- and the fills no longer write the rows only such a kernel reads: h0 | h1
# in forward, the input-gradient outputs in backward (DESIGN.md section 4.4 has the table of who writes and who reads every row).
# Decided from shapes and flags alone, so the forward, its recomputation and the backward agree.  "0": the launches and fills as
# before (A/B, tests).  Independent of the three switches above; never with the fp8 route, row tables (`kept`) or padded segments,
# where the lists do not apply either.
SKIP_ZERO_ROWS = os.environ.get("ONEPEACE_SKIP_ZERO_ROWS", "1") != "0"


def _dense_fwd_sums_k_in_one_piece(M, N, K, epilogue, has_bias, device):
    """_dense_dgrad_sums_k_in_one_piece for a forward launch of hip.gemm_nt with its own epilogue."""
    scratch = hip.splitk_scratch(M, N, K, epilogue, device)
    ws = scratch.numel() if scratch is not None else 0
    key = (M, N, K, epilogue, has_bias, ws, hip.TUNE.gemm())
    if key not in _dense_fwd_plans:
        _, splits, _, tail = hip.gemm_plan(M, N, K, epilogue, has_bias, ws)
        _dense_fwd_plans[key] = splits == 1 and (tail == 0 or hip.gemm_plan(tail, N, K, epilogue, has_bias, ws)[1] == 1)
    return _dense_fwd_plans[key]


def _fwd_windows_apply(segs, nlists, nouts, dense, device, flags=True):
    """Do window lists serve the forward launches of a branch?  Decided from shapes and flags alone (the forward and its recomputation
    agree): switched on, `flags` (the caller's: no row tables, no branch output, no fp8, no padded segment), some segment has
    multipliers, shapes the persistent kernel and the list format take, and no dense launch ([(M, N, K, epilogue, has_bias)], the
    hip.gemm_nt launches the lists replace) that splits K.  segs: [(ps, row0, S, B, ps stride)]."""
    if not SKIP_ZERO_FWD or not flags or all(q[0] is None for q in segs) or len(segs) > 4 or nlists > 4 or nouts > 4:
        return False
    if any(ps is not None and (ps.dtype != torch.float32 or not ps.is_contiguous() or ps.numel() <= (B - 1) * st) for ps, _, _, B, st in segs):
        return False
    if any(S * B >= 1 << 27 or row0 + S * B + 256 * 64 >= 1 << 28 for _, row0, S, B, _ in segs):
        return False
    mrs = max([q[2] for q in segs if hip.mwindow_rule(q[2])[1]] or [1])
    for M, N, K, epi, has_bias in dense:
        if N % 256 != 0 or K % 64 != 0 or K < 128 or M * max(N, K) >= 1 << 30 or mrs * max(N, K) >= 1 << 23:
            return False
        if not _dense_fwd_sums_k_in_one_piece(M, N, K, epi, has_bias, device):
            return False
    return True


class _WgradQueue:
    """Weight-gradient GEMMs that accumulate into flat gradient views, collected while a layer's backward runs (FFN branch
    first, then the attention branch, which flushes): launched alone each of them has 36 ... 288 output tiles for 256 CUs and
    needs split-K slabs + a fold; together they are 1440 tiles for one persistent launch without split-K.  The operands are
    kept alive until the launch is enqueued; the reducer hears about a parameter only after that."""

    def __init__(self):
        self.items, self.done, self.after, self.armed, self.epoch = [], [], [], False, 0
        self.lists = []  # per item: hip.live_ktiles' (list, count) or None

    def reset(self):
        """Forget everything a backward pass that raised left behind (the engine does not run queue_callback callbacks then):
        stale operands must not be accumulated into the freshly zeroed gradients of the next step, and the end-of-backward
        safety net has to be registered again.  Called by distributed.FlatParameters.zero_grad / BucketedGradReducer.reset."""
        self.items, self.done, self.after, self.armed = [], [], [], False
        self.lists = []
        self.epoch += 1

    @staticmethod
    def _span(out):
        """Byte range [lo, hi) an output view covers in its storage (rows may be strided)."""
        lo = out.data_ptr()
        return lo, lo + ((out.shape[0] - 1) * out.stride(0) + out.shape[1]) * out.element_size()

    def add(self, dy, x, out, params, side=None, after=None, ktiles=None):
        """side: (W, rowdot [N / 128, M], gamma) -- `dy` carries NO layer scale: the launch adds gamma[m] * product[m] to out[m] and writes the
        partial sums of W[m][n] * product[m][n] over 128-column slots to rowdot (hip.gemm_tn_grouped: rscale);
        after: called once the launch that holds this problem is enqueued (before the parameters are reported);
        ktiles: (list, count) of _live_ktiles -- the rows of dy outside those 64-row tiles are zero."""
        lo, hi = self._span(out)
        for it in self.items:  # the grouped launch read-modify-writes C tiles without ordering between problems: two
            l2, h2 = self._span(it[2])  # contributions to one (overlapping) view go out as two launches, stream-ordered
            if lo < h2 and l2 < hi:
                self.flush()
                break
        self.items.append((dy, x, out, True, side))
        self.lists.append(ktiles)
        self.done.extend(params)
        if after is not None:
            self.after.append(after)
        if not self.armed:  # safety net: whatever is still queued when autograd finishes this backward pass goes out then
            self.armed = True
            epoch = self.epoch
            torch.autograd.Variable._execution_engine.queue_callback(lambda: self._end_of_backward(epoch))
        if len(self.items) >= hip.TN_GROUP_MAX:
            self.flush()

    def _end_of_backward(self, epoch):
        if epoch != self.epoch:  # a reset() came in between: this callback belongs to an abandoned pass
            return
        self.armed = False
        self.flush()

    def flush(self):
        items, done, after, lists = self.items, self.done, self.after, self.lists
        self.items, self.done, self.after, self.lists = [], [], [], []
        if items:
            kw = {"ktiles": lists} if any(k is not None for k in lists) else {}
            if len(items) == 1 or not hip.gemm_tn_grouped(items, **kw):  # a lone problem keeps the split-K launch of op_gemm_tn
                for dy, x, out, _, side in items:
                    if side is None:
                        hip.gemm_tn(dy, x, out, True)
                    else:  # (rare: the side product rides on the grouped launch only) the product once, used twice
                        prod = hip.gemm_tn(dy, x, None, False)
                        W, rowdot, gamma = side
                        out.addcmul_(prod, gamma.detach().unsqueeze(1))
                        rowdot.zero_()  # [slots, M]: the whole row dot goes into slot 0
                        for r0 in range(0, prod.shape[0], 256):  # (row blocks: no fp32 copies of whole matrices)
                            rowdot[0, r0:r0 + 256] = (W.detach()[r0:r0 + 256].float() * prod[r0:r0 + 256].float()).sum(1)
        for f in after:
            f()
        for q in done:
            _direct_grad_done(q)


_wgrad_queue = _WgradQueue()


def _wgrad_queueable(K, M, N, ldy, ldx, grad_view):
    return (GROUPED_WGRAD and K % 64 == 0 and K >= 64 and grad_view.stride(0) % 8 == 0 and grad_view.stride(1) == 1
            and grad_view.data_ptr() % 16 == 0  # op_gemm_tn_grouped's rule for C: ldc % 8 == 0, 16-byte aligned (else launch now)
            and hip.gemm_tn_supported(K, M, N, ldy, ldx))


def wgrad_into(dy, x, grad_view, params, side=None, after=None, ktiles=None):
    """grad_view (+)= dy^T x for the flat-buffer gradient views of `params` (one view spanning all of them).  Deferred into the
    layer's grouped launch when the shape allows, else launched now; either way every parameter's completion is signalled.
    side / after: see _WgradQueue.add (the caller has checked dgamma_from_wgrad_ok: the problem IS queueable)."""
    K, M = dy.shape
    if _wgrad_queueable(K, M, x.shape[1], dy.stride(0), x.stride(0), grad_view):
        _wgrad_queue.add(dy, x, grad_view, params, side, after, ktiles)
        return
    assert side is None and after is None, "wgrad_into: a side product was promised for a problem the grouped launch does not take"
    wgrad(dy, x, out=grad_view, accumulate=True)
    for q in params:
        _direct_grad_done(q)


# --------------------------------------------------------------------------------------------------------------
# layer-scale gradient without the branch output (round 5)
# --------------------------------------------------------------------------------------------------------------
# out = resid + ps * gamma * y with y = x W^T + b (transformer_layer.py:70-88).  dgamma[n] = sum_m ps dout[m][n] y[m][n] needs y in
# backward -- a second output of the residual GEMM (its epilogue then moves three times the bytes of a plain launch) that is kept for
# backward (2 H bytes per token and branch) and read again by op_resid_bwd.  But
#     dgamma[n] = sum_k W[n][k] * G[n][k] + b[n] * g0[n],     G = (ps dout)^T x,   g0 = sum_m ps dout,
# and the weight gradient the step computes anyway is dW = gamma[n] * G.  (Round 6) The branch gradient op_resid_bwd writes is
# u = ps dout WITHOUT gamma; the grouped weight-gradient launch multiplies u^T x = G (its fp32 accumulators) with W into a row vector
# -- that IS the first term, for any gamma including 0 -- and adds gamma[n] * G to the bf16 gradient; the input gradient
# u . (gamma o W) reads a gamma-scaled transposed copy of W (rebuilt with the others after every optimiser step).  Round 5 fed the
# launch the gamma-scaled gradient and divided the row vector by gamma: wrong (0) where gamma == 0.  y is neither written nor kept.
DGAMMA_FROM_WGRAD = os.environ.get("ONEPEACE_DGAMMA_FROM_WGRAD", "1") != "0"


def _rowdot_slots(device, weights):
    """The side-product buffer of a branch: fp32 [sum_i in_i / 128, out] -- weight i ([out, in_i]: the last Linear of one weight set
    that shares gamma) owns in_i / 128 consecutive slots, each written exactly once by the grouped launch (no zeroing, no atomics).
    Returns (buffer, [per-weight [in_i / 128, out] views])."""
    n = [w.shape[1] // 128 for w in weights]
    buf = torch.empty(sum(n), weights[0].shape[0], dtype=torch.float32, device=device)
    views, off = [], 0
    for k in n:
        views.append(buf[off:off + k])
        off += k
    return buf, views


def dgamma_from_wgrad_ok(rows, gamma, weights, biases, needs_g, needs_w):  # rows: per weight, the token rows of its gradient GEMM
    """Forward-time decision (it fixes whether the branch output is written at all): gamma and every last-Linear weight / bias of the
    branch accumulate in place in the flat gradient buffer, all of them want a gradient, and the weight gradients will ride on the
    grouped launch with full 256 x 256 tiles."""
    if not (DGAMMA_FROM_WGRAD and needs_g and all(needs_w) and gamma is not None and _direct_grad(gamma) and gamma.dtype == torch.bfloat16):
        return False
    for k, w in zip(rows, weights):
        if not (_direct_grad(w) and w.is_contiguous() and w.shape[0] % 256 == 0 and w.shape[1] % 256 == 0 and w.data_ptr() % 16 == 0
                and _wgrad_queueable(k, w.shape[0], w.shape[1], w.shape[0], w.shape[1], w.grad)):
            return False
    return all(b is None or _direct_grad(b) for b in biases)


def flush_wgrads():
    _wgrad_queue.flush()


def reset_wgrads():
    """Drop weight-gradient problems a failed backward pass left queued (see _WgradQueue.reset)."""
    _wgrad_queue.reset()


def _direct_grad(param):
    """True when `param` lives in distributed.FlatParameters: its .grad is a pre-allocated, pre-zeroed view the weight
    gradient GEMM can accumulate into directly (no autograd accumulation pass, no temporary dW tensor)."""
    return getattr(param, "_op_flat", False) and param.grad is not None


def _direct_grad_done(param):
    """One backward contribution to a directly accumulated gradient finished; the last one notifies the reducer."""
    left = getattr(param, "_op_pending", 1) - 1
    param._op_pending = left
    if left <= 0:
        cb = getattr(param, "_op_on_final", None)
        if cb is not None:
            cb(param)


def gemm_any(A, W, bias=None, out_f32=False, alpha=None):
    """A[M,K] @ W[N,K]^T (+bias) through the HIP GEMM for ANY K, N (zero-pads K to 64 / N to 8 on the host)."""
    M, K = A.shape
    N = W.shape[0]
    Kp, Np = _round_up(K, 64), _round_up(N, 8)
    if Kp != K:
        A = torch.nn.functional.pad(A, (0, Kp - K))
        W = torch.nn.functional.pad(W, (0, Kp - K))
    if Np != N:
        W = torch.nn.functional.pad(W, (0, 0, 0, Np - N))
        if bias is not None:
            bias = torch.nn.functional.pad(bias, (0, Np - N))
    A = A.contiguous()
    W = W.contiguous()
    if out_f32:
        out = hip.gemm_nt(A, [W], [bias] if bias is not None else None, epilogue=hip.EPI_F32, alpha=alpha)
    else:
        out = hip.gemm_nt(A, [W], [bias] if bias is not None else None)
    return out if Np == N else out[:, :N].contiguous()


def hip_eligible(x):
    """The HIP path takes bf16 CUDA tensors; anything else runs the torch reference ops of the mirrors."""
    return x.is_cuda and x.dtype == torch.bfloat16


# --------------------------------------------------------------------------------------------------------------
# retrieval: k best gallery rows per query (metrics/recall.py:31-51 without the score matrix)
# --------------------------------------------------------------------------------------------------------------
def similarity_topk(query, gallery, k, splits=None):
    """(scores fp32 [M, k] descending, indices int64 [M, k]) of the k largest query[m] . gallery[n].  Exact ties: lower n first;
    NaN ranks above +inf.  bf16 CUDA inputs run op_sim_topk (hip.sim_topk), which never forms the [M, N] scores; anything else
    computes fp32 scores and a stable descending sort -- the same order."""
    if hip_eligible(query) and hip_eligible(gallery):
        return hip.sim_topk(query, gallery, k, splits=splits)
    if not 1 <= k <= gallery.shape[0]:
        raise ValueError("similarity_topk: need 1 <= k <= N, got k = %d, N = %d" % (k, gallery.shape[0]))
    scores = query.float() @ gallery.float().t()
    scores = torch.where(scores == 0, torch.zeros_like(scores), scores)  # -0 ties with +0, as in the kernel's key
    vals, idx = torch.sort(scores, dim=1, descending=True, stable=True)
    return vals[:, :k].contiguous(), idx[:, :k].contiguous()


# --------------------------------------------------------------------------------------------------------------
# classification: average precision per class (metrics/map.py:35-44 without the host copy, the host sorts and sklearn)
# --------------------------------------------------------------------------------------------------------------
def _average_precision_torch(scores, positive):
    """The formula of op_average_precision in torch: a stable descending sort per class, integer cumulative counts, fp64 quotients.
    A position's threshold is the LAST position of its run of equal scores: CNT = that position (1-based), TP = the positives up to it."""
    N, C = scores.shape
    v, order = torch.sort(scores, dim=0, descending=True, stable=True)
    y = positive.gather(0, order).long()
    tp_upto = torch.cumsum(y, dim=0)
    pos = torch.arange(1, N + 1, device=scores.device).unsqueeze(1).expand(N, C)
    last = torch.ones(N, C, dtype=torch.bool, device=scores.device)
    last[:-1] = v[:-1] != v[1:]  # +-inf and -0 / +0 compare as values
    ends = torch.where(last, pos, torch.full_like(pos, N))
    cnt = torch.flip(torch.cummin(torch.flip(ends, (0,)), dim=0)[0], (0,))  # the nearest run end at or after each position
    tp = tp_upto.gather(0, cnt - 1)
    terms = torch.where(y.bool(), tp.double() / cnt.double(), torch.zeros((), dtype=torch.float64, device=scores.device))
    npos = y.sum(0)
    ap = torch.where(npos > 0, terms.sum(0) / npos.clamp(min=1).double(), torch.zeros((), dtype=torch.float64, device=scores.device))
    return ap, npos


def average_precision(scores, targets):
    """(ap fp64 [C], npos int64 [C]): per class c the average precision of scores[:, c] against the binary targets[:, c], as sklearn's
    average_precision_score(targets, scores, average=None) defines it -- the mean over the positives i of
    #{positives scoring >= s_i} / #{samples scoring >= s_i}, tied scores sharing one threshold; 0.0 for a class without positives.
    scores fp32 / bf16 / fp16 (cast to fp32 first), targets bool / integer (non-zero = positive) / float (0 or 1).  ValueError, as
    sklearn raises: different shapes, a NaN score, a float target other than 0 or 1.  CUDA inputs run op_average_precision
    (hip.average_precision: the [N, C] scores never leave the device; one sync for the checks); anything else the torch statement of
    the same formula."""
    if scores.dim() != 2 or tuple(scores.shape) != tuple(targets.shape):
        raise ValueError("average_precision: scores and targets must be [N, C] of one shape, got %s and %s" % (
            tuple(scores.shape), tuple(targets.shape)))
    if scores.shape[0] < 1 or scores.shape[1] < 1:
        raise ValueError("average_precision: need N >= 1 and C >= 1, got %s" % (tuple(scores.shape),))
    if not scores.is_floating_point():
        raise ValueError("average_precision: scores must be floating point, got %s" % scores.dtype)
    targets = targets.to(scores.device)
    scores = scores.float()
    bad_target = ((targets != 0) & (targets != 1)).any() if targets.is_floating_point() else torch.zeros((), dtype=torch.bool, device=scores.device)
    has_nan, bad_target = torch.stack([torch.isnan(scores).any(), bad_target]).tolist()
    if has_nan:
        raise ValueError("average_precision: scores contain NaN")
    if bad_target:
        raise ValueError("average_precision: float targets must be 0 or 1")
    positive = targets != 0
    if scores.is_cuda:
        ap, npos = hip.average_precision(scores, positive.to(torch.uint8))
        return ap, npos.long()
    return _average_precision_torch(scores, positive)


# --------------------------------------------------------------------------------------------------------------
# image pre-processing: hub_interface.py:94-101 (Resize((S, S), BICUBIC), ToTensor, Normalize) on decoded images
# --------------------------------------------------------------------------------------------------------------
def _is_pil(im):
    return type(im).__module__.startswith("PIL.") and hasattr(im, "convert")


def preprocess_images(images, size, mean=None, std=None, dtype=torch.float32, device="cpu", crops=None, center_crop=False, flips=None,
                      jitter=None, blur=None, randaug=None):
    """[B, 3, size, size] in `dtype` on `device` from decoded RGB images (uint8 [H, W, 3] arrays / tensors or PIL images of any
    size): PIL's Image.resize((size, size), BICUBIC), ToTensor and Normalize (CLIP mean / std by default) in torchvision's fp32
    order, then the cast -- the reference's transform, bit for bit.  On a CUDA device this is op_image_resize_normalize
    (hip.image_resize_normalize: one H2D copy of the uint8 pixels, resize and normalisation on the GPU; PIL is not needed for
    arrays); on the CPU it is PIL itself and the same torch arithmetic (the reference's own path).

    The geometry of the training / evaluation transforms rides on the same pass.  crops: one (top, left, h, w) per image
    (torchvision's F.resized_crop order; imageprep.random_resized_crop_params draws RandomResizedCrop's), the box is resized instead of
    the image.  center_crop=True: torchvision's Resize(size) + CenterCrop(size) (shorter side to size, the longer to
    int(size * long / short), window at int(round((n - size) / 2.0))); exclusive with crops.  flips: one bool per image,
    RandomHorizontalFlip, applied last as in the reference's Compose.  A box outside its image or with h or w < 1 is a ValueError
    before anything is copied.

    The photometric steps of the train transforms sit between the resize and ToTensor.  jitter: the (ops, factors) tables of
    color_jitter (RandomDistortion / ColorJitter; augment.ColorJitter.params draws them); blur: one GaussianBlur radius per image, None
    or <= 0 for an image that is not blurred (augment.GaussianBlur.params).  With either, the device route is the resize to uint8
    [B, size, size, 3], op_image_color_jitter, op_image_gaussian_blur and op_image_normalize_flip with the flips; the CPU route is the same
    chain in PIL, in the reference's Compose order (resize, distortion, blur, flip).  With both None the path and the results are those
    of the plain resize.

    randaug: the (ops, args, fill) tables of rand_augment (augment.RandAugment.params draws them), timm's create_transform order
    (image_classify_dataset.py:65-77): the flip comes BEFORE RandAugment.  The device route is the resize to uint8 with the flips inside
    the resize pass, rand_augment, then op_image_normalize_flip without flips; the CPU route the same order in PIL.  Together with
    jitter or blur it is a ValueError (timm drops the colour jitter when auto_augment is set, and the two positions of the flip must not
    be mixed).  With randaug=None the paths and the results are those described above."""
    import numpy as np

    from . import imageprep
    mean = imageprep.CLIP_MEAN if mean is None else tuple(mean)
    std = imageprep.CLIP_STD if std is None else tuple(std)
    imageprep.check_size(size)
    if crops is not None and center_crop:
        raise ValueError("preprocess_images: crops and center_crop are mutually exclusive")
    images = list(images)
    if crops is not None:
        hw = [(im.size[1], im.size[0]) if _is_pil(im) else tuple(im.shape[:2]) for im in images]
        crops = imageprep.check_crops(crops, hw)
    if flips is not None:
        flips = imageprep.check_flips(flips, len(images))
    photometric = jitter is not None or blur is not None
    if randaug is not None:
        if photometric:
            raise ValueError("preprocess_images: randaug excludes jitter and blur (timm's create_transform drops the colour jitter with auto_augment)")
        randaug = imageprep.check_randaug(randaug, len(images))
    if jitter is not None:
        jitter = imageprep.check_jitter(jitter, len(images))
    if blur is not None:
        blur_radii = list(blur.tolist() if hasattr(blur, "tolist") else blur)
        blur = imageprep.blur_table(blur_radii)  # (validates; the device route's tables)
        if len(blur[0]) != len(images):
            raise ValueError("blur: need one radius per image, got %d for %d images" % (len(blur[0]), len(images)))
    dev = torch.device(device)
    if dev.type == "cuda":
        arrs = [np.asarray(im.convert("RGB")) if _is_pil(im) else im for im in images]
        kdt = dtype if dtype in (torch.bfloat16, torch.float32) else torch.float32
        if randaug is not None:
            packed = imageprep.pack_images(arrs, size, crops=crops, center_crop=center_crop, flips=flips)
            u8 = hip.image_resize_normalize(packed, dtype=torch.uint8, device=dev)
            return hip.image_normalize_flip(_rand_augment_device(u8, *randaug), mean, std, kdt, None).to(dtype)
        if photometric:
            packed = imageprep.pack_images(arrs, size, crops=crops, center_crop=center_crop)
            u8 = hip.image_resize_normalize(packed, dtype=torch.uint8, device=dev)
            if jitter is not None:
                hip.image_color_jitter(u8, *jitter)
            if blur is not None:
                hip.image_gaussian_blur(u8, *blur)
            return hip.image_normalize_flip(u8, mean, std, kdt, flips).to(dtype)
        packed = imageprep.pack_images(arrs, size, crops=crops, center_crop=center_crop, flips=flips)
        return hip.image_resize_normalize(packed, mean, std, kdt, dev).to(dtype)
    from PIL import Image
    out = []
    for i, im in enumerate(images):
        im = im.convert("RGB") if _is_pil(im) else Image.fromarray(imageprep.as_rgb_array(im))
        if crops is not None:
            top, left, h, w = crops[i]
            im = im.crop((left, top, left + w, top + h)).resize((size, size), Image.BICUBIC)
        elif center_crop:
            new_h, new_w, top, left = imageprep.center_crop_geometry(im.size[1], im.size[0], size)
            im = im.resize((new_w, new_h), Image.BICUBIC).crop((left, top, left + size, top + size))
        else:
            im = im.resize((size, size), Image.BICUBIC)
        if jitter is not None:
            im = _pil_jitter(im, jitter[0][i], jitter[1][i])
        if blur is not None and blur[3][i]:
            im = _pil_blur(im, blur_radii[i])
        if flips is not None and flips[i]:
            im = im.transpose(Image.FLIP_LEFT_RIGHT)
        if randaug is not None:
            for op, arg in zip(randaug[0][i], randaug[1][i]):
                im = _pil_randaug(im, op, arg, randaug[2])
        u8 = torch.from_numpy(np.array(im, dtype=np.uint8))
        out.append(imageprep.to_tensor_normalize(u8, mean, std))
    return torch.stack(out).to(device=dev, dtype=dtype) if out else torch.empty(0, 3, size, size, dtype=dtype, device=dev)


# --------------------------------------------------------------------------------------------------------------
# photometric train transforms on the resized uint8 batch: RandomDistortion / ColorJitter (utils/transforms.py:144-157) and GaussianBlur
# (utils/transforms.py:160-188), then ToTensor / Normalize / flip
# --------------------------------------------------------------------------------------------------------------
def _pil_jitter(im, ops, factors):
    """torchvision's ColorJitter steps on a PIL image: ImageEnhance.Brightness / Contrast / Color in the order of `ops`."""
    from PIL import ImageEnhance
    enhancers = {1: ImageEnhance.Brightness, 2: ImageEnhance.Contrast, 3: ImageEnhance.Color}
    for op, f in zip(ops, factors):
        if int(op) != 0:
            im = enhancers[int(op)](im).enhance(float(f))
    return im


def _pil_blur(im, radius):
    from PIL import ImageFilter
    return im.filter(ImageFilter.GaussianBlur(radius=float(radius)))


def _u8_images(u8, what):
    if not torch.is_tensor(u8) or u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
        raise ValueError("%s: need a uint8 [B, H, W, 3] tensor" % what)
    if u8.is_cuda:
        from . import imageprep
        if u8.shape[1] != u8.shape[2]:
            raise ValueError("%s: a device batch must be square, got %s" % (what, tuple(u8.shape)))
        if u8.shape[0]:
            imageprep.check_size(u8.shape[1])
        if not u8.is_contiguous():
            raise ValueError("%s: a device batch must be contiguous (the kernels work in place)" % what)


def _pil_each(u8, fn):
    """u8[i] = fn(i, PIL image of u8[i]) for a CPU batch, in place."""
    import numpy as np
    from PIL import Image
    for i in range(u8.shape[0]):
        im = fn(i, Image.fromarray(u8[i].contiguous().numpy()))
        if im is not None:
            u8[i] = torch.from_numpy(np.array(im, dtype=np.uint8))
    return u8


def color_jitter(u8, ops, factors):
    """ColorJitter IN PLACE on u8 = uint8 [B, S, S, 3]; returns u8.  ops int [B, 3]: the chain of image i in the order it is applied (0 none,
    1 brightness, 2 contrast, 3 saturation: imageprep.JITTER_OPS / jitter_table); factors [B, 3]: the enhancement factors, finite and
    >= 0.  Each step is PIL's ImageEnhance (what torchvision's ColorJitter runs on a PIL image), bit for bit: on a CUDA device
    op_image_color_jitter (S a multiple of 16 in [16, 1024]), on the CPU PIL itself.  Hue is not provided (the reference passes hue = 0)."""
    from . import imageprep
    _u8_images(u8, "color_jitter")
    tab_ops, tab_f = imageprep.check_jitter((ops, factors), u8.shape[0])
    if u8.is_cuda:
        return hip.image_color_jitter(u8, tab_ops, tab_f)
    return _pil_each(u8, lambda i, im: _pil_jitter(im, tab_ops[i], tab_f[i]) if tab_ops[i].any() else None)


def gaussian_blur(u8, radii):
    """ImageFilter.GaussianBlur(radius) IN PLACE on u8 = uint8 [B, S, S, 3]; returns u8.  radii: one per image, None or <= 0 = not blurred.
    On a CUDA device op_image_gaussian_blur (S a multiple of 16 in [16, 1024]; radii up to a box radius of 32, i.e. ~33), on the CPU PIL
    itself; bit for bit the same."""
    from . import imageprep
    _u8_images(u8, "gaussian_blur")
    radii = list(radii.tolist() if hasattr(radii, "tolist") else radii)
    if len(radii) != u8.shape[0]:
        raise ValueError("gaussian_blur: need one radius per image, got %d for %d images" % (len(radii), u8.shape[0]))
    table = imageprep.blur_table(radii)
    if u8.is_cuda:
        return hip.image_gaussian_blur(u8, *table)
    return _pil_each(u8, lambda i, im: _pil_blur(im, radii[i]) if table[3][i] else None)


def normalize_images(u8, mean=None, std=None, dtype=torch.float32, flips=None):
    """[B, 3, S, S] in `dtype` from u8 = uint8 [B, S, S, 3]: ToTensor and Normalize in torchvision's fp32 order ((u / 255 - mean) / std, CLIP
    mean / std by default), RandomHorizontalFlip where flips[i] is set, then the cast.  On a CUDA device op_image_normalize_flip -- the
    store of the resize kernel, so both routes share one arithmetic -- on the CPU imageprep.to_tensor_normalize."""
    from . import imageprep
    _u8_images(u8, "normalize_images")
    mean = imageprep.CLIP_MEAN if mean is None else tuple(mean)
    std = imageprep.CLIP_STD if std is None else tuple(std)
    if flips is not None and not (u8.is_cuda and torch.is_tensor(flips) and flips.is_cuda):  # (flags already on the device stay there)
        flips = imageprep.check_flips(flips, u8.shape[0])
    if u8.is_cuda:
        kdt = dtype if dtype in (torch.bfloat16, torch.float32) else torch.float32
        return hip.image_normalize_flip(u8, mean, std, kdt, flips).to(dtype)
    if flips is not None and any(flips):
        u8 = torch.where(torch.tensor(flips).view(-1, 1, 1, 1), u8.flip(2), u8)
    return imageprep.to_tensor_normalize(u8, mean, std).to(dtype)


# --------------------------------------------------------------------------------------------------------------
# RandAugment and RandomErasing of timm's create_transform (data/vision_data/image_classify_dataset.py:65-77; augment.RandAugment /
# augment.RandomErasing draw the tables)
# --------------------------------------------------------------------------------------------------------------
def _pil_randaug(im, op, arg, fill):
    """One RandAugment op of timm's auto_augment.py on a PIL RGB image, by its code (imageprep.RANDAUG_OPS): the Pillow calls timm makes."""
    from PIL import Image, ImageEnhance, ImageOps
    op = int(op)
    if op == 0:
        return im
    if op == 1:
        return ImageOps.autocontrast(im)
    if op == 2:
        return ImageOps.equalize(im)
    if op == 3:
        return ImageOps.invert(im)
    if op == 4:
        return ImageOps.posterize(im, int(arg[0]))
    if op == 5:
        return ImageOps.solarize(im, int(arg[0]))
    if op == 6:
        lut = [min(255, i + int(arg[0])) if i < 128 else i for i in range(256)]
        return im.point(lut + lut + lut)
    if op in (7, 8, 9, 10):
        enhancer = {7: ImageEnhance.Color, 8: ImageEnhance.Contrast, 9: ImageEnhance.Brightness, 10: ImageEnhance.Sharpness}[op]
        return enhancer(im).enhance(float(arg[0]))
    if op == 11:
        return im.transform(im.size, Image.AFFINE, tuple(float(v) for v in arg), resample=Image.BICUBIC, fillcolor=tuple(fill))
    raise ValueError("rand_augment: unknown op code %d" % op)


def _rand_augment_device(u8, tab_ops, tab_args, fill):
    """The layers of validated tables on a device batch: per layer op_image_randaug_layer for its own ops and op_image_color_jitter, with
    a one-op chain, for the images whose op is Color / Contrast / Brightness.  An image has one op per layer, so the two calls of a
    layer touch different images."""
    import numpy as np

    from . import imageprep
    B = u8.shape[0]
    if B == 0 or not tab_ops.any():
        return u8
    scratch = torch.empty_like(u8) if (tab_ops == 10).any() or (tab_ops == 11).any() else u8.new_empty(0)
    for layer in range(tab_ops.shape[1]):
        ops_l, args_l = tab_ops[:, layer], tab_args[:, layer]
        enhance = (ops_l >= 7) & (ops_l <= 9)
        own = np.where(enhance, 0, ops_l).astype(np.int32)
        if own.any():
            if scratch.numel() == 0:  # (the entry wants a scratch even when no op of the layer writes it)
                scratch = torch.empty_like(u8)
            hip.image_randaug_layer(u8, own, args_l, fill, scratch)
        if enhance.any():
            chain = np.zeros((B, 3), dtype=np.int32)
            factors = np.ones((B, 3), dtype=np.float32)
            chain[enhance, 0] = [imageprep.RANDAUG_TO_JITTER[int(o)] for o in ops_l[enhance]]
            factors[enhance, 0] = args_l[enhance, 0]
            hip.image_color_jitter(u8, chain, factors)
    return u8


def rand_augment(u8, ops, args, fill):
    """RandAugment IN PLACE on u8 = uint8 [B, S, S, 3]; returns u8.  ops int [B, L] and args fp64 [B, L, 6]: the L layers of image i in the
    order they are applied (imageprep.RANDAUG_OPS / randaug_table; augment.RandAugment.params draws them), fill: the three bytes Affine
    gives the pixels it does not cover.  Every op is the Pillow call timm's auto_augment.py makes (ImageOps, ImageEnhance,
    Image.transform(AFFINE, BICUBIC) with Image.rotate's matrix), byte for byte: on a CUDA device op_image_randaug_layer and, for Color /
    Contrast / Brightness, op_image_color_jitter, layer by layer (S a multiple of 16 in [16, 1024]); on the CPU Pillow itself."""
    from . import imageprep
    _u8_images(u8, "rand_augment")
    tab_ops, tab_args, fill = imageprep.check_randaug((ops, args, fill), u8.shape[0])
    if u8.is_cuda:
        return _rand_augment_device(u8, tab_ops, tab_args, fill)

    def each(i, im):
        if not tab_ops[i].any():
            return None
        for op, arg in zip(tab_ops[i], tab_args[i]):
            im = _pil_randaug(im, op, arg, fill)
        return im
    return _pil_each(u8, each)


def erase_images(x, boxes, noise):
    """RandomErasing's store IN PLACE on x [B, 3, H, W]; returns x.  boxes int [B, 4] = (top, left, h, w) per image, h = 0 for an image
    that is not erased; noise: ONE fp32 tensor on x's device holding the 3 h w values of every erased image back to back, in the order of
    the batch.  x[i, :, top:top+h, left:left+w] = noise_i.view(3, h, w).to(x.dtype) (timm/data/random_erasing.py), bit for bit: on a CUDA
    device op_image_erase in one launch (square bf16 / fp32 batches; anything else is a ValueError), on the CPU the torch statement.
    ValueError: a box outside the image, a noise buffer of the wrong size."""
    import numpy as np
    if not torch.is_tensor(x) or x.dim() != 4 or x.shape[1] != 3:
        raise ValueError("erase_images: x must be [B, 3, H, W]")
    B, _, H, W = x.shape
    boxes = np.asarray(boxes.cpu() if torch.is_tensor(boxes) else boxes, dtype=np.int64).reshape(-1, 4)
    if boxes.shape[0] != B:
        raise ValueError("erase_images: need one (top, left, h, w) per image, got %d for %d images" % (boxes.shape[0], B))
    offs, total = np.zeros(B, dtype=np.int64), 0
    for i, (top, left, h, w) in enumerate(boxes.tolist()):
        offs[i] = total
        if h == 0:
            continue
        if h < 0 or w < 1 or top < 0 or left < 0 or top + h > H or left + w > W:
            raise ValueError("erase_images: box %d (top %d, left %d, h %d, w %d) is empty or outside the %d x %d image" % (i, top, left, h, w, H, W))
        total += 3 * h * w
    have = 0 if noise is None else noise.numel()
    if have != total or (total and (noise.dtype != torch.float32 or noise.device != x.device)):
        raise ValueError("erase_images: noise must be fp32 on x's device with %d values (3 h w per erased image), got %d" % (total, have))
    if x.is_cuda:
        if H != W or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_contiguous():
            raise ValueError("erase_images: a device batch must be square, contiguous and fp32 or bf16, got %s %s" % (x.dtype, tuple(x.shape)))
        return hip.image_erase(x, boxes, noise.contiguous().view(-1) if total else None, offs)
    flat = noise.reshape(-1) if total else None
    for i, (top, left, h, w) in enumerate(boxes.tolist()):
        if h > 0:
            x[i, :, top:top + h, left:left + w] = flat[offs[i]:offs[i] + 3 * h * w].view(3, h, w).to(x.dtype)
    return x


# --------------------------------------------------------------------------------------------------------------
# Mixup / CutMix: timm's Mixup as data/vision_data/image_classify_dataset.py:46-51, 117-130 uses it (augment.Mixup draws the tables)
# --------------------------------------------------------------------------------------------------------------
def _mix_images_torch(x, kind, lam, oml, box, out_dtype):
    """The reference's statement per sample, in fp32 on x's device: x.mul(lam).add(x.flip(0).mul(1 - lam)) where kind is 1, the partner's
    pixels inside the box where it is 2, x elsewhere; then ONE cast to out_dtype."""
    B, _, H, W = x.shape
    xf = x.float()
    part = xf.flip(0)
    v = lambda t: t.to(xf.device).view(B, 1, 1, 1)
    mixed = xf.mul(v(lam)).add(part.mul(v(oml)))
    ys = torch.arange(H, device=xf.device).view(1, 1, H, 1)
    xs = torch.arange(W, device=xf.device).view(1, 1, 1, W)
    b = box.to(xf.device).view(B, 4, 1, 1, 1)
    inside = (ys >= b[:, 0]) & (ys < b[:, 1]) & (xs >= b[:, 2]) & (xs < b[:, 3])
    k = v(kind)
    return torch.where(k == 1, mixed, torch.where((k == 2) & inside, part, xf)).to(out_dtype)


def mix_images(x, params, out_dtype=None, inplace=False):
    """Mixup / CutMix of an image batch x [B, C, H, W] with the per-sample tables params = (kind int32 [B], lam fp32 [B],
    one_minus_lam fp32 [B], box int32 [B, 4] as yl, yh, xl, xh) of augment.Mixup.params: sample i is mixed with sample B - 1 - i of
    the ORIGINAL batch -- kind 0 copy, 1 x[i] * lam + x[j] * one_minus_lam (two rounded fp32 products, one rounded sum: torch's
    x.mul_(lam).add_(x.flip(0).mul_(1 - lam)) bit for bit), 2 the partner's pixels inside the box.  CUDA fp32 / bf16 batches run
    op_mix_images (one read and one write of the batch, in place without a clone); anything else, and shapes the kernel does not
    support (W or C H W not a multiple of 8), the torch statement (the reference's own path).  bf16 inputs are widened, mixed in
    fp32 and rounded ONCE (torch's bf16 arithmetic would round three times).  out_dtype: float32 / bfloat16 (default: x's);
    inplace=True (out_dtype = x's dtype) writes into x and returns it."""
    if x.dim() != 4:
        raise ValueError("mix_images: x must be [B, C, H, W], got %s" % (tuple(x.shape),))
    out_dtype = x.dtype if out_dtype is None else out_dtype
    if inplace and out_dtype != x.dtype:
        raise ValueError("mix_images: in place needs out_dtype = x's dtype, got %s for %s" % (out_dtype, x.dtype))
    B = x.shape[0]
    as_t = lambda t, dt: (t if torch.is_tensor(t) else torch.as_tensor(t)).to(dt).reshape(-1)
    kind, lam, oml, box = params
    kind, lam, oml, box = as_t(kind, torch.int32), as_t(lam, torch.float32), as_t(oml, torch.float32), as_t(box, torch.int32)
    if not (kind.numel() == lam.numel() == oml.numel() == B and box.numel() == 4 * B):
        raise ValueError("mix_images: tables must have B = %d rows (box [B, 4])" % B)
    dts = (torch.float32, torch.bfloat16)
    if x.is_cuda and x.dtype in dts and out_dtype in dts and B > 0:
        xc = x if x.is_contiguous() else x.contiguous()
        out = xc if (inplace and xc is x) else torch.empty(xc.shape, dtype=out_dtype, device=x.device)
        got = hip.mix_images(xc, hip.mix_tables((kind, lam, oml, box.view(B, 4)), B, x.device), out)
        if got is not None:
            return x.copy_(got) if (inplace and got is not x) else got
    res = _mix_images_torch(x, kind, lam, oml, box.view(B, 4), out_dtype)
    return x.copy_(res) if inplace else res


def mix_targets(target, num_classes, lam=1.0, smoothing=0.0):
    """fp32 [B, num_classes]: timm's mixup_target in torch ops on the labels' device -- off = smoothing / C, on = 1 - smoothing + off,
    y1 = full(off).scatter_(1, t, on), y2 the same of t.flip(0), y1 * lam + y2 * (1 - lam).  lam: a Python float (batch mode) or one
    value per sample ([B] tensor / array, elem and pair modes).  The soft targets ops.classify_loss consumes (ROW_LOSS_SOFT)."""
    off = smoothing / num_classes
    on = 1.0 - smoothing + off
    t = target.long().view(-1, 1)

    def one_hot(idx):
        return torch.full((idx.shape[0], num_classes), off, dtype=torch.float32, device=idx.device).scatter_(1, idx, on)

    if not isinstance(lam, (int, float)):
        lam = (lam if torch.is_tensor(lam) else torch.as_tensor(lam)).to(device=t.device, dtype=torch.float32).view(-1, 1)
    return one_hot(t) * lam + one_hot(t.flip(0)) * (1.0 - lam)


# --------------------------------------------------------------------------------------------------------------
# audio pre-processing: base_dataset.py:84-102 / hub_interface.py:170-193 (layer norm, crop, tile, pad) on decoded clips
# --------------------------------------------------------------------------------------------------------------
def _audio_item(item, sample_rate, resample):
    """(as_clip array, rate) of one input of preprocess_audio / resample_audio: a WAV path (the file's rate), a (clip, rate) pair, or a
    clip taken to be at `sample_rate`.  Without `resample` another rate is audioprep.check_rate's ValueError."""
    import os

    import numpy as np

    from . import audioprep
    rate = sample_rate
    if isinstance(item, tuple) and len(item) == 2 and (torch.is_tensor(item[0]) or isinstance(item[0], (np.ndarray, list, str, bytes, os.PathLike))):
        item, rate = item
        audioprep._check_rates(rate, sample_rate)
    if isinstance(item, (str, bytes, os.PathLike)):
        item, rate = audioprep.read_wav(item)
    if not resample:
        audioprep.check_rate(rate, sample_rate)
    return audioprep.as_clip(item), int(rate)


def resample_audio(clips, rates, sample_rate=16000, device="cpu"):
    """(wavs fp32 [B, Tmax] on `device`, lengths int64 [B] on the host): each clip (int16 PCM [n] / [n, 2] or float [n] / [n, C]) brought
    from its rate to `sample_rate` and to mono, zero-padded to the longest.  The filter is audioprep.resample_filter's Kaiser-windowed
    sinc, y[n] = L sum_j x[j] h[n M - j L] with zeros outside the clip, ceil(n L / M) samples: scipy.signal.resample_poly(x, L, M,
    window=h), NOT librosa's soxr -- results differ from the reference's by the difference between the two low-pass filters.  On a
    CUDA device this is op_audio_resample (hip.audio_resample: one H2D copy of samples, descriptors and fp32 taps; each value within
    (T + 3) 2^-24 L sum_j |x[j] h[n M - j L]| of the exact one); on the CPU it is audioprep.resample, accumulated in fp64 and rounded
    once.  A clip already at `sample_rate` is not filtered: its mono fp32 samples pass through."""
    import numpy as np

    from . import audioprep
    if len(rates) != len(clips):
        raise ValueError("resample_audio: %d clips and %d rates" % (len(clips), len(rates)))
    arrs = [audioprep.as_clip(c) for c in clips]
    for r in rates:
        audioprep._check_rates(r, sample_rate)
    dev = torch.device(device)
    same = [int(r) == int(sample_rate) for r in rates]
    if dev.type == "cuda":
        packed = audioprep.pack_resample(arrs, rates, sample_rate)
        lengths = packed.lengths
        wavs = hip.audio_resample(packed, dev)
        for i, a in enumerate(arrs):
            if same[i]:
                wavs[i, : lengths[i]] = torch.from_numpy(audioprep.mono64(a).astype(np.float32)).to(dev)
        wavs = wavs[:, : max(lengths, default=0)]
    else:
        feats = [audioprep.mono64(a).astype(np.float32) if same[i] else audioprep.resample(a, int(rates[i]), int(sample_rate))
                 for i, a in enumerate(arrs)]
        lengths = [w.shape[0] for w in feats]
        wavs = torch.zeros(len(feats), max(lengths, default=0))
        for i, w in enumerate(feats):
            wavs[i, : lengths[i]] = torch.from_numpy(w)
        wavs = wavs.to(dev)
    return wavs, torch.tensor(lengths, dtype=torch.int64)


def preprocess_audio(clips, sample_rate=16000, max_seconds=15, min_seconds=1, dtype=torch.float32, device="cpu", resample=False):
    """(wavs [B, T] in `dtype` on `device`, lengths int64 [B] on the host) from audio clips: WAV paths, int16 PCM [n] / [n, 2] or float
    [n] / [n, C] arrays or tensors at `sample_rate`, or (clip, rate) pairs, mixed freely.  Per clip: mean over the channels,
    F.layer_norm over the whole clip, crop to sample_rate * max_seconds samples, a clip shorter than sample_rate * min_seconds repeated
    up to that length; then right-padding with zeros to the longest clip T (`lengths` are the samples before the padding).  On a CUDA
    device this is op_audio_normalize_pad (hip.audio_normalize_pad: one H2D copy of the staged samples, statistics in integers / fp64,
    each value within 2^-24 (4 |y| + 2 |mean| rstd) of the fp64 result); on the CPU it is audioprep.postprocess, the reference's own
    torch arithmetic.  resample=False: a file or pair at another rate is a ValueError.  resample=True: such a clip is first resampled
    as by resample_audio (this project's Kaiser-windowed sinc, not the reference's soxr), and the layer norm runs over the whole
    resampled clip before the crop; on a device that is op_audio_resample, then op_audio_normalize_pad reading the resampled clips
    from the device buffer, with no host round trip.  Clips at `sample_rate` are computed exactly as with resample=False."""
    from . import audioprep
    items = [_audio_item(c, sample_rate, resample) for c in clips]
    arrs, rates = [a for a, _ in items], [r for _, r in items]
    max_len, min_len = int(sample_rate * max_seconds), int(sample_rate * min_seconds)
    dev = torch.device(device)
    other = any(r != int(sample_rate) for r in rates)
    if dev.type == "cuda":
        kdt = dtype if dtype in (torch.bfloat16, torch.float32) else torch.float32
        if other:
            packed = audioprep.pack_resample(arrs, rates, sample_rate, norm=(max_len, min_len))
            wavs = hip.audio_normalize_pad_device(hip.audio_resample(packed, dev), packed, kdt)
            return wavs.to(dtype), torch.tensor(packed.out_lengths, dtype=torch.int64)
        packed = audioprep.pack_clips(arrs, max_len, min_len)
        return hip.audio_normalize_pad(packed, kdt, dev).to(dtype), torch.tensor(packed.lengths, dtype=torch.int64)
    if other:
        arrs = [a if r == int(sample_rate) else audioprep.resample(a, r, int(sample_rate)) for a, r in items]
    feats = [audioprep.postprocess(a, sample_rate, max_seconds, min_seconds) for a in arrs]
    wavs = torch.zeros(len(feats), max([w.numel() for w in feats], default=0))
    for i, w in enumerate(feats):
        wavs[i, : w.numel()] = w
    return wavs.to(device=dev, dtype=dtype), torch.tensor([w.numel() for w in feats], dtype=torch.int64)


# --------------------------------------------------------------------------------------------------------------
# LayerNorm (+ optional fused GELU)
# --------------------------------------------------------------------------------------------------------------
class LayerNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b, eps, gelu):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        need = any(ctx.needs_input_grad[:3])
        y, mean, rstd = hip.layernorm_fwd(x2, w, b, eps, gelu=gelu, want_stats=need)
        if need:
            ctx.save_for_backward(x2, w, b, mean, rstd)
            ctx.gelu = gelu
        return y.view(shape)

    @staticmethod
    def backward(ctx, dy):
        x2, w, b, mean, rstd = ctx.saved_tensors
        dy2 = dy.reshape(x2.shape)
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        dx, dw, db = hip.layernorm_bwd(dy2, x2, w, b, mean, rstd, gelu=ctx.gelu,
                                       need_wgrad=w is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2]))
        return dx.view(dy.shape), dw, db, None, None


def layer_norm(x, w, b, eps=1e-5, gelu=False):
    return LayerNormFn.apply(x, w, b, eps, gelu)


# --------------------------------------------------------------------------------------------------------------
# Linear  y = x W^T + b
# --------------------------------------------------------------------------------------------------------------
class LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1])
        if not x2.is_contiguous():
            x2 = x2.contiguous()
        y = gemm_any(x2, w, b)
        ctx.save_for_backward(x2, w)
        ctx.has_bias = b is not None
        return y.view(*shape[:-1], w.shape[0])

    @staticmethod
    def backward(ctx, dy):
        x2, w = ctx.saved_tensors
        dy2 = dy.reshape(-1, w.shape[0])
        if not dy2.is_contiguous():
            dy2 = dy2.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = gemm_any(dy2, _transposed(w)).view(*dy.shape[:-1], w.shape[1])
        if ctx.needs_input_grad[1]:
            if dy2.shape[1] % 8 == 0 and x2.shape[1] % 8 == 0:
                dw = wgrad(dy2, x2)
            else:
                dw = gemm_any(_t_pad(dy2), _t_pad(x2))
        if ctx.has_bias and ctx.needs_input_grad[2]:
            dy8 = dy2 if dy2.shape[1] % 8 == 0 else torch.nn.functional.pad(dy2, (0, 8 - dy2.shape[1] % 8))
            db = hip.colsum(dy8.contiguous())[: w.shape[0]]
        return dx, dw, db


def linear(x, w, b=None):
    return LinearFn.apply(x, w, b)


# --------------------------------------------------------------------------------------------------------------
# relative-position bias image  [heads][S][Spad]  (and its transpose for the dK/dV kernel)
# --------------------------------------------------------------------------------------------------------------
class RelPosBias:
    """Per-forward handle: bf16 images of table[bucket] plus the fp32 accumulator the attention backward adds into."""

    def __init__(self, table, bucket_i32, S, ids=None):
        """ids: optional int32 [B, K] position ids (masked pretraining: a different kept-token subset per sample) -- the images
        are then per sample, [B, heads, K, Kpad], built straight from the table (no dense [B, heads, S, S] tensor, no gathers),
        and S is K."""
        self.ids = ids
        self.S, self.Spad = S, hip.attn_spad(S)
        self.num_rel, self.heads = table.shape
        self.bucket = bucket_i32
        self.table = table
        self.acc = None
        self._imageT = None
        self._frag = None
        self.image = _RelPosImageFn.apply(table, self)

    @property
    def frag(self):
        """Fragment-major copy of the image for the resident forward kernel (built on first use, shared by all layers)."""
        if self._frag is None:
            self._frag = hip.attn_bias_pack(self.image.detach(), self.S)
        return self._frag

    @property
    def imageT(self):
        """out[h][key][query]: what the dK/dV kernel reads (built on first use in a backward pass)."""
        if self._imageT is None:
            if self.ids is not None:
                self._imageT = hip.relpos_bias_build_ids(self.table.detach(), self.bucket, self.ids, self.Spad, transposed=True)
            else:
                self._imageT = hip.relpos_bias_build(self.table.detach(), self.bucket, self.S, self.Spad, transposed=True)
        return self._imageT

    def grad_accumulator(self, B):
        """fp32 [slabs, heads, S, Spad]: the attention backward of every layer that uses this table adds its dS sums here
        (per-sample images: one slab per sample)."""
        if self.acc is None:
            self.acc = hip.attn_dbias_buffer(B, self.S, self.heads, self.Spad, self.image.device, per_sample=self.ids is not None)
        elif self.ids is None:  # layers that skip their dropped samples call with different batch sizes: slab counts differ
            need = hip.lib().op_attn_bwd_dbias_slabs(B, self.S, self.heads, hip.TUNE.attn_bwd())
            if need > self.acc.shape[0]:
                grown = torch.zeros(need, *self.acc.shape[1:], dtype=self.acc.dtype, device=self.acc.device)
                grown[:self.acc.shape[0]] = self.acc
                self.acc = grown
        return self.acc


class DenseBias:
    """Handle for a PER-SAMPLE additive bias [B, heads, S, S] (what the adapters' gather of a different token subset per
    sample produces in masked pretraining, adapter/image.py:229-246 / common.take_bias): same interface as RelPosBias, but
    the images are [B, heads, S, Spad], and the attention backward returns one gradient slab per sample, which flows back
    into the dense tensor (and through autograd's gather into the table)."""

    def __init__(self, dense):
        B, self.heads, self.S, _ = dense.shape
        self.B, self.Spad = B, hip.attn_spad(self.S)
        self.acc = None
        self._imageT = None
        self._frag = None
        self.image = _DenseBiasFn.apply(dense, self)

    @property
    def frag(self):
        if self._frag is None:
            self._frag = hip.attn_bias_pack(self.image.detach(), self.S)
        return self._frag

    @property
    def imageT(self):
        if self._imageT is None:
            img = self.image.detach()
            t = torch.zeros_like(img)
            t[..., : self.S] = img[..., : self.S].transpose(2, 3)
            self._imageT = t
        return self._imageT

    def grad_accumulator(self, B):
        if self.acc is None:
            self.acc = hip.attn_dbias_buffer(B, self.S, self.heads, self.Spad, self.image.device, per_sample=True)
        return self.acc


class _DenseBiasFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dense, handle):
        ctx.handle_ref = weakref.ref(handle)
        ctx.S = dense.shape[-1]
        B, heads, S, _ = dense.shape
        img = torch.zeros(B, heads, S, hip.attn_spad(S), dtype=dense.dtype, device=dense.device)
        img[..., :S] = dense
        return img

    @staticmethod
    def backward(ctx, _unused):
        h = ctx.handle_ref()
        if h is None or h.acc is None:
            return torch.zeros(_unused.shape[:-1] + (ctx.S,), dtype=_unused.dtype, device=_unused.device), None
        g = h.acc[..., : ctx.S].to(_unused.dtype)
        h.acc = None
        return g, None


class _RelPosImageFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, table, handle):
        ctx.handle_ref = weakref.ref(handle)  # the layers' ctx keep the handle alive until their backward ran
        ctx.shape = tuple(table.shape)
        if handle.ids is not None:
            return hip.relpos_bias_build_ids(table, handle.bucket, handle.ids, handle.Spad)
        return hip.relpos_bias_build(table, handle.bucket, handle.S, handle.Spad)

    @staticmethod
    def backward(ctx, _unused):
        # The attention backward kernels add dS straight into handle.acc (fp32); the tensor gradient that autograd
        # routes here is a placeholder that only orders this node after every consuming layer.
        h = ctx.handle_ref()
        if h is None or h.acc is None:
            return torch.zeros(ctx.shape, dtype=torch.bfloat16, device=_unused.device), None
        if h.ids is not None:
            dtable = hip.relpos_bias_bwd_ids(h.acc, h.bucket, h.ids, h.num_rel)
        else:
            dtable = hip.relpos_bias_bwd(h.acc.sum(0), h.bucket, h.num_rel, h.S, h.Spad)
        h.acc = None
        return dtable.to(torch.bfloat16), None


# --------------------------------------------------------------------------------------------------------------
# the fused encoder layer
# --------------------------------------------------------------------------------------------------------------
_DIRECT_WEIGHTS = ("wq", "wk", "wv", "wo", "w0", "w1", "w2")
ATTN_PARAMS = ("ln1_w", "ln1_b", "wq", "bq", "wk", "wv", "bv", "aln_w", "aln_b", "wo", "bo", "g1")
FFN_PARAMS = ("ln2_w", "ln2_b", "w0", "w1", "fln_w", "fln_b", "w2", "b2", "g2")
LAYER_PARAMS = ATTN_PARAMS + FFN_PARAMS


class StreamSeg:
    """One stream's rows inside a packed [sum B*S, H] activation matrix: B samples of S tokens starting at row `row0`, with their
    own relative-position bias handle (RelPosBias-like or None) and key-padding bytes.  A single-stream layer is one segment;
    a lock-step pass over several modalities (transformer_encoder.forward_multi) has one per modality.  pad: rows behind the B*S
    token rows that still belong to the segment (zero rows of a packed kept-sample matrix, hip.KeptRows): LayerNorms and GEMMs run
    over them, the attention core does not."""
    __slots__ = ("name", "B", "S", "row0", "bias", "key_pad", "pad")

    def __init__(self, name, B, S, row0, bias=None, key_pad=None, pad=0):
        self.name, self.B, self.S, self.row0, self.bias, self.key_pad, self.pad = name, B, S, row0, bias, key_pad, pad

    @property
    def tokens(self):
        return self.B * self.S

    @property
    def rows(self):
        return self.B * self.S + self.pad

    @property
    def end(self):
        return self.row0 + self.B * self.S + self.pad

    def frag(self, limit):
        return self.bias.frag if self.bias is not None and self.S <= limit else None


def _attn_forward(x2, P, segs, heads, scale, rowscale, rps, keep, want_y=True, xmap=None, out=None, listed=False):
    """x_mid = x + rowscale * g1 * out_proj(subLN(attention(LN1(x))))  on the packed rows x2 [N, H]: LayerNorm, the fused q|k|v
    projection, the sub-LayerNorm and the output projection run over ALL rows in one launch each, the attention core per
    segment.  rowscale: fp32 drop-path multipliers indexed by row // rps (None = 1).  want_y: also write the branch output y1
    (only the gradient of gamma_1 needs it).  xmap (hip.KeptRows.rowmap) + out: x2 is the FULL matrix, the branch runs on its rows
    xmap[r] and writes x_mid for them into `out` (a full matrix; the other rows are the caller's).  listed (the caller's flags: no
    `kept`, gamma_1's gradient does not need y1): the two GEMMs may run over ONE window list of all rows (SKIP_ZERO_FWD)."""
    H = x2.shape[1]
    xln1, mean1, rstd1 = hip.layernorm_fwd(x2, P["ln1_w"], P["ln1_b"], want_stats=keep, x_rows=xmap)
    Nr = xln1.shape[0]
    full = _qkv_rows_that_fill_whole_rounds(Nr, 3 * H) if QKV_ROUND_SPLIT and H % 128 == 0 else Nr
    win, mrs, qkv, x_mid = None, 1, None, None
    if (listed and rowscale is not None and xmap is None and out is None and not (keep and want_y) and H % 256 == 0 and Nr % rps == 0
            and sum(sg.rows for sg in segs) == Nr and all(sg.S % rps == 0 and sg.row0 % rps == 0 for sg in segs)):
        wsegs = [(rowscale[sg.row0 // rps:], sg.row0, sg.S, sg.B, sg.S // rps) for sg in segs]
        dense = [(m, 3 * H, H, hip.EPI_BIAS, True) for m in ((full, Nr - full) if full < Nr else (Nr,))] + [(Nr, H, H, hip.EPI_RESID, True)]
        if _fwd_windows_apply(wsegs, 1, 2, dense, x2.device, flags=not any(sg.pad for sg in segs)):
            qkv = torch.empty(Nr, 3 * H, dtype=x2.dtype, device=x2.device)
            x_mid = torch.empty_like(x2)
            win = hip.live_mwindows_fwd(wsegs, [[(i, 0, 0) for i in range(len(segs))]], [qkv, x_mid], [None, x2])[0]
            mrs = max([sg.S for sg in segs if hip.mwindow_rule(sg.S)[1]] or [1])
    if win is not None and hip.gemm_nt_windows_fwd([xln1], [[P["wq"], P["wk"], P["wv"]]], [[P["bq"], None, P["bv"]]], [qkv], win, H,
                                                   max_row_stride=mrs):
        pass  # (one listed launch over all rows instead of the whole-rounds + tail pair)
    elif H % 128 == 0:
        if full < Nr:  # (689.8 / 689.7 -> 687.3 / 687.0 ms on the headline step, same box: profiles/r5_experiments.md section 12)
            qkv = torch.empty(Nr, 3 * H, dtype=x2.dtype, device=x2.device)
            for lo, hi in ((0, full), (full, Nr)):
                hip.gemm_nt(xln1[lo:hi], [P["wq"], P["wk"], P["wv"]], [P["bq"], None, P["bv"]], n_seg=H, N=3 * H, out=qkv[lo:hi])
        else:
            qkv = hip.gemm_nt(xln1, [P["wq"], P["wk"], P["wv"]], [P["bq"], None, P["bv"]], n_seg=H, N=3 * H)
    else:
        qkv = torch.empty(xln1.shape[0], 3 * H, dtype=x2.dtype, device=x2.device)
        for i, (w, b) in enumerate(((P["wq"], P["bq"]), (P["wk"], None), (P["wv"], P["bv"]))):
            hip.gemm_nt(xln1, [w], [b] if b is not None else None, out=qkv[:, i * H:(i + 1) * H], ldc=3 * H)
    attn = torch.empty_like(xln1)
    lses = []
    for sg in segs:
        r = slice(sg.row0, sg.end)
        _, lse = hip.attn_fwd(qkv[r, :H], qkv[r, H:2 * H], qkv[r, 2 * H:], 3 * H, sg.B, sg.S, heads, scale,
                              sg.bias.image.detach() if sg.bias is not None else None, sg.key_pad, hip.attn_spad(sg.S), out=attn[r],
                              want_lse=keep, bias_frag=sg.frag(hip.ATTN_RESIDENT_MAX_S))
        lses.append(lse)
        if sg.pad:  # rows of no sample: the out-proj weight gradient multiplies them with exact zeros, so they must be finite
            attn[sg.end - sg.pad:sg.end].zero_()
    if P["aln_w"] is not None:
        aln, mean_a, rstd_a = hip.layernorm_fwd(attn, P["aln_w"], P["aln_b"], want_stats=keep)
    else:
        aln, mean_a, rstd_a = attn, None, None
    y1 = torch.empty_like(xln1) if keep and want_y else None
    if win is None or not hip.gemm_nt_windows_fwd([aln], [[P["wo"]]], [[P["bo"]]], [x_mid], win, H, epilogue=hip.EPI_RESID, resids=[x2],
                                                  gammas=[P["g1"]], rowscales=[rowscale], rows_per_sample=[rps], max_row_stride=mrs):
        x_mid = hip.gemm_nt(aln, [P["wo"]], [P["bo"]], epilogue=hip.EPI_RESID, resid=x2, gamma=P["g1"], rowscale=rowscale,
                            rows_per_sample=rps, h0=y1, out=out, resid_rows=xmap)
    if not keep:
        return x_mid, None
    acts = dict(xln1=xln1, mean1=mean1, rstd1=rstd1, qkv=qkv, attn=attn, aln=aln, mean_a=mean_a, rstd_a=rstd_a, y1=y1)
    for i, lse in enumerate(lses):
        acts["lse%d" % i] = lse
    return x_mid, acts


QKV_ROUND_SPLIT = os.environ.get("ONEPEACE_QKV_ROUND_SPLIT", "1") != "0"
# (round 6, ABI 9) a branch that runs on the samples stochastic depth keeps (hip.KeptRows) reads and writes the FULL activation /
# gradient matrix through the row table (KeptRows.rowmap: LayerNorm forward / backward, op_resid_bwd, the residual epilogue of the
# branch's last GEMM) instead of through packed copies -- no op_rows_gather / op_rows_merge passes (17.4 ms of the 586 ms step with
# skip_dropped_branches, profiles/r6_bench_skip_dropped_last_step.txt), the same bits.  "0": round 4's packed copies (A/B, tests).
SKIP_ROW_TABLES = os.environ.get("ONEPEACE_SKIP_ROW_TABLES", "1") != "0"


def _row_tables(kept):
    return kept is not None and SKIP_ROW_TABLES and not FP8_FFN


def _qkv_rows_that_fill_whole_rounds(rows, n_out, cus=256, max_tail=512):
    """Largest multiple of 256 rows whose 256 x 256 tiles are a whole number of rounds of `cus` workgroups, when that leaves at most
    `max_tail` rows for a second, small launch and saves a round (73 088 rows x 4608 columns: 5 148 tiles = 20.1 rounds -- 28 tiles
    cost a 21st round; 284 row tiles = 5 112 tiles = 20 rounds + a 384-row launch); else `rows`."""
    tn, tm = (n_out + 255) // 256, (rows + 255) // 256
    rounds = -(-tm * tn // cus)
    tm_main = (rounds - 1) * cus // tn
    full = tm_main * 256
    return full if 0 < rows - full <= max_tail and tm_main > 0 else rows


GEGLU_SPLIT = os.environ.get("ONEPEACE_GEGLU_SPLIT", "1") != "0"
SEPARATE_DELTA = os.environ.get("ONEPEACE_SEPARATE_DELTA", "0") == "1"  # A/B switch: op_attn_bwd_delta pass instead of the fused one


def _geglu_split(Fd, fln_w):
    """Training forward of the GeGLU: plain two-segment GEMM writing h0 | h1 + op_ln_geglu_fwd instead of the EPI_GEGLU epilogue
    (which keeps the erf on the GEMM's critical path: one wave per SIMD cannot hide ~16 VALU per output element) followed by a
    LayerNorm pass over g.  Needs the inner sub-LayerNorm (scale_fc) and whole 256-column tiles per weight segment."""
    return GEGLU_SPLIT and fln_w is not None and Fd % 256 == 0


def _register_direct(ctx, names, params, needs):
    """Weights whose gradient GEMM accumulates straight into the flat gradient buffer (distributed.FlatParameters).
    Keeps (name, Parameter object) pairs: saved_tensors hands back fresh tensor objects without .grad / attributes."""
    ctx.direct = tuple((n, q) for n, q, ng in zip(names, params, needs) if ng and q is not None and _direct_grad(q))
    for _, q in ctx.direct:
        q._op_pending = getattr(q, "_op_pending", 0) + 1


def _targets(direct, *names):
    """(grad views, accumulate) for a kernel that produces the gradients of `names` together: in-place accumulation
    only when every one of them lives in the flat gradient buffer."""
    if all(n in direct for n in names):
        return [direct[n].grad for n in names], True
    return [None] * len(names), False


def _finish(direct, G, names, values, accumulated):
    for n, v in zip(names, values):
        if accumulated:
            _direct_grad_done(direct[n])
        else:
            G[n] = v


def _return_grads(names, params, G, direct):
    """Gradients handed back to autograd: None for absent parameters and for the ones accumulated in place -- unless a
    producer fell back to a temporary, which is then folded into the flat buffer here."""
    out = []
    for n, q in zip(names, params):
        g = G.get(n) if q is not None else None
        if g is not None and n in direct:
            direct[n].grad.add_(g.view_as(direct[n].grad))
            _direct_grad_done(direct[n])
            g = None
        out.append(g)
    return out


def _resid_backward(dout, y, gamma, ps, S, gname, bname, direct, G, needs, g0=None, rows=None, fold=None, skip_zero_rows=False):
    """Gradient of  resid + ps * gamma * (y)  w.r.t. the branch output and -- where they are wanted -- gamma and the last
    Linear's bias, in one pass.  g0 (fp32 [H]): gamma's gradient is NOT taken here (no y: dgamma_from_wgrad_ok); the kernel fills g0
    with sum_m ps * dout for op_gamma_grad_finish instead and returns ps * dout WITHOUT gamma.
    fold (a dict; one call per segment of rows that share gamma but not the bias): gamma's gradient is left to the caller -- a
    temporary is summed into fold[gname] in fp32, an in-place accumulation is not reported -- who finishes it once, after the last
    segment."""
    names = tuple(n for n, present in ((gname, gamma is not None and g0 is None), (bname, True)) if present and needs.get(n))
    tgt, acc = _targets(direct, *names) if names else ([], False)
    t = dict(zip(names, tgt))
    dgamma = (t[gname] if acc else True) if gname in t else None
    dbias = (t[bname] if acc else True) if bname in t else None
    dy, dg, db = hip.resid_bwd(dout, y if dgamma is not None else None, gamma, ps, S, dgamma=dgamma, dbias=dbias, accumulate=acc, g0=g0,
                               dout_rows=rows, skip_zero_rows=skip_zero_rows)  # (rows: dout is the full matrix, the pass runs on its rows rows[m])
    if fold is not None and gname in t:
        if not acc:
            fold[gname] = fold[gname] + dg.float() if gname in fold else dg.float()
        names = tuple(n for n in names if n != gname)
    _finish(direct, G, names, tuple({gname: dg, bname: db}[n] for n in names), acc)
    return dy


def _adjacent_grads(direct, names):
    """The parameters `names` in the memory order of their flat gradient views when those views tile ONE contiguous range
    (distributed.FlatParameters lays a layer's decayed weights out back to back), else None.  A merged weight-gradient GEMM
    then writes all of them with one launch (and one split-K fold) instead of one launch each."""
    if not all(n in direct for n in names):
        return None
    order = sorted(names, key=lambda n: direct[n].grad.data_ptr())
    for a, b in zip(order, order[1:]):
        ga, gb = direct[a].grad, direct[b].grad
        if not ga.is_contiguous() or ga.data_ptr() + ga.numel() * ga.element_size() != gb.data_ptr() or ga.shape[1:] != gb.shape[1:]:
            return None
    return order


def _span(direct, order):
    """One [sum rows, cols] view over the adjacent gradient views of `order`."""
    g0 = direct[order[0]].grad
    return torch.as_strided(g0, (sum(direct[n].grad.shape[0] for n in order), g0.shape[1]), (g0.shape[1], 1))


def _weight_grad_fn(ctx, G):
    direct = dict(ctx.direct)

    def weight_grad(name, dyv, xv, side=None, after=None, ktiles=None):
        target = direct.get(name)
        if target is not None:
            wgrad_into(dyv, xv, target.grad, (target,), side, after, ktiles)
        else:
            assert side is None and after is None
            G[name] = wgrad(dyv, xv)
    return weight_grad, direct


def _gamma_finish_hook(rowdot, gamma_param, pairs, done):
    """After the grouped launch: dgamma += sum_s rowdot[s] + sum b_i g0_i into gamma's flat gradient view, and gamma's in-place
    contribution is reported (the reducer may all-reduce its bucket)."""
    def run():
        hip.gamma_grad_finish(rowdot, pairs, gamma_param.grad, True)
        if done:
            _direct_grad_done(gamma_param)
    return run


def _save(ctx, keep, acts, *tensors):
    if keep:  # 288 GB of HBM: keep the intermediates instead of recomputing them in backward
        ctx.act_names = [k for k, v in acts.items() if v is not None]
        ctx.save_for_backward(*tensors, *[acts[k] for k in ctx.act_names])
    else:
        ctx.act_names = None
        ctx.save_for_backward(*tensors)


def _restore(ctx, saved_acts, optional):
    A = dict(zip(ctx.act_names, saved_acts))
    for k in optional:
        A.setdefault(k, None)
    return A


class AttnBranchFn(torch.autograd.Function):
    """First half of transformer_layer.py:165-228: x + droppath(gamma_1 * self_attn(LN(x))), forward + backward in HIP, over the
    packed rows of one or more streams.

    x2: [N, H] bf16 contiguous rows (batch-major per segment; a segment may itself be a joint text+image / text+audio
    stream).  segs: [StreamSeg] covering the N rows.  rowscale: fp32 drop-path multipliers (0 or 1/keep) indexed by
    row // rps, or None.  imgs: one bias image per segment (or None) -- only there to put the tables into the autograd graph."""

    @staticmethod
    def forward(ctx, x2, segs, rowscale, rps, heads, save_acts, kept, *rest):
        nseg = len(segs)
        params = rest[nseg:]
        P = dict(zip(ATTN_PARAMS, params))
        need_grad = any(ctx.needs_input_grad) and bool(int(save_acts) & 2)  # bit 1: autograd is recording (_save_flags) -- a
        keep = bool(int(save_acts) & 1) and need_grad                       # no-grad teacher pass registers and keeps nothing
        first_param = 7 + nseg
        needs = dict(zip(ATTN_PARAMS, ctx.needs_input_grad[first_param:]))
        x_full = x2
        mapped = _row_tables(kept)  # the kept samples' rows through the row table (no packed copy of x, no merge pass)
        if kept is not None and not mapped:  # the branch runs on the rows of the samples it keeps (segs / rowscale describe THOSE rows)
            x2 = hip.rows_gather(x_full, kept)
        H = x2.shape[1]
        N = kept.total if mapped else x2.shape[0]
        scale = (H // heads) ** -0.5
        # gamma_1's gradient from the out-proj weight gradient instead of from the branch output (then y1 is never written)
        ctx.dg_fused = need_grad and dgamma_from_wgrad_ok([N], P["g1"], [P["wo"]], [P["bo"]], needs["g1"], [needs["wo"]])
        if mapped:
            x_mid = torch.empty_like(x_full)
            _, acts = _attn_forward(x_full, P, segs, heads, scale, rowscale, rps, keep, want_y=needs["g1"] and not ctx.dg_fused,
                                    xmap=kept.rowmap(), out=x_mid)
            hip.rows_merge(x_full, None, kept, out=x_mid)  # (the dropped samples' rows: copied)
        else:
            x_mid, acts = _attn_forward(x2, P, segs, heads, scale, rowscale, rps, keep, want_y=needs["g1"] and not ctx.dg_fused,
                                        listed=kept is None and ctx.dg_fused)
            if kept is not None:
                x_mid = hip.rows_merge(x_full, x_mid, kept)
        ctx.kept, ctx.mapped = kept, mapped
        ctx.segs, ctx.dims, ctx.n_params, ctx.first_param = segs, (N, H, heads, scale, rps), len(params), first_param
        ctx.direct = ()
        if need_grad:
            _register_direct(ctx, ATTN_PARAMS, params, ctx.needs_input_grad[first_param:])
        if keep:  # activations only a frozen parameter's gradient would read are not kept
            if not needs["wo"]:
                acts["aln"] = None if P["aln_w"] is not None else acts["aln"]
            if not (needs["wq"] or needs["wk"] or needs["wv"]):
                acts["xln1"] = None
        ctx.cheap = keep and bool(int(save_acts) & 4)
        if ctx.cheap:  # (set_recompute_cheap) re-created in backward from x2 / attn, which are kept anyway
            acts["xln1"] = None
            if P["aln_w"] is not None:
                acts["aln"] = None
        _save(ctx, keep, acts, x2, rowscale, *params)
        return x_mid

    @staticmethod
    def backward(ctx, dx_mid):
        x2, rowscale, *rest = ctx.saved_tensors
        params, saved_acts = rest[:ctx.n_params], rest[ctx.n_params:]
        N, H, heads, scale, rps = ctx.dims
        segs = ctx.segs
        nseg = len(segs)
        P = dict(zip(ATTN_PARAMS, params))
        # what autograd actually asks for (frozen parameters -- stage-2 audio-language pretraining freezes the whole attention
        # branch, one_peace_pretrain.py:98-104 -- cost no weight-gradient GEMM, column sum or LayerNorm parameter reduction)
        needs = {n: bool(ng) and q is not None for n, q, ng in zip(ATTN_PARAMS, params, ctx.needs_input_grad[ctx.first_param:])}
        need_x = bool(ctx.needs_input_grad[0])
        want_dbias = [sg.bias is not None and sg.bias.image.requires_grad for sg in segs]
        kept, mapped = ctx.kept, ctx.mapped
        xmap = kept.rowmap() if mapped else None  # (mapped: x2 is the FULL matrix the forward read through the table)
        if ctx.act_names is not None:
            A = _restore(ctx, saved_acts, ("mean_a", "rstd_a", "y1", "xln1", "aln"))
            if ctx.cheap:  # the weight-gradient operands that were not kept: the same kernels on the same rows, bit for bit
                if needs["wq"] or needs["wk"] or needs["wv"]:
                    A["xln1"] = hip.layernorm_fwd(x2, P["ln1_w"], P["ln1_b"], x_rows=xmap)[0]
                if needs["wo"] and P["aln_w"] is not None:
                    A["aln"] = hip.layernorm_fwd(A["attn"], P["aln_w"], P["aln_b"])[0]
        else:  # recompute (the reference's checkpoint_activations behaviour)
            _, A = _attn_forward(x2, P, segs, heads, scale, rowscale, rps, True, want_y=not ctx.dg_fused, xmap=xmap,
                                 out=torch.empty_like(x2) if mapped else None, listed=kept is None and ctx.dg_fused)
        if not dx_mid.is_contiguous():
            dx_mid = dx_mid.contiguous()
        dx_full = dx_mid
        if kept is not None and not mapped:  # rows of dropped samples: the gradient passes through the skip connection untouched
            dx_mid = hip.rows_gather(dx_full, kept)
        G = {}
        weight_grad, direct = _weight_grad_fn(ctx, G)
        # out-proj and q|k|v weight gradients: both run over ALL rows, one list serves both (rows of dropped samples are zero in dy1, and
        # so in everything the branch derives from it)
        kt1 = None
        whole = rowscale is not None and kept is None and N % rps == 0 and not any(sg.pad for sg in segs) and sum(sg.rows for sg in segs) == N
        if whole:
            kt1 = _live_ktiles([(rowscale, 0, rps, N // rps)], [(0, N)], dx_mid.device)[0]
        # the two input gradients over all rows (out-proj, q|k|v) share ONE window list; their outputs exist before it is built,
        # because the launch that builds it also writes the zero rows.  (SKIP_ZERO_ROWS) d subLN(attn) and d LN1(x) are each read by one
        # LayerNorm backward, which takes the multipliers; without the sub-LayerNorm the dense attention backward reads the former
        upstream = ("ln1_w", "ln1_b", "wq", "bq", "wk", "wv", "bv", "aln_w", "aln_b")
        need_up = need_x or any(want_dbias) or any(needs[n] for n in upstream)
        need_dxln1 = need_x or needs["ln1_w"] or needs["ln1_b"]
        win1, daln, dxln1 = None, None, None
        if need_up and whole and all(sg.S % rps == 0 and sg.row0 % rps == 0 for sg in segs):
            daln = torch.empty(N, H, dtype=dx_mid.dtype, device=dx_mid.device)
            dxln1 = torch.empty_like(daln) if need_dxln1 else None
            filled, unread = _bwd_fills([(daln, P["aln_w"] is not None), (dxln1, True)])
            win1 = _dgrad_windows([(rowscale[sg.row0 // rps:], sg.row0, sg.S, sg.B, sg.S // rps) for sg in segs],
                                  [[(i, 0, 0) for i in range(nseg)]], filled,
                                  [(N, H, H)] + ([(N, H, 3 * H)] if need_dxln1 else []), unread=unread)
        zr_b = SKIP_ZERO_ROWS and win1 is not None  # the row kernels of this backward leave out the rows of dropped samples
        if ctx.dg_fused:  # dy1 = rowscale * dx_mid, WITHOUT gamma_1 (weight gradient: rscale; input gradient: scaled weight copy)
            g0 = torch.empty(H, dtype=torch.float32, device=dx_mid.device)
            dy1 = _resid_backward(dx_mid, None, P["g1"], rowscale, rps, "g1", "bo", direct, G, needs, g0=g0, rows=xmap, skip_zero_rows=zr_b)
            rowdot, (rd_wo,) = _rowdot_slots(dx_mid.device, [P["wo"]])
            weight_grad("wo", dy1, A["aln"], side=(P["wo"], rd_wo, P["g1"]),
                        after=_gamma_finish_hook(rowdot, direct["g1"], [(P["bo"], g0)] if P["bo"] is not None else [], True), ktiles=kt1)
            wo_t = _transposed(P["wo"], scale=P["g1"])
        else:
            dy1 = _resid_backward(dx_mid, A["y1"], P["g1"], rowscale, rps, "g1", "bo", direct, G, needs, rows=xmap, skip_zero_rows=zr_b)
            if needs["wo"]:
                weight_grad("wo", dy1, A["aln"], ktiles=kt1)
            wo_t = None
        dx = None
        if need_up:
            wo_in = wo_t if wo_t is not None else _transposed(P["wo"])
            if win1 is None or not _dgrad_listed([dy1], [wo_in], [daln], win1[0], segs):
                daln = hip.gemm_nt(dy1, [wo_in])
            if P["aln_w"] is not None:
                want = needs["aln_w"] or needs["aln_b"]
                (tw, tb), acc = _targets(direct, "aln_w", "aln_b") if want else ((None, None), False)
                dattn, dw_, db_ = hip.layernorm_bwd(daln, A["attn"], P["aln_w"], P["aln_b"], A["mean_a"], A["rstd_a"], dw=tw, db=tb,
                                                    accumulate=acc, need_wgrad=want, ps=rowscale if zr_b else None, rows_per_sample=rps)
                if want:
                    _finish(direct, G, ("aln_w", "aln_b"), (dw_, db_), acc)
            else:
                dattn = daln
            # column order of the packed q|k|v gradient: the memory order of the three weights' flat gradient views when those
            # are adjacent (then ONE weight-gradient launch writes all three), q, k, v otherwise
            qkv_names = ("wq", "wk", "wv")
            order = _adjacent_grads(direct, qkv_names) if all(needs[n] for n in qkv_names) and H % 8 == 0 else None
            cols = tuple(order) if order else qkv_names
            slot = {n: i for i, n in enumerate(cols)}
            qkv = A["qkv"]
            dqkv = torch.empty_like(qkv)
            for i, sg in enumerate(segs):
                r = slice(sg.row0, sg.end)
                if sg.pad:  # rows of no sample: zero gradient (they are operand rows of the q|k|v weight gradient)
                    dqkv[sg.end - sg.pad:sg.end].zero_()
                dparts = {n: dqkv[r, slot[n] * H:(slot[n] + 1) * H] for n in qkv_names}
                _attn_backward(qkv[r], dattn[r], A["attn"][r], A["lse%d" % i], sg.B, sg.S, heads, scale,
                               sg.bias.image.detach() if sg.bias is not None else None, sg.bias.imageT if sg.bias is not None else None,
                               sg.key_pad, sg.bias.grad_accumulator(sg.B) if want_dbias[i] else None, sg.frag(384),
                               dparts["wq"], dparts["wk"], dparts["wv"])
            bias_of = {"wq": "bq", "wv": "bv"}
            bnames = tuple(bias_of[n] for n in cols if n in bias_of and needs[bias_of[n]])
            if bnames:
                tgt, acc = _targets(direct, *bnames)
                if H % 8 == 0:
                    outs = [None, None, None]
                    for n, t_ in zip(bnames, tgt):
                        outs[slot["wq" if n == "bq" else "wv"]] = t_ if acc else torch.empty(H, dtype=dqkv.dtype, device=dqkv.device)
                    hip.colsum_segments(dqkv, H, outs, accumulate=acc)
                    _finish(direct, G, bnames, tuple(outs[slot["wq" if n == "bq" else "wv"]] for n in bnames), acc)
                else:
                    sums = hip.colsum(dqkv)
                    for n in bnames:
                        i = slot["wq" if n == "bq" else "wv"]
                        G[n] = sums[i * H:(i + 1) * H]
            if order:  # one problem: dW[3H, H] straight into the three adjacent flat gradient views
                wgrad_into(dqkv, A["xln1"], _span(direct, order), [direct[n] for n in order], ktiles=kt1)
            elif any(n in direct for n in qkv_names) or not all(needs[n] for n in qkv_names):
                for n in qkv_names:
                    if needs[n]:
                        weight_grad(n, dqkv[:, slot[n] * H:(slot[n] + 1) * H], A["xln1"], ktiles=kt1)
            else:
                dW = wgrad(dqkv, A["xln1"])  # [3H, H]
                G["wq"], G["wk"], G["wv"] = dW[:H], dW[H:2 * H], dW[2 * H:]
            if need_dxln1:
                wqkv_t = _transposed(tuple(P[n] for n in cols))
                if win1 is None or not _dgrad_listed([dqkv], [wqkv_t], [dxln1], win1[0], segs):
                    dxln1 = hip.gemm_nt(dqkv, [wqkv_t])
                want = needs["ln1_w"] or needs["ln1_b"]
                (tw, tb), acc = _targets(direct, "ln1_w", "ln1_b") if want else ((None, None), False)
                # (mapped: the kept samples' rows of a NEW full matrix -- the incoming gradient may be the caller's tensor --, the dropped
                # samples' rows copied below)
                dx, dw_, db_ = hip.layernorm_bwd(dxln1, x2, P["ln1_w"], P["ln1_b"], A["mean1"], A["rstd1"], add=dx_mid, dw=tw, db=tb,
                                                 accumulate=acc, need_wgrad=want, dx=torch.empty_like(dx_full) if mapped else None,
                                                 x_rows=xmap, ps=rowscale if zr_b else None, rows_per_sample=rps)
                if want:
                    _finish(direct, G, ("ln1_w", "ln1_b"), (dw_, db_), acc)
        if dx is None and need_x:  # nothing upstream of the residual wanted a gradient: only the skip connection carries one
            dx = dx_full
        elif dx is not None and mapped:
            hip.rows_merge(dx_full, None, kept, out=dx)
        elif dx is not None and kept is not None:
            dx = hip.rows_merge(dx_full, dx, kept)
        flush_wgrads()  # the layer's weight gradients (this branch's and the FFN branch's, which ran before it) as one launch
        grads = _return_grads(ATTN_PARAMS, params, G, direct)
        dimgs = []
        for sg, w in zip(segs, want_dbias):  # placeholders (see _RelPosImageFn.backward); the real gradients went into bias.acc
            # ONE placeholder per handle and backward pass: the engine counts the image node's dependencies by graph edges (an undefined
            # gradient still decrements them), so the node runs after every consuming layer either way -- forty placeholders made autograd
            # materialise and add forty [heads, S, Spad] zero images per stream and step (3 fills + 3 adds per layer in the step trace)
            if w and not getattr(sg.bias, "_grad_routed", False):
                sg.bias._grad_routed = True
                img = sg.bias.image
                dimgs.append(torch.zeros((), dtype=img.dtype, device=img.device).expand(img.shape))
            else:
                dimgs.append(None)
        return (dx, None, None, None, None, None, None, *dimgs, *grads)


FFN_SHARED = ("ln2_w", "ln2_b", "g2")                       # shared by every modality (final_layer_norm, gamma_2)
FFN_OWN = ("w0", "w1", "fln_w", "fln_b", "w2", "b2")          # one set per modality (text_ffn / image_ffn / audio_ffn)


class FfnBranchMultiFn(torch.autograd.Function):
    """Second half of transformer_layer.py:165-228: x + droppath(gamma_2 * <modality>_ffn(LN(x))) on the packed rows of one or more
    modalities, each segment through its OWN FFN weights (a single stream, ffn_branch, is one segment).  final_layer_norm (forward and
    backward) runs over all rows in one launch; with several segments the two narrow GEMMs of the branch -- down-projection + residual
    (N = H, K = F) and the input gradient of wi_0 | wi_1 (N = H, K = 2F) -- are ONE grouped launch over the modalities
    (op_gemm_nt_grouped: a text pass alone is 192 tiles on 256 CUs, the image pass 3.02 rounds; one segment takes op_gemm_nt, whose
    kernel choice for a lone problem can differ); the wide ones (GeGLU up-projection, its LN(F), the input gradient of the
    down-projection) and the weight gradients stay per modality.

    x2: [N, H]; segs: [StreamSeg] (only row0 / B / S are used); pss: per segment fp32 [B] drop-path multipliers or None;
    params: ln2_w, ln2_b, g2, then (w0, w1, fln_w, fln_b, w2, b2) per segment."""

    @staticmethod
    def _compute(x2, segs, pss, params, keep, want_y, grad=None, xmap=None, listed=False, info=None):
        """grad: the pass belongs to a training step (default: keep).  The GeGLU form is chosen by THAT, not by `keep`: with
        checkpoint_activations the forward (keep = False) and its recomputation in backward (keep = True) must run the same kernels, or
        the LayerNorm(F) statistics the gradients use are not those of the forward output.  No-grad inference keeps the fused
        GeGLU epilogue (one store instead of three; h0 / h1 rounded to bf16 only in the split form: a bf16-level train / eval difference).
        xmap (hip.KeptRows.rowmap, not with the fp8 FFN): x2 is the FULL matrix, the branch runs on its rows xmap[r]; the returned
        `out` is a full matrix in which the rows of the kept samples are written (the others are the caller's).
        listed (the caller's flags: no `kept`, gamma_2's gradient does not need y2): the split form's wi_0 | wi_1 launches become ONE
        grouped launch over a window list, which also serves the grouped down-projection (SKIP_ZERO_FWD).
        info (a dict): info["zero_rows"] tells whether h0 | h1 went without the fill (SKIP_ZERO_ROWS): the rows of dropped samples that
        no window covers hold NOTHING then, and every later reader of h0 | h1 has to leave them out as op_ln_geglu_fwd did here."""
        nseg = len(segs)
        shared = dict(zip(FFN_SHARED, params[:3]))
        own = [dict(zip(FFN_OWN, params[3 + 6 * i:9 + 6 * i])) for i in range(nseg)]
        H = x2.shape[1]
        N = xmap.numel() if xmap is not None else x2.shape[0]
        Fd = own[0]["w0"].shape[0]
        dev, dt = x2.device, x2.dtype
        has_fln = own[0]["fln_w"] is not None
        split = (keep if grad is None else grad) and _geglu_split(Fd, own[0]["fln_w"])
        fp8 = FP8_FFN and H % 128 == 0 and Fd % 128 == 0  # opt-in: e4m3 operands with per-row scales, fp32 accumulation (csrc/fp8.hip)
        gq = None
        if fp8 and split:  # (round 5) all rows of all streams: the fp8 operands come out of the kernels that produce the bf16 rows
            xln2, mean2, rstd2, (xq, xs) = hip.layernorm_fwd(x2, shared["ln2_w"], shared["ln2_b"], want_stats=keep, q8=True)
            gq, gs = torch.empty(N, Fd, dtype=torch.uint8, device=dev), torch.empty(N, dtype=torch.float32, device=dev)
        else:
            xln2, mean2, rstd2 = hip.layernorm_fwd(x2, shared["ln2_w"], shared["ln2_b"], want_stats=keep, x_rows=xmap)
            if fp8:
                xq, xs = hip.quant_fp8_rows(xln2)
        if split:
            hh = torch.empty(N, 2 * Fd, dtype=dt, device=dev)
            g, h0, h1 = None, hh[:, :Fd], hh[:, Fd:]
        else:
            g = torch.empty(N, Fd, dtype=dt, device=dev)
            h0 = torch.empty(N, Fd, dtype=dt, device=dev) if keep else None
            h1 = torch.empty(N, Fd, dtype=dt, device=dev) if keep else None
        gln = torch.empty(N, Fd, dtype=dt, device=dev) if has_fln else g
        mean_f = torch.empty(N, dtype=torch.float32, device=dev) if (keep or split) and has_fln else None
        rstd_f = torch.empty(N, dtype=torch.float32, device=dev) if (keep or split) and has_fln else None
        L = hip.lib()
        rs = [slice(sg.row0, sg.end) for sg in segs]
        win, mrs, out, listed_up, zero_rows = None, 1, None, False, False
        if listed and split and not fp8 and xmap is None and not (keep and want_y) and nseg <= 3 and H % 256 == 0:
            wsegs = [(ps, sg.row0, sg.S, sg.B, 1) for ps, sg in zip(pss, segs)]
            dense = [(sg.rows, 2 * Fd, H, hip.EPI_BIAS, False) for sg in segs] + ([(segs[0].rows, H, Fd, hip.EPI_RESID, True)] if nseg == 1 else [])
            if _fwd_windows_apply(wsegs, 1, 2, dense, dev, flags=not any(sg.pad for sg in segs)):
                out = torch.empty_like(x2)
                zero_rows = SKIP_ZERO_ROWS  # (h0 | h1: only LayerNorm_F(GeGLU) forward / backward read them, and both take ps)
                win = hip.live_mwindows_fwd(wsegs, [[(i, i, sg.row0) for i, sg in enumerate(segs)]], [None if zero_rows else hh, out],
                                            [None, x2])[0]
                mrs = max([sg.S for sg in segs if hip.mwindow_rule(sg.S)[1]] or [1])
                listed_up = hip.gemm_nt_windows_fwd([xln2[r] for r in rs], [[P["w0"], P["w1"]] for P in own], None, [hh[r] for r in rs], win, Fd,
                                                    max_row_stride=mrs)
        if info is not None:
            info["zero_rows"] = zero_rows
        for sg, P, ps in zip(segs, own, pss):
            r = slice(sg.row0, sg.end)
            if split:
                if fp8:
                    w01q, w01s = _fp8_weight_pair(P["w0"], P["w1"])
                    hip.gemm_nt_fp8(xq[r], xs[r], [w01q], [w01s], out=hh[r])
                elif not listed_up:
                    hip.gemm_nt(xln2[r], [P["w0"], P["w1"]], n_seg=Fd, N=2 * Fd, out=hh[r])
                hip.ln_geglu_fwd(h0[r], h1[r], P["fln_w"], P["fln_b"], out=gln[r], mean=mean_f[r], rstd=rstd_f[r],
                                 q8=(gq[r], gs[r]) if fp8 else None, ps=ps if zero_rows else None, rows_per_sample=sg.S)
                continue
            if fp8:
                (w0q, w0s), (w1q, w1s) = _fp8_weight(P["w0"]), _fp8_weight(P["w1"])
                hip.gemm_nt_fp8(xq[r], xs[r], [w0q, w1q], [w0s, w1s], epilogue=hip.EPI_GEGLU, h0=h0[r] if keep else None,
                                h1=h1[r] if keep else None, out=g[r])
            else:
                hip.gemm_nt(xln2[r], [P["w0"], P["w1"]], epilogue=hip.EPI_GEGLU, h0=h0[r] if keep else None, h1=h1[r] if keep else None,
                            out=g[r])
            if has_fln:
                hip._check(L.op_layernorm_fwd(hip.ptr(g[r]), hip.ptr(P["fln_w"]), hip.ptr(P["fln_b"]), hip.ptr(gln[r]),
                                              hip.ptr(mean_f[r]) if keep else None, hip.ptr(rstd_f[r]) if keep else None, sg.rows, Fd, 1e-5, 0,
                                              hip.DT_BF16, None, hip.stream()), "op_layernorm_fwd")
        y2 = torch.empty(N, H, dtype=dt, device=dev) if keep and want_y else None
        if out is None:
            out = torch.empty_like(x2)  # (with xmap: the full matrix)
        if fp8:  # one fp8 launch per modality (the grouped persistent launch is bf16 only)
            if gq is None:
                gq, gs = hip.quant_fp8_rows(gln)
            for sg, P, r, ps in zip(segs, own, rs, pss):
                w2q, w2s = _fp8_weight(P["w2"])
                hip.gemm_nt_fp8(gq[r], gs[r], [w2q], [w2s], bias=P["b2"], epilogue=hip.EPI_RESID, resid=x2[r], gamma=shared["g2"], rowscale=ps,
                                rows_per_sample=sg.S, h0=y2[r] if y2 is not None else None, out=out[r])
            acts = dict(xln2=xln2, mean2=mean2, rstd2=rstd2, h0=h0, h1=h1, gln=gln, mean_f=mean_f, rstd_f=rstd_f, y2=y2) if keep else None
            return out, acts
        tabs = [xmap[r] for r in rs] if xmap is not None else None  # (row tables: every problem writes ITS rows of the shared full matrix)
        if win is not None and hip.gemm_nt_windows_fwd([gln[r] for r in rs], [[P["w2"]] for P in own], [[P["b2"]] for P in own], [out[r] for r in rs],
                                                       win, H, epilogue=hip.EPI_RESID, resids=[x2[r] for r in rs], gammas=[shared["g2"]] * nseg,
                                                       rowscales=list(pss), rows_per_sample=[sg.S for sg in segs], max_row_stride=mrs):
            acts = dict(xln2=xln2, mean2=mean2, rstd2=rstd2, h0=h0, h1=h1, gln=gln, mean_f=mean_f, rstd_f=rstd_f, y2=y2) if keep else None
            return out, acts
        grouped = nseg > 1 and hip.gemm_nt_grouped(
            [gln[r] for r in rs], [P["w2"] for P in own], biases=[P["b2"] for P in own],
            outs=[out[r] for r in rs] if tabs is None else [out] * nseg, epilogue=hip.EPI_RESID,
            h0s=[y2[r] for r in rs] if y2 is not None else None, resids=[x2[r] for r in rs] if tabs is None else [x2] * nseg,
            gammas=[shared["g2"]] * nseg, rowscales=list(pss), rows_per_sample=[sg.S for sg in segs], resid_rows=tabs) is not None
        if not grouped:  # one segment, or a shape outside the persistent kernel: one launch per modality
            for i, (sg, P, r, ps) in enumerate(zip(segs, own, rs, pss)):
                hip.gemm_nt(gln[r], [P["w2"]], [P["b2"]], epilogue=hip.EPI_RESID, resid=x2[r] if tabs is None else x2, gamma=shared["g2"],
                            rowscale=ps, rows_per_sample=sg.S, h0=y2[r] if y2 is not None else None, out=out[r] if tabs is None else out,
                            resid_rows=tabs[i] if tabs is not None else None)
        acts = dict(xln2=xln2, mean2=mean2, rstd2=rstd2, h0=h0, h1=h1, gln=gln, mean_f=mean_f, rstd_f=rstd_f, y2=y2) if keep else None
        return out, acts

    @staticmethod
    def forward(ctx, x2, segs, pss, save_acts, kept, *params):
        nseg = len(segs)
        Fd = params[3].shape[0]
        need_grad = any(ctx.needs_input_grad) and bool(int(save_acts) & 2)
        keep = bool(int(save_acts) & 1) and need_grad
        needs = ctx.needs_input_grad[5:]
        has_fln = params[5] is not None
        x_full = x2
        mapped = _row_tables(kept)  # (see AttnBranchFn.forward)
        if kept is not None and not mapped:  # the branch runs on the rows of the samples it keeps (segs / pss describe THOSE rows)
            x2 = hip.rows_gather(x_full, kept)
        H = x2.shape[1]
        N = kept.total if mapped else x2.shape[0]
        w2s, b2s = [params[3 + 6 * i + 4] for i in range(nseg)], [params[3 + 6 * i + 5] for i in range(nseg)]
        ctx.dg_fused = need_grad and dgamma_from_wgrad_ok([sg.rows for sg in segs], params[2], w2s, b2s, bool(needs[2]),
                                                           [bool(needs[3 + 6 * i + 4]) for i in range(nseg)])
        info = {}
        out, acts = FfnBranchMultiFn._compute(x2, segs, pss, params, keep, bool(needs[2]) and not ctx.dg_fused, grad=bool(int(save_acts) & 2),
                                              xmap=kept.rowmap() if mapped else None, listed=kept is None and ctx.dg_fused, info=info)
        ctx.zero_rows = info["zero_rows"]
        if mapped:
            hip.rows_merge(x_full, None, kept, out=out)  # (the dropped samples' rows: copied)
        elif kept is not None:
            out = hip.rows_merge(x_full, out, kept)
        ctx.kept, ctx.mapped = kept, mapped
        ctx.segs, ctx.n_params, ctx.dims = segs, len(params), (N, H, Fd)
        ctx.direct = ()
        names = list(FFN_SHARED) + ["%s@%d" % (n, i) for i in range(nseg) for n in FFN_OWN]
        ctx.names = names
        if need_grad:
            _register_direct(ctx, names, params, needs)
        if keep:  # activations only a frozen parameter's gradient would read are not kept
            nd = dict(zip(names, needs))
            if not any(nd["w0@%d" % i] or nd["w1@%d" % i] for i in range(nseg)):
                acts["xln2"] = None
            if has_fln and not any(nd["w2@%d" % i] for i in range(nseg)):
                acts["gln"] = None
        ctx.cheap = keep and bool(int(save_acts) & 4)
        if ctx.cheap:  # (set_recompute_cheap; also with the fp8 forward: backward reads the bf16 rows, which the same kernels re-create)
            acts["xln2"] = None
            if _geglu_split(Fd, params[5]):  # LN_F(gelu(h0) * h1) comes back from the kept h0 | h1
                acts["gln"] = None
        _save(ctx, keep, acts or {}, x2, *[ps for ps in pss], *params)
        ctx.n_ps = len(pss)
        return out

    @staticmethod
    def backward(ctx, dout):
        x2, *rest = ctx.saved_tensors
        pss, rest = rest[:ctx.n_ps], rest[ctx.n_ps:]
        params, saved_acts = rest[:ctx.n_params], rest[ctx.n_params:]
        segs, names = ctx.segs, ctx.names
        nseg = len(segs)
        N, H, Fd = ctx.dims
        P = dict(zip(names, params))
        needs = {n: bool(ng) and q is not None for n, q, ng in zip(names, params, ctx.needs_input_grad[5:])}
        need_x = bool(ctx.needs_input_grad[0])
        kept, mapped = ctx.kept, ctx.mapped
        xmap = kept.rowmap() if mapped else None  # (mapped: x2 is the FULL matrix the forward read through the table)
        if ctx.act_names is not None:
            A = _restore(ctx, saved_acts, ("mean_f", "rstd_f", "y2", "gln", "xln2"))
            if ctx.cheap:
                if any(needs["%s@%d" % (n, i)] for i in range(nseg) for n in ("w0", "w1")):
                    A["xln2"] = hip.layernorm_fwd(x2, P["ln2_w"], P["ln2_b"], x_rows=xmap)[0]
                if A["gln"] is None and any(needs["w2@%d" % i] for i in range(nseg)):
                    A["gln"] = torch.empty(N, Fd, dtype=x2.dtype, device=x2.device)
                    for i, sg in enumerate(segs):
                        r = slice(sg.row0, sg.end)
                        hip.ln_geglu_fwd(A["h0"][r], A["h1"][r], P["fln_w@%d" % i], P["fln_b@%d" % i], out=A["gln"][r], want_stats=False,
                                         ps=pss[i] if ctx.zero_rows else None, rows_per_sample=sg.S)
        else:  # recompute (the reference's checkpoint_activations behaviour)
            info = {}
            _, A = FfnBranchMultiFn._compute(x2, segs, pss, params, True, not ctx.dg_fused, xmap=xmap, listed=kept is None and ctx.dg_fused,
                                             info=info)
            assert info["zero_rows"] == ctx.zero_rows
        if not dout.is_contiguous():
            dout = dout.contiguous()
        dout_full = dout
        if kept is not None and not mapped:
            dout = hip.rows_gather(dout_full, kept)
        G = {}
        weight_grad, direct = _weight_grad_fn(ctx, G)
        has_fln = P["fln_w@0"] is not None
        dev, dt = dout.device, dout.dtype
        upstream = need_x or needs["ln2_w"] or needs["ln2_b"] or any(
            needs["%s@%d" % (n, i)] for i in range(nseg) for n in ("w0", "w1", "fln_w", "fln_b"))
        dh = torch.empty(N, 2 * Fd, dtype=dt, device=dev) if upstream else None
        dgln = torch.empty(N, Fd, dtype=dt, device=dev) if upstream else None
        colsets = []
        fold = {} if nseg > 1 else None  # gamma_2 is shared: its gradient accumulates over the segments
        fused = ctx.dg_fused  # gamma_2's gradient from the three down-projection weight gradients (no y2: dgamma_from_wgrad_ok)
        fp8b = FP8_FFN and FP8_FFN_DGRAD and H % 128 == 0 and Fd % 128 == 0
        (rowdot, rd_views), pairs = (_rowdot_slots(dev, [P["w2@%d" % i] for i in range(nseg)]), []) if fused else ((None, None), None)
        # per segment ONE list for its down-projection and wi_0 | wi_1 weight gradients (the segment's own rows), all in one launch
        kts = [None] * nseg
        if kept is None and not any(sg.pad for sg in segs):
            kts = _live_ktiles([(pss[i], sg.row0, sg.S, sg.B) for i, sg in enumerate(segs)], [(sg.row0, sg.rows) for sg in segs], dev)
        # input gradients: list i for segment i's down-projection launch, list nseg for the grouped wi_0 | wi_1 launch of all segments
        # (entries carry the problem index); the fp8 route stays dense
        need_dxln2 = upstream and (need_x or needs["ln2_w"] or needs["ln2_b"])
        wins, dxln2 = None, None
        ln2_one = nseg == 1 and segs[0].row0 == 0 and segs[0].rows == N
        if upstream and kept is None and not any(sg.pad for sg in segs) and not fp8b:
            dxln2 = torch.empty(N, H, dtype=dt, device=dev) if need_dxln2 else None
            # (SKIP_ZERO_ROWS) d LN_F(g) is read by op_ln_geglu_bwd alone, which takes its segment's multipliers; d LN2(x) by the
            # LayerNorm backward over ALL rows, which takes one (ps, S) pair: one segment
            filled, unread = _bwd_fills([(dgln, has_fln), (dxln2, ln2_one)])
            wins = _dgrad_windows([(pss[i], sg.row0, sg.S, sg.B, 1) for i, sg in enumerate(segs)],
                                  [[(i, 0, sg.row0)] for i, sg in enumerate(segs)] + ([[(i, i, sg.row0) for i, sg in enumerate(segs)]] if need_dxln2 else []),
                                  filled,
                                  [(sg.rows, Fd, H) for sg in segs] + ([(sg.rows, H, 2 * Fd) for sg in segs] if need_dxln2 and nseg == 1 else []),
                                  unread=unread)
        zr_b = SKIP_ZERO_ROWS and wins is not None  # the row kernels of this backward leave out the rows of dropped samples
        for i, sg in enumerate(segs):
            r = slice(sg.row0, sg.end)
            k = lambda n: "%s@%d" % (n, i)  # noqa: E731
            g0 = None
            if fused:  # (g0 also switches the kernel to the un-scaled branch gradient: dy2 = ps * dout without gamma_2)
                g0 = torch.empty(H, dtype=torch.float32, device=dev)
                if P[k("b2")] is not None:
                    pairs.append((P[k("b2")], g0))
            dy2 = _resid_backward(dout_full if mapped else dout[r], A["y2"][r] if A["y2"] is not None else None, P["g2"], pss[i], sg.S,
                                  "g2", k("b2"), direct, G, needs, g0=g0, rows=xmap[r] if mapped else None, fold=fold, skip_zero_rows=zr_b)
            if fused:  # (the hook rides on the last segment's problem: by then every (bias, g0) pair is listed)
                weight_grad(k("w2"), dy2, A["gln"][r], side=(P[k("w2")], rd_views[i], P["g2"]),
                            after=_gamma_finish_hook(rowdot, direct["g2"], pairs, True) if i == nseg - 1 else None, ktiles=kts[i])
            elif needs[k("w2")]:
                weight_grad(k("w2"), dy2, A["gln"][r], ktiles=kts[i])
            if not upstream:
                colsets.append(None)
                continue
            w2t = _transposed(P[k("w2")], scale=P["g2"] if fused else None)
            if fp8b:  # (opt-in, round 6) d LN_F(g) = dy W2 on e4m3 operands: the gradient rows and the transposed weight copy row-quantised
                hip.gemm_nt_fp8(*hip.quant_fp8_rows(dy2), *[[x] for x in _fp8_derived(w2t)], out=dgln[r])
            elif wins is None or not _dgrad_listed([dy2], [w2t], [dgln[r]], wins[i], [sg]):
                hip.gemm_nt(dy2, [w2t], out=dgln[r])
            pair = (k("w0"), k("w1"))
            order = _adjacent_grads(direct, pair) if needs[pair[0]] and needs[pair[1]] and Fd % 8 == 0 else None
            cols = tuple(order) if order else pair
            colsets.append(cols)
            dpart = {n: dh[r, j * Fd:(j + 1) * Fd] for j, n in enumerate(cols)}
            if has_fln:
                want = needs[k("fln_w")] or needs[k("fln_b")]
                (tw, tb2), acc = _targets(direct, k("fln_w"), k("fln_b")) if want else ((None, None), False)
                _, _, dw_, db2_ = hip.ln_geglu_bwd(dgln[r], A["h0"][r], A["h1"][r], P[k("fln_w")], A["mean_f"][r], A["rstd_f"][r], dw=tw,
                                                   db=tb2, accumulate=acc, need_wgrad=want, dh0=dpart[pair[0]], dh1=dpart[pair[1]],
                                                   ps=pss[i] if zr_b or ctx.zero_rows else None, rows_per_sample=sg.S)
                if want:
                    _finish(direct, G, (k("fln_w"), k("fln_b")), (dw_, db2_), acc)
            else:
                d0, d1 = hip.geglu_bwd(dgln[r], A["h0"][r], A["h1"][r])
                dpart[pair[0]].copy_(d0)
                dpart[pair[1]].copy_(d1)
            if order:
                wgrad_into(dh[r], A["xln2"][r], _span(direct, order), [direct[n] for n in order], ktiles=kts[i])
            else:
                for n in pair:
                    if needs[n]:
                        weight_grad(n, dpart[n], A["xln2"][r], ktiles=kts[i])
        if fold is not None and needs["g2"] and not fused:  # the fp32 sum of temporaries (_return_grads folds it into a flat view),
            if "g2" in fold:                                   # or every segment accumulated in place
                G["g2"] = fold["g2"].to(dt)
            else:
                _direct_grad_done(direct["g2"])
        dx = None
        if need_dxln2:
            if dxln2 is None:
                dxln2 = torch.empty(N, H, dtype=dt, device=dev)
            rs = [slice(sg.row0, sg.end) for sg in segs]
            wts = [_transposed(tuple(P[n] for n in cols)) for cols in colsets]
            if fp8b:  # one fp8 launch per modality (the grouped persistent launch is bf16 only)
                for r, wt in zip(rs, wts):
                    hip.gemm_nt_fp8(*hip.quant_fp8_rows(dh[r]), *[[x] for x in _fp8_derived(wt)], out=dxln2[r])
            elif wins is not None and _dgrad_listed([dh[r] for r in rs], wts, [dxln2[r] for r in rs], wins[nseg], segs):
                pass
            elif nseg == 1 or hip.gemm_nt_grouped([dh[r] for r in rs], wts, outs=[dxln2[r] for r in rs]) is None:
                for r, wt in zip(rs, wts):
                    hip.gemm_nt(dh[r], [wt], out=dxln2[r])
            want = needs["ln2_w"] or needs["ln2_b"]
            (tw, tb), acc = _targets(direct, "ln2_w", "ln2_b") if want else ((None, None), False)
            dx, dw_, db_ = hip.layernorm_bwd(dxln2, x2, P["ln2_w"], P["ln2_b"], A["mean2"], A["rstd2"], add=dout, dw=tw, db=tb,
                                             accumulate=acc, need_wgrad=want, dx=torch.empty_like(dout_full) if mapped else None, x_rows=xmap,
                                             ps=pss[0] if zr_b and ln2_one else None, rows_per_sample=segs[0].S)
            if want:
                _finish(direct, G, ("ln2_w", "ln2_b"), (dw_, db_), acc)
        if dx is None and need_x:
            dx = dout_full
        elif dx is not None and mapped:
            hip.rows_merge(dout_full, None, kept, out=dx)  # (the dropped samples' rows: the gradient of the skip connection, copied)
        elif dx is not None and kept is not None:
            dx = hip.rows_merge(dout_full, dx, kept)
        grads = _return_grads(names, params, G, direct)
        return (dx, None, None, None, None, *grads)


def ffn_branch_multi(x2, segs, pss, shared, own, save_acts=True, kept=None):
    """shared: (ln2_w, ln2_b, g2); own: per segment (w0, w1, fln_w, fln_b, w2, b2); save_acts False: recompute in backward.
    kept (hip.KeptRows): as attn_branch_multi -- segs and pss describe the packed rows of the kept samples."""
    flat = list(shared)
    for o in own:
        flat += list(o)
    return FfnBranchMultiFn.apply(x2, segs, tuple(pss), _save_flags(save_acts), kept, *flat)


_SCALE_ROWS = {}


def kept_segments(kept, segs, device):
    """The packed-row view of a branch that skips its dropped samples: ([StreamSeg] over the rows of hip.KeptRows `kept`, an fp32
    vector of the drop-path multiplier 1/keep_prob long enough for every row- or sample-indexed use).  segs: the full-matrix
    segments (bias handles and key-padding rows are taken from them; key padding is gathered per kept sample)."""
    out = []
    for i, sg in enumerate(segs):
        key_pad = sg.key_pad.index_select(0, kept.kept_list(i)) if sg.key_pad is not None else None
        out.append(StreamSeg(sg.name, kept.n_kept[i], sg.S, kept.dst_row0[i], sg.bias, key_pad, pad=kept.dst_rows[i] - kept.n_kept[i] * sg.S))
    key = (device, kept.scale)
    vec = _SCALE_ROWS.get(key)
    if vec is None or vec.numel() < kept.total + 8:
        if len(_SCALE_ROWS) > 256:
            _SCALE_ROWS.clear()
        vec = _SCALE_ROWS[key] = torch.full((max(kept.full_rows, kept.total) + 8,), kept.scale, dtype=torch.float32, device=device)
    return out, vec


def _attn_backward(qkv, dattn, attn, lse, B, S, heads, scale, bias_img, biasT, key_pad, dbias_acc, bias_frag, dq, dk, dv):
    """Attention backward; dq / dk / dv: [N, H] column blocks of one packed [N, 3H] gradient matrix (any block order)."""
    H = heads * 64
    dev = qkv.device
    Spad = hip.attn_spad(S)
    delta = torch.empty(B, heads, Spad, dtype=torch.float32, device=dev)  # workspace of the call (rowsum(dO o O), from the dQ kernels)
    if attn.stride(0) != dattn.stride(0) or SEPARATE_DELTA:  # (the fused delta reads both with one row stride)
        hip._check(hip.lib().op_attn_bwd_delta(hip.ptr(dattn), hip.ptr(attn), dattn.stride(0), hip.ptr(delta), B, S, Spad, heads,
                                               hip.stream()), "op_attn_bwd_delta")
        attn = None
    hip.attn_bwd_launch(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], 3 * H, dattn, bias_img, biasT, key_pad, lse, delta, dq, dk,
                        dv, dq.stride(0), dbias_acc, B, S, Spad, heads, scale, bias_frag, out=attn)


def attn_branch(x, bias, key_pad, ps, heads, params, save_acts=False):
    """Single stream: x [B, S, H] contiguous; bias: RelPosBias-like handle or None; key_pad: uint8 [B, Spad] or None; ps: fp32 [B]
    drop-path multipliers or None."""
    B, S, H = x.shape
    seg = StreamSeg("x", B, S, 0, bias, key_pad)
    out = AttnBranchFn.apply(x.reshape(B * S, H), [seg], ps, S, heads, _save_flags(save_acts), None, bias.image if bias is not None else None, *params)
    return out.view(B, S, H)


def attn_branch_multi(x2, segs, ps_rows, heads, params, save_acts=False, kept=None):
    """Lock-step pass: x2 [sum rows, H] holds the rows of several streams (segs); ps_rows: fp32 [sum rows] per-row drop-path
    multipliers or None.  The attention-branch weights are modality-shared (transformer_layer.py:111-138), so LayerNorm, q|k|v,
    sub-LayerNorm and out-proj (and, in backward, their input- and weight-gradient GEMMs) are ONE launch over all rows.
    kept (hip.KeptRows): the branch runs only on the samples stochastic depth keeps -- segs and ps_rows then describe the PACKED
    rows (kept_segments), x2 stays the full matrix; rows of dropped samples pass through unchanged, forward and backward."""
    return AttnBranchFn.apply(x2, segs, ps_rows, 1, heads, _save_flags(save_acts), kept,
                              *[sg.bias.image if sg.bias is not None else None for sg in segs], *params)


def _save_flags(save_acts):
    """bit 0: keep the activations; bit 1: autograd is recording (inside Function.forward grad mode is always off); bit 2: keep them
    WITHOUT the four LayerNorm-type outputs backward can re-create (set_recompute_cheap).  The GeGLU form of
    the FFN is chosen by bit 1 -- not by which parameters happen to be trainable: a frozen branch (stage-2 pretraining) and a trainable
    one must give the same forward bits, and so must a checkpointed forward and its recomputation."""
    return int(bool(save_acts)) | (2 if torch.is_grad_enabled() else 0) | (4 if RECOMPUTE_CHEAP and save_acts else 0)


def ffn_branch(x, ps, params, save_acts=False):
    """Single stream: x [B, S, H] contiguous; ps: fp32 [B] drop-path multipliers or None; params in FFN_PARAMS order."""
    B, S, H = x.shape
    P = dict(zip(FFN_PARAMS, params))
    out = ffn_branch_multi(x.reshape(B * S, H), [StreamSeg("x", B, S, 0)], [ps], [P[n] for n in FFN_SHARED], [[P[n] for n in FFN_OWN]],
                           save_acts)
    return out.view(B, S, H)


# --------------------------------------------------------------------------------------------------------------
# contrastive head
# --------------------------------------------------------------------------------------------------------------
class L2NormalizeFn(torch.autograd.Function):
    """F.normalize(x, dim=1) (one_peace_retrieval.py:112)."""

    @staticmethod
    def forward(ctx, x):
        y, inv = hip.l2norm_fwd(x.contiguous())
        ctx.save_for_backward(y, inv)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, inv = ctx.saved_tensors
        return hip.l2norm_bwd(dy.contiguous(), y, inv)


def l2_normalize(x):
    return L2NormalizeFn.apply(x)


class InfoNCEFn(torch.autograd.Function):
    """image_text_pretrain_loss.py:164-185: both directions of scale * local @ all^T -> fp32 log-softmax -> NLL.

    a_local/b_local: [b, H] bf16 (with grad).  a_all/b_all: [n, H] bf16 gathered copies (no grad flows into them).
    scale: fp32 0-d tensor (logit_scale.exp()).  Returns (loss, a_hits, b_hits)."""

    @staticmethod
    def forward(ctx, a_local, b_local, a_all, b_all, scale, rank, label_smoothing):
        b = a_local.shape[0]
        t0 = rank * b
        scale_f = scale.detach().float().reshape(1)
        sims, rows = [], []
        for loc, allv in ((a_local, b_all), (b_local, a_all)):
            sim = gemm_any(loc.detach(), allv.detach(), out_f32=True, alpha=scale_f)
            loss_r, hit_r, dot_r = hip.infonce_rows(sim, t0, label_smoothing, gscale=0.5 / b, write_grad=True)
            sims.append(sim)  # now holds d loss / d sim
            rows.append((loss_r, hit_r, dot_r))
        loss = 0.5 * (rows[0][0].mean() + rows[1][0].mean())
        ctx.save_for_backward(a_local, b_local, a_all, b_all, scale_f, sims[0], sims[1], rows[0][2], rows[1][2])
        ctx.scale_dtype = scale.dtype
        hits_a, hits_b = rows[0][1].sum(), rows[1][1].sum()
        ctx.mark_non_differentiable(hits_a, hits_b)  # counters for logging, as under the reference's no-grad argmax
        return loss, hits_a, hits_b

    @staticmethod
    def backward(ctx, gl, _ga, _gb):
        a_local, b_local, a_all, b_all, scale_f, ds_ab, ds_ba, dot_ab, dot_ba = ctx.saved_tensors
        g = gl.float()
        coef = (g * scale_f).reshape(1)
        da = gemm_any(ds_ab.to(torch.bfloat16), hip.transpose(b_all.contiguous()), out_f32=True, alpha=coef)
        db = gemm_any(ds_ba.to(torch.bfloat16), hip.transpose(a_all.contiguous()), out_f32=True, alpha=coef)
        dscale = (g * (dot_ab.sum() + dot_ba.sum()) / scale_f).reshape(()).to(ctx.scale_dtype)
        return da.to(a_local.dtype), db.to(b_local.dtype), None, None, dscale, None, None


def info_nce(a_local, b_local, a_all, b_all, scale, rank=0, label_smoothing=0.0):
    return InfoNCEFn.apply(a_local, b_local, a_all, b_all, scale, rank, label_smoothing)


class DclFn(torch.autograd.Function):
    """Masked-token contrastive loss (image_text_pretrain_loss.py:187-208): rows = the MASKED student tokens, columns =
    every teacher token of the batch, target of row i = the teacher token at the same position.

    student [m, H] and teacher [n, H] are L2-normalised bf16; the caller has permuted the teacher rows so that the m
    masked positions come first in student order (softmax is permutation invariant), i.e. the target of row i is column
    i.  The [m, n] similarity matrix (22 k x 32 k at b=128) is never materialised: row blocks of `block` rows go
    through GEMM (fp32) -> op_infonce_rows (loss + d loss / d sim in place) -> GEMM with the teacher, and only the
    [m, H] student gradient is kept for backward.  The teacher carries no gradient (it is detached in the reference)."""

    @staticmethod
    def forward(ctx, student, teacher, scale, label_smoothing, block):
        m, H = student.shape
        teacher = teacher.detach().contiguous()
        teacher_t = hip.transpose(teacher)  # [H, n]: the NT operand of d student = d sim @ teacher
        alpha = torch.full((1,), float(scale), dtype=torch.float32, device=student.device)
        dstudent = torch.empty(m, H, dtype=torch.float32, device=student.device)
        total = torch.zeros((), dtype=torch.float32, device=student.device)
        for r0 in range(0, m, block):
            rows = student[r0:r0 + block].detach().contiguous()
            sim = gemm_any(rows, teacher, out_f32=True, alpha=alpha)
            loss_r, _, _ = hip.infonce_rows(sim, r0, label_smoothing, gscale=1.0 / m, write_grad=True)
            total += loss_r.sum()
            dstudent[r0:r0 + block] = gemm_any(sim.to(torch.bfloat16), teacher_t, out_f32=True, alpha=alpha)
            del sim  # else the next block's sim is allocated while this one is alive: two blocks of sims at the peak
        ctx.save_for_backward(dstudent)
        ctx.dtype = student.dtype
        return total / m

    @staticmethod
    def backward(ctx, g):
        (dstudent,) = ctx.saved_tensors
        return (dstudent * g.float()).to(ctx.dtype), None, None, None, None


def dcl_loss(student, teacher, scale, label_smoothing=0.0, block=4096):
    return DclFn.apply(student, teacher, scale, label_smoothing, block)


# --------------------------------------------------------------------------------------------------------------
# fine-tuning losses (one_peace/criterions/{classify_loss,hinge_loss,refcoco_loss}.py): loss, logged counter and gradient from one
# kernel pass (csrc/losses.hip) instead of a chain of small launches
# --------------------------------------------------------------------------------------------------------------
def loss_hip_eligible(logits):
    """op_row_loss / op_box_loss take bf16 and fp32 CUDA logits [B, C]; anything else runs the reference's torch formulae."""
    return logits.is_cuda and logits.dim() == 2 and logits.dtype in (torch.bfloat16, torch.float32)


class RowLossFn(torch.autograd.Function):
    """(sum of the row losses, sum of the row counters) of op_row_loss, both fp32 0-d; the fp32 gradient is formed in the same pass and
    kept for backward.  The sum over the rows is the kernel's fixed-order fp32 sum."""

    @staticmethod
    def forward(ctx, logits, targets, mode, label_smoothing, margin):
        x = logits.detach()
        if x.stride(1) != 1:
            x = x.contiguous()
        sums, _, _, dlogits = hip.row_loss(x, targets, mode, label_smoothing, margin, write_grad=ctx.needs_input_grad[0])
        if dlogits is not None:
            ctx.save_for_backward(dlogits)
        ctx.dtype = logits.dtype
        loss, counter = sums[0], sums[1]
        ctx.mark_non_differentiable(counter)  # logged, as under the reference's no_grad
        return loss, counter

    @staticmethod
    def backward(ctx, g, _gc):
        (dlogits,) = ctx.saved_tensors
        return (dlogits * g.float()).to(ctx.dtype), None, None, None, None


def _dense_targets(targets, logits):
    targets = targets.to(logits.device)
    if targets.dtype not in (torch.bfloat16, torch.float32):
        targets = targets.float()
    return targets if targets.stride(1) == 1 else targets.contiguous()


def classify_loss(logits, targets, use_multi_label=False, label_smoothing=0.0):
    """(loss_sum, n_correct) of classify_loss.py:51-64 for logits [B, C].  use_multi_label: binary cross-entropy with logits against
    targets [B, C], n_correct = the targets at the arg-max.  Else targets [B, C] are soft labels (they need not sum to 1):
    sum -t logp, n_correct = sum p t; targets [B] int64 are classes: F.cross_entropy with torch's label smoothing (eps / C on every
    class) and ignore_index -100, n_correct = the arg-max hits.  CUDA logits in bf16 / fp32 run op_row_loss (fp32 loss and counter,
    run-to-run identical; a class outside [0, C) other than -100 gives a NaN loss where torch raises a device assert); anything else the
    reference's own torch calls."""
    if loss_hip_eligible(logits):
        if use_multi_label or targets.dim() == 2:
            if tuple(targets.shape) != tuple(logits.shape):
                raise ValueError("classify_loss: targets %s do not match logits %s" % (tuple(targets.shape), tuple(logits.shape)))
            mode = hip.ROW_LOSS_MULTI if use_multi_label else hip.ROW_LOSS_SOFT
            return RowLossFn.apply(logits, _dense_targets(targets, logits), mode, 0.0, 1.0)
        if tuple(targets.shape) != (logits.shape[0],):
            raise ValueError("classify_loss: targets %s do not match logits %s" % (tuple(targets.shape), tuple(logits.shape)))
        return RowLossFn.apply(logits, targets.to(logits.device, torch.int64).contiguous(), hip.ROW_LOSS_HARD, float(label_smoothing), 1.0)
    if use_multi_label:
        loss = F.binary_cross_entropy_with_logits(logits, targets, reduction="sum")
        with torch.no_grad():
            n_correct = targets.gather(1, logits.argmax(1, keepdim=True)).sum()
    elif targets.dim() == 2:
        log_probs = F.log_softmax(logits, dim=-1, dtype=torch.float32)  # fairseq's utils.log_softmax
        loss = (-targets * log_probs).sum()
        with torch.no_grad():
            n_correct = (log_probs.exp() * targets).sum()
    else:
        loss = F.cross_entropy(logits, targets, label_smoothing=label_smoothing, reduction="sum")
        with torch.no_grad():
            n_correct = logits.argmax(1).eq(targets).sum()
    return loss, n_correct


def hinge_loss(logits, targets, margin=1.0):
    """(loss_sum, n_correct) of hinge_loss.py:51-53 for logits [B, num_choices] and int64 targets [B]:
    sum max(0, margin + logits - logits[target]) over every choice, the target's own included, and the arg-max hits.  The reference
    hard-codes `1 +` and ignores its own `margin` option; here margin is honoured, which equals the reference at the default 1.0.
    CUDA logits in bf16 / fp32 run op_row_loss; anything else the reference's torch calls."""
    if loss_hip_eligible(logits):
        if tuple(targets.shape) != (logits.shape[0],):
            raise ValueError("hinge_loss: targets %s do not match logits %s" % (tuple(targets.shape), tuple(logits.shape)))
        return RowLossFn.apply(logits, targets.to(logits.device, torch.int64).contiguous(), hip.ROW_LOSS_HINGE, 0.0, float(margin))
    positive_logits = logits.gather(1, targets.unsqueeze(1))
    loss = torch.max(torch.tensor(0.0).to(logits.device), margin + logits - positive_logits).sum()
    n_correct = logits.argmax(1).eq(targets).sum()
    return loss, n_correct


def giou_diagonal(boxes1, boxes2):
    """The diagonal of torchvision.ops.generalized_box_iou(boxes1, boxes2), boxes [N, 4] as (x1, y1, x2, y2): the published formulae
    (clamped intersection and enclosing extents, iou - (enclosing - union) / enclosing) for the pairs (i, i) only."""
    if boxes1.dtype not in (torch.float32, torch.float64):
        boxes1, boxes2 = boxes1.float(), boxes2.float()  # torchvision's _upcast
    area1 = (boxes1[:, 2] - boxes1[:, 0]) * (boxes1[:, 3] - boxes1[:, 1])
    area2 = (boxes2[:, 2] - boxes2[:, 0]) * (boxes2[:, 3] - boxes2[:, 1])
    wh = (torch.min(boxes1[:, 2:], boxes2[:, 2:]) - torch.max(boxes1[:, :2], boxes2[:, :2])).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]
    union = area1 + area2 - inter
    iou = inter / union
    whi = (torch.max(boxes1[:, 2:], boxes2[:, 2:]) - torch.min(boxes1[:, :2], boxes2[:, :2])).clamp(min=0)
    areai = whi[:, 0] * whi[:, 1]
    return iou - (areai - union) / areai


def box_loss_torch(logits, targets, nsentences=None):
    """refcoco_loss.py:36-46 in torch, the [B, B] GIoU matrix replaced by its diagonal."""
    output_coords = logits.sigmoid()
    loss = F.l1_loss(output_coords, targets, reduction="sum")
    loss = loss / (logits.shape[0] if nsentences is None else nsentences)
    valid_indices = (output_coords[:, :2] < output_coords[:, 2:]).all(1)
    ious = giou_diagonal(output_coords[valid_indices], targets[valid_indices])
    return loss + (1 - ious).mean()


class BoxLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, targets):
        out, dlogits = hip.box_loss(logits.detach().contiguous(), targets, write_grad=ctx.needs_input_grad[0])
        if dlogits is not None:
            ctx.save_for_backward(dlogits)
        ctx.dtype = logits.dtype
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        return (dlogits * g.float()).to(ctx.dtype), None


def box_loss(logits, targets):
    """The loss of refcoco_loss.py:36-46 for box logits [B, 4] and target boxes [B, 4] as (x1, y1, x2, y2) in [0, 1]:
    sum |sigmoid(logits) - targets| / B + the mean of 1 - GIoU over the rows whose predicted box has x1 < x2 and y1 < y2 (NaN when
    there is none, as the mean of an empty tensor).  CUDA logits in bf16 / fp32 run op_box_loss (fp32 loss); anything else the torch
    statement.  No [B, B] GIoU matrix and no torchvision either way."""
    if logits.dim() != 2 or logits.shape[1] != 4 or tuple(targets.shape) != tuple(logits.shape):
        raise ValueError("box_loss: logits and targets must be [B, 4], got %s and %s" % (tuple(logits.shape), tuple(targets.shape)))
    if loss_hip_eligible(logits):
        return BoxLossFn.apply(logits, targets.to(logits.device, torch.float32).contiguous())
    return box_loss_torch(logits, targets)


# --------------------------------------------------------------------------------------------------------------
# fine-tuning head: single-query attention pooling (one_peace_base.py:154-170 between the projections; csrc/attnpool.hip)
# --------------------------------------------------------------------------------------------------------------
def attention_pool_torch(k, v, q, key_padding_mask=None):
    """one_peace_base.py:154-170 with k = k_proj(x), v = v_proj(x) given as [B, S, H]: the same torch ops in the same order and the same
    dtypes (bmm at the input dtype, masked_fill_ with -inf, softmax(dtype=float32), type_as, bmm), on the reference's own layout
    (time-major [S, B * heads, hd] viewed batch-major).  No 1 / sqrt(hd) factor.  key_padding_mask None: nothing is masked."""
    B, S, H = k.shape
    heads, hd = q.shape[-2], q.shape[-1]
    q = q.reshape(1, 1, heads, hd).expand(1, B, -1, -1).reshape(1, B * heads, hd).transpose(0, 1)
    k = k.transpose(0, 1).contiguous().view(S, B * heads, hd).transpose(0, 1)
    v = v.transpose(0, 1).contiguous().view(S, B * heads, hd).transpose(0, 1)
    attn_weights = torch.bmm(q, k.transpose(1, 2))
    attn_weights = attn_weights.view(B, heads, 1, S)
    if key_padding_mask is not None:
        key_padding_mask = key_padding_mask.to(torch.bool).view(B, 1, 1, S).contiguous()
        attn_weights.masked_fill_(key_padding_mask.expand(B, heads, 1, S), -math.inf)
    attn_weights_float = F.softmax(attn_weights, dim=-1, dtype=torch.float32)  # fairseq's utils.softmax
    attn_probs = attn_weights_float.type_as(attn_weights)
    attn_probs = attn_probs.view(B * heads, 1, S)
    attn = torch.bmm(attn_probs, v)
    return attn.reshape(B, H)


class AttentionPoolFn(torch.autograd.Function):
    """op_attn_pool_fwd / op_attn_pool_bwd; the fp32 probabilities [B, heads, S] are kept for the backward, the per-sample partials of
    the query gradient are summed over the batch by one torch.sum (fixed order, no atomics)."""

    @staticmethod
    def forward(ctx, k, v, q, pad):
        out, p = hip.attn_pool_fwd(k, v, q, pad)
        ctx.save_for_backward(k, v, q, p)
        return out

    @staticmethod
    def backward(ctx, dout):
        k, v, q, p = ctx.saved_tensors
        dk, dv, dq_part = hip.attn_pool_bwd(dout.contiguous(), k, v, q, p)
        return dk, dv, torch.sum(dq_part, dim=0).view(q.shape).to(q.dtype), None


def attention_pool(k, v, q, key_padding_mask=None):
    """[B, H] = the heads' softmax(q_h . k_s) weighted sums of v over the unmasked keys (no 1 / sqrt(hd)): MultiheadAttentionPooling
    between its projections.  k, v: [B, S, H]; q: [heads, hd] or the reference's parameter [1, 1, heads, hd]; key_padding_mask: [B, S],
    non-zero = pad.  bf16 CUDA tensors inside the kernels' limits (hip.attn_pool_supported) run op_attn_pool_fwd / _bwd, where a masked
    key is skipped (its k / v rows never read, zero gradient rows); everything else -- CPU, fp32, fp16, hd % 8 != 0, hd > 128,
    S > 4096, unaligned strides -- runs attention_pool_torch.  A sample with every key masked gives NaN either way."""
    heads, hd = q.shape[-2], q.shape[-1]
    if k.dim() != 3 or k.shape != v.shape or k.shape[2] != heads * hd or q.numel() != heads * hd:
        raise ValueError("attention_pool: k %s, v %s must be [B, S, heads * hd] for q %s" % (tuple(k.shape), tuple(v.shape), tuple(q.shape)))
    if key_padding_mask is not None and tuple(key_padding_mask.shape) != tuple(k.shape[:2]):
        raise ValueError("attention_pool: key_padding_mask %s does not match k %s" % (tuple(key_padding_mask.shape), tuple(k.shape)))
    if hip_eligible(k) and hip_eligible(v) and hip_eligible(q):
        if k.stride() != v.stride() and k.is_contiguous():
            v = v.contiguous()
        if hip.attn_pool_supported(k, v, heads, hd):
            pad = key_padding_mask
            if pad is not None:
                pad = pad.to(k.device)
                if pad.dtype not in (torch.bool, torch.uint8):
                    pad = pad != 0
                if pad.shape[1] > 1 and pad.stride(1) != 1:
                    pad = pad.contiguous()
            return AttentionPoolFn.apply(k, v, q.reshape(heads, hd).contiguous(), pad)
    return attention_pool_torch(k, v, q, key_padding_mask)


# --------------------------------------------------------------------------------------------------------------
# vision-branch classifier head: mean of the patch tokens + fc_norm (one_peace_vision/classification/models_vit.py:431-434;
# csrc/tokenpool.hip)
# --------------------------------------------------------------------------------------------------------------
def token_mean_norm_torch(x, weight, bias, eps=1e-5):
    """models_vit.py:432-433 with global_pool: the same torch ops in the same order and dtypes.  x: [B, S, H], row 0 is CLS."""
    x = x[:, 1:, :].mean(dim=1)
    return F.layer_norm(x, (x.shape[-1],), weight, bias, eps)


class TokenMeanNormFn(torch.autograd.Function):
    """op_token_mean_ln_fwd / op_token_mean_ln_bwd; the fp32 mean row and its statistics are kept for the backward, which writes the
    gradient of the whole activation tensor once (CLS row zero).  The [H] parts are cast to the parameters' dtype."""

    @staticmethod
    def forward(ctx, x, weight, bias, eps):
        y, pooled, mean, rstd = hip.token_mean_ln_fwd(x, weight, bias, eps)
        ctx.save_for_backward(pooled, weight, mean, rstd)
        ctx.tokens, ctx.has_bias = x.shape[1], bias is not None
        return y

    @staticmethod
    def backward(ctx, dy):
        pooled, weight, mean, rstd = ctx.saved_tensors
        need_w = weight is not None and ctx.needs_input_grad[1]
        need_b = ctx.has_bias and ctx.needs_input_grad[2]
        need_x = ctx.needs_input_grad[0]
        if not (need_x or need_w or need_b):
            return None, None, None, None
        dy = dy.contiguous()
        if dy.data_ptr() % 16:  # (a view that starts inside a row of a larger buffer: the entry wants 16-byte alignment)
            dy = dy.clone()
        dw = db = parts = None
        if need_w or need_b:
            parts = torch.empty(2, dy.shape[1], dtype=torch.float32, device=dy.device)
        dx, _, _ = hip.token_mean_ln_bwd(dy, pooled, weight, mean, rstd, ctx.tokens, want_dx=need_x, want_parts=False,
                                         dw_part=parts[0] if need_w else None, db_part=parts[1] if need_b else None)
        if parts is not None:
            dw, db = parts.to(dy.dtype).unbind(0)  # the parameters' dtype: bf16 on this route; one cast for the pair
        return dx, dw if need_w else None, db if need_b else None, None


def token_mean_norm(x, weight, bias, eps=1e-5):
    """[B, H] = LayerNorm(mean over the tokens 1 ... S - 1 of x [B, S, H]; weight, bias, eps): OnePeaceViT.forward_head before its Linear.
    bf16 CUDA tensors inside the kernels' limits (hip.token_pool_supported: H % 8 == 0, H <= 8192, 2 <= S <= 65536, strides multiples
    of 8) run op_token_mean_ln_fwd / _bwd, which never read the CLS row and keep the mean in fp32 between the two steps (the reference
    rounds it to bf16 first); everything else -- CPU, fp32, fp16, odd H, unaligned views -- runs token_mean_norm_torch."""
    if x.dim() != 3 or x.shape[1] < 2:
        raise ValueError("token_mean_norm: x %s must be [B, S, H] with S >= 2 (CLS and at least one token)" % (tuple(x.shape),))
    if hip_eligible(x) and all(t is None or hip_eligible(t) for t in (weight, bias)):
        w = weight.contiguous() if weight is not None else None
        b = bias.contiguous() if bias is not None else None
        if hip.token_pool_supported(x, w, b):
            return TokenMeanNormFn.apply(x, w, b, float(eps))
    return token_mean_norm_torch(x, weight, bias, eps)


# --------------------------------------------------------------------------------------------------------------
# video branch (one_peace_vision/video/mmaction_custom/models/backbones/onepeace.py; csrc/frameattn.hip): temporal attention over the
# frames of a clip on the batch-major rows, the packed q|k|v projection and the spatial attention core as autograd functions
# --------------------------------------------------------------------------------------------------------------
def temporal_attention_torch(qkv, B, T, N, heads, scale=None):
    """onepeace.py:234-247 between the projections and the sub-LayerNorm, as called from :331-337, on the project's rows: qkv
    [B * T * N, 3 H] packed q | k | v, row (b, t, n).  The two rearranges of :331 and :337 ('n (b t) d -> t (b n) d' and back) as
    views + copies, q * scaling, bmm, fp32 softmax cast back to the input dtype, bmm.  Returns [B * T * N, H] in the same row order."""
    R, H3 = qkv.shape
    H = H3 // 3
    hd = H // heads
    if R != B * T * N or H3 != 3 * heads * hd:
        raise ValueError("temporal_attention: qkv %s is not [B * T * N = %d, 3 * heads * hd]" % (tuple(qkv.shape), B * T * N))
    scale = hd ** -0.5 if scale is None else scale
    x = qkv.view(B, T, N, 3, heads, hd).permute(3, 1, 0, 2, 4, 5)                      # [3, T, (B, N, heads), hd]: time-major
    q, k, v = (t.reshape(T, B * N * heads, hd).transpose(0, 1) for t in x.unbind(0))   # [B * N * heads, T, hd]
    w = torch.bmm(q * scale, k.transpose(1, 2))
    p = F.softmax(w, dim=-1, dtype=torch.promote_types(w.dtype, torch.float32)).to(w.dtype)  # (in fp32 for bf16 / fp16 inputs)
    a = torch.bmm(p, v)                                                                # [(B, N, heads), T, hd]
    return a.view(B, N, heads, T, hd).permute(0, 3, 1, 2, 4).reshape(R, H)


class TemporalAttentionFn(torch.autograd.Function):
    """op_attn_frames_fwd / op_attn_frames_bwd: the packed q|k|v rows are read where they lie, the output and the packed gradient are
    written in the same row order; only qkv is kept (the backward recomputes p)."""

    @staticmethod
    def forward(ctx, qkv, B, T, N, heads, scale):
        H = qkv.shape[1] // 3
        out = hip.attn_frames_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], B, T, N, heads, scale)
        ctx.save_for_backward(qkv)
        ctx.dims = (B, T, N, heads, scale)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, = ctx.saved_tensors
        B, T, N, heads, scale = ctx.dims
        H = qkv.shape[1] // 3
        if dout.stride(1) != 1 or dout.stride(0) % 8 or dout.stride(0) < H or dout.data_ptr() % 16:
            dout = dout.contiguous()
        return hip.attn_frames_bwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], dout, B, T, N, heads, scale), None, None, None, None, None


def temporal_attention(qkv, B, T, N, heads, scale=None):
    """[B * T * N, H] = softmax_t'(scale * q_t . k_t') v_t' per (video b, token n, head): self-attention over the T frames of a clip on
    the packed q|k|v rows [B * T * N, 3 H] (row (b, t, n)).  bf16 CUDA tensors inside the kernels' limits (hip.attn_frames_supported:
    head_dim 64, T <= 32) run op_attn_frames_fwd / _bwd -- no rearranged copy, p kept in fp32; everything else -- CPU, fp32, fp16,
    hd != 64, T > 32, unaligned views -- runs temporal_attention_torch."""
    if qkv.dim() != 2 or qkv.shape[0] != B * T * N or qkv.shape[1] % (3 * heads):
        raise ValueError("temporal_attention: qkv %s must be [B * T * N = %d, 3 * heads * hd]" % (tuple(qkv.shape), B * T * N))
    hd = qkv.shape[1] // (3 * heads)
    scale = hd ** -0.5 if scale is None else float(scale)
    if hip_eligible(qkv) and hip.attn_frames_supported(qkv, B, T, N, heads, hd):
        return TemporalAttentionFn.apply(qkv, B, T, N, heads, scale)
    return temporal_attention_torch(qkv, B, T, N, heads, scale)


class PackedQKVFn(torch.autograd.Function):
    """[R, 3 H] = x [R, H] through q_proj | k_proj | v_proj as ONE GEMM with the three weights as segments (k_proj has no bias).  A
    frozen weight costs no weight-gradient GEMM and a frozen bias no column sum."""

    @staticmethod
    def forward(ctx, x, wq, bq, wk, wv, bv):
        H = wq.shape[0]
        qkv = hip.gemm_nt(x, [wq, wk, wv], [bq, None, bv], n_seg=H, N=3 * H)
        ctx.save_for_backward(x if any(ctx.needs_input_grad[i] for i in (1, 3, 4)) else None, wq, wk, wv)
        ctx.biases = (bq is not None, bv is not None)
        return qkv

    @staticmethod
    def backward(ctx, dqkv):
        x, wq, wk, wv = ctx.saved_tensors
        H = wq.shape[0]
        if not dqkv.is_contiguous():
            dqkv = dqkv.contiguous()
        need = ctx.needs_input_grad
        dx = hip.gemm_nt(dqkv, [_transposed((wq, wk, wv))]) if need[0] else None
        dws = [wgrad(dqkv[:, i * H:(i + 1) * H], x) if need[j] else None for i, j in ((0, 1), (1, 3), (2, 4))]
        dbq = dbv = None
        want_q, want_v = ctx.biases[0] and need[2], ctx.biases[1] and need[5]
        if want_q or want_v:
            outs = [torch.empty(H, dtype=dqkv.dtype, device=dqkv.device) if w else None for w in (want_q, False, want_v)]
            hip.colsum_segments(dqkv, H, outs)
            dbq, dbv = outs[0], outs[2]
        return dx, dws[0], dbq, dws[1], dws[2], dbv


def packed_qkv(x, wq, bq, wk, wv, bv):
    """x [R, H] bf16 contiguous -> q | k | v [R, 3 H]."""
    return PackedQKVFn.apply(x, wq, bq, wk, wv, bv)


class SpatialAttentionFn(torch.autograd.Function):
    """The attention core of the fused layer on its own: packed q|k|v [B * S, 3 H] in, [B * S, H] out, over hip.attn_fwd /
    hip.attn_bwd_launch exactly as _attn_forward / _attn_backward call them (head_dim 64).  bias: a RelPosBias handle or None, a
    CONSTANT here: the table gets no gradient from this function.  A frozen table is the reference's video fine-tuning state
    (video/train.py:187-190); when the table requires a gradient the caller takes the torch ops for this product instead
    (spatial_attention below raises, video_vit.VideoEncoderLayer routes) -- the kernels' own bias-gradient accumulation stays with
    AttnBranchFn, whose callers it was measured for."""

    @staticmethod
    def forward(ctx, qkv, bias, B, S, heads, scale):
        H = heads * 64
        keep = ctx.needs_input_grad[0]
        attn, lse = hip.attn_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], qkv.stride(0), B, S, heads, scale,
                                 bias.image.detach() if bias is not None else None, None, hip.attn_spad(S), want_lse=keep,
                                 bias_frag=bias.frag if bias is not None and S <= hip.ATTN_RESIDENT_MAX_S else None)
        if keep:
            ctx.save_for_backward(qkv, attn, lse)
        ctx.bias, ctx.dims = bias, (B, S, heads, scale)
        return attn

    @staticmethod
    def backward(ctx, dattn):
        qkv, attn, lse = ctx.saved_tensors
        B, S, heads, scale = ctx.dims
        H = heads * 64
        bias = ctx.bias
        if not dattn.is_contiguous():
            dattn = dattn.contiguous()
        dqkv = torch.empty_like(qkv)
        _attn_backward(qkv, dattn, attn, lse, B, S, heads, scale, bias.image.detach() if bias is not None else None,
                       bias.imageT if bias is not None else None, None, None, bias.frag if bias is not None and S <= 384 else None,
                       dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:])
        return dqkv, None, None, None, None, None


def spatial_attention(qkv, bias, B, S, heads, scale=None):
    """Attention of B sequences of S tokens on packed q|k|v rows [B * S, 3 * heads * 64] (bf16, device, contiguous) with a shared,
    FROZEN relative-position bias (RelPosBias handle or None).  -> [B * S, heads * 64]."""
    if bias is not None and bias.image.requires_grad:
        raise ValueError("spatial_attention: the relative-position table requires a gradient; this core treats the bias as a constant "
                         "(take the torch ops, as video_vit.VideoEncoderLayer does)")
    scale = 64 ** -0.5 if scale is None else float(scale)
    return SpatialAttentionFn.apply(qkv, bias, B, S, heads, scale)


# --------------------------------------------------------------------------------------------------------------
# pretraining masks (csrc/masks.hip; pretrain_masks.py draws the keys): every random choice is select(candidates, k, keys)
# --------------------------------------------------------------------------------------------------------------
def _select_rank(cand, keys, in_row=None):
    """The place of every item of a row in the order of select(): candidates by (key descending, index ascending), then the row's other
    items by index, then what lies beyond the row.  cand, in_row: bool [B, n]; keys: int [B, n], non-negative.  int64 [B, n]."""
    B, n = keys.shape
    idx = torch.arange(n, device=keys.device)
    word = (torch.where(cand, (keys.long() & 0x7FFFFFFF) + 1, torch.zeros((), dtype=torch.int64, device=keys.device)) << 31) | (0x7FFFFFFF - idx)
    if in_row is not None:
        word = torch.where(in_row, word, torch.full((), -1, dtype=torch.int64, device=keys.device))
    order = torch.argsort(word, dim=1, descending=True, stable=True)
    rank = torch.empty_like(order)
    rank.scatter_(1, order, idx.expand(B, n).contiguous())
    return rank


def _preserve_ids(mask, rowlen, width):
    """collate_fn's layout: int64 [B, width] = the ascending positions < rowlen[b] with mask False, then -1; (ids, kept counts)."""
    B, S = mask.shape
    pos = torch.arange(S, device=mask.device).expand(B, S)
    kept = ~mask & (pos < rowlen.view(B, 1))
    first = torch.sort(torch.where(kept, pos, pos + S), dim=1).values
    count = kept.sum(1)
    if width > S:
        first = torch.cat([first, first.new_zeros(B, width - S)], dim=1)
    col = torch.arange(width, device=mask.device).expand(B, width)
    return torch.where(col < count.view(B, 1), first[:, :width], torch.full((), -1, dtype=torch.int64, device=mask.device)), count


def _mask_keys(keys, name, shape=None):
    if not torch.is_tensor(keys) or keys.dim() != 2 or keys.dtype != torch.int32 or (shape is not None and tuple(keys.shape) != tuple(shape)):
        raise ValueError("%s must be an int32 tensor [B, n]%s" % (name, "" if shape is None else " of shape %s" % (tuple(shape),)))
    if keys.shape[1] > hip.MASK_MAX_ITEMS:
        raise ValueError("%s: %d items per row, at most %d" % (name, keys.shape[1], hip.MASK_MAX_ITEMS))
    return keys.contiguous()


def patch_masks(keys_a, keys_b, m1, extra):
    """The image masks of image_text_pretrain_dataset.py:85-104 for a batch: (image_mask bool [B, N + 1], image_ids int64 [B, N + 1 - m1],
    vl_mask bool [B, N + 1], vl_ids int64 [B, m1 - extra + 1]).  keys_a, keys_b: int32 [B, N] >= 0.  image mask = select(all, m1, keys_a)
    (randperm(N)[:m1]); vl mask = (not image-masked) U select(image-masked, extra, keys_b).  Position 0 (CLS) is never masked, patch j is
    position j + 1.  m1 = int(N * image_mask_ratio), extra = int(N * vl_image_mask_ratio) - (N - m1): host ints.  ValueError unless
    0 <= extra <= m1 <= N <= 4096.  CUDA keys: op_mask_patches, one launch; CPU keys: the same rule in torch, the same bits."""
    keys_a = _mask_keys(keys_a, "patch_masks: keys_a")
    keys_b = _mask_keys(keys_b, "patch_masks: keys_b", keys_a.shape)
    B, N = keys_a.shape
    m1, extra = int(m1), int(extra)
    if N < 1 or not 0 <= m1 <= N or not 0 <= extra <= m1:
        raise ValueError("patch_masks: need 0 <= extra <= m1 <= N and N >= 1, got extra %d, m1 %d, N %d" % (extra, m1, N))
    if keys_a.is_cuda:
        return hip.mask_patches(keys_a, m1, keys_b, extra)
    every = torch.ones(B, N, dtype=torch.bool)
    m = _select_rank(every, keys_a) < m1
    vl = ~m | (_select_rank(m, keys_b) < extra)
    cls = torch.zeros(B, 1, dtype=torch.bool)
    m, vl = torch.cat([cls, m], 1), torch.cat([cls, vl], 1)
    rowlen = torch.full((B,), N + 1)
    return m, _preserve_ids(m, rowlen, N + 1 - m1)[0], vl, _preserve_ids(vl, rowlen, m1 - extra + 1)[0]


def word_masks(src_tokens, word_start, keys_a, p, keys_b=None, vl_ratio=None, pad=1, width=None):
    """Whole-word text masks of a batch (add_whole_word_mask, image_text_pretrain_dataset.py:121-139, and the vl text mask of :73-77):
    (mask bool [B, L + 1], ids int64 [B, width], vl_mask, vl_ids (None without keys_b), overflow: a 0-dim bool tensor on the batch's device).
    src_tokens: int64 [B, L] as the model receives it: the caption's tokens, eos, then `pad`; n = non-pad count - 1 tokens, token t at
    position t + 1; position 0 (CLS), eos and pads are never masked.  word_start: uint8 [vocab] on the same device (whole_word_table).
    With W word starts among the row's tokens, k = ceil(float32(W) * p) starts are select(starts, k, keys_a), each masked with the tokens
    after it up to the next start or the caption's end.  vl mask (keys_b and vl_ratio given) = select(tokens not masked,
    int(n * vl_ratio), keys_b); when fewer tokens are unmasked, masked tokens follow in index order (the reference's argsort leaves that
    case open).  A row with n == 0 or W == 0 gets no masked token, where the reference asserts.
    ids: the ascending positions 0 ... n + 1 with mask False, then -1.  width=None takes the batch maximum of each mask, which costs ONE
    device-to-host read; an int, or a pair for (ids, vl_ids), is an upper bound and costs no synchronisation: a row that keeps more
    positions has its ids truncated to the first `width`, and `overflow` is True.
    CUDA tokens: op_mask_words, one launch; CPU tokens: the same rule in torch, the same bits."""
    if not torch.is_tensor(src_tokens) or src_tokens.dim() != 2 or src_tokens.dtype != torch.int64:
        raise ValueError("word_masks: src_tokens must be an int64 tensor [B, L]")
    B, L = src_tokens.shape
    if not 1 <= L <= hip.MASK_MAX_ITEMS:
        raise ValueError("word_masks: L = %d tokens per row, need 1 ... %d" % (L, hip.MASK_MAX_ITEMS))
    keys_a = _mask_keys(keys_a, "word_masks: keys_a", (B, L))
    vl = keys_b is not None
    if vl != (vl_ratio is not None):
        raise ValueError("word_masks: keys_b and vl_ratio go together")
    if vl:
        keys_b = _mask_keys(keys_b, "word_masks: keys_b", (B, L))
    if not 0.0 <= p <= 1.0 or (vl and not 0.0 <= vl_ratio <= 1.0):
        raise ValueError("word_masks: mask ratios must lie in [0, 1]")
    if word_start.dtype != torch.uint8 or word_start.dim() != 1 or word_start.device != src_tokens.device:
        raise ValueError("word_masks: word_start must be a uint8 [vocab] tensor on the tokens' device")
    widths = (None, None) if width is None else (tuple(width) if isinstance(width, (tuple, list)) else (width, width))
    if width is not None and not all(0 <= int(w) <= L + 1 for w in widths):
        raise ValueError("word_masks: width must lie in [0, L + 1]")
    dev = src_tokens.device
    if src_tokens.is_cuda:
        if L > 1 and src_tokens.stride(1) != 1:
            src_tokens = src_tokens.contiguous()
        m, ids, vm, vids, counts = hip.mask_words(src_tokens, word_start.contiguous(), keys_a, p, keys_b, vl_ratio if vl else 0.0, pad,
                                                  widths[0], widths[1])
        if not vl:
            counts = counts[:1]
    else:
        nonpad = src_tokens.ne(pad).sum(1)
        n = (nonpad - 1).clamp(min=0)
        in_cap = torch.arange(L).expand(B, L) < n.view(B, 1)
        vocab = word_start.numel()
        ws = word_start[src_tokens.clamp(0, vocab - 1)].ne(0) & in_cap & (src_tokens >= 0) & (src_tokens < vocab)
        W = ws.sum(1)
        k = torch.ceil(W.float() * p).long().clamp(max=W)  # torch's own rounding of is_word_start.float().sum() * p
        chosen = ws & (_select_rank(ws, keys_a, in_cap) < k.view(B, 1))
        wid = torch.cumsum(ws.long(), 1)  # the word a token belongs to; 0 before the first start
        hit = torch.zeros(B, L + 1, dtype=torch.int64).scatter_add_(1, wid * chosen, chosen.long())
        hit[:, 0] = 0
        tm = hit.gather(1, wid).ne(0) & in_cap
        cls = torch.zeros(B, 1, dtype=torch.bool)
        m = torch.cat([cls, tm], 1)
        rowlen = nonpad + 1
        ids, c0 = _preserve_ids(m, rowlen, L + 1 if widths[0] is None else int(widths[0]))
        vm = vids = None
        counts = c0.view(1, B)
        if vl:
            k2 = (n.double() * vl_ratio).long().clamp(max=n)
            vm = torch.cat([cls, in_cap & (_select_rank(in_cap & ~tm, keys_b, in_cap) < k2.view(B, 1))], 1)
            vids, c1 = _preserve_ids(vm, rowlen, L + 1 if widths[1] is None else int(widths[1]))
            counts = torch.stack([c0, c1])
    if width is None:
        most = counts.max(1).values.tolist() if B else [0] * counts.shape[0]  # the one device-to-host read
        ids = ids[:, :most[0]].contiguous()
        if vl:
            vids = vids[:, :most[1]].contiguous()
        overflow = torch.zeros((), dtype=torch.bool, device=dev)
    else:
        lim = torch.tensor([int(w) for w in widths[:counts.shape[0]]], device=dev).view(-1, 1)
        overflow = (counts > lim).any()
    return m, ids, vm, vids, overflow


def block_counts(frames, mask_prob, mask_length, mask_prob_adjust=0.0):
    """(K, target) of compute_block_mask_1d for a clip of `frames` frames, in Python double arithmetic exactly as data_utils.py:153-157 and
    :191 write them: K = int(T * ((p + adjust) / length)) centres, target = int(T * p) masked frames."""
    T = int(frames)
    return int(T * ((mask_prob + mask_prob_adjust) / mask_length)), int(T * mask_prob)


def block_masks(frames, centers, keys, mask_prob, mask_length, mask_prob_adjust=0.0, width=None, inverse_mask=False, require_same_masks=True,
                expand_adjcent=False, mask_dropout=0.0, non_overlapping=False):
    """compute_block_mask_1d (one_peace/utils/data_utils.py:110-231) on its default path, the one the audio dataset calls, for a batch of
    clips of different lengths: (mask bool [B, Tmax + 1], ids int64 [B, width]).  frames: a host sequence of B frame counts T_b;
    centers: int32 [B, Kmax] in [0, T_b), row b's first K_b are used; keys: int32 [B, Tmax] >= 0; (K_b, target_b) = block_counts(T_b, ...).
    Frames clamp(c + i - length // 2, 0, T_b - 1), i < length, are masked for every centre; with n masked frames, n > target unmasks
    select(masked, n - target, keys) and n < target masks select(unmasked, target - n, keys).  Frame j is position j + 1, position 0
    (CLS) is never masked, rows are padded to the batch width with False.  width=None: max_b(T_b + 1 - target_b), known on the host.
    The other paths of the reference (non_overlapping, expand_adjcent, mask_dropout, inverse_mask, require_same_masks=False) raise
    NotImplementedError.  CUDA keys: op_mask_blocks, one launch; CPU keys: the same rule in torch, the same bits."""
    import numpy as np
    if inverse_mask or not require_same_masks or expand_adjcent or mask_dropout or non_overlapping:
        raise NotImplementedError("block_masks: only compute_block_mask_1d's default path (overlapping blocks, require_same_masks) is provided")
    keys = _mask_keys(keys, "block_masks: keys")
    B, Tmax = keys.shape
    if not torch.is_tensor(centers) or centers.dim() != 2 or centers.dtype != torch.int32 or centers.shape[0] != B or centers.device != keys.device:
        raise ValueError("block_masks: centers must be an int32 tensor [B, Kmax] on the keys' device")
    centers = centers.contiguous()
    Kmax, length = centers.shape[1], int(mask_length)
    frames = [int(t) for t in frames]
    if len(frames) != B or Tmax < 1 or not 1 <= length <= hip.MASK_MAX_ITEMS or Kmax > hip.MASK_MAX_ITEMS or not 0.0 <= mask_prob <= 1.0:
        raise ValueError("block_masks: need B frame counts, 1 <= Tmax, 1 <= mask_length <= %d, Kmax <= %d, 0 <= mask_prob <= 1" % (
            hip.MASK_MAX_ITEMS, hip.MASK_MAX_ITEMS))
    rows = np.zeros((B, 3), dtype=np.int32)
    for b, T in enumerate(frames):
        K, target = block_counts(T, mask_prob, length, mask_prob_adjust)
        if not 0 <= T <= Tmax or not 0 <= K <= Kmax:
            raise ValueError("block_masks: clip %d: T = %d, K = %d, need 0 <= T <= Tmax = %d and 0 <= K <= Kmax = %d" % (b, T, K, Tmax, Kmax))
        rows[b] = (T, K, target)
    need = int((rows[:, 0] + 1 - rows[:, 2]).max()) if B else 1
    width = need if width is None else int(width)
    if not need <= width <= Tmax + 1:
        raise ValueError("block_masks: width = %d, need %d ... %d" % (width, need, Tmax + 1))
    if keys.is_cuda:
        return hip.mask_blocks(rows, centers, keys, length, width)
    T, K, target = (torch.from_numpy(rows[:, i].astype(np.int64)).view(B, 1) for i in range(3))
    f = torch.zeros(B, Tmax + 1, dtype=torch.bool)
    used = torch.arange(Kmax).expand(B, Kmax) < K
    for i in range(length):
        q = torch.minimum((centers.long() + (i - length // 2)).clamp(min=0), (T - 1).clamp(min=0))
        f.scatter_(1, torch.where(used, q, torch.full((), Tmax, dtype=torch.int64)), torch.ones(B, Kmax, dtype=torch.bool))
    f = f[:, :Tmax]
    in_row = torch.arange(Tmax).expand(B, Tmax) < T
    n = f.sum(1, keepdim=True)
    drop = n > target
    change = (f == drop) & in_row & (_select_rank((f == drop) & in_row, keys, in_row) < (n - target).abs())
    f = torch.where(change, ~drop, f)
    m = torch.cat([torch.zeros(B, 1, dtype=torch.bool), f], 1)
    return m, _preserve_ids(m, T.view(B) + 1, width)[0]


# --------------------------------------------------------------------------------------------------------------
# detection branch (one_peace_vision/det/models/onepeace.py; csrc/windowattn.hip): attention inside the 16 x 16 windows of a token map
# on the batch-major rows, with the shared window bias and the decomposed relative positions
# --------------------------------------------------------------------------------------------------------------
def decomposed_rel_index(size, device=None):
    """detectron2's get_rel_pos for q_size == k_size == size and a table of 2 * size - 1 rows: [size, size] with entry (i, j) = i - j +
    size - 1, the row of rel_pos that query coordinate i and key coordinate j share."""
    c = torch.arange(size, device=device)
    return c[:, None] - c[None, :] + (size - 1)


def window_attention_torch(qkv, bias, rel_h, rel_w, B, Hg, Wg, heads, window, scale=None, pad_row=None):
    """det/models/onepeace.py:197-213 between the projections and the sub-LayerNorm as called from :308-325 in a window block, on the
    project's rows: qkv [B * Hg * Wg, 3 H] packed q | k | v, row (b, y, x).  window_partition with padding to a multiple of `window`,
    (q * scale) @ k^T, + bias ([heads, window^2, window^2] or None), add_decomposed_rel_pos with the unscaled q (rel_h, rel_w
    [2 * window - 1, hd] or None together), fp32 softmax cast back, @ v, window_unpartition and the crop.  detectron2 pads the normed
    activation with zeros BEFORE the projections, so a padded token's q | k | v is the projection of a zero row -- q_proj.bias | 0 |
    v_proj.bias in the reference; the caller passes that row as pad_row [3 H].  It defaults to zeros (exact for projections without a
    bias) and matters only on a grid that is not a multiple of `window`.  Any window size, any grid, CPU, fp32, fp16.  Returns
    [B * Hg * Wg, H] in the same row order."""
    R, H3 = qkv.shape
    H = H3 // 3
    hd = H // heads
    if R != B * Hg * Wg or H3 != 3 * heads * hd:
        raise ValueError("window_attention: qkv %s is not [B * Hg * Wg = %d, 3 * heads * hd]" % (tuple(qkv.shape), B * Hg * Wg))
    scale = hd ** -0.5 if scale is None else scale
    w = int(window)
    ph, pw = (w - Hg % w) % w, (w - Wg % w) % w
    Hp, Wp = Hg + ph, Wg + pw
    x = qkv.view(B, Hg, Wg, H3)
    if ph or pw:
        full = (qkv.new_zeros(H3) if pad_row is None else pad_row.to(qkv.dtype)).expand(B, Hp, Wp, H3).clone()
        full[:, :Hg, :Wg] = x
        x = full
    nh, nw = Hp // w, Wp // w
    x = x.view(B, nh, w, nw, w, 3, heads, hd).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B * nh * nw * heads, w * w, hd)
    q, k, v = x.unbind(0)
    attn = torch.bmm(q * scale, k.transpose(1, 2))
    if bias is not None:
        attn = (attn.view(-1, heads, w * w, w * w) + bias.to(attn.dtype)).view(-1, w * w, w * w)
    if rel_h is not None:
        idx = decomposed_rel_index(w, qkv.device)
        rq = q.reshape(-1, w, w, hd)
        th = torch.einsum("bhwc,hkc->bhwk", rq, rel_h.to(q.dtype)[idx])
        tw = torch.einsum("bhwc,wkc->bhwk", rq, rel_w.to(q.dtype)[idx])
        attn = (attn.view(-1, w, w, w, w) + th[:, :, :, :, None] + tw[:, :, :, None, :]).view(-1, w * w, w * w)
    p = F.softmax(attn, dim=-1, dtype=torch.promote_types(attn.dtype, torch.float32)).to(attn.dtype)
    a = torch.bmm(p, v)                                                                # [(B, nh, nw, heads), w * w, hd]
    a = a.view(B, nh, nw, heads, w, w, hd).permute(0, 1, 4, 2, 5, 3, 6).reshape(B, Hp, Wp, H)
    return a[:, :Hg, :Wg].reshape(R, H)


class WindowAttentionFn(torch.autograd.Function):
    """op_attn_window_fwd / op_attn_window_bwd: the packed q|k|v rows are read where they lie, the output and the packed gradient are
    written in the same row order; only the inputs are kept (the backward recomputes s and p).  Gradients for qkv, bias (the sum of the
    kernel's slabs, cast to bias.dtype), rel_h and rel_w (the sum of its parts); slabs and parts are asked for only where
    needs_input_grad says so."""

    @staticmethod
    def forward(ctx, qkv, bias, rel_h, rel_w, B, Hg, Wg, heads, scale):
        H = qkv.shape[1] // 3
        bias_k = None if bias is None else bias.detach().to(torch.bfloat16).contiguous()
        rel_hk = None if rel_h is None else rel_h.detach().to(torch.bfloat16).contiguous()
        rel_wk = None if rel_w is None else rel_w.detach().to(torch.bfloat16).contiguous()
        out = hip.attn_window_fwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], bias_k, rel_hk, rel_wk, B, Hg, Wg, heads, scale)
        ctx.save_for_backward(qkv, bias_k, rel_hk, rel_wk)
        ctx.dims = (B, Hg, Wg, heads, scale)
        ctx.dtypes = (None if bias is None else bias.dtype, None if rel_h is None else rel_h.dtype, None if rel_w is None else rel_w.dtype)
        return out

    @staticmethod
    def backward(ctx, dout):
        qkv, bias, rel_h, rel_w = ctx.saved_tensors
        B, Hg, Wg, heads, scale = ctx.dims
        H = qkv.shape[1] // 3
        if dout.stride(1) != 1 or dout.stride(0) % 8 or dout.stride(0) < H or dout.data_ptr() % 16:
            dout = dout.contiguous()
        need = ctx.needs_input_grad
        want_dbias = bias is not None and need[1]
        want_drel = rel_h is not None and (need[2] or need[3])
        dqkv, parts, slabs = hip.attn_window_bwd(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], bias, rel_h, rel_w, dout, B, Hg, Wg, heads,
                                                 scale, want_drel=want_drel, want_dbias=want_dbias)
        dbias = slabs.sum(0).to(ctx.dtypes[0]) if want_dbias else None
        drel = parts.sum(0) if want_drel else None
        drel_h = drel[0].to(ctx.dtypes[1]) if want_drel and need[2] else None
        drel_w = drel[1].to(ctx.dtypes[2]) if want_drel and need[3] else None
        return dqkv if need[0] else None, dbias, drel_h, drel_w, None, None, None, None, None


def window_attention(qkv, bias, rel_h, rel_w, B, Hg, Wg, heads, window, scale=None, pad_row=None):
    """[B * Hg * Wg, H]: softmax attention inside the window x window windows of a [B, Hg, Wg] token map on the packed q|k|v rows
    [B * Hg * Wg, 3 H] (row (b, y, x)), with the shared bias [heads, window^2, window^2] and the decomposed relative positions rel_h,
    rel_w [2 * window - 1, hd] (each may be None; rel_h and rel_w together).  bf16 CUDA tensors inside the kernels' limits
    (hip.attn_window_supported: head_dim 64, window 16, a grid of multiples of 16) run op_attn_window_fwd / _bwd -- no partitioned copy,
    no expanded bias, s and p in fp32; everything else -- CPU, fp32, fp16, other windows, grids that need padding -- runs
    window_attention_torch (see there for pad_row)."""
    if qkv.dim() != 2 or qkv.shape[0] != B * Hg * Wg or qkv.shape[1] % (3 * heads):
        raise ValueError("window_attention: qkv %s must be [B * Hg * Wg = %d, 3 * heads * hd]" % (tuple(qkv.shape), B * Hg * Wg))
    if (rel_h is None) != (rel_w is None):
        raise ValueError("window_attention: rel_h and rel_w must be given together")
    hd = qkv.shape[1] // (3 * heads)
    scale = hd ** -0.5 if scale is None else float(scale)
    tables = [t for t in (bias, rel_h, rel_w) if t is not None]
    if (hip_eligible(qkv) and all(t.is_cuda for t in tables) and hip.attn_window_supported(qkv, B, Hg, Wg, heads, hd, window)
            and (bias is None or tuple(bias.shape) == (heads, 256, 256))):
        return WindowAttentionFn.apply(qkv, bias, rel_h, rel_w, B, Hg, Wg, heads, scale)
    return window_attention_torch(qkv, bias, rel_h, rel_w, B, Hg, Wg, heads, window, scale, pad_row)
