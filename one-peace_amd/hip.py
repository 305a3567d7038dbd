"""ctypes binding of the C-ABI HIP library (include/onepeace_hip.h).

Every entry point takes raw device pointers + sizes + a hipStream_t; this module converts torch tensors,
passes ``torch.cuda.current_stream()`` and turns a non-zero return code into ``RuntimeError`` (so the
reference trainer's OOM / NaN handling paths still see Python exceptions).  There is NO CPU
fallback here: if the library is missing, loading fails loudly.
"""
import ctypes
import os
from ctypes import c_double, c_float, c_int, c_int64, c_ubyte, c_void_p

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ONEPEACE_HIP_LIB") or os.path.join(_HERE, "lib", "libonepeace_hip.so")  # (override: instrumented builds of tools/)
_lib = None

DT_BF16, DT_F32 = 0, 1
EPI_BIAS, EPI_F32, EPI_GEGLU, EPI_RESID = 0, 1, 2, 3
PROF_GEMM, PROF_ATTN = 0, 1
ATTN_RESIDENT_MAX_S = 320  # sequences up to this length run the resident-K/V attention kernels (csrc/attention.hip: RES_MAX_S)

P = c_void_p
I64 = c_int64

# name -> (restype, argtypes); kept in the order of include/onepeace_hip.h
SIGNATURES = {
    "op_abi_version": (c_int, []),
    "op_last_error": (ctypes.c_char_p, []),
    "op_prof_enable": (c_int, [c_int]),
    "op_prof_reserve": (c_int, [c_int]),
    "op_prof_collect": (c_int, [P, P, P, c_int]),
    "op_layernorm_fwd": (c_int, [P, P, P, P, P, P, I64, I64, c_float, c_int, c_int, P, P]),
    "op_layernorm_bwd_workspace_bytes": (I64, [I64, I64]),
    "op_attn_bwd_dbias_slabs": (I64, [I64, I64, I64, I64]),
    "op_layernorm_bwd": (c_int, [P, P, P, P, P, P, P, P, P, P, P, I64, I64, c_int, c_int, c_int, P, P]),
    "op_gemm_plan": (c_int, [c_int64, c_int64, c_int64, c_int, c_int, c_int64, I64, P]),
    "op_gemm_nt": (c_int, [P, I64, P, P, P, I64, I64, P, P, P, P, I64, P, P, P, I64, P, P, I64, P, I64, I64, I64,
                           c_int, P, I64, I64, P, I64, P]),
    "op_gemm_nt_grouped": (c_int, [I64, P, P, I64, P, I64, P, P, I64, P, P, P, I64, P, P, P, I64, I64, c_int, I64, P, I64, P]),
    "op_gemm_tn": (c_int, [P, I64, P, I64, P, I64, I64, I64, I64, c_int, P, I64, I64, P]),
    "op_gemm_tn_grouped_counter_bytes": (I64, []),
    "op_gemm_tn_grouped_plan": (I64, [I64, P, P, P, I64, I64, P, I64]),
    "op_gemm_tn_grouped": (c_int, [I64, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, I64, P]),
    "op_gemm_tn_grouped_lists": (c_int, [I64, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, P, I64, P]),
    "op_live_ktiles": (c_int, [I64, P, P, P, P, I64, P, P, P, P, P]),
    "op_live_mwindows": (c_int, [I64, P, P, P, P, P, P, P, P, P, P, I64, P, P, P, I64, P, P, P, P, P]),
    "op_gemm_nt_grouped_windows": (c_int, [I64, P, P, I64, P, I64, P, I64, I64, I64, P, P, I64, I64, I64, P]),
    "op_live_mwindows_fwd": (c_int, [I64, P, P, P, P, P, P, P, P, P, P, I64, P, P, P, I64, P, P, P, P, P, P, P]),
    "op_gemm_nt_grouped_windows_fwd": (c_int, [I64, P, P, I64, P, I64, I64, P, P, I64, P, I64, P, P, P, I64, I64, c_int, P, P, I64, I64,
                                               I64, P]),
    "op_gemm_nt_batched": (c_int, [P, I64, I64, P, I64, I64, P, I64, P, I64, I64, I64, I64, I64, I64, P]),
    "op_audio_conv1_ln_gelu_fwd": (c_int, [P, I64, P, P, P, P, P, P, P, I64, I64, c_float, P]),
    "op_audio_conv1_ln_gelu_bwd_workspace_bytes": (I64, [I64]),
    "op_audio_conv1_ln_gelu_bwd": (c_int, [P, P, I64, P, P, P, P, P, P, P, P, P, P, P, I64, I64, c_int, P]),
    "op_transpose": (c_int, [P, P, I64, I64, I64, I64, P]),
    "op_transpose_scaled": (c_int, [P, P, I64, I64, I64, I64, P, P]),
    "op_transpose_batched": (c_int, [P, I64, I64, P]),
    "op_transpose_desc_bytes": (I64, []),
    "op_colsum_workspace_bytes": (I64, [I64]),
    "op_colsum_segments": (c_int, [P, P, P, P, P, I64, I64, I64, c_int, P]),
    "op_resid_bwd_workspace_bytes": (I64, [I64]),
    "op_resid_bwd": (c_int, [P, P, P, P, I64, P, P, P, P, P, I64, I64, c_int, P, P]),
    "op_resid_bwd_skip": (c_int, [P, P, P, P, I64, P, P, P, P, P, I64, I64, c_int, P, P]),
    "op_layernorm_bwd_skip": (c_int, [P, P, P, P, P, P, P, P, P, P, I64, I64, c_int, P, I64, P]),
    "op_gamma_grad_finish": (c_int, [P, I64, P, P, P, P, P, P, P, I64, c_int, P]),
    "op_ln_geglu_bwd": (c_int, [P, P, P, P, P, P, P, P, I64, I64, P, P, P, I64, I64, c_int, P]),
    "op_ln_geglu_fwd": (c_int, [P, P, I64, P, P, P, P, P, I64, I64, c_float, P]),
    "op_ln_geglu_bwd_skip": (c_int, [P, P, P, P, P, P, P, P, I64, I64, P, P, P, I64, I64, c_int, P, I64, P]),
    "op_ln_geglu_fwd_skip": (c_int, [P, P, I64, P, P, P, P, P, I64, I64, c_float, P, I64, P]),
    "op_colsum": (c_int, [P, P, P, I64, P, P, P, I64, I64, c_int, c_int, P]),
    "op_geglu_bwd": (c_int, [P, P, P, P, P, I64, P]),
    "op_scale_rows": (c_int, [P, P, P, I64, P, I64, I64, P]),
    "op_l2norm_fwd": (c_int, [P, P, P, I64, I64, c_float, c_int, P]),
    "op_l2norm_bwd": (c_int, [P, P, P, P, I64, I64, c_int, P]),
    "op_infonce_rows": (c_int, [P, I64, I64, I64, I64, c_float, c_float, P, P, P, c_int, P]),
    "op_adamw_step": (c_int, [P, P, P, P, I64, c_float, c_float, c_float, c_float, c_float, I64, c_float, P, c_float, P]),
    "op_adamw_step_groups": (c_int, [P, P, P, P, I64, P, P, P, I64, c_float, c_float, c_float, c_float, I64, c_float, P, c_float, P]),
    "op_adamw_step_groups_master": (c_int, [P, P, P, P, P, I64, P, P, P, I64, c_float, c_float, c_float, c_float, I64, c_float, P,
                                           c_float, P]),
    "op_ema_step": (c_int, [P, P, I64, c_float, c_float, P]),
    "op_adamw_step_groups_ema": (c_int, [P, P, P, P, P, P, I64, P, P, P, I64, c_float, c_float, c_float, c_float, I64, c_float, P,
                                        c_float, c_float, c_float, P]),
    "op_adamw_step_shard": (c_int, [P, P, I64, I64, I64, P, P, P, P, P, P, P, I64, c_float, c_float, c_float, c_float, I64, c_float, P,
                                   c_float, c_float, c_float, P]),
    "op_sqnorm": (c_int, [P, I64, P, P, P]),
    "op_relpos_bias_build": (c_int, [P, P, I64, P, I64, I64, I64, c_int, P]),
    "op_relpos_bias_bwd": (c_int, [P, I64, I64, P, P, I64, P, I64, P, P, I64, P]),
    "op_relpos_bias_build_ids": (c_int, [P, P, I64, P, P, I64, I64, I64, I64, c_int, P]),
    "op_relpos_bias_fold_ids": (c_int, [P, P, P, I64, I64, I64, I64, I64, P]),
    "op_attn_fwd": (c_int, [P, P, P, I64, P, I64, P, P, P, I64, P, I64, I64, I64, I64, I64, I64, c_float, I64, P]),
    "op_attn_bias_frag_elems": (I64, [I64, I64]),
    "op_attn_bias_pack": (c_int, [P, P, I64, I64, I64, P]),
    "op_attn_bwd_delta": (c_int, [P, P, I64, P, I64, I64, I64, I64, P]),
    "op_attn_bwd": (c_int, [P, P, P, I64, P, P, I64, P, P, P, I64, P, P, P, P, P, P, I64, P, I64, I64, I64, I64, I64, c_float, I64, P]),
    "op_quant_fp8_rows": (c_int, [P, I64, P, I64, P, I64, I64, P]),
    "op_layernorm_fwd_q8": (c_int, [P, P, P, P, P, P, P, P, I64, I64, c_float, P]),
    "op_ln_geglu_fwd_q8": (c_int, [P, P, I64, P, P, P, P, P, P, P, I64, I64, c_float, P]),
    "op_gemm_nt_fp8": (c_int, [P, I64, P, P, P, I64, P, P, P, P, I64, P, P, P, I64, P, P, I64, I64, I64, I64, c_int, I64, P]),
    "op_rows_gather": (c_int, [P, P, P, I64, P, P, P, P, P, P, P, I64, I64, P]),
    "op_rows_merge": (c_int, [P, P, P, P, I64, P, P, P, P, P, P, P, I64, I64, P]),
    "op_rows_map": (c_int, [P, P, I64, P, P, P, P, P, P, P, I64, P]),
    "op_sim_topk_splits": (I64, [I64, I64, I64]),
    "op_sim_topk_workspace_bytes": (I64, [I64, I64, I64, I64]),
    "op_sim_topk": (c_int, [P, I64, P, I64, I64, I64, I64, I64, P, P, P, I64, I64, P]),
    "op_image_resize_normalize": (c_int, [P, I64, P, P, I64, P, I64, I64, P, P, P, c_int, P, I64, P]),
    "op_image_resize_normalize_flip": (c_int, [P, I64, P, P, I64, P, I64, I64, P, P, P, c_int, P, I64, P, P]),
    "op_mix_images": (c_int, [P, P, c_int, c_int, I64, I64, I64, I64, P, P, P, P, P]),
    "op_image_color_jitter": (c_int, [P, I64, I64, P, P, P, P, P, P]),
    "op_image_gaussian_blur": (c_int, [P, I64, I64, P, P, P, P, P, P, P]),
    "op_image_normalize_flip": (c_int, [P, I64, I64, P, P, P, c_int, P, P]),
    "op_image_randaug_layer": (c_int, [P, I64, I64, P, P, P, P, P, P, P, P]),
    "op_image_erase": (c_int, [P, c_int, I64, I64, P, P, P, P, P]),
    "op_audio_normalize_pad": (c_int, [P, I64, P, P, I64, I64, I64, P, I64, c_int, P, I64, P]),
    "op_audio_resample": (c_int, [P, I64, P, P, I64, P, I64, P, I64, P]),
    "op_average_precision_workspace_bytes": (I64, [I64, I64]),
    "op_average_precision": (c_int, [P, I64, P, I64, I64, I64, P, P, P, I64, P]),
    "op_row_loss": (c_int, [P, c_int, I64, P, c_int, I64, I64, I64, c_int, c_float, c_float, c_float, P, P, P, P, P]),
    "op_box_loss": (c_int, [P, c_int, P, I64, c_float, P, P, P]),
    "op_attn_pool_fwd": (c_int, [P, P, I64, I64, P, P, I64, P, P, I64, I64, I64, I64, P]),
    "op_attn_pool_bwd": (c_int, [P, P, P, I64, I64, P, P, P, P, I64, I64, P, I64, I64, I64, I64, P]),
    "op_token_mean_ln_fwd": (c_int, [P, I64, I64, P, P, c_float, P, P, P, P, P, I64, I64, I64, P]),
    "op_token_mean_ln_bwd": (c_int, [P, P, P, P, P, P, I64, I64, P, P, I64, I64, I64, P]),
    "op_attn_frames_fwd": (c_int, [P, P, P, I64, P, I64, I64, I64, I64, I64, I64, c_float, P]),
    "op_attn_frames_bwd": (c_int, [P, P, P, I64, P, I64, P, P, P, I64, I64, I64, I64, I64, I64, c_float, P]),
    "op_attn_window_parts": (c_int, [I64, I64, I64, P, P]),
    "op_attn_window_fwd": (c_int, [P, P, P, I64, P, P, P, P, I64, I64, I64, I64, I64, I64, I64, c_float, P]),
    "op_attn_window_bwd": (c_int, [P, P, P, I64, P, P, P, P, I64, P, P, P, I64, P, P, I64, I64, I64, I64, I64, I64, c_float, P]),
    "op_mask_patches": (c_int, [P, P, I64, I64, I64, I64, P, P, P, P, P]),
    "op_mask_words": (c_int, [P, I64, I64, I64, I64, P, I64, P, P, c_float, c_double, P, P, I64, P, P, I64, P, P]),
    "op_mask_blocks": (c_int, [P, P, P, I64, P, I64, I64, I64, P, P, I64, P]),
}


# libonepeace_probe.so (include/onepeace_probe.h): lane-map and power probes -- test / measurement infrastructure, not product ABI
PROBE_SIGNATURES = {
    "op_last_error": (ctypes.c_char_p, []),
    "op_probe_mfma16": (c_int, [P, P, P, c_int, P]),
    "op_probe_mfma32": (c_int, [P, P, P, c_int, P]),
    "op_probe_tr16": (c_int, [P, P, P, c_int, P]),
    "op_probe_glds": (c_int, [P, P, c_int, P, P]),
    "op_probe_mfma_f8": (c_int, [P, P, P, P, P, c_int, P]),
    "op_probe_mfma_rate": (c_int, [P, P, P, c_int, c_int, P]),
    "op_probe_lds_atomic": (c_int, [P, P, c_int, c_int, c_int, P]),
    "op_probe_occupy": (c_int, [P, ctypes.c_longlong, c_int, ctypes.c_longlong, P, P]),
}


class Tuning:
    """Kernel-flavour selection for tests and tools.  The C library keeps no tuning state: every GEMM / attention entry point
    takes a per-call `tune` word (include/onepeace_hip.h), and this host-side object is where the Python binding keeps the
    values it passes.  Production code never touches it (all zeros = the defaults)."""

    def __init__(self):
        self.reset()

    def reset(self):
        self.tile_mode = 0       # 0 auto, 1 force 128x128, 2 force 256x256
        self.fullline = 2        # flavour of the 256x256 NT kernel: 0 BK = 32, 1 eight-wave full-line, 2 auto, 3 four-wave full-line
        self.tail_rows = 1       # 0 off, 1 default, 2 whenever it saves a round, 3 always
        self.gm = 0              # M-tiles per L2 group (0 auto)
        self.force_splits = 0    # forced K-split count of small problems (tools)
        self.glds = 1            # 1 LDS-DMA staging, 0 register-staged operands
        self.sched = int(os.environ.get("ONEPEACE_TUNE_SCHED", "0"))  # four-wave NT launches: 0 auto (persistent gemm256p_kernel for K <= 2048), 1 / 3 gemm256v_kernel, 6 gemm256p_kernel for every single problem (A/B), 7 one tile per workgroup: gemm256v_kernel, grouped launches unrolled into the tile list (distributed.share_cus_with_collectives)
        self.fp8_small = 0       # op_gemm_nt_fp8: 1 = keep the 128 x 128 kernel (tests, A/B)
        self.merge_dbias = 1     # attention backward: 1 merged dQ + dBias kernel, 0 separate kernels
        self.resident = 1        # attention forward: bit 0 resident kernels on; bits 1-2 ablations (tools)
        self.attn_waves = 0      # resident forward kernel: waves per workgroup (0 = production rule; tests / A-B timing)
        self.attn_pers = 1       # attention forward: 1 persistent kernel for 193 ... 257 tokens (round 4), 0 the resident one
        self.dbias_chunks_r2 = 0  # merged dQ + dBias kernel: round 2's batch-chunk rule (A/B timing)
        self.dkdv_keys = 0       # dK/dV kernel: 0 auto, 1 = 128 keys per workgroup, 2 = 64 (A/B timing)
        self.dbias_chunks = 0    # merged dQ + dBias kernel: forced number of batch chunks (0 = the library's rule; A/B timing)
        self.attn_pers_dkdv = 1  # attention backward: persistent dK / dV kernel behind the persistent dQ kernel (round 4), 0 the rounds 1-3 kernel
        self.attn_lone_keys = 1  # dK/dV: a trailing block of <= 16 keys (the 257th token) split over the waves by queries (round 4), 0 one wave
        self.attn_pers_bwd = 1   # attention backward: 1 persistent dQ (+ dBias) kernel for 193 ... 257 tokens (round 4), 0 rounds 1-3

    def gemm(self):
        fl = {2: 0, 0: 1, 1: 2, 3: 3}.get(self.fullline, 0)
        tr = 0 if self.tail_rows == 1 else self.tail_rows + 1
        return (self.tile_mode | fl << 2 | tr << 4 | (self.gm & 31) << 7 | (self.force_splits & 15) << 15
                | (0 if self.glds else 1) << 19 | (self.sched & 7) << 20)

    def attn_fwd(self):
        return (0 if self.resident & 1 else 1) | ((self.resident >> 1) & 3) << 1 | (self.attn_waves & 15) << 3 | (0 if self.attn_pers else 128)

    def attn_bwd(self):
        return ((0 if self.merge_dbias else 1) | (2 if self.dbias_chunks_r2 else 0) | (self.dkdv_keys & 3) << 2 | (self.dbias_chunks & 63) << 4
                | (0 if self.attn_pers_bwd else 1024) | (0 if self.attn_lone_keys else 2048) | (0 if self.attn_pers_dkdv else 4096))


TUNE = Tuning()


class _LibProxy:
    """The ctypes library plus the historical op_*_set_* knob functions, now pure Python on `TUNE` (tools/ and tests/ written
    against the round-1 ABI keep working; the shared library no longer exports or stores any knob)."""

    def __init__(self, cdll):
        self._cdll = cdll

    def __getattr__(self, name):
        return getattr(self._cdll, name)

    @staticmethod
    def op_gemm_set_tile(mode):
        old = TUNE.tile_mode
        if mode >= 60:
            TUNE.force_splits = mode - 60
        elif mode >= 50:
            TUNE.tail_rows = mode - 50
        elif mode >= 40:
            TUNE.gm = mode - 40
        elif mode >= 20:
            if 0 <= mode - 20 <= 3:  # other values were ignored by the round-1 C knob as well
                TUNE.fullline = mode - 20
        elif mode >= 10:
            pass  # (rounds 1-4: timing ablations of the BK = 32 kernel, removed in round 5)
        else:
            TUNE.tile_mode = mode
        return old

    @staticmethod
    def op_gemm_set_staging(glds):
        old, TUNE.glds = TUNE.glds, 1 if glds else 0
        return old

    @staticmethod
    def op_attn_set_merge_dbias(on):
        old, TUNE.merge_dbias = TUNE.merge_dbias, 1 if on else 0
        return old

    @staticmethod
    def op_attn_set_resident(mode):
        old, TUNE.resident = TUNE.resident, int(mode)
        return old


def lib():
    """Load the shared library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                "%s not found: build it with `python one-peace_amd/build.py` (hipcc, gfx950). "
                "There is no CPU fallback for the HIP path." % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = _LibProxy(L)
    return _lib


_probe_lib = None


def probe_lib():
    """The probe library (tests/test_probes_gpu.py, bench.py's power-limited MFMA rate); built next to the product library."""
    global _probe_lib
    if _probe_lib is None:
        path = os.path.join(os.path.dirname(LIB_PATH), "libonepeace_probe.so")
        if not os.path.exists(path):
            raise RuntimeError("%s not found: build it with `python one-peace_amd/build.py`" % path)
        L = ctypes.CDLL(path)
        for name, (res, args) in PROBE_SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _probe_lib = L
    return _probe_lib


def _check_probe(rc, what):
    if rc != 0:
        msg = probe_lib().op_last_error()
        raise RuntimeError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ""))


def available():
    return os.path.exists(LIB_PATH) and torch.cuda.is_available()


def _check(rc, what):
    if rc != 0:
        msg = lib().op_last_error()
        raise RuntimeError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ""))


def ptr(t):
    return None if t is None else c_void_p(t.data_ptr())


def stream():
    return c_void_p(torch.cuda.current_stream().cuda_stream)


def _dt(t):
    if t.dtype == torch.bfloat16:
        return DT_BF16
    if t.dtype == torch.float32:
        return DT_F32
    raise TypeError("unsupported dtype %s" % t.dtype)


def _req(t, name, dtype=None):
    if t is None:
        return
    if not t.is_cuda:
        raise RuntimeError("%s must be a CUDA(HIP) tensor" % name)
    if not t.is_contiguous():
        raise RuntimeError("%s must be contiguous" % name)
    if dtype is not None and t.dtype != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, t.dtype))


# ---------------------------------------------------------------------------------------------------
# thin tensor-level wrappers (no autograd here; see ops.py)
# ---------------------------------------------------------------------------------------------------
def layernorm_fwd(x2d, w, b, eps=1e-5, gelu=False, want_stats=True, q8=False, x_rows=None):
    """q8=True (bf16, no GELU): returns (y, mean, rstd, (fp8 bytes, row scales)) -- the output also row-quantised to e4m3, bit-identical
    to quant_fp8_rows(y), without a pass of its own.  x_rows (int32 [rows], KeptRows.rowmap): the input rows are rows x_rows[r] of the
    larger matrix x2d (< 0: a row of zeros); the outputs have x_rows.numel() rows."""
    _req(x2d, "x")
    rows, cols = x2d.shape
    if x_rows is not None:
        assert not q8 and x_rows.dtype == torch.int32 and x_rows.is_contiguous()
        rows = x_rows.numel()
    y = torch.empty(rows, cols, dtype=x2d.dtype, device=x2d.device)
    mean = rstd = None
    if want_stats:
        mean = torch.empty(rows, dtype=torch.float32, device=x2d.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    if q8:
        assert not gelu and x2d.dtype == torch.bfloat16
        q = torch.empty(rows, cols, dtype=torch.uint8, device=x2d.device)
        qs = torch.empty(rows, dtype=torch.float32, device=x2d.device)
        _check(lib().op_layernorm_fwd_q8(ptr(x2d), ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), ptr(q), ptr(qs), rows, cols, eps, stream()),
               "op_layernorm_fwd_q8")
        return y, mean, rstd, (q, qs)
    _check(lib().op_layernorm_fwd(ptr(x2d), ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), rows, cols, eps,
                                  int(gelu), _dt(x2d), ptr(x_rows), stream()), "op_layernorm_fwd")
    return y, mean, rstd


_ws_cache = {}


def workspace(nbytes, device, tag="ws"):
    """Grow-only scratch buffer per (device, tag, stream); caller-owned memory as the C ABI requires."""
    key = (device, tag, torch.cuda.current_stream(device).cuda_stream)  # per stream: launches on different streams may overlap
    buf = _ws_cache.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=device)
        _ws_cache[key] = buf
    return buf


def layernorm_bwd(dy, x, w, b, mean, rstd, gelu=False, need_wgrad=True, dw=None, db=None, accumulate=False, add=None,
                  dx=None, x_rows=None, ps=None, rows_per_sample=1):
    """x_rows (int32 [rows of dy]): x, add and dx are rows x_rows[r] of larger matrices; dx must be given (dx = add: in place, the
    rows no entry names keep `add`).
    ps (bf16, no GELU, no x_rows; fp32, one stochastic-depth multiplier per rows_per_sample rows): the rows of samples with ps == 0 are
    not read -- dx gets +0 there or the bits of `add`, dw / db nothing (op_layernorm_bwd_skip)."""
    rows, cols = x.shape
    if x_rows is not None:
        assert dx is not None and dx.shape == x.shape and (add is None or add.shape == x.shape) and x_rows.dtype == torch.int32
        rows = x_rows.numel()
        assert dy.shape[0] == rows
    if dx is None:
        dx = torch.empty_like(x)
    ws = None
    if need_wgrad and w is not None:
        if dw is None:
            dw = torch.empty_like(w)
            db = torch.empty_like(w)
            accumulate = False
        ws = workspace(lib().op_layernorm_bwd_workspace_bytes(rows, cols), x.device, "ln")
    else:
        dw = db = None
    if ps is not None:
        assert x.dtype == torch.bfloat16 and not gelu and x_rows is None
        _check(lib().op_layernorm_bwd_skip(ptr(dy), ptr(x), ptr(w), ptr(mean), ptr(rstd), ptr(add), ptr(dx), ptr(dw), ptr(db), ptr(ws), rows,
                                           cols, int(accumulate), *_skip_args(ps, rows_per_sample, rows, x.device), stream()),
               "op_layernorm_bwd_skip")
        return dx, dw, db
    _check(lib().op_layernorm_bwd(ptr(dy), ptr(x), ptr(w), ptr(b), ptr(mean), ptr(rstd), ptr(add), ptr(dx), ptr(dw), ptr(db),
                                  ptr(ws), rows, cols, int(gelu), int(accumulate), _dt(x), ptr(x_rows), stream()), "op_layernorm_bwd")
    return dx, dw, db


SPLITK_WS_BYTES = 768 << 20
GEMM_ALGO_BYTES = [0, 0]  # [bytes, launches]: operands read once + outputs written once (bench.py's roofline.traffic yardstick)


def splitk_scratch(M, N, K, epilogue, device):
    """The fp32 scratch gemm_nt hands to op_gemm_nt for an [M, K] x [N, K]^T launch (the planner may then split K), or None: bias-free
    plain launches with few tiles and a long K (weight gradients, dgrads), and the small latency-bound launches (a few M-tiles: the
    leftover rows of a tail-rows split, batch-1 feature extraction) whose bias / residual epilogue the fold kernel applies.  The library
    decides; handing the scratch over costs nothing.  (ops._dense_dgrad_sums_k_in_one_piece asks the same question through this.)"""
    if epilogue in (EPI_BIAS, EPI_RESID) and (K >= 2048 or M <= 1024):
        # at most 8 fp32 slabs of the output (the planner's limit); small launches (feature extraction under hipGraph
        # capture, where every capture stream gets its own scratch) then pin megabytes, not the training-size buffer
        return workspace(min(SPLITK_WS_BYTES, 32 * M * N), device, "gemm_splitk")
    return None


def gemm_nt(A, Bs, biases=None, out=None, epilogue=EPI_BIAS, n_seg=0, h0=None, h1=None, resid=None, gamma=None,
            rowscale=None, rows_per_sample=0, alpha=None, N=None, ldc=None, splitk=True, resid_rows=None):
    """C[M,N] = A[M,K] @ cat(Bs)[N,K]^T with the fused epilogue.  Bs: list of 1-3 [n_seg,K] weights (GeGLU: [W0, W1]).
    resid_rows (int32 [M], residual epilogue): resid and out are FULL matrices, row m of the launch reads / writes their row
    resid_rows[m] (< 0: dropped); h0 stays [M, N]."""
    M, K = A.shape
    if resid_rows is not None:
        assert epilogue == EPI_RESID and out is not None and resid is not None and out.shape == resid.shape and resid_rows.numel() == M
        assert resid_rows.dtype == torch.int32 and resid_rows.is_contiguous()
    Bs = list(Bs) + [None] * (3 - len(Bs))
    biases = list(biases or []) + [None] * (3 - len(biases or []))
    if epilogue == EPI_GEGLU:
        Nn = Bs[0].shape[0]
    else:
        Nn = N if N is not None else sum(b.shape[0] for b in Bs if b is not None)
        if n_seg == 0:
            n_seg = Bs[0].shape[0]
    if out is None:
        out = torch.empty(M, Nn, dtype=torch.float32 if epilogue == EPI_F32 else torch.bfloat16, device=A.device)
    ldc_ = ldc if ldc is not None else out.stride(0)
    ws = splitk_scratch(M, Nn, K, epilogue, A.device) if splitk else None
    ws_bytes = ws.numel() if ws is not None else 0
    outs = 1 + (2 if h1 is not None else (1 if h0 is not None else 0))
    GEMM_ALGO_BYTES[0] += 2 * (M * K + Nn * K * (2 if epilogue == EPI_GEGLU else 1) + (M * Nn if resid is not None else 0)) \
        + out.element_size() * M * Nn * outs
    GEMM_ALGO_BYTES[1] += 1
    _check(lib().op_gemm_nt(ptr(A), A.stride(0), ptr(Bs[0]), ptr(Bs[1]), ptr(Bs[2]), Bs[0].stride(0), n_seg,
                            ptr(biases[0]), ptr(biases[1]), ptr(biases[2]), ptr(out), ldc_, ptr(h0), ptr(h1),
                            ptr(resid), resid.stride(0) if resid is not None else 0, ptr(gamma), ptr(rowscale),
                            rows_per_sample, ptr(alpha), M, Nn, K, epilogue, ptr(ws), ws_bytes, TUNE.gemm(), ptr(resid_rows),
                            out.shape[0] if resid_rows is not None else 0, stream()), "op_gemm_nt")
    return out


def _ptr_array(items, n):
    arr = (c_void_p * n)()
    for i, t in enumerate(items or ()):
        arr[i] = None if t is None else t.data_ptr()
    return arr


def gemm_nt_grouped(As, Ws, biases=None, outs=None, epilogue=EPI_BIAS, h0s=None, h1s=None, resids=None, gammas=None,
                    rowscales=None, rows_per_sample=None, resid_rows=None):
    """(resid_rows: per problem an int32 row table, see gemm_nt -- outs / resids are then the full matrices, one row count for all.)
    One launch for up to three problems out_p = epilogue(A_p @ W_p^T) with a common N, K (the per-modality FFNs of a layer).
    As: [M_p, K] tensors with a common row stride; Ws: per problem one weight, or (wi_0, wi_1) for the GeGLU epilogue.
    Returns the list of outputs, or None when the shape does not qualify for the persistent kernel (caller falls back)."""
    n = len(As)
    K = As[0].shape[1]
    pairs = [w if isinstance(w, (tuple, list)) else (w, None) for w in Ws]
    N = pairs[0][0].shape[0]
    if outs is None:
        outs = [torch.empty(a.shape[0], N, dtype=torch.bfloat16, device=a.device) for a in As]
    lda, ldb, ldc = As[0].stride(0), pairs[0][0].stride(0), outs[0].stride(0)
    ldr = resids[0].stride(0) if resids and resids[0] is not None else 0
    if any(a.stride(0) != lda or a.shape[1] != K for a in As) or any(w[0].stride(0) != ldb or w[0].shape != (N, K) for w in pairs) \
            or any(o.stride(0) != ldc for o in outs) or (ldr and any(r.stride(0) != ldr for r in resids)):
        return None
    flatB, flatb = [], []
    for i, (w0, w1) in enumerate(pairs):
        flatB += [w0, w1]
        flatb += [biases[i] if biases else None, None]
    Ms = (c_int64 * n)(*[a.shape[0] for a in As])
    rps = (c_int64 * n)(*[(rows_per_sample[i] if rows_per_sample else 0) for i in range(n)])
    for i, a in enumerate(As):
        outs_n = 1 + (2 if h1s and h1s[i] is not None else (1 if h0s and h0s[i] is not None else 0))
        GEMM_ALGO_BYTES[0] += 2 * (a.shape[0] * K + N * K * (2 if epilogue == EPI_GEGLU else 1)
                                   + (a.shape[0] * N if resids and resids[i] is not None else 0)) + 2 * a.shape[0] * N * outs_n
    GEMM_ALGO_BYTES[1] += 1
    rc = lib().op_gemm_nt_grouped(n, _ptr_array(As, n), Ms, lda, _ptr_array(flatB, 2 * n), ldb, _ptr_array(flatb, 2 * n),
                                  _ptr_array(outs, n), ldc, _ptr_array(h0s, n), _ptr_array(h1s, n), _ptr_array(resids, n), ldr,
                                  _ptr_array(gammas, n), _ptr_array(rowscales, n), rps, N, K, epilogue, TUNE.gemm(),
                                  _ptr_array(resid_rows, n) if resid_rows is not None else None,
                                  outs[0].shape[0] if resid_rows is not None else 0, stream())
    if rc == -95:
        return None
    _check(rc, "op_gemm_nt_grouped")
    return outs


def quant_fp8_rows(x2d, out=None):
    """bf16 [rows, cols] -> (fp8 e4m3 bytes [rows, cols] as uint8, fp32 row scales [rows]) with x ~= q * scale[row].
    out: an earlier result to overwrite in place (derived weight copies keep their addresses across optimiser steps)."""
    rows, cols = x2d.shape
    if out is not None:
        q, scale = out
    else:
        q = torch.empty(rows, cols, dtype=torch.uint8, device=x2d.device)
        scale = torch.empty(rows, dtype=torch.float32, device=x2d.device)
    _check(lib().op_quant_fp8_rows(ptr(x2d), x2d.stride(0), ptr(q), q.stride(0), ptr(scale), rows, cols, stream()), "op_quant_fp8_rows")
    return q, scale


def gemm_nt_fp8(A8, sa, B8s, sbs, bias=None, out=None, epilogue=EPI_BIAS, h0=None, h1=None, resid=None, gamma=None, rowscale=None,
                rows_per_sample=0):
    """C[M,N] bf16 = epilogue((A8 @ B8^T) * sa[:, None] * sb[None, :]) on the fp8 MFMA path; A8 [M,K] / B8 [N,K] uint8 (e4m3),
    per-row fp32 scales.  B8s / sbs: [W] or, for the GeGLU epilogue, [W0, W1]."""
    M, K = A8.shape
    N = B8s[0].shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=A8.device)
    B1, sb1 = (B8s[1], sbs[1]) if len(B8s) > 1 else (None, None)
    _check(lib().op_gemm_nt_fp8(ptr(A8), A8.stride(0), ptr(sa), ptr(B8s[0]), ptr(B1), B8s[0].stride(0), ptr(sbs[0]), ptr(sb1),
                                ptr(bias), ptr(out), out.stride(0), ptr(h0), ptr(h1), ptr(resid),
                                resid.stride(0) if resid is not None else 0, ptr(gamma), ptr(rowscale), rows_per_sample, M, N, K,
                                epilogue, int(TUNE.fp8_small), stream()), "op_gemm_nt_fp8")
    return out


def gemm_plan(M, N, K, epilogue=EPI_BIAS, has_bias=True, workspace_bytes=SPLITK_WS_BYTES):
    """(tile, K-splits, epilogue-in-fold-kernel, tail rows) op_gemm_nt would use; a host-only query (works without a GPU)."""
    out = (ctypes.c_int * 4)()
    _check(lib().op_gemm_plan(M, N, K, epilogue, int(has_bias), workspace_bytes, TUNE.gemm(), ctypes.cast(out, P)), "op_gemm_plan")
    return out[0], out[1], bool(out[2]), out[3]


def gemm_tn_supported(K, M, N, lda, ldb, ldc=0):
    return (K % 64 == 0 and M % 8 == 0 and N % 8 == 0 and lda % 8 == 0 and ldb % 8 == 0 and ldc % 8 == 0 and M >= 8 and N >= 8
            and 31 * lda + M < (1 << 30) and 31 * ldb + N < (1 << 30))


def gemm_nt_batched(A, W, bias, out, rows, K):
    """out[z] = A_z W[z]^T (+ bias[z]) for z < G as ONE launch.  A: [G, *, lda] whose batch z starts at A[z] and whose ROWS are read with
    stride A.stride(1) as K-wide (possibly overlapping) patches; W [G, N, K] contiguous; bias [G, N] or None; out [G, rows, N]."""
    G, N = W.shape[0], W.shape[1]
    assert W.is_contiguous() and out.is_contiguous() and out.shape == (G, rows, N) and A.stride(2) == 1
    GEMM_ALGO_BYTES[0] += 2 * G * (rows * K + N * K + rows * N)
    GEMM_ALGO_BYTES[1] += 1
    _check(lib().op_gemm_nt_batched(ptr(A), A.stride(1), A.stride(0), ptr(W), K, N * K, ptr(bias), N if bias is not None else 0, ptr(out), N,
                                    rows * N, rows, N, K, G, stream()), "op_gemm_nt_batched")
    return out


def audio_conv1_ln_gelu_fwd(wav, stride, w0, b0, lnw, lnb, rows, eps, slack_rows=0):
    """GELU(LN(conv(wav))) of the feature extractor's first block straight from the flat waveform: y [rows + slack_rows, C] (the slack
    rows zero: the next block's strided patch view reads past the last row), mean, rstd [rows]."""
    C = w0.shape[0]
    assert w0.is_contiguous() and w0.numel() == C * 10 and wav.is_contiguous() and (rows == 0 or wav.numel() >= stride * (rows - 1) + 10)
    y = torch.empty(rows + slack_rows, C, dtype=torch.bfloat16, device=wav.device)
    if slack_rows:
        y[rows:].zero_()
    mean = torch.empty(rows, dtype=torch.float32, device=wav.device)
    rstd = torch.empty(rows, dtype=torch.float32, device=wav.device)
    # (rows = 0: nothing is written; w0 stands in for the empty tensors' null addresses)
    _check(lib().op_audio_conv1_ln_gelu_fwd(_ptr_rows(wav, w0), stride, ptr(w0), ptr(b0), ptr(lnw), ptr(lnb), _ptr_rows(y, w0), _ptr_rows(mean, w0),
                                            _ptr_rows(rstd, w0), rows, C, eps, stream()), "op_audio_conv1_ln_gelu_fwd")
    return y, mean, rstd


def audio_conv1_ln_gelu_bwd(dy, wav, stride, w0, b0, lnw, lnb, mean, rstd, accumulate=False, out=None):
    """Parameter gradients of audio_conv1_ln_gelu_fwd (bf16): dw0 [C, 10], db0 [C] | None, dlnw [C] | None, dlnb [C] | None.
    out = (dw0, db0, dlnw, dlnb): the caller's tensors (None where the parameter is None), overwritten or (accumulate) added to;
    without `out` they are allocated and accumulate is ignored.  An empty dy (no rows): zeros, or `out` untouched when accumulating."""
    rows, C = dy.shape
    if out is None:
        mk = lambda ref, shape: torch.empty(shape, dtype=torch.bfloat16, device=dy.device) if ref is not None else None  # noqa: E731
        out = torch.empty(C, 10, dtype=torch.bfloat16, device=dy.device), mk(b0, C), mk(lnw, C), mk(lnb, C)
        accumulate = False
    dw0, db0, dlw, dlb = out
    for t, ref, n in ((dw0, w0, C * 10), (db0, b0, C), (dlw, lnw, C), (dlb, lnb, C)):
        assert (t is None) == (ref is None) and (t is None or (t.dtype == torch.bfloat16 and t.is_contiguous() and t.numel() == n))
    ws = workspace(lib().op_audio_conv1_ln_gelu_bwd_workspace_bytes(C), dy.device, "audio_conv1")
    _check(lib().op_audio_conv1_ln_gelu_bwd(_ptr_rows(dy, ws), _ptr_rows(wav, ws), stride, ptr(w0), ptr(b0), ptr(lnw), ptr(lnb), _ptr_rows(mean, ws),
                                            _ptr_rows(rstd, ws), ptr(dw0), ptr(db0), ptr(dlw), ptr(dlb), ptr(ws), rows, C, int(accumulate), stream()),
           "op_audio_conv1_ln_gelu_bwd")
    return dw0, db0, dlw, dlb


def gemm_tn_grouped_plan(sizes, workgroups=256, tune=0):
    """[(M, N, K)] -> [(queue, problem, tile_m, tile_n)] in draw order: op_gemm_tn_grouped's schedule (host-only query)."""
    n = len(sizes)
    cap = sum(((m + 255) // 256) * ((nn + 255) // 256) for m, nn, _ in sizes)
    out = (ctypes.c_int32 * (4 * cap))()
    arr = lambda j: (c_int64 * n)(*[q[j] for q in sizes])  # noqa: E731
    cnt = lib().op_gemm_tn_grouped_plan(n, arr(0), arr(1), arr(2), int(workgroups), int(tune), ctypes.cast(out, P), cap)
    if cnt < 0:
        raise RuntimeError("op_gemm_tn_grouped_plan failed (%d)" % cnt)
    return [tuple(out[4 * i:4 * i + 4]) for i in range(cnt)]


def gemm_tn(A_km, B_kn, out=None, accumulate=False, splitk=True):
    """C[M,N] (+)= A_km^T @ B_kn with A_km [K, M], B_kn [K, N] (row-major, last dim contiguous): dW = dy^T x without copies.
    splitk=False: no scratch is handed over, every output tile runs its whole K (tests: the grouped launch's yardstick)."""
    K, M = A_km.shape
    N = B_kn.shape[1]
    if out is None:
        out = torch.empty(M, N, dtype=torch.bfloat16, device=A_km.device)
        accumulate = False
    ws = workspace(SPLITK_WS_BYTES, A_km.device, "gemm_splitk") if splitk else None
    GEMM_ALGO_BYTES[0] += 2 * (K * M + K * N + M * N * (2 if accumulate else 1))
    GEMM_ALGO_BYTES[1] += 1
    _check(lib().op_gemm_tn(ptr(A_km), A_km.stride(0), ptr(B_kn), B_kn.stride(0), ptr(out), out.stride(0), M, N, K,
                            int(accumulate), ptr(ws), ws.numel() if ws is not None else 0, TUNE.gemm(), stream()), "op_gemm_tn")
    return out


_tn_counters = {}
TN_GROUP_MAX = 16


def live_ktiles(segs, probs, device):
    """Live K-tile lists (op_live_ktiles) for weight-gradient problems over one row matrix whose rows of dropped samples are zero.
    segs: [(ps fp32 [B] | None, row0, S, B)]; probs: [(row0, rows)], rows % 64 == 0.  Returns per problem (list int32 [rows / 64], count
    int32 [1]): views of ONE buffer, filled by one launch, never read by the host."""
    ns, n = len(segs), len(probs)
    sizes = [rows // 64 for _, rows in probs]
    buf = torch.empty(sum(sizes) + n, dtype=torch.int32, device=device)
    lists, off = [], n
    for p, k in enumerate(sizes):
        lists.append((buf[off:off + k], buf[p:p + 1]))
        off += k
    i64 = lambda k, vals: (c_int64 * k)(*[int(v) for v in vals])  # noqa: E731
    for ps, _, _, B in segs:
        assert ps is None or (ps.dtype == torch.float32 and ps.is_contiguous() and ps.numel() >= B and ps.device == buf.device)
    _check(lib().op_live_ktiles(ns, _ptr_array([q[0] for q in segs], ns), i64(ns, [q[1] for q in segs]), i64(ns, [q[2] for q in segs]),
                                i64(ns, [q[3] for q in segs]), n, i64(n, [q[0] for q in probs]), i64(n, [q[1] for q in probs]),
                                _ptr_array([q[0] for q in lists], n), _ptr_array([q[1] for q in lists], n), stream()), "op_live_ktiles")
    return lists


def mwindow_rule(S):
    """How a segment of S-row samples is cut into 256-row windows for the input-gradient GEMMs: (wps, odd).  wps > 0: every kept sample
    gets wps windows from its first row on -- chosen when they carry at most 5 % surplus rows; odd: S % 256 == 1, the windows leave
    out each sample's last row, and those rows of ALL samples form strided windows (256 samples each).  wps == 0: the aligned 256-row
    tiles of the segment."""
    odd = S % 256 == 1 and S > 1
    Sp = S - 1 if odd else S
    wps = -(-Sp // 256)
    if wps * 256 * 100 <= 105 * Sp:
        return wps, odd
    return 0, False


def live_mwindows(segs, lists, outs):
    """Window lists (op_live_mwindows) for input-gradient GEMMs over one row matrix whose rows of dropped samples are zero, and +0 in
    the rows of `outs` the listed launches will not write.  segs: [(ps fp32 | None, row0, S, B[, ps stride = 1])], sample b has the multiplier ps[b * stride]; lists: per list the members
    [(segment index, problem index, row at which the problem's operand starts)], a segment in at most two lists; outs: bf16 matrices
    parallel to the row matrix.  Returns per list (windows int32 [2 * max] -- two words per entry --, count int32 [1]): views of ONE buffer, never read by the host."""
    return _live_mwindows(segs, lists, outs, None)


def _live_mwindows(segs, lists, outs, _srcs):
    """live_mwindows (_srcs None) and live_mwindows_fwd."""
    ns, nl, no = len(segs), len(lists), len(outs)
    dev = outs[0].device if outs else next(q[0] for q in segs if q[0] is not None).device
    segs = [tuple(q) + (1,) * (5 - len(q)) for q in segs]
    wps = [mwindow_rule(q[2])[0] for q in segs]
    odd = [int(mwindow_rule(q[2])[1]) for q in segs]
    units = [(q[3] if w else -(-q[2] * q[3] // 256)) * max(w, 1) + (-(-q[3] // 256) if o else 0) for w, o, q in zip(wps, odd, segs)]
    sizes = [sum(units[i] for i, _, _ in members) for members in lists]
    buf = torch.empty(2 * sum(sizes) + nl + (nl & 1), dtype=torch.int32, device=dev)
    res, off = [], nl + (nl & 1)  # (the two-word entries stay 8-byte aligned: the GEMM reads one with a single 64-bit load)
    for l, k in enumerate(sizes):
        res.append((buf[off:off + 2 * k], buf[l:l + 1]))
        off += 2 * k
    ref = [[-1, 0, 0, -1, 0, 0] for _ in segs]
    for l, members in enumerate(lists):
        for i, prob, base in members:
            k = 0 if ref[i][0] < 0 else 3
            assert ref[i][k] < 0, "a segment feeds at most two lists"
            ref[i][k:k + 3] = [l, prob, base]
    i64 = lambda vals: (c_int64 * len(vals))(*[int(v) for v in vals])  # noqa: E731
    for ps, _, _, B, st in segs:
        assert ps is None or (ps.dtype == torch.float32 and ps.is_contiguous() and ps.numel() > (B - 1) * st and ps.device == buf.device)
    for o in outs:
        assert o.dtype == torch.bfloat16 and o.dim() == 2 and o.stride(1) == 1 and o.device == buf.device
    args = (ns, _ptr_array([q[0] for q in segs], ns), i64([q[4] for q in segs]), i64([q[1] for q in segs]),
            i64([q[2] for q in segs]), i64([q[3] for q in segs]), i64(wps), i64(odd), i64([v for r in ref for v in (r[0], r[3])]),
            i64([v for r in ref for v in (r[1], r[4])]), i64([v for r in ref for v in (r[2], r[5])]), nl,
            _ptr_array([q[0] for q in res], nl), _ptr_array([q[1] for q in res], nl), i64(sizes), no,
            _ptr_array(outs, max(no, 1)), i64([o.stride(0) for o in outs] or [0]), i64([o.shape[1] for o in outs] or [0]),
            i64([o.shape[0] for o in outs] or [0]))
    if _srcs is None:
        _check(lib().op_live_mwindows(*args, stream()), "op_live_mwindows")
    else:  # (live_mwindows_fwd)
        for o, q in zip(outs, _srcs):
            assert q is None or (q.dtype == torch.bfloat16 and q.shape == o.shape and q.stride(1) == 1 and q.device == o.device)
        _check(lib().op_live_mwindows_fwd(*args, _ptr_array(_srcs, no), i64([0 if q is None else q.stride(0) for q in _srcs]), stream()),
               "op_live_mwindows_fwd")
    return res


def live_mwindows_fwd(segs, lists, outs, srcs):
    """live_mwindows for the FORWARD launches of a residual branch (gemm_nt_windows_fwd): the same lists; the rows of outs[o] that no window
    covers get a copy of the same rows of srcs[o] (the residual output takes the residual input) or, with srcs[o] None, +0.
    An entry of outs may be None: a matrix of the branch that gets NO fill, because every reader of its rows leaves out the rows of
    dropped samples (h0 | h1 under ops.SKIP_ZERO_ROWS); the launch does not hear of it."""
    assert len(srcs) == len(outs)
    pairs = [(o, q) for o, q in zip(outs, srcs) if o is not None]
    assert len(pairs) >= 1
    return _live_mwindows(segs, lists, [o for o, _ in pairs], [q for _, q in pairs])


def gemm_nt_windows_fwd(As, Wss, biases, outs, windows, n_seg, epilogue=EPI_BIAS, resids=None, gammas=None, rowscales=None,
                        rows_per_sample=None, max_row_stride=1, tune=None):
    """The rows of out_p = epilogue(A_p @ cat(Wss[p])^T + cat(biases[p])) that the entries of `windows` name, nothing else: the forward
    form of gemm_nt_windows.  Wss[p] / biases[p]: the 1-3 weights [n_seg, K] (bias vectors or None) of the column segments of problem
    p (q | k | v: n_seg = H; wi_0 | wi_1: n_seg = F).  EPI_RESID: out = resid + rowscale[m // rows_per_sample] * gamma * (...) with m
    the row inside its problem.  Returns False (nothing launched) when the shape does not qualify."""
    n = len(As)
    nw = len(Wss[0])
    K, N = As[0].shape[1], n_seg * nw
    lda, ldb, ldc = As[0].stride(0), Wss[0][0].stride(0), outs[0].stride(0)
    ldr = resids[0].stride(0) if resids else 0
    assert all(a.stride(0) == lda and a.shape[1] == K and a.stride(1) == 1 for a in As) and all(o.stride(0) == ldc and o.shape[1] == N for o in outs)
    assert all(len(ws) == nw and all(w.stride(0) == ldb and w.shape == (n_seg, K) for w in ws) for ws in Wss)
    assert all(o.shape[0] == a.shape[0] for a, o in zip(As, outs)) and (not resids or all(r.stride(0) == ldr and r.shape == o.shape for r, o in zip(resids, outs)))
    lst, cnt = windows
    assert lst.dtype == torch.int32 and cnt.dtype == torch.int32 and lst.is_contiguous() and lst.numel() >= 2 and lst.data_ptr() % 8 == 0
    if max_row_stride * max(lda, ldc, ldr) >= 1 << 23 or n_seg % 256 != 0:
        return False
    flatW = [w for ws in Wss for w in list(ws) + [None] * (3 - nw)]
    flatb = [b for bs in (biases or [[None] * nw] * n) for b in list(bs) + [None] * (3 - nw)]
    rps = (c_int64 * n)(*[(rows_per_sample[i] if rows_per_sample else 0) for i in range(n)])
    rc = lib().op_gemm_nt_grouped_windows_fwd(n, _ptr_array(As, n), (c_int64 * n)(*[a.shape[0] for a in As]), lda, _ptr_array(flatW, 3 * n), ldb,
                                              n_seg, _ptr_array(flatb, 3 * n), _ptr_array(outs, n), ldc, _ptr_array(resids, n), ldr,
                                              _ptr_array(gammas, n), _ptr_array(rowscales, n), rps, N, K, epilogue, ptr(lst), ptr(cnt),
                                              lst.numel() // 2, max_row_stride, TUNE.gemm() if tune is None else int(tune), stream())
    if rc == -95:
        return False
    _check(rc, "op_gemm_nt_grouped_windows_fwd")
    for a in As:  # (the dense launch's bytes, as in gemm_nt_windows)
        GEMM_ALGO_BYTES[0] += 2 * (a.shape[0] * K + N * K + (a.shape[0] * N if resids else 0)) + 2 * a.shape[0] * N
    GEMM_ALGO_BYTES[1] += 1
    return True


def gemm_nt_windows(As, Ws, outs, windows, max_row_stride=1, tune=None):
    """The rows of out_p = A_p @ W_p^T that the entries of `windows` (live_mwindows' (list, count)) name, nothing else: one launch of the
    persistent kernel for up to three problems with a common N, K and row strides.  max_row_stride: the largest sample length with
    strided windows in the list (mwindow_rule's odd).  Returns False (nothing launched) when the shape does not qualify."""
    n = len(As)
    K, N = As[0].shape[1], Ws[0].shape[0]
    lda, ldb, ldc = As[0].stride(0), Ws[0].stride(0), outs[0].stride(0)
    assert all(a.stride(0) == lda and a.shape[1] == K and a.stride(1) == 1 for a in As) and all(o.stride(0) == ldc and o.shape[1] == N for o in outs)
    assert all(w.stride(0) == ldb and w.shape == (N, K) for w in Ws) and all(o.shape[0] == a.shape[0] for a, o in zip(As, outs))
    lst, cnt = windows
    assert lst.dtype == torch.int32 and cnt.dtype == torch.int32 and lst.is_contiguous() and lst.numel() >= 2 and lst.data_ptr() % 8 == 0
    if max_row_stride * max(lda, ldc) >= 1 << 23:
        return False
    rc = lib().op_gemm_nt_grouped_windows(n, _ptr_array(As, n), (c_int64 * n)(*[a.shape[0] for a in As]), lda, _ptr_array(Ws, n), ldb,
                                          _ptr_array(outs, n), ldc, N, K, ptr(lst), ptr(cnt), lst.numel() // 2, max_row_stride,
                                          TUNE.gemm() if tune is None else int(tune), stream())
    if rc == -95:
        return False
    _check(rc, "op_gemm_nt_grouped_windows")
    for a in As:  # (the dense launch's bytes and, in the profiling slot, its 2 M N K: both overstate a listed launch by the skipped share)
        GEMM_ALGO_BYTES[0] += 2 * (a.shape[0] * K + N * K) + 2 * a.shape[0] * N
    GEMM_ALGO_BYTES[1] += 1
    return True


def gemm_tn_grouped(problems, tune=0, ktiles=None):
    """ONE persistent launch for up to 16 weight-gradient GEMMs, no split-K (csrc/gemm.hip: gemm256w_tn_grouped_kernel).
    problems: [(A_km [K, M], B_kn [K, N], out [M, N] bf16, accumulate[, (W [M, N] bf16, rowdot fp32 [N / 128, M][, rscale bf16 [M]])])].
    Returns False (nothing launched) when a problem does not qualify for the transpose-read kernel -- the caller then runs gemm_tn per
    problem.  (W, rowdot): rowdot[s][m] = sum over the 128 columns n of slot s of W[m][n] * (this launch's fp32 product)[m][n] (written,
    every entry once); rscale: out[m] += rscale[m] * product[m] while rowdot sums the unscaled product -- see gamma_grad_finish.
    ktiles: per problem None or live_ktiles' (list, count): only those 64-row K-tiles run (the rows of A in the others are zero)."""
    n = len(problems)
    dev = problems[0][0].device
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    ctr = _tn_counters.get(key)
    if ctr is None:  # zeroed once; every launch re-arms it
        ctr = _tn_counters[key] = torch.zeros(int(lib().op_gemm_tn_grouped_counter_bytes()), dtype=torch.uint8, device=dev)
    arr = lambda vals: (c_int64 * n)(*vals)  # noqa: E731
    As, Bs, Cs = [q[0] for q in problems], [q[1] for q in problems], [q[2] for q in problems]
    acc = (ctypes.c_int32 * n)(*[int(bool(q[3])) for q in problems])
    side = [tuple(q[4]) + (None,) * (3 - len(q[4])) if len(q) > 4 and q[4] is not None else (None, None, None) for q in problems]
    Ws, Rs, Ss = [x[0] for x in side], [x[1] for x in side], [x[2] for x in side]
    has_side = any(r is not None for r in Rs)
    for sc, r, a, b in zip(Ss, Rs, As, Bs):
        assert sc is None or (sc.dtype == torch.bfloat16 and sc.is_contiguous() and sc.numel() == a.shape[1])
        assert r is None or (r.dtype == torch.float32 and r.is_contiguous() and r.shape == (b.shape[1] // 128, a.shape[1])), "rowdot: fp32 [N / 128, M]"
    head = (n, _ptr_array(As, n), arr([a.stride(0) for a in As]), _ptr_array(Bs, n), arr([b.stride(0) for b in Bs]),
            _ptr_array(Cs, n), arr([c.stride(0) for c in Cs]), arr([a.shape[1] for a in As]),
            arr([b.shape[1] for b in Bs]), arr([a.shape[0] for a in As]), acc,
            _ptr_array(Ws, n) if has_side else None, arr([w.stride(0) if w is not None else 0 for w in Ws]) if has_side else None,
            _ptr_array(Rs, n) if has_side else None, _ptr_array(Ss, n) if any(x is not None for x in Ss) else None)
    if ktiles is not None and any(k is not None for k in ktiles):
        for k, a in zip(ktiles, As):
            assert k is None or (k[0].dtype == torch.int32 and k[1].dtype == torch.int32 and k[0].numel() >= a.shape[0] // 64)
        rc = lib().op_gemm_tn_grouped_lists(*head, _ptr_array([k[0] if k is not None else None for k in ktiles], n),
                                            _ptr_array([k[1] if k is not None else None for k in ktiles], n), ptr(ctr), int(tune), stream())
    else:
        rc = lib().op_gemm_tn_grouped(*head, ptr(ctr), int(tune), stream())
    if rc == -95:
        return False
    _check(rc, "op_gemm_tn_grouped")
    for a, b, c, ac in [q[:4] for q in problems]:
        K, M = a.shape
        GEMM_ALGO_BYTES[0] += 2 * (K * M + K * b.shape[1] + M * b.shape[1] * (2 if ac else 1))
    GEMM_ALGO_BYTES[1] += 1
    return True


def transpose(x2d, out=None, scale=None):
    """out[c][r] = x2d[r][c] (* scale[r]: bf16 [rows], the product rounded to bf16)."""
    rows, cols = x2d.shape
    if out is None:
        out = torch.empty(cols, rows, dtype=x2d.dtype, device=x2d.device)
    assert scale is None or (scale.dtype == torch.bfloat16 and scale.is_contiguous() and scale.numel() == rows)
    _check(lib().op_transpose_scaled(ptr(x2d), ptr(out), rows, cols, x2d.stride(0), out.stride(0), ptr(scale), stream()), "op_transpose")
    return out


def transpose_table(jobs, device):
    """jobs: [(src [rows, cols] (last dim contiguous), dst view [cols, rows] (last dim contiguous)[, scale bf16 [rows] or None])] ->
    (device table, total tiles) for transpose_batched; the table stays valid as long as the tensors keep their storage."""
    import struct
    assert lib().op_transpose_desc_bytes() == 56
    raw, tile0 = b"", 0
    for job in jobs:
        src, dst = job[:2]
        scale = job[2] if len(job) > 2 else None
        rows, cols = src.shape
        tx, ty = (cols + 63) // 64, (rows + 63) // 64
        raw += struct.pack("<QQiiqqiiQ", src.data_ptr(), dst.data_ptr(), rows, cols, src.stride(0), dst.stride(0), tile0, tx,
                           scale.data_ptr() if scale is not None else 0)
        tile0 += tx * ty
    table = torch.frombuffer(bytearray(raw), dtype=torch.uint8).to(device)
    return table, tile0


def transpose_batched(table, n, total_tiles):
    _check(lib().op_transpose_batched(ptr(table), n, total_tiles, stream()), "op_transpose_batched")


def _ptr_rows(t, stand_in):
    """ptr(t) for an operand of M rows.  An EMPTY tensor (M = 0) has a null address, which the entry points refuse before they look at M:
    the address of `stand_in` (the launch's workspace) goes in its place -- no row of it is read or written."""
    return ptr(stand_in) if t is not None and t.numel() == 0 else ptr(t)


def colsum(x, y=None, rowscale=None, rows_per_sample=0, mul=None, out=None, accumulate=False, out_dtype=torch.bfloat16):
    """M = 0: the sum over no rows -- zeros, or `out` untouched when accumulating."""
    M, N = x.shape
    if out is None:
        out = torch.empty(N, dtype=out_dtype, device=x.device)
        accumulate = False
    ws = workspace(lib().op_colsum_workspace_bytes(N), x.device, "colsum")
    _check(lib().op_colsum(_ptr_rows(x, ws), _ptr_rows(y, ws), _ptr_rows(rowscale, ws), rows_per_sample, ptr(mul), ptr(out), ptr(ws), M, N,
                           int(accumulate), _dt(out), stream()), "op_colsum")
    return out


def colsum_segments(x, seg_cols, outs=None, accumulate=False):
    """Per-segment column sums of x [M, n_seg*seg_cols]; outs: list of bf16 [seg_cols] targets / None (skip) per segment."""
    M, N = x.shape
    n_seg = N // seg_cols
    if outs is None:
        outs = [torch.empty(seg_cols, dtype=x.dtype, device=x.device) for _ in range(n_seg)]
        accumulate = False
    o = list(outs) + [None] * (3 - len(outs))
    ws = workspace(lib().op_colsum_workspace_bytes(N), x.device, "colsum")
    _check(lib().op_colsum_segments(_ptr_rows(x, ws), ptr(o[0]), ptr(o[1]), ptr(o[2]), ptr(ws), M, n_seg, seg_cols, int(accumulate),
                                    stream()), "op_colsum_segments")
    return outs


def resid_bwd(dout, y=None, gamma=None, rowscale=None, rows_per_sample=0, dgamma=None, dbias=None, accumulate=False, g0=None,
              dout_rows=None, skip_zero_rows=False):
    """dbranch = rowscale*gamma*dout plus the column reductions dgamma / dbias in one pass.  dgamma / dbias: True
    (allocate), a bf16 [N] tensor (write or, with accumulate, add into it) or None (skip).  g0: fp32 [N] that receives
    sum_m rowscale*dout (dbias without the gamma factor: gamma_grad_finish's operand) -- and dbranch is then rowscale*dout WITHOUT
    gamma (the weight-gradient launch's rscale and the gamma-scaled transposed weight carry it).
    skip_zero_rows: the rows whose multiplier is 0 are not read; dbranch gets +0 there (op_resid_bwd_skip)."""
    M, N = dout.shape
    if dout_rows is not None:  # dout: a larger matrix, row m of the pass = its row dout_rows[m] (< 0: zeros); the result has M rows
        assert dout_rows.dtype == torch.int32 and dout_rows.is_contiguous() and dout.is_contiguous()
        M = dout_rows.numel()
    out = torch.empty(M, N, dtype=dout.dtype, device=dout.device)
    if dgamma is True:
        dgamma = torch.empty(N, dtype=dout.dtype, device=dout.device)
    if dbias is True:
        dbias = torch.empty(N, dtype=dout.dtype, device=dout.device)
    ws = None
    if dgamma is not None or dbias is not None or g0 is not None or M == 0:
        ws = workspace(lib().op_resid_bwd_workspace_bytes(N), dout.device, "resid")
    assert g0 is None or (g0.dtype == torch.float32 and g0.is_contiguous() and g0.numel() == N)
    # (M = 0: g0 and the non-accumulating dgamma / dbias come back as zeros, the sums over no rows)
    entry = "op_resid_bwd_skip" if skip_zero_rows and rowscale is not None else "op_resid_bwd"
    _check(getattr(lib(), entry)(_ptr_rows(dout, ws), _ptr_rows(y if dgamma is not None else None, ws), ptr(gamma), _ptr_rows(rowscale, ws),
              rows_per_sample, _ptr_rows(out, ws), ptr(dgamma), ptr(dbias), ptr(g0), ptr(ws), M, N, int(accumulate),
              _ptr_rows(dout_rows, ws), stream()), entry)
    return out, dgamma, dbias


def gamma_grad_finish(rowdot, pairs, dgamma, accumulate):
    """dgamma (+)= sum_s rowdot[s] + sum_i b_i * g0_i.  rowdot: fp32 [slots, N], the partial row dots of gemm_tn_grouped over the
    un-gamma-scaled gradient (several weight sets that share gamma: their slots one after the other); pairs: up to three (bias bf16 [N]
    or None, g0 fp32 [N])."""
    assert rowdot.dtype == torch.float32 and rowdot.dim() == 2 and rowdot.is_contiguous() and len(pairs) <= 3 and dgamma.dtype == torch.bfloat16
    assert rowdot.shape[1] == dgamma.numel()
    flat = []
    for b, g0 in list(pairs) + [(None, None)] * (3 - len(pairs)):
        flat += [ptr(b), ptr(g0)]
    _check(lib().op_gamma_grad_finish(ptr(rowdot), rowdot.shape[0], *flat, ptr(dgamma), rowdot.shape[1], int(accumulate), stream()),
           "op_gamma_grad_finish")
    return dgamma


def _skip_args(ps, rows_per_sample, rows, device):
    """(ps, rows per sample) of the *_skip entries: fp32, contiguous, one multiplier for every sample the rows reach."""
    rps = int(rows_per_sample)
    assert rps >= 1 and ps.dtype == torch.float32 and ps.is_contiguous() and ps.device == device and ps.numel() * rps >= rows
    return ptr(ps), rps


def ln_geglu_bwd(dy, h0, h1, w, mean, rstd, dw=None, db=None, accumulate=False, need_wgrad=True, dh0=None, dh1=None, ps=None,
                 rows_per_sample=1):
    """Backward of LayerNorm_F(gelu(h0)*h1): returns dh0, dh1, dw, db (dw/db allocated unless given; None with need_wgrad=False).
    dh0 / dh1 may be given as column blocks of one wider matrix (same row stride, last dim contiguous).
    ps (fp32, one stochastic-depth multiplier per rows_per_sample rows): the rows of samples with ps == 0 are not read -- dh0 | dh1 get
    +0 there, dw / db nothing (op_ln_geglu_bwd_skip)."""
    rows, cols = h0.shape
    if dh0 is None:
        dh0, dh1 = torch.empty_like(h0), torch.empty_like(h1)
    assert dh0.stride(0) == dh1.stride(0) and dh0.stride(1) == 1 and dh1.stride(1) == 1
    assert h0.stride(0) == h1.stride(0) and h0.stride(1) == 1 and h1.stride(1) == 1
    ws = None
    if need_wgrad:
        if dw is None:
            dw, db, accumulate = torch.empty_like(w), torch.empty_like(w), False
        ws = workspace(lib().op_layernorm_bwd_workspace_bytes(rows, cols), h0.device, "ln")
    else:
        dw = db = None
    if ps is not None:
        _check(lib().op_ln_geglu_bwd_skip(ptr(dy), ptr(h0), ptr(h1), ptr(w), ptr(mean), ptr(rstd), ptr(dh0), ptr(dh1), dh0.stride(0),
                                          h0.stride(0), ptr(dw), ptr(db), ptr(ws), rows, cols, int(accumulate),
                                          *_skip_args(ps, rows_per_sample, rows, h0.device), stream()), "op_ln_geglu_bwd_skip")
        return dh0, dh1, dw, db
    _check(lib().op_ln_geglu_bwd(ptr(dy), ptr(h0), ptr(h1), ptr(w), ptr(mean), ptr(rstd), ptr(dh0), ptr(dh1), dh0.stride(0),
                                 h0.stride(0), ptr(dw), ptr(db), ptr(ws), rows, cols, int(accumulate), stream()), "op_ln_geglu_bwd")
    return dh0, dh1, dw, db


def ln_geglu_fwd(h0, h1, w, b, eps=1e-5, want_stats=True, out=None, mean=None, rstd=None, q8=None, ps=None, rows_per_sample=1):
    """LayerNorm_F(bf16(gelu(h0) * h1)); h0 / h1 may be column blocks of one wider matrix.  Returns y, mean, rstd.
    q8 = (fp8 bytes [rows, cols], scales [rows]): also filled with the row-quantised output (see layernorm_fwd).
    ps (not with q8; see ln_geglu_bwd): the rows of samples with ps == 0 are not read -- y gets +0 there, mean / rstd are not written."""
    rows, cols = h0.shape
    assert h0.stride(0) == h1.stride(0) and h0.stride(1) == 1 and h1.stride(1) == 1
    y = out if out is not None else torch.empty(rows, cols, dtype=h0.dtype, device=h0.device)
    if want_stats and mean is None:
        mean = torch.empty(rows, dtype=torch.float32, device=h0.device)
        rstd = torch.empty(rows, dtype=torch.float32, device=h0.device)
    if q8 is not None:
        assert ps is None, "the fp8 route runs every row"
        assert q8[0].is_contiguous() and q8[0].shape == (rows, cols) and y.is_contiguous()
        _check(lib().op_ln_geglu_fwd_q8(ptr(h0), ptr(h1), h0.stride(0), ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), ptr(q8[0]), ptr(q8[1]),
                                        rows, cols, eps, stream()), "op_ln_geglu_fwd_q8")
        return y, mean, rstd
    if ps is not None:
        _check(lib().op_ln_geglu_fwd_skip(ptr(h0), ptr(h1), h0.stride(0), ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), rows, cols, eps,
                                          *_skip_args(ps, rows_per_sample, rows, h0.device), stream()), "op_ln_geglu_fwd_skip")
        return y, mean, rstd
    _check(lib().op_ln_geglu_fwd(ptr(h0), ptr(h1), h0.stride(0), ptr(w), ptr(b), ptr(y), ptr(mean), ptr(rstd), rows, cols, eps, stream()),
           "op_ln_geglu_fwd")
    return y, mean, rstd


def geglu_bwd(dg, h0, h1):
    dh0, dh1 = torch.empty_like(h0), torch.empty_like(h1)
    _check(lib().op_geglu_bwd(ptr(dg), ptr(h0), ptr(h1), ptr(dh0), ptr(dh1), dg.numel(), stream()), "op_geglu_bwd")
    return dh0, dh1


def scale_rows(dout, gamma=None, rowscale=None, rows_per_sample=0):
    M, N = dout.shape
    out = torch.empty_like(dout)
    _check(lib().op_scale_rows(ptr(dout), ptr(gamma), ptr(rowscale), rows_per_sample, ptr(out), M, N, stream()),
           "op_scale_rows")
    return out


def l2norm_fwd(x, out_dtype=torch.bfloat16, eps=1e-12):
    """(y, inv): inv[row] = 1 / max(||x||, eps), negative where the eps clamp was taken (l2norm_bwd then gives dy / eps)."""
    rows, cols = x.shape
    y = torch.empty(rows, cols, dtype=out_dtype, device=x.device)
    inv = torch.empty(rows, dtype=torch.float32, device=x.device)
    _check(lib().op_l2norm_fwd(ptr(x), ptr(y), ptr(inv), rows, cols, eps, _dt(y), stream()), "op_l2norm_fwd")
    return y, inv


def l2norm_bwd(dy, y, inv):
    rows, cols = y.shape
    dx = torch.empty(rows, cols, dtype=torch.bfloat16, device=y.device)
    _check(lib().op_l2norm_bwd(ptr(dy), ptr(y), ptr(inv), ptr(dx), rows, cols, _dt(y), stream()), "op_l2norm_bwd")
    return dx


def infonce_rows(sim, target0, label_smoothing=0.0, gscale=1.0, write_grad=True):
    rows, n = sim.shape
    dev = sim.device
    loss = torch.empty(rows, dtype=torch.float32, device=dev)
    hit = torch.empty(rows, dtype=torch.float32, device=dev)
    dot = torch.empty(rows, dtype=torch.float32, device=dev)
    _check(lib().op_infonce_rows(ptr(sim), rows, n, sim.stride(0), target0, label_smoothing, gscale, ptr(loss), ptr(hit),
                                 ptr(dot), int(write_grad), stream()), "op_infonce_rows")
    return loss, hit, dot


def adamw_step(p, g, m, v, lr, beta1, beta2, eps, weight_decay, step, grad_scale=1.0, grad_sqnorm=None, clip_norm=0.0):
    _check(lib().op_adamw_step(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), lr, beta1, beta2, eps, weight_decay, step,
                               grad_scale, ptr(grad_sqnorm), clip_norm, stream()), "op_adamw_step")


def adamw_step_groups(p, g, m, v, group_end8, group_lr_scale, group_wd, lr, beta1, beta2, eps, step, grad_scale=1.0,
                      grad_sqnorm=None, clip_norm=0.0):
    """One launch over the whole flat buffer; group tables are device tensors (int64 ends in 8-element vectors, fp32 scales)."""
    _check(lib().op_adamw_step_groups(ptr(p), ptr(g), ptr(m), ptr(v), p.numel(), ptr(group_end8), ptr(group_lr_scale),
                                      ptr(group_wd), group_end8.numel(), lr, beta1, beta2, eps, step, grad_scale, ptr(grad_sqnorm),
                                      clip_norm, stream()), "op_adamw_step_groups")


def adamw_step_groups_master(p, master, g, m, v, group_end8, group_lr_scale, group_wd, lr, beta1, beta2, eps, step, grad_scale=1.0,
                             grad_sqnorm=None, clip_norm=0.0):
    """adamw_step_groups with an fp32 master copy: `master` (fp32, as long as p) is read and updated, the bf16 `p` is only written,
    as the round-to-nearest-even cast of the new master."""
    _check(lib().op_adamw_step_groups_master(ptr(p), ptr(master), ptr(g), ptr(m), ptr(v), p.numel(), ptr(group_end8),
                                             ptr(group_lr_scale), ptr(group_wd), group_end8.numel(), lr, beta1, beta2, eps, step,
                                             grad_scale, ptr(grad_sqnorm), clip_norm, stream()), "op_adamw_step_groups_master")


def _req_ema(t, p, name="ema"):
    """The kernels run over p.numel() elements of `t`: a shorter, strided or non-fp32 buffer would be read and written out of bounds."""
    if t is None:
        return  # the C entry refuses a null average
    _req(t, name, torch.float32)
    _req(p, "p", torch.bfloat16)
    if t.numel() != p.numel():
        raise RuntimeError("%s has %d elements, p has %d" % (name, t.numel(), p.numel()))


def ema_step(ema, p, keep, take):
    """ema (fp32) <- fmaf(take, float(p), keep * ema) over the flat bf16 `p`: one step of the fp32 weight average (ema.FlatEMA)."""
    _req_ema(ema, p)
    _check(lib().op_ema_step(ptr(ema), ptr(p), p.numel(), keep, take, stream()), "op_ema_step")


def adamw_step_groups_ema(p, master, g, m, v, ema, group_end8, group_lr_scale, group_wd, lr, beta1, beta2, eps, step, ema_keep,
                          ema_take, grad_scale=1.0, grad_sqnorm=None, clip_norm=0.0):
    """adamw_step_groups (master None) or adamw_step_groups_master, and ema_step on the parameters it stores, in one launch."""
    _req_ema(ema, p)
    if master is not None:
        _req_ema(master, p, "master")
    _check(lib().op_adamw_step_groups_ema(ptr(p), ptr(master), ptr(g), ptr(m), ptr(v), ptr(ema), p.numel(), ptr(group_end8),
                                          ptr(group_lr_scale), ptr(group_wd), group_end8.numel(), lr, beta1, beta2, eps, step,
                                          grad_scale, ptr(grad_sqnorm), clip_norm, ema_keep, ema_take, stream()),
           "op_adamw_step_groups_ema")


def adamw_step_shard(p, g, first8, count8, m, v, master, ema, group_end8, group_lr_scale, group_wd, lr, beta1, beta2, eps, step,
                     ema_keep=0.0, ema_take=0.0, grad_scale=1.0, grad_sqnorm=None, clip_norm=0.0):
    """The grouped step over the vectors [first8, first8 + count8) of the FULL flat buffers p and g (optim.ShardedFusedAdamW): m, v and
    the optional master and ema are fp32 buffers of that range alone (8 * count8 elements); the group tables are the global ones.
    count8 == 0 is the C entry's OP_OK without a launch; its empty buffers (torch gives them a null address) are not handed over."""
    _req(p, "p", torch.bfloat16)
    _req(g, "g", torch.bfloat16)
    if g.numel() != p.numel():
        raise RuntimeError("g has %d elements, p has %d" % (g.numel(), p.numel()))
    for t, name in ((m, "m"), (v, "v"), (master, "master"), (ema, "ema")):
        if t is not None:  # the kernel runs over 8 * count8 elements of each: a shorter buffer would be read and written out of bounds
            _req(t, name, torch.float32)
            if t.numel() != 8 * count8:
                raise RuntimeError("%s has %d elements, the range has %d" % (name, t.numel(), 8 * count8))
    if count8 == 0 and 0 <= first8 <= p.numel() // 8:
        return
    _check(lib().op_adamw_step_shard(ptr(p), ptr(g), p.numel(), first8, count8, ptr(m), ptr(v), ptr(master), ptr(ema), ptr(group_end8),
                                     ptr(group_lr_scale), ptr(group_wd), group_end8.numel(), lr, beta1, beta2, eps, step, grad_scale,
                                     ptr(grad_sqnorm), clip_norm, ema_keep, ema_take, stream()), "op_adamw_step_shard")


def sqnorm(x, out=None):
    """Sum of squares of a flat bf16 tensor -> fp32 device scalar [1]."""
    if out is None:
        out = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = workspace(4096, x.device, "sqnorm")
    _check(lib().op_sqnorm(ptr(x), x.numel(), ptr(ws), ptr(out), stream()), "op_sqnorm")
    return out


def relpos_bias_build(table, bucket_i32, S, Spad, transposed=False):
    """[heads][S][Spad] bf16 image of table[bucket]; transposed=True gives out[h][key][query]."""
    heads = table.shape[1]
    out = torch.empty(heads, S, Spad, dtype=torch.bfloat16, device=table.device)
    _check(lib().op_relpos_bias_build(ptr(table), ptr(bucket_i32), bucket_i32.stride(0), ptr(out), heads, S, Spad,
                                      int(transposed), stream()), "op_relpos_bias_build")
    return out


PAIR_SEG = 32  # positions per segment of op_relpos_bias_bwd's pair lists


def relpos_pairs(bucket_i32, S, num_rel):
    """(pos, seg, bucket_seg, nseg) of op_relpos_bias_bwd for bucket[:S, :S]: the positions i*S + j grouped by bucket (a stable sort:
    row-major within a bucket), cut into segments of at most PAIR_SEG.  Device work only, no host synchronisation (a joint stream
    builds its bucket matrix every forward, possibly inside a hipGraph capture): nseg is the host-side bound S*S / PAIR_SEG + num_rel
    on the segment count, the segments past the real ones are empty.  Cached on the bucket tensor (the adapters keep theirs)."""
    key = (S, num_rel, bucket_i32._version)
    cached = getattr(bucket_i32, "_op_pairs", None)
    if cached is not None and cached[0] == key:
        return cached[1]
    dev = bucket_i32.device
    vals, order = torch.sort(bucket_i32[:S, :S].reshape(-1).long(), stable=True)
    pair_off = torch.searchsorted(vals, torch.arange(num_rel + 1, device=dev))   # bucket r = sorted positions pair_off[r] .. [r+1]
    bucket_seg = torch.zeros(num_rel + 1, dtype=torch.int64, device=dev)
    bucket_seg[1:] = ((pair_off[1:] - pair_off[:-1] + PAIR_SEG - 1) // PAIR_SEG).cumsum(0)
    nseg = S * S // PAIR_SEG + num_rel
    t = torch.arange(nseg, device=dev)
    r = torch.searchsorted(bucket_seg[1:], t, right=True)                          # bucket of segment t; num_rel past the last one
    rc = r.clamp(max=num_rel - 1)
    seg = torch.full((nseg + 1,), S * S, dtype=torch.int64, device=dev)
    seg[:nseg] = torch.where(r < num_rel, pair_off[rc] + (t - bucket_seg[rc]) * PAIR_SEG, S * S)
    res = (order.to(torch.int32), seg.to(torch.int32), bucket_seg.to(torch.int32), nseg)
    bucket_i32._op_pairs = (key, res)
    return res


def relpos_bias_bwd(dbias_f32, bucket_i32, num_rel, S, Spad):
    """Table gradient [num_rel, heads] of the bias image dbias [heads, S, Spad] (fp32), summed in a fixed order."""
    heads = dbias_f32.shape[0]
    pos, seg, bucket_seg, nseg = relpos_pairs(bucket_i32, S, num_rel)
    dtable = torch.empty(num_rel, heads, dtype=torch.float32, device=dbias_f32.device)
    partial = torch.empty(nseg, heads, dtype=torch.float32, device=dbias_f32.device)
    _check(lib().op_relpos_bias_bwd(ptr(dbias_f32), S, Spad, ptr(pos), ptr(seg), nseg, ptr(bucket_seg), num_rel, ptr(partial), ptr(dtable),
                                    heads, stream()), "op_relpos_bias_bwd")
    return dtable


def relpos_bias_build_ids(table, bucket_i32, ids_i32, Kpad, transposed=False):
    """Per-sample images [B, heads, K, Kpad] of table[bucket[ids[b, i], ids[b, j]]] (see op_relpos_bias_build_ids)."""
    B, K = ids_i32.shape
    heads = table.shape[1]
    out = torch.empty(B, heads, K, Kpad, dtype=torch.bfloat16, device=table.device)
    _check(lib().op_relpos_bias_build_ids(ptr(table), ptr(bucket_i32), bucket_i32.stride(0), ptr(ids_i32), ptr(out), B, heads, K, Kpad,
                                          int(transposed), stream()), "op_relpos_bias_build_ids")
    return out


def relpos_bias_bwd_ids(dbias_f32, bucket_i32, ids_i32, num_rel):
    B, heads, K, Kpad = dbias_f32.shape
    Sfull = bucket_i32.shape[0]
    dense = torch.zeros(heads, Sfull, Sfull, dtype=torch.float32, device=dbias_f32.device)
    _check(lib().op_relpos_bias_fold_ids(ptr(dbias_f32), ptr(ids_i32), ptr(dense), Sfull, B, heads, K, Kpad, stream()),
           "op_relpos_bias_fold_ids")
    return relpos_bias_bwd(dense, bucket_i32, num_rel, Sfull, Sfull)


def attn_spad(S):
    """Padded key/query extent shared by the bias images, key-pad masks, lse and delta rows."""
    return ((S + 127) // 128) * 128


def _bias_bstride(bias):
    """bias [heads, S, Spad]: one image for all samples (stride 0); [B, heads, S, Spad]: one image per sample."""
    return bias.stride(0) if bias is not None and bias.dim() == 4 else 0


def attn_bias_pack(image, S):
    """Row-major bias image(s) [heads, S, Spad] or [B, heads, S, Spad] -> the fragment-major layout the resident forward
    kernel adds with the matrix pipe (flat bf16 tensor; see op_attn_bias_pack)."""
    n_img = image.numel() // (image.shape[-2] * image.shape[-1])
    out = torch.empty(lib().op_attn_bias_frag_elems(n_img, S), dtype=torch.bfloat16, device=image.device)
    _check(lib().op_attn_bias_pack(ptr(image), ptr(out), n_img, S, image.shape[-1], stream()), "op_attn_bias_pack")
    return out


def attn_fwd(q, k, v, ld, B, S, heads, scale, bias=None, key_pad=None, Spad=0, out=None, want_lse=True, bias_frag=None):
    """q, k, v: bf16 views into [B*S, ld] rows (head h at columns h*64..); returns out [B*S, heads*64] and
    lse [B, heads, Spad] (fp32, natural log; entries >= S are unspecified).  bias_frag: attn_bias_pack(bias, S) -- with it
    sequences of up to 320 keys take the resident-K/V kernel (without it a biased call runs the streaming kernel)."""
    dev = q.device
    H = heads * 64
    Spad = Spad or attn_spad(S)
    if out is None:
        out = torch.empty(B * S, H, dtype=torch.bfloat16, device=dev)
    lse = torch.empty(B, heads, Spad, dtype=torch.float32, device=dev) if want_lse else None
    _check(lib().op_attn_fwd(ptr(q), ptr(k), ptr(v), ld, ptr(bias), _bias_bstride(bias), ptr(bias_frag), ptr(key_pad), ptr(out), out.stride(0),
                             ptr(lse), Spad, B, S, Spad, heads, 64, scale, TUNE.attn_fwd(), stream()), "op_attn_fwd")
    return out, lse


def attn_bwd(q, k, v, ld, dout, out, lse, B, S, heads, scale, bias=None, biasT=None, key_pad=None, Spad=0, dqkv=None,
             want_dbias=False, bias_frag=None):
    """Returns dqkv [B*S, 3H] (dq | dk | dv packed like a fused projection output) and dbias fp32: [heads,S,Spad] for a
    shared bias image, [B,heads,S,Spad] when bias / biasT hold one image per sample."""
    dev = q.device
    H = heads * 64
    Spad = Spad or attn_spad(S)
    delta = torch.empty(B, heads, Spad, dtype=torch.float32, device=dev)  # workspace: filled by the dQ kernels (out is passed)
    assert out.stride(0) == dout.stride(0)
    if dqkv is None:
        dqkv = torch.empty(B * S, 3 * H, dtype=torch.bfloat16, device=dev)
    per_sample = bias is not None and bias.dim() == 4
    dbias = attn_dbias_buffer(B, S, heads, Spad, dev, per_sample) if want_dbias else None
    dq, dk, dv = dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:]
    attn_bwd_launch(q, k, v, ld, dout, bias, biasT, key_pad, lse, delta, dq, dk, dv, dqkv.stride(0), dbias, B, S, Spad, heads, scale,
                    bias_frag, out=out)
    if dbias is None:
        return dqkv, None
    return dqkv, (dbias if per_sample else dbias.sum(0))


def attn_bwd_launch(q, k, v, ld, dout, bias, biasT, key_pad, lse, delta, dq, dk, dv, ldg, dbias, B, S, Spad, heads, scale,
                    bias_frag=None, out=None):
    """out (the forward output, row stride as dout): delta is then only a workspace, computed inside the call."""
    _check(lib().op_attn_bwd(ptr(q), ptr(k), ptr(v), ld, ptr(dout), ptr(out), dout.stride(0), ptr(bias), ptr(biasT), ptr(bias_frag),
                             _bias_bstride(bias),
                             ptr(key_pad), ptr(lse), ptr(delta), ptr(dq), ptr(dk), ptr(dv), ldg, ptr(dbias), B, S, Spad, heads,
                             64, scale, TUNE.attn_bwd(), stream()), "op_attn_bwd")


def attn_dbias_buffer(B, S, heads, Spad, device, per_sample=False):
    """Zeroed fp32 [slabs, heads, S, Spad] accumulator for op_attn_bwd's dbias: a shared bias image gets one slab per
    batch chunk (the gradient is the sum over dim 0), per-sample images one slab per sample (slab b = gradient of image b)."""
    slabs = B if per_sample else lib().op_attn_bwd_dbias_slabs(B, S, heads, TUNE.attn_bwd())
    return torch.zeros(slabs, heads, S, Spad, dtype=torch.float32, device=device)


class profile_kernels:
    """Context manager: record HIP-event pairs around gemm/attention launches on their launch stream."""

    def __enter__(self):
        lib().op_prof_enable(1)
        return self

    def __exit__(self, *exc):
        lib().op_prof_enable(0)

    @staticmethod
    def collect(n=4):
        ms = (c_double * n)()
        cnt = (c_int64 * n)()
        work = (c_double * n)()
        lib().op_prof_collect(ms, cnt, work, n)
        return [dict(ms=ms[i], count=cnt[i], work=work[i]) for i in range(n)]


class KeptRows:
    """The samples ONE residual branch of ONE layer keeps under stochastic depth, as the row packing op_rows_gather / op_rows_merge
    work with.  segs: [(src_row0, S, n_samples, kept sample numbers ascending)] per segment of the packed activation matrix;
    `lists`: the device int32 tensor that holds, from `base` on, for every segment its kept list followed by its inverse list
    (position among the kept samples or -1) -- built for the whole stack at once by `pack_kept_lists` (one host-to-device copy per
    step).  Every segment's packed rows are rounded up to a multiple of `pad` (zero rows: the weight-gradient kernels want
    K % 64 == 0, whole 256-row tiles avoid tail launches)."""

    def __init__(self, segs, lists, base, full_rows, scale, pad=256):
        n = len(segs)
        assert 1 <= n <= 4
        self.lists, self.full_rows, self.scale, self.nseg = lists, int(full_rows), float(scale), n
        self.S = [int(s[1]) for s in segs]
        self.n_samples = [int(s[2]) for s in segs]
        self.n_kept = [len(s[3]) for s in segs]
        self.src_row0 = [int(s[0]) for s in segs]
        self.dst_rows = [-(-(k * S) // pad) * pad for k, S in zip(self.n_kept, self.S)]
        self.dst_row0, self.off_kept, self.off_inv = [], [], []
        r, o = 0, int(base)
        for k, ns, dr in zip(self.n_kept, self.n_samples, self.dst_rows):
            self.dst_row0.append(r)
            self.off_kept.append(o)
            self.off_inv.append(o + k)
            r, o = r + dr, o + k + ns
        self.total, self.list_end = r, o
        arr = lambda v: (c_int64 * n)(*v)  # noqa: E731
        self._c = tuple(arr(v) for v in (self.src_row0, self.dst_row0, self.S, self.n_kept, self.dst_rows, self.n_samples))
        self._c_kept, self._c_inv = arr(self.off_kept), arr(self.off_inv)

    def kept_list(self, i):
        """Device int32 view: the kept sample numbers of segment i (e.g. to index_select the key-padding rows)."""
        return self.lists[self.off_kept[i]:self.off_kept[i] + self.n_kept[i]]

    def rowmap(self):
        """Device int32 [total]: the row of the full matrix behind every packed row (-1: a surplus row of a rounded-up segment) -- the
        table the kernels that read / write THROUGH the packing take (op_rows_map; built once per branch and step, on first use)."""
        m = getattr(self, "_rowmap", None)
        if m is None:
            m = torch.empty(self.total, dtype=torch.int32, device=self.lists.device)
            c = self._c
            _check(lib().op_rows_map(ptr(m), ptr(self.lists), self.nseg, c[0], c[1], c[2], c[3], c[4], c[5], self._c_kept, self.total,
                                     stream()), "op_rows_map")
            self._rowmap = m
        return m


def pack_kept_lists(plans):
    """plans: [[(src_row0, S, n_samples, kept list)] per segment] per branch -> (int32 CPU tensor with all kept / inverse lists, the
    offset of each plan's first entry).  Host only."""
    out, bases = [], []
    for segs in plans:
        bases.append(len(out))
        for _, _, ns, kept in segs:
            inv = [-1] * ns
            for j, smp in enumerate(kept):
                inv[smp] = j
            out.extend(int(v) for v in kept)
            out.extend(inv)
    return torch.tensor(out if out else [0], dtype=torch.int32), bases


def rows_gather(src, kr):
    """Pack the rows of the kept samples: [kr.total, cols] (zero rows where a segment is rounded up)."""
    assert src.dim() == 2 and src.is_contiguous() and src.shape[0] == kr.full_rows and src.dtype == torch.bfloat16
    dst = torch.empty(kr.total, src.shape[1], dtype=src.dtype, device=src.device)
    c = kr._c
    _check(lib().op_rows_gather(ptr(src), ptr(dst), ptr(kr.lists), kr.nseg, c[0], c[1], c[2], c[3], c[4], c[5], kr._c_kept, kr.total,
                                src.shape[1], stream()), "op_rows_gather")
    return dst


def rows_merge(base, upd, kr, out=None):
    """base with the rows of the kept samples replaced by the packed rows `upd`; out=base: in place.  upd=None (out given, not base):
    only the rows of the DROPPED samples are copied into out (the kept rows were written through KeptRows.rowmap)."""
    assert base.dim() == 2 and base.is_contiguous() and base.shape[0] == kr.full_rows and base.dtype == torch.bfloat16
    if upd is None:
        assert out is not None and out is not base and out.shape == base.shape and out.is_contiguous()
    else:
        assert upd.is_contiguous() and upd.shape[0] == kr.total and upd.dtype == torch.bfloat16 and base.shape[1] == upd.shape[1]
    if out is None:
        out = torch.empty_like(base)
    c = kr._c
    _check(lib().op_rows_merge(ptr(base), ptr(upd), ptr(out), ptr(kr.lists), kr.nseg, c[0], c[1], c[2], c[3], c[4], c[5], kr._c_inv,
                               kr.full_rows, base.shape[1], stream()), "op_rows_merge")
    return out


SIM_TOPK_MAX_K = 64


def sim_topk(q, g, k, splits=None):
    """(vals fp32 [M, k] descending, idx int64 [M, k]): the k largest q[m] . g[n] per query row (op_sim_topk; the [M, N] scores are
    never formed).  q [M, D], g [N, D] bf16 CUDA with unit column stride; D is zero-padded to a multiple of 32 when needed.  Exact
    ties: lower n first; NaN above +inf.  splits: None / 0 = the library's choice, else the gallery split count (tests)."""
    assert q.dtype == torch.bfloat16 and g.dtype == torch.bfloat16 and q.is_cuda and g.is_cuda, "sim_topk takes bf16 CUDA tensors"
    assert q.dim() == 2 and g.dim() == 2 and q.shape[1] == g.shape[1], "sim_topk: q [M, D] and g [N, D]"
    M, D = q.shape
    N = g.shape[0]
    if not 1 <= k <= min(N, SIM_TOPK_MAX_K):
        raise ValueError("sim_topk: need 1 <= k <= min(N, %d), got k = %d, N = %d" % (SIM_TOPK_MAX_K, k, N))

    def operand(x):
        if D % 32 or x.stride(1) != 1 or x.stride(0) % 8 or x.data_ptr() % 16:
            Dp = (D + 31) // 32 * 32
            y = torch.zeros(x.shape[0], Dp, dtype=x.dtype, device=x.device)
            y[:, :D] = x
            return y
        return x

    q, g = operand(q), operand(g)
    vals = torch.empty(M, k, dtype=torch.float32, device=q.device)
    idx = torch.empty(M, k, dtype=torch.int32, device=q.device)
    if M == 0:
        return vals, idx.long()
    s = int(splits or 0)
    ws_bytes = lib().op_sim_topk_workspace_bytes(M, N, k, s)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=q.device) if ws_bytes else None
    _check(lib().op_sim_topk(ptr(q), q.stride(0), ptr(g), g.stride(0), M, N, q.shape[1], k, ptr(vals), ptr(idx), ptr(ws), ws_bytes, s,
                             stream()), "op_sim_topk")
    return vals, idx.long()


DT_U8 = 2  # op_image_resize_normalize only: the resized uint8 pixels, [B, S, S, 3]
_IMAGE_OUT = {torch.bfloat16: DT_BF16, torch.float32: DT_F32, torch.uint8: DT_U8}


def image_resize_normalize(packed, mean=None, std=None, dtype=torch.bfloat16, device=None):
    """[B, 3, S, S] bf16 / fp32 (or uint8 [B, S, S, 3] for dtype=torch.uint8) of an imageprep.PackedImages batch on a device
    (op_image_resize_normalize): PIL's bicubic Resize((S, S)), then (u / 255 - mean) / std in fp32 and the cast, bit for bit.  The
    packed host buffer goes to the device in ONE copy; the uint8 intermediate is a workspace of packed.workspace_bytes."""
    if dtype not in _IMAGE_OUT:
        raise TypeError("image_resize_normalize: dtype must be bfloat16, float32 or uint8, got %s" % dtype)
    if dtype != torch.uint8 and (mean is None or std is None):
        raise ValueError("image_resize_normalize: mean and std are required for a normalised output")
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    B, S = len(packed), packed.size
    out = torch.empty((B, S, S, 3) if dtype == torch.uint8 else (B, 3, S, S), dtype=dtype, device=dev)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        buf = packed.host.to(dev, non_blocking=packed.host.is_pinned())
        ws = torch.empty(packed.workspace_bytes, dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        m = (c_float * 3)(*mean) if mean is not None else None
        sd = (c_float * 3)(*std) if std is not None else None
        args = (c_void_p(base), packed.src_bytes, c_void_p(base + packed.desc_off), packed.desc.ctypes.data_as(c_void_p), B,
                c_void_p(base + packed.coef_off), packed.coef_count, S, m, sd, ptr(out), _IMAGE_OUT[dtype], ptr(ws), ws.numel())
        if getattr(packed, "flip_off", None) is None:
            _check(lib().op_image_resize_normalize(*args, stream()), "op_image_resize_normalize")
        else:  # the per-image flip flags travel in the same buffer (imageprep.pack_images(flips = ...))
            _check(lib().op_image_resize_normalize_flip(*args, c_void_p(base + packed.flip_off), stream()), "op_image_resize_normalize_flip")
    return out


ENOTSUP = -95  # OP_ENOTSUP (csrc/common.h)


def mix_tables(params, B, device):
    """The (kind int32 [B], lam fp32 [B], one_minus_lam fp32 [B], box int32 [B, 4]) tables of ops.mix_images on `device`, staged as ONE
    16 x B-byte buffer (one H2D copy) when they come from the host."""
    import numpy as np
    kind, lam, oml, box = params
    if all(torch.is_tensor(t) and t.device == device for t in params):
        return (kind.to(torch.int32).contiguous(), lam.to(torch.float32).contiguous(), oml.to(torch.float32).contiguous(),
                box.to(torch.int32).contiguous())
    host = np.empty((7, B), dtype=np.int32)
    as_np = lambda t: t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    host[0] = as_np(kind).astype(np.int32).reshape(B)
    host[1] = as_np(lam).astype(np.float32).reshape(B).view(np.int32)
    host[2] = as_np(oml).astype(np.float32).reshape(B).view(np.int32)
    host[3:] = as_np(box).astype(np.int32).reshape(B, 4).T
    dev = torch.from_numpy(host).to(device)
    return dev[0], dev[1].view(torch.float32), dev[2].view(torch.float32), dev[3:].t().contiguous()


def mix_images(x, params, out=None):
    """op_mix_images on x [B, C, H, W] bf16 / fp32 (contiguous, CUDA) with the device tables `params` of mix_tables: Mixup / CutMix of
    sample i with sample B - 1 - i into `out` (x itself = in place; None = a new tensor of x's dtype).  Returns out, or None when the
    library answers OP_ENOTSUP (W or C H W not a multiple of 8, unaligned pointers): the caller takes the torch route."""
    _req(x, "x")
    out = torch.empty_like(x) if out is None else out
    _req(out, "out")
    if x.dim() != 4 or out.shape != x.shape:
        raise ValueError("mix_images: x and out must be [B, C, H, W] of one shape, got %s and %s" % (tuple(x.shape), tuple(out.shape)))
    kind, lam, oml, box = params
    B, C, H, W = x.shape
    for t, name, dt, n in ((kind, "kind", torch.int32, B), (lam, "lam", torch.float32, B), (oml, "one_minus_lam", torch.float32, B),
                           (box, "box", torch.int32, 4 * B)):
        _req(t, name, dt)
        if t.numel() != n:
            raise ValueError("mix_images: %s has %d elements, need %d" % (name, t.numel(), n))
    if B == 0 or C * H * W == 0:
        return out
    with torch.cuda.device(x.device):
        rc = lib().op_mix_images(ptr(x), ptr(out), _dt(x), _dt(out), B, C * H * W, H, W, ptr(kind), ptr(lam), ptr(oml), ptr(box), stream())
    if rc == ENOTSUP:
        return None
    _check(rc, "op_mix_images")
    return out


def _u8_batch(u8, what):
    """(B, S) of a dense uint8 [B, S, S, 3] CUDA batch."""
    _req(u8, "u8", torch.uint8)
    if u8.dim() != 4 or u8.shape[3] != 3 or u8.shape[1] != u8.shape[2]:
        raise ValueError("%s: need uint8 [B, S, S, 3], got %s" % (what, tuple(u8.shape)))
    return u8.shape[0], u8.shape[1]


def image_color_jitter(u8, ops, factors):
    """op_image_color_jitter IN PLACE on u8 [B, S, S, 3] (uint8, contiguous, CUDA): per image the chain ops int32 [B, 3] (0 none, 1 brightness,
    2 contrast, 3 saturation) with factors fp32 [B, 3] (host arrays, imageprep.jitter_table), PIL.ImageEnhance bit for bit.  The tables
    and the zeroed sum(L) workspace go to the device as ONE 28 x B-byte buffer.  Returns u8."""
    import numpy as np
    B, S = _u8_batch(u8, "image_color_jitter")
    ops = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(B, 3))
    fac = np.ascontiguousarray(np.asarray(factors, dtype=np.float32).reshape(B, 3))
    if B == 0:
        return u8
    host = np.zeros(7 * B, dtype=np.int32)
    host[:3 * B], host[3 * B:6 * B] = ops.reshape(-1), fac.view(np.int32).reshape(-1)
    with torch.cuda.device(u8.device):
        dev = torch.from_numpy(host).to(u8.device)
        base = dev.data_ptr()
        _check(lib().op_image_color_jitter(ptr(u8), B, S, c_void_p(base), c_void_p(base + 12 * B), ops.ctypes.data_as(c_void_p),
                                           fac.ctypes.data_as(c_void_p), c_void_p(base + 24 * B), stream()), "op_image_color_jitter")
    return u8


def image_gaussian_blur(u8, R, ww, fw, on):
    """op_image_gaussian_blur IN PLACE on u8 [B, S, S, 3] (uint8, contiguous, CUDA): ImageFilter.GaussianBlur bit for bit, with the per-image
    box parameters R, ww, fw (imageprep.gaussian_box_params) and on flags (0 = not blurred, not touched), host arrays of B entries; they go
    to the device as ONE 16 x B-byte buffer.  Returns u8."""
    import numpy as np
    B, S = _u8_batch(u8, "image_gaussian_blur")
    R = np.ascontiguousarray(np.asarray(R, dtype=np.int32).reshape(B))
    on = np.ascontiguousarray(np.asarray(on, dtype=np.uint8).reshape(B))
    if B == 0:
        return u8
    host = np.zeros(4 * B, dtype=np.uint32)
    host[:B], host[B:2 * B], host[2 * B:3 * B] = R.view(np.uint32), np.asarray(ww, dtype=np.uint32).reshape(B), np.asarray(fw, dtype=np.uint32).reshape(B)
    host[3 * B:].view(np.uint8)[:B] = on
    with torch.cuda.device(u8.device):
        dev = torch.from_numpy(host.view(np.int32)).to(u8.device)
        base = dev.data_ptr()
        _check(lib().op_image_gaussian_blur(ptr(u8), B, S, c_void_p(base), c_void_p(base + 4 * B), c_void_p(base + 8 * B), c_void_p(base + 12 * B),
                                            R.ctypes.data_as(c_void_p), on.ctypes.data_as(c_void_p), stream()), "op_image_gaussian_blur")
    return u8


def image_normalize_flip(u8, mean, std, dtype=torch.float32, flips=None):
    """[B, 3, S, S] bf16 / fp32 from u8 [B, S, S, 3] (uint8, contiguous, CUDA): op_image_normalize_flip, the ToTensor / Normalize arithmetic, the
    cast and the flip of op_image_resize_normalize_flip.  flips: None, or one flag per image (a uint8 CUDA tensor, or host values)."""
    B, S = _u8_batch(u8, "image_normalize_flip")
    if dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("image_normalize_flip: dtype must be bfloat16 or float32, got %s" % dtype)
    out = torch.empty((B, 3, S, S), dtype=dtype, device=u8.device)
    if B == 0:
        return out
    with torch.cuda.device(u8.device):
        if flips is not None and not (torch.is_tensor(flips) and flips.is_cuda):
            flips = torch.as_tensor([1 if f else 0 for f in (flips.tolist() if hasattr(flips, "tolist") else flips)], dtype=torch.uint8).to(u8.device)
        if flips is not None:
            _req(flips, "flips", torch.uint8)
            if flips.numel() != B:
                raise ValueError("image_normalize_flip: need one flip flag per image, got %d for %d images" % (flips.numel(), B))
        _check(lib().op_image_normalize_flip(ptr(u8), B, S, (c_float * 3)(*mean), (c_float * 3)(*std), ptr(out), _IMAGE_OUT[dtype], ptr(flips),
                                             stream()), "op_image_normalize_flip")
    return out


def image_randaug_layer(u8, ops, args, fill, scratch=None):
    """op_image_randaug_layer IN PLACE on u8 [B, S, S, 3] (uint8, contiguous, CUDA): one RandAugment layer, ops int32 [B] (imageprep.RANDAUG_OPS;
    not 7 ... 9, which are op_image_color_jitter's) with args fp64 [B, 6] (host arrays), fill = the three bytes of Affine's uncovered pixels.
    The tables and the histogram workspace go to the device as ONE buffer; scratch: a uint8 tensor of u8's size to reuse between layers.
    Returns u8."""
    import numpy as np
    B, S = _u8_batch(u8, "image_randaug_layer")
    ops = np.ascontiguousarray(np.asarray(ops, dtype=np.int32).reshape(B))
    args = np.ascontiguousarray(np.asarray(args, dtype=np.float64).reshape(B, 6))
    if B == 0 or not ops.any():
        return u8
    fill = (c_ubyte * 3)(*[int(v) for v in fill])
    uses_hist = bool(((ops == 1) | (ops == 2)).any())
    head = 8 * B  # int64 words: args [6 B], ops [B / 2, padded to B], then the histograms
    host = np.zeros(head + (384 * B if uses_hist else 0), dtype=np.int64)
    host[:6 * B] = args.view(np.int64).reshape(-1)
    host[6 * B:8 * B].view(np.int32)[:B] = ops
    with torch.cuda.device(u8.device):
        dev = torch.from_numpy(host).to(u8.device)
        base = dev.data_ptr()
        if scratch is None:
            scratch = torch.empty_like(u8)
        _req(scratch, "scratch", torch.uint8)
        if scratch.numel() != u8.numel():
            raise ValueError("image_randaug_layer: the scratch must have u8's size")
        # (without a histogram op the workspace is never read or written: it stands on the tables)
        _check(lib().op_image_randaug_layer(ptr(u8), B, S, c_void_p(base + 48 * B), c_void_p(base), ops.ctypes.data_as(c_void_p),
                                            args.ctypes.data_as(c_void_p), fill, c_void_p(base + (64 * B if uses_hist else 0)), ptr(scratch),
                                            stream()), "op_image_randaug_layer")
    return u8


def image_erase(x, boxes, noise, noise_off):
    """op_image_erase IN PLACE on x [B, 3, S, S] bf16 / fp32 (contiguous, CUDA): x[i, :, top:top+h, left:left+w] = the 3 h w fp32 values of
    `noise` (a CUDA fp32 tensor) at noise_off[i], cast once; boxes int32 [B, 4] (top, left, h, w; h = 0: untouched) and noise_off int64 [B]
    are host arrays, staged in ONE buffer.  Returns x."""
    import numpy as np
    _req(x, "x")
    if x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3]:
        raise ValueError("image_erase: need x [B, 3, S, S], got %s" % (tuple(x.shape),))
    B, S = x.shape[0], x.shape[2]
    boxes = np.ascontiguousarray(np.asarray(boxes, dtype=np.int32).reshape(B, 4))
    offs = np.ascontiguousarray(np.asarray(noise_off, dtype=np.int64).reshape(B))
    if B == 0 or S == 0:
        return x
    need = max([0] + [int(o) + 3 * int(b[2]) * int(b[3]) for o, b in zip(offs, boxes) if b[2] > 0])
    if need and (noise is None or noise.numel() < need or int(offs.min()) < 0):
        raise ValueError("image_erase: the noise buffer holds %d values, the boxes need %d" % (0 if noise is None else noise.numel(), need))
    if noise is not None:
        _req(noise, "noise", torch.float32)
    host = np.zeros(3 * B, dtype=np.int64)
    host[:B], host[B:].view(np.int32)[:4 * B] = offs, boxes.reshape(-1)
    with torch.cuda.device(x.device):
        dev = torch.from_numpy(host).to(x.device)
        base = dev.data_ptr()
        _check(lib().op_image_erase(ptr(x), _dt(x), B, S, c_void_p(base + 8 * B), boxes.ctypes.data_as(c_void_p), ptr(noise), c_void_p(base),
                                    stream()), "op_image_erase")
    return x


def audio_normalize_pad(packed, dtype=torch.float32, device=None):
    """[B, T] fp32 / bf16 of an audioprep.PackedClips batch on a device (op_audio_normalize_pad): channel mean, layer norm over each
    whole clip, crop to max_len, tiling up to min_len, zero padding to T = the longest output, the cast.  The packed host buffer
    (samples + descriptor table) goes to the device in ONE copy; the statistics partials are a workspace of packed.workspace_bytes."""
    if dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("audio_normalize_pad: dtype must be bfloat16 or float32, got %s" % dtype)
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    B, T = len(packed), packed.T
    out = torch.empty((B, T), dtype=dtype, device=dev)
    if B == 0:
        return out
    with torch.cuda.device(dev):
        buf = packed.host.to(dev, non_blocking=packed.host.is_pinned())
        ws = torch.empty(max(packed.workspace_bytes, 16), dtype=torch.uint8, device=dev)
        base = buf.data_ptr()
        _check(lib().op_audio_normalize_pad(c_void_p(base), packed.src_bytes, c_void_p(base + packed.desc_off),
                                            packed.desc.ctypes.data_as(c_void_p), B, packed.max_len, packed.min_len, ptr(out), T,
                                            DT_BF16 if dtype == torch.bfloat16 else DT_F32, ptr(ws), ws.numel(), stream()),
               "op_audio_normalize_pad")
    return out


def audio_resample(packed, device=None):
    """Run op_audio_resample on an audioprep.PackedResample batch: the packed host buffer (clips, descriptors, coefficient tables and,
    where staged, the normaliser's descriptors) goes to the device in ONE copy.  Staged with norm=None it returns the resampled clips
    as fp32 [B, rows] (row i zero behind packed.lengths[i]; the rows of clips already at the target rate stay zero, the caller owns
    them).  Staged with norm=(max_len, min_len) it returns the uint8 device buffer of packed.total_bytes -- host part, then the
    resampled mono fp32 clips at packed.out_off -- for audio_normalize_pad_device."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    with torch.cuda.device(dev):
        buf = torch.empty(packed.total_bytes, dtype=torch.uint8, device=dev)
        buf[:packed.host.numel()].copy_(packed.host, non_blocking=packed.host.is_pinned())
        base = buf.data_ptr()
        if packed.norm_desc is None:
            out = torch.zeros((len(packed), packed.rows), dtype=torch.float32, device=dev)
            out_ptr = out.data_ptr()
        else:
            out, out_ptr = buf, base + packed.out_off
        if len(packed.which):
            _check(lib().op_audio_resample(c_void_p(base), packed.src_bytes, c_void_p(base + packed.desc_off),
                                           packed.desc.ctypes.data_as(c_void_p), len(packed.which), c_void_p(base + packed.coef_off),
                                           packed.coef_count, c_void_p(out_ptr), packed.out_bytes, stream()), "op_audio_resample")
    return out


def audio_normalize_pad_device(buf, packed, dtype=torch.float32):
    """audio_normalize_pad on a packed buffer that is already on the device: `buf` is audio_resample's buffer of a PackedResample staged
    with norm=(max_len, min_len), whose normaliser descriptors point at the resampled clips (and at the staged source of clips that
    needed no resampling).  No host round trip: op_audio_normalize_pad reads what op_audio_resample wrote, in stream order."""
    if dtype not in (torch.bfloat16, torch.float32):
        raise TypeError("audio_normalize_pad_device: dtype must be bfloat16 or float32, got %s" % dtype)
    B, T = len(packed), packed.T
    out = torch.empty((B, T), dtype=dtype, device=buf.device)
    if B == 0:
        return out
    with torch.cuda.device(buf.device):
        ws = torch.empty(max(packed.workspace_bytes, 16), dtype=torch.uint8, device=buf.device)
        base = buf.data_ptr()
        _check(lib().op_audio_normalize_pad(c_void_p(base), packed.total_bytes, c_void_p(base + packed.norm_desc_off),
                                            packed.norm_desc.ctypes.data_as(c_void_p), B, packed.max_len, packed.min_len, ptr(out), T,
                                            DT_BF16 if dtype == torch.bfloat16 else DT_F32, ptr(ws), ws.numel(), stream()),
               "op_audio_normalize_pad")
    return out


def average_precision(scores, targets):
    """(ap fp64 [C], npos int32 [C]) of scores fp32 [N, C] and targets uint8 [N, C] (non-zero = positive) on a device
    (op_average_precision): per class the mean over the positives i of #{positives scoring >= s_i} / #{samples scoring >= s_i}, 0.0 for
    a class without positives.  Unit column stride, any row stride; the keys, target bits and partial sums are a workspace of
    op_average_precision_workspace_bytes(N, C)."""
    assert scores.dtype == torch.float32 and targets.dtype == torch.uint8 and scores.is_cuda and targets.is_cuda, \
        "average_precision takes fp32 scores and uint8 targets on a CUDA device"
    assert scores.dim() == 2 and scores.shape == targets.shape, "average_precision: scores and targets [N, C]"
    N, C = scores.shape
    if N < 1 or C < 1:
        raise ValueError("average_precision: need N >= 1 and C >= 1, got [%d, %d]" % (N, C))
    if scores.stride(1) != 1 or scores.stride(0) < C:
        scores = scores.contiguous()
    if targets.stride(1) != 1 or targets.stride(0) < C:
        targets = targets.contiguous()
    with torch.cuda.device(scores.device):
        ap = torch.empty(C, dtype=torch.float64, device=scores.device)
        npos = torch.empty(C, dtype=torch.int32, device=scores.device)
        ws_bytes = lib().op_average_precision_workspace_bytes(N, C)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=scores.device)
        _check(lib().op_average_precision(ptr(scores), scores.stride(0), ptr(targets), targets.stride(0), N, C, ptr(ap), ptr(npos),
                                          ptr(ws), ws_bytes, stream()), "op_average_precision")
    return ap, npos


ROW_LOSS_HARD, ROW_LOSS_SOFT, ROW_LOSS_MULTI, ROW_LOSS_HINGE = 0, 1, 2, 3


def row_loss(logits, targets, mode, label_smoothing=0.0, margin=1.0, gscale=1.0, write_grad=True):
    """op_row_loss on logits [B, C] (bf16 / fp32, unit column stride; a column slice of a wider matrix is fine).  targets: int64 [B] in
    the hard and hinge modes, bf16 / fp32 [B, C] in the soft and multi-label modes.  Returns (sums fp32 [2] = (sum of the row losses,
    sum of the row counters), row_loss fp32 [B], row_correct fp32 [B], dlogits fp32 [B, C] or None)."""
    assert logits.is_cuda and logits.dim() == 2 and logits.stride(1) == 1, "row_loss takes CUDA logits [B, C] with unit column stride"
    B, C = logits.shape
    dense = mode in (ROW_LOSS_SOFT, ROW_LOSS_MULTI)
    if dense:
        assert targets.is_cuda and tuple(targets.shape) == (B, C) and targets.stride(1) == 1, "row_loss: targets [B, C], unit column stride"
        tdt, ldt = _dt(targets), targets.stride(0)
    else:
        _req(targets, "targets", torch.int64)
        assert tuple(targets.shape) == (B,), "row_loss: targets [B]"
        tdt, ldt = 0, 0
    dev = logits.device
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    correct = torch.empty(B, dtype=torch.float32, device=dev)
    dlogits = torch.empty(B, C, dtype=torch.float32, device=dev) if write_grad else None
    sums = torch.zeros(2, dtype=torch.float32, device=dev) if B == 0 else torch.empty(2, dtype=torch.float32, device=dev)
    _check(lib().op_row_loss(ptr(logits), _dt(logits), logits.stride(0) if B > 1 else max(C, logits.stride(0)), ptr(targets), tdt,
                             ldt if B > 1 else max(C, ldt), B, C, mode, label_smoothing, margin, gscale, ptr(loss), ptr(correct),
                             ptr(dlogits), ptr(sums), stream()), "op_row_loss")
    return sums, loss, correct, dlogits


def box_loss(logits, targets, gscale=1.0, write_grad=True):
    """op_box_loss on contiguous logits [B, 4] (bf16 / fp32) and fp32 targets [B, 4].  Returns (out fp32 [2] = (loss, valid rows),
    dlogits fp32 [B, 4] or None)."""
    _req(logits, "logits")
    _req(targets, "targets", torch.float32)
    assert logits.dim() == 2 and logits.shape[1] == 4 and tuple(targets.shape) == tuple(logits.shape), "box_loss: logits, targets [B, 4]"
    B = logits.shape[0]
    out = torch.full((2,), float("nan"), dtype=torch.float32, device=logits.device) if B == 0 else torch.empty(
        2, dtype=torch.float32, device=logits.device)
    dlogits = torch.empty(B, 4, dtype=torch.float32, device=logits.device) if write_grad else None
    _check(lib().op_box_loss(ptr(logits), _dt(logits), ptr(targets), B, gscale, ptr(out), ptr(dlogits), stream()), "op_box_loss")
    return out, dlogits


ATTN_POOL_MAX_S = 4096  # csrc/attnpool.hip: AP_MAX_S


def attn_pool_supported(k, v, heads, hd):
    """The limits of op_attn_pool_fwd / _bwd for k, v [B, S, heads * hd] (any batch / row strides the kernel takes)."""
    if k.dim() != 3 or k.shape != v.shape or k.shape[2] != heads * hd or k.stride() != v.stride():
        return False
    B, S, _ = k.shape
    return (hd % 8 == 0 and 8 <= hd <= 128 and 1 <= S <= ATTN_POOL_MAX_S and B >= 1 and k.stride(2) == 1
            and k.stride(1) % 8 == 0 and k.stride(1) >= heads * hd and k.stride(0) % 8 == 0 and k.stride(0) >= 0
            and k.data_ptr() % 16 == 0 and v.data_ptr() % 16 == 0)


def _attn_pool_kv(k, v, heads, hd):
    for t, name in ((k, "k"), (v, "v")):
        if not t.is_cuda or t.dtype != torch.bfloat16 or t.dim() != 3 or t.stride(2) != 1:
            raise RuntimeError("attn_pool: %s must be a bf16 CUDA(HIP) tensor [B, S, heads * hd] with unit column stride" % name)
    if k.shape != v.shape or k.stride() != v.stride() or k.shape[2] != heads * hd:
        raise RuntimeError("attn_pool: k %s / v %s must share shape and strides, last dim heads * hd = %d" % (
            tuple(k.shape), tuple(v.shape), heads * hd))
    B, S, _ = k.shape
    ld = k.stride(1) if S > 1 else max(k.stride(1), heads * hd)     # (torch gives a size-1 dimension any stride)
    bs = k.stride(0) if B > 1 else 0
    return B, S, ld, bs


def attn_pool_fwd(k, v, q, pad=None, out=None, p=None):
    """op_attn_pool_fwd: k, v bf16 [B, S, heads * hd] (shared strides, unit column stride), q bf16 [heads, hd] contiguous, pad uint8 /
    bool [B, S] (non-zero = masked; unit column stride) or None.  Returns (out bf16 [B, heads * hd], p fp32 [B, heads, S])."""
    heads, hd = q.shape
    _req(q, "q", torch.bfloat16)
    B, S, ld, bs = _attn_pool_kv(k, v, heads, hd)
    ld_pad = 0
    if pad is not None:
        if pad.dtype == torch.bool:
            pad = pad.view(torch.uint8)
        if not pad.is_cuda or pad.dtype != torch.uint8 or tuple(pad.shape) != (B, S) or (S > 1 and pad.stride(1) != 1):
            raise RuntimeError("attn_pool_fwd: pad must be a uint8 / bool CUDA(HIP) tensor [B, S] with unit column stride")
        ld_pad = pad.stride(0) if B > 1 else max(pad.stride(0), S)
    if out is None:
        out = torch.empty(B, heads * hd, dtype=torch.bfloat16, device=k.device)
    if p is None:
        p = torch.empty(B, heads, S, dtype=torch.float32, device=k.device)
    assert out.is_contiguous() and out.dtype == torch.bfloat16 and tuple(out.shape) == (B, heads * hd)
    assert p.is_contiguous() and p.dtype == torch.float32 and p.numel() == B * heads * S
    _check(lib().op_attn_pool_fwd(ptr(k), ptr(v), ld, bs, ptr(q), ptr(pad), ld_pad, ptr(out), ptr(p), B, S, heads, hd, stream()),
           "op_attn_pool_fwd")
    return out, p


def attn_pool_bwd(dout, k, v, q, p, dk=None, dv=None, dq_part=None):
    """op_attn_pool_bwd: returns (dk, dv bf16 [B, S, heads * hd], dq_part fp32 [B, heads * hd]); the caller sums dq_part over B.
    dk / dv may be given as views with their own (shared) strides."""
    heads, hd = q.shape
    _req(q, "q", torch.bfloat16)
    _req(dout, "dout", torch.bfloat16)
    _req(p, "p", torch.float32)
    B, S, ld, bs = _attn_pool_kv(k, v, heads, hd)
    if dk is None:
        dk = torch.empty(B, S, heads * hd, dtype=torch.bfloat16, device=k.device)
        dv = torch.empty(B, S, heads * hd, dtype=torch.bfloat16, device=k.device)
    _, _, ldg, bsg = _attn_pool_kv(dk, dv, heads, hd)
    assert dk.shape == k.shape and tuple(dout.shape) == (B, heads * hd) and p.numel() == B * heads * S
    if dq_part is None:
        dq_part = torch.empty(B, heads * hd, dtype=torch.float32, device=k.device)
    assert dq_part.is_contiguous() and dq_part.dtype == torch.float32 and tuple(dq_part.shape) == (B, heads * hd)
    _check(lib().op_attn_pool_bwd(ptr(dout), ptr(k), ptr(v), ld, bs, ptr(q), ptr(p), ptr(dk), ptr(dv), ldg, bsg, ptr(dq_part), B, S, heads,
                                  hd, stream()), "op_attn_pool_bwd")
    return dk, dv, dq_part


TOKEN_POOL_MAX_SPLITS = 16  # include/onepeace_hip.h: OP_TOKEN_POOL_MAX_SPLITS (csrc/tokenpool.hip: TP_MAX_SPLITS)
TOKEN_POOL_MAX_B = 1 << 20


def _token_pool_strides(x):
    """(ld, batch_stride) of a [B, S, H] view as the entries take them (torch gives a size-1 dimension any stride)."""
    B, S, H = x.shape
    return x.stride(1), (x.stride(0) if B > 1 else 0)


def token_pool_supported(x, w=None, b=None):
    """The limits of op_token_mean_ln_fwd / _bwd for x [B, S, H] (any batch / row strides the kernels take), w and b [H] or None."""
    if x.dim() != 3 or x.dtype != torch.bfloat16 or not x.is_cuda:
        return False
    B, S, H = x.shape
    for t in (w, b):
        if t is not None and not (t.is_cuda and t.dtype == torch.bfloat16 and tuple(t.shape) == (H,) and t.is_contiguous()
                                  and t.data_ptr() % 16 == 0):
            return False
    ld, bs = _token_pool_strides(x)
    return (H % 8 == 0 and 8 <= H <= 8192 and 2 <= S <= 65536 and 1 <= B <= TOKEN_POOL_MAX_B and x.stride(2) == 1 and ld % 8 == 0
            and ld >= H and bs % 8 == 0 and bs >= 0 and x.data_ptr() % 16 == 0)


def _token_pool_view(t, name):
    if not t.is_cuda or t.dtype != torch.bfloat16 or t.dim() != 3 or t.stride(2) != 1:
        raise RuntimeError("token_mean_ln: %s must be a bf16 CUDA(HIP) tensor [B, S, H] with unit column stride" % name)
    return tuple(t.shape) + _token_pool_strides(t)


def token_mean_ln_fwd(x, w, b, eps=1e-5, y=None, pooled=None, mean=None, rstd=None):
    """op_token_mean_ln_fwd: x bf16 [B, S, H] (own strides, unit column stride), w / b bf16 [H] or None.  Returns (y bf16 [B, H],
    pooled fp32 [B, H], mean fp32 [B], rstd fp32 [B]); the split partials live in the grow-only workspace of this stream."""
    B, S, H, ld, bs = _token_pool_view(x, "x")
    _req(w, "w", torch.bfloat16)
    _req(b, "b", torch.bfloat16)
    dev = x.device
    if y is None:
        y = torch.empty(B, H, dtype=torch.bfloat16, device=dev)
    if pooled is None:
        pooled = torch.empty(B, H, dtype=torch.float32, device=dev)
    if mean is None:
        mean = torch.empty(B, dtype=torch.float32, device=dev)
    if rstd is None:
        rstd = torch.empty(B, dtype=torch.float32, device=dev)
    for t, name, dt, shape in ((y, "y", torch.bfloat16, (B, H)), (pooled, "pooled", torch.float32, (B, H)),
                               (mean, "mean", torch.float32, (B,)), (rstd, "rstd", torch.float32, (B,))):
        _req(t, name, dt)
        assert tuple(t.shape) == shape, "%s must be %s" % (name, shape)
    part = workspace(4 * B * TOKEN_POOL_MAX_SPLITS * H, dev, "token_pool")
    _check(lib().op_token_mean_ln_fwd(ptr(x), ld, bs, ptr(w), ptr(b), eps, ptr(y), ptr(pooled), ptr(mean), ptr(rstd), ptr(part), B, S, H,
                                      stream()), "op_token_mean_ln_fwd")
    return y, pooled, mean, rstd


def token_mean_ln_bwd(dy, pooled, w, mean, rstd, S, dx=None, want_parts=True, dw_part=None, db_part=None, want_dx=True):
    """op_token_mean_ln_bwd: returns (dx bf16 [B, S, H], dw_part, db_part fp32 [H] or None).  dx may be given as a view with its own
    strides; every element of [B, S, H] is written, row 0 with zeros.  dw_part / db_part may be given (contiguous fp32 [H], e.g. the two
    rows of one [2, H] buffer; either may stay None); with neither given, want_parts says whether the pair is allocated here.
    want_dx=False (and no dx given): the parts alone, dx is neither allocated nor written and None is returned for it."""
    _req(dy, "dy", torch.bfloat16)
    _req(pooled, "pooled", torch.float32)
    _req(mean, "mean", torch.float32)
    _req(rstd, "rstd", torch.float32)
    _req(w, "w", torch.bfloat16)
    B, H = dy.shape
    assert tuple(pooled.shape) == (B, H) and mean.numel() == B and rstd.numel() == B
    if dx is None and want_dx:
        dx = torch.empty(B, S, H, dtype=torch.bfloat16, device=dy.device)
    ldg, bsg = H, S * H
    if dx is not None:
        Bx, Sx, Hx, ldg, bsg = _token_pool_view(dx, "dx")
        assert (Bx, Sx, Hx) == (B, S, H), "dx must be [B, S, H]"
    if want_parts and dw_part is None and db_part is None:
        dw_part, db_part = torch.empty(2, H, dtype=torch.float32, device=dy.device).unbind(0)
    _req(dw_part, "dw_part", torch.float32)
    _req(db_part, "db_part", torch.float32)
    _check(lib().op_token_mean_ln_bwd(ptr(dy), ptr(pooled), ptr(w), ptr(mean), ptr(rstd), ptr(dx), ldg, bsg, ptr(dw_part), ptr(db_part),
                                      B, S, H, stream()), "op_token_mean_ln_bwd")
    return dx, dw_part, db_part


ATTN_FRAMES_MAX_T = 32  # csrc/frameattn.hip: one lane per (head, frame), at most 32 frames


def _frames_cols(t, H, name):
    """Row stride of a [R, H] bf16 view as op_attn_frames_* take it (a column block of a wider matrix is fine)."""
    if not t.is_cuda or t.dtype != torch.bfloat16 or t.dim() != 2 or t.shape[1] != H or (H > 1 and t.stride(1) != 1):
        raise RuntimeError("attn_frames: %s must be a bf16 CUDA(HIP) tensor [R, heads * 64] with unit column stride" % name)
    return t.stride(0) if t.shape[0] > 1 else max(t.stride(0), H)


def attn_frames_supported(qkv, B, T, N, heads, hd):
    """The limits of op_attn_frames_fwd / _bwd for a packed q|k|v matrix [B * T * N, 3 * heads * hd]."""
    H = heads * hd
    if qkv.dim() != 2 or not qkv.is_cuda or qkv.dtype != torch.bfloat16 or tuple(qkv.shape) != (B * T * N, 3 * H):
        return False
    ld = qkv.stride(0) if qkv.shape[0] > 1 else max(qkv.stride(0), 3 * H)
    return (hd == 64 and 1 <= T <= ATTN_FRAMES_MAX_T and N >= 1 and heads >= 1 and B >= 1 and B * N * heads < 2 ** 31
            and qkv.stride(1) == 1 and ld % 8 == 0 and ld >= 3 * H and qkv.data_ptr() % 16 == 0)


def attn_frames_fwd(q, k, v, B, T, N, heads, scale, out=None):
    """op_attn_frames_fwd: q, k, v bf16 [B * T * N, heads * 64] views sharing one row stride (the column blocks of a packed projection
    output), rows ordered (b, t, n).  Returns out bf16 [B * T * N, heads * 64] (own row stride when given)."""
    H = heads * 64
    ld = _frames_cols(q, H, "q")
    if _frames_cols(k, H, "k") != ld or _frames_cols(v, H, "v") != ld or not (q.shape[0] == k.shape[0] == v.shape[0] == B * T * N):
        raise RuntimeError("attn_frames_fwd: q, k, v must share the row stride and have B * T * N = %d rows" % (B * T * N))
    if out is None:
        out = torch.empty(B * T * N, H, dtype=torch.bfloat16, device=q.device)
    ldo = _frames_cols(out, H, "out")
    assert out.shape[0] == B * T * N
    _check(lib().op_attn_frames_fwd(ptr(q), ptr(k), ptr(v), ld, ptr(out), ldo, B, T, N, heads, 64, scale, stream()), "op_attn_frames_fwd")
    return out


def attn_frames_bwd(q, k, v, dout, B, T, N, heads, scale, dqkv=None):
    """op_attn_frames_bwd: returns dqkv bf16 [B * T * N, 3 H], dq | dk | dv packed like a fused projection output (every element
    written).  p is recomputed from q and k: the forward's output is not needed."""
    H = heads * 64
    ld = _frames_cols(q, H, "q")
    if _frames_cols(k, H, "k") != ld or _frames_cols(v, H, "v") != ld or not (q.shape[0] == k.shape[0] == v.shape[0] == B * T * N):
        raise RuntimeError("attn_frames_bwd: q, k, v must share the row stride and have B * T * N = %d rows" % (B * T * N))
    ldo = _frames_cols(dout, H, "dout")
    assert dout.shape[0] == B * T * N
    if dqkv is None:
        dqkv = torch.empty(B * T * N, 3 * H, dtype=torch.bfloat16, device=q.device)
    assert dqkv.dim() == 2 and tuple(dqkv.shape) == (B * T * N, 3 * H)
    dq, dk, dv = dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:]
    ldg = _frames_cols(dq, H, "dq")
    _check(lib().op_attn_frames_bwd(ptr(q), ptr(k), ptr(v), ld, ptr(dout), ldo, ptr(dq), ptr(dk), ptr(dv), ldg, B, T, N, heads, 64, scale,
                                    stream()), "op_attn_frames_bwd")
    return dqkv


ATTN_WINDOW = 16  # csrc/windowattn.hip: 16 x 16 windows, 256 keys of 64 dims


def attn_window_supported(qkv, B, Hg, Wg, heads, hd, window=ATTN_WINDOW):
    """The limits of op_attn_window_fwd / _bwd for a packed q|k|v matrix [B * Hg * Wg, 3 * heads * hd]."""
    H = heads * hd
    if qkv.dim() != 2 or not qkv.is_cuda or qkv.dtype != torch.bfloat16 or tuple(qkv.shape) != (B * Hg * Wg, 3 * H):
        return False
    ld = qkv.stride(0) if qkv.shape[0] > 1 else max(qkv.stride(0), 3 * H)
    return (hd == 64 and window == ATTN_WINDOW and Hg >= 16 and Wg >= 16 and Hg % 16 == 0 and Wg % 16 == 0 and heads >= 1 and B >= 1
            and B * (Hg // 16) * (Wg // 16) * heads < 2 ** 31 and qkv.stride(1) == 1 and ld % 8 == 0 and ld >= 3 * H
            and qkv.data_ptr() % 16 == 0)


def attn_window_parts(B, Hg, Wg, heads):
    """(parts, slabs) of op_attn_window_bwd: the leading sizes of drel_part [parts, 2, 31, 64] and dbias_slabs [slabs, heads, 256, 256]."""
    parts, slabs = ctypes.c_int64(0), ctypes.c_int64(0)
    _check(lib().op_attn_window_parts(B, (Hg // 16) * (Wg // 16), heads, ctypes.byref(parts), ctypes.byref(slabs)), "op_attn_window_parts")
    return parts.value, slabs.value


def _window_tables(bias, rel_h, rel_w, heads, what):
    if bias is not None and (not bias.is_cuda or bias.dtype != torch.bfloat16 or tuple(bias.shape) != (heads, 256, 256)
                             or not bias.is_contiguous()):
        raise RuntimeError("%s: bias must be a contiguous bf16 CUDA(HIP) tensor [heads, 256, 256]" % what)
    if (rel_h is None) != (rel_w is None):
        raise RuntimeError("%s: rel_h and rel_w must be given together" % what)
    for t in (rel_h, rel_w):
        if t is not None and (not t.is_cuda or t.dtype != torch.bfloat16 or tuple(t.shape) != (31, 64) or not t.is_contiguous()):
            raise RuntimeError("%s: rel_h and rel_w must be contiguous bf16 CUDA(HIP) tensors [31, 64]" % what)


def attn_window_fwd(q, k, v, bias, rel_h, rel_w, B, Hg, Wg, heads, scale, out=None):
    """op_attn_window_fwd: q, k, v bf16 [B * Hg * Wg, heads * 64] views sharing one row stride (the column blocks of a packed projection
    output), rows ordered (b, y, x); bias bf16 [heads, 256, 256] or None; rel_h, rel_w bf16 [31, 64] or None together.  Returns out bf16
    [B * Hg * Wg, heads * 64] (own row stride when given)."""
    H, R = heads * 64, B * Hg * Wg
    ld = _frames_cols(q, H, "q")
    if _frames_cols(k, H, "k") != ld or _frames_cols(v, H, "v") != ld or not (q.shape[0] == k.shape[0] == v.shape[0] == R):
        raise RuntimeError("attn_window_fwd: q, k, v must share the row stride and have B * Hg * Wg = %d rows" % R)
    _window_tables(bias, rel_h, rel_w, heads, "attn_window_fwd")
    if out is None:
        out = torch.empty(R, H, dtype=torch.bfloat16, device=q.device)
    ldo = _frames_cols(out, H, "out")
    assert out.shape[0] == R
    _check(lib().op_attn_window_fwd(ptr(q), ptr(k), ptr(v), ld, ptr(bias), ptr(rel_h), ptr(rel_w), ptr(out), ldo, B, Hg, Wg, heads, 64,
                                    ATTN_WINDOW, scale, stream()), "op_attn_window_fwd")
    return out


def attn_window_bwd(q, k, v, bias, rel_h, rel_w, dout, B, Hg, Wg, heads, scale, dqkv=None, drel_part=None, dbias_slabs=None,
                    want_drel=False, want_dbias=False):
    """op_attn_window_bwd: returns (dqkv, drel_part, dbias_slabs).  dqkv bf16 [R, 3 H], dq | dk | dv packed like a fused projection
    output (every element written).  drel_part fp32 [parts, 2, 31, 64] and dbias_slabs fp32 [slabs, heads, 256, 256] are computed when
    given or asked for (want_*), else None; the caller sums them over the leading axis.  s and p are recomputed: the forward's output is
    not needed."""
    H, R = heads * 64, B * Hg * Wg
    ld = _frames_cols(q, H, "q")
    if _frames_cols(k, H, "k") != ld or _frames_cols(v, H, "v") != ld or not (q.shape[0] == k.shape[0] == v.shape[0] == R):
        raise RuntimeError("attn_window_bwd: q, k, v must share the row stride and have B * Hg * Wg = %d rows" % R)
    _window_tables(bias, rel_h, rel_w, heads, "attn_window_bwd")
    ldo = _frames_cols(dout, H, "dout")
    assert dout.shape[0] == R
    if dqkv is None:
        dqkv = torch.empty(R, 3 * H, dtype=torch.bfloat16, device=q.device)
    assert dqkv.dim() == 2 and tuple(dqkv.shape) == (R, 3 * H)
    dq, dk, dv = dqkv[:, :H], dqkv[:, H:2 * H], dqkv[:, 2 * H:]
    ldg = _frames_cols(dq, H, "dq")
    if want_drel or want_dbias or drel_part is not None or dbias_slabs is not None:   # (the counts are needed for nothing else)
        parts, slabs = attn_window_parts(B, Hg, Wg, heads)
    if drel_part is None and want_drel:
        drel_part = torch.empty(parts, 2, 31, 64, dtype=torch.float32, device=q.device)
    if dbias_slabs is None and want_dbias:
        dbias_slabs = torch.empty(slabs, heads, 256, 256, dtype=torch.float32, device=q.device)
    if drel_part is not None:
        _req(drel_part, "drel_part", torch.float32)
        assert tuple(drel_part.shape) == (parts, 2, 31, 64) and drel_part.is_contiguous()
    if dbias_slabs is not None:
        _req(dbias_slabs, "dbias_slabs", torch.float32)
        assert tuple(dbias_slabs.shape) == (slabs, heads, 256, 256) and dbias_slabs.is_contiguous()
    _check(lib().op_attn_window_bwd(ptr(q), ptr(k), ptr(v), ld, ptr(bias), ptr(rel_h), ptr(rel_w), ptr(dout), ldo, ptr(dq), ptr(dk), ptr(dv),
                                    ldg, ptr(drel_part), ptr(dbias_slabs), B, Hg, Wg, heads, 64, ATTN_WINDOW, scale, stream()),
           "op_attn_window_bwd")
    return dqkv, drel_part, dbias_slabs


MASK_MAX_ITEMS = 4096  # csrc/masks.hip: MK_MAX, the items (positions without CLS) of one row


def _check_mask(rc, what):
    if rc == -22:  # OP_EINVAL: a bad argument of the caller
        msg = lib().op_last_error()
        raise ValueError(msg.decode() if msg else what)
    _check(rc, what)


def _mask_out(out, i, shape, dtype, device, name):
    t = None if out is None else out[i]
    if t is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _req(t, name, dtype)
    if tuple(t.shape) != tuple(shape):
        raise ValueError("%s: need shape %s, got %s" % (name, tuple(shape), tuple(t.shape)))
    return t


def mask_patches(keys_a, m1, keys_b=None, extra=0, out=None):
    """op_mask_patches.  keys_a (and keys_b, for the vl mask) int32 [B, N] (contiguous, CUDA).  Returns (mask bool [B, N + 1],
    ids int64 [B, N + 1 - m1], vl_mask bool [B, N + 1] or None, vl_ids int64 [B, m1 - extra + 1] or None).  out: a 4-tuple of tensors to
    write into (entries may be None)."""
    _req(keys_a, "keys_a", torch.int32)
    _req(keys_b, "keys_b", torch.int32)
    if keys_a.dim() != 2 or (keys_b is not None and keys_b.shape != keys_a.shape):
        raise ValueError("mask_patches: need keys_a [B, N] and keys_b of the same shape")
    B, N = keys_a.shape
    m1, extra = int(m1), int(extra)
    if not 0 <= m1 <= N or (keys_b is not None and not 0 <= extra <= m1):
        raise ValueError("mask_patches: need 0 <= extra <= m1 <= N, got extra %d, m1 %d, N %d" % (extra, m1, N))
    dev, vl = keys_a.device, keys_b is not None
    with torch.cuda.device(dev):
        mask = _mask_out(out, 0, (B, N + 1), torch.bool, dev, "mask")
        ids = _mask_out(out, 1, (B, N + 1 - m1), torch.int64, dev, "ids")
        vl_mask = _mask_out(out, 2, (B, N + 1), torch.bool, dev, "vl_mask") if vl else None
        vl_ids = _mask_out(out, 3, (B, m1 - extra + 1), torch.int64, dev, "vl_ids") if vl else None
        _check_mask(lib().op_mask_patches(ptr(keys_a), ptr(keys_b), B, N, m1, extra, ptr(mask), ptr(ids), ptr(vl_mask), ptr(vl_ids), stream()),
                    "op_mask_patches")
    return mask, ids, vl_mask, vl_ids


def mask_words(src_tokens, table, keys_a, p, keys_b=None, vl_ratio=0.0, pad=1, width=None, vl_width=None, out=None):
    """op_mask_words.  src_tokens int64 [B, L] (rows may be strided), table uint8 [vocab], keys_a / keys_b int32 [B, L] (CUDA).
    width / vl_width: the columns of the ids, None = L + 1 (every row fits).  Returns (mask bool [B, L + 1], ids int64 [B, width],
    vl_mask, vl_ids (None without keys_b), counts int32 [2, B]: the kept positions of each row, which may exceed the width given: the ids
    of such a row are truncated).  Nothing is synchronised.  out: a 5-tuple of tensors to write into (entries may be None)."""
    _req(table, "table", torch.uint8)
    _req(keys_a, "keys_a", torch.int32)
    _req(keys_b, "keys_b", torch.int32)
    if not src_tokens.is_cuda or src_tokens.dtype != torch.int64 or src_tokens.dim() != 2 or (src_tokens.shape[1] > 1 and src_tokens.stride(1) != 1):
        raise ValueError("mask_words: src_tokens must be a CUDA int64 [B, L] tensor with unit column stride")
    B, L = src_tokens.shape
    if tuple(keys_a.shape) != (B, L) or (keys_b is not None and tuple(keys_b.shape) != (B, L)):
        raise ValueError("mask_words: keys must have the shape of src_tokens, %s" % ((B, L),))
    ld = src_tokens.stride(0) if B > 1 else L
    dev, vl = src_tokens.device, keys_b is not None
    width = L + 1 if width is None else int(width)
    vl_width = L + 1 if vl_width is None else int(vl_width)
    with torch.cuda.device(dev):
        mask = _mask_out(out, 0, (B, L + 1), torch.bool, dev, "mask")
        ids = _mask_out(out, 1, (B, width), torch.int64, dev, "ids")
        vl_mask = _mask_out(out, 2, (B, L + 1), torch.bool, dev, "vl_mask") if vl else None
        vl_ids = _mask_out(out, 3, (B, vl_width), torch.int64, dev, "vl_ids") if vl else None
        counts = _mask_out(out, 4, (2, B), torch.int32, dev, "counts")
        _check_mask(lib().op_mask_words(ptr(src_tokens), ld, B, L, int(pad), ptr(table), table.numel(), ptr(keys_a), ptr(keys_b), float(p),
                                        float(vl_ratio), ptr(mask), ptr(ids), width, ptr(vl_mask), ptr(vl_ids), vl_width if vl else 0,
                                        ptr(counts), stream()), "op_mask_words")
    return mask, ids, vl_mask, vl_ids, counts


def mask_blocks(rows, centers, keys, length, width=None, out=None):
    """op_mask_blocks.  rows: a host int32 [B, 3] array of (T, K, target) per clip; centers int32 [B, Kmax], keys int32 [B, Tmax] (CUDA).
    width: the columns of the ids, None = max(T + 1 - target).  Returns (mask bool [B, Tmax + 1], ids int64 [B, width]).  The table goes
    to the device in one copy.  out: a 2-tuple of tensors to write into."""
    import numpy as np
    _req(centers, "centers", torch.int32)
    _req(keys, "keys", torch.int32)
    if keys.dim() != 2 or centers.dim() != 2 or centers.shape[0] != keys.shape[0]:
        raise ValueError("mask_blocks: need centers [B, Kmax] and keys [B, Tmax]")
    B, Tmax = keys.shape
    Kmax = centers.shape[1]
    rows = np.ascontiguousarray(np.asarray(rows, dtype=np.int32).reshape(B, 3))
    if width is None:
        width = int((rows[:, 0] + 1 - rows[:, 2]).max()) if B else 1
    dev = keys.device
    with torch.cuda.device(dev):
        mask = _mask_out(out, 0, (B, Tmax + 1), torch.bool, dev, "mask")
        ids = _mask_out(out, 1, (B, int(width)), torch.int64, dev, "ids")
        rows_dev = torch.from_numpy(rows).to(dev)
        _check_mask(lib().op_mask_blocks(ptr(rows_dev), rows.ctypes.data_as(c_void_p), ptr(centers) if Kmax else None, Kmax, ptr(keys), Tmax, B,
                                         int(length), ptr(mask), ptr(ids), int(width), stream()), "op_mask_blocks")
    return mask, ids


def mfma_rate_probe(seconds=1.0, waves_per_cu=8, data="normal", device=None):
    """The bf16 MFMA rate this GPU sustains with nothing else going on (op_probe_mfma_rate: register operands only), after the
    package has settled at its power limit: {"tflops", "mhz" (shader clock over the loop, mean / min / max), "ms", "workgroups"}.
    `data`: "normal" (random normal operands, what a training step multiplies), "zeros" (no toggling: the clock stays at its maximum)."""
    device = device or torch.device("cuda", torch.cuda.current_device())
    cus = torch.cuda.get_device_properties(device).multi_processor_count
    wgs = cus * max(1, (int(waves_per_cu) + 3) // 4)
    g = torch.Generator().manual_seed(1)
    img = (torch.randn(8 * 64 * 8, generator=g) * 0.5 if data == "normal" else torch.zeros(8 * 64 * 8)).to(device=device, dtype=torch.bfloat16)
    out = torch.empty(wgs * 256, dtype=torch.float32, device=device)
    clk = torch.zeros(wgs * 2, dtype=torch.int64, device=device)
    iters, ms = 20000, 0.0
    for leg in range(3):  # calibrate, settle (clock and power follow the load with a delay), report
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(device))
        _check_probe(probe_lib().op_probe_mfma_rate(ptr(img), ptr(out), ptr(clk), wgs, iters, stream()), "op_probe_mfma_rate")
        e1.record(torch.cuda.current_stream(device))
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if leg == 0:
            iters = max(1, int(iters * seconds * 1e3 / ms))
    c = clk.view(wgs, 2).double().cpu()
    mhz = c[:, 0] / (c[:, 1] * 0.01)
    return {"tflops": wgs * 4 * iters * 64 * 16384.0 / (ms * 1e-3) / 1e12, "ms": ms, "workgroups": wgs,
            "mhz": {"mean": float(mhz.mean()), "min": float(mhz.min()), "max": float(mhz.max())}}
