/* onepeace_hip.h -- C ABI of libonepeace_hip.so: the ONE-PEACE hot path as hand-written HIP for MI355X (gfx950).
 *
 * The reference (OFA-Sys/ONE-PEACE @ 2024-10-08) has no FFI of its own: its "operator API" is three import-time seams
 * in Python.  This header is the boundary a binding for those seams talks to; every entry point
 * names the reference code it replaces (file:line relative to the reference tree).  The Python binding that ships
 * here is one-peace_amd/hip.py (ctypes); INTEGRATION.md shows the reference-side stubs.
 *
 * Contract (all functions):
 *   - plain pointers + sizes, no framework types.  Pointers are DEVICE pointers unless stated otherwise.
 *   - the caller owns every buffer (inputs, outputs, workspaces); the library never allocates, frees or keeps a
 *     pointer past the call.
 *   - work is enqueued asynchronously on `stream` (a hipStream_t passed as void*); no internal synchronisation.
 *     Stateless and re-entrant: no tuning knobs or caches live in the library (kernel flavours are selected by the per-call
 *     `tune` word of the GEMM / attention entry points, 0 = production defaults); safe from the Python main thread,
 *     autograd's backward thread and recompute.  The only process-wide state is the opt-in launch profiler (op_prof_*:
 *     mutex-protected event log, off by default) and hipFuncSetAttribute bookkeeping (idempotent).
 *   - return 0 on success, a negative errno-style code (-22 EINVAL, -95 ENOTSUP) or a positive hipError_t otherwise;
 *     never throws, never aborts.  op_last_error() gives the thread-local message.
 *   - dtype codes: 0 = bf16, 1 = f32.  Matrices are row-major; `ld*` are row strides in ELEMENTS.
 */
#ifndef ONEPEACE_HIP_H
#define ONEPEACE_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- library ------------------------------------------------------------------------------------------------ */
int op_abi_version(void); /* 2: per-call `tune` words replaced the process-wide knob setters; 3: op_gemm_nt_grouped, op_ln_geglu_fwd, ldd / ldh of op_ln_geglu_bwd, `out` of op_attn_bwd; 4: op_gemm_tn_grouped; 5: op_probe_mfma_rate, op_rows_gather / op_rows_merge, 16-byte rule of op_gemm_tn_grouped's C; 6: the op_probe_* entry points left for libonepeace_probe.so (include/onepeace_probe.h), op_gemm_nt_grouped answers OP_ENOTSUP for the GeGLU epilogue, op_gemm_tn_grouped_plan takes the workgroup count and tune word; 7: W / ldw / rowdot of op_gemm_tn_grouped, g0 of op_resid_bwd, op_gamma_grad_finish, op_gemm_nt_batched, op_audio_conv1_ln_gelu_fwd / _bwd; 8: the layer-scale gradient without a division -- rscale of op_gemm_tn_grouped, op_transpose_scaled + the scale member of the op_transpose_batched descriptor, op_resid_bwd leaves gamma out of dbranch when g0 is asked for, op_gamma_grad_finish lost its gamma argument; rowdot is a [N / 128][M] matrix of partial sums written once each (no atomics); 9: row tables -- a residual branch that runs on the samples stochastic depth keeps reads and writes the FULL activation matrix through op_rows_map's table instead of through packed copies: x_rows of op_layernorm_fwd / op_layernorm_bwd, dout_rows of op_resid_bwd, resid_rows / resid_rows_total of op_gemm_nt and op_gemm_nt_grouped, op_rows_merge without `upd` copies the dropped samples' rows only; op_prof_reserve; 10: run-to-run identical gradients -- op_relpos_bias_bwd sums the table gradient in a fixed order from pair lists instead of scattering with atomics, op_relpos_bias_bwd_ids became op_relpos_bias_fold_ids, the separate dBias kernel of op_attn_bwd adds into one slab per batch chunk; (still 10, additive) op_live_ktiles + op_gemm_tn_grouped_lists: the weight gradients skip the K-tiles of samples stochastic depth dropped; (still 10, additive) op_live_mwindows + op_gemm_nt_grouped_windows: the input gradients skip their row blocks; (still 10, additive) op_live_mwindows_fwd + op_gemm_nt_grouped_windows_fwd: the forward GEMMs of a residual branch skip them too; (still 10, additive) op_ln_geglu_fwd_skip / op_ln_geglu_bwd_skip / op_layernorm_bwd_skip / op_resid_bwd_skip: the row kernels do not read the rows of dropped samples */
const char* op_last_error(void);

/* Live per-kernel-family timing with HIP events recorded on the launch stream (used by bench.py's `roofline`).
 * family 0 = GEMM (work = flops), 1 = attention forward, 2 = attention backward.  HOST pointers. */
int op_prof_enable(int on);
int op_prof_reserve(int events); /* pre-creates events (two per profiled launch; created without the system-scope fence) */
int op_prof_collect(double* ms, int64_t* count, double* work, int n_families);

/* ---- LayerNorm (+ optional fused exact-erf GELU) ---------------------------------------------------------------
 * Replaces one_peace/models/components.py:23-26,47-52 (torch.nn.LayerNorm / flash_attn layer_norm seam) for
 * self_attn_layer_norm, self_attn.ln (sub-LN), final_layer_norm, the FFN LN(F) (transformer_layer.py:154), the
 * per-modality final norms (transformer_encoder.py:201-220), and with act_gelu=1 the LayerNorm->GELU pairs of the
 * stems (adapter/image.py:66-75, adapter/audio.py:293-301).  x,y [rows, cols] contiguous; w,b [cols] or NULL;
 * mean,rstd fp32 [rows] (NULL = not wanted).  cols % 8 == 0, cols <= 8192. */
/* (ABI 9) x_rows: nullable DEVICE int32 [rows] (op_rows_map): row r of the input is row x_rows[r] of a LARGER matrix x; an entry < 0
 * stands for a row of zeros (the surplus rows of a rounded-up segment).  y / mean / rstd are indexed by r. */
int op_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd, int64_t rows,
                     int64_t cols, float eps, int act_gelu, int dtype, const int* x_rows, void* stream);
int64_t op_layernorm_bwd_workspace_bytes(int64_t rows, int64_t cols);
/* dx = LN backward (+ `add`: gradient arriving through the residual path, may be NULL, may alias dx);
 * dw, db [cols] optional (need `workspace`); accumulate != 0 adds into dw/db. */
int op_layernorm_bwd(const void* dy, const void* x, const void* w, const void* b, const float* mean, const float* rstd,
                     const void* add, void* dx, void* dw, void* db, void* workspace, int64_t rows, int64_t cols,
                     int act_gelu, int accumulate, int dtype, const int* x_rows, void* stream);
/* (ABI 9) x_rows as in op_layernorm_fwd: x, add AND dx are then rows x_rows[r] of larger matrices (dy, mean, rstd by r); rows with an
 * entry < 0 are not stored.  With dx == add (in place) the rows no entry names keep `add`: the gradient of the skip connection. */
/* (additive, ABI 10) op_layernorm_bwd (bf16, no GELU, no row table) without the rows of the samples stochastic depth dropped (ps /
 * rows_per_sample as in op_ln_geglu_fwd_skip): nothing of dy, x, mean, rstd is read for a row with ps == 0; dx gets +0 there, or the
 * bits of the `add` row (dx may be add); dw / db get no contribution.  Other rows, dw and db: op_layernorm_bwd's bits.  ps null:
 * op_layernorm_bwd.  rows < 2^31. */
int op_layernorm_bwd_skip(const void* dy, const void* x, const void* w, const float* mean, const float* rstd, const void* add, void* dx,
                          void* dw, void* db, void* workspace, int64_t rows, int64_t cols, int accumulate, const float* ps,
                          int64_t rows_per_sample, void* stream);

/* ---- bf16 MFMA GEMM  C[M,N] = A[M,K] . W[N,K]^T  with fused epilogues ---------------------------------------------
 * Replaces: q/k/v/out projections (multihead_attention.py:63-66,103-105,124; up to three weight segments of n_seg rows
 * per launch, k_proj has no bias), GeGLU (transformer_layer.py:54-67), Linear(F->H) (:156), fused_dropout_res
 * (transformer_layer.py:70-88), the similarity matmuls of the contrastive head (image_text_pretrain_loss.py:171-172),
 * text/image/audio_proj (one_peace_retrieval.py:110-121) and the hMLP patch convolutions (adapter/image.py:66-75).
 * epilogue 0: C(bf16) = acc + bias
 *          1: C(f32)  = alpha[0] * acc + bias             (alpha: device scalar or NULL)
 *          2: GeGLU:  C(bf16)[M,N] = gelu(A W0^T) * (A W1^T); B0 = wi_0, B1 = wi_1 ([N,K] each); h0/h1 (optional, both
 *             or none) receive the two pre-activations for the backward pass
 *          3: C(bf16) = resid + rowscale[m / rows_per_sample] * gamma[n] * (acc + bias[n]); gamma/rowscale NULL = 1;
 *             resid may alias C; h0 (optional) receives acc + bias.
 * K % 64 == 0, N % 8 == 0, lda/ldb % 8 == 0 (host pads otherwise: one-peace_amd/ops.py gemm_any); ldc % 8 == 0 for the bf16 outputs
 * (C, h0, h1 share it), ldc % 4 == 0 for epilogue 1: rows are stored in 16-byte pieces.  Anything else returns -22.
 * workspace (optional fp32 scratch): lets the launch planner split K over several workgroups for bias-free epilogue-0
 * launches with few output tiles and a long K (weight gradients); tile size (128^2 / 256^2) and the split are chosen
 * from a wave-quantisation model. */
int op_gemm_nt(const void* A, int64_t lda, const void* B0, const void* B1, const void* B2, int64_t ldb, int64_t n_seg,
               const void* bias0, const void* bias1, const void* bias2, void* C, int64_t ldc, void* h0, void* h1,
               const void* resid, int64_t ldr, const void* gamma, const float* rowscale, int64_t rows_per_sample,
               const float* alpha, int64_t M, int64_t N, int64_t K, int epilogue, void* workspace, int64_t workspace_bytes,
               int64_t tune, const int* resid_rows, int64_t resid_rows_total, void* stream);
/* (ABI 9) resid_rows: nullable DEVICE int32 [M] (op_rows_map), residual epilogue only: `resid` and `C` are the BASES of matrices of
 * resid_rows_total rows (each below 4 GiB), the residual is read from and the result written to row resid_rows[m]; rows with an entry
 * < 0 are computed and dropped.  h0 (the branch output) and rowscale stay indexed by m.  The packed rows of the samples a residual
 * branch keeps go straight back to their places (transformer_layer.py:78-88 without the products by zero). */
/* C[M,N] (bf16) = A^T B with A [K,M] (lda), B [K,N] (ldb) row-major bf16: the weight-gradient GEMM dW = dy^T x of
 * nn.Linear (autograd of components.py:29-34 users) straight from the activation matrices (transpose-read fragments,
 * no transposed copies).  K % 64 == 0, M/N/lda/ldb/ldc % 8 == 0, else returns -95 (use op_transpose + op_gemm_nt).
 * accumulate != 0: C += A^T B.  workspace: optional fp32 scratch enabling split-K. */
int op_gemm_tn(const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int64_t M, int64_t N, int64_t K,
               int accumulate, void* workspace, int64_t workspace_bytes, int64_t tune, void* stream);
/* Grouped form of op_gemm_nt: up to three problems C_p[M_p,N] = epilogue(A_p[M_p,K] . W_p[N,K]^T) that share N, K, the leading
 * dimensions and the epilogue (0 bias, 2 GeGLU, 3 residual) in ONE launch of the persistent 256x256 kernel -- replaces the three
 * per-modality FFN launches of an encoder layer (transformer_layer.py:203-226: text / image / audio rows go through their own
 * text_ffn / image_ffn / audio_ffn).  Every array argument is a HOST array: A, M, C, h0, h1, resid, gamma, rowscale,
 * rows_per_sample have nprob entries; B and bias have 2 * nprob ([2p] = the weight / its bias, [2p + 1] = wi_1 of a GeGLU problem).
 * h0 / h1 / resid / gamma / rowscale / bias (arrays or entries) may be NULL.  Results are bit-identical to nprob op_gemm_nt calls.
 * Needs N % 256 == 0 (GeGLU: % 128), K % 64 == 0, K >= 128, lda / ldb / ldc % 8 == 0, operands < 2 GiB; else returns -95. */
int op_gemm_nt_grouped(int64_t nprob, const void* const* A, const int64_t* M, int64_t lda, const void* const* B, int64_t ldb,
                       const void* const* bias, void* const* C, int64_t ldc, void* const* h0, void* const* h1,
                       const void* const* resid, int64_t ldr, const void* const* gamma, const float* const* rowscale,
                       const int64_t* rows_per_sample, int64_t N, int64_t K, int epilogue, int64_t tune, const int* const* resid_rows,
                       int64_t resid_rows_total, void* stream); /* resid_rows: nullable HOST array of nprob DEVICE tables, see op_gemm_nt */
/* (ABI 7) `batch` equally shaped products  C_z[M,N] = A_z[M,K] W_z[N,K]^T (+ bias_z[N])  with operands at constant element strides as ONE
 * launch (blockIdx.z = z; 128 x 128 tiles, no split-K): the per-group GEMMs of the audio adapter's grouped positional Conv1d over
 * strided patch views (one_peace/models/adapter/audio.py:57-84; each group alone fills half the chip).  bias nullable.  K % 64 == 0,
 * N / lda / ldb / ldc and every stride % 8 == 0. */
int op_gemm_nt_batched(const void* A, int64_t lda, int64_t stride_a, const void* W, int64_t ldb, int64_t stride_b, const void* bias,
                       int64_t stride_bias, void* C, int64_t ldc, int64_t stride_c, int64_t M, int64_t N, int64_t K, int64_t batch,
                       void* stream);
/* (ABI 7) First block of the audio feature extractor, fused and straight from the waveform (one_peace/models/adapter/audio.py:254-311,
 * ConvFeatureExtractionModel block 0: Conv1d(1 -> C, kernel 10, stride `stride`, optional bias) -> LayerNorm over channels -> GELU):
 *   y[r][c] = GELU(LN_C(bf16(sum_j w0[c][j] * wav[stride * r + j] (+ b0[c]))))        rows x C bf16, C <= 512, C % 8 == 0
 * mean / rstd [rows] fp32 are kept for the backward, which RECOMPUTES the row from its ten samples and returns the parameter gradients
 * (dw0 [C, 10], db0 [C], dlnw [C], dlnb [C]; bf16; nullable except dw0; overwritten or accumulated) -- the 2.1 GB convolution output
 * of the headline batch is never written, re-read or kept.  workspace: op_audio_conv1_ln_gelu_bwd_workspace_bytes(C).
 * rows = 0 (valid pointers): the forward writes nothing; the backward's sums over no rows are zero -- non-accumulating gradients are
 * cleared, accumulating ones stay; both return OP_OK. */
int op_audio_conv1_ln_gelu_fwd(const void* wav, int64_t stride, const void* w0, const void* b0, const void* lnw, const void* lnb, void* y,
                               float* mean, float* rstd, int64_t rows, int64_t C, float eps, void* stream);
int64_t op_audio_conv1_ln_gelu_bwd_workspace_bytes(int64_t C);
int op_audio_conv1_ln_gelu_bwd(const void* dy, const void* wav, int64_t stride, const void* w0, const void* b0, const void* lnw, const void* lnb,
                               const float* mean, const float* rstd, void* dw0, void* db0, void* dlnw, void* dlnb, void* workspace,
                               int64_t rows, int64_t C, int accumulate, void* stream);
/* Grouped form of op_gemm_tn: up to 16 weight-gradient GEMMs  C_i[M_i,N_i] (bf16, ldc_i) (+)= A_i^T B_i  with their own operands,
 * sizes, K_i and outputs as ONE persistent launch WITHOUT split-K: the tile list of all problems is walked by one workgroup per
 * CU (per-XCD queues of WAVES -- as many consecutive tiles of a problem's tile rectangle as the XCD has workgroups, all of one K, so
 * that what an XCD runs at the same time shares its operand panels through the L2; longest K first, work stealing), every output tile runs its whole K
 * and is written / accumulated exactly once -- no fp32 slabs, no fold kernel.  Replaces the weight-gradient launches autograd
 * makes per nn.Linear of an encoder layer (transformer_layer.py:165-228 backward: q|k|v, out_proj, wi_0|wi_1 and wo of every
 * modality FFN); per-tile results are bit-identical to an unsplit op_gemm_tn.  Every array argument is a HOST array of nprob
 * entries.  counters: op_gemm_tn_grouped_counter_bytes() bytes of device memory zeroed ONCE by the caller (the launch re-arms
 * it; one block per stream).  Shape rules per problem as op_gemm_tn (+ ldc % 8 == 0 and C_i 16-byte aligned: the gradient is read-modify-written in 16-byte pieces); returns -95 and launches nothing when a
 * problem does not qualify.  tune: bits 0-9 forced number of workgroups (0 = one per CU); bit 10: round 4's form of the queues
 * (waves of a multiple of six tiles, the odd workgroups of an XCD draw single tiles from the back; A/B timing). */
int64_t op_gemm_tn_grouped_counter_bytes(void);
/* Host-only (no GPU needed): the tile queues op_gemm_tn_grouped builds for these sizes, `workgroups` (0: one per CU; 256 without a
 * device) and `tune` -- records of four int32 (queue 0..7, problem index of the caller, tile row, tile column) queue by queue in
 * draw order; returns the record count (= the number of 256 x 256 output tiles, each exactly once) or -22 when `cap` records do
 * not suffice. */
int64_t op_gemm_tn_grouped_plan(int64_t nprob, const int64_t* M, const int64_t* N, const int64_t* K, int64_t workgroups, int64_t tune,
                                int32_t* out, int64_t cap);
/* (ABI 7) W / ldw / rowdot: nullable HOST arrays; for a problem with rowdot[i] != NULL (requires accumulate[i], M_i and N_i multiples
 * of 256, W_i [M_i, N_i] bf16 16-byte aligned, ldw_i % 8 == 0) the launch also WRITES the partial row dots
 *   rowdot_i[s][m] = sum_{n in [128 s, 128 s + 128)} W_i[m][n] * P_i[m][n],   s < N_i / 128,   rowdot_i: fp32 [N_i / 128][M_i]
 * (ABI 8: every entry stored exactly once -- no atomics, no zeroing, run-to-run identical; ABI 7 added into one [M_i] vector with fp32
 * atomics; P_i = THIS launch's fp32 product A_i^T B_i before it is rounded into C_i).
 * (ABI 8) rscale: nullable HOST array; rscale[i] != NULL (bf16 [M_i], only with rowdot[i]) makes the accumulation
 * C_i[m][:] += rscale_i[m] * P_i[m][:] while rowdot still sums W_i * the UNSCALED P_i.  With A = rowscale * dout, the output gradient
 * of a residual branch WITHOUT the layer scale (op_resid_bwd with g0), B = input of the branch's last Linear, W = that Linear's
 * weight and rscale = gamma:  C += the weight gradient gamma[n] * (A^T B)[n][:], and sum_s rowdot[s][n] = sum_k W[n][k] * (A^T B)[n][k] IS the
 * layer-scale gradient sum_rows rowscale * dout * (x W^T) (+ the bias term of op_gamma_grad_finish) -- for any gamma, including 0 --
 * and the branch output y never has to be written or kept (one_peace/models/transformer/transformer_layer.py:70-88). */
int op_gemm_tn_grouped(int64_t nprob, const void* const* A, const int64_t* lda, const void* const* B, const int64_t* ldb, void* const* C,
                       const int64_t* ldc, const int64_t* M, const int64_t* N, const int64_t* K, const int32_t* accumulate,
                       const void* const* W, const int64_t* ldw, float* const* rowdot, const void* const* rscale, void* counters,
                       int64_t tune, void* stream);
/* op_gemm_tn_grouped with live K-tile lists.  ktiles / n_ktiles: nullable HOST arrays of nprob nullable DEVICE pointers; a problem with
 * ktiles[i] != NULL (then n_ktiles[i] too) runs only the 64-row K-tiles ktiles[i][0 .. *n_ktiles[i]) -- ascending int32 tile indices
 * < K_i / 64, written on the device before the launch (op_live_ktiles), never read by the host -- instead of all K_i / 64.  The rows of
 * A_i in the tiles left out must be zero (a residual branch's gradient rows of the samples stochastic depth dropped: op_resid_bwd
 * multiplied them by ps = 0): every fp32 accumulator starts at +0 and a +-0 product leaves it bit for bit what it was, so C_i and
 * rowdot_i equal those of the full launch -- unless B_i holds inf / NaN in such a row (0 * inf = NaN is then skipped, not computed).
 * An empty list leaves an accumulated C_i untouched and writes zeros otherwise; rowdot_i is written (zeros) either way.  A problem
 * without a list runs as in op_gemm_tn_grouped, which is this entry point with both arrays NULL.  Additive: op_abi_version() stays 10. */
int op_gemm_tn_grouped_lists(int64_t nprob, const void* const* A, const int64_t* lda, const void* const* B, const int64_t* ldb, void* const* C,
                             const int64_t* ldc, const int64_t* M, const int64_t* N, const int64_t* K, const int32_t* accumulate,
                             const void* const* W, const int64_t* ldw, float* const* rowdot, const void* const* rscale,
                             const int32_t* const* ktiles, const int32_t* const* n_ktiles, void* counters, int64_t tune, void* stream);
/* Live K-tile lists of up to 8 weight-gradient problems over ONE row matrix in one tiny launch, no host synchronisation.  Segments
 * (HOST arrays, nseg <= 4): rows [row0_i, row0_i + S_i * B_i) are B_i samples of S_i rows with DEVICE multipliers ps_i (fp32 [B_i];
 * NULL entry: all kept); rows of no segment belong to no sample.  Problems (HOST arrays, nprob <= 8): rows [prob_row0_p, prob_row0_p +
 * prob_rows_p), prob_rows_p % 64 == 0.  ktiles[p] (DEVICE int32 [prob_rows_p / 64]) receives, ascending and relative to prob_row0_p,
 * the indices of the 64-row tiles that hold a row of a sample with ps != 0; n_ktiles[p] (DEVICE int32) their number.
 * Additive: op_abi_version() stays 10. */
int op_live_ktiles(int64_t nseg, const float* const* ps, const int64_t* row0, const int64_t* S, const int64_t* B, int64_t nprob,
                   const int64_t* prob_row0, const int64_t* prob_rows, int32_t* const* ktiles, int32_t* const* n_ktiles, void* stream);
/* Window lists for the INPUT-gradient GEMMs of such a branch, and the zero rows those launches leave out: one launch, no host
 * synchronisation.  Segments as in op_live_ktiles, plus ps_stride[i] (sample b has the multiplier ps_i[b * ps_stride[i]]: a per-row
 * vector serves with ps_stride = S) and wps[i]: > 0 -- every sample with ps != 0 is listed as wps[i] windows of 256
 * rows from its first row on (odd[i] != 0, for S = 256 n + 1: and the last row of EVERY sample in strided windows of 256 samples);
 * 0 -- the aligned 256-row tiles of the segment that hold a row of such a sample.  seg_list / seg_prob /
 * seg_base (HOST, nseg x 2): the up to two lists a segment feeds (-1: none), the problem index its entries carry there and the row
 * of the row matrix at which that problem's operand starts (<= row0_i); an entry is two words, prob << 28 | (row - base) and
 * rows << 16 | row stride.  windows[l] (DEVICE int32 [2 * max_windows[l]]) and n_windows[l] (DEVICE int32) for nlist <= 4 lists, filled segment by segment, ascending.  out (nout <= 4,
 * may be 0): bf16 matrices of out_rows[o] rows parallel to the row matrix (row stride out_ld[o], out_cols[o] columns, both % 8 == 0);
 * the rows of every sample / tile that is not listed are set to +0 in each of them.  Additive: op_abi_version() stays 10. */
int op_live_mwindows(int64_t nseg, const float* const* ps, const int64_t* ps_stride, const int64_t* row0, const int64_t* S, const int64_t* B,
                     const int64_t* wps, const int64_t* odd, const int64_t* seg_list, const int64_t* seg_prob, const int64_t* seg_base, int64_t nlist,
                     int32_t* const* windows,
                     int32_t* const* n_windows, const int64_t* max_windows, int64_t nout, void* const* out, const int64_t* out_ld,
                     const int64_t* out_cols, const int64_t* out_rows, void* stream);
/* op_gemm_nt_grouped's plain form (no bias) over a window list: computes the rows r, r + s, ... (n of them, n <= 256) of C_p for the
 * two-word entries (prob << 28 | r, n << 16 | s) of windows[0 .. *n_windows) (DEVICE int32 [2 * max_windows], 8-byte aligned, written on the device
 * before the launch -- op_live_mwindows --, never read by the host; max_windows sizes the grid) and writes no other row.  s = 1: r is
 * any row of the problem; blocks may overlap (the same bits twice) and may pass the problem's end (fetched as zeros, not stored).
 * s > 1 (<= max_row_stride, with max_row_stride * lda and * ldc < 2^23): one row of each of n consecutive s-row samples.  B: ONE weight per problem.  Every listed block has the bits
 * of the dense launch: same operands, same K order.  A non-finite operand in a row that is not listed is not multiplied (the dense
 * launch gives NaN there).  OP_ENOTSUP as op_gemm_nt_grouped.  Additive: op_abi_version() stays 10. */
int op_gemm_nt_grouped_windows(int64_t nprob, const void* const* A, const int64_t* M, int64_t lda, const void* const* B, int64_t ldb,
                               void* const* C, int64_t ldc, int64_t N, int64_t K, const int32_t* windows, const int32_t* n_windows,
                               int64_t max_windows, int64_t max_row_stride, int64_t tune, void* stream);
/* The same two for the FORWARD launches of a residual branch (q | k | v and out-proj + residual; wi_0 | wi_1 and down-projection +
 * residual), whose rows of dropped samples the epilogue or a later kernel multiplies by 0.  Additive: op_abi_version() stays 10.
 * op_live_mwindows_fwd: op_live_mwindows plus, per output, a source matrix out_src[o] (bf16, 16-byte aligned, row stride out_src_ld[o]
 * % 8 == 0, not the output itself; null: +0 as above) whose rows are COPIED into the rows no window covers: the residual output takes
 * the residual input, which is what the dense epilogue's fma(0, y, res) gives.  nout >= 1.
 * op_gemm_nt_grouped_windows_fwd: B / bias hold 3 entries per problem, the weights [n_seg, K] and bias vectors (may be null) of the
 * N / n_seg <= 3 column segments of its output (n_seg % 256 == 0).  epilogue 0: C = A W^T + b; epilogue 3: C = resid + rowscale[m /
 * rows_per_sample] * gamma * (A W^T + b), m the row inside its problem (of a strided window too; rows * rows_per_sample < 2^32);
 * resid (row stride ldr, max_row_stride * ldr < 2^23) / gamma / rowscale / rows_per_sample per problem as in op_gemm_nt_grouped; no
 * branch output, no row table.  A listed row has the bits of the dense launch, no other row is written. */
int op_live_mwindows_fwd(int64_t nseg, const float* const* ps, const int64_t* ps_stride, const int64_t* row0, const int64_t* S, const int64_t* B,
                         const int64_t* wps, const int64_t* odd, const int64_t* seg_list, const int64_t* seg_prob, const int64_t* seg_base,
                         int64_t nlist, int32_t* const* windows, int32_t* const* n_windows, const int64_t* max_windows, int64_t nout,
                         void* const* out, const int64_t* out_ld, const int64_t* out_cols, const int64_t* out_rows,
                         const void* const* out_src, const int64_t* out_src_ld, void* stream);
int op_gemm_nt_grouped_windows_fwd(int64_t nprob, const void* const* A, const int64_t* M, int64_t lda, const void* const* B, int64_t ldb,
                                   int64_t n_seg, const void* const* bias, void* const* C, int64_t ldc, const void* const* resid, int64_t ldr,
                                   const void* const* gamma, const float* const* rowscale, const int64_t* rows_per_sample, int64_t N,
                                   int64_t K, int epilogue, const int32_t* windows, const int32_t* n_windows, int64_t max_windows,
                                   int64_t max_row_stride, int64_t tune, void* stream);
/* `tune` (op_gemm_nt, op_gemm_tn, op_gemm_plan): per-call tuning word, 0 = what production uses.  The library keeps NO tuning
 * state, so every entry point is a pure function of its arguments; tests and tools select a kernel flavour with the call:
 * bits 0-1 tile (0 auto: a cost model picks 128x128 or 256x256 tiles, K-splits and the tail-rows split; 1 force 128x128;
 * 2 force 256x256); bits 2-3 flavour of the 256x256 NT kernel (0 auto, 1 BK = 32, 2 eight-wave full-line, 3 four-wave full-line); bits 4-6 tail-rows split (0 default, 1 off,
 * 3 whenever it saves a round, 4 always); bits 7-11 M-tiles per L2 group (0 auto); bits 12-14 timing ablations of the 256x256
 * kernel (tools; wrong results); bits 15-18 forced K-split count of small problems (tools); bit 19 register-staged operands
 * instead of LDS-DMA (global_load_lds); bits 20-22 kernel of the four-wave NT launches (0 auto, 1 / 3 one-tile workgroups with
 * that instruction schedule, 6 persistent workgroups, 7 the round-2 kernel; op_gemm_nt_grouped: persistent workgroups unless 7). */
/* Host-only query (no GPU needed): the launch decision op_gemm_nt takes for a dense, single-segment problem.
 * plan[0] = tile (128 | 256), plan[1] = K-splits, plan[2] = 1 if the epilogue runs in the split-K fold kernel,
 * plan[3] = leftover rows (M % 256) split off into a second, small launch (0 = none). */
int op_gemm_plan(int64_t M, int64_t N, int64_t K, int epilogue, int has_bias, int64_t workspace_bytes, int64_t tune, int* plan);

/* ---- fp8 (OCP e4m3) variant of the FFN GEMMs: BASELINE configs[4], explicit opt-in (csrc/fp8.hip) -------------------------
 * No reference counterpart (the reference trains in bf16/fp16, trainer.py:86-88); replaces, when the caller opts in, the
 * forward GEMMs of transformer_layer.py:54-67,149-157 and (round 6) the two input-gradient GEMMs of their backward (the weight
 * gradients stay bf16).  op_quant_fp8_rows: any cols % 8 == 0 (rows wider than 8192 columns are read twice).  Per-row quantisation (x ~= q * scale[row], q = e4m3 of x * 448 / amax_row),
 * fp32 accumulation on v_mfma_scale_f32_16x16x128_f8f6f4, dequantisation by scale_a[m] * scale_b[n] in the epilogue. */
int op_quant_fp8_rows(const void* x, int64_t ldx, void* q, int64_t ldq, float* scale, int64_t rows, int64_t cols, void* stream);
/* Round 5 (ABI 6): op_layernorm_fwd (bf16, no GELU) / op_ln_geglu_fwd that ALSO write their output row-quantised to fp8 e4m3 -- q8
 * [rows, cols] bytes, q8_scale [rows] fp32, bit-identical to op_quant_fp8_rows(y) -- so that the fp8 FFN forward needs no
 * quantisation pass of its own (transformer_layer.py:196-199: the sub-LayerNorm in front of the FFN; :149-157: LayerNorm(F)). */
int op_layernorm_fwd_q8(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd, void* q8, float* q8_scale,
                        int64_t rows, int64_t cols, float eps, void* stream);
int op_ln_geglu_fwd_q8(const void* h0, const void* h1, int64_t ldh, const void* w, const void* b, void* y, float* mean, float* rstd, void* q8,
                       float* q8_scale, int64_t rows, int64_t cols, float eps, void* stream);
/* epilogue 0: + bias; 2: GeGLU (B0 = wi_0, B1 = wi_1, scales sb0 / sb1, optional h0 / h1); 3: residual epilogue of op_gemm_nt.
 * A8 [M,K], B8 [N,K] fp8 bytes (row strides lda / ldb in bytes, multiples of 16); K % 128 == 0; C / h0 / h1 / resid bf16. */
int op_gemm_nt_fp8(const void* A8, int64_t lda, const float* sa, const void* B0, const void* B1, int64_t ldb, const float* sb0,
                   const float* sb1, const void* bias, void* C, int64_t ldc, void* h0, void* h1, const void* resid, int64_t ldr,
                   const void* gamma, const float* rowscale, int64_t rows_per_sample, int64_t M, int64_t N, int64_t K, int epilogue,
                   int64_t tune, void* stream);

/* ---- attention ---------------------------------------------------------------------------------------------------
 * Replaces multihead_attention.py:102-115 (bmm QK^T, += attn_mask, fp32 softmax, bmm PV) and the xformers seam
 * :79-101, plus the dense-bias assembly of transformer_encoder.py:144-162: bias is the per-table image
 * [heads][S][Spad] from op_relpos_bias_build, key padding a byte mask [B][Spad] (non-zero = masked key).
 * q,k,v: bf16 rows of `ld` elements, row = b*S + s, head h at columns [h*64, h*64+64) (a packed [B*S, 3H] projection
 * output serves all three).  out [B*S][ldo]; lse fp32 [B][heads][lse_ld] (natural log) or NULL.  head_dim == 64.
 * Spad >= S rounded up to 128 when bias/key_pad/backward are used.
 * bias_batch_stride: 0 = one bias image shared by all samples; otherwise elements between per-sample images
 * [B][heads][S][Spad] (masked pretraining gathers a different token subset per sample, adapter/image.py:229-246); the
 * backward then returns one dbias slab per sample.
 * bias_frag (optional): the same image(s) in the fragment-major layout of op_attn_bias_pack; with it (or without any
 * bias) sequences of up to 320 keys run the resident-K/V kernel, which adds the bias with the matrix pipe; a biased call
 * without bias_frag always runs the streaming kernel.
 * Preconditions the kernels do not check (tests/test_attention_fp64_gpu.py runs everything else against fp64): S >= 1 (every
 * row index is clamped to S - 1); bias entries inside [0, S) are FINITE -- keys are masked through key_pad, not with -inf in the
 * image (the matrix-pipe routes add the bias as a product with a selector, where 0 * inf would turn a whole query block into
 * NaN); every sample keeps at least one unmasked key (a row with all keys masked has no softmax: NaN, as in the reference). */
int op_attn_fwd(const void* q, const void* k, const void* v, int64_t ld, const void* bias, int64_t bias_batch_stride,
                const void* bias_frag, const void* key_pad, void* out, int64_t ldo, float* lse, int64_t lse_ld, int64_t B,
                int64_t S, int64_t Spad, int64_t heads, int64_t head_dim, float scale, int64_t tune, void* stream);
/* Fragment-major repack of n_img row-major bias images [n_img][S][Spad] (n_img = heads, or B * heads for per-sample
 * images): dst [n_img][ceil(S/16)][ceil(S/32)][64 lanes][8] bf16 = op_attn_bias_frag_elems(n_img, S) elements, zero
 * outside the sequence.  (No reference counterpart: the reference adds a dense [B, heads, S, S] tensor,
 * multihead_attention.py:107-108.) */
int64_t op_attn_bias_frag_elems(int64_t n_img, int64_t S);
int op_attn_bias_pack(const void* src, void* dst, int64_t n_img, int64_t S, int64_t Spad, void* stream);
/* delta[b][h][q] = sum_d dout*out (fp32, row stride Spad) */
int op_attn_bwd_delta(const void* dout, const void* out, int64_t ldo, float* delta, int64_t B, int64_t S, int64_t Spad,
                      int64_t heads, void* stream);
/* autograd of the above (reference: torch autograd through the bmm/softmax ops).  biasT = bias with rows = key; its pad
 * columns [S, Spad) must hold FINITE values (op_relpos_bias_build writes zeros): the dK/dV kernel adds the bias with the matrix
 * pipe, where 0 * NaN would leak into live rows.  lse / delta entries and the q-major image's columns at [S, Spad) stay
 * unspecified.  bias_frag (optional): op_attn_bias_pack of `bias`; with it the merged dQ + dBias kernel adds the bias with
 * the matrix pipe too.  dq/dk/dv rows have stride ldg; dbias fp32 [slabs][heads][S][Spad] (optional, accumulated into:
 * pre-zero it; the gradient is the sum over slabs, slabs = op_attn_bwd_dbias_slabs(B, S, heads, tune)). */
int64_t op_attn_bwd_dbias_slabs(int64_t B, int64_t S, int64_t heads, int64_t tune);
/* out (nullable): the forward output rows (same stride ldo as dout).  Given, `delta` is a WORKSPACE of the call: the dQ kernels
 * compute delta = rowsum(dout o out) per head from fragments they load anyway and the dK/dV kernel, launched behind them, reads
 * it -- op_attn_bwd_delta's pass over both matrices is not needed.  NULL: `delta` must hold op_attn_bwd_delta's result. */
int op_attn_bwd(const void* q, const void* k, const void* v, int64_t ld, const void* dout, const void* out, int64_t ldo,
                const void* bias, const void* biasT, const void* bias_frag, int64_t bias_batch_stride, const void* key_pad,
                const float* lse, float* delta, void* dq,
                void* dk, void* dv, int64_t ldg, float* dbias, int64_t B, int64_t S, int64_t Spad, int64_t heads,
                int64_t head_dim, float scale, int64_t tune, void* stream);

/* ---- relative-position bias tables -------------------------------------------------------------------------------
 * Replaces get_rel_pos_bias of adapter/image.py:164-171, adapter/text.py:76-83, adapter/audio.py:117-124:
 * out[h][i][j] = table[bucket[i][j]][h] (bf16 [heads][S][Spad], columns >= S zero); transposed != 0 -> out[h][j][i]. */
int op_relpos_bias_build(const void* table, const int* bucket, int64_t bucket_ld, void* out, int64_t heads, int64_t S,
                         int64_t Spad, int transposed, void* stream);
/* (ABI 10) dtable[r][h] = sum of dbias[h][i][j] (fp32 [heads][S][Spad]) over the positions with bucket[i][j] == r, summed in a fixed
 * order: the same bits every run.  pos: int32 i*S + j of every position, grouped by bucket (row-major within a bucket); seg: int32
 * [nseg + 1], segment t = pos[seg[t] .. seg[t+1]), each inside one bucket; bucket_seg: int32 [num_rel + 1], bucket r = segments
 * bucket_seg[r] .. bucket_seg[r+1].  partial_ws: fp32 [nseg][heads] workspace.  dtable fp32 [num_rel][heads] is overwritten. */
int op_relpos_bias_bwd(const float* dbias, int64_t S, int64_t Spad, const int* pos, const int* seg, int64_t nseg, const int* bucket_seg,
                       int64_t num_rel, float* partial_ws, float* dtable, int64_t heads, void* stream);
/* Per-sample images for the masked-pretraining passes (adapter/image.py:188-204,229-246, adapter/text.py, adapter/audio.py:
 * gather_features selects rows and columns preserve_ids[b] of the dense bias): out[b][h][i][j] = table[bucket[ids[b][i]][ids[b][j]]][h]
 * straight from the table -- out [B][heads][K][Kpad] bf16, pad columns zero; transposed != 0: rows = keys.  ids [B][K] int32
 * position ids (padding already mapped to a valid id, adapter/image.py:241-243; it is masked through key_pad).  The backward
 * (ABI 10: op_relpos_bias_fold_ids) folds the per-sample gradient slabs dbias [B][heads][K][Kpad] of op_attn_bwd into dense_ws (fp32
 * [heads][Sfull][Sfull], zeroed by the caller; Sfull = extent of the bucket table), which op_relpos_bias_bwd (S = Spad = Sfull) then
 * sums onto the table.  The fold adds with fp32 atomics: samples that share a position add in no fixed order. */
int op_relpos_bias_build_ids(const void* table, const int* bucket, int64_t bucket_ld, const int* ids, void* out, int64_t B,
                             int64_t heads, int64_t K, int64_t Kpad, int transposed, void* stream);
int op_relpos_bias_fold_ids(const float* dbias, const int* ids, float* dense_ws, int64_t Sfull, int64_t B, int64_t heads, int64_t K,
                            int64_t Kpad, void* stream);

/* ---- HBM-bound helpers of the layer backward -----------------------------------------------------------------------
 * (the reference gets these from autograd over transformer_layer.py:54-88,149-157) */
int op_transpose(const void* in, void* out, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out, void* stream);
/* (ABI 8) out[c][r] = bf16(scale[r] * in[r][c]); scale: bf16 [rows] or NULL (= op_transpose).  The input-gradient copy of the last
 * Linear of a residual branch with the layer scale folded in: dx = (rowscale * dout) . (gamma o W)
 * (one_peace/models/transformer/transformer_layer.py:70-88; the operand op_resid_bwd writes with g0 carries no gamma). */
int op_transpose_scaled(const void* in, void* out, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out, const void* scale,
                        void* stream);
/* Many transposes in one launch (the dgrad copies of all weights after an optimiser step).  table: DEVICE array of n
 * descriptors, op_transpose_desc_bytes() bytes each, laid out as { const void* in; void* out; int32 rows, cols;
 * int64 ld_in, ld_out; int32 tile0, tiles_x; const void* scale; } with tile0 = running sum of ceil(cols/64)*ceil(rows/64),
 * tiles_x = ceil(cols/64) and scale as in op_transpose_scaled (NULL = none); total_tiles = that sum over all descriptors. */
int op_transpose_batched(const void* table, int64_t n, int64_t total_tiles, void* stream);
int64_t op_transpose_desc_bytes(void);
int64_t op_colsum_workspace_bytes(int64_t N);
/* Per-segment column sums of x [M, n_seg*seg_cols]: the q/k/v bias gradients of the fused projection
 * (one_peace/models/transformer/multihead_attention.py:57-62; a null out_i skips that segment).  workspace: op_colsum_workspace_bytes(n_seg*seg_cols). */
int op_colsum_segments(const void* x, void* out0, void* out1, void* out2, void* workspace, int64_t M, int64_t n_seg,
                       int64_t seg_cols, int accumulate, void* stream);
/* Backward of out = resid + rowscale[m/rps] * gamma[n] * y[m][n] (layer-scale + drop-path residual,
 * one_peace/models/transformer/transformer_layer.py:70-88,190-196,224-226) in one pass:
 * dbranch = rowscale*gamma*dout; dgamma (+)= sum_m rowscale*dout*y; dbias (+)= sum_m rowscale*gamma*dout.  Nullable: y+dgamma, gamma,
 * rowscale, dbias, g0.  (ABI 7) g0 (fp32 [N], overwritten): sum_m rowscale*dout, i.e. dbias WITHOUT the gamma factor -- what
 * op_gamma_grad_finish multiplies with the last Linear's bias when dgamma is taken from the weight gradient instead of from y.
 * (ABI 8) With g0 != NULL (an alternative to y + dgamma) dbranch = rowscale*dout, WITHOUT gamma: the weight-gradient launch applies
 * gamma to its output rows (op_gemm_tn_grouped: rscale) and the input-gradient GEMM reads a gamma-scaled weight copy
 * (op_transpose_scaled), so that the layer-scale gradient needs no division by gamma.
 * M = 0 (valid pointers): the sums over no rows are zero -- g0 and the non-accumulating dgamma / dbias are cleared, nothing else is written. */
int64_t op_resid_bwd_workspace_bytes(int64_t N);
int op_resid_bwd(const void* dout, const void* y, const void* gamma, const float* rowscale, int64_t rows_per_sample,
                 void* dbranch, void* dgamma, void* dbias, float* g0, void* workspace, int64_t M, int64_t N, int accumulate,
                 const int* dout_rows, void* stream); /* (ABI 9) dout_rows: nullable DEVICE int32 [M]: row m of dout is row dout_rows[m] of a larger matrix (< 0: zeros); y / dbranch by m */
/* (additive, ABI 10) op_resid_bwd that reads the multiplier of a row first: where rowscale[m / rows_per_sample] == 0 nothing of
 * dout / y is loaded, dbranch gets +0 and the column sums no contribution.  Other rows and the sums: op_resid_bwd's bits. */
int op_resid_bwd_skip(const void* dout, const void* y, const void* gamma, const float* rowscale, int64_t rows_per_sample,
                      void* dbranch, void* dgamma, void* dbias, float* g0, void* workspace, int64_t M, int64_t N, int accumulate,
                      const int* dout_rows, void* stream);
/* (ABI 7; 8: no gamma argument, no division, partial slots instead of atomics) Layer-scale gradient of a residual branch
 * out = resid + rowscale * gamma * (x W^T + b)  WITHOUT the branch output:
 *   dgamma[n] (+)= sum_{s < slots} rowdot[s][n] + sum_i b_i[n] * g0_i[n]
 * rowdot: fp32 [slots][N], op_gemm_tn_grouped's partial row dots over the UNSCALED gradient of one or more weight sets laid out slot
 * after slot (sum_s = sum_k W[n][k] * ((rowscale*dout)^T x)[n][k]); folded in slot order: deterministic;
 * (b_i, g0_i): bias of the last Linear and op_resid_bwd's g0 for up to three weight sets that share gamma (the three modality FFNs of
 * a lock-step layer, transformer_layer.py:203-226; b_i NULL = no bias).  Exact for every gamma, 0 included (the reference:
 * transformer_layer.py:78-88).  dgamma: bf16 [N]. */
int op_gamma_grad_finish(const float* rowdot, int64_t slots, const void* b0, const float* g00, const void* b1, const float* g01,
                         const void* b2, const float* g02, void* dgamma, int64_t N, int accumulate, void* stream);
/* Backward of LayerNorm_F(gelu(h0) * h1) w.r.t. h0, h1 and the LayerNorm affine in one pass (the FFN's GeGLU + inner
 * sub-LayerNorm, transformer_layer.py:64-67,111-118); mean/rstd: forward statistics.  workspace: op_layernorm_bwd_workspace_bytes.
 * ldh: row stride of h0 / h1 (0 = cols).  ldd: row stride (elements) of dh0 / dh1, 0 = cols -- the two gradients may be the halves of one [rows, 2 * cols] matrix, which
 * is then ONE operand for the merged wi_0 | wi_1 weight-gradient and input-gradient GEMMs. */
int op_ln_geglu_bwd(const void* dy, const void* h0, const void* h1, const void* w, const float* mean, const float* rstd,
                    void* dh0, void* dh1, int64_t ldd, int64_t ldh, void* dw, void* db, void* workspace, int64_t rows,
                    int64_t cols, int accumulate, void* stream);
/* Forward of the same pair: y [rows, cols] = LayerNorm_F(bf16(gelu(h0) * h1)) with exact-erf GELU, + mean / rstd (nullable).
 * h0 / h1: row stride ldh (0 = cols) -- the halves of the [rows, 2 * cols] output of ONE plain two-segment up-projection GEMM
 * (wi_0 | wi_1).  Used by the training path instead of the GEMM's EPI_GEGLU epilogue: the erf costs the GEMM more than this
 * HBM-bound pass costs in total. */
int op_ln_geglu_fwd(const void* h0, const void* h1, int64_t ldh, const void* w, const void* b, void* y, float* mean, float* rstd,
                    int64_t rows, int64_t cols, float eps, void* stream);
/* (additive, ABI 10) The same pair without the rows of the samples stochastic depth dropped: row r belongs to sample
 * r / rows_per_sample (>= 1; 1 serves a per-row vector), ps: DEVICE fp32, one multiplier per sample.  Where ps[sample] == 0 nothing of
 * the row is read (h0 | h1, dy, mean and rstd may hold anything there, NaN included).  Forward: y gets +0 there; mean / rstd of the row
 * are not written.  Backward: dh0 | dh1 get +0 and dw / db no contribution -- what op_ln_geglu_bwd gives for an exact-zero dy row.
 * All other rows, and dw / db, have the plain entries' bits.  ps null: the plain entries.  rows < 2^31. */
int op_ln_geglu_fwd_skip(const void* h0, const void* h1, int64_t ldh, const void* w, const void* b, void* y, float* mean, float* rstd,
                         int64_t rows, int64_t cols, float eps, const float* ps, int64_t rows_per_sample, void* stream);
int op_ln_geglu_bwd_skip(const void* dy, const void* h0, const void* h1, const void* w, const float* mean, const float* rstd,
                         void* dh0, void* dh1, int64_t ldd, int64_t ldh, void* dw, void* db, void* workspace, int64_t rows,
                         int64_t cols, int accumulate, const float* ps, int64_t rows_per_sample, void* stream);
/* out[n] = (accumulate ? out[n] : 0) + mul[n] * sum_m rowscale[m/rps] * x[m][n] * (y ? y[m][n] : 1); y/rowscale/mul NULL ok */
int op_colsum(const void* x, const void* y, const float* rowscale, int64_t rows_per_sample, const void* mul, void* out,
              void* workspace, int64_t M, int64_t N, int accumulate, int out_dtype, void* stream);
/* GeGLU backward: dh0 = dg*h1*gelu'(h0), dh1 = dg*gelu(h0) */
int op_geglu_bwd(const void* dg, const void* h0, const void* h1, void* dh0, void* dh1, int64_t numel, void* stream);
/* dbranch[m][n] = rowscale[m/rps] * gamma[n] * dout[m][n]  (backward of fused_dropout_res wrt the branch) */
int op_scale_rows(const void* dout, const void* gamma, const float* rowscale, int64_t rows_per_sample, void* dbranch,
                  int64_t M, int64_t N, void* stream);

/* ---- contrastive head ----------------------------------------------------------------------------------------------
 * F.normalize(x, dim=1) of one_peace_retrieval.py:112,116,120 / one_peace_pretrain.py:165-173.  inv_norm[row] =
 * 1 / max(||x||, eps), negated where ||x|| < eps: the backward of such a row is dy / eps, as clamp_min gives. */
int op_l2norm_fwd(const void* x, void* y, float* inv_norm, int64_t rows, int64_t cols, float eps, int out_dtype, void* stream);
int op_l2norm_bwd(const void* dy, const void* y, const float* inv_norm, void* dx, int64_t rows, int64_t cols, int y_dtype,
                  void* stream);
/* compute_itc_loss / compute_atc_loss + adjust_label_smoothed_nll_loss (image_text_pretrain_loss.py:17-27,164-185;
 * audio_text_pretrain_loss.py:160-181): per row of sim [rows][n] (fp32): fp32 log-softmax, NLL at target0+row with the
 * reference's eps/(n-1) smoothing, argmax hit, <dsim, sim>; sim is overwritten by gscale * dloss_row/dsim. */
int op_infonce_rows(float* sim, int64_t rows, int64_t n, int64_t ld, int64_t target0, float label_smoothing, float gscale,
                    float* row_loss, float* row_hit, float* row_dot, int write_grad, void* stream);

/* ---- optimiser -------------------------------------------------------------------------------------------------------
 * One AdamW update over a flat bf16 parameter range, the rule of one_peace/optim/adam.py:186-253 (what the reference
 * runs without apex): fp32 moments, decoupled decay before the update, eps added to sqrt(v).  g is multiplied by
 * grad_scale inside the kernel (1/world after a SUM all-reduce).  numel % 8 == 0, step >= 1.  With grad_sqnorm and clip_norm > 0
 * the gradient is also multiplied by clamp(clip_norm / (|grad_scale| sqrt(*grad_sqnorm) + 1e-6), max = 1); a NaN sum of squares
 * makes every parameter and moment of the range NaN (nothing is stepped with the unclipped gradient), +inf gives coefficient 0. */
int op_adamw_step(void* p, const void* g, float* m, float* v, int64_t numel, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int64_t step, float grad_scale, const float* grad_sqnorm, float clip_norm,
                  void* stream);
/* The same update over a flat buffer partitioned into n_groups <= 256 contiguous parameter groups, ONE launch: the param groups
 * of trainer.py:265-278 / utils/layer_decay.py:34-77 ("layer_<id>_<decay|no_decay>" with lr_scale and weight_decay; lr_g = lr *
 * lr_scale_g as optim/base_optimizer.py:8-14 sets it).  group_end8[g] (device, ascending, int64) = end of group g in 8-element
 * vectors; group_lr_scale / group_weight_decay: device fp32 tables. */
int op_adamw_step_groups(void* p, const void* g, float* m, float* v, int64_t numel, const int64_t* group_end8,
                         const float* group_lr_scale, const float* group_weight_decay, int64_t n_groups, float lr, float beta1,
                         float beta2, float eps, int64_t step, float grad_scale, const float* grad_sqnorm, float clip_norm,
                         void* stream);
/* op_adamw_step_groups with an fp32 master copy of the parameters: the reference's `bf16: true` with `memory_efficient_bf16: false`,
 * where trainer.py:297-307 selects FP16Optimizer (one_peace/optim/fp16_optimizer.py).  There build_fp32_params makes a flat fp32
 * copy of the parameters, _sync_fp16_grads_to_fp32 widens the bf16 gradients, clip_grad_norm folds the clip coefficient into a
 * factor the fp32 gradients are multiplied by, step runs Adam on the fp32 copy and _sync_fp32_params_to_fp16 casts it back to
 * bf16.  Here: master (fp32 [numel], device) is read in the place of float(p), updated by the same expressions and stored; p
 * (bf16) is only WRITTEN, with the round-to-nearest-even bf16 of the master value just stored; m, v, g, the group tables, grad_scale
 * and the clip handling are those of op_adamw_step_groups.  28 B/param of traffic instead of 22, 4 B/param more memory.
 * Clip ordering: in this arrangement the reference itself scales FP32 gradients by the clip coefficient, so the in-kernel fp32
 * scaling is the reference's own order here -- not the deviation one-peace_amd/optim.py documents for the memory-efficient path
 * (where the reference rounds the clipped gradient to bf16 first).
 * Same argument checks as op_adamw_step_groups, and master != NULL.  Additive: op_abi_version() stays 10. */
int op_adamw_step_groups_master(void* p, float* master, const void* g, float* m, float* v, int64_t numel,
                                const int64_t* group_end8, const float* group_lr_scale, const float* group_weight_decay,
                                int64_t n_groups, float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale,
                                const float* grad_sqnorm, float clip_norm, void* stream);
/* One step of the exponential moving average of the weights, kept in fp32 (the reference's EMAModule with `ema_fp32: true`,
 * trainer.py:243-250 and :895-907; the averaging rule is fairseq/modules/ema_module.py:101-127): for every element
 *     ema = fmaf(take, float(p), fl32(keep * ema))        keep = float(decay), take = float(1.0 - decay)
 * with the product and the fma rounded separately -- bit for bit torch's `ema.mul_(decay); ema.add_(p.float(), alpha=1 - decay)`.
 * ema: fp32 [numel], read and written; p: bf16 [numel], only read.  keep = 0, take = 1 copies p (updates < ema_start_update).
 * numel % 8 == 0.  10 B/param.  Additive: op_abi_version() stays 10. */
int op_ema_step(float* ema, const void* p, int64_t numel, float keep, float take, void* stream);
/* op_adamw_step_groups (master == NULL) or op_adamw_step_groups_master (master != NULL), and op_ema_step on the parameters that
 * step stores, in ONE launch: p, master, m and v receive bit for bit what the unfused entry gives, ema what op_ema_step gives from
 * the new bf16 p (never from the master: the reference's EMA reads the model).  30 B/param without the master, 36 with it, against
 * 22 + 10 and 28 + 10 for the pair.  Argument checks of op_adamw_step_groups, and ema != NULL; ema must not overlap master.
 * Additive: op_abi_version() stays 10. */
int op_adamw_step_groups_ema(void* p, float* master, const void* g, float* m, float* v, float* ema, int64_t numel,
                             const int64_t* group_end8, const float* group_lr_scale, const float* group_weight_decay,
                             int64_t n_groups, float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale,
                             const float* grad_sqnorm, float clip_norm, float ema_keep, float ema_take, void* stream);
/* The grouped step over ONE RANGE of the flat buffers: the optimiser state sharded over the data-parallel ranks, what the reference
 * runs with `use_distributed_fused_adam: true` (one_peace/optim/adam.py:58-70 -> optim/distributed_fused_adam.py: apex's
 * DistributedFusedAdam partitions the state, every rank updates its partition, the parameters are gathered afterwards).
 * p, g: bases of the FULL flat bf16 buffers of numel elements (numel % 8 == 0).  The vectors [first8, first8 + count8) are updated,
 * nothing else of p is touched and g is only read.  m, v, master, ema: fp32 buffers of the RANGE, 8 * count8 elements each, local
 * vector 0 = global vector first8; master and ema may each be NULL (the four arrangements of op_adamw_step_groups, _master and
 * _ema; ema_keep / ema_take are unused without ema).  group_end8 / group_lr_scale / group_weight_decay: the GLOBAL tables of
 * op_adamw_step_groups, unshifted.  grad_sqnorm: the sum of squares of the FULL gradient buffer.  Every element of the range
 * receives bit for bit what the whole-buffer entry of the same arrangement stores for it: the same kernel runs, with the range's
 * global start added to the vector index for the group lookup only.
 * Refused, with nothing launched: a null p, g, m, v or table; numel % 8 != 0; first8 < 0; count8 < 0; first8 + count8 > numel / 8;
 * n_groups outside 1..256; step < 1; ema overlapping master.  count8 == 0 returns OP_OK without a launch.
 * Additive: op_abi_version() stays 10. */
int op_adamw_step_shard(void* p, const void* g, int64_t numel, int64_t first8, int64_t count8, float* m, float* v, float* master,
                        float* ema, const int64_t* group_end8, const float* group_lr_scale, const float* group_weight_decay,
                        int64_t n_groups, float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale,
                        const float* grad_sqnorm, float clip_norm, float ema_keep, float ema_take, void* stream);
/* out[0] = sum of squares of a bf16 vector in fp32 (the global gradient norm of fairseq/fairseq/utils.py:349-391 over the
 * flat gradient buffer; feeds op_adamw_step's device-side clip coefficient, trainer.py:929).  workspace: 1024 floats. */
int op_sqnorm(const void* x, int64_t numel, float* workspace, float* out, void* stream);

/* ---- stochastic depth without the multiplications by zero ------------------------------------------------------------
 * The reference multiplies the branch output of a dropped sample by 0 (transformer_layer.py:78-88: fused_dropout_res).  These two
 * entries pack the rows of the samples a residual branch KEEPS into a smaller matrix (the branch then runs on that alone) and merge
 * its result back.  Per segment i < nseg (<= 4; a segment = the B samples x S tokens of one modality inside the packed activation
 * matrix), host arrays: src_row0 (first row in the full matrix), dst_row0 (first row in the packed matrix), S, n_kept, dst_rows
 * (>= n_kept * S, rounded up by the caller; the surplus rows are written as ZEROS so that they add nothing to a weight gradient),
 * n_samples, list_off (start of the segment's list inside `list`, a DEVICE int32 array).
 *   op_rows_gather: list = the kept sample numbers, ascending:  dst[dst_row0 + j*S + t] = src[src_row0 + list[j]*S + t].
 *   op_rows_merge:  list = per sample its position among the kept ones or -1:  out[r] = upd[dst_row0 + list[sample]*S + t] for
 *                   kept samples, base[r] otherwise; out may be base (then only the kept rows are written).
 * bf16 rows of `cols` elements (cols % 8 == 0), densely packed. */
int op_rows_gather(const void* src, void* dst, const int* list, int64_t nseg, const int64_t* src_row0, const int64_t* dst_row0,
                   const int64_t* S, const int64_t* n_kept, const int64_t* dst_rows, const int64_t* n_samples, const int64_t* list_off,
                   int64_t dst_total, int64_t cols, void* stream);
int op_rows_merge(const void* base, const void* upd, void* out, const int* list, int64_t nseg, const int64_t* src_row0,
                  const int64_t* dst_row0, const int64_t* S, const int64_t* n_kept, const int64_t* dst_rows, const int64_t* n_samples,
                  const int64_t* list_off, int64_t total, int64_t cols, void* stream);
/* (ABI 9) op_rows_merge with upd == NULL (out != base): only the rows of the DROPPED samples are copied base -> out (the kept rows were
 * written through a row table).  op_rows_map: map[r] (DEVICE int32 [dst_total]) = the row of the full matrix that packed row r stands
 * for -- what op_rows_gather would read -- or -1 for the surplus rows; `list` = the kept lists as for op_rows_gather. */
int op_rows_map(int* map, const int* list, int64_t nseg, const int64_t* src_row0, const int64_t* dst_row0, const int64_t* S,
                const int64_t* n_kept, const int64_t* dst_rows, const int64_t* n_samples, const int64_t* list_off, int64_t dst_total,
                void* stream);

/* ---- retrieval: similarity top-k without the score matrix (csrc/retrieval.hip) ----------------------------------------------
 * Replaces the materialised score matrix of the Recall metric (one_peace/metrics/recall.py:31-51: image_logits @ text_logits.t(),
 * then topk(k=10, dim=1) in each direction).  Additive: op_abi_version() stays 10, no existing entry point changed.
 * For every query row m < M of Q bf16 [M, D] (ldq) the k largest scores Q[m] . G[n] (fp32 accumulation) over the gallery G bf16 [N, D]
 * (ldg): vals fp32 [M, k] descending, idx int32 [M, k].  Order: key = (ordered fp32 bits << 32) | ~n, larger first -- higher score,
 * then lower n on exact ties; NaN (any) ranks above +inf, -0 equals +0.  The scores never reach global memory.  Results are
 * bit-identical for every split count.  1 <= k <= 64, k <= N < 2^31, D % 32 == 0 (host zero-pads), ldq / ldg >= D and % 8 == 0, Q / G
 * 16-byte aligned; else OP_EINVAL.  splits: gallery splits of the first kernel (0 = auto, at most 512; op_sim_topk_splits gives the
 * number used); with more than one, the partial lists go to `workspace` ([M, splits, k] 64-bit keys, op_sim_topk_workspace_bytes)
 * and a second kernel merges them. */
int64_t op_sim_topk_splits(int64_t M, int64_t N, int64_t splits);
int64_t op_sim_topk_workspace_bytes(int64_t M, int64_t N, int64_t k, int64_t splits);
int op_sim_topk(const void* Q, int64_t ldq, const void* G, int64_t ldg, int64_t M, int64_t N, int64_t D, int64_t k, float* vals, int* idx,
                void* workspace, int64_t workspace_bytes, int64_t splits, void* stream);

/* ---- image pre-processing: PIL-exact bicubic resize + ToTensor + Normalize (csrc/image.hip) ----------------------------------
 * Replaces the hub's host transform (one_peace/models/one_peace/hub_interface.py:94-101: Resize((S, S), BICUBIC), ToTensor, Normalize
 * with the CLIP mean / std of data/base_dataset.py:23-24) for B decoded uint8 RGB images of different sizes; bit-identical to
 * PIL's Image.resize for 8-bit images followed by torchvision's fp32 arithmetic ((u / 255 - mean) / std, IEEE divisions) and, for
 * bf16, a round-to-nearest-even cast.  Additive: op_abi_version() stays 10, no existing entry point changed.
 * src: packed HWC uint8 images; image i starts at byte desc[i].src_off, and 16 readable bytes must follow its last pixel (src_bytes).
 * desc: int64 [B][11] per image {src_off, H, W, cx_off, kx, cy_off, ky, tmp_off, row0, rows, vfirst}, on the DEVICE; desc_host: the same
 * table in HOST memory (validated here, sizes the launches).  coef: int32 records built on the host (one-peace_amd/imageprep.py:
 * bicubic_coeffs, Pillow's precompute_coeffs + normalize_coeffs_8bpc): S column records of 4 + kx ints at cx_off and S row records of
 * 4 + ky ints at cy_off, each {first source sample, taps, 0, 0, 22-bit weights (|w| < 2^23), zero-padded}; kx, ky, cx_off, cy_off
 * multiples of 4.  row0 / rows: the source rows the row records read (row0 = first row's first sample, rows up to the last row's
 * last sample).  workspace: the uint8 intermediate, rows x S x 3 bytes per image at tmp_off (16-aligned).  vfirst = 1 (PIL's order for
 * an image more than 100 times taller than wide that shrinks vertically): the vertical pass runs first, row0 = 0, rows = S and the
 * intermediate is S x W x 3 bytes.
 * out: [B, 3, S, S] bf16 (out_dtype 0) or f32 (1), or uint8 [B, S, S, 3] (2: the resized pixels; mean / stdev unused).  mean, stdev:
 * HOST float[3].  16 <= S <= 1024, S % 16 == 0, 1 <= H, W < 2^30, B <= 65535; src, coef, out, workspace 16-byte aligned; else
 * OP_EINVAL before anything is launched.  Two launches: the first pass into the workspace, then the second pass and the output. */
int op_image_resize_normalize(const void* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int64_t B,
                              const int* coef, int64_t coef_count, int64_t S, const float* mean, const float* stdev, void* out,
                              int out_dtype, void* workspace, int64_t workspace_bytes, void* stream);
/* The same entry with the geometry of the training and evaluation transforms.  Additive: op_abi_version() stays 10;
 * op_image_resize_normalize is this entry with flip = NULL and is unchanged.
 * RandomHorizontalFlip (data/vision_data/image_classify_dataset.py:59, data/vision_data/nlvr2_dataset.py:37): flip = uint8 [B] on the
 * DEVICE, non-zero = image i is stored mirrored (column S - 1 - x), in all three output types; NULL = no image is.  The flip comes last, as
 * in the reference's Compose.  RandomResizedCrop(S, scale, BICUBIC) (data/pretrain_data/image_text_pretrain_dataset.py:46-53) and Resize(S)
 * + CenterCrop(S) (image_classify_dataset.py:78-84) need no kernel work: PIL's crop(box).resize((S, S)) is the same two passes with the
 * records of a box-sized image whose first-sample fields are shifted by the box origin, and the centre crop is a window of S records of the
 * aspect-preserving resize (one-peace_amd/imageprep.py: pack_images(crops = ..., center_crop = ...)); the records of an image may
 * therefore start anywhere inside it. */
int op_image_resize_normalize_flip(const void* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int64_t B,
                                   const int* coef, int64_t coef_count, int64_t S, const float* mean, const float* stdev, void* out,
                                   int out_dtype, void* workspace, int64_t workspace_bytes, const uint8_t* flip, void* stream);

/* ---- batch augmentation: Mixup / CutMix in one pass over the batch (csrc/augment.hip) ------------------------------------------------
 * Replaces the full-batch torch passes of timm's Mixup as the reference's image-classification collater uses it
 * (data/vision_data/image_classify_dataset.py:46-51, 117-130).  Additive: op_abi_version() stays 10, no existing entry point changed.
 * x: [B, CHW] bf16 (in_dtype 0) or f32 (1), dense, CHW = channels * H * W; out: the same shape in out_dtype.  out may be x itself when
 * the dtypes agree (in place), else the two must not overlap.  kind int32 [B], lam / one_minus_lam fp32 [B] and box int32 [B, 4]
 * (yl, yh, xl, xh) are DEVICE tables.  Sample i is mixed with its partner j = B - 1 - i of the ORIGINAL batch:
 *   kind 0  out[i] = x[i]
 *   kind 1  out[i] = fadd_rn(fmul_rn(x[i], lam[i]), fmul_rn(x[j], one_minus_lam[i])): two rounded fp32 products and one rounded sum, never
 *           an fma -- torch's x.mul_(lam).add_(x.flip(0).mul_(1 - lam)) bit for bit in fp32
 *   kind 2  out[i] = x[j] where yl <= y < yh and xl <= x < xh, x[i] elsewhere (an empty box copies; nothing is read through the box)
 * Any other kind copies.  bf16 inputs are widened exactly; a bf16 output is ONE round-to-nearest-even cast of the fp32 value, as
 * torch.Tensor.to(bfloat16).  A work item owns the same 8 elements of samples i and j, reads both, then writes both: in place needs no
 * clone; for odd B the middle sample is its own partner.  One read and one write of the batch, no workspace, no atomics: two runs give
 * the same bits.  OP_ENOTSUP without a launch unless W % 8 == 0, CHW % 8 == 0 and x, out are 16-byte aligned (the caller falls back);
 * OP_EINVAL before any launch: unknown dtype, B < 0 or > 131070, H or W < 1, CHW not a multiple of H * W or >= 2^31, null or misaligned tables,
 * partially overlapping x / out.  B == 0 returns without a launch. */
int op_mix_images(const void* x, void* out, int in_dtype, int out_dtype, int64_t B, int64_t CHW, int64_t H, int64_t W, const int* kind,
                  const float* lam, const float* one_minus_lam, const int* box, void* stream);

/* ---- photometric train transforms on the resized uint8 batch: ColorJitter, GaussianBlur, ToTensor / Normalize (csrc/photometric.hip) ----
 * The steps of the reference's train transforms between the resize and ToTensor, on img = dense uint8 [B, S, S, 3] on the device (what
 * op_image_resize_normalize* writes with out_dtype 2), bit for bit PIL.  Additive: op_abi_version() stays 10, no existing entry point
 * changed.  All three: 16 <= S <= 1024, S % 16 == 0, 0 <= B <= 65535, img 16-byte aligned; else OP_EINVAL before anything is launched.
 * B == 0 returns without a launch.
 *
 * op_image_color_jitter, in place: RandomDistortion = torchvision ColorJitter through PIL.ImageEnhance (utils/transforms.py:144-157;
 * data/vl_data/nlvr2_dataset.py:35, data/vision_data/image_classify_dataset.py:57).  ops int32 [B, 3] (0 none, 1 brightness, 2 contrast,
 * 3 saturation), applied in order, and factor fp32 [B, 3] are DEVICE tables; ops_host / factor_host the same tables in HOST memory
 * (validated here, decide the launches).  Every op is Image.blend(degenerate, image, f) per byte:
 *   t = fadd_rn((float)d, fmul_rn(f, (float)(p - d))) -- two rounded fp32 operations, never an fma -- then clipped to 0 ... 255 and truncated
 * with d = 0 (brightness), L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 of the pixel (saturation), or the image's
 * m = (2 sum(L) + S S) / (2 S S) as it is when the contrast op runs (contrast).  sums: DEVICE uint32 [B] workspace, zeroed and filled here.
 * One launch sums L for the images with a contrast op (integer atomics: two runs give the same bits; skipped when no image has one), one
 * applies the chain; an image whose three ops are 0 is neither read nor written, and a batch of such images launches nothing.
 * OP_EINVAL: an op outside 0 ... 3, more than one contrast op in an image, a negative or non-finite factor, null or misaligned tables.
 *
 * op_image_gaussian_blur, in place: ImageFilter.GaussianBlur (utils/transforms.py:160-188; data/vl_data/refcoco_dataset.py:33,
 * nlvr2_dataset.py:36, image_classify_dataset.py:58): three extended box blurs along x, then three along y, each
 *   out[x] = (acc ww + far fw + 2^23) >> 24 in 32-bit unsigned arithmetic, acc = sum of in[clamp(x + i)] for |i| <= R,
 *   far = in[clamp(x - R - 1)] + in[clamp(x + R + 1)].
 * R int32 [B], ww / fw uint32 [B] (one-peace_amd/imageprep.py: gaussian_box_params) and on uint8 [B] are DEVICE tables, R_host / on_host
 * HOST copies.  Images with on == 0 are not touched; a batch of them launches nothing.  Two launches: rows, then columns, each staging what
 * it overwrites in LDS first.  OP_EINVAL: R outside 0 ... 32 for an image with on != 0, null or misaligned tables.
 *
 * op_image_normalize_flip: ToTensor, Normalize and RandomHorizontalFlip (image_classify_dataset.py:59-63, nlvr2_dataset.py:37-41,
 * refcoco_dataset.py:34-35) of src uint8 [B, S, S, 3] into out [B, 3, S, S] bf16 (out_dtype 0) or f32 (1): the arithmetic, the cast and the
 * flip flags (flip uint8 [B] on the DEVICE or NULL) of op_image_resize_normalize_flip -- one device function serves both.  mean, stdev: HOST
 * float[3].  out 16-byte aligned and not overlapping src. */
int op_image_color_jitter(void* img, int64_t B, int64_t S, const int* ops, const float* factor, const int* ops_host,
                          const float* factor_host, unsigned* sums, void* stream);
int op_image_gaussian_blur(void* img, int64_t B, int64_t S, const int* R, const unsigned* ww, const unsigned* fw, const uint8_t* on,
                           const int* R_host, const uint8_t* on_host, void* stream);
int op_image_normalize_flip(const void* src, int64_t B, int64_t S, const float* mean, const float* stdev, void* out, int out_dtype,
                            const uint8_t* flip, void* stream);

/* ---- RandAugment and RandomErasing of timm's create_transform (csrc/randaugment.hip) -------------------------------------------------
 * The two steps of the reference's default image-classification train transform that the entries above do not cover
 * (data/vision_data/image_classify_dataset.py:65-77: timm.data.create_transform(auto_augment='rand-m9-mstd0.5-inc1',
 * interpolation='bicubic', re_prob=0.25, re_mode='pixel', re_count=1)).  timm's RandAugment ops are Pillow calls on the resized image;
 * every op below gives Pillow's bytes.  Additive: op_abi_version() stays 10, no existing entry point changed.
 *
 * op_image_randaug_layer, in place on img = dense uint8 [B, S, S, 3]: ONE RandAugment layer, i.e. one op per image.  16 <= S <= 1024,
 * S % 16 == 0, 0 <= B <= 65535, img and scratch 16-byte aligned.  op int32 [B] and arg fp64 [B, 6] are DEVICE tables, op_host / arg_host
 * the same tables in HOST memory (validated here, decide the launches); fill: HOST uint8[3], the colour of Affine's uncovered pixels;
 * hist: DEVICE uint32 [B, 3, 256] workspace, zeroed and filled here; scratch: DEVICE uint8 [B, S, S, 3], not overlapping img.
 * Per channel c and byte p:
 *    1 AutoContrast  ImageOps.autocontrast: lo / hi = first / last non-empty bin of the channel's histogram; hi <= lo: unchanged; else in
 *                    fp64 scale = 255.0 / (hi - lo), offset = -lo * scale, lut[i] = clamp((int)(i * scale + offset), 0, 255) -- a rounded
 *                    product, a rounded sum, truncation toward zero
 *    2 Equalize      ImageOps.equalize: fewer than two non-empty bins: unchanged; step = (S S - count of the last non-empty bin) / 255;
 *                    0: unchanged; else lut[i] = min(255, (step / 2 + the counts of the bins below i) / step), integers only
 *    3 Invert        255 - p
 *    4 Posterize     p & ~(2^(8 - bits) - 1), bits = arg[0] in 0 ... 7 (timm returns the image for bits >= 8: that is op 0)
 *    5 Solarize      p < thresh ? p : 255 - p, thresh = arg[0] in 0 ... 256
 *    6 SolarizeAdd   p < 128 ? min(255, p + add) : p, add = arg[0] in 0 ... 255
 *   10 Sharpness     ImageEnhance.Sharpness: d = ImageFilter.SMOOTH of the layer's input = (2 s + 13) / 26 in integers, s = the 3 x 3 sum
 *                    with centre weight 5, the one-pixel border copied; then Image.blend(d, p, (float)arg[0]), the two-rounding fp32 blend
 *                    of op_image_color_jitter (one device function serves both)
 *   11 Affine        Image.transform(size, AFFINE, arg[0 ... 5], BICUBIC, fillcolor=fill): for output pixel (x, y), in fp64 with one rounding
 *                    per operation, xin = a0 (x + 0.5) + a1 (y + 0.5) + a2, yin = a3 (x + 0.5) + a4 (y + 0.5) + a5; outside [0, S): fill;
 *                    else the 4 x 4 bicubic of Geometry.c around (xin - 0.5, yin - 0.5) -- columns clamped, row 0 clamped, a later row
 *                    outside the image repeats the row value before it -- and the byte is 0 for v <= 0, 255 for v >= 255, else (uint8)v
 *                    (truncated).  Rotate, ShearX / Y and TranslateX / Y are this op with the coefficients of imageprep.affine_coeffs.
 * Codes 7 Color, 8 Contrast, 9 Brightness are op_image_color_jitter's ops 3, 2, 1 and are refused here.  An image with op 0 is neither read
 * nor written; a batch of such images launches nothing.  Launches: the histograms (integer atomics: two runs give the same bits; a bin
 * holds at most 2^20; only when an image has op 1 or 2), the apply pass (pointwise ops in place through a LUT each workgroup builds in
 * LDS; ops 10 and 11 read img and write scratch), the copy of the images of ops 10 and 11 back into img (only when one occurs).
 * OP_EINVAL before any launch: S or B out of range, null, misaligned or overlapping buffers, an op outside 0 ... 6, 10, 11, bits, thresh or
 * add not an integer in its range, a negative or non-finite sharpness factor, a non-finite affine coefficient.  B == 0 launches nothing.
 *
 * op_image_erase, in place on x [B, 3, S, S] bf16 (dtype 0) or f32 (1), 1 <= S <= 16384: RandomErasing's store,
 *   x[i, :, top:top+h, left:left+w] = noise_i.view(3, h, w).to(x.dtype), i.e. element [c, top + r, left + q] = noise[noise_off[i] + (c h + r) w + q],
 * a bf16 value ONE round-to-nearest-even cast.  box int32 [B, 4] = (top, left, h, w), h = 0: untouched; noise fp32 (3 h w values per erased
 * image) and noise_off int64 [B] are DEVICE buffers, box_host the boxes in HOST memory.  One launch; none when no image is erased.
 * OP_EINVAL before the launch: unknown dtype, S or B out of range, null or misaligned pointers, a box with h < 0, w < 1 or outside the image. */
int op_image_randaug_layer(void* img, int64_t B, int64_t S, const int* op, const double* arg, const int* op_host, const double* arg_host,
                           const uint8_t* fill, unsigned* hist, void* scratch, void* stream);
int op_image_erase(void* x, int dtype, int64_t B, int64_t S, const int* box, const int* box_host, const float* noise,
                   const int64_t* noise_off, void* stream);

/* ---- audio pre-processing: channel mean + whole-clip layer norm + crop / tile / pad (csrc/audioprep.hip) -----------------------
 * Replaces the host loop of one_peace/models/one_peace/hub_interface.py:170-193 and data/base_dataset.py:84-102 (audio_postprocess:
 * feats.mean(-1), F.layer_norm(feats, feats.shape) over the WHOLE clip, crop to max_len samples from the start, repeat the normalised
 * clip up to min_len, then collate_tokens' right-padding with 0) for B decoded clips of different lengths.  Additive: op_abi_version()
 * stays 10, no existing entry point changed.
 * src: the clips back to back, clip i at byte desc[i].src_off (a multiple of 16): frames x channels interleaved samples, int16 PCM
 * (format 0; value s / 32768, stereo (l + r) / 65536, exact) or fp32 (format 1; stereo fl(l + r) * 0.5).  desc: int64 [B][6] per clip
 * {src_off, frames, channels, format, out_len, part_off}, on the DEVICE; desc_host: the same table in HOST memory (validated here,
 * sizes the launches).  out_len = max(min(frames, max_len), min_len); part_off = the sum of ceil(frames / 8192) over the clips before
 * this one (its first 16-byte statistics partial in the workspace).  workspace: 16 bytes per 8192 frames of every clip.
 * out: [B, T] bf16 (out_dtype 0, round-to-nearest-even) or f32 (1): out[i, t] = (x[t mod min(frames, max_len)] - mean) * rstd for
 * t < out_len and 0 behind it, with mean and rstd = 1 / sqrt(var + 1e-5) (biased variance) formed in fp64 and rounded to fp32; int16
 * statistics are integer sums.  Per sample |out - fp64 result| <= 2^-24 (4 |y| + 2 |mean| rstd) for f32.  A clip's values depend on
 * nothing else in the batch, nor on its row or T; two runs give the same bits (no atomics).
 * 1 <= frames <= 2^27, channels 1 or 2, 0 <= min_len <= max_len <= 2^27, out_len <= T <= 2^27, B <= 65535; src, out, workspace
 * 16-byte aligned; else OP_EINVAL before anything is launched.  Two launches: statistics partials, then normalise + pad. */
int op_audio_normalize_pad(const void* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int64_t B, int64_t max_len,
                           int64_t min_len, void* out, int64_t T, int out_dtype, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- audio sample-rate conversion: polyphase Kaiser-windowed sinc (csrc/audioresample.hip) ------------------------------------
 * Replaces the resampling of one_peace/models/one_peace/hub_interface.py:175 (librosa.load(audio, sr=16000): soxr on the host) for B
 * decoded clips of different rates and lengths, in one launch.  The filter is this project's own, defined in closed form on the host
 * (one-peace_amd/audioprep.py: resample_filter); it is NOT soxr's, so resampled audio differs from the reference's by the difference
 * between the two low-pass filters.  Additive: op_abi_version() stays 10, no existing entry point changed.
 * src: the clips in op_audio_normalize_pad's source layout (int16 PCM or fp32, 1 or 2 interleaved channels, clip i at the 16-aligned
 * byte desc[i].src_off).  desc: int64 [B][12] per clip {src_off, frames, channels, format, L, M, T, half, coef_off, out_frames, dst_off,
 * 0}, on the DEVICE; desc_host: the same table in HOST memory (validated here, sizes the launch).  The rate ratio is L / M in lowest
 * terms, h[-half ... half] the low-pass at L times the input rate, T = floor(2 half / L) + 1 the taps per output and
 * out_frames = ceil(frames L / M).  coef: fp32 tables built on the host; the clip's table starts at element coef_off (a multiple of 4)
 * and holds L rows of Tp = 4 ceil(T / 4) taps: row p, tap t = fp32(L h[p + (floor((half - p) / L) - t) L]), 0 outside the filter and
 * for t >= T.  Clips of the same rate share a table.
 * out: clip i's mono fp32 samples at byte dst_off (a multiple of 16): op_audio_normalize_pad's source layout with format 1 and one
 * channel.  out[n] = L sum_j x[j] h[n M - j L] over 0 <= j < frames, x = the channel mean (int16: s / 32768, (l + r) / 65536, exact;
 * fp32 stereo: fl(l + r) * 0.5): Tp fp32 fused multiply-adds in four interleaved partial sums.  With S[n] = L sum_j |x[j] h[n M - j L]|,
 * |out[n] - exact| <= (T + 3) 2^-24 S[n].  Nothing outside [0, frames) of a clip is read and nothing outside its out_frames samples
 * written; n M is formed in 64 bits.  No atomics: two runs give the same bits, and a clip's values depend on nothing else in the batch.
 * 1 <= frames, out_frames <= 2^27, channels 1 or 2, 1 <= L <= 640, L <= half, floor(255 M / L) + Tp + 2 <= 8192 (the input window of a
 * workgroup's 256 outputs, staged in LDS), B <= 65535; src, coef, out 16-byte aligned; else OP_EINVAL before anything is launched. */
int op_audio_resample(const void* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int64_t B, const float* coef,
                      int64_t coef_count, void* out, int64_t out_bytes, void* stream);

/* ---- classification metrics: average precision per class without a sort or a host copy (csrc/metrics.hip) ---------------------
 * Replaces the host path of the MAP metric (one_peace/metrics/map.py:35-44: torch.sigmoid(preds).cpu().numpy(), then sklearn's
 * average_precision_score(targets, preds, average=None): a device-to-host copy of [N, C] floats and one host sort per class).
 * Additive: op_abi_version() stays 10, no existing entry point changed.
 * scores: fp32 [N, C], row stride ld_scores elements; targets: uint8 [N, C], row stride ld_targets bytes, non-zero = positive.
 * ap: fp64 [C]; npos: int32 [C] = P_c, the positives of class c.  With CNT_c(i) = #{j : s_jc >= s_ic} and TP_c(i) = #{j : y_jc != 0 and
 * s_jc >= s_ic}: ap[c] = 0.0 when P_c = 0 (sklearn 1.7.2's value, which it gives with a warning), else
 * ap[c] = (sum over the positives i of TP_c(i) / CNT_c(i)) / P_c -- sklearn's sum over thresholds of (recall step) x precision, tied scores
 * sharing one threshold as in precision_recall_curve.  Order is by fp32 value: -0 equals +0, +-inf are ordinary values; a NaN (refused by
 * the Python wrapper, as sklearn raises on it) ranks above +inf.  The counts are exact integers; every quotient is a correctly rounded
 * fp64 division; the terms are summed in an order fixed by the class's own column (64 positives at a time in sample order, a fixed tree
 * inside the 64, then the groups in sequence) with no floating-point atomics: |ap[c] - exact| <= (P_c + 2) 2^-53, two runs give the same
 * bits, and a class's result depends on nothing in the other columns, nor on C, ld_scores or ld_targets.
 * workspace: op_average_precision_workspace_bytes(N, C) = 4 N C + 16 C ceil(N / 64) bytes (ordered keys, target bits and partial sums,
 * class-major), 16-byte aligned.  1 <= N < 2^31, 1 <= C <= 65535, ld_scores, ld_targets >= C; else OP_EINVAL before anything is
 * launched.  Three launches: keys and target bits, counts and partial sums (N P_c pair tests per class), the per-class finish. */
int64_t op_average_precision_workspace_bytes(int64_t N, int64_t C);
int op_average_precision(const float* scores, int64_t ld_scores, const uint8_t* targets, int64_t ld_targets, int64_t N, int64_t C,
                         double* ap, int* npos, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- fine-tuning losses: loss, logged counter and gradient in one pass over the logits (csrc/losses.hip) -------------------------
 * Additive: op_abi_version() stays 10, no existing entry point changed.
 * op_row_loss: logits [B, C], bf16 (dtype 0) or fp32 (dtype 1), row stride ld >= C elements.  Per row it writes row_loss fp32 [B],
 * row_correct fp32 [B] and, when dlogits is non-null, dlogits fp32 [B, C] (dense) = gscale * d row_loss / d logits.  When sums is non-null
 * a second launch writes sums[0] = sum of row_loss, sums[1] = sum of row_correct, in a fixed order.  fp32 math, the row maximum
 * subtracted before every exponential; the row is read from memory once (staged in LDS up to 4096 columns; later columns are read again
 * from the caches); no floating-point atomics: two runs give the same bits.  mode:
 *   0 hard   one_peace/criterions/classify_loss.py:62-64: F.cross_entropy(logits, targets, label_smoothing = eps, reduction = 'sum')
 *            and logits.argmax(1).eq(targets).  targets int64 [B].  row_loss = (1 - eps) nll + (eps / C) sum_c -logp_c (torch's
 *            smoothing: over C, not the C - 1 of op_infonce_rows); row_correct = (argmax == target), the lowest index winning a tie.
 *            Target -100 (ignore_index): loss 0, gradient 0, correct 0.  Any other target outside [0, C): loss NaN, gradient 0, correct 0;
 *            nothing is read at such an index.
 *   1 soft   classify_loss.py:56-60: utils.log_softmax, (-targets * log_probs).sum(), (log_probs.exp() * targets).sum().  targets [B, C]
 *            bf16 / fp32 (target_dtype), row stride ld_targets; they need not sum to 1.  row_loss = sum_c -t_c logp_c,
 *            row_correct = sum_c p_c t_c, gradient p_c sum_k t_k - t_c.
 *   2 multi  classify_loss.py:51-54: F.binary_cross_entropy_with_logits(logits, targets, reduction = 'sum') and
 *            targets.gather(1, logits.argmax(1, keepdim = True)).  row_loss = sum_c max(x, 0) - x t + log1p(exp(-|x|)), gradient
 *            sigmoid(x) - t, row_correct = t[argmax x].
 *   3 hinge  one_peace/criterions/hinge_loss.py:49-53: rows of C = num_choices logits, targets int64 [B] (outside [0, C): as in mode 0,
 *            without an ignore_index).  row_loss = sum_k max(0, (margin + x_k) - x_target), the k = target term included; where the
 *            argument is exactly 0 the subgradient is 0.5, as torch.max(tensor, tensor) gives; row_correct = (argmax == target).  The
 *            reference hard-codes `1 +` and ignores its own margin option; here margin is honoured (equal at the default 1.0).
 * A NaN logit makes that row's loss NaN and ranks as the row's arg-max, as in torch.  label_smoothing is read in mode 0, margin in mode 3,
 * target_dtype and ld_targets in modes 1 and 2.  OP_EINVAL before any launch: null or misaligned pointers, B < 0, C < 1, ld < C,
 * ld_targets < C, unknown mode or dtype, label_smoothing outside [0, 1).  B == 0 returns without a launch. */
int op_row_loss(const void* logits, int dtype, int64_t ld, const void* targets, int target_dtype, int64_t ld_targets, int64_t B, int64_t C,
                int mode, float label_smoothing, float margin, float gscale, float* row_loss, float* row_correct, float* dlogits,
                float* sums, void* stream);
/* one_peace/criterions/refcoco_loss.py:36-46 with B = nsentences: logits [B, 4] bf16 / fp32 (dense), targets fp32 [B, 4] (x1, y1, x2, y2).
 * o = sigmoid(logits); out[0] = sum |o - t| / B + the mean over the valid rows (o_x1 < o_x2 and o_y1 < o_y2) of 1 - GIoU(o_i, t_i),
 * out[1] = the number of valid rows.  GIoU by the formulae of torchvision.ops.generalized_box_iou (clamped intersection and enclosing
 * extents, iou - (enclosing - union) / enclosing), the diagonal only: no [B, B] matrix.  dlogits (may be null) fp32 [B, 4] =
 * gscale * d out[0] / d logits through the sigmoid, with torch's subgradients: sign(0) = 0, 1/2 to each side of a tied max / min, the
 * clamp passing the gradient at 0.  With no valid row out[0] is NaN (the mean of an empty tensor) and the gradient is that of the L1
 * term.  One workgroup: the valid rows are counted, in a fixed order, before anything is divided.  B < 2^24; B == 0 returns without
 * a launch. */
int op_box_loss(const void* logits, int dtype, const float* targets, int64_t B, float gscale, float* out, float* dlogits, void* stream);

/* ---- single-query attention pooling of the fine-tuning head (csrc/attnpool.hip) ---------------------------------------------------
 * Additive: op_abi_version() stays 10, no existing entry point changed.
 * op_attn_pool_fwd replaces one_peace/models/one_peace/one_peace_base.py:157 and :160-170 (MultiheadAttentionPooling.forward between
 * the K / V projections and out_proj: the expanded query, bmm, masked_fill_, fp32 softmax, bmm, reshape); op_attn_pool_bwd replaces
 * the autograd backward of those lines.  The projections of :158-159 and :171 stay GEMMs of their own.
 * k, v: bf16, element (b, s, h, d) at b * batch_stride + s * ld + h * hd + d (strides in elements): a [:, 1:, :] slice, or the two
 * halves of one [B, S, 2 H] buffer, need no copy.  q: bf16 [heads * hd], one learned query per head.  pad: uint8 [B, ld_pad], non-zero
 * = masked key, or NULL.  out: bf16 [B, heads * hd], dense.  p: fp32 [B, heads, S], the probabilities, kept for the backward.
 *   scores  s_s = q_h . k[b, s, h, :] in fp32, WITHOUT a 1 / sqrt(hd) factor (the reference has none, :157-160)
 *   p       = softmax over the unmasked keys in fp32, the maximum subtracted (expf, one division per key)
 *   out     = sum_s p_s v[b, s, h, :] in fp32, rounded to bf16 once (to nearest even)
 * op_attn_pool_bwd, with p as stored and c = sum_s p_s dp_s per (b, h):  dp_s = dout_h . v_s,  ds_s = p_s (dp_s - c),
 * dv_s = p_s dout_h,  dk_s = ds_s q_h,  dq_part[b, h, :] = sum_s ds_s k_s.  dout: bf16 [B, heads * hd], dense.  dk, dv: bf16 with their
 * own strides ldg / batch_stride_g; EVERY element of [B, S, heads * hd] is written.  dq_part: fp32 [B, heads * hd], one partial per
 * sample: the caller sums it over B (no atomics).
 * Masked keys -- a DEVIATION from the reference: a masked key gets p = 0 exactly and is skipped, not multiplied by zero; its rows of k
 * and v are never read and its rows of dk and dv are zeros (the backward takes p_s == 0 as the mark).  A non-finite value in a masked row
 * of k or v therefore reaches no output, where the reference's bmm turns it into NaN.  A sample whose keys are ALL masked gives NaN in
 * p, out and its gradients, as in the reference (softmax over a row of -inf).
 * Every sum runs in a fixed order: two runs give the same bits, and the results of sample b do not depend on B.
 * Limits (OP_EINVAL with a message otherwise, nothing launched): hd % 8 == 0 and 8 <= hd <= 128; 1 <= S <= 4096; ld, ldg >= heads * hd;
 * ld, ldg and the batch strides multiples of 8; batch_stride_g >= (S - 1) * ldg + heads * hd when B > 1; every bf16 pointer and dq_part
 * aligned to 16 bytes; ld_pad >= S; B * heads < 2^31.  B == 0 returns without a launch.  Nothing is allocated or synchronised. */
int op_attn_pool_fwd(const void* k, const void* v, int64_t ld, int64_t batch_stride, const void* q, const uint8_t* pad, int64_t ld_pad,
                     void* out, float* p, int64_t B, int64_t S, int64_t heads, int64_t hd, void* stream);
int op_attn_pool_bwd(const void* dout, const void* k, const void* v, int64_t ld, int64_t batch_stride, const void* q, const float* p,
                     void* dk, void* dv, int64_t ldg, int64_t batch_stride_g, float* dq_part, int64_t B, int64_t S, int64_t heads,
                     int64_t hd, void* stream);

/* ---- mean-pool head of the vision-branch classifier (csrc/tokenpool.hip) -------------------------------------------------------------
 * Additive: op_abi_version() stays 10, no existing entry point changed.
 * op_token_mean_ln_fwd replaces one_peace_vision/classification/models_vit.py:431-434 up to the head's Linear (OnePeaceViT.forward_head
 * with global_pool: x[:, 1:, :].mean(dim=1), then fc_norm); op_token_mean_ln_bwd replaces the autograd backward of those two lines (the
 * expanded mean, the zero-filled slice gradient, the LayerNorm backward).  The Linear of :434 stays a GEMM of its own.
 * x: bf16, element (b, s, h) at b * batch_stride + s * ld + h (strides in elements): a view of a larger buffer needs no copy.  Row s = 0
 * (CLS) is NEVER read.  w, b: bf16 [H], either may be NULL (1 resp. 0).  y: bf16 [B, H], dense.  pooled: fp32 [B, H]; mean, rstd: fp32
 * [B]: kept for the backward.
 *   pooled  = (sum_{s >= 1} x[b, s, :]) / (S - 1) in fp32 -- a DEVIATION from the reference, which rounds the mean to bf16 before the norm
 *   mean, rstd = the statistics of pooled[b, :] over H in fp32 (two passes; rstd = 1 / sqrt(var + eps), var the biased variance)
 *   y       = (pooled - mean) * rstd * w + b, rounded to bf16 once (to nearest even)
 * part: fp32 workspace of the caller, B * OP_TOKEN_POOL_MAX_SPLITS * H elements.  The tokens of a sample are summed in P splits (P a
 * function of S alone, at most OP_TOKEN_POOL_MAX_SPLITS) by separate workgroups into part [B, P, H]; the pass that normalises adds the
 * P partials in index order.  Its contents mean nothing after the call.
 * op_token_mean_ln_bwd, with pooled, mean, rstd as stored, xhat = (pooled - mean) * rstd, g = dy * w, c1 = mean_h(g), c2 = mean_h(g xhat):
 *   dpool = rstd * (g - c1 - xhat * c2) in fp32;   dx[b, s, :] = bf16(dpool[b, :] / (S - 1)) for every s >= 1, +0 for s = 0.
 * dy: bf16 [B, H], dense.  dx: bf16 with its own strides ldg / batch_stride_g; EVERY element of [B, S, H] is written (the value is
 * converted once per column and stored down the rows).  dw_part, db_part: fp32 [H], the sums over b, in index order, of dy * xhat and
 * of dy; WRITTEN, not accumulated; either may be NULL.  dx may be NULL too (the parts alone; its strides are still checked), not all three.
 * Every sum runs in a fixed order and there are no atomics: two runs give the same bits, and the results of sample b do not depend on B.
 * Limits (OP_EINVAL with a message otherwise, nothing launched): H % 8 == 0 and 8 <= H <= 8192; 2 <= S <= 65536; B <= 2^20; ld, ldg >= H;
 * ld, ldg and the batch strides non-negative multiples of 8; batch_stride_g >= (S - 1) * ldg + H when B > 1; every pointer but mean and
 * rstd (4 bytes) aligned to 16 bytes; eps >= 0.  B == 0 returns without a launch.  Nothing is allocated or synchronised. */
#define OP_TOKEN_POOL_MAX_SPLITS 16
int op_token_mean_ln_fwd(const void* x, int64_t ld, int64_t batch_stride, const void* w, const void* b, float eps, void* y,
                         float* pooled, float* mean, float* rstd, float* part, int64_t B, int64_t S, int64_t H, void* stream);
int op_token_mean_ln_bwd(const void* dy, const float* pooled, const void* w, const float* mean, const float* rstd, void* dx, int64_t ldg,
                         int64_t batch_stride_g, float* dw_part, float* db_part, int64_t B, int64_t S, int64_t H, void* stream);

/* ---- temporal attention of the video branch (csrc/frameattn.hip) ---------------------------------------------------------------------
 * Additive: op_abi_version() stays 10, no existing entry point changed.
 * op_attn_frames_fwd replaces one_peace_vision/video/mmaction_custom/models/backbones/onepeace.py:234-247 (MultiheadAttention.forward
 * between its projections and the sub-LayerNorm: the head views, q * scaling, bmm, softmax, bmm, the transpose back) as called from
 * :331-337, INCLUDING the two rearranges 'n (b t) d -> t (b n) d' (:331) and 't (b n) d -> n (b t) d' (:337): self-attention over the T
 * frames of a clip, one sequence per (video b, token position n, head h), no bias, no mask, no dropout.  op_attn_frames_bwd replaces the
 * autograd backward of those lines.  The projections, the LayerNorms and the adapters of :334-336 are row-wise and stay what they are.
 * Layout: every tensor is bf16; element (b, t, n, h, d) lies at ((b * T + t) * N + n) * ld + h * hd + d (strides in elements): the
 * project's batch-major rows of B * T frames with N tokens each.  q, k, v share ld: the three column blocks of one packed [R, 3 H]
 * projection output (R = B * T * N, H = heads * hd) serve without a copy.  out and dout use the same row order with the stride ldo,
 * dq / dk / dv with ldg: they may be the column blocks of one packed [R, 3 H] gradient matrix.  Columns beyond heads * hd of a row are
 * neither read nor written.
 *   forward   s = scale * (q_t . k_t') in fp32 (a 64-term dot, then the factor);  p = softmax over t' in fp32, the maximum subtracted
 *             (expf);  out_t = (sum_t' e_t' v_t') / (sum_t' e_t') in fp32, rounded to bf16 once (to nearest even).
 *             DEVIATION from the reference's bf16 run: s and p are never rounded to bf16 (the reference's bmm outputs are), and q is not
 *             rounded after the scaling (the reference's `q *= self.scaling` is): more accurate, not bit-compatible.
 *   backward  p is RECOMPUTED from q and k: nothing but q, k, v is kept from the forward, `out` is not an argument.  dp = dout_t . v_t',
 *             c = sum_t' p dp,  ds = p (dp - c),  dv_t' = sum_t p dout_t,  dq_t = scale * sum_t' ds k_t',  dk_t' = scale * sum_t ds q_t;
 *             each rounded to bf16 once.  EVERY element of [R, heads * hd] of dq, dk and dv is written.
 * No atomics, every sum in a fixed order inside one lane: two runs give the same bits, and the bits of sequence (b, n, h) depend on its
 * own T rows, T and scale alone -- not on B, N or heads.
 * Limits (OP_EINVAL with a message otherwise, nothing launched; checked before the device is touched): hd == 64; 1 <= T <= 32;
 * N, heads >= 1; B >= 0; ld, ldo, ldg multiples of 8 and >= heads * hd; every pointer non-null and aligned to 16 bytes;
 * B * N * heads < 2^31.  Offsets are 64-bit.  B == 0 returns without a launch.  Nothing is allocated or synchronised. */
int op_attn_frames_fwd(const void* q, const void* k, const void* v, int64_t ld, void* out, int64_t ldo, int64_t B, int64_t T, int64_t N,
                       int64_t heads, int64_t hd, float scale, void* stream);
int op_attn_frames_bwd(const void* q, const void* k, const void* v, int64_t ld, const void* dout, int64_t ldo, void* dq, void* dk, void* dv,
                       int64_t ldg, int64_t B, int64_t T, int64_t N, int64_t heads, int64_t hd, float scale, void* stream);

/* ---- pretraining masks: whole words, image patches, audio blocks (csrc/masks.hip) --------------------------------------------------
 * Additive: op_abi_version() stays 10, no existing entry point changed.
 * Every random choice is select(candidates, k, keys): the k items first in the order (key descending, index ascending) over the
 * candidates; the row's other items follow them in index order.  Keys are int32 >= 0 (the sign bit is ignored).  The outputs are a pure
 * function of (inputs, keys, counts): no atomics, no global scratch, two runs give the same bits.  One workgroup per (row, mask kind)
 * sorts the row's keys in LDS (bitonic, next power of two) and compacts the kept positions by ballot and popcount.
 * Layout of every mask: uint8 (torch.bool) [B, S], S = items + 1; position 0 is CLS and never masked, item t sits at position t + 1,
 * positions beyond the row's own length are False.  ids: int64 [B, width], the ascending positions of the row with mask False (padding
 * positions left out), then -1: what collate_fn (one_peace/data/__init__.py:50-81, merge(..., pad=-1)) gives.
 * Limits: at most 4096 items per row, B < 2^31; OP_EINVAL with a message before anything is launched otherwise.  B == 0 returns without
 * a launch.
 * op_mask_patches replaces one_peace/data/pretrain_data/image_text_pretrain_dataset.py:85-94 and :99-104.  keys_a, keys_b: [B, N].
 * mask = select(all, m1, keys_a), ids [B, N + 1 - m1].  vl_mask = (not masked) U select(masked, extra, keys_b), vl_ids [B, m1 - extra + 1];
 * 0 <= extra <= m1 <= N.  keys_b, vl_mask and vl_ids may all be NULL: the first mask alone.
 * op_mask_words replaces add_whole_word_mask (image_text_pretrain_dataset.py:121-139, audio_text_pretrain_dataset.py:98-116) and
 * image_text_pretrain_dataset.py:73-77, :97-98, :101-102.  src_tokens: int64 [B, L], row stride ld: the caption's tokens, eos, then
 * `pad`.  n = (tokens != pad) - 1 (0 for an all-pad row); positions 0 ... n + 1 belong to the row.  table: uint8 [vocab];
 * ws[t] = table[token t] != 0 for t < n (a token outside [0, vocab) starts no word), W = sum ws, k = ceil(float32(W) * p) in fp32 as
 * torch rounds is_word_start.float().sum() * p.  The k starts select(ws, k, keys_a) are masked, each with the tokens after it up to the
 * next start or the caption's end.  A row with n == 0 or W == 0 gets no masked token (the reference asserts).  With keys_b, vl_mask,
 * vl_ids: vl_mask = select(tokens not masked, int(n * vl_ratio), keys_b), the product in fp64; masked tokens follow in index order when
 * fewer are unmasked.  counts: int32 [2, B] (kind, row) = the row's kept positions; a row that keeps more than width (vl_width) positions
 * has its ids truncated to the first width, never written out of bounds.  keys_a, keys_b: [B, L].  0 <= p, vl_ratio <= 1.
 * op_mask_blocks replaces one_peace/utils/data_utils.py:147-175 and :187-226 (compute_block_mask_1d: overlapping blocks,
 * require_same_masks, no expand_adjcent, mask_dropout or inverse_mask) and audio_text_pretrain_dataset.py:77-78, :81-82.
 * rows: int32 [B, 3] = (T, K, target) per clip, on the device, and rows_host, the same table in host memory, which is what is checked:
 * 0 <= T <= Tmax, 0 <= K <= Kmax, 0 <= target <= T, T + 1 - target <= width.  centers: int32 [B, Kmax]; keys: [B, Tmax].
 * Frames clamp(c + i - length / 2, 0, T - 1), i < length, are masked for each of the row's first K centres; with n masked frames,
 * n > target unmasks select(masked, n - target, keys), n < target masks select(unmasked, target - n, keys). */
int op_mask_patches(const int* keys_a, const int* keys_b, int64_t B, int64_t N, int64_t m1, int64_t extra, uint8_t* mask, int64_t* ids,
                    uint8_t* vl_mask, int64_t* vl_ids, void* stream);
int op_mask_words(const int64_t* src_tokens, int64_t ld, int64_t B, int64_t L, int64_t pad, const uint8_t* table, int64_t vocab,
                  const int* keys_a, const int* keys_b, float p, double vl_ratio, uint8_t* mask, int64_t* ids, int64_t width,
                  uint8_t* vl_mask, int64_t* vl_ids, int64_t vl_width, int* counts, void* stream);
int op_mask_blocks(const int* rows, const int* rows_host, const int* centers, int64_t Kmax, const int* keys, int64_t Tmax, int64_t B,
                   int64_t length, uint8_t* mask, int64_t* ids, int64_t width, void* stream);

/* ---- window attention of the detection branch (csrc/windowattn.hip) -----------------------------------------------------------------
 * Additive: op_abi_version() stays 10, no existing entry point changed.
 * op_attn_window_fwd replaces one_peace_vision/det/models/onepeace.py:197-213 (MultiheadAttention.forward between its projections and
 * the sub-LayerNorm) as called from :308-325 in a window block, INCLUDING window_partition and window_unpartition (:310, :325), the
 * expanded window bias of :398-401 and add_decomposed_rel_pos (:207): self-attention inside the 16 x 16 windows of a token map, one
 * sequence of 256 tokens per (sample b, window, head h).  op_attn_window_bwd replaces the autograd backward of those lines.
 * Layout: every activation tensor is bf16; element (b, y, x, h, d) lies at ((b * Hg + y) * Wg + x) * ld + 64 h + d (strides in
 * elements): the project's batch-major rows of a [B, Hg, Wg, D] map.  q, k, v share ld (the three column blocks of one packed [R, 3 H]
 * projection output), out and dout use ldo, dq / dk / dv use ldg and may be the blocks of one packed gradient matrix.  Window (wy, wx)
 * holds y in [16 wy, 16 wy + 16) and x likewise; the in-window index is i = 16 (y % 16) + x % 16 (detectron2's window_partition order).
 * bias: bf16 [heads][256][256], query-major, shared by all windows and samples, or NULL.  rel_h, rel_w: bf16 [31][64], shared by all
 * heads, or NULL together.
 *   forward   s[i][j] = scale * (q_i . k_j) + bias[h][i][j] + q_i . rel_h[iy - jy + 15] + q_i . rel_w[ix - jx + 15] in fp32, the UNSCALED
 *             q in the last two terms (:204-207);  p = softmax over the 256 keys, the maximum subtracted;  out = p v, rounded to bf16
 *             once.
 *   backward  s and p are RECOMPUTED from q, k, v, bias, rel_*: nothing else is kept from the forward.  dp = dout . v,
 *             c = sum_j p dp in fp32 from the resident p and dp (never from a rounded out),  ds = p (dp - c),  dv = p^T dout,
 *             dk = scale * ds^T q,  dTh[i][jy] = sum_jx ds[i][(jy, jx)],  dTw[i][jx] = sum_jy ds[i][(jy, jx)],
 *             dq_i = scale * sum_j ds k_j + sum_jy dTh[i][jy] rel_h[iy - jy + 15] + sum_jx dTw[i][jx] rel_w[ix - jx + 15].
 *             EVERY element of [R, heads * 64] of dq, dk and dv is written.
 *             drel_part (optional): fp32 [parts][2][31][64]; entry (0, r, d) holds sum dTh[i][jy] q_i[d] over the part's share of
 *             (b, window, head, i, jy) with iy - jy + 15 == r, entry (1, r, d) the same for w.  dbias_slabs (optional): fp32
 *             [slabs][heads][256][256], each slab the sum of ds over its share of (b, window).  Every element of both is written, by an
 *             empty share too; the caller sums over the leading axis.  op_attn_window_parts(B, windows, heads, &parts, &slabs) gives
 *             the two counts (windows = (Hg / 16) * (Wg / 16)).  With a NULL pointer that work is skipped (frozen tables, inference).
 *             With both NULL the backward runs one workgroup per (b, window, head), as the forward does; dq, dk, dv have the same bits.
 * STATED DEVIATIONS: every product runs on the matrix pipe (v_mfma_f32_32x32x16_bf16, fp32 accumulation), and these fp32 operands are
 * rounded to bf16 (to nearest even) first: e = exp(s - max) before e v (the division by sum e follows in fp32);  p before p^T dout;
 * ds before ds k and ds^T q;  dTh and dTw before the products with rel_h / rel_w (dq) and with q (drel_part).  s, the softmax
 * statistics, c, ds itself, dTh, dTw and the dbias slabs are fp32.  The backward takes max, sum e and sum e dp tile by tile with a
 * running maximum (two sweeps over the keys; s is computed twice with the same bits).  exp is v_exp_f32 of (s - max) * log2 e.
 * No atomics, every sum in a fixed order: two runs give the same bits in every output, and the bits of out, dq, dk, dv of a (b, window,
 * head) depend on that window's own rows, bias[h], rel_* and scale alone -- not on B, the grid or heads.  Nothing is allocated or
 * synchronised.
 * Limits (OP_EINVAL with a message otherwise, checked before the device is touched, nothing launched): hd == 64 and window == 16;
 * Hg % 16 == 0 and Wg % 16 == 0; ld, ldo, ldg multiples of 8 and >= heads * 64; every pointer that is given aligned to 16 bytes;
 * B * windows * heads < 2^31.  Offsets are 64-bit.  B == 0 returns without a launch. */
int op_attn_window_parts(int64_t B, int64_t windows, int64_t heads, int64_t* parts, int64_t* slabs);
int op_attn_window_fwd(const void* q, const void* k, const void* v, int64_t ld, const void* bias, const void* rel_h, const void* rel_w,
                       void* out, int64_t ldo, int64_t B, int64_t Hg, int64_t Wg, int64_t heads, int64_t hd, int64_t window, float scale,
                       void* stream);
int op_attn_window_bwd(const void* q, const void* k, const void* v, int64_t ld, const void* bias, const void* rel_h, const void* rel_w,
                       const void* dout, int64_t ldo, void* dq, void* dk, void* dv, int64_t ldg, void* drel_part, void* dbias_slabs,
                       int64_t B, int64_t Hg, int64_t Wg, int64_t heads, int64_t hd, int64_t window, float scale, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ONEPEACE_HIP_H */
