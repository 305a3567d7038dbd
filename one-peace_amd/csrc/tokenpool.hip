// Mean-pool head of the vision-branch classifier (include/onepeace_hip.h: op_token_mean_ln_fwd, op_token_mean_ln_bwd): the device
// computation of OnePeaceViT.forward_head with global_pool, one_peace_vision/classification/models_vit.py:431-434 up to the head's
// Linear: x[:, 1:, :].mean(dim=1) and fc_norm, and the autograd backward of those two lines.
//
// Lanes run along H, each holding 8 adjacent columns (one 16-byte load or store); the CLS row (s = 0) is never read.
//   forward   token_partial_kernel: one workgroup per (sample, split, 512 columns).  The S - 1 patch tokens are cut into P splits of
//             `rows` tokens (tp_splits: a function of S alone); the four waves of a workgroup take the rows of their split in turn
//             (four 16-byte loads in flight per lane), add them in row order in fp32 and meet in LDS in wave order ->
//             part [B, P, H].  token_norm_kernel: one workgroup per sample adds the P partials in index order, divides by S - 1 ->
//             pooled (fp32, kept for the backward); mean and variance over H in two passes over registers; y = bf16 once.
//   backward  token_bwd_kernel: one workgroup per (sample, 64 rows of dx).  Every workgroup of a sample repeats the LayerNorm backward
//             of that sample's row from dy, pooled, w, mean, rstd (12 KB from L2 against 196 KB written at H = 1536; the same
//             instructions in the same order: the same bits in every workgroup), converts dpool / (S - 1) to bf16 ONCE per column
//             and stores that vector down its rows; row 0 gets zeros.  token_parts_kernel: dw_part / db_part, the terms of 16
//             samples staged in LDS side by side, each column's terms added in sample order.
// Every sum has a fixed order (rows of a wave, waves, splits; shuffles, waves; samples): no atomics, two runs give the same bits, and
// nothing a sample's workgroups compute depends on B.
#include "common.h"

#include <math.h>

namespace {

constexpr int TP_THREADS = 256;
constexpr int TP_ROWS = 64;        // tokens of a split while S - 1 <= TP_ROWS * TP_MAX_SPLITS; rows of dx per backward workgroup
constexpr int TP_MAX_SPLITS = 16;  // include/onepeace_hip.h: OP_TOKEN_POOL_MAX_SPLITS (the caller sizes `part` by it)
constexpr int TP_U = 4;            // rows in flight per lane
constexpr int TP_MAX_NP = 4;       // column passes of a 256-lane workgroup: H <= 8192

// the S - 1 patch tokens in P splits of `rows` tokens (the last one may hold fewer): a function of S alone
inline void tp_splits(int64_t S, int& rows, int& P) {
  const int64_t T = S - 1;
  rows = (int)((T + TP_MAX_SPLITS - 1) / TP_MAX_SPLITS);
  if (rows < TP_ROWS) rows = TP_ROWS;
  P = (int)((T + rows - 1) / rows);
}

__device__ __forceinline__ float tp_block_sum(float v, float* red4) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  v = ((red4[0] + red4[1]) + red4[2]) + red4[3];
  __syncthreads();
  return v;
}

__global__ __launch_bounds__(TP_THREADS) void token_partial_kernel(const bf16_t* __restrict__ x, int64_t ld, int64_t batch_stride,
                                                                   float* __restrict__ part, int S, int H, int rows, int P) {
  __shared__ __align__(16) float red[4][64][8];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t b = blockIdx.x / P;
  const int p = blockIdx.x % P;
  const int col = (blockIdx.y * 64 + lane) * 8;
  const bool live = col < H;
  const int s0 = 1 + p * rows;
  const int s1 = min(S, s0 + rows);
  const bf16_t* __restrict__ xb = x + b * batch_stride + col;
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  if (live) {
    for (int s = s0 + wave; s < s1; s += 4 * TP_U) {
      bf16x8 raw[TP_U];
#pragma unroll
      for (int u = 0; u < TP_U; ++u) {
#pragma unroll
        for (int j = 0; j < 8; ++j) raw[u][j] = (bf16_t)0.f;
        if (s + 4 * u < s1) raw[u] = *reinterpret_cast<const bf16x8*>(xb + (int64_t)(s + 4 * u) * ld);
      }
#pragma unroll
      for (int u = 0; u < TP_U; ++u) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] += (float)raw[u][j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[wave][lane][j] = acc[j];
  __syncthreads();
  if (wave == 0 && live) {
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = ((red[0][lane][j] + red[1][lane][j]) + red[2][lane][j]) + red[3][lane][j];
    Vec8<float>::store(part + ((int64_t)blockIdx.x * H + col), acc);
  }
}

template <int NP>
__global__ __launch_bounds__(TP_THREADS) void token_norm_kernel(const float* __restrict__ part, const bf16_t* __restrict__ w,
                                                                const bf16_t* __restrict__ bias, float eps, bf16_t* __restrict__ y,
                                                                float* __restrict__ pooled, float* __restrict__ mean,
                                                                float* __restrict__ rstd, int S, int H, int P) {
  __shared__ float red4[4];
  const int64_t b = blockIdx.x;
  const float tokens = (float)(S - 1);
  float v[NP][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int col = (threadIdx.x + i * TP_THREADS) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
    if (col < H) {
      for (int p = 0; p < P; ++p) {
        float t[8];
        Vec8<float>::load(part + ((b * P + p) * H + col), t);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] += t[j];
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[i][j] = v[i][j] / tokens;
        sum += v[i][j];
      }
      Vec8<float>::store(pooled + b * H + col, v[i]);
    }
  }
  const float mu = tp_block_sum(sum, red4) / (float)H;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    if ((threadIdx.x + i * TP_THREADS) * 8 < H) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = v[i][j] - mu;
        sq = fmaf(d, d, sq);
      }
    }
  }
  const float rs = 1.0f / sqrtf(tp_block_sum(sq, red4) / (float)H + eps);
  if (threadIdx.x == 0) {
    mean[b] = mu;
    rstd[b] = rs;
  }
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int col = (threadIdx.x + i * TP_THREADS) * 8;
    if (col < H) {
      float wv[8], bv[8], o[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        wv[j] = 1.f;
        bv[j] = 0.f;
      }
      if (w) Vec8<bf16_t>::load(w + col, wv);
      if (bias) Vec8<bf16_t>::load(bias + col, bv);
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mu) * rs * wv[j] + bv[j];
      Vec8<bf16_t>::store(y + b * H + col, o);
    }
  }
}

template <int NP>
__global__ __launch_bounds__(TP_THREADS) void token_bwd_kernel(const bf16_t* __restrict__ dy, const float* __restrict__ pooled,
                                                               const bf16_t* __restrict__ w, const float* __restrict__ mean,
                                                               const float* __restrict__ rstd, bf16_t* __restrict__ dx, int64_t ldg,
                                                               int64_t batch_stride_g, int S, int H, int chunks) {
  __shared__ float red4[4];
  const int64_t b = blockIdx.x / chunks;
  const int chunk = blockIdx.x % chunks;
  const float mu = mean[b], rs = rstd[b];
  float g[NP][8], xh[NP][8];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int col = (threadIdx.x + i * TP_THREADS) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) g[i][j] = xh[i][j] = 0.f;
    if (col < H) {
      float wv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) wv[j] = 1.f;
      if (w) Vec8<bf16_t>::load(w + col, wv);
      Vec8<bf16_t>::load(dy + b * H + col, g[i]);
      Vec8<float>::load(pooled + b * H + col, xh[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        g[i][j] *= wv[j];
        xh[i][j] = (xh[i][j] - mu) * rs;
        s1 += g[i][j];
        s2 = fmaf(g[i][j], xh[i][j], s2);
      }
    }
  }
  const float c1 = tp_block_sum(s1, red4) / (float)H;
  const float c2 = tp_block_sum(s2, red4) / (float)H;
  const float tokens = (float)(S - 1);
  const int r0 = chunk * TP_ROWS, r1 = min(S, r0 + TP_ROWS);
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int col = (threadIdx.x + i * TP_THREADS) * 8;
    if (col < H) {
      bf16x8 val, zero;  // the same value down every row: converted once per column
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        val[j] = (bf16_t)(rs * (g[i][j] - c1 - xh[i][j] * c2) / tokens);
        zero[j] = (bf16_t)0.f;
      }
      bf16_t* __restrict__ out = dx + b * batch_stride_g + col;
      for (int s = r0; s < r1; ++s) *reinterpret_cast<bf16x8*>(out + (int64_t)s * ldg) = s == 0 ? zero : val;
    }
  }
}

// dw_part[h] = sum_b dy[b, h] xhat[b, h], db_part[h] = sum_b dy[b, h], the samples in index order.  One workgroup per 128 columns.  A
// walk of B samples per lane costs a memory latency per few samples and keeps three workgroups busy, so the terms of TPP_SAMPLES samples
// are loaded side by side (lane = 8 columns of one sample, 16-byte loads) and staged in LDS; then lane t adds column t & 127 of the dw
// terms (t < 128) or of the db terms down the staged samples, in index order, while the next round's loads are in flight.
constexpr int TPP_COLS = 128;
constexpr int TPP_SAMPLES = 16;

__global__ __launch_bounds__(TP_THREADS) void token_parts_kernel(const bf16_t* __restrict__ dy, const float* __restrict__ pooled,
                                                                 const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                 float* __restrict__ dw_part, float* __restrict__ db_part, int B, int H) {
  __shared__ __align__(16) float terms[2][TPP_SAMPLES][TPP_COLS];  // [dy xhat | dy]
  const int cv = threadIdx.x & 15, slot = threadIdx.x >> 4;
  const int col = blockIdx.x * TPP_COLS + cv * 8;
  const bool live = col < H;
  const int oc = threadIdx.x & (TPP_COLS - 1), which = threadIdx.x >> 7;
  bf16x8 d;
  Vec8<float>::raw_t p;
  float mu = 0.f, rs = 0.f;
  bool on = live && slot < B;
  if (on) {
    d = Vec8<bf16_t>::ldraw(dy + (int64_t)slot * H + col);
    p = Vec8<float>::ldraw(pooled + (int64_t)slot * H + col);
    mu = mean[slot];
    rs = rstd[slot];
  }
  float acc = 0.f;
  for (int b0 = 0; b0 < B; b0 += TPP_SAMPLES) {
    if (on) {
      float dv[8], xv[8], tw[8];
      Vec8<bf16_t>::cvt(d, dv);
      Vec8<float>::cvt(p, xv);
#pragma unroll
      for (int j = 0; j < 8; ++j) tw[j] = dv[j] * ((xv[j] - mu) * rs);
      Vec8<float>::store(&terms[0][slot][cv * 8], tw);
      Vec8<float>::store(&terms[1][slot][cv * 8], dv);
    }
    __syncthreads();
    const int b = b0 + TPP_SAMPLES + slot;  // the next round's sample of this lane
    on = live && b < B;
    if (on) {
      d = Vec8<bf16_t>::ldraw(dy + (int64_t)b * H + col);
      p = Vec8<float>::ldraw(pooled + (int64_t)b * H + col);
      mu = mean[b];
      rs = rstd[b];
    }
    const int n = min(TPP_SAMPLES, B - b0);
    for (int s = 0; s < n; ++s) acc += terms[which][s][oc];
    __syncthreads();
  }
  float* __restrict__ out = which == 0 ? dw_part : db_part;
  if (out && blockIdx.x * TPP_COLS + oc < H) out[blockIdx.x * TPP_COLS + oc] = acc;
}

// the limits both entries share; `what` names the entry in the message
int tp_check_shape(const char* what, int64_t ld, int64_t batch_stride, int64_t B, int64_t S, int64_t H) {
  OP_CHECK_ARG(H >= 8 && H <= 8192 && H % 8 == 0, "%s: H = %lld, need a multiple of 8 in 8 ... 8192", what, (long long)H);
  OP_CHECK_ARG(S >= 2 && S <= 65536, "%s: S = %lld, need 2 <= S <= 65536 (CLS and at least one patch token)", what, (long long)S);
  OP_CHECK_ARG(B >= 0 && B <= (int64_t(1) << 20), "%s: B = %lld, need 0 <= B <= 2^20", what, (long long)B);
  OP_CHECK_ARG(ld % 8 == 0 && ld >= H, "%s: row stride = %lld, need a multiple of 8 and >= H = %lld", what, (long long)ld, (long long)H);
  OP_CHECK_ARG(batch_stride % 8 == 0 && batch_stride >= 0, "%s: batch stride = %lld, need a non-negative multiple of 8", what,
               (long long)batch_stride);
  return OP_OK;
}

inline bool tp_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int op_token_mean_ln_fwd(const void* x, int64_t ld, int64_t batch_stride, const void* w, const void* b, float eps, void* y,
                                    float* pooled, float* mean, float* rstd, float* part, int64_t B, int64_t S, int64_t H,
                                    void* stream) {
  const int rc = tp_check_shape("op_token_mean_ln_fwd", ld, batch_stride, B, S, H);
  if (rc != OP_OK) return rc;
  OP_CHECK_ARG(x && y && pooled && mean && rstd && part, "op_token_mean_ln_fwd: x, y, pooled, mean, rstd and part must be non-null");
  OP_CHECK_ARG(tp_aligned16(x) && tp_aligned16(w) && tp_aligned16(b) && tp_aligned16(y) && tp_aligned16(pooled) && tp_aligned16(part) &&
                   (((uintptr_t)mean | (uintptr_t)rstd) & 3) == 0,
               "op_token_mean_ln_fwd: x, w, b, y, pooled and part must be aligned to 16 bytes, mean and rstd to 4");
  OP_CHECK_ARG(eps >= 0.f, "op_token_mean_ln_fwd: eps = %g, need >= 0", (double)eps);
  if (B == 0) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  int rows, P;
  tp_splits(S, rows, P);
  hipLaunchKernelGGL(token_partial_kernel, dim3((unsigned)(B * P), (unsigned)ceil_div(H, 512)), dim3(TP_THREADS), 0, st, (const bf16_t*)x,
                     ld, batch_stride, part, (int)S, (int)H, rows, P);
  OP_LAUNCH_CHECK();
  return op_with_int<1, 2, 3, 4>(ceil_div(H, 8 * TP_THREADS), [&](auto np) {
    hipLaunchKernelGGL((token_norm_kernel<decltype(np)::value>), dim3((unsigned)B), dim3(TP_THREADS), 0, st, (const float*)part,
                       (const bf16_t*)w, (const bf16_t*)b, eps, (bf16_t*)y, pooled, mean, rstd, (int)S, (int)H, P);
    OP_LAUNCH_CHECK();
    return OP_OK;
  });
}

extern "C" int op_token_mean_ln_bwd(const void* dy, const float* pooled, const void* w, const float* mean, const float* rstd, void* dx,
                                    int64_t ldg, int64_t batch_stride_g, float* dw_part, float* db_part, int64_t B, int64_t S, int64_t H,
                                    void* stream) {
  const int rc = tp_check_shape("op_token_mean_ln_bwd", ldg, batch_stride_g, B, S, H);
  if (rc != OP_OK) return rc;
  OP_CHECK_ARG(B <= 1 || batch_stride_g >= (S - 1) * ldg + H,
               "op_token_mean_ln_bwd: batch_stride_g = %lld, need >= (S - 1) * ldg + H = %lld (the samples' rows of dx must not overlap)",
               (long long)batch_stride_g, (long long)((S - 1) * ldg + H));
  OP_CHECK_ARG(dy && pooled && mean && rstd, "op_token_mean_ln_bwd: dy, pooled, mean and rstd must be non-null");
  OP_CHECK_ARG(dx || dw_part || db_part, "op_token_mean_ln_bwd: dx, dw_part and db_part are all null: nothing to compute");
  OP_CHECK_ARG(tp_aligned16(dy) && tp_aligned16(pooled) && tp_aligned16(w) && tp_aligned16(dx) && tp_aligned16(dw_part) &&
                   tp_aligned16(db_part) && (((uintptr_t)mean | (uintptr_t)rstd) & 3) == 0,
               "op_token_mean_ln_bwd: dy, pooled, w, dx, dw_part and db_part must be aligned to 16 bytes, mean and rstd to 4");
  if (B == 0) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int chunks = ceil_div(S, TP_ROWS);
  static_assert(TP_MAX_NP * 8 * TP_THREADS == 8192, "the column passes cover H <= 8192");
  const int launched = !dx ? OP_OK : op_with_int<1, 2, 3, 4>(ceil_div(H, 8 * TP_THREADS), [&](auto np) {
    hipLaunchKernelGGL((token_bwd_kernel<decltype(np)::value>), dim3((unsigned)(B * chunks)), dim3(TP_THREADS), 0, st, (const bf16_t*)dy,
                       pooled, (const bf16_t*)w, mean, rstd, (bf16_t*)dx, ldg, batch_stride_g, (int)S, (int)H, chunks);
    OP_LAUNCH_CHECK();
    return OP_OK;
  });
  if (launched != OP_OK) return launched;
  if (dw_part || db_part) {
    hipLaunchKernelGGL(token_parts_kernel, dim3((unsigned)ceil_div(H, TPP_COLS)), dim3(TP_THREADS), 0, st, (const bf16_t*)dy, pooled, mean,
                       rstd, dw_part, db_part, (int)B, (int)H);
    OP_LAUNCH_CHECK();
  }
  return OP_OK;
}
