// LayerNorm forward/backward for gfx950, optional fused exact-erf GELU on the output.
//
// Replaces: one_peace/models/components.py:23-26,47-52 (torch.nn.LayerNorm / flash_attn layer_norm seam)
// and, with act=1, the LayerNorm->GELU pairs of adapter/image.py:66-75 and adapter/audio.py:293-301.
//
// Roofline: pure HBM.  Algorithmic bytes (bf16): fwd 4*cols B/row (+8 B stats), bwd 6*cols B/row
// read (x, dy) + write (dx) (+ the two [cols] reductions, negligible).
// Mapping: one wavefront (64 lanes) per row when cols <= 2048, a whole 256-thread workgroup per row
// above that; every lane moves 16-byte (bf16x8) or 32-byte (f32x8) chunks, statistics in fp32 with a
// centred second pass (same numerics as torch: biased variance, eps inside the rsqrt).
#include "common.h"

namespace {

constexpr int LN_MAX_BLOCKS = 4096;       // workspace bound for the dw/db partials
constexpr int g_ln_blocks_fwd = 512, g_ln_blocks_bwd = 512;  // persistent-grid caps (round-1 sweep: tools/ln_sweep.py, profiles/)
// The fused GeGLU + LayerNorm(F) passes have their own caps (tools/ln_geglu_sweep.py, 32 896 x 6144, round 3): forward 256 / 512 /
// 1024 / 2048 / 4096 workgroups -> 0.389 / 0.265 / 0.240 / 0.237 / 0.236 ms; backward (dw / db partials per workgroup) 0.530 /
// 0.403 / 0.417 / 0.448 / 0.507 ms.
#ifndef OP_LN_GEGLU_BLOCKS_FWD
#define OP_LN_GEGLU_BLOCKS_FWD 2048
#endif
#ifndef OP_LN_GEGLU_BLOCKS_BWD
#define OP_LN_GEGLU_BLOCKS_BWD 512
#endif

template <int NW>
__device__ __forceinline__ float group_sum(float v, float* red) {
  v = wave_sum(v);
  if (NW == 1) return v;
  const int wid = threadIdx.x >> 6;
  __syncthreads();  // protect `red` from the previous use
  if ((threadIdx.x & 63) == 0) red[wid] = v;
  __syncthreads();
  float t = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) t += red[i];
  return t;
}

// Two sums with ONE barrier pair (the backward kernels need mean(dy w) and mean(dy w xhat) of the same row); red: >= 2 * NW floats.
template <int NW>
__device__ __forceinline__ void group_sum2(float& a, float& b, float* red) {
  a = wave_sum(a);
  b = wave_sum(b);
  if (NW == 1) return;
  const int wid = threadIdx.x >> 6;
  __syncthreads();  // protect `red` from the previous use
  if ((threadIdx.x & 63) == 0) { red[wid] = a; red[NW + wid] = b; }
  __syncthreads();
  float ta = 0.f, tb = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) { ta += red[i]; tb += red[NW + i]; }
  a = ta;
  b = tb;
}

// amax of a row held by NW waves, from the per-lane fp8_amax_acc bit patterns (NaN-propagating, common.h)
template <int NW>
__device__ __forceinline__ float group_amax(int m, float* red) {
  const float v = fp8_wave_amax(m);
  if (NW == 1) return v;
  const int wid = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[wid] = v;
  __syncthreads();
  int t = __float_as_int(red[0]);
#pragma unroll
  for (int i = 1; i < NW; ++i) t = max(t, __float_as_int(red[i]));
  return __int_as_float(t);
}

// Q8 (round 5; bf16, no GELU): the row is ALSO written as fp8 e4m3 with a per-row scale -- exactly what op_quant_fp8_rows makes of the
// bf16 output (amax over the bf16-rounded values), without its pass over the output: the operand of the fp8 FFN GEMMs (csrc/fp8.hip).
template <typename T, int CH, int NW, bool GELU, bool NT, bool Q8 = false>  // NT: non-temporal row accesses (tensors far beyond the caches: training)
__global__ __launch_bounds__(256) void ln_fwd_kernel(const T* __restrict__ x, const T* __restrict__ w,
                                                     const T* __restrict__ b, T* __restrict__ y,
                                                     float* __restrict__ mean_out, float* __restrict__ rstd_out,
                                                     int64_t rows, int cols, float eps, uint8_t* __restrict__ q8 = nullptr,
                                                     float* __restrict__ q8_scale = nullptr, const int* __restrict__ xmap = nullptr) {
  // xmap (nullable, ABI 9): row r of the input is row xmap[r] of a LARGER matrix x (< 0: no row -- normalised as a row of zeros, which is
  // what op_rows_gather's packed copy holds there); y / mean / rstd are indexed by r.  The packed rows of the samples a residual
  // branch keeps, read straight from the full activation matrix.
  __shared__ float red[4];
  constexpr int G = 64 * NW;
  const int tig = (NW == 1) ? (threadIdx.x & 63) : threadIdx.x;
  const int64_t row0 = (NW == 1) ? ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) : blockIdx.x;
  const int64_t rstep = (NW == 1) ? (int64_t)gridDim.x * 4 : gridDim.x;
  const float inv = 1.0f / (float)cols;

  float wv[CH][8], bv[CH][8];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = (tig + G * i) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) { wv[i][j] = 1.f; bv[i][j] = 0.f; }
    if (c < cols) {
      if (w) Vec8<T>::load(w + c, wv[i]);
      if (b) Vec8<T>::load(b + c, bv[i]);
    }
  }
  // NW == 4: every thread of the block walks the same rows (uniform trip count -> barriers are safe).
  // The next row is requested before the current one is reduced: twice the bytes in flight per wave.
  typedef typename Vec8<T>::raw_t raw_t;
  raw_t cur[CH], nxt[CH];
  // (the table entry of a row is requested one row BEFORE its data: behind each other in one trip, every row paid an L2 latency)
  auto fetch = [&](int64_t src, raw_t (&dst)[CH]) {  // (uniform per row group: the entry is the same for every thread of the row)
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
        if (src >= 0) dst[i] = ldraw_sel<T, NT>(x + src * (int64_t)cols + c);
        else dst[i] = raw_t{};
      }
    }
  };
  int64_t nsrc = row0 + rstep < rows ? (xmap ? (int64_t)xmap[row0 + rstep] : row0 + rstep) : -1;
  if (row0 < rows) fetch(xmap ? (int64_t)xmap[row0] : row0, cur);
  for (int64_t row = row0; row < rows; row += rstep) {
    const int64_t nrow = row + rstep, nnrow = nrow + rstep;
    if (nrow < rows) fetch(nsrc, nxt);
    if (nnrow < rows) nsrc = xmap ? (int64_t)xmap[nnrow] : nnrow;
    float v[CH][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
        Vec8<T>::cvt(cur[i], v[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += v[i][j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
      }
    }
    const float mean = group_sum<NW>(s, red) * inv;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; ss += d * d; }
      }
    }
    const float rstd = rsqrtf(group_sum<NW>(ss, red) * inv + eps);
    T* yr = y + row * (int64_t)cols;
    int amax = 0;  // bits of max |output| (fp8_amax_acc)
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float t = (v[i][j] - mean) * rstd * wv[i][j] + bv[i][j];
          o[j] = GELU ? gelu_erf(t) : t;
        }
        store_sel<T, NT>(yr + c, o);
        if constexpr (Q8) {  // the output as the next reader sees it (rounded to T); v is free now
#pragma unroll
          for (int j = 0; j < 8; ++j) { v[i][j] = (float)(T)o[j]; amax = fp8_amax_acc(amax, v[i][j]); }
        }
      }
    }
    if constexpr (Q8) {
      float qinv;
      const float sc = fp8_row_scale(group_amax<NW>(amax, red), qinv);
      uint8_t* qr = q8 + row * (int64_t)cols;
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int c = (tig + G * i) * 8;
        if (c < cols) *reinterpret_cast<u32x2*>(qr + c) = fp8_pack8(v[i], qinv);
      }
      if (tig == 0) q8_scale[row] = sc;
    }
    if (tig == 0) {
      if (mean_out) mean_out[row] = mean;
      if (rstd_out) rstd_out[row] = rstd;
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) cur[i] = nxt[i];
  }
}

// y = LayerNorm_F(bf16(gelu(h0) * h1)) straight from the two pre-activations of the GeGLU up-projection (row stride ldh: they are
// the halves of one [rows, 2 * cols] matrix written by a PLAIN two-segment GEMM).  Takes the exact-erf GELU (16 VALU instructions
// per element, 13 % of the fused-epilogue GEMM: one wave per SIMD cannot hide it) out of the GEMM's epilogue and into a kernel
// that is HBM-bound with VALU to spare; the product is rounded to bf16 before the statistics, exactly as the backward
// (ln_geglu_bwd_kernel) re-creates it.  Algorithmic bytes: 2 reads + 1 write of [rows, cols] bf16.
// SKIP (never with Q8): row r belongs to sample r / rps, and a row whose sample has the stochastic-depth multiplier ps == 0 is DROPPED:
// nothing of it is loaded (h0 | h1 may hold anything there, NaN included), y gets +0 and mean / rstd are left alone -- every reader of
// that y row multiplies it by an exact zero, and the backward skips the row by the same rule.  The rule of a row is read before the
// row's loads are issued (one trip ahead of them); it is the same for all threads that share a barrier (NW == 4: the
// workgroup walks one row; NW == 1: the reductions are wave-level and a wave walks one row).
template <int CH, int NW, bool Q8 = false, bool SKIP = false>  // Q8: see ln_fwd_kernel
__global__ __launch_bounds__(NW == 1 ? 256 : 64 * NW) void ln_geglu_fwd_kernel(const bf16_t* __restrict__ h0, const bf16_t* __restrict__ h1,
                                                           int64_t ldh, const bf16_t* __restrict__ w, const bf16_t* __restrict__ b,
                                                           bf16_t* __restrict__ y, float* __restrict__ mean_out,
                                                           float* __restrict__ rstd_out, int64_t rows, int cols, float eps,
                                                           uint8_t* __restrict__ q8 = nullptr, float* __restrict__ q8_scale = nullptr,
                                                           const float* __restrict__ ps = nullptr, int rps = 1) {
  static_assert(!(Q8 && SKIP), "the fp8 route runs every row");
  __shared__ float red[4];
  constexpr int G = 64 * NW;
  const int tig = (NW == 1) ? (threadIdx.x & 63) : threadIdx.x;
  // (SKIP: the wave index as a scalar, so that the walk and its multipliers stay in scalar registers)
  const int wave = SKIP ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);
  const int64_t row0 = (NW == 1) ? ((int64_t)blockIdx.x * 4 + wave) : blockIdx.x;
  const int64_t rstep = (NW == 1) ? (int64_t)gridDim.x * 4 : gridDim.x;
  const float inv = 1.0f / (float)cols;
  auto ps_of = [&](int64_t r) { return ps[(uint32_t)r / (uint32_t)rps]; };  // (SKIP; the host checks rows < 2^31)
  float wv[CH][8], bv[CH][8];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = (tig + G * i) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) { wv[i][j] = 1.f; bv[i][j] = 0.f; }
    if (c < cols) {
      if (w) Vec8<bf16_t>::load(w + c, wv[i]);
      if (b) Vec8<bf16_t>::load(b + c, bv[i]);
    }
  }
  bf16x8 c0[CH], c1[CH], n0[CH], n1[CH];
  // The walk: next_live() gives the next row of this wave / workgroup that is not dropped (every row without SKIP); the dropped rows
  // on the way get their +0 here.  The multiplier of the row AFTER the one returned is requested at once and used a trip later, so
  // only a run of dropped rows waits for its loads.
  int64_t rahead = row0;
  float pahead = 1.f;
  if constexpr (SKIP) pahead = row0 < rows ? ps_of(row0) : 1.f;
  auto next_live = [&]() {
    int64_t r = rahead;
    if constexpr (SKIP) {
      float p = pahead;
      while (r < rows && p == 0.f) {  // (uniform over the threads that share a barrier: no barrier inside, the same trips outside)
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int c = (tig + G * i) * 8;
          if (c < cols) Vec8<bf16_t>::store_nt(y + r * (int64_t)cols + c, z);
        }
        r += rstep;
        p = r < rows ? ps_of(r) : 1.f;
      }
      pahead = r + rstep < rows ? ps_of(r + rstep) : 1.f;
    }
    rahead = r + rstep;
    return r;
  };
  const int64_t first = next_live();
  if (first < rows) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
        c0[i] = Vec8<bf16_t>::ldraw_nt(h0 + first * ldh + c);
        c1[i] = Vec8<bf16_t>::ldraw_nt(h1 + first * ldh + c);
      }
    }
  }
  for (int64_t row = first; row < rows;) {
    const int64_t nrow = next_live();  // (known before the next row's loads are issued)
    if (nrow < rows) {
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int c = (tig + G * i) * 8;
        if (c < cols) {
          n0[i] = Vec8<bf16_t>::ldraw_nt(h0 + nrow * ldh + c);
          n1[i] = Vec8<bf16_t>::ldraw_nt(h1 + nrow * ldh + c);
        }
      }
    }
    float v[CH][8];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
        float a[8], bb[8];
        Vec8<bf16_t>::cvt(c0[i], a);
        Vec8<bf16_t>::cvt(c1[i], bb);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          v[i][j] = (float)(bf16_t)(gelu_erf(a[j]) * bb[j]);
          s += v[i][j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
      }
    }
    const float mean = group_sum<NW>(s, red) * inv;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float d = v[i][j] - mean; ss += d * d; }
      }
    }
    const float rstd = rsqrtf(group_sum<NW>(ss, red) * inv + eps);
    bf16_t* yr = y + row * (int64_t)cols;
    int amax = 0;  // bits of max |output| (fp8_amax_acc)
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mean) * rstd * wv[i][j] + bv[i][j];
        Vec8<bf16_t>::store_nt(yr + c, o);
        if constexpr (Q8) {
#pragma unroll
          for (int j = 0; j < 8; ++j) { v[i][j] = (float)(bf16_t)o[j]; amax = fp8_amax_acc(amax, v[i][j]); }
        }
      }
    }
    if constexpr (Q8) {
      float qinv;
      const float sc = fp8_row_scale(group_amax<NW>(amax, red), qinv);
      uint8_t* qr = q8 + row * (int64_t)cols;
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int c = (tig + G * i) * 8;
        if (c < cols) *reinterpret_cast<u32x2*>(qr + c) = fp8_pack8(v[i], qinv);
      }
      if (tig == 0) q8_scale[row] = sc;
    }
    if (tig == 0) {
      if (mean_out) mean_out[row] = mean;
      if (rstd_out) rstd_out[row] = rstd;
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) { c0[i] = n0[i]; c1[i] = n1[i]; }
    row = nrow;
  }
}

// dx = rstd * (dy*w - mean(dy*w) - xhat * mean(dy*w*xhat));  dw = sum_rows dy*xhat;  db = sum_rows dy.
// Partial dw/db of each workgroup go to ws[gridDim.x][2][cols] (fp32); ln_bwd_reduce_kernel folds them.
// SKIP (see ln_geglu_fwd_kernel; never with xmap): a dropped row has an exact-zero dy row in the dense step; nothing of dy, x, mean and
// rstd is loaded for it, dx gets +0 -- or, with `add`, the 16-byte copies of the add row (nothing at all where dx IS add) -- and dw / db
// get nothing from it.
template <typename T, int CH, int NW, bool GELU, bool NT, bool SKIP = false>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const T* __restrict__ dy, const T* __restrict__ x,
                                                     const T* __restrict__ w, const T* __restrict__ b,
                                                     const float* __restrict__ mean_in,
                                                     const float* __restrict__ rstd_in, const T* __restrict__ add,
                                                     T* __restrict__ dx, float* __restrict__ ws, int64_t rows, int cols,
                                                     const int* __restrict__ xmap = nullptr, const float* __restrict__ ps = nullptr,
                                                     int rps = 1) {
  // xmap (nullable, ABI 9; see ln_fwd_kernel): x, add and dx are rows xmap[r] of LARGER matrices (dy / mean / rstd are indexed by r);
  // a row without a source (< 0) is a row of zeros for x, has no `add` and is not stored.  dx may be `add` (in place: only the mapped
  // rows change -- the rows of dropped samples keep the gradient of the skip connection).
  extern __shared__ __attribute__((aligned(16))) float smem[];  // NW==1: [4][cols] ; NW==4: [4]
  float* red = smem;
  constexpr int G = 64 * NW;
  const int tig = (NW == 1) ? (threadIdx.x & 63) : threadIdx.x;
  const int wid = SKIP ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);  // (SKIP: a scalar, see ln_geglu_fwd_kernel)
  const int64_t row0 = (NW == 1) ? ((int64_t)blockIdx.x * 4 + wid) : blockIdx.x;
  const int64_t rstep = (NW == 1) ? (int64_t)gridDim.x * 4 : gridDim.x;
  const float inv = 1.0f / (float)cols;

  float wv[CH][8], bv[CH][8], dwa[CH][8], dba[CH][8];
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = (tig + G * i) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) { wv[i][j] = 1.f; bv[i][j] = 0.f; dwa[i][j] = 0.f; dba[i][j] = 0.f; }
    if (c < cols) {
      if (w) Vec8<T>::load(w + c, wv[i]);
      if (GELU && b) Vec8<T>::load(b + c, bv[i]);
    }
  }
  typedef typename Vec8<T>::raw_t raw_t;
  raw_t curx[CH], curg[CH], nxtx[CH], nxtg[CH], addv[CH];
  // The walk (see ln_geglu_fwd_kernel): the next row that is not dropped; the dropped rows on the way get their dx here
  auto ps_of = [&](int64_t r) { return ps[(uint32_t)r / (uint32_t)rps]; };  // (SKIP; the host checks rows < 2^31)
  int64_t rahead = row0;
  float pahead = 1.f;
  if constexpr (SKIP) pahead = row0 < rows ? ps_of(row0) : 1.f;
  auto next_live = [&]() {
    int64_t r = rahead;
    if constexpr (SKIP) {
      float p = pahead;
      while (r < rows && p == 0.f) {  // (uniform over the threads that share a barrier: no barrier inside, the same trips outside)
        if (add != dx) {
#pragma unroll
          for (int i = 0; i < CH; ++i) {
            const int c = (tig + G * i) * 8;
            if (c < cols) {
              raw_t v = raw_t{};
              if (add) v = ldraw_sel<T, NT>(add + r * (int64_t)cols + c);
              *reinterpret_cast<raw_t*>(dx + r * (int64_t)cols + c) = v;
            }
          }
        }
        r += rstep;
        p = r < rows ? ps_of(r) : 1.f;
      }
      pahead = r + rstep < rows ? ps_of(r + rstep) : 1.f;
    }
    rahead = r + rstep;
    return r;
  };
  int64_t first = row0;  // (without SKIP the walk is row0, row0 + rstep, ...: none of the state above is live)
  if constexpr (SKIP) first = next_live();
  // (uniform per row group; the entry of row r + 2 steps is requested while row r is computed: see ln_fwd_kernel)
  int64_t src = first < rows ? (xmap ? (int64_t)xmap[first] : first) : -1;
  int64_t nsrc = first + rstep < rows ? (xmap ? (int64_t)xmap[first + rstep] : first + rstep) : -1, nnsrc = -1;
  if (first < rows) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
        if (src >= 0) curx[i] = ldraw_sel<T, NT>(x + src * (int64_t)cols + c);
        else curx[i] = raw_t{};
        curg[i] = ldraw_sel<T, NT>(dy + first * (int64_t)cols + c);
      }
    }
  }
  for (int64_t row = first; row < rows;) {
    const float mean = mean_in[row], rstd = rstd_in[row];
    int64_t nrow = row + rstep;
    if constexpr (SKIP) nsrc = nrow = next_live();  // (known before the next row's loads are issued; no row table)
    const int64_t nnrow = nrow + rstep;
    if (nnrow < rows) nnsrc = xmap ? (int64_t)xmap[nnrow] : nnrow;
#pragma unroll
    for (int i = 0; i < CH; ++i) {  // residual-path gradient of this row + both operands of the next row
      const int c = (tig + G * i) * 8;
      if (c < cols) {
        if (add && src >= 0) addv[i] = ldraw_sel<T, NT>(add + src * (int64_t)cols + c);
        if (nrow < rows) {
          if (nsrc >= 0) nxtx[i] = ldraw_sel<T, NT>(x + nsrc * (int64_t)cols + c);
          else nxtx[i] = raw_t{};
          nxtg[i] = ldraw_sel<T, NT>(dy + nrow * (int64_t)cols + c);
        }
      }
    }
    float xh[CH][8], g[CH][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
        Vec8<T>::cvt(curx[i], xh[i]);
        Vec8<T>::cvt(curg[i], g[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          xh[i][j] = (xh[i][j] - mean) * rstd;
          if (GELU) g[i][j] *= gelu_erf_grad(xh[i][j] * wv[i][j] + bv[i][j]);
          dwa[i][j] += g[i][j] * xh[i][j];
          dba[i][j] += g[i][j];
          const float gw = g[i][j] * wv[i][j];
          g[i][j] = gw;
          s1 += gw;
          s2 += gw * xh[i][j];
        }
      }
    }
    group_sum2<NW>(s1, s2, red);
    const float c1 = s1 * inv, c2 = s2 * inv;
    T* dr = dx + (src >= 0 ? src : 0) * (int64_t)cols;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols && src >= 0) {
        float o[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = rstd * (g[i][j] - c1 - xh[i][j] * c2);
        if (add) {
          float av[8];
          Vec8<T>::cvt(addv[i], av);
#pragma unroll
          for (int j = 0; j < 8; ++j) o[j] += av[j];
        }
        store_sel<T, NT>(dr + c, o);
      }
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) { curx[i] = nxtx[i]; curg[i] = nxtg[i]; }
    src = nsrc;
    nsrc = nnsrc;
    row = nrow;
  }
  if (ws == nullptr) return;  // uniform
  float* wsb = ws + (int64_t)blockIdx.x * 2 * cols;
  if (NW == 1) {
    // fold the 4 waves (same column mapping, different rows) through LDS, dw then db
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int c = (tig + G * i) * 8;
        if (c < cols) {
#pragma unroll
          for (int j = 0; j < 8; ++j) smem[wid * cols + c + j] = pass == 0 ? dwa[i][j] : dba[i][j];
        }
      }
      __syncthreads();
      for (int c = threadIdx.x; c < cols; c += 256)
        wsb[pass * cols + c] = smem[c] + smem[cols + c] + smem[2 * cols + c] + smem[3 * cols + c];
    }
  } else {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { wsb[c + j] = dwa[i][j]; wsb[cols + c + j] = dba[i][j]; }
      }
    }
  }
}

// LayerNorm(F) backward fused with the GeGLU backward (transformer_layer.py:64-67,111-118): the FFN's inner
// sub-LayerNorm takes g = gelu(h0) * h1; g is RECOMPUTED from the saved h0/h1 (never stored for backward) and
//   dg  = rstd * (dy*w - mean(dy*w) - xhat * mean(dy*w*xhat)),   xhat = (g - mean) * rstd
//   dh0 = dg * h1 * gelu'(h0),   dh1 = dg * gelu(h0)
// Algorithmic bytes: 3 reads + 2 writes of [rows, cols] bf16 (the unfused pair moved 8 passes).
// SKIP (see ln_geglu_fwd_kernel): a dropped row has an exact-zero dy row in the dense step; nothing of it is loaded (dy, h0 | h1, mean,
// rstd), dh0 | dh1 get +0 and dw / db get nothing from it.
template <int CH, int NW, bool SKIP = false>
__global__ __launch_bounds__(NW == 1 ? 256 : 64 * NW) void ln_geglu_bwd_kernel(const bf16_t* __restrict__ dy, const bf16_t* __restrict__ h0,
                                                           const bf16_t* __restrict__ h1, const bf16_t* __restrict__ w,
                                                           const float* __restrict__ mean_in,
                                                           const float* __restrict__ rstd_in, bf16_t* __restrict__ dh0,
                                                           bf16_t* __restrict__ dh1, int64_t ldd, int64_t ldh, float* __restrict__ ws,
                                                           int64_t rows, int cols, const float* __restrict__ ps = nullptr, int rps = 1) {
  extern __shared__ __attribute__((aligned(16))) float smem[];  // NW==1: [4][cols] ; NW==4: [4]
  float* red = smem;
  constexpr int G = 64 * NW;
  const int tig = (NW == 1) ? (threadIdx.x & 63) : threadIdx.x;
  const int wid = SKIP ? __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) : (int)(threadIdx.x >> 6);  // (SKIP: a scalar, see ln_geglu_fwd_kernel)
  const int64_t row0 = (NW == 1) ? ((int64_t)blockIdx.x * 4 + wid) : blockIdx.x;
  const int64_t rstep = (NW == 1) ? (int64_t)gridDim.x * 4 : gridDim.x;
  const float inv = 1.0f / (float)cols;
  auto ps_of = [&](int64_t r) { return ps[(uint32_t)r / (uint32_t)rps]; };  // (SKIP; the host checks rows < 2^31)
  float dwa[CH][8], dba[CH][8];
  bf16x8 wraw[CH];  // the LayerNorm weight stays packed (4 registers per 8 columns; unpacked where it is used: one VALU op per element)
#pragma unroll
  for (int i = 0; i < CH; ++i) {
    const int c = (tig + G * i) * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) { dwa[i][j] = 0.f; dba[i][j] = 0.f; }
#pragma unroll
    for (int j = 0; j < 8; ++j) wraw[i][j] = (bf16_t)1.0f;
    if (c < cols && w) wraw[i] = Vec8<bf16_t>::ldraw(w + c);
  }
  // Registers (<= 256 for two waves per SIMD): the row is kept as raw bf16 (h0, h1) + fp32 dy*w, Phi(h0) and gelu'(h0) across the two
  // block reductions, so that the NEXT row's three operands can already be in flight.
  bf16x8 r0[CH], r1[CH], rg[CH], n0[CH], n1[CH], ng[CH];
  // The walk (see ln_geglu_fwd_kernel): the next row that is not dropped; the dropped rows on the way get their +0 here
  int64_t rahead = row0;
  float pahead = 1.f;
  if constexpr (SKIP) pahead = row0 < rows ? ps_of(row0) : 1.f;
  auto next_live = [&]() {
    int64_t r = rahead;
    if constexpr (SKIP) {
      float p = pahead;
      while (r < rows && p == 0.f) {  // (uniform over the threads that share a barrier: no barrier inside, the same trips outside)
        const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < CH; ++i) {
          const int c = (tig + G * i) * 8;
          if (c < cols) {
            Vec8<bf16_t>::store_nt(dh0 + r * ldd + c, z);
            Vec8<bf16_t>::store_nt(dh1 + r * ldd + c, z);
          }
        }
        r += rstep;
        p = r < rows ? ps_of(r) : 1.f;
      }
      pahead = r + rstep < rows ? ps_of(r + rstep) : 1.f;
    }
    rahead = r + rstep;
    return r;
  };
  const int64_t first = next_live();
  if (first < rows) {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
        r0[i] = Vec8<bf16_t>::ldraw_nt(h0 + first * ldh + c);
        r1[i] = Vec8<bf16_t>::ldraw_nt(h1 + first * ldh + c);
        rg[i] = Vec8<bf16_t>::ldraw_nt(dy + first * (int64_t)cols + c);
      }
    }
  }
  for (int64_t row = first; row < rows;) {
    const float mean = mean_in[row], rstd = rstd_in[row];
    const int64_t nrow = next_live();  // (known before the next row's loads are issued)
    if (nrow < rows) {
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int c = (tig + G * i) * 8;
        if (c < cols) {
          n0[i] = Vec8<bf16_t>::ldraw_nt(h0 + nrow * ldh + c);
          n1[i] = Vec8<bf16_t>::ldraw_nt(h1 + nrow * ldh + c);
          ng[i] = Vec8<bf16_t>::ldraw_nt(dy + nrow * (int64_t)cols + c);
        }
      }
    }
    float gw[CH][8], cdfs[CH][8], gps[CH][8];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
        float a[8], b[8];
        Vec8<bf16_t>::cvt(r0[i], a);
        Vec8<bf16_t>::cvt(r1[i], b);
        Vec8<bf16_t>::cvt(rg[i], gw[i]);
        float wv[8];
        asm volatile("" : "+v"(wraw[i]));  // (keeps the unpacking inside the row loop: hoisted, it is 24 registers again)
        Vec8<bf16_t>::cvt(wraw[i], wv);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float cdf, pdf;
          gelu_parts(a[j], cdf, pdf);
          cdfs[i][j] = cdf;
          gps[i][j] = cdf + a[j] * pdf;  // gelu'(h0): kept for the output pass (round 5: that pass took a second exponential per element)
          // the forward rounded g to bf16 before the LayerNorm statistics were taken
          const float gval = (float)(bf16_t)(a[j] * cdf * b[j]);
          const float xh = (gval - mean) * rstd;
          const float d = gw[i][j];
          dwa[i][j] += d * xh;
          dba[i][j] += d;
          const float t = d * wv[j];
          gw[i][j] = t;
          s1 += t;
          s2 += t * xh;
        }
      }
    }
    group_sum2<NW>(s1, s2, red);
    const float c1 = s1 * inv, c2 = s2 * inv;
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
        float a[8], b[8], o0[8], o1[8];
        Vec8<bf16_t>::cvt(r0[i], a);
        Vec8<bf16_t>::cvt(r1[i], b);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float ge = a[j] * cdfs[i][j];  // Phi(h0) and gelu'(h0) are kept from the first pass: no transcendental here
          const float xh = ((float)(bf16_t)(ge * b[j]) - mean) * rstd;
          // the unfused path rounded dg to bf16 between the two kernels; keep fp32 here
          const float dg = rstd * (gw[i][j] - c1 - xh * c2);
          o0[j] = dg * b[j] * gps[i][j];
          o1[j] = dg * ge;
        }
        Vec8<bf16_t>::store_nt(dh0 + row * ldd + c, o0);
        Vec8<bf16_t>::store_nt(dh1 + row * ldd + c, o1);
      }
    }
#pragma unroll
    for (int i = 0; i < CH; ++i) { r0[i] = n0[i]; r1[i] = n1[i]; rg[i] = ng[i]; }
    row = nrow;
  }
  if (ws == nullptr) return;  // uniform
  float* wsb = ws + (int64_t)blockIdx.x * 2 * cols;
  if (NW == 1) {
#pragma unroll
    for (int pass = 0; pass < 2; ++pass) {
      __syncthreads();
#pragma unroll
      for (int i = 0; i < CH; ++i) {
        const int c = (tig + G * i) * 8;
        if (c < cols) {
#pragma unroll
          for (int j = 0; j < 8; ++j) smem[wid * cols + c + j] = pass == 0 ? dwa[i][j] : dba[i][j];
        }
      }
      __syncthreads();
      for (int c = threadIdx.x; c < cols; c += 256)
        wsb[pass * cols + c] = smem[c] + smem[cols + c] + smem[2 * cols + c] + smem[3 * cols + c];
    }
  } else {
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = (tig + G * i) * 8;
      if (c < cols) {
#pragma unroll
        for (int j = 0; j < 8; ++j) { wsb[c + j] = dwa[i][j]; wsb[cols + c + j] = dba[i][j]; }
      }
    }
  }
}

inline int ln_grid(int64_t rows, int nw, int cap) {
  int64_t blocks = nw == 1 ? (rows + 3) / 4 : rows;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// cols -> (CH 16-byte chunks per lane, NW waves per row): one wave per row up to 2048 columns, a 256-thread workgroup above; a row
// holds at most 64 * NW * CH * 8 columns.  The ONLY place that knows the ladder (tests/ln_ref.py:ch_nw mirrors it).
struct LnRoute { int max_cols, ch, nw; };
constexpr LnRoute LN_ROUTES[] = {{512, 1, 1}, {1024, 2, 1}, {1536, 3, 1}, {2048, 4, 1}, {4096, 2, 4}, {6144, 3, 4}, {8192, 4, 4}};
constexpr int ln_route(int cols) {  // index into LN_ROUTES, -1 above 8192
  for (int i = 0; i < 7; ++i)
    if (cols <= LN_ROUTES[i].max_cols) return i;
  return -1;
}
constexpr bool ln_route_is(int cols, int ch, int nw) { return LN_ROUTES[ln_route(cols)].ch == ch && LN_ROUTES[ln_route(cols)].nw == nw; }
static_assert(ln_route_is(8, 1, 1) && ln_route_is(512, 1, 1), "cols <= 512");
static_assert(ln_route_is(520, 2, 1) && ln_route_is(1024, 2, 1), "cols <= 1024");
static_assert(ln_route_is(1032, 3, 1) && ln_route_is(1536, 3, 1), "cols <= 1536");
static_assert(ln_route_is(1544, 4, 1) && ln_route_is(2048, 4, 1), "cols <= 2048");
static_assert(ln_route_is(2056, 2, 4) && ln_route_is(4096, 2, 4), "cols <= 4096");
static_assert(ln_route_is(4104, 3, 4) && ln_route_is(6144, 3, 4), "cols <= 6144");
static_assert(ln_route_is(6152, 4, 4) && ln_route_is(8192, 4, 4) && ln_route(8200) == -1, "cols <= 8192");

// f(CH, NW) (as std::integral_constant) for the route of `cols`
template <typename F> int ln_with_route(int cols, F&& f) {
  const int r = ln_route(cols);
  if (r < 0) { op_set_error("layernorm: cols %d > 8192 unsupported", cols); return OP_ENOTSUP; }
  return op_with_int<0, 1, 2, 3, 4, 5, 6>(r, [&](auto i) {
    return f(std::integral_constant<int, LN_ROUTES[decltype(i)::value].ch>{}, std::integral_constant<int, LN_ROUTES[decltype(i)::value].nw>{});
  });
}

// cache policy: non-temporal row accesses for a TRAINING pass over a matrix of >= 64 MiB -- it streams once, and what it left in L2 /
// Infinity Cache only displaced the next GEMM's panels (-2 % on the headline step with the hint on every row-wise kernel); inference
// keeps the default policy: there the consumer finds the row matrix in the caches (+1 ... 5 % with the hint at the image tower's
// sizes; profiles/r4_nontemporal_ab.txt)
inline bool ln_streams(int64_t rows, int cols, size_t elem) { return rows * cols * (int64_t)elem >= ((int64_t)64 << 20); }

// Q8 (bf16, no GELU, default cache policy: the only instantiations there are) also writes q8 / q8_scale
template <typename T, bool GELU, bool Q8 = false>
int ln_fwd_dispatch(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd, int64_t rows, int cols, float eps,
                    hipStream_t s, const int* xmap, void* q8 = nullptr, float* q8_scale = nullptr) {
  // (a training pass is one whose caller wants the statistics: a backward follows)
  const bool nt = !Q8 && mean != nullptr && ln_streams(rows, cols, sizeof(T));
  return ln_with_route(cols, [&](auto ch, auto nw) {
    constexpr int CH = decltype(ch)::value, NW = decltype(nw)::value;
    auto launch = [&](auto ntc) {
      hipLaunchKernelGGL((ln_fwd_kernel<T, CH, NW, GELU, decltype(ntc)::value, Q8>), dim3(ln_grid(rows, NW, g_ln_blocks_fwd)), dim3(256), 0,
                         s, (const T*)x, (const T*)w, (const T*)b, (T*)y, mean, rstd, rows, cols, eps, (uint8_t*)q8, q8_scale, xmap);
      OP_LAUNCH_CHECK();
      return OP_OK;
    };
    if constexpr (Q8) return launch(std::false_type{});
    else return op_with_bool(nt, launch);
  });
}

// dw / db from the per-workgroup partials of a backward kernel ([grid][2][cols] fp32)
template <typename T>
int ln_reduce_dw_db(float* ws, void* dw, void* db, int grid, int cols, int accumulate, hipStream_t s) {
  hipLaunchKernelGGL((partials_reduce3_kernel<T>), dim3(ceil_div(cols, 32), 2), dim3(256), 0, s, ws, ws + cols, (const float*)nullptr,
                     (const bf16_t*)nullptr, (const bf16_t*)nullptr, (const bf16_t*)nullptr, (T*)dw, (T*)db, (T*)nullptr, grid,
                     (int64_t)2 * cols, cols, accumulate);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

template <typename T, bool GELU, bool SKIP = false>  // SKIP: rows of samples with ps == 0 are not read (see ln_bwd_kernel)
int ln_bwd_dispatch(const void* dy, const void* x, const void* w, const void* b, const float* mean, const float* rstd,
                    const void* add, void* dx, void* dw, void* db, float* ws, int64_t rows, int cols, int accumulate,
                    hipStream_t s, const int* xmap, const float* ps = nullptr, int rps = 1) {
  float* wsk = (dw || db) ? ws : nullptr;
  const bool nt = ln_streams(rows, cols, sizeof(T));
  return ln_with_route(cols, [&](auto ch, auto nw) {
    constexpr int CH = decltype(ch)::value, NW = decltype(nw)::value;
    const int grid = ln_grid(rows, NW, g_ln_blocks_bwd);
    const size_t sh = (NW == 1) ? (size_t)4 * cols * sizeof(float) : 64;
    const int rc = op_with_bool(nt, [&](auto ntc) {
      hipLaunchKernelGGL((ln_bwd_kernel<T, CH, NW, GELU, decltype(ntc)::value, SKIP>), dim3(grid), dim3(256), sh, s, (const T*)dy, (const T*)x,
                         (const T*)w, (const T*)b, mean, rstd, (const T*)add, (T*)dx, wsk, rows, cols, xmap, ps, rps);
      OP_LAUNCH_CHECK();
      return OP_OK;
    });
    return rc != OP_OK || !wsk ? rc : ln_reduce_dw_db<T>(ws, dw, db, grid, cols, accumulate, s);
  });
}

template <bool Q8, bool SKIP = false>  // SKIP: rows of samples with ps == 0 are not read (see ln_geglu_fwd_kernel)
int ln_geglu_fwd_dispatch(const void* h0, const void* h1, int64_t ldh, const void* w, const void* b, void* y, float* mean, float* rstd,
                          void* q8, float* q8_scale, int64_t rows, int cols, float eps, hipStream_t s, const float* ps = nullptr,
                          int rps = 1) {
  return ln_with_route(cols, [&](auto ch, auto nw) {
    constexpr int CH = decltype(ch)::value, NW = decltype(nw)::value;
    hipLaunchKernelGGL((ln_geglu_fwd_kernel<CH, NW, Q8, SKIP>), dim3(ln_grid(rows, NW, OP_LN_GEGLU_BLOCKS_FWD)), dim3(NW == 1 ? 256 : 64 * NW), 0,
                       s, (const bf16_t*)h0, (const bf16_t*)h1, ldh, (const bf16_t*)w, (const bf16_t*)b, (bf16_t*)y, mean, rstd, rows,
                       cols, eps, (uint8_t*)q8, q8_scale, ps, rps);
    OP_LAUNCH_CHECK();
    return OP_OK;
  });
}

template <bool SKIP>
int ln_geglu_bwd_dispatch(const void* dy, const void* h0, const void* h1, const void* w, const float* mean, const float* rstd, void* dh0,
                          void* dh1, int64_t ldd, int64_t ldh, void* dw, void* db, float* wsk, int64_t rows, int cols, int accumulate,
                          hipStream_t s, const float* ps = nullptr, int rps = 1) {
  return ln_with_route(cols, [&](auto ch, auto nw) {
    constexpr int CH = decltype(ch)::value, NW = decltype(nw)::value;
    const int grid = ln_grid(rows, NW, OP_LN_GEGLU_BLOCKS_BWD);
    const size_t sh = (NW == 1) ? (size_t)4 * cols * sizeof(float) : 64;
    hipLaunchKernelGGL((ln_geglu_bwd_kernel<CH, NW, SKIP>), dim3(grid), dim3(NW == 1 ? 256 : 64 * NW), sh, s, (const bf16_t*)dy,
                       (const bf16_t*)h0, (const bf16_t*)h1, (const bf16_t*)w, mean, rstd, (bf16_t*)dh0, (bf16_t*)dh1, ldd, ldh, wsk,
                       rows, cols, ps, rps);
    OP_LAUNCH_CHECK();
    return wsk ? ln_reduce_dw_db<bf16_t>(wsk, dw, db, grid, cols, accumulate, s) : OP_OK;
  });
}

}  // namespace

extern "C" {


// Bytes of fp32 workspace op_layernorm_bwd needs for dw/db partials.
int64_t op_layernorm_bwd_workspace_bytes(int64_t rows, int64_t cols) {
  (void)rows;
  return (int64_t)LN_MAX_BLOCKS * 2 * cols * (int64_t)sizeof(float);
}

int op_layernorm_fwd(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd, int64_t rows,
                     int64_t cols, float eps, int act_gelu, int dtype, const int* x_rows, void* stream) {
  OP_CHECK_ARG(x && y, "layernorm_fwd: null x/y");
  OP_CHECK_ARG(rows >= 0 && cols > 0 && cols % 8 == 0, "layernorm_fwd: cols=%lld must be a positive multiple of 8",
               (long long)cols);
  if (rows == 0) return OP_OK;
  OP_CHECK_ARG(dtype == OP_DT_BF16 || dtype == OP_DT_F32, "layernorm_fwd: bad dtype %d", dtype);
  return op_with_bool(dtype == OP_DT_BF16, [&](auto bf) {
    return op_with_bool(act_gelu != 0, [&](auto gelu) {
      return ln_fwd_dispatch<op_elem_t<decltype(bf)::value>, decltype(gelu)::value>(x, w, b, y, mean, rstd, rows, (int)cols, eps,
                                                                                   (hipStream_t)stream, x_rows);
    });
  });
}

// op_layernorm_fwd for bf16 without GELU that ALSO writes the output row-quantised to fp8 e4m3: q8 [rows, cols] bytes and
// q8_scale [rows] fp32, bit-identical to op_quant_fp8_rows(y) -- the activation operand of op_gemm_nt_fp8 without a pass of its own
// (the sub-LayerNorm in front of the FFN, transformer_layer.py:196-199, when the opt-in fp8 forward is on).
int op_layernorm_fwd_q8(const void* x, const void* w, const void* b, void* y, float* mean, float* rstd, void* q8, float* q8_scale,
                        int64_t rows, int64_t cols, float eps, void* stream) {
  OP_CHECK_ARG(x && y && q8 && q8_scale, "layernorm_fwd_q8: null pointer");
  OP_CHECK_ARG(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 8192, "layernorm_fwd_q8: cols=%lld unsupported", (long long)cols);
  if (rows == 0) return OP_OK;
  return ln_fwd_dispatch<bf16_t, false, true>(x, w, b, y, mean, rstd, rows, (int)cols, eps, (hipStream_t)stream, nullptr, q8, q8_scale);
}

// dx = LN backward (+ add, the gradient arriving through the residual path, optional and may alias dx)
int op_layernorm_bwd(const void* dy, const void* x, const void* w, const void* b, const float* mean, const float* rstd,
                     const void* add, void* dx, void* dw, void* db, void* workspace, int64_t rows, int64_t cols,
                     int act_gelu, int accumulate, int dtype, const int* x_rows, void* stream) {
  OP_CHECK_ARG(dy && x && dx && mean && rstd, "layernorm_bwd: null pointer");
  OP_CHECK_ARG(rows >= 0 && cols > 0 && cols % 8 == 0, "layernorm_bwd: cols=%lld must be a positive multiple of 8",
               (long long)cols);
  OP_CHECK_ARG(!(dw || db) || workspace, "layernorm_bwd: dw/db requested without workspace");
  if (rows == 0) return OP_OK;
  OP_CHECK_ARG(dtype == OP_DT_BF16 || dtype == OP_DT_F32, "layernorm_bwd: bad dtype %d", dtype);
  return op_with_bool(dtype == OP_DT_BF16, [&](auto bf) {
    return op_with_bool(act_gelu != 0, [&](auto gelu) {
      return ln_bwd_dispatch<op_elem_t<decltype(bf)::value>, decltype(gelu)::value>(
          dy, x, w, b, mean, rstd, add, dx, dw, db, (float*)workspace, rows, (int)cols, accumulate, (hipStream_t)stream, x_rows);
    });
  });
}

// (additive: op_abi_version() stays 10) op_layernorm_bwd for bf16 without GELU and without a row table that leaves out the rows of the
// samples stochastic depth dropped (see op_ln_geglu_fwd_skip for ps / rows_per_sample): nothing of dy, x, mean and rstd is read for such
// a row; dx gets +0 there, or with `add` the bits of the add row (dx may be add itself); dw / db get no contribution -- what
// op_layernorm_bwd gives for the exact-zero dy row the dense step has there, up to the sign of a zero in add.  Every other row, dw and
// db have op_layernorm_bwd's bits.  ps null: op_layernorm_bwd.
int op_layernorm_bwd_skip(const void* dy, const void* x, const void* w, const float* mean, const float* rstd, const void* add, void* dx,
                          void* dw, void* db, void* workspace, int64_t rows, int64_t cols, int accumulate, const float* ps,
                          int64_t rows_per_sample, void* stream) {
  if (!ps) return op_layernorm_bwd(dy, x, w, nullptr, mean, rstd, add, dx, dw, db, workspace, rows, cols, 0, accumulate, OP_DT_BF16, nullptr, stream);
  OP_CHECK_ARG(dy && x && dx && mean && rstd, "layernorm_bwd_skip: null pointer");
  OP_CHECK_ARG(rows >= 0 && cols > 0 && cols % 8 == 0, "layernorm_bwd_skip: cols=%lld must be a positive multiple of 8", (long long)cols);
  OP_CHECK_ARG(!(dw || db) || workspace, "layernorm_bwd_skip: dw/db requested without workspace");
  OP_CHECK_ARG(rows < ((int64_t)1 << 31) && rows_per_sample >= 1 && rows_per_sample < ((int64_t)1 << 31),
               "layernorm_bwd_skip: rows=%lld rows_per_sample=%lld", (long long)rows, (long long)rows_per_sample);
  if (rows == 0) return OP_OK;
  return ln_bwd_dispatch<bf16_t, false, true>(dy, x, w, nullptr, mean, rstd, add, dx, dw, db, (float*)workspace, rows, (int)cols, accumulate,
                                              (hipStream_t)stream, nullptr, ps, (int)rows_per_sample);
}

// y [rows, cols] = LayerNorm(bf16(gelu(h0) * h1)) (+ mean / rstd, nullable); h0, h1: row stride ldh (0 = cols).
int op_ln_geglu_fwd(const void* h0, const void* h1, int64_t ldh, const void* w, const void* b, void* y, float* mean, float* rstd,
                    int64_t rows, int64_t cols, float eps, void* stream) {
  OP_CHECK_ARG(h0 && h1 && y, "ln_geglu_fwd: null pointer");
  if (ldh <= 0) ldh = cols;
  OP_CHECK_ARG(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 8192 && ldh >= cols && ldh % 8 == 0, "ln_geglu_fwd: cols=%lld ldh=%lld unsupported",
               (long long)cols, (long long)ldh);
  if (rows == 0) return OP_OK;
  return ln_geglu_fwd_dispatch<false>(h0, h1, ldh, w, b, y, mean, rstd, nullptr, nullptr, rows, (int)cols, eps, (hipStream_t)stream);
}

// op_ln_geglu_fwd that also writes the row-quantised fp8 copy of its output (see op_layernorm_fwd_q8): the operand of the fp8 down-projection.
int op_ln_geglu_fwd_q8(const void* h0, const void* h1, int64_t ldh, const void* w, const void* b, void* y, float* mean, float* rstd, void* q8,
                       float* q8_scale, int64_t rows, int64_t cols, float eps, void* stream) {
  OP_CHECK_ARG(h0 && h1 && y && q8 && q8_scale, "ln_geglu_fwd_q8: null pointer");
  if (ldh <= 0) ldh = cols;
  OP_CHECK_ARG(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 8192 && ldh >= cols && ldh % 8 == 0, "ln_geglu_fwd_q8: cols=%lld ldh=%lld unsupported",
               (long long)cols, (long long)ldh);
  if (rows == 0) return OP_OK;
  return ln_geglu_fwd_dispatch<true>(h0, h1, ldh, w, b, y, mean, rstd, q8, q8_scale, rows, (int)cols, eps, (hipStream_t)stream);
}

// Backward of  y = LayerNorm_F(gelu(h0) * h1) * w + b  w.r.t. h0, h1, w, b in one pass (bf16 only); mean/rstd are the
// forward statistics of g = gelu(h0) * h1.  Replaces the LayerNorm backward + GeGLU backward pair of the FFN
// (one_peace/models/transformer/transformer_layer.py:64-67,111-118); g itself is not needed.
int op_ln_geglu_bwd(const void* dy, const void* h0, const void* h1, const void* w, const float* mean, const float* rstd,
                    void* dh0, void* dh1, int64_t ldd, int64_t ldh, void* dw, void* db, void* workspace, int64_t rows, int64_t cols,
                    int accumulate, void* stream) {
  OP_CHECK_ARG(dy && h0 && h1 && dh0 && dh1 && mean && rstd, "ln_geglu_bwd: null pointer");
  if (ldd <= 0) ldd = cols;
  if (ldh <= 0) ldh = cols;
  OP_CHECK_ARG(ldd >= cols && ldd % 8 == 0 && ldh >= cols && ldh % 8 == 0, "ln_geglu_bwd: row strides %lld / %lld", (long long)ldd, (long long)ldh);
  OP_CHECK_ARG(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 8192, "ln_geglu_bwd: cols=%lld unsupported", (long long)cols);
  OP_CHECK_ARG(!(dw || db) || workspace, "ln_geglu_bwd: dw/db requested without workspace");
  if (rows == 0) return OP_OK;
  float* wsk = (dw || db) ? (float*)workspace : nullptr;
  return ln_geglu_bwd_dispatch<false>(dy, h0, h1, w, mean, rstd, dh0, dh1, ldd, ldh, dw, db, wsk, rows, (int)cols, accumulate,
                                      (hipStream_t)stream);
}

// (additive: op_abi_version() stays 10) op_ln_geglu_fwd / op_ln_geglu_bwd that leave out the rows of the samples stochastic depth
// dropped: row r belongs to sample r / rows_per_sample (>= 1; a per-row vector: 1), and where ps[sample] == 0 NOTHING of the row is
// read -- h0 | h1 (and dy, mean, rstd in backward) may hold anything there.  Forward: y gets +0 in such a row, mean / rstd are not
// written.  Backward: dh0 | dh1 get +0, dw / db get no contribution -- what the plain entry gives for the exact-zero dy row the dense
// step has there.  Every other row has the plain entry's bits, and so have dw / db.  ps null: the plain entry.  rows < 2^31.
int op_ln_geglu_fwd_skip(const void* h0, const void* h1, int64_t ldh, const void* w, const void* b, void* y, float* mean, float* rstd,
                         int64_t rows, int64_t cols, float eps, const float* ps, int64_t rows_per_sample, void* stream) {
  if (!ps) return op_ln_geglu_fwd(h0, h1, ldh, w, b, y, mean, rstd, rows, cols, eps, stream);
  OP_CHECK_ARG(h0 && h1 && y, "ln_geglu_fwd_skip: null pointer");
  if (ldh <= 0) ldh = cols;
  OP_CHECK_ARG(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 8192 && ldh >= cols && ldh % 8 == 0, "ln_geglu_fwd_skip: cols=%lld ldh=%lld unsupported",
               (long long)cols, (long long)ldh);
  OP_CHECK_ARG(rows < ((int64_t)1 << 31) && rows_per_sample >= 1 && rows_per_sample < ((int64_t)1 << 31),
               "ln_geglu_fwd_skip: rows=%lld rows_per_sample=%lld", (long long)rows, (long long)rows_per_sample);
  if (rows == 0) return OP_OK;
  return ln_geglu_fwd_dispatch<false, true>(h0, h1, ldh, w, b, y, mean, rstd, nullptr, nullptr, rows, (int)cols, eps, (hipStream_t)stream,
                                            ps, (int)rows_per_sample);
}

int op_ln_geglu_bwd_skip(const void* dy, const void* h0, const void* h1, const void* w, const float* mean, const float* rstd,
                         void* dh0, void* dh1, int64_t ldd, int64_t ldh, void* dw, void* db, void* workspace, int64_t rows, int64_t cols,
                         int accumulate, const float* ps, int64_t rows_per_sample, void* stream) {
  if (!ps) return op_ln_geglu_bwd(dy, h0, h1, w, mean, rstd, dh0, dh1, ldd, ldh, dw, db, workspace, rows, cols, accumulate, stream);
  OP_CHECK_ARG(dy && h0 && h1 && dh0 && dh1 && mean && rstd, "ln_geglu_bwd_skip: null pointer");
  if (ldd <= 0) ldd = cols;
  if (ldh <= 0) ldh = cols;
  OP_CHECK_ARG(ldd >= cols && ldd % 8 == 0 && ldh >= cols && ldh % 8 == 0, "ln_geglu_bwd_skip: row strides %lld / %lld", (long long)ldd, (long long)ldh);
  OP_CHECK_ARG(rows >= 0 && cols > 0 && cols % 8 == 0 && cols <= 8192, "ln_geglu_bwd_skip: cols=%lld unsupported", (long long)cols);
  OP_CHECK_ARG(!(dw || db) || workspace, "ln_geglu_bwd_skip: dw/db requested without workspace");
  OP_CHECK_ARG(rows < ((int64_t)1 << 31) && rows_per_sample >= 1 && rows_per_sample < ((int64_t)1 << 31),
               "ln_geglu_bwd_skip: rows=%lld rows_per_sample=%lld", (long long)rows, (long long)rows_per_sample);
  if (rows == 0) return OP_OK;
  float* wsk = (dw || db) ? (float*)workspace : nullptr;
  return ln_geglu_bwd_dispatch<true>(dy, h0, h1, w, mean, rstd, dh0, dh1, ldd, ldh, dw, db, wsk, rows, (int)cols, accumulate,
                                     (hipStream_t)stream, ps, (int)rows_per_sample);
}

}  // extern "C"
