// Audio pre-processing of the hub and the datasets (include/onepeace_hip.h: op_audio_normalize_pad).  Replaces the host loop of
// one_peace/models/one_peace/hub_interface.py:170-193 and data/base_dataset.py:84-102 (audio_postprocess) -- channel mean, F.layer_norm
// over the WHOLE clip, crop to max_len, repeat the normalised clip up to min_len, right-pad with zeros, cast -- for a batch of decoded
// clips (int16 PCM or fp32 samples, 1 or 2 interleaved channels) of different lengths.
//
// ap_stats_kernel: workgroup = (chunk of AP_CHUNK frames, clip).  It writes one 16-byte partial per chunk.
//   int16: {sum u, sum u^2} as int64, u = s (mono, value u / 2^15) or l + r (stereo, value u / 2^16): exact.
//   fp32:  {mean_c, M2_c} as fp64, accumulated as sum d, sum d^2 with d = x - p around the pivot p = the chunk's FIRST frame.  The pivot
//          is a member of the chunk, so sum d^2 <= (cnt + 1) M2_c and the subtraction sum d^2 - (sum d)^2 / cnt loses at most
//          log2(cnt + 1) = 13 of fp64's 53 bits, whatever the offset of the signal.
// ap_normalize_kernel: workgroup = (chunk of AP_CHUNK output samples, clip).  It re-merges the clip's partials in a fixed order (lane-
//   strided sums, a shuffle tree, the four waves in sequence) -- integers for int16; for fp32 mean = sum cnt_c mean_c / n, then
//   M2 = sum (M2_c + cnt_c (mean_c - mean)^2), every term non-negative -- forms mean and rstd = 1 / sqrt(M2 / n + 1e-5) once in fp64,
//   rounds both to fp32 and writes (x - mean) * rstd: one subtraction and one multiplication per sample, no contraction possible.
// Nothing depends on B, T or the clip's position: the chunk size is a constant, there are no atomics, and a sample's value is formed by
// the same two operations on the vector path, the scalar head / tail path and the tiling path.
// Output addresses: 16-byte groups are counted from `out` itself (row b starts at element b T, which need not be a multiple of the group),
// so every group inside a block's range is one 16-byte store; the groups a range cuts are written element by element by the two blocks
// that share them.  The source frames of a group are one run in memory unless the clip is tiled; they are read with vector loads of the
// frame's natural alignment (gfx950 serves an unaligned dwordx4 from global memory).
#include "common.h"

#include <algorithm>

namespace {

constexpr int AP_THREADS = 256;
constexpr int AP_CHUNK = 8192;  // frames per statistics partial and output samples per normalise block: a constant of the kernel
constexpr int AP_DESC = 6;      // int64 per clip: src_off, frames, channels, format, out_len, part_off
constexpr int AP_FMT_S16 = 0;
constexpr int AP_FMT_F32 = 1;
constexpr int64_t AP_MAX_FRAMES = int64_t(1) << 27;

struct alignas(16) ApPartial {
  int64_t a, b;  // int16: sum u, sum u^2; fp32: the bits of the doubles mean_c, M2_c
};

template <int FMT, int CH> struct ApFrame {
  static constexpr int BYTES = (FMT == AP_FMT_S16 ? 2 : 4) * CH;
  static constexpr int PER16 = 16 / BYTES;  // frames per 16-byte load
};

__device__ __forceinline__ int ap_lo16(unsigned w) { return (int)(short)(w & 0xffffu); }
__device__ __forceinline__ int ap_hi16(unsigned w) { return (int)w >> 16; }

// NW dwords from p, which is aligned to ALIGN bytes only
template <int NW, int ALIGN> __device__ __forceinline__ void ap_load_words(const uint8_t* p, unsigned (&w)[NW]) {
  if constexpr (NW == 2) {
    u32x2 v;
    __builtin_memcpy(&v, __builtin_assume_aligned(p, ALIGN < 8 ? ALIGN : 8), 8);
    w[0] = v.x, w[1] = v.y;
  } else {
#pragma unroll
    for (int j = 0; j < NW / 4; ++j) {
      u32x4 v;
      __builtin_memcpy(&v, __builtin_assume_aligned(p + 16 * j, ALIGN), 16);
      w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
    }
  }
}

// the integer u of K int16 frames (mono: the sample; stereo: l + r)
template <int CH, int K> __device__ __forceinline__ void ap_ints(const unsigned (&w)[K * CH / 2], int (&u)[K]) {
#pragma unroll
  for (int j = 0; j < K * CH / 2; ++j) {
    if constexpr (CH == 1)
      u[2 * j] = ap_lo16(w[j]), u[2 * j + 1] = ap_hi16(w[j]);
    else
      u[j] = ap_lo16(w[j]) + ap_hi16(w[j]);
  }
}

// the fp32 mono values of K frames from f on: step 1 of audio_postprocess.  int16: u / 2^15 or (l + r) / 2^16, exact; fp32 stereo:
// fl(l + r) * 0.5, which is feats.mean(-1)
template <int FMT, int CH, int K, int ALIGN> __device__ __forceinline__ void ap_frames(const uint8_t* clip, int64_t f, float (&x)[K]) {
  constexpr int NW = K * ApFrame<FMT, CH>::BYTES / 4;
  unsigned w[NW];
  ap_load_words<NW, ALIGN>(clip + f * ApFrame<FMT, CH>::BYTES, w);
  if constexpr (FMT == AP_FMT_S16) {
    int u[K];
    ap_ints<CH, K>(w, u);
#pragma unroll
    for (int j = 0; j < K; ++j) x[j] = (float)u[j] * (CH == 1 ? 0x1p-15f : 0x1p-16f);
  } else {
#pragma unroll
    for (int j = 0; j < K; ++j)
      x[j] = CH == 1 ? __uint_as_float(w[j]) : (__uint_as_float(w[2 * j]) + __uint_as_float(w[2 * j + 1])) * 0.5f;
  }
}

template <int FMT, int CH> __device__ __forceinline__ int ap_int1(const uint8_t* clip, int64_t f) {
  const short* p = reinterpret_cast<const short*>(clip) + f * CH;
  return CH == 1 ? (int)p[0] : (int)p[0] + (int)p[1];
}

template <int FMT, int CH> __device__ __forceinline__ float ap_frame1(const uint8_t* clip, int64_t f) {
  if constexpr (FMT == AP_FMT_S16) {
    return (float)ap_int1<FMT, CH>(clip, f) * (CH == 1 ? 0x1p-15f : 0x1p-16f);
  } else {
    const float* p = reinterpret_cast<const float*>(clip) + f * CH;
    return CH == 1 ? p[0] : (p[0] + p[1]) * 0.5f;
  }
}

// the block's sum in every thread, in a fixed order: shuffle tree per wave, then wave 0 + 1 + 2 + 3
template <typename T> __device__ __forceinline__ T ap_block_sum(T v, T* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  __syncthreads();  // the previous call's readers are done with lds
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  T s = lds[0];
#pragma unroll
  for (int w = 1; w < AP_THREADS / 64; ++w) s += lds[w];
  return s;
}

__device__ __forceinline__ double ap_as_double(int64_t v) { return __longlong_as_double(v); }
__device__ __forceinline__ int64_t ap_as_int(double v) { return __double_as_longlong(v); }

template <int FMT, int CH>
__device__ __forceinline__ void ap_stats_chunk(const uint8_t* clip, int64_t f0, int cnt, ApPartial* out, void* lds) {
  constexpr int K = ApFrame<FMT, CH>::PER16;
  const int tid = threadIdx.x, nvec = cnt / K;
  if constexpr (FMT == AP_FMT_S16) {
    int64_t s = 0, q = 0;
    for (int v = tid; v < nvec; v += AP_THREADS) {
      unsigned w[4];
      int u[K];
      ap_load_words<4, 16>(clip + (f0 + (int64_t)v * K) * ApFrame<FMT, CH>::BYTES, w);
      ap_ints<CH, K>(w, u);
#pragma unroll
      for (int j = 0; j < K; ++j) s += u[j], q += (int64_t)u[j] * u[j];
    }
    for (int r = nvec * K + tid; r < cnt; r += AP_THREADS) {
      const int u = ap_int1<FMT, CH>(clip, f0 + r);
      s += u, q += (int64_t)u * u;
    }
    s = ap_block_sum(s, reinterpret_cast<int64_t*>(lds));
    q = ap_block_sum(q, reinterpret_cast<int64_t*>(lds));
    if (tid == 0) out->a = s, out->b = q;
  } else {
    const double p = (double)ap_frame1<FMT, CH>(clip, f0);
    double s = 0.0, q = 0.0;
    for (int v = tid; v < nvec; v += AP_THREADS) {
      float x[K];
      ap_frames<FMT, CH, K, 16>(clip, f0 + (int64_t)v * K, x);
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double d = (double)x[j] - p;
        s += d, q = fma(d, d, q);
      }
    }
    for (int r = nvec * K + tid; r < cnt; r += AP_THREADS) {
      const double d = (double)ap_frame1<FMT, CH>(clip, f0 + r) - p;
      s += d, q = fma(d, d, q);
    }
    s = ap_block_sum(s, reinterpret_cast<double*>(lds));
    q = ap_block_sum(q, reinterpret_cast<double*>(lds));
    if (tid == 0) {
      out->a = ap_as_int(p + s / (double)cnt);
      out->b = ap_as_int(fmax(q - s * s / (double)cnt, 0.0));
    }
  }
}

__global__ __launch_bounds__(AP_THREADS) void ap_stats_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                                              ApPartial* __restrict__ part) {
  __shared__ int64_t lds[AP_THREADS / 64];
  const int64_t* d = desc + (int64_t)blockIdx.y * AP_DESC;
  const int64_t n = d[1], f0 = (int64_t)blockIdx.x * AP_CHUNK;
  if (f0 >= n) return;
  const uint8_t* clip = src + d[0];
  const int cnt = (int)min((int64_t)AP_CHUNK, n - f0), ch = (int)d[2], fmt = (int)d[3];
  ApPartial* out = part + d[5] + blockIdx.x;
  if (fmt == AP_FMT_S16) {
    if (ch == 1) ap_stats_chunk<AP_FMT_S16, 1>(clip, f0, cnt, out, lds);
    else ap_stats_chunk<AP_FMT_S16, 2>(clip, f0, cnt, out, lds);
  } else {
    if (ch == 1) ap_stats_chunk<AP_FMT_F32, 1>(clip, f0, cnt, out, lds);
    else ap_stats_chunk<AP_FMT_F32, 2>(clip, f0, cnt, out, lds);
  }
}

// mean and rstd of a clip from its partials, the same in every thread and in every block of the clip
__device__ __forceinline__ void ap_merge(const ApPartial* __restrict__ part, int64_t n, int ch, int fmt, void* lds, float& mean, float& rstd) {
  const int nchunks = (int)((n + AP_CHUNK - 1) / AP_CHUNK);
  double m, var;
  if (fmt == AP_FMT_S16) {
    int64_t s = 0, q = 0;
    for (int c = threadIdx.x; c < nchunks; c += AP_THREADS) s += part[c].a, q += part[c].b;
    s = ap_block_sum(s, reinterpret_cast<int64_t*>(lds));
    q = ap_block_sum(q, reinterpret_cast<int64_t*>(lds));
    // n q - s^2 >= 0 in 128 bits (q < 2^59, |s| < 2^44), then two fp64 roundings
    const uint64_t un = (uint64_t)n, uq = (uint64_t)q, us = (uint64_t)(s < 0 ? -s : s);
    const uint64_t nq_lo = un * uq, nq_hi = __umul64hi(un, uq), ss_lo = us * us, ss_hi = __umul64hi(us, us);
    const uint64_t lo = nq_lo - ss_lo, hi = nq_hi - ss_hi - (nq_lo < ss_lo ? 1 : 0);
    const double num = (double)hi * 18446744073709551616.0 + (double)lo;
    const double scale = ch == 1 ? 0x1p-15 : 0x1p-16;
    m = (double)s / (double)n * scale;
    var = num / (double)n / (double)n * (scale * scale);
  } else {
    double a = 0.0;
    for (int c = threadIdx.x; c < nchunks; c += AP_THREADS) {
      const double cnt = (double)min((int64_t)AP_CHUNK, n - (int64_t)c * AP_CHUNK);
      a = fma(cnt, ap_as_double(part[c].a), a);
    }
    m = ap_block_sum(a, reinterpret_cast<double*>(lds)) / (double)n;
    double b = 0.0;
    for (int c = threadIdx.x; c < nchunks; c += AP_THREADS) {
      const double cnt = (double)min((int64_t)AP_CHUNK, n - (int64_t)c * AP_CHUNK);
      const double dm = ap_as_double(part[c].a) - m;
      b += ap_as_double(part[c].b) + cnt * dm * dm;
    }
    var = ap_block_sum(b, reinterpret_cast<double*>(lds)) / (double)n;
  }
  mean = (float)m;
  rstd = (float)(1.0 / sqrt(var + 1e-5));
}

template <typename OutT> __device__ __forceinline__ OutT ap_cast(float v) { return (OutT)v; }  // bf16: round-to-nearest-even

template <int FMT, int CH, typename OutT>
__device__ __forceinline__ void ap_write(const uint8_t* clip, int64_t ncrop, int64_t L, float mean, float rstd, OutT* __restrict__ out,
                                         int64_t row0, int64_t t0, int64_t t1) {
  constexpr int VEC = 16 / (int)sizeof(OutT);
  typedef OutT OutV __attribute__((ext_vector_type(VEC)));
  const int64_t g0 = row0 + t0, g1 = row0 + t1;
  const int64_t G1 = (g1 + VEC - 1) / VEC;
  for (int64_t G = g0 / VEC + threadIdx.x; G < G1; G += AP_THREADS) {
    const int64_t ge = G * VEC, t = ge - row0;
    const bool whole = ge >= g0 && ge + VEC <= g1;
    float y[VEC];
    if (whole && t + VEC <= ncrop) {  // the main path: VEC source frames in a row
      ap_frames<FMT, CH, VEC, ApFrame<FMT, CH>::BYTES>(clip, t, y);
#pragma unroll
      for (int j = 0; j < VEC; ++j) y[j] = (y[j] - mean) * rstd;
    } else {  // the groups a block's range cuts, the clip's end, tiled samples (frame t mod ncrop) and the zero padding
#pragma unroll
      for (int j = 0; j < VEC; ++j) {
        const int64_t tt = t + j;
        y[j] = 0.f;
        if (tt >= t0 && tt < t1 && tt < L) {
          const int64_t f = tt < ncrop ? tt : (int64_t)((unsigned)tt % (unsigned)ncrop);
          y[j] = (ap_frame1<FMT, CH>(clip, f) - mean) * rstd;
        }
      }
    }
    if (whole) {
      OutV r;
#pragma unroll
      for (int j = 0; j < VEC; ++j) r[j] = ap_cast<OutT>(y[j]);
      *reinterpret_cast<OutV*>(out + ge) = r;
    } else {
#pragma unroll
      for (int j = 0; j < VEC; ++j)
        if (ge + j >= g0 && ge + j < g1) out[ge + j] = ap_cast<OutT>(y[j]);
    }
  }
}

template <typename OutT>
__global__ __launch_bounds__(AP_THREADS) void ap_normalize_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                                                  const ApPartial* __restrict__ part, OutT* __restrict__ out, int64_t T,
                                                                  int64_t max_len) {
  __shared__ int64_t lds[AP_THREADS / 64];
  const int64_t* d = desc + (int64_t)blockIdx.y * AP_DESC;
  const int64_t n = d[1], L = d[4];
  const int ch = (int)d[2], fmt = (int)d[3];
  const int64_t t0 = (int64_t)blockIdx.x * AP_CHUNK, t1 = min(t0 + AP_CHUNK, T);
  const int64_t ncrop = min(n, max_len), row0 = (int64_t)blockIdx.y * T;
  const uint8_t* clip = src + d[0];
  float mean = 0.f, rstd = 0.f;
  if (t0 < L) ap_merge(part + d[5], n, ch, fmt, lds, mean, rstd);  // uniform over the block; blocks of pure padding skip it
  if (fmt == AP_FMT_S16) {
    if (ch == 1) ap_write<AP_FMT_S16, 1, OutT>(clip, ncrop, L, mean, rstd, out, row0, t0, t1);
    else ap_write<AP_FMT_S16, 2, OutT>(clip, ncrop, L, mean, rstd, out, row0, t0, t1);
  } else {
    if (ch == 1) ap_write<AP_FMT_F32, 1, OutT>(clip, ncrop, L, mean, rstd, out, row0, t0, t1);
    else ap_write<AP_FMT_F32, 2, OutT>(clip, ncrop, L, mean, rstd, out, row0, t0, t1);
  }
}

}  // namespace

extern "C" int op_audio_normalize_pad(const void* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int64_t B,
                                      int64_t max_len, int64_t min_len, void* out, int64_t T, int out_dtype, void* workspace,
                                      int64_t workspace_bytes, void* stream) {
  OP_CHECK_ARG(B >= 0 && B <= 65535, "op_audio_normalize_pad: B = %lld, need 0 ... 65535", (long long)B);
  OP_CHECK_ARG(out_dtype == OP_DT_BF16 || out_dtype == OP_DT_F32, "op_audio_normalize_pad: out_dtype = %d, need 0 (bf16) or 1 (f32)",
               out_dtype);
  OP_CHECK_ARG(max_len >= 1 && max_len <= AP_MAX_FRAMES && min_len >= 0 && min_len <= max_len,
               "op_audio_normalize_pad: max_len = %lld, min_len = %lld, need 0 <= min_len <= max_len, 1 <= max_len <= 2^27",
               (long long)max_len, (long long)min_len);
  OP_CHECK_ARG(T >= 0 && T <= AP_MAX_FRAMES, "op_audio_normalize_pad: T = %lld, need 0 ... 2^27", (long long)T);
  if (B == 0) return OP_OK;
  OP_CHECK_ARG(src && desc && desc_host && out && workspace, "op_audio_normalize_pad: null pointer");
  OP_CHECK_ARG(((uintptr_t)src & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)desc & 7) == 0,
               "op_audio_normalize_pad: src, out and workspace must be 16-byte aligned, desc 8-byte aligned");
  int64_t chunks = 0, max_chunks = 0;
  for (int64_t i = 0; i < B; ++i) {
    const int64_t* d = desc_host + i * AP_DESC;
    const int64_t src_off = d[0], n = d[1], ch = d[2], fmt = d[3], L = d[4], part_off = d[5];
    OP_CHECK_ARG(n >= 1 && n <= AP_MAX_FRAMES, "op_audio_normalize_pad: clip %lld has %lld frames, need 1 ... 2^27", (long long)i,
                 (long long)n);
    OP_CHECK_ARG(ch == 1 || ch == 2, "op_audio_normalize_pad: clip %lld has %lld channels, need 1 or 2", (long long)i, (long long)ch);
    OP_CHECK_ARG(fmt == AP_FMT_S16 || fmt == AP_FMT_F32, "op_audio_normalize_pad: clip %lld: sample format %lld, need 0 (int16) or 1 (f32)",
                 (long long)i, (long long)fmt);
    const int64_t bytes = n * ch * (fmt == AP_FMT_S16 ? 2 : 4);
    OP_CHECK_ARG(src_off >= 0 && src_off % 16 == 0 && src_off <= src_bytes && bytes <= src_bytes - src_off,
                 "op_audio_normalize_pad: clip %lld (offset %lld, a multiple of 16; %lld bytes) overruns src (%lld bytes)", (long long)i,
                 (long long)src_off, (long long)bytes, (long long)src_bytes);
    OP_CHECK_ARG(L == std::max(std::min(n, max_len), min_len) && L <= T,
                 "op_audio_normalize_pad: clip %lld: out_len = %lld, need max(min(frames, max_len), min_len) = %lld <= T = %lld",
                 (long long)i, (long long)L, (long long)std::max(std::min(n, max_len), min_len), (long long)T);
    OP_CHECK_ARG(part_off == chunks, "op_audio_normalize_pad: clip %lld: part_off = %lld, need the running sum of ceil(frames / %d) = %lld",
                 (long long)i, (long long)part_off, AP_CHUNK, (long long)chunks);
    const int64_t c = (n + AP_CHUNK - 1) / AP_CHUNK;
    chunks += c;
    max_chunks = std::max(max_chunks, c);
  }
  OP_CHECK_ARG(chunks * (int64_t)sizeof(ApPartial) <= workspace_bytes,
               "op_audio_normalize_pad: workspace of %lld bytes, need %lld (16 per %d frames of each clip)", (long long)workspace_bytes,
               (long long)(chunks * (int64_t)sizeof(ApPartial)), AP_CHUNK);
  hipStream_t st = (hipStream_t)stream;
  const uint8_t* s = (const uint8_t*)src;
  ApPartial* part = (ApPartial*)workspace;
  hipLaunchKernelGGL(ap_stats_kernel, dim3((unsigned)max_chunks, (unsigned)B), dim3(AP_THREADS), 0, st, s, desc, part);
  OP_LAUNCH_CHECK();
  const dim3 grid((unsigned)((T + AP_CHUNK - 1) / AP_CHUNK), (unsigned)B);
  if (out_dtype == OP_DT_BF16)
    hipLaunchKernelGGL(ap_normalize_kernel<bf16_t>, grid, dim3(AP_THREADS), 0, st, s, desc, part, (bf16_t*)out, T, max_len);
  else
    hipLaunchKernelGGL(ap_normalize_kernel<float>, grid, dim3(AP_THREADS), 0, st, s, desc, part, (float*)out, T, max_len);
  OP_LAUNCH_CHECK();
  return OP_OK;
}
