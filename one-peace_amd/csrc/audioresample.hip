// Sample-rate conversion of the hub's audio inputs (include/onepeace_hip.h: op_audio_resample).  Replaces the resampling half of
// librosa.load(path, sr=16000) in one_peace/models/one_peace/hub_interface.py:170-175 with a polyphase Kaiser-windowed sinc filter that
// is defined in closed form on the host (one-peace_amd/audioprep.py: resample_filter); the reference's soxr filter is a different low-pass.
//
// y[n] = L sum_j x[j] h[n M - j L] over 0 <= j < N, |n M - j L| <= half.  With q = floor(n M / L), p = n M - q L (the phase) and
// s = floor((half - p) / L), the terms are j = q - s + t for t = 0 ... T - 1 with the tap L h[p + (s - t) L]: row p of the coefficient
// table (audioprep.resample_taps; fp32(L h), zero where |p + (s - t) L| > half, zero-padded to Tp = 4 ceil(T / 4) taps so that a row is a
// whole number of 16-byte loads).  A thread's taps and its inputs are both unit-stride in t.
//
// ar_resample_kernel: workgroup = (AR_OUT consecutive outputs, clip).  It stages the input window of its outputs in LDS as fp32 mono --
// the channel mean and the int16 scale are applied while staging: s / 2^15, (l + r) / 2^16 (both exact), fl(l + r) * 0.5 -- with zeros
// for j outside [0, N), so nothing outside the clip is ever read.  Then every thread runs Tp fused multiply-adds over its row (four
// accumulators, one per component of the 16-byte tap load, summed as (a0 + a1) + (a2 + a3)) and stores one fp32.  The padding taps are
// exact zeros.  For L = 1 every thread reads the same row.  No atomics; an output depends on its clip's samples and its row only, not
// on the batch, the clip's position or the grid: two runs give the same bits.  n M is formed in 64 bits (it passes 2^31 after five
// minutes of 44.1 kHz audio).
#include "common.h"

#include <algorithm>

namespace {

constexpr int AR_THREADS = 256;
constexpr int AR_OUT = 256;     // outputs per workgroup, one per thread
constexpr int AR_WINDOW = 8192; // fp32 samples of the staged window: 32 KiB of LDS
constexpr int AR_DESC = 12;     // int64 per clip: src_off, frames, channels, format, L, M, T, half, coef_off, out_frames, dst_off, 0
constexpr int AR_FMT_S16 = 0;
constexpr int AR_FMT_F32 = 1;
constexpr int64_t AR_MAX_FRAMES = int64_t(1) << 27;
constexpr int64_t AR_MAX_L = 640;

// fp32 mono value of frame f: the first step of librosa.load(mono=True) / feats.mean(-1), as csrc/audioprep.hip forms it
template <int FMT, int CH> __device__ __forceinline__ float ar_frame(const uint8_t* clip, int64_t f) {
  if constexpr (FMT == AR_FMT_S16) {
    const short* p = reinterpret_cast<const short*>(clip) + f * CH;
    return CH == 1 ? (float)(int)p[0] * 0x1p-15f : (float)((int)p[0] + (int)p[1]) * 0x1p-16f;
  } else {
    const float* p = reinterpret_cast<const float*>(clip) + f * CH;
    return CH == 1 ? p[0] : (p[0] + p[1]) * 0.5f;
  }
}

template <int FMT, int CH>
__device__ __forceinline__ void ar_stage(const uint8_t* clip, int64_t n_in, int64_t jlo, int count, float* win) {
  for (int i = threadIdx.x; i < count; i += AR_THREADS) {
    const int64_t j = jlo + i;
    win[i] = (j >= 0 && j < n_in) ? ar_frame<FMT, CH>(clip, j) : 0.f;
  }
}

__global__ __launch_bounds__(AR_THREADS) void ar_resample_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                                                 const float* __restrict__ coef, uint8_t* __restrict__ out) {
  __shared__ float win[AR_WINDOW];
  const int64_t* d = desc + (int64_t)blockIdx.y * AR_DESC;
  const int64_t n_out = d[9], n0 = (int64_t)blockIdx.x * AR_OUT;
  if (n0 >= n_out) return;  // uniform over the block
  const int64_t n_in = d[1], L = d[4], M = d[5], half = d[7];
  const int ch = (int)d[2], fmt = (int)d[3], Tp = ((int)d[6] + 3) & ~3;
  const uint8_t* clip = src + d[0];
  const int64_t nl = min(n0 + AR_OUT - 1, n_out - 1);
  const int64_t q0 = n0 * M / L, ql = nl * M / L, K = half / L;
  const int64_t jlo = q0 - K;  // s <= K: the first input of any output of the block
  // K - 1 <= s, so the last input is at most ql - (K - 1) + Tp - 1; the host checked that this fits the window
  const int count = (int)min(ql - q0 + Tp + 1, (int64_t)AR_WINDOW);
  if (fmt == AR_FMT_S16) {
    if (ch == 1) ar_stage<AR_FMT_S16, 1>(clip, n_in, jlo, count, win);
    else ar_stage<AR_FMT_S16, 2>(clip, n_in, jlo, count, win);
  } else {
    if (ch == 1) ar_stage<AR_FMT_F32, 1>(clip, n_in, jlo, count, win);
    else ar_stage<AR_FMT_F32, 2>(clip, n_in, jlo, count, win);
  }
  __syncthreads();
  const int64_t n = n0 + threadIdx.x;
  if (n >= n_out) return;
  const int64_t nm = n * M, q = nm / L, p = nm - q * L, s = (half - p) / L;
  const int base = (int)(q - q0 + K - s);  // 0 <= base, base + Tp <= count
  const f32x4* row = reinterpret_cast<const f32x4*>(coef + d[8] + p * Tp);
  const float* x = win + base;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 4
  for (int t = 0; t < Tp / 4; ++t) {
    const f32x4 c = row[t];
    a0 = __builtin_fmaf(x[4 * t], c.x, a0);
    a1 = __builtin_fmaf(x[4 * t + 1], c.y, a1);
    a2 = __builtin_fmaf(x[4 * t + 2], c.z, a2);
    a3 = __builtin_fmaf(x[4 * t + 3], c.w, a3);
  }
  reinterpret_cast<float*>(out + d[10])[n] = (a0 + a1) + (a2 + a3);
}

}  // namespace

extern "C" int op_audio_resample(const void* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int64_t B,
                                 const float* coef, int64_t coef_count, void* out, int64_t out_bytes, void* stream) {
  OP_CHECK_ARG(B >= 0 && B <= 65535, "op_audio_resample: B = %lld, need 0 ... 65535", (long long)B);
  if (B == 0) return OP_OK;
  OP_CHECK_ARG(src && desc && desc_host && coef && out, "op_audio_resample: null pointer");
  OP_CHECK_ARG(((uintptr_t)src & 15) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)coef & 15) == 0 && ((uintptr_t)desc & 7) == 0,
               "op_audio_resample: src, coef and out must be 16-byte aligned, desc 8-byte aligned");
  OP_CHECK_ARG(src_bytes >= 0 && coef_count >= 0 && out_bytes >= 0, "op_audio_resample: negative size");
  int64_t max_blocks = 0;
  for (int64_t i = 0; i < B; ++i) {
    const int64_t* d = desc_host + i * AR_DESC;
    const int64_t src_off = d[0], n = d[1], ch = d[2], fmt = d[3], L = d[4], M = d[5], T = d[6], half = d[7], coef_off = d[8], n_out = d[9],
                  dst_off = d[10];
    OP_CHECK_ARG(n >= 1 && n <= AR_MAX_FRAMES, "op_audio_resample: clip %lld has %lld frames, need 1 ... 2^27", (long long)i, (long long)n);
    OP_CHECK_ARG(ch == 1 || ch == 2, "op_audio_resample: clip %lld has %lld channels, need 1 or 2", (long long)i, (long long)ch);
    OP_CHECK_ARG(fmt == AR_FMT_S16 || fmt == AR_FMT_F32, "op_audio_resample: clip %lld: sample format %lld, need 0 (int16) or 1 (f32)",
                 (long long)i, (long long)fmt);
    const int64_t bytes = n * ch * (fmt == AR_FMT_S16 ? 2 : 4);
    OP_CHECK_ARG(src_off >= 0 && src_off % 16 == 0 && src_off <= src_bytes && bytes <= src_bytes - src_off,
                 "op_audio_resample: clip %lld (offset %lld, a multiple of 16; %lld bytes) overruns src (%lld bytes)", (long long)i,
                 (long long)src_off, (long long)bytes, (long long)src_bytes);
    OP_CHECK_ARG(L >= 1 && L <= AR_MAX_L && M >= 1 && M <= (int64_t(1) << 24),
                 "op_audio_resample: clip %lld: ratio L / M = %lld / %lld, need 1 <= L <= 640 and 1 <= M <= 2^24", (long long)i, (long long)L,
                 (long long)M);
    OP_CHECK_ARG(half >= L && half <= (int64_t(1) << 24) && T == 2 * half / L + 1,
                 "op_audio_resample: clip %lld: half = %lld, taps T = %lld, need L <= half <= 2^24 and T = floor(2 half / L) + 1",
                 (long long)i, (long long)half, (long long)T);
    const int64_t Tp = (T + 3) / 4 * 4;
    OP_CHECK_ARG((AR_OUT - 1) * M / L + Tp + 2 <= AR_WINDOW,
                 "op_audio_resample: clip %lld: the window of %d outputs, floor(%d M / L) + 4 ceil(T / 4) + 2 = %lld samples, exceeds %d",
                 (long long)i, AR_OUT, AR_OUT - 1, (long long)((AR_OUT - 1) * M / L + Tp + 2), AR_WINDOW);
    OP_CHECK_ARG(coef_off >= 0 && coef_off % 4 == 0 && coef_off <= coef_count && L * Tp <= coef_count - coef_off,
                 "op_audio_resample: clip %lld: the table at coef_off = %lld (a multiple of 4) of %lld x %lld taps overruns coef (%lld)",
                 (long long)i, (long long)coef_off, (long long)L, (long long)Tp, (long long)coef_count);
    OP_CHECK_ARG(n_out == (n * L + M - 1) / M && n_out <= AR_MAX_FRAMES,
                 "op_audio_resample: clip %lld: out_frames = %lld, need ceil(frames L / M) = %lld <= 2^27", (long long)i, (long long)n_out,
                 (long long)((n * L + M - 1) / M));
    OP_CHECK_ARG(dst_off >= 0 && dst_off % 16 == 0 && dst_off <= out_bytes && n_out * 4 <= out_bytes - dst_off,
                 "op_audio_resample: clip %lld: output (offset %lld, a multiple of 16; %lld bytes) overruns out (%lld bytes)", (long long)i,
                 (long long)dst_off, (long long)(n_out * 4), (long long)out_bytes);
    max_blocks = std::max(max_blocks, (n_out + AR_OUT - 1) / AR_OUT);
  }
  hipLaunchKernelGGL(ar_resample_kernel, dim3((unsigned)max_blocks, (unsigned)B), dim3(AR_THREADS), 0, (hipStream_t)stream,
                     (const uint8_t*)src, desc, coef, (uint8_t*)out);
  OP_LAUNCH_CHECK();
  return OP_OK;
}
