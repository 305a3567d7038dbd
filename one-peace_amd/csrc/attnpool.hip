// Single-query attention pooling (include/onepeace_hip.h: op_attn_pool_fwd, op_attn_pool_bwd): the device computation of the
// fine-tuning head, MultiheadAttentionPooling.forward of one_peace/models/one_peace/one_peace_base.py:154-170 between the K / V
// projections and out_proj.  One learned query per head attends over the S keys of a sample; there is no 1 / sqrt(hd) factor (:157-160).
//
// Both kernels: one workgroup of 256 lanes per (sample, head).  G = the power of two >= hd / 8 lanes share a key, each holding 8
// adjacent columns (one 16-byte load of k or v); 256 / G keys are in flight per pass, four passes are issued back to back.  Lanes whose
// columns lie past hd (hd / 8 no power of two) load and store nothing.  The row of scores / probabilities lives in LDS (S <= 4096).
//   forward   scores q_h . k_s (fp32, butterfly over the G lanes) -> LDS; row maximum; e_s = expf(score - max), their sum; p_s = e_s / sum
//             -> LDS and p [B, heads, S]; out = sum_s p_s v_s in fp32 per lane, folded over the key groups (wave butterfly, then the four
//             waves in order) and rounded to bf16 once.
//   backward  dp_s = dout_h . v_s and dv_s = p_s dout_h in one pass over v (c = sum_s p_s dp_s folded over the workgroup); then
//             ds_s = p_s (dp_s - c), dk_s = ds_s q_h and dq_part[b, h] = sum_s ds_s k_s in one pass over k.
// Every sum has a fixed order (a lane's strided partial, shuffles, the waves in order): no atomics, two runs give the same bits, and a
// sample's results do not depend on the batch it is launched in.
// Masked keys (pad != 0) are SKIPPED: p = 0 exactly, their rows of k and v are never read, their rows of dk and dv are written as zeros.
// The backward recognises them by p == 0 (which also covers a live key whose exponential underflowed: all its terms are zero).  The
// reference multiplies by zero instead (torch.bmm), so there a non-finite value in a masked row of k or v reaches the output; here it
// does not.  A sample whose keys are ALL masked gives 0 / 0 = NaN in p, out and every gradient of that sample, as in the reference.
#include "common.h"

#include <math.h>

namespace {

constexpr int AP_THREADS = 256;
constexpr int AP_MAX_S = 4096;  // keys of a sample: one fp32 row in LDS (16 KiB; the backward holds two)
constexpr int AP_U = 4;         // passes issued back to back (independent 16-byte loads in flight per lane)

__device__ __forceinline__ float ap_block_max(float v, float* red4) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(red4[0], red4[1]), fmaxf(red4[2], red4[3]));
  __syncthreads();
  return v;
}

__device__ __forceinline__ float ap_block_sum(float v, float* red4) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = v;
  __syncthreads();
  v = ((red4[0] + red4[1]) + red4[2]) + red4[3];
  __syncthreads();
  return v;
}

// sum over the G lanes that share a key (adjacent lanes of one wave)
template <int G> __device__ __forceinline__ float ap_group_sum(float v) {
#pragma unroll
  for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// acc[0..8) summed over the 256 / G key groups of the workgroup: the lanes of a wave that hold the same columns, then the four waves in
// order.  The result is valid in the lanes tid < G.  red: 4 * G * 8 floats.
template <int G> __device__ __forceinline__ void ap_fold_keys(float (&acc)[8], float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
#pragma unroll
    for (int o = G; o < 64; o <<= 1) acc[j] += __shfl_xor(acc[j], o);
  }
  if (lane < G) {
#pragma unroll
    for (int j = 0; j < 8; ++j) red[(wave * G + lane) * 8 + j] = acc[j];
  }
  __syncthreads();
  if (tid < G) {
#pragma unroll
    for (int j = 0; j < 8; ++j)
      acc[j] = ((red[tid * 8 + j] + red[(G + tid) * 8 + j]) + red[(2 * G + tid) * 8 + j]) + red[(3 * G + tid) * 8 + j];
  }
}

__device__ __forceinline__ float ap_dot8(const bf16x8& r, const float (&w)[8]) {
  float d = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) d = fmaf((float)r[j], w[j], d);
  return d;
}

__device__ __forceinline__ bf16x8 ap_zero8() {
  bf16x8 z;
#pragma unroll
  for (int j = 0; j < 8; ++j) z[j] = (bf16_t)0.f;
  return z;
}

__device__ __forceinline__ void ap_store8(bf16_t* p, const float (&w)[8], float a) {  // p[0..8) = bf16(a * w)
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (bf16_t)(a * w[j]);
  *reinterpret_cast<bf16x8*>(p) = r;
}

template <int G>
__global__ __launch_bounds__(AP_THREADS) void attn_pool_fwd_kernel(const bf16_t* __restrict__ k, const bf16_t* __restrict__ v, int64_t ld,
                                                                   int64_t batch_stride, const bf16_t* __restrict__ q,
                                                                   const uint8_t* __restrict__ pad, int64_t ld_pad,
                                                                   bf16_t* __restrict__ out, float* __restrict__ p, int S, int heads,
                                                                   int hd) {
  constexpr int KP = AP_THREADS / G;  // keys per pass
  __shared__ __align__(16) float sc[AP_MAX_S];
  __shared__ __align__(16) float red[4 * G * 8];
  __shared__ float red4[4];
  const int tid = threadIdx.x, c = tid & (G - 1), kg = tid / G;
  const int64_t b = blockIdx.x / heads;
  const int h = blockIdx.x % heads;
  const bool live = c * 8 < hd;
  const int64_t col = (int64_t)h * hd + c * 8;
  const bf16_t* __restrict__ kb = k + b * batch_stride + col;
  const bf16_t* __restrict__ vb = v + b * batch_stride + col;
  const uint8_t* __restrict__ pb = pad ? pad + b * ld_pad : nullptr;
  float qv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) qv[j] = 0.f;
  if (live) Vec8<bf16_t>::load(q + col, qv);

  // scores -> sc (a masked key: -inf), the row maximum over the live keys
  const float ninf = -__builtin_inff();
  float mx = ninf;
  for (int s0 = 0; s0 < S; s0 += KP * AP_U) {
    bf16x8 raw[AP_U];
    bool on[AP_U];
#pragma unroll
    for (int u = 0; u < AP_U; ++u) {
      const int s = s0 + u * KP + kg;
      on[u] = s < S && !(pb && pb[s]);
      raw[u] = ap_zero8();
      if (on[u] && live) raw[u] = *reinterpret_cast<const bf16x8*>(kb + (int64_t)s * ld);
    }
#pragma unroll
    for (int u = 0; u < AP_U; ++u) {
      const int s = s0 + u * KP + kg;
      const float d = ap_group_sum<G>(ap_dot8(raw[u], qv));
      if (on[u]) mx = fmaxf(mx, d);
      if (c == 0 && s < S) sc[s] = on[u] ? d : ninf;
    }
  }
  mx = ap_block_max(mx, red4);  // (its barriers also complete sc)

  float part = 0.f;
  for (int s = tid; s < S; s += AP_THREADS) {
    const float x = sc[s];
    const float e = x == ninf ? 0.f : expf(x - mx);
    sc[s] = e;
    part += e;
  }
  const float tot = ap_block_sum(part, red4);
  float* __restrict__ pp = p + ((int64_t)b * heads + h) * S;
  for (int s = tid; s < S; s += AP_THREADS) {
    const float ps = sc[s] / tot;  // every key masked: 0 / 0 = NaN, as the reference's softmax over a row of -inf
    sc[s] = ps;
    pp[s] = ps;
  }
  __syncthreads();

  // out = sum_s p_s v_s over the keys with p_s != 0
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int s0 = 0; s0 < S; s0 += KP * AP_U) {
    bf16x8 raw[AP_U];
    float ps[AP_U];
#pragma unroll
    for (int u = 0; u < AP_U; ++u) {
      const int s = s0 + u * KP + kg;
      ps[u] = s < S ? sc[s] : 0.f;
      raw[u] = ap_zero8();
      if (ps[u] != 0.f && live) raw[u] = *reinterpret_cast<const bf16x8*>(vb + (int64_t)s * ld);
    }
#pragma unroll
    for (int u = 0; u < AP_U; ++u) {
      if (ps[u] != 0.f) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = fmaf(ps[u], (float)raw[u][j], acc[j]);
      }
    }
  }
  ap_fold_keys<G>(acc, red);
  if (tid < G && live) Vec8<bf16_t>::store(out + b * ((int64_t)heads * hd) + col, acc);
}

template <int G>
__global__ __launch_bounds__(AP_THREADS) void attn_pool_bwd_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ k,
                                                                   const bf16_t* __restrict__ v, int64_t ld, int64_t batch_stride,
                                                                   const bf16_t* __restrict__ q, const float* __restrict__ p,
                                                                   bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int64_t ldg,
                                                                   int64_t batch_stride_g, float* __restrict__ dq_part, int S, int heads,
                                                                   int hd) {
  constexpr int KP = AP_THREADS / G;
  __shared__ __align__(16) float sp[AP_MAX_S];
  __shared__ __align__(16) float sdp[AP_MAX_S];
  __shared__ __align__(16) float red[4 * G * 8];
  __shared__ float red4[4];
  const int tid = threadIdx.x, c = tid & (G - 1), kg = tid / G;
  const int64_t b = blockIdx.x / heads;
  const int h = blockIdx.x % heads;
  const bool live = c * 8 < hd;
  const int64_t col = (int64_t)h * hd + c * 8;
  const int64_t H = (int64_t)heads * hd;
  const bf16_t* __restrict__ kb = k + b * batch_stride + col;
  const bf16_t* __restrict__ vb = v + b * batch_stride + col;
  bf16_t* __restrict__ dkb = dk + b * batch_stride_g + col;
  bf16_t* __restrict__ dvb = dv + b * batch_stride_g + col;
  const float* __restrict__ pp = p + ((int64_t)b * heads + h) * S;
  float qv[8], g[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) qv[j] = g[j] = 0.f;
  if (live) {
    Vec8<bf16_t>::load(q + col, qv);
    Vec8<bf16_t>::load(dout + b * H + col, g);
  }

  // one pass over v: dp_s = dout . v_s -> sdp, p_s -> sp, dv_s = p_s dout, c = sum_s p_s dp_s
  float cpart = 0.f;
  for (int s0 = 0; s0 < S; s0 += KP * AP_U) {
    bf16x8 raw[AP_U];
    float ps[AP_U];
#pragma unroll
    for (int u = 0; u < AP_U; ++u) {
      const int s = s0 + u * KP + kg;
      ps[u] = s < S ? pp[s] : 0.f;
      raw[u] = ap_zero8();
      if (ps[u] != 0.f && live) raw[u] = *reinterpret_cast<const bf16x8*>(vb + (int64_t)s * ld);
    }
#pragma unroll
    for (int u = 0; u < AP_U; ++u) {
      const int s = s0 + u * KP + kg;
      const float d = ap_group_sum<G>(ap_dot8(raw[u], g));
      if (s < S) {
        if (live) {
          if (ps[u] != 0.f) ap_store8(dvb + (int64_t)s * ldg, g, ps[u]);
          else *reinterpret_cast<bf16x8*>(dvb + (int64_t)s * ldg) = ap_zero8();
        }
        if (c == 0) {
          sp[s] = ps[u];
          sdp[s] = d;
          if (ps[u] != 0.f) cpart = fmaf(ps[u], d, cpart);
        }
      }
    }
  }
  const float cc = ap_block_sum(cpart, red4);  // (its barriers also complete sp and sdp)

  // one pass over k: ds_s = p_s (dp_s - c), dk_s = ds_s q, dq = sum_s ds_s k_s
  float acc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] = 0.f;
  for (int s0 = 0; s0 < S; s0 += KP * AP_U) {
    bf16x8 raw[AP_U];
    float ps[AP_U];
#pragma unroll
    for (int u = 0; u < AP_U; ++u) {
      const int s = s0 + u * KP + kg;
      ps[u] = s < S ? sp[s] : 0.f;
      raw[u] = ap_zero8();
      if (ps[u] != 0.f && live) raw[u] = *reinterpret_cast<const bf16x8*>(kb + (int64_t)s * ld);
    }
#pragma unroll
    for (int u = 0; u < AP_U; ++u) {
      const int s = s0 + u * KP + kg;
      if (s < S && live) {
        if (ps[u] != 0.f) {
          const float ds = ps[u] * (sdp[s] - cc);
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] = fmaf(ds, (float)raw[u][j], acc[j]);
          ap_store8(dkb + (int64_t)s * ldg, qv, ds);
        } else {
          *reinterpret_cast<bf16x8*>(dkb + (int64_t)s * ldg) = ap_zero8();
        }
      }
    }
  }
  ap_fold_keys<G>(acc, red);
  if (tid < G && live) Vec8<float>::store(dq_part + b * H + col, acc);
}

int ap_group_width(int64_t hd) {
  int g = 1;
  while (g * 8 < hd) g <<= 1;
  return g;
}

// the limits both entries share; `what` names the entry in the message
int ap_check_shape(const char* what, int64_t ld, int64_t batch_stride, int64_t B, int64_t S, int64_t heads, int64_t hd) {
  OP_CHECK_ARG(hd >= 8 && hd <= 128 && hd % 8 == 0, "%s: hd = %lld, need a multiple of 8 in 8 ... 128", what, (long long)hd);
  OP_CHECK_ARG(S >= 1 && S <= AP_MAX_S, "%s: S = %lld, need 1 <= S <= %d", what, (long long)S, AP_MAX_S);
  OP_CHECK_ARG(heads >= 1 && heads <= 4096, "%s: heads = %lld, need 1 ... 4096", what, (long long)heads);
  OP_CHECK_ARG(B >= 0 && B * heads < (int64_t(1) << 31), "%s: B = %lld, need 0 <= B and B * heads < 2^31", what, (long long)B);
  OP_CHECK_ARG(ld % 8 == 0 && ld >= heads * hd, "%s: ld = %lld, need a multiple of 8 and >= heads * hd = %lld", what, (long long)ld,
               (long long)(heads * hd));
  OP_CHECK_ARG(batch_stride % 8 == 0 && batch_stride >= 0, "%s: batch_stride = %lld, need a non-negative multiple of 8", what,
               (long long)batch_stride);
  return OP_OK;
}

}  // namespace

extern "C" int op_attn_pool_fwd(const void* k, const void* v, int64_t ld, int64_t batch_stride, const void* q, const uint8_t* pad,
                                int64_t ld_pad, void* out, float* p, int64_t B, int64_t S, int64_t heads, int64_t hd, void* stream) {
  const int rc = ap_check_shape("op_attn_pool_fwd", ld, batch_stride, B, S, heads, hd);
  if (rc != OP_OK) return rc;
  OP_CHECK_ARG(k && v && q && out && p, "op_attn_pool_fwd: k, v, q, out and p must be non-null");
  OP_CHECK_ARG((((uintptr_t)k | (uintptr_t)v | (uintptr_t)q | (uintptr_t)out) & 15) == 0 && ((uintptr_t)p & 3) == 0,
               "op_attn_pool_fwd: k, v, q and out must be aligned to 16 bytes, p to 4");
  OP_CHECK_ARG(!pad || ld_pad >= S, "op_attn_pool_fwd: ld_pad = %lld, need >= S = %lld", (long long)ld_pad, (long long)S);
  if (B == 0) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  return op_with_int<1, 2, 4, 8, 16>(ap_group_width(hd), [&](auto g) {
    hipLaunchKernelGGL((attn_pool_fwd_kernel<decltype(g)::value>), dim3((unsigned)(B * heads)), dim3(AP_THREADS), 0, st, (const bf16_t*)k,
                       (const bf16_t*)v, ld, batch_stride, (const bf16_t*)q, pad, ld_pad, (bf16_t*)out, p, (int)S, (int)heads, (int)hd);
    OP_LAUNCH_CHECK();
    return OP_OK;
  });
}

extern "C" int op_attn_pool_bwd(const void* dout, const void* k, const void* v, int64_t ld, int64_t batch_stride, const void* q,
                                const float* p, void* dk, void* dv, int64_t ldg, int64_t batch_stride_g, float* dq_part, int64_t B,
                                int64_t S, int64_t heads, int64_t hd, void* stream) {
  int rc = ap_check_shape("op_attn_pool_bwd", ld, batch_stride, B, S, heads, hd);
  if (rc != OP_OK) return rc;
  OP_CHECK_ARG(ldg % 8 == 0 && ldg >= heads * hd, "op_attn_pool_bwd: ldg = %lld, need a multiple of 8 and >= heads * hd = %lld",
               (long long)ldg, (long long)(heads * hd));
  OP_CHECK_ARG(batch_stride_g % 8 == 0 && (B <= 1 || batch_stride_g >= (S - 1) * ldg + heads * hd),
               "op_attn_pool_bwd: batch_stride_g = %lld, need a multiple of 8 and >= (S - 1) * ldg + heads * hd = %lld (the samples' rows "
               "of dk / dv must not overlap)", (long long)batch_stride_g, (long long)((S - 1) * ldg + heads * hd));
  OP_CHECK_ARG(dout && k && v && q && p && dk && dv && dq_part, "op_attn_pool_bwd: every pointer must be non-null");
  OP_CHECK_ARG((((uintptr_t)dout | (uintptr_t)k | (uintptr_t)v | (uintptr_t)q | (uintptr_t)dk | (uintptr_t)dv | (uintptr_t)dq_part) & 15) == 0 &&
                   ((uintptr_t)p & 3) == 0,
               "op_attn_pool_bwd: dout, k, v, q, dk, dv and dq_part must be aligned to 16 bytes, p to 4");
  if (B == 0) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  return op_with_int<1, 2, 4, 8, 16>(ap_group_width(hd), [&](auto g) {
    hipLaunchKernelGGL((attn_pool_bwd_kernel<decltype(g)::value>), dim3((unsigned)(B * heads)), dim3(AP_THREADS), 0, st, (const bf16_t*)dout,
                       (const bf16_t*)k, (const bf16_t*)v, ld, batch_stride, (const bf16_t*)q, p, (bf16_t*)dk, (bf16_t*)dv, ldg,
                       batch_stride_g, dq_part, (int)S, (int)heads, (int)hd);
    OP_LAUNCH_CHECK();
    return OP_OK;
  });
}
