// Temporal attention of the video branch (include/onepeace_hip.h: op_attn_frames_fwd, op_attn_frames_bwd): self-attention over the T
// frames of a clip, one sequence per (video b, token position n, head h), read from and written to the project's batch-major rows
// (frame-major inside a video) -- one_peace_vision/video/mmaction_custom/models/backbones/onepeace.py:234-247 as called from :331-337,
// the two rearranges of :331 and :337 included: element (b, t, n, h, d) at ((b * T + t) * N + n) * ld + h * 64 + d.
//
// One wavefront (= one workgroup) per (b, n, group of G = 64 / TP heads), TP = 8, 16 or 32 >= T: lane = (head of the group, frame).
//   global   a frame's row of the group is G * 128 contiguous bytes: every global access is one 16-byte vector per lane, consecutive
//            lanes along the row (the stride N * ld is between frames).  Tiles pass through LDS both ways, so loads and stores are the
//            same coalesced shape and every lane meets its own 64-element row in LDS.
//   LDS      a staged tile holds 64 rows (head, frame) of 64 bf16, row stride 144 bytes (one 16-byte access of padding), head blocks
//            staggered by another 16 bytes: a lane's walk down its own row and the broadcast reads of a key row (all lanes of a head read
//            the same address) are conflict-free.  64 rows per wave whatever T is: LDS per wave, and with it the occupancy, does not
//            depend on T (forward 18.3 KB: 8 waves per CU; backward 36.3 KB: 4 waves per CU, one per SIMD).
//   forward  tiles Q and K staged, V kept in flight in registers; lane (h, t) holds q_t in fp32 and writes its T scores over its own
//            (consumed) Q row; V then takes K's tile; p = exp(s - max), out = (sum p v) / (sum p); the bf16 row goes out through the Q tile.
//   backward K and V tiles: s and dp of query row t (the lane's q_t and dout_t in registers), written TRANSPOSED ([head][t'][t], fp32)
//            into two score tiles; softmax statistics, c = sum p dp, p and ds in place; dq_t = scale * sum ds k.  Then the Q and dO
//            tiles (their 16-byte vectors waited in registers) replace K and V, and lane (h, t') reads ITS row of p and ds in 16-byte
//            pieces: dv_t' = sum_t p do_t, dk_t' = scale * sum_t ds q_t.  Nothing is recomputed between the two halves.
// The two small products stay on the VALU (fp32 FMA on bf16 values widened by one shift / mask): DESIGN.md 4.13 says why, and what the
// matrix pipe would buy.  Every sum runs in a fixed order inside one lane: no atomics, no cross-lane reduction, two runs give the same
// bits, and a sequence's bits depend on nothing but its own rows, T and scale (not on B, N, heads or the group it falls into).
#include "common.h"

#include <math.h>

namespace {

constexpr int FA_ROWV = 9;                   // 16-byte vectors per staged row: 8 of data + 1 of padding
constexpr int FA_TILE = 64 * FA_ROWV + 8;    // vectors per tile: 64 rows + one vector of stagger per head block (at most 8)
constexpr int FA_SROW = 36;                  // floats per row of a score tile: TP <= 32 + padding, 144 bytes

template <int TP> struct Fa {
  static constexpr int G = 64 / TP;             // heads per wavefront
  static constexpr int HV = TP * FA_ROWV + 1;   // vectors per head block
  static __device__ __forceinline__ int row(int hh, int t) { return hh * HV + t * FA_ROWV; }
  static __device__ __forceinline__ int srow(int hh, int t) { return (hh * TP + t) * FA_SROW; }

  // the tile's 512 vectors, 8 per lane: vector i = frame i / (8 G), 16-byte piece i % (8 G) of the group's G * 128 bytes of that row
  static __device__ __forceinline__ void load(const bf16_t* __restrict__ p, int64_t base, int64_t tstride, int T, int gh, int lane,
                                              u32x4 (&raw)[8]) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int i = it * 64 + lane, t = i / (8 * G), c = i % (8 * G);
      raw[it] = (u32x4){0u, 0u, 0u, 0u};
      if (t < T && (c >> 3) < gh) raw[it] = *reinterpret_cast<const u32x4*>(p + base + t * tstride + c * 8);
    }
  }
  static __device__ __forceinline__ void put(u32x4* tile, int lane, const u32x4 (&raw)[8]) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int i = it * 64 + lane, t = i / (8 * G), c = i % (8 * G);
      tile[row(c >> 3, t) + (c & 7)] = raw[it];
    }
  }
  static __device__ __forceinline__ void store(bf16_t* __restrict__ p, int64_t base, int64_t tstride, int T, int gh, int lane,
                                               const u32x4* tile) {
#pragma unroll
    for (int it = 0; it < 8; ++it) {
      const int i = it * 64 + lane, t = i / (8 * G), c = i % (8 * G);
      if (t < T && (c >> 3) < gh) *reinterpret_cast<u32x4*>(p + base + t * tstride + c * 8) = tile[row(c >> 3, t) + (c & 7)];
    }
  }
};

__device__ __forceinline__ float fa_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float fa_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

__device__ __forceinline__ void fa_row_f32(const u32x4* row, float (&v)[64]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const u32x4 w = row[j];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[j * 8 + 2 * e] = fa_lo(w[e]);
      v[j * 8 + 2 * e + 1] = fa_hi(w[e]);
    }
  }
}
// sum_d a[d] * row[d]: the even and the odd elements in two chains, each in index order, then (even + odd)
__device__ __forceinline__ float fa_dot(const float (&a)[64], const u32x4* row) {
  float s0 = 0.f, s1 = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const u32x4 w = row[j];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s0 = fmaf(a[j * 8 + 2 * e], fa_lo(w[e]), s0);
      s1 = fmaf(a[j * 8 + 2 * e + 1], fa_hi(w[e]), s1);
    }
  }
  return s0 + s1;
}
__device__ __forceinline__ void fa_axpy(float (&acc)[64], float a, const u32x4* row) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const u32x4 w = row[j];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      acc[j * 8 + 2 * e] = fmaf(a, fa_lo(w[e]), acc[j * 8 + 2 * e]);
      acc[j * 8 + 2 * e + 1] = fmaf(a, fa_hi(w[e]), acc[j * 8 + 2 * e + 1]);
    }
  }
}
// row = bf16(v * mul), rounded once (to nearest even)
__device__ __forceinline__ void fa_row_bf16(u32x4* row, const float (&v)[64], float mul) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    bf16x8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (bf16_t)(v[j * 8 + e] * mul);
    row[j] = __builtin_bit_cast(u32x4, r);
  }
}

struct FaItem {
  int64_t bn;  // b * N + n
  int h0, gh;  // first head of the group, heads in it
};
template <int TP> __device__ __forceinline__ FaItem fa_item(int heads, int ngroups) {
  FaItem it;
  it.bn = blockIdx.x / (unsigned)ngroups;
  it.h0 = (int)(blockIdx.x % (unsigned)ngroups) * Fa<TP>::G;
  it.gh = min(Fa<TP>::G, heads - it.h0);
  return it;
}
// offset of (b, t = 0, n, h0, 0) for row stride ld
__device__ __forceinline__ int64_t fa_base(const FaItem& it, int64_t ld, int T, int N) {
  const int64_t b = it.bn / N, n = it.bn % N;
  return (b * T * N + n) * ld + (int64_t)it.h0 * 64;
}

template <int TP>
__global__ __launch_bounds__(64, 2) void attn_frames_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                             const bf16_t* __restrict__ v, int64_t ld, bf16_t* __restrict__ out,
                                                             int64_t ldo, int T, int N, int heads, int ngroups, float scale) {
  using F = Fa<TP>;
  __shared__ u32x4 tq[FA_TILE], tk[FA_TILE];
  const int lane = threadIdx.x;
  const FaItem item = fa_item<TP>(heads, ngroups);
  const int64_t base = fa_base(item, ld, T, N), tstride = (int64_t)N * ld;
  u32x4 rq[8], rk[8], rv[8];
  F::load(q, base, tstride, T, item.gh, lane, rq);
  F::load(k, base, tstride, T, item.gh, lane, rk);
  F::load(v, base, tstride, T, item.gh, lane, rv);
  F::put(tq, lane, rq);
  F::put(tk, lane, rk);
  __syncthreads();
  const int hh = lane / TP, t = lane % TP;
  const bool active = t < T && hh < item.gh;
  const int chunks = (T + 3) >> 2;
  u32x4* own = tq + F::row(hh, t);
  float m = -INFINITY;
  if (active) {
    float qf[64];
    fa_row_f32(own, qf);
    for (int c = 0; c < chunks; ++c) {
      float s4[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int tp = 4 * c + u;
        s4[u] = -INFINITY;
        if (tp < T) {
          s4[u] = scale * fa_dot(qf, tk + F::row(hh, tp));
          m = fmaxf(m, s4[u]);
        }
      }
      own[c] = (u32x4){__float_as_uint(s4[0]), __float_as_uint(s4[1]), __float_as_uint(s4[2]), __float_as_uint(s4[3])};  // over q_t
    }
  }
  __syncthreads();  // every lane is done with K
  F::put(tk, lane, rv);
  __syncthreads();
  if (active) {
    float acc[64];
#pragma unroll
    for (int d = 0; d < 64; ++d) acc[d] = 0.f;
    float l = 0.f;
    for (int c = 0; c < chunks; ++c) {
      const u32x4 s4 = own[c];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int tp = 4 * c + u;
        if (tp < T) {
          const float p = expf(__uint_as_float(s4[u]) - m);
          l += p;
          fa_axpy(acc, p, tk + F::row(hh, tp));
        }
      }
    }
    fa_row_bf16(own, acc, 1.0f / l);
  }
  __syncthreads();
  F::store(out, fa_base(item, ldo, T, N), (int64_t)N * ldo, T, item.gh, lane, tq);
}

template <int TP>
__global__ __launch_bounds__(64) void attn_frames_bwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                             const bf16_t* __restrict__ v, int64_t ld, const bf16_t* __restrict__ dout,
                                                             int64_t ldo, bf16_t* __restrict__ dq, bf16_t* __restrict__ dk,
                                                             bf16_t* __restrict__ dv, int64_t ldg, int T, int N, int heads, int ngroups,
                                                             float scale) {
  using F = Fa<TP>;
  __shared__ u32x4 ta[FA_TILE], tb[FA_TILE];                  // K then Q (and dq, dk on their way out) | V then dO (and dv)
  __shared__ __align__(16) float sp[64 * FA_SROW], sd[64 * FA_SROW];  // [head][t'][t]: s -> e -> p | dp -> ds
  const int lane = threadIdx.x;
  const FaItem item = fa_item<TP>(heads, ngroups);
  const int64_t base = fa_base(item, ld, T, N), tstride = (int64_t)N * ld;
  const int64_t gbase = fa_base(item, ldg, T, N), gstride = (int64_t)N * ldg;
  u32x4 rq[8], ro[8], rk[8], rv[8];
  F::load(q, base, tstride, T, item.gh, lane, rq);
  F::load(dout, fa_base(item, ldo, T, N), (int64_t)N * ldo, T, item.gh, lane, ro);
  F::load(k, base, tstride, T, item.gh, lane, rk);
  F::load(v, base, tstride, T, item.gh, lane, rv);
  F::put(ta, lane, rq);
  F::put(tb, lane, ro);
  __syncthreads();
  const int hh = lane / TP, t = lane % TP;
  const bool active = t < T && hh < item.gh;
  float acc[64], acc2[64];  // q_t, dout_t; then dq_t; then dk_t', dv_t'
  if (active) {
    fa_row_f32(ta + F::row(hh, t), acc);
    fa_row_f32(tb + F::row(hh, t), acc2);
  }
  __syncthreads();
  F::put(ta, lane, rk);
  F::put(tb, lane, rv);
  __syncthreads();
  if (active) {
    float m = -INFINITY;
    for (int tp = 0; tp < T; ++tp) {
      const float s = scale * fa_dot(acc, ta + F::row(hh, tp));
      const float dp = fa_dot(acc2, tb + F::row(hh, tp));
      m = fmaxf(m, s);
      sp[F::srow(hh, tp) + t] = s;
      sd[F::srow(hh, tp) + t] = dp;
    }
    float l = 0.f, cu = 0.f;
    for (int tp = 0; tp < T; ++tp) {
      const float e = expf(sp[F::srow(hh, tp) + t] - m);
      l += e;
      cu = fmaf(e, sd[F::srow(hh, tp) + t], cu);
      sp[F::srow(hh, tp) + t] = e;
    }
    const float inv = 1.0f / l;
    const float cc = cu * inv;
#pragma unroll
    for (int d = 0; d < 64; ++d) acc[d] = 0.f;
    for (int tp = 0; tp < T; ++tp) {
      const float p = sp[F::srow(hh, tp) + t] * inv;
      const float ds = p * (sd[F::srow(hh, tp) + t] - cc);
      sp[F::srow(hh, tp) + t] = p;
      sd[F::srow(hh, tp) + t] = ds;
      fa_axpy(acc, ds, ta + F::row(hh, tp));
    }
  }
  __syncthreads();  // every lane is done with K and V; p and ds are complete
  if (active) fa_row_bf16(ta + F::row(hh, t), acc, scale);
  __syncthreads();
  F::store(dq, gbase, gstride, T, item.gh, lane, ta);
  __syncthreads();
  F::put(ta, lane, rq);
  F::put(tb, lane, ro);
  __syncthreads();
  if (active) {  // the lane is now key row t' = t
#pragma unroll
    for (int d = 0; d < 64; ++d) acc[d] = acc2[d] = 0.f;
    const int chunks = (T + 3) >> 2;
    for (int c = 0; c < chunks; ++c) {
      const f32x4 p4 = *reinterpret_cast<const f32x4*>(&sp[F::srow(hh, t) + 4 * c]);
      const f32x4 d4 = *reinterpret_cast<const f32x4*>(&sd[F::srow(hh, t) + 4 * c]);
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int tq = 4 * c + u;
        if (tq < T) {
          fa_axpy(acc, d4[u], ta + F::row(hh, tq));   // dk_t' += ds[t][t'] q_t
          fa_axpy(acc2, p4[u], tb + F::row(hh, tq));  // dv_t' += p[t][t'] dout_t
        }
      }
    }
  }
  __syncthreads();
  if (active) {
    fa_row_bf16(ta + F::row(hh, t), acc, scale);
    fa_row_bf16(tb + F::row(hh, t), acc2, 1.0f);
  }
  __syncthreads();
  F::store(dk, gbase, gstride, T, item.gh, lane, ta);
  F::store(dv, gbase, gstride, T, item.gh, lane, tb);
}

inline bool fa_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the limits both entries share; `what` names the entry in the message
int fa_check_shape(const char* what, int64_t B, int64_t T, int64_t N, int64_t heads, int64_t hd) {
  OP_CHECK_ARG(hd == 64, "%s: hd = %lld, need 64", what, (long long)hd);
  OP_CHECK_ARG(T >= 1 && T <= 32, "%s: T = %lld, need 1 <= T <= 32", what, (long long)T);
  OP_CHECK_ARG(N >= 1 && heads >= 1, "%s: N = %lld, heads = %lld, need >= 1", what, (long long)N, (long long)heads);
  OP_CHECK_ARG(B >= 0, "%s: B = %lld, need >= 0", what, (long long)B);
  OP_CHECK_ARG(heads < (int64_t(1) << 31) && N < (int64_t(1) << 31) && (B == 0 || N * heads <= ((int64_t(1) << 31) - 1) / B),
               "%s: B * N * heads = %lld * %lld * %lld, need < 2^31", what, (long long)B, (long long)N, (long long)heads);
  return OP_OK;
}
int fa_check_ld(const char* what, const char* name, int64_t ld, int64_t heads, int64_t hd) {
  OP_CHECK_ARG(ld % 8 == 0 && ld >= heads * hd, "%s: %s = %lld, need a multiple of 8 and >= heads * hd = %lld", what, name, (long long)ld,
               (long long)(heads * hd));
  return OP_OK;
}

}  // namespace

extern "C" int op_attn_frames_fwd(const void* q, const void* k, const void* v, int64_t ld, void* out, int64_t ldo, int64_t B, int64_t T,
                                  int64_t N, int64_t heads, int64_t hd, float scale, void* stream) {
  int rc = fa_check_shape("op_attn_frames_fwd", B, T, N, heads, hd);
  if (rc == OP_OK) rc = fa_check_ld("op_attn_frames_fwd", "ld", ld, heads, hd);
  if (rc == OP_OK) rc = fa_check_ld("op_attn_frames_fwd", "ldo", ldo, heads, hd);
  if (rc != OP_OK) return rc;
  OP_CHECK_ARG(q && k && v && out, "op_attn_frames_fwd: q, k, v and out must be non-null");
  OP_CHECK_ARG(fa_aligned16(q) && fa_aligned16(k) && fa_aligned16(v) && fa_aligned16(out),
               "op_attn_frames_fwd: q, k, v and out must be aligned to 16 bytes");
  if (B == 0) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int tp = T <= 8 ? 8 : (T <= 16 ? 16 : 32);
  return op_with_int<8, 16, 32>(tp, [&](auto tpc) {
    constexpr int TP = decltype(tpc)::value;
    const int ngroups = ceil_div(heads, 64 / TP);
    hipLaunchKernelGGL((attn_frames_fwd_kernel<TP>), dim3((unsigned)(B * N * ngroups)), dim3(64), 0, st, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, ld, (bf16_t*)out, ldo, (int)T, (int)N, (int)heads, ngroups, scale);
    OP_LAUNCH_CHECK();
    return OP_OK;
  });
}

extern "C" int op_attn_frames_bwd(const void* q, const void* k, const void* v, int64_t ld, const void* dout, int64_t ldo, void* dq,
                                  void* dk, void* dv, int64_t ldg, int64_t B, int64_t T, int64_t N, int64_t heads, int64_t hd,
                                  float scale, void* stream) {
  int rc = fa_check_shape("op_attn_frames_bwd", B, T, N, heads, hd);
  if (rc == OP_OK) rc = fa_check_ld("op_attn_frames_bwd", "ld", ld, heads, hd);
  if (rc == OP_OK) rc = fa_check_ld("op_attn_frames_bwd", "ldo", ldo, heads, hd);
  if (rc == OP_OK) rc = fa_check_ld("op_attn_frames_bwd", "ldg", ldg, heads, hd);
  if (rc != OP_OK) return rc;
  OP_CHECK_ARG(q && k && v && dout && dq && dk && dv, "op_attn_frames_bwd: every pointer must be non-null");
  OP_CHECK_ARG(fa_aligned16(q) && fa_aligned16(k) && fa_aligned16(v) && fa_aligned16(dout) && fa_aligned16(dq) && fa_aligned16(dk) &&
                   fa_aligned16(dv),
               "op_attn_frames_bwd: q, k, v, dout, dq, dk and dv must be aligned to 16 bytes");
  if (B == 0) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int tp = T <= 8 ? 8 : (T <= 16 ? 16 : 32);
  return op_with_int<8, 16, 32>(tp, [&](auto tpc) {
    constexpr int TP = decltype(tpc)::value;
    const int ngroups = ceil_div(heads, 64 / TP);
    hipLaunchKernelGGL((attn_frames_bwd_kernel<TP>), dim3((unsigned)(B * N * ngroups)), dim3(64), 0, st, (const bf16_t*)q,
                       (const bf16_t*)k, (const bf16_t*)v, ld, (const bf16_t*)dout, ldo, (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, ldg, (int)T,
                       (int)N, (int)heads, ngroups, scale);
    OP_LAUNCH_CHECK();
    return OP_OK;
  });
}
