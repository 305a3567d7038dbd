// Window attention of the detection branch (include/onepeace_hip.h: op_attn_window_fwd, op_attn_window_bwd): self-attention inside the
// 16 x 16 windows of a [B, Hg, Wg, D] token map, one sequence of 256 tokens per (sample b, window, head h), read from and written to the
// project's batch-major rows -- one_peace_vision/det/models/onepeace.py:197-213 as called from :308-325, with window_partition and
// window_unpartition, the expanded window bias of :398-401 and add_decomposed_rel_pos folded in: element (b, y, x, h, d) at
// ((b * Hg + y) * Wg + x) * ld + h * 64 + d, window (wy, wx) = rows y in [16 wy, 16 wy + 16), x likewise, i = 16 (y % 16) + x % 16.
//
// One workgroup of 4 waves per (b, window, head); every product runs on v_mfma_f32_32x32x16_bf16 (lane maps: C/D col = lane & 31,
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5); A/B lane (r, half) holds k = 8 half + 0..7 of row / column r).
//   query pass  a wave owns 64 queries, 32 at a time.  S^T = K Q^T (A = K rows, B = Q rows, both 16-byte fragments straight from the
//               packed rows): the lane holds ONE query's scores against 128 of the 256 keys in registers, its partner lane (lane ^ 32)
//               the other 128, so max, sum and c = sum p dp are in-lane sums plus one exchange.  R = rel Q^T (31 rows padded to 32) is
//               one more tile per table; it passes through a per-wave LDS scratch so that the lane can pick Th[jy] = R[iy - jy + 15].
//               The fp32 tile is the next product's B operand with no lane movement (converted to bf16 pairwise, k order permuted):
//               out^T = V^T P^T and dq^T = K^T dS^T take their A operand from a transposed LDS image [d][token] of V resp. K.
//   key pass    (backward only) a wave owns 64 keys, 32 at a time.  S = Q K^T in the other orientation (lane = key), p and ds rebuilt
//               from the row statistics m, 1 / l, c and the Th / Tw tables the query pass left in LDS; dv^T = dO^T P and
//               dk^T = Q^T dS take the transposed images of dO and Q.  drel = G^T Q (G the scatter of dTh / dTw onto the 31 offsets)
//               is one tile per wave from the same Q image.
// Roundings to bf16 before a matrix-pipe product (stated deviations, include/onepeace_hip.h): exp(s - m) before P V; the normalised p
// before p^T dO; ds before ds K, ds^T Q; dTh / dTw before the products with rel and with q.  Everything else is fp32: s, the softmax,
// c = sum_j p dp (from the resident p and dp, never from a rounded out), dTh, dTw, the dbias slabs.
// No atomics; every sum has a fixed order; a (b, window, head)'s bits depend on its own rows, bias[h], rel and scale only.
// With slabs or parts asked for, the backward grid is slabs x heads workgroups (else one per (b, window, head)); each walks its share of (b, window) in order, so that its dbias slab (plain fp32
// read-modify-write in global memory, each element by the one lane that owns it) and its drel part (likewise) are sums in a fixed order.
#include "common.h"

#include <math.h>

namespace {

constexpr int WA_XT = 264;   // elements per row of a transposed image [64 d][256 tokens + 8]
constexpr int WA_RL = 72;    // elements per row of a staged rel table [32 offsets][64 + 8]
constexpr int WA_RT = 40;    // elements per row of a transposed rel table [64 d][32 offsets + 8]
constexpr int WA_RW = 33;    // floats per row of the per-wave scratch [2 tables][32 queries][32 offsets + 1]
constexpr int WA_TT = 17;    // floats per row of the Th / Tw tables [2][256 queries][16 + 1]

constexpr int WA_XT_BYTES = 64 * WA_XT * 2;          // 33792
constexpr int WA_REL_BYTES = 2 * 32 * WA_RL * 2;     // 9216
constexpr int WA_RELT_BYTES = 2 * 64 * WA_RT * 2;    // 10240
constexpr int WA_RW_BYTES = 4 * 2 * 32 * WA_RW * 4;  // 33792: four waves
constexpr int WA_STAT_BYTES = 3 * 256 * 4;           // 3072
constexpr int WA_TT_BYTES = 2 * 256 * WA_TT * 4;     // 34816
constexpr int WA_GT_BYTES = 2 * 32 * WA_XT * 2;      // 33792
constexpr int WA_FWD_LDS = WA_XT_BYTES + WA_REL_BYTES + WA_RW_BYTES;                                                       // 76800
constexpr int WA_BWD_LDS = 2 * WA_XT_BYTES + WA_REL_BYTES + WA_RELT_BYTES + WA_STAT_BYTES + WA_TT_BYTES + WA_GT_BYTES;  // 158720
static_assert(WA_RW_BYTES == WA_XT_BYTES, "the per-wave scratch and the dO image share one region");
static_assert(WA_BWD_LDS <= 160 * 1024, "LDS of the backward");

__device__ __forceinline__ f32x16 wa_mma(bf16x8 a, bf16x8 b, f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
// The fragments of K, V (query pass) and Q, dO (key pass) are the same in both passes of a wave; hoisted out of the pass loop they would
// hold 128 to 256 registers.  The pass takes its base pointer through this, which the optimiser cannot see through.
__device__ __forceinline__ const bf16_t* wa_opaque(const bf16_t* p) {
  asm volatile("" : "+s"(p));
  return p;
}
__device__ __forceinline__ f32x16 wa_zero() {
  f32x16 z;
#pragma unroll
  for (int e = 0; e < 16; ++e) z[e] = 0.f;
  return z;
}
// row of token i of the window whose token 0 is row0
__device__ __forceinline__ int64_t wa_row(int64_t row0, int Wg, int i) { return row0 + (int64_t)(i >> 4) * Wg + (i & 15); }
// elements 8 hl ... 8 hl + 7 of k-step s of a row: the A / B fragment of v_mfma_f32_32x32x16_bf16 in natural k order
__device__ __forceinline__ bf16x8 wa_frag(const bf16_t* row, int s, int hl) { return *reinterpret_cast<const bf16x8*>(row + 16 * s + 8 * hl); }
// the A fragment that goes with an accumulator tile used as B operand: k-step s of 32 tokens from t0 on, token order
// 16 s + 8 (j >> 2) + 4 hl + (j & 3)
__device__ __forceinline__ bf16x8 wa_frag_perm(const bf16_t* xrow, int t0, int s, int hl) {
  const bf16x4 lo = *reinterpret_cast<const bf16x4*>(xrow + t0 + 16 * s + 4 * hl);
  const bf16x4 hi = *reinterpret_cast<const bf16x4*>(xrow + t0 + 16 * s + 8 + 4 * hl);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}
// registers 8 s ... 8 s + 7 of an accumulator tile, each rounded to bf16 once (to nearest even)
__device__ __forceinline__ bf16x8 wa_acc_frag(const f32x16& x, int s) {
  bf16x8 f;
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = (bf16_t)x[8 * s + e];
  return f;
}

// transposed image xt[d][token] of the window's 256 rows of one head (src points at the head's column block)
__device__ __forceinline__ void wa_stage_T(bf16_t* xt, const bf16_t* __restrict__ src, int64_t row0, int Wg, int64_t ld, int tid) {
  const bf16_t* row = src + wa_row(row0, Wg, tid) * ld;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const bf16x8 x = *reinterpret_cast<const bf16x8*>(row + 8 * c);
#pragma unroll
    for (int e = 0; e < 8; ++e) xt[(8 * c + e) * WA_XT + tid] = x[e];
  }
}
// rel_h | rel_w [31][64] as rows [2][32][WA_RL] (row 31 = 0) and, when relt is given, transposed [2][64][WA_RT] (column 31 = 0)
__device__ __forceinline__ void wa_stage_rel(bf16_t* rel, bf16_t* relt, const bf16_t* __restrict__ rel_h, const bf16_t* __restrict__ rel_w,
                                             int tid) {
  for (int e = tid; e < 2 * 32 * 64; e += 256) {
    const int tbl = e >> 11, r = (e >> 6) & 31, d = e & 63;
    const bf16_t x = r < 31 ? (tbl ? rel_w : rel_h)[r * 64 + d] : (bf16_t)0.f;
    rel[(tbl * 32 + r) * WA_RL + d] = x;
    if (relt) relt[(tbl * 64 + d) * WA_RT + r] = x;
  }
}

__device__ __forceinline__ int64_t wa_row0(int64_t bw, int Hg, int Wg) {
  const int nwx = Wg >> 4, windows = (Hg >> 4) * nwx;
  const int64_t b = bw / windows;
  const int w = (int)(bw % windows);
  return (b * Hg + 16 * (w / nwx)) * Wg + 16 * (w % nwx);
}

// The decomposed terms of the lane's query i: th[jy] = Th[i][jy] = q_i . rel_h[iy - jy + 15], tw[e] = Tw[i][jx], jx = (e & 3) + 8 (e >> 2)
// + 4 hl (the jx of the lane's score registers).  rw is the wave's scratch; the two block barriers are uniform.
__device__ __forceinline__ void wa_rel_q(const bf16_t* rel, float* rw, const bf16x8 (&qf)[4], int i, int lane, float (&th)[16],
                                         float (&tw)[8]) {
  const int r = lane & 31, hl = lane >> 5;
#pragma unroll
  for (int e = 0; e < 16; ++e) th[e] = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) tw[e] = 0.f;
  if (rel) {
#pragma unroll
    for (int tbl = 0; tbl < 2; ++tbl) {
      f32x16 acc = wa_zero();
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = wa_mma(wa_frag(rel + (tbl * 32 + r) * WA_RL, s, hl), qf[s], acc);
#pragma unroll
      for (int e = 0; e < 16; ++e) rw[(tbl * 32 + r) * WA_RW + (e & 3) + 8 * (e >> 2) + 4 * hl] = acc[e];
    }
  }
  __syncthreads();
  if (rel) {
    const int iy = i >> 4, ix = i & 15;
#pragma unroll
    for (int jy = 0; jy < 16; ++jy) th[jy] = rw[r * WA_RW + iy - jy + 15];
#pragma unroll
    for (int e = 0; e < 8; ++e) tw[e] = rw[(32 + r) * WA_RW + ix - ((e & 3) + 8 * (e >> 2) + 4 * hl) + 15];
  }
  __syncthreads();
}
// Scores of the lane's query i against keys 32 t ... 32 t + 31: register e holds s[i][j], j = 32 t + (e & 3) + 8 (e >> 2) + 4 hl.
// The same call gives the same bits (the backward makes it twice).
__device__ __forceinline__ f32x16 wa_score_tile(const bf16_t* __restrict__ kh, const bf16_t* __restrict__ biash, int64_t row0, int Wg,
                                                int64_t ld, const bf16x8 (&qf)[4], int i, int lane, float scale, float th0, float th1,
                                                const float (&tw)[8], int t) {
  const int r = lane & 31, hl = lane >> 5;
  f32x16 acc = wa_zero();
  const bf16_t* krow = kh + wa_row(row0, Wg, 32 * t + r) * ld;
#pragma unroll
  for (int s = 0; s < 4; ++s) acc = wa_mma(wa_frag(krow, s, hl), qf[s], acc);
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float b4[4] = {0.f, 0.f, 0.f, 0.f};
    if (biash) {
      const bf16x4 bb = *reinterpret_cast<const bf16x4*>(biash + (int64_t)i * 256 + 32 * t + 8 * g + 4 * hl);
#pragma unroll
      for (int e = 0; e < 4; ++e) b4[e] = (float)bb[e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float s = scale * acc[4 * g + e];
      s += b4[e];
      s += (g >> 1) ? th1 : th0;  // jy = 2 t + (g >> 1)
      s += tw[e + 4 * (g & 1)];
      acc[4 * g + e] = s;
    }
  }
  return acc;
}
// st: s -> exp(s - m); returns m and l (the sum over all 256 keys, partner lane included)
__device__ __forceinline__ void wa_softmax_q(f32x16 (&st)[8], float& m, float& l) {
  m = -INFINITY;
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) m = fmaxf(m, st[t][e]);
  m = fmaxf(m, __shfl_xor(m, 32));
  l = 0.f;
#pragma unroll
  for (int t = 0; t < 8; ++t)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const float p = __expf(st[t][e] - m);
      st[t][e] = p;
      l += p;
    }
  l += __shfl_xor(l, 32);
}
// acc^T[d][query] -> 8-byte pieces of the lane's row: d = 32 dt + 8 g + 4 hl + 0..3
__device__ __forceinline__ void wa_store_T(bf16_t* __restrict__ dst, const f32x16 (&acc)[2], float mul, int hl) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      bf16x4 o;
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] = (bf16_t)(acc[dt][4 * g + e] * mul);
      *reinterpret_cast<bf16x4*>(dst + 32 * dt + 8 * g + 4 * hl) = o;
    }
}

__global__ __launch_bounds__(256) void attn_window_fwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                              const bf16_t* __restrict__ v, int64_t ld, const bf16_t* __restrict__ bias,
                                                              const bf16_t* __restrict__ rel_h, const bf16_t* __restrict__ rel_w,
                                                              bf16_t* __restrict__ out, int64_t ldo, int Hg, int Wg, int heads,
                                                              float scale) {
  extern __shared__ __align__(16) unsigned char wa_lds[];
  bf16_t* vt = reinterpret_cast<bf16_t*>(wa_lds);
  bf16_t* rel = reinterpret_cast<bf16_t*>(wa_lds + WA_XT_BYTES);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hl = lane >> 5;
  float* rw = reinterpret_cast<float*>(wa_lds + WA_XT_BYTES + WA_REL_BYTES) + wave * (2 * 32 * WA_RW);
  const int h = (int)(blockIdx.x % (unsigned)heads);
  const int64_t row0 = wa_row0(blockIdx.x / (unsigned)heads, Hg, Wg);
  const bf16_t *qh = q + 64 * h, *kh = k + 64 * h, *vh = v + 64 * h;
  const bf16_t* biash = bias ? bias + (int64_t)h * 65536 : nullptr;
  const bool has_rel = rel_h != nullptr;
  wa_stage_T(vt, vh, row0, Wg, ld, tid);
  if (has_rel) wa_stage_rel(rel, nullptr, rel_h, rel_w, tid);
  __syncthreads();
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    const int i = 64 * wave + 32 * pass + r;
    const int64_t row = wa_row(row0, Wg, i);
    bf16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = wa_frag(qh + row * ld, s, hl);
    f32x16 st[8];
    float th[16], tw[8], m, l;
    wa_rel_q(has_rel ? rel : nullptr, rw, qf, i, lane, th, tw);
    const bf16_t* khp = wa_opaque(kh);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      st[t] = wa_score_tile(khp, biash, row0, Wg, ld, qf, i, lane, scale, th[2 * t], th[2 * t + 1], tw, t);
      __builtin_amdgcn_sched_barrier(0);  // keep the next tile's loads behind this tile: registers
    }
    wa_softmax_q(st, m, l);
    f32x16 acc[2] = {wa_zero(), wa_zero()};
#pragma unroll
    for (int t = 0; t < 8; ++t)
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const bf16x8 pf = wa_acc_frag(st[t], s);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) acc[dt] = wa_mma(wa_frag_perm(vt + (32 * dt + r) * WA_XT, 32 * t, s, hl), pf, acc[dt]);
        __builtin_amdgcn_sched_barrier(0);
      }
    wa_store_T(out + row * ldo + 64 * h, acc, 1.0f / l, hl);
  }
}

__global__ __launch_bounds__(256) void attn_window_bwd_kernel(const bf16_t* __restrict__ q, const bf16_t* __restrict__ k,
                                                              const bf16_t* __restrict__ v, int64_t ld, const bf16_t* __restrict__ bias,
                                                              const bf16_t* __restrict__ rel_h, const bf16_t* __restrict__ rel_w,
                                                              const bf16_t* __restrict__ dout, int64_t ldo, bf16_t* __restrict__ dq,
                                                              bf16_t* __restrict__ dk, bf16_t* __restrict__ dv, int64_t ldg,
                                                              float* __restrict__ drel_part, float* __restrict__ dbias_slabs, int64_t BW,
                                                              int per, int Hg, int Wg, int heads, float scale) {
  extern __shared__ __align__(16) unsigned char wa_lds[];
  bf16_t* xa = reinterpret_cast<bf16_t*>(wa_lds);                    // K^T, then Q^T
  bf16_t* xb = reinterpret_cast<bf16_t*>(wa_lds + WA_XT_BYTES);      // the waves' scratch, then dO^T
  bf16_t* rel = reinterpret_cast<bf16_t*>(wa_lds + 2 * WA_XT_BYTES);
  bf16_t* relt = reinterpret_cast<bf16_t*>(wa_lds + 2 * WA_XT_BYTES + WA_REL_BYTES);
  float* stat = reinterpret_cast<float*>(wa_lds + 2 * WA_XT_BYTES + WA_REL_BYTES + WA_RELT_BYTES);  // m | 1 / l | c
  float* tt = stat + 3 * 256;                                                                         // Th | Tw
  bf16_t* gt = reinterpret_cast<bf16_t*>(wa_lds + 2 * WA_XT_BYTES + WA_REL_BYTES + WA_RELT_BYTES + WA_STAT_BYTES + WA_TT_BYTES);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hl = lane >> 5;
  float* rw = reinterpret_cast<float*>(xb) + wave * (2 * 32 * WA_RW);
  const int h = (int)(blockIdx.x % (unsigned)heads);
  const int64_t slab = blockIdx.x / (unsigned)heads;
  const bf16_t *qh = q + 64 * h, *kh = k + 64 * h, *vh = v + 64 * h, *doh = dout + 64 * h;
  const bf16_t* biash = bias ? bias + (int64_t)h * 65536 : nullptr;
  const bool has_rel = rel_h != nullptr;
  float* slabh = dbias_slabs ? dbias_slabs + (slab * heads + h) * 65536 : nullptr;
  const int64_t bw0 = slab * per, bw1 = bw0 + per < BW ? bw0 + per : BW;
  if (has_rel) wa_stage_rel(rel, relt, rel_h, rel_w, tid);
  if (slabh && bw0 >= bw1)  // an empty share still owns its slab
    for (int e = tid; e < 16384; e += 256) reinterpret_cast<f32x4*>(slabh)[e] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
  for (int64_t bw = bw0; bw < bw1; ++bw) {
    const int64_t row0 = wa_row0(bw, Hg, Wg);
    const bool first = bw == bw0;
    __syncthreads();  // the previous item is done with Q^T, dO^T and G^T
    wa_stage_T(xa, kh, row0, Wg, ld, tid);
    __syncthreads();
    // ---- query pass ----
  #pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
      const int i = 64 * wave + 32 * pass + r;
      const int64_t row = wa_row(row0, Wg, i);
      bf16x8 qf[4], dof[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        qf[s] = wa_frag(qh + row * ld, s, hl);
        dof[s] = wa_frag(doh + row * ldo, s, hl);
      }
      float th[16], tw[8];
      wa_rel_q(has_rel ? rel : nullptr, rw, qf, i, lane, th, tw);
      if (has_rel) {  // the tables for the key pass
        if (hl == 0) {
#pragma unroll
          for (int e = 0; e < 16; ++e) tt[i * WA_TT + e] = th[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) tt[(256 + i) * WA_TT + (e & 3) + 8 * (e >> 2) + 4 * hl] = tw[e];
      }
      // sweep 1: m, l = sum exp(s - m) and cu = sum exp(s - m) dp over the lane's 128 keys, tile by tile (the running maximum rescales
      // l and cu), then the partner lane's 128
      float m = -INFINITY, l = 0.f, cu = 0.f;
      const float* thr = rw + r * WA_RW + (i >> 4) + 15;  // Th[i][jy] = thr[-jy]: table 0 of the scratch stays for both sweeps
#pragma unroll 1
      for (int t = 0; t < 8; ++t) {
        const float th0 = has_rel ? thr[-2 * t] : 0.f, th1 = has_rel ? thr[-2 * t - 1] : 0.f;
        const f32x16 sc = wa_score_tile(kh, biash, row0, Wg, ld, qf, i, lane, scale, th0, th1, tw, t);
        f32x16 dp = wa_zero();
        const bf16_t* vrow = vh + wa_row(row0, Wg, 32 * t + r) * ld;
#pragma unroll
        for (int s = 0; s < 4; ++s) dp = wa_mma(wa_frag(vrow, s, hl), dof[s], dp);
        float mt = m;
#pragma unroll
        for (int e = 0; e < 16; ++e) mt = fmaxf(mt, sc[e]);
        const float al = __expf(m - mt);  // 0 at the first tile (m = -inf)
        l *= al;
        cu *= al;
        m = mt;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float ex = __expf(sc[e] - m);
          l += ex;
          cu = fmaf(ex, dp[e], cu);
        }
      }
      {
        const float mo = __shfl_xor(m, 32), lo = __shfl_xor(l, 32), co = __shfl_xor(cu, 32);
        const float mn = fmaxf(m, mo), a0 = __expf(m - mn), a1 = __expf(mo - mn);
        l = l * a0 + lo * a1;  // (products, then one sum: the same bits in both lanes)
        cu = cu * a0 + co * a1;
        m = mn;
      }
      const float inv = 1.0f / l;
      const float c = cu * inv;
      if (hl == 0) {
        stat[i] = m;
        stat[256 + i] = inv;
        stat[512 + i] = c;
      }
      // sweep 2: the same tiles again, p = exp(s - m) / l, ds = p (dp - c)
      float dtw[8];  // dTw[i][jx] of the lane's eight jx; dTh[i][2 t], [2 t + 1] leave with their tile (table 1 of the scratch is free)
#pragma unroll
      for (int e = 0; e < 8; ++e) dtw[e] = 0.f;
      f32x16 acc[2] = {wa_zero(), wa_zero()};
#pragma unroll 1
      for (int t = 0; t < 8; ++t) {
        const float th0 = has_rel ? thr[-2 * t] : 0.f, th1 = has_rel ? thr[-2 * t - 1] : 0.f;
        f32x16 ds = wa_score_tile(kh, biash, row0, Wg, ld, qf, i, lane, scale, th0, th1, tw, t);
        f32x16 dp = wa_zero();
        const bf16_t* vrow = vh + wa_row(row0, Wg, 32 * t + r) * ld;
#pragma unroll
        for (int s = 0; s < 4; ++s) dp = wa_mma(wa_frag(vrow, s, hl), dof[s], dp);
        float d0 = 0.f, d1 = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const float pe = __expf(ds[e] - m) * inv;
          ds[e] = pe * (dp[e] - c);
          if (e < 8) d0 += ds[e];
          else d1 += ds[e];
          dtw[(e & 3) + 4 * ((e >> 2) & 1)] += ds[e];
        }
        if (has_rel) {
          d0 += __shfl_xor(d0, 32);
          d1 += __shfl_xor(d1, 32);
          if (hl == 0) {
            rw[(32 + r) * WA_RW + 2 * t] = d0;
            rw[(32 + r) * WA_RW + 2 * t + 1] = d1;
          }
        }
        if (slabh) {
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            f32x4* p4 = reinterpret_cast<f32x4*>(slabh + (int64_t)i * 256 + 32 * t + 8 * g + 4 * hl);
            f32x4 x = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (!first) x = *p4;
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] += ds[4 * g + e];
            *p4 = x;
          }
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bf16x8 df = wa_acc_frag(ds, s);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) acc[dt] = wa_mma(wa_frag_perm(xa + (32 * dt + r) * WA_XT, 32 * t, s, hl), df, acc[dt]);
        }
      }
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[dt][e] *= scale;
      if (has_rel) {
        // the lane's eight dTw join the dTh in table 1 of the scratch: row r = dTh[0..15] | dTw[0..15]
#pragma unroll
        for (int e = 0; e < 8; ++e) rw[(32 + r) * WA_RW + 16 + (e & 3) + 8 * (e >> 2) + 4 * hl] = dtw[e];
      }
      __syncthreads();
      if (has_rel) {
        const int iy = i >> 4, ix = i & 15;
#pragma unroll
        for (int tbl = 0; tbl < 2; ++tbl)
#pragma unroll
          for (int s = 0; s < 2; ++s) {
            bf16x8 gf;  // G[i][offset = 16 s + 8 hl + j] = dT[i][(iy | ix) + 15 - offset], 0 outside the window
#pragma unroll
            for (int j = 0; j < 8; ++j) {
              const int off = 16 * s + 8 * hl + j, idx = (tbl ? ix : iy) + 15 - off;
              const float gv = (idx >= 0 && idx < 16) ? rw[(32 + r) * WA_RW + 16 * tbl + (idx & 15)] : 0.f;
              gf[j] = (bf16_t)gv;
              gt[(tbl * 32 + off) * WA_XT + i] = gf[j];
            }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) acc[dt] = wa_mma(wa_frag(relt + (tbl * 64 + 32 * dt + r) * WA_RT, s, hl), gf, acc[dt]);
          }
      }
      wa_store_T(dq + row * ldg + 64 * h, acc, 1.0f, hl);
      __syncthreads();
    }
    // ---- key pass ----
    __syncthreads();
    wa_stage_T(xa, qh, row0, Wg, ld, tid);
    wa_stage_T(xb, doh, row0, Wg, ldo, tid);
    __syncthreads();
  #pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
      const int j = 64 * wave + 32 * pass + r, jy = j >> 4, jx = j & 15;
      const int64_t row = wa_row(row0, Wg, j);
      bf16x8 kf[4], vf[4];
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        kf[s] = wa_frag(kh + row * ld, s, hl);
        vf[s] = wa_frag(vh + row * ld, s, hl);
      }
      f32x16 adk[2] = {wa_zero(), wa_zero()}, adv[2] = {wa_zero(), wa_zero()};
#pragma unroll 1
      for (int u = 0; u < 8; ++u) {
        f32x16 sa = wa_zero(), da = wa_zero();
        const int64_t urow = wa_row(row0, Wg, 32 * u + r);
        const bf16_t *qrow = wa_opaque(qh) + urow * ld, *dorow = wa_opaque(doh) + urow * ldo;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
          sa = wa_mma(wa_frag(qrow, s, hl), kf[s], sa);
          da = wa_mma(wa_frag(dorow, s, hl), vf[s], da);
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = 32 * u + (e & 3) + 8 * (e >> 2) + 4 * hl;
          float s = scale * sa[e];
          s += biash ? (float)biash[(int64_t)i * 256 + j] : 0.f;
          s += has_rel ? tt[i * WA_TT + jy] : 0.f;
          s += has_rel ? tt[(256 + i) * WA_TT + jx] : 0.f;
          const float p = __expf(s - stat[i]) * stat[256 + i];
          sa[e] = p;
          da[e] = p * (da[e] - stat[512 + i]);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          const bf16x8 pf = wa_acc_frag(sa, s), df = wa_acc_frag(da, s);
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) {
            adv[dt] = wa_mma(wa_frag_perm(xb + (32 * dt + r) * WA_XT, 32 * u, s, hl), pf, adv[dt]);
            adk[dt] = wa_mma(wa_frag_perm(xa + (32 * dt + r) * WA_XT, 32 * u, s, hl), df, adk[dt]);
          }
        }
      }
      wa_store_T(dk + row * ldg + 64 * h, adk, scale, hl);
      wa_store_T(dv + row * ldg + 64 * h, adv, 1.0f, hl);
    }
    if (has_rel && drel_part) {  // drel[tbl][offset][d] += sum_i G[i][offset] q_i[d]: wave (tbl = wave >> 1, dt = wave & 1) owns one tile
      const int tbl = wave >> 1, dt = wave & 1;
      f32x16 acc = wa_zero();
#pragma unroll 4
      for (int ks = 0; ks < 16; ++ks)
        acc = wa_mma(wa_frag(gt + (tbl * 32 + r) * WA_XT, ks, hl), wa_frag(xa + (32 * dt + r) * WA_XT, ks, hl), acc);
      float* part = drel_part + ((int64_t)blockIdx.x * 2 + tbl) * (31 * 64) + 32 * dt + r;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int off = (e & 3) + 8 * (e >> 2) + 4 * hl;
        if (off < 31) part[off * 64] = (first ? 0.f : part[off * 64]) + acc[e];
      }
    }
  }
  if (drel_part && !(has_rel && bw0 < bw1))  // nothing was summed: the part is still written
    for (int e = tid; e < 2 * 31 * 64; e += 256) drel_part[(int64_t)blockIdx.x * (2 * 31 * 64) + e] = 0.f;
}

inline bool wa_aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the limits both entries share; `what` names the entry in the message
int wa_check_shape(const char* what, int64_t B, int64_t Hg, int64_t Wg, int64_t heads, int64_t hd, int64_t window) {
  OP_CHECK_ARG(hd == 64, "%s: hd = %lld, need 64", what, (long long)hd);
  OP_CHECK_ARG(window == 16, "%s: window = %lld, need 16", what, (long long)window);
  OP_CHECK_ARG(Hg >= 16 && Wg >= 16 && Hg % 16 == 0 && Wg % 16 == 0 && Hg < (1 << 20) && Wg < (1 << 20),
               "%s: grid %lld x %lld, need positive multiples of 16", what, (long long)Hg, (long long)Wg);
  OP_CHECK_ARG(heads >= 1 && heads < (int64_t(1) << 31), "%s: heads = %lld, need >= 1", what, (long long)heads);
  OP_CHECK_ARG(B >= 0, "%s: B = %lld, need >= 0", what, (long long)B);
  const int64_t windows = (Hg / 16) * (Wg / 16);
  OP_CHECK_ARG(B == 0 || windows * heads <= ((int64_t(1) << 31) - 1) / B, "%s: B * windows * heads = %lld * %lld * %lld, need < 2^31", what,
               (long long)B, (long long)windows, (long long)heads);
  return OP_OK;
}
int wa_check_ld(const char* what, const char* name, int64_t ld, int64_t heads) {
  OP_CHECK_ARG(ld % 8 == 0 && ld >= heads * 64, "%s: %s = %lld, need a multiple of 8 and >= heads * 64 = %lld", what, name, (long long)ld,
               (long long)(heads * 64));
  return OP_OK;
}
// shares of (b, window) a head's workgroups split: about one workgroup per compute unit of the 256
inline int64_t wa_slabs(int64_t BW, int64_t heads) {
  int64_t s = 256 / heads;
  if (s < 1) s = 1;
  if (s > BW) s = BW;
  if (s < 1) s = 1;
  const int64_t per = (BW + s - 1) / s;
  return per > 0 ? (BW + per - 1) / per : 1;  // no share is empty
}

}  // namespace

extern "C" int op_attn_window_parts(int64_t B, int64_t windows, int64_t heads, int64_t* parts, int64_t* slabs) {
  OP_CHECK_ARG(B >= 0 && windows >= 1 && heads >= 1 && parts && slabs, "op_attn_window_parts: B = %lld, windows = %lld, heads = %lld",
               (long long)B, (long long)windows, (long long)heads);
  const int64_t s = wa_slabs(B * windows, heads);
  *slabs = s;
  *parts = s * heads;
  return OP_OK;
}

extern "C" int op_attn_window_fwd(const void* q, const void* k, const void* v, int64_t ld, const void* bias, const void* rel_h,
                                  const void* rel_w, void* out, int64_t ldo, int64_t B, int64_t Hg, int64_t Wg, int64_t heads, int64_t hd,
                                  int64_t window, float scale, void* stream) {
  int rc = wa_check_shape("op_attn_window_fwd", B, Hg, Wg, heads, hd, window);
  if (rc == OP_OK) rc = wa_check_ld("op_attn_window_fwd", "ld", ld, heads);
  if (rc == OP_OK) rc = wa_check_ld("op_attn_window_fwd", "ldo", ldo, heads);
  if (rc != OP_OK) return rc;
  OP_CHECK_ARG(q && k && v && out, "op_attn_window_fwd: q, k, v and out must be non-null");
  OP_CHECK_ARG((rel_h == nullptr) == (rel_w == nullptr), "op_attn_window_fwd: rel_h and rel_w must be given together");
  OP_CHECK_ARG(wa_aligned16(q) && wa_aligned16(k) && wa_aligned16(v) && wa_aligned16(out) && wa_aligned16(bias) && wa_aligned16(rel_h) &&
                   wa_aligned16(rel_w),
               "op_attn_window_fwd: every pointer must be aligned to 16 bytes");
  if (B == 0) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  OP_ENSURE_LDS(attn_window_fwd_kernel, WA_FWD_LDS, "op_attn_window_fwd");
  const int64_t windows = (Hg / 16) * (Wg / 16);
  hipLaunchKernelGGL(attn_window_fwd_kernel, dim3((unsigned)(B * windows * heads)), dim3(256), WA_FWD_LDS, st, (const bf16_t*)q,
                     (const bf16_t*)k, (const bf16_t*)v, ld, (const bf16_t*)bias, (const bf16_t*)rel_h, (const bf16_t*)rel_w, (bf16_t*)out,
                     ldo, (int)Hg, (int)Wg, (int)heads, scale);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

extern "C" int op_attn_window_bwd(const void* q, const void* k, const void* v, int64_t ld, const void* bias, const void* rel_h,
                                  const void* rel_w, const void* dout, int64_t ldo, void* dq, void* dk, void* dv, int64_t ldg,
                                  void* drel_part, void* dbias_slabs, int64_t B, int64_t Hg, int64_t Wg, int64_t heads, int64_t hd,
                                  int64_t window, float scale, void* stream) {
  int rc = wa_check_shape("op_attn_window_bwd", B, Hg, Wg, heads, hd, window);
  if (rc == OP_OK) rc = wa_check_ld("op_attn_window_bwd", "ld", ld, heads);
  if (rc == OP_OK) rc = wa_check_ld("op_attn_window_bwd", "ldo", ldo, heads);
  if (rc == OP_OK) rc = wa_check_ld("op_attn_window_bwd", "ldg", ldg, heads);
  if (rc != OP_OK) return rc;
  OP_CHECK_ARG(q && k && v && dout && dq && dk && dv, "op_attn_window_bwd: q, k, v, dout, dq, dk and dv must be non-null");
  OP_CHECK_ARG((rel_h == nullptr) == (rel_w == nullptr), "op_attn_window_bwd: rel_h and rel_w must be given together");
  OP_CHECK_ARG(wa_aligned16(q) && wa_aligned16(k) && wa_aligned16(v) && wa_aligned16(dout) && wa_aligned16(dq) && wa_aligned16(dk) &&
                   wa_aligned16(dv) && wa_aligned16(bias) && wa_aligned16(rel_h) && wa_aligned16(rel_w) && wa_aligned16(drel_part) &&
                   wa_aligned16(dbias_slabs),
               "op_attn_window_bwd: every pointer must be aligned to 16 bytes");
  if (B == 0) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  OP_ENSURE_LDS(attn_window_bwd_kernel, WA_BWD_LDS, "op_attn_window_bwd");
  // without slabs and parts nothing ties the items of a share together: one (b, window, head) per workgroup, as in the forward
  const int64_t BW = B * (Hg / 16) * (Wg / 16), slabs = (drel_part || dbias_slabs) ? wa_slabs(BW, heads) : BW;
  const int64_t per = (BW + slabs - 1) / slabs;
  hipLaunchKernelGGL(attn_window_bwd_kernel, dim3((unsigned)(slabs * heads)), dim3(256), WA_BWD_LDS, st, (const bf16_t*)q, (const bf16_t*)k,
                     (const bf16_t*)v, ld, (const bf16_t*)bias, (const bf16_t*)rel_h, (const bf16_t*)rel_w, (const bf16_t*)dout, ldo,
                     (bf16_t*)dq, (bf16_t*)dk, (bf16_t*)dv, ldg, (float*)drel_part, (float*)dbias_slabs, BW, (int)per, (int)Hg, (int)Wg,
                     (int)heads, scale);
  OP_LAUNCH_CHECK();
  return OP_OK;
}
