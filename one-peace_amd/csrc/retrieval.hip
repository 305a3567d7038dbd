// Similarity top-k for retrieval (include/onepeace_hip.h: op_sim_topk).  Replaces the materialised score matrix of the reference's
// Recall metric (one_peace/metrics/recall.py:31-51: image_logits @ text_logits.t(), then topk(10) in each direction): for every query
// row the k best gallery rows are found without the [M, N] scores ever reaching global memory.
//
// sim_topk_kernel: a workgroup (4 waves) owns 128 query rows and walks a contiguous range of 128-column gallery tiles (its split).  Per
// tile the 128 x 128 scores are an MFMA GEMM tile (v_mfma_f32_16x16x32_bf16, each wave 64 x 64, K staged through LDS 64 at a time);
// then the scores are compared, in registers, against a per-row threshold = the row's current k-th best key.  Only keys above it
// are appended to a per-row candidate buffer in LDS, and one thread per row inserts them into its sorted list (LDS).  With one split
// the lists are the result; otherwise they go to the workspace [M, splits, k] and sim_topk_merge_kernel picks the k best per row.
//
// Order: key = (ordered fp32 bits << 32) | ~n, larger wins -> higher score first, lower gallery index first on exact ties; every NaN
// is +NaN and ranks above +inf (as torch.topk), -0 counts as +0.  Keys are unique, so the top-k SET is unique.  Every pair's dot
// product accumulates its 32-wide k steps in the same order from zero whatever the tile / split, so the scores -- and hence the
// result -- are bit-identical for every split count.
#include "common.h"

#include <algorithm>

namespace {

constexpr int ST_BM = 128, ST_BN = 128, ST_BK = 64;
constexpr int ST_PITCH = ST_BK + 8;  // bf16 per LDS operand row: 144 B, so the 16 rows of a fragment read fall on distinct banks
constexpr int ST_CAP = 32;            // candidates per row and round: 2 waves x 16 columns
constexpr int ST_THREADS = 256;
constexpr int ST_MAX_K = 64, ST_MAX_SPLITS = 512, ST_MERGE_HEADS = ST_MAX_SPLITS / 64;
constexpr int ST_SLOTS = 512;  // resident workgroups: 256 CUs x 2 (the kernel's registers allow two per CU)
constexpr int ST_OPND_BYTES = 2 * ST_BM * ST_PITCH * 2;            // Q and G tiles; the candidate buffer aliases them
constexpr int ST_FIXED_BYTES = ST_OPND_BYTES + ST_BM * 8 + ST_BM * 4;  // + thresholds + candidate counts
static_assert(ST_BM * ST_CAP * 8 <= ST_OPND_BYTES, "candidate buffer must fit in the operand tiles");

__device__ __forceinline__ uint32_t st_ordered(float s) {
  uint32_t u = __float_as_uint(s);
  if (__builtin_isnan(s)) u = 0x7fc00000u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ uint64_t st_key(float s, uint32_t n) { return ((uint64_t)st_ordered(s) << 32) | (uint32_t)~n; }

__device__ __forceinline__ float st_score(uint64_t key) {
  const uint32_t o = (uint32_t)(key >> 32);
  return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

__device__ __forceinline__ int st_index(uint64_t key) { return (int)~(uint32_t)key; }

__global__ __launch_bounds__(ST_THREADS, 2) void sim_topk_kernel(const bf16_t* __restrict__ Q, int64_t ldq, const bf16_t* __restrict__ G,
                                                              int64_t ldg, int64_t M, int64_t N, int D, int k, int splits,
                                                              int64_t tiles_per_split, float* __restrict__ vals, int* __restrict__ idx,
                                                              uint64_t* __restrict__ ws) {
  extern __shared__ __align__(16) unsigned char smem[];
  bf16_t* sq = reinterpret_cast<bf16_t*>(smem);
  bf16_t* sg = sq + ST_BM * ST_PITCH;
  uint64_t* cand = reinterpret_cast<uint64_t*>(smem);  // only between K loops
  uint64_t* thr = reinterpret_cast<uint64_t*>(smem + ST_OPND_BYTES);
  int* cnt = reinterpret_cast<int*>(thr + ST_BM);
  uint64_t* list = reinterpret_cast<uint64_t*>(smem + ST_FIXED_BYTES);  // [ST_BM][k], descending, 0 = empty

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wm = wave >> 1, wn = wave & 1;
  const int fr = lane & 15, fk = (lane >> 4) * 8;  // fragment row / k offset of this lane
  const int64_t m0 = (int64_t)blockIdx.x * ST_BM;
  const int split = blockIdx.y;
  const int64_t ntiles = (N + ST_BN - 1) / ST_BN;
  const int64_t t_begin = (int64_t)split * tiles_per_split;
  const int64_t t_end = min(ntiles, t_begin + tiles_per_split);
  const int nk = (D + ST_BK - 1) / ST_BK;

  if (tid < ST_BM) {
    thr[tid] = 0;
    cnt[tid] = 0;
    for (int j = 0; j < k; ++j) list[tid * k + j] = 0;
  }
  __syncthreads();

  // global -> register staging: chunk i of this thread = 16 bytes at row (tid >> 3) + 32 i, k offset (tid & 7) * 8
  const int lrow = tid >> 3, lk = (tid & 7) * 8;
  for (int64_t t = t_begin; t < t_end; ++t) {
    const int64_t n0 = t * ST_BN;
    f32x4 acc[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int b = 0; b < 4; ++b) acc[a][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

    u32x4 rq[4], rg[4];
    auto load = [&](int k0) {
      const bool kin = k0 + lk < D;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int64_t mq = m0 + lrow + 32 * i, ng = n0 + lrow + 32 * i;
        rq[i] = (kin && mq < M) ? *reinterpret_cast<const u32x4*>(Q + mq * ldq + k0 + lk) : (u32x4){0u, 0u, 0u, 0u};
        rg[i] = (kin && ng < N) ? *reinterpret_cast<const u32x4*>(G + ng * ldg + k0 + lk) : (u32x4){0u, 0u, 0u, 0u};
      }
    };
    load(0);
    for (int ks = 0; ks < nk; ++ks) {
      __syncthreads();  // the previous step's fragment reads (or the previous tile's merge) are done
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        *reinterpret_cast<u32x4*>(sq + (lrow + 32 * i) * ST_PITCH + lk) = rq[i];
        *reinterpret_cast<u32x4*>(sg + (lrow + 32 * i) * ST_PITCH + lk) = rg[i];
      }
      __syncthreads();
      if (ks + 1 < nk) load((ks + 1) * ST_BK);
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        if (ks * ST_BK + s * 32 >= D) break;  // uniform: D % 64 == 32 leaves the last stage half full
        bf16x8 af[4], bf[4];
#pragma unroll
        for (int a = 0; a < 4; ++a) af[a] = *reinterpret_cast<const bf16x8*>(sq + (wm * 64 + a * 16 + fr) * ST_PITCH + s * 32 + fk);
#pragma unroll
        for (int b = 0; b < 4; ++b) bf[b] = *reinterpret_cast<const bf16x8*>(sg + (wn * 64 + b * 16 + fr) * ST_PITCH + s * 32 + fk);
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int b = 0; b < 4; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a], bf[b], acc[a][b], 0, 0, 0);
      }
    }
    __syncthreads();  // operand tiles -> candidate buffer

    // acc[a][b][i] = score of query row wm*64 + a*16 + (lane>>4)*4 + i and gallery column wn*64 + b*16 + (lane&15).
    // Round b: the 32 columns b of both column waves; at most ST_CAP candidates per row.
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int64_t n = n0 + wn * 64 + b * 16 + fr;
      if (n < N) {
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int row = wm * 64 + a * 16 + (lane >> 4) * 4 + i;
            const uint64_t key = st_key(acc[a][b][i], (uint32_t)n);
            if (m0 + row < M && key > thr[row]) cand[row * ST_CAP + atomicAdd(&cnt[row], 1)] = key;
          }
      }
      __syncthreads();
      if (tid < ST_BM) {
        const int c = cnt[tid];
        if (c) {
          uint64_t* L = list + tid * k;
          uint64_t lo = L[k - 1];
          for (int j = 0; j < c; ++j) {
            const uint64_t x = cand[tid * ST_CAP + j];
            if (x > lo) {
              int p = k - 1;
              while (p > 0 && L[p - 1] < x) {
                L[p] = L[p - 1];
                --p;
              }
              L[p] = x;
              lo = L[k - 1];
            }
          }
          thr[tid] = lo;
          cnt[tid] = 0;
        }
      }
      __syncthreads();
    }
  }

  if (tid < ST_BM && m0 + tid < M) {
    const uint64_t* L = list + tid * k;
    const int64_t m = m0 + tid;
    if (splits == 1) {
      for (int j = 0; j < k; ++j) {
        vals[m * k + j] = st_score(L[j]);
        idx[m * k + j] = st_index(L[j]);
      }
    } else {
      for (int j = 0; j < k; ++j) ws[(m * splits + split) * k + j] = L[j];
    }
  }
}

// One wave per query row: k rounds of "largest head among the splits' sorted lists"; lane l holds splits l, l + 64, ... (<= 8).
__global__ __launch_bounds__(256) void sim_topk_merge_kernel(const uint64_t* __restrict__ ws, int64_t M, int k, int splits,
                                                             float* __restrict__ vals, int* __restrict__ idx) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;
  const uint64_t* W = ws + row * splits * k;
  int pos[ST_MERGE_HEADS];
  uint64_t head[ST_MERGE_HEADS];
#pragma unroll
  for (int h = 0; h < ST_MERGE_HEADS; ++h) {
    const int s = lane + 64 * h;
    pos[h] = 0;
    head[h] = s < splits ? W[s * k] : 0;
  }
  for (int j = 0; j < k; ++j) {
    uint64_t best = head[0];
    int bh = 0;
#pragma unroll
    for (int h = 1; h < ST_MERGE_HEADS; ++h)
      if (head[h] > best) {
        best = head[h];
        bh = h;
      }
    uint64_t m = best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const uint64_t other = __shfl_xor(m, o);
      m = other > m ? other : m;
    }
    if (lane == 0) {
      vals[row * k + j] = st_score(m);
      idx[row * k + j] = st_index(m);
    }
    if (best == m && m != 0) {  // keys are unique: exactly one lane owns the winner
#pragma unroll
      for (int h = 0; h < ST_MERGE_HEADS; ++h)
        if (h == bh) {
          ++pos[h];
          head[h] = pos[h] < k ? W[(lane + 64 * h) * k + pos[h]] : 0;
        }
    }
  }
}

int64_t st_splits(int64_t M, int64_t N, int64_t splits) {
  const int64_t ntiles = (N + ST_BN - 1) / ST_BN, mblocks = (M + ST_BM - 1) / ST_BM;
  int64_t s = splits;
  if (s <= 0) {  // auto: the fewest splits that minimise (rounds of ST_SLOTS resident workgroups) x (tiles per workgroup)
    int64_t best = -1;
    for (int64_t c = 1; c <= std::min<int64_t>(ST_MAX_SPLITS, ntiles) && (c == 1 || mblocks * c <= 64 * ST_SLOTS); ++c) {
      const int64_t tps = (ntiles + c - 1) / c, cost = (mblocks * c + ST_SLOTS - 1) / ST_SLOTS * tps;
      if (best < 0 || cost < best) {
        best = cost;
        s = c;
      }
    }
  }
  s = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(s, ST_MAX_SPLITS), ntiles));
  const int64_t tps = (ntiles + s - 1) / s;
  return (ntiles + tps - 1) / tps;  // no empty split
}

}  // namespace

extern "C" int64_t op_sim_topk_splits(int64_t M, int64_t N, int64_t splits) {
  if (M <= 0 || N <= 0) return 1;
  return st_splits(M, N, splits);
}

extern "C" int64_t op_sim_topk_workspace_bytes(int64_t M, int64_t N, int64_t k, int64_t splits) {
  if (M <= 0 || N <= 0 || k <= 0) return 0;
  const int64_t s = st_splits(M, N, splits);
  return s == 1 ? 0 : M * s * k * 8;
}

extern "C" int op_sim_topk(const void* Q, int64_t ldq, const void* G, int64_t ldg, int64_t M, int64_t N, int64_t D, int64_t k,
                           float* vals, int* idx, void* workspace, int64_t workspace_bytes, int64_t splits, void* stream) {
  OP_CHECK_ARG(k >= 1 && k <= ST_MAX_K, "op_sim_topk: k = %lld, need 1 <= k <= %d", (long long)k, ST_MAX_K);
  OP_CHECK_ARG(N >= k && N < (int64_t(1) << 31), "op_sim_topk: N = %lld, need k <= N < 2^31", (long long)N);
  OP_CHECK_ARG(M >= 0, "op_sim_topk: M = %lld < 0", (long long)M);
  OP_CHECK_ARG(D > 0 && D % 32 == 0 && D < (int64_t(1) << 30), "op_sim_topk: D = %lld, need D %% 32 == 0 (zero-pad)", (long long)D);
  OP_CHECK_ARG(ldq >= D && ldg >= D && ldq % 8 == 0 && ldg % 8 == 0, "op_sim_topk: ldq = %lld, ldg = %lld, need >= D and %% 8 == 0",
               (long long)ldq, (long long)ldg);
  OP_CHECK_ARG(Q && G && vals && idx && ((uintptr_t)Q & 15) == 0 && ((uintptr_t)G & 15) == 0,
               "op_sim_topk: Q, G, vals, idx must be non-null, Q and G 16-byte aligned");
  OP_CHECK_ARG(splits >= 0 && splits <= ST_MAX_SPLITS, "op_sim_topk: splits = %lld, need 0 (auto) ... %d", (long long)splits,
               ST_MAX_SPLITS);
  if (M == 0) return OP_OK;
  const int64_t s = st_splits(M, N, splits);
  const int64_t need = s == 1 ? 0 : M * s * k * 8;
  OP_CHECK_ARG(need == 0 || (workspace && workspace_bytes >= need && ((uintptr_t)workspace & 7) == 0),
               "op_sim_topk: %lld splits need %lld workspace bytes (8-aligned), got %lld", (long long)s, (long long)need,
               (long long)workspace_bytes);
  const int64_t ntiles = (N + ST_BN - 1) / ST_BN;
  const int64_t tps = (ntiles + s - 1) / s;
  const int lds = ST_FIXED_BYTES + ST_BM * (int)k * 8;
  OP_ENSURE_LDS(sim_topk_kernel, ST_FIXED_BYTES + ST_BM * ST_MAX_K * 8, "op_sim_topk");
  hipStream_t st = (hipStream_t)stream;
  dim3 grid((unsigned)((M + ST_BM - 1) / ST_BM), (unsigned)s);
  hipLaunchKernelGGL(sim_topk_kernel, grid, dim3(ST_THREADS), lds, st, (const bf16_t*)Q, ldq, (const bf16_t*)G, ldg, M, N, (int)D,
                     (int)k, (int)s, tps, vals, idx, (uint64_t*)workspace);
  OP_LAUNCH_CHECK();
  if (s > 1) {
    hipLaunchKernelGGL(sim_topk_merge_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, st, (const uint64_t*)workspace, M, (int)k,
                       (int)s, vals, idx);
    OP_LAUNCH_CHECK();
  }
  return OP_OK;
}
