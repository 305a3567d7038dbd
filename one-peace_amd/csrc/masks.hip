// Pretraining masks on the device: image patches, whole words, audio blocks (include/onepeace_hip.h, "pretraining masks").
//
// Every random choice is select(candidates, k, keys): the k items first in the order (key descending, index ascending) over the
// candidates, the row's other items after them in index order.  One workgroup per (row, mask kind) holds the row's sort words in LDS,
//   candidate      (uint64(key + 1) << 32) | (0xFFFFFFFF - index)
//   other item                               (0xFFFFFFFF - index)
//   beyond the row  0
// sorts them DESCENDING with a bitonic network over the next power of two, marks the first k, and compacts the kept positions with
// __ballot / popcount inside a wave and a prefix over the four wave totals in LDS.  No global scratch, no atomics: the outputs are a pure
// function of (inputs, keys, counts), and two runs give the same bits.
#include <cmath>

#include "common.h"

namespace {

constexpr int MK_THREADS = 256;  // four waves
constexpr int MK_WAVES = MK_THREADS / 64;
constexpr int MK_MAX = 4096;     // items per row (positions without CLS): 1024 x 1024 images, 80 s of audio

struct MkShared {
  uint64_t w[MK_MAX];  // sort words
  uint8_t f[MK_MAX];   // the mask being built, per item
  uint8_t g[MK_MAX];   // words: the word-start bits; second masks: the first mask
  int part[MK_WAVES];
  int total;
};

__device__ __forceinline__ int mk_pow2(int n) {
  int p = 2;
  while (p < n) p <<= 1;
  return p;
}

// sum of v over the workgroup, the same value in every thread (two barriers; sh.part / sh.total are free again on return)
__device__ __forceinline__ int mk_block_sum(MkShared& sh, int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) sh.part[threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int i = 0; i < MK_WAVES; ++i) t += sh.part[i];
  __syncthreads();
  return t;
}

__device__ __forceinline__ uint64_t mk_word(bool in_row, bool cand, int key, int i) {
  if (!in_row) return 0;
  const uint64_t lo = 0xFFFFFFFFu - (unsigned)i;
  return cand ? ((uint64_t)(((unsigned)key & 0x7FFFFFFFu) + 1u) << 32) | lo : lo;
}

// sh.w[0 .. n2) descending.  Enters and leaves with a barrier.
__device__ void mk_sort(MkShared& sh, int n2) {
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < n2; i += MK_THREADS) {
        const int x = i ^ j;
        if (x > i) {
          const uint64_t a = sh.w[i], b = sh.w[x];
          if (((i & k) == 0) ? a < b : a > b) {
            sh.w[i] = b;
            sh.w[x] = a;
          }
        }
      }
      __syncthreads();
    }
  }
}

// dst[item] = value for the first k sorted items (k <= the items of the row, so no zero word is among them).  Leaves with a barrier.
__device__ __forceinline__ void mk_mark(MkShared& sh, uint8_t* dst, int k, uint8_t value) {
  for (int j = threadIdx.x; j < k; j += MK_THREADS) {
    const uint64_t w = sh.w[j];
    if (w != 0) dst[0xFFFFFFFFu - (unsigned)(w & 0xFFFFFFFFu)] = value;
  }
  __syncthreads();
}

// Position 0 is CLS, item t sits at position t + 1; positions [0, rowlen) belong to the row, [rowlen, S) are padding.
// mask[pos] = masked (False on CLS and padding) for pos < S; ids = the ascending kept positions of the row, then -1 up to width; kept
// positions beyond width are dropped.  Returns the row's kept count (not truncated).
__device__ int mk_emit(MkShared& sh, const uint8_t* f, int rowlen, int S, uint8_t* __restrict__ mask, int64_t* __restrict__ ids, int width) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int run = 0;
  for (int base = 0; base < S; base += MK_THREADS) {
    const int pos = base + threadIdx.x;
    const bool masked = pos >= 1 && pos < rowlen && f[pos - 1] != 0;
    const bool kept = pos < rowlen && !masked;
    const unsigned long long bal = __ballot(kept);
    if (lane == 0) sh.part[wave] = __popcll(bal);
    __syncthreads();
    int before = 0, all = 0;
#pragma unroll
    for (int i = 0; i < MK_WAVES; ++i) {
      before += i < wave ? sh.part[i] : 0;
      all += sh.part[i];
    }
    const int slot = run + before + __popcll(bal & ((1ull << lane) - 1ull));
    if (kept && slot < width) ids[slot] = pos;
    if (pos < S) mask[pos] = masked ? 1 : 0;
    run += all;
    __syncthreads();
  }
  for (int i = run + threadIdx.x; i < width; i += MK_THREADS) ids[i] = -1;
  return run;
}

// ---- patches --------------------------------------------------------------------------------------------------------------------
// blockIdx.y = 0: the image mask = select(all, m1, keys_a).  1: the vl mask = (not image-masked) U select(image-masked, extra, keys_b).
__global__ __launch_bounds__(MK_THREADS) void mask_patches_kernel(const int* __restrict__ keys_a, const int* __restrict__ keys_b, int N, int m1,
                                                                  int extra, uint8_t* __restrict__ mask, int64_t* __restrict__ ids,
                                                                  uint8_t* __restrict__ vl_mask, int64_t* __restrict__ vl_ids) {
  __shared__ MkShared sh;
  const int64_t b = blockIdx.x;
  const int kind = blockIdx.y, n2 = mk_pow2(N), S = N + 1;
  const int* ka = keys_a + b * N;
  for (int i = threadIdx.x; i < n2; i += MK_THREADS) {
    sh.w[i] = mk_word(i < N, true, i < N ? ka[i] : 0, i);
    if (i < N) sh.f[i] = 0;
  }
  mk_sort(sh, n2);
  mk_mark(sh, sh.f, m1, 1);
  if (kind == 0) {
    mk_emit(sh, sh.f, S, S, mask + b * S, ids + b * (S - m1), S - m1);
    return;
  }
  const int* kb = keys_b + b * N;
  for (int i = threadIdx.x; i < n2; i += MK_THREADS) {
    sh.w[i] = mk_word(i < N, i < N && sh.f[i] != 0, i < N ? kb[i] : 0, i);
    if (i < N) sh.g[i] = sh.f[i] ? 0 : 1;
  }
  mk_sort(sh, n2);
  mk_mark(sh, sh.g, extra, 1);
  const int keep = m1 - extra + 1;
  mk_emit(sh, sh.g, S, S, vl_mask + b * S, vl_ids + b * keep, keep);
}

// ---- whole words ----------------------------------------------------------------------------------------------------------------
// blockIdx.y = 0: k = ceil(float32(W) * p) word starts chosen by keys_a, each extended over its word.  1: on top of that,
// select(tokens not masked by 0, int(n * vl_ratio), keys_b).  counts[kind * B + b] = the row's kept positions.
__global__ __launch_bounds__(MK_THREADS) void mask_words_kernel(const int64_t* __restrict__ src, int64_t ld, int64_t B, int L, int64_t pad,
                                                                const uint8_t* __restrict__ table, int64_t vocab, const int* __restrict__ keys_a,
                                                                const int* __restrict__ keys_b, float p, double vl_ratio,
                                                                uint8_t* __restrict__ mask, int64_t* __restrict__ ids, int width,
                                                                uint8_t* __restrict__ vl_mask, int64_t* __restrict__ vl_ids, int vl_width,
                                                                int* __restrict__ counts) {
  __shared__ MkShared sh;
  const int64_t b = blockIdx.x;
  const int kind = blockIdx.y, n2 = mk_pow2(L), S = L + 1;
  const int64_t* row = src + b * ld;
  int c = 0;
  for (int i = threadIdx.x; i < L; i += MK_THREADS) c += row[i] != pad;
  const int nonpad = mk_block_sum(sh, c);
  const int n = nonpad > 0 ? nonpad - 1 : 0;  // the caption's tokens; token n is eos
  c = 0;
  for (int i = threadIdx.x; i < L; i += MK_THREADS) {
    uint8_t ws = 0;
    if (i < n) {
      const int64_t t = row[i];
      ws = t >= 0 && t < vocab && table[t] != 0;
    }
    sh.g[i] = ws;
    sh.f[i] = 0;
    c += ws;
  }
  const int W = mk_block_sum(sh, c);
  int k = (int)ceilf(__fmul_rn((float)W, p));
  k = k < 0 ? 0 : (k > W ? W : k);
  const int* ka = keys_a + b * L;
  for (int i = threadIdx.x; i < n2; i += MK_THREADS) sh.w[i] = mk_word(i < n, i < n && sh.g[i] != 0, i < n ? ka[i] : 0, i);
  mk_sort(sh, n2);
  mk_mark(sh, sh.f, k, 1);
  // a chosen start covers the tokens after it that start no word, up to the next start or the end of the caption.  Only starts are
  // tested, only non-starts are written: no thread reads what another writes
  for (int i = threadIdx.x; i < n; i += MK_THREADS)
    if (sh.g[i] && sh.f[i])
      for (int u = i + 1; u < n && !sh.g[u]; ++u) sh.f[u] = 1;
  __syncthreads();
  if (kind == 0) {
    const int kept = mk_emit(sh, sh.f, nonpad + 1, S, mask + b * S, ids + b * width, width);
    if (threadIdx.x == 0) counts[b] = kept;
    return;
  }
  int k2 = (int)((double)n * vl_ratio);
  k2 = k2 < 0 ? 0 : (k2 > n ? n : k2);
  const int* kb = keys_b + b * L;
  for (int i = threadIdx.x; i < n2; i += MK_THREADS) {
    sh.w[i] = mk_word(i < n, i < n && sh.f[i] == 0, i < n ? kb[i] : 0, i);
    if (i < L) sh.g[i] = 0;
  }
  mk_sort(sh, n2);
  mk_mark(sh, sh.g, k2, 1);
  const int kept = mk_emit(sh, sh.g, nonpad + 1, S, vl_mask + b * S, vl_ids + b * vl_width, vl_width);
  if (threadIdx.x == 0) counts[B + b] = kept;
}

// ---- blocks ---------------------------------------------------------------------------------------------------------------------
// rows[b] = (T, K, target).  Spans of `length` frames around the K centres, clamped to the clip; then frames are masked or unmasked by
// keys until exactly `target` are masked.
__global__ __launch_bounds__(MK_THREADS) void mask_blocks_kernel(const int* __restrict__ rows, const int* __restrict__ centers, int Kmax,
                                                                 const int* __restrict__ keys, int Tmax, int length,
                                                                 uint8_t* __restrict__ mask, int64_t* __restrict__ ids, int width) {
  __shared__ MkShared sh;
  const int64_t b = blockIdx.x;
  const int S = Tmax + 1;
  int T = rows[3 * b], K = rows[3 * b + 1], target = rows[3 * b + 2];
  T = T < 0 ? 0 : (T > Tmax ? Tmax : T);  // (the entry has checked the host copy of the table; the clamps keep a differing device copy in bounds)
  K = T == 0 || K < 0 ? 0 : (K > Kmax ? Kmax : K);
  target = target < 0 ? 0 : (target > T ? T : target);
  for (int i = threadIdx.x; i < T; i += MK_THREADS) sh.f[i] = 0;
  __syncthreads();
  const int* cen = centers + b * Kmax;
  const int off = length / 2;
  for (int j = threadIdx.x; j < K; j += MK_THREADS) {
    const int64_t c0 = (int64_t)cen[j] - off;
    for (int i = 0; i < length; ++i) {
      const int64_t q = c0 + i;
      sh.f[q < 0 ? 0 : (q > T - 1 ? T - 1 : (int)q)] = 1;  // (several threads may store the same 1)
    }
  }
  __syncthreads();
  int c = 0;
  for (int i = threadIdx.x; i < T; i += MK_THREADS) c += sh.f[i];
  const int n = mk_block_sum(sh, c);
  if (n != target) {  // uniform
    const bool drop = n > target;
    const int n2 = mk_pow2(T);
    const int* kr = keys + b * Tmax;
    for (int i = threadIdx.x; i < n2; i += MK_THREADS) sh.w[i] = mk_word(i < T, i < T && (sh.f[i] != 0) == drop, i < T ? kr[i] : 0, i);
    mk_sort(sh, n2);
    mk_mark(sh, sh.f, drop ? n - target : target - n, drop ? 0 : 1);
  }
  mk_emit(sh, sh.f, T + 1, S, mask + b * S, ids + b * width, width);
}

bool mk_aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" int op_mask_patches(const int* keys_a, const int* keys_b, int64_t B, int64_t N, int64_t m1, int64_t extra, uint8_t* mask,
                               int64_t* ids, uint8_t* vl_mask, int64_t* vl_ids, void* stream) {
  const char* what = "op_mask_patches";
  OP_CHECK_ARG(N >= 1 && N <= MK_MAX, "%s: N = %lld patches, need 1 ... %d", what, (long long)N, MK_MAX);
  OP_CHECK_ARG(B >= 0 && B <= 0x7FFFFFFF, "%s: B = %lld, need 0 ... 2^31 - 1", what, (long long)B);
  OP_CHECK_ARG(m1 >= 0 && m1 <= N, "%s: m1 = %lld masked patches, need 0 ... N = %lld", what, (long long)m1, (long long)N);
  const bool vl = vl_mask || vl_ids || keys_b;
  if (vl) OP_CHECK_ARG(extra >= 0 && extra <= m1, "%s: extra = %lld, need 0 ... m1 = %lld", what, (long long)extra, (long long)m1);
  if (B == 0) return OP_OK;
  OP_CHECK_ARG(keys_a && mask && ids && (!vl || (keys_b && vl_mask && vl_ids)), "%s: null pointer", what);
  OP_CHECK_ARG(mk_aligned(keys_a, 4) && mk_aligned(keys_b, 4) && mk_aligned(ids, 8) && mk_aligned(vl_ids, 8),
               "%s: keys must be 4-byte aligned, ids 8-byte aligned", what);
  hipLaunchKernelGGL(mask_patches_kernel, dim3((unsigned)B, vl ? 2 : 1), dim3(MK_THREADS), 0, (hipStream_t)stream, keys_a, keys_b, (int)N, (int)m1,
                     (int)extra, mask, ids, vl_mask, vl_ids);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

extern "C" int op_mask_words(const int64_t* src_tokens, int64_t ld, int64_t B, int64_t L, int64_t pad, const uint8_t* table, int64_t vocab,
                             const int* keys_a, const int* keys_b, float p, double vl_ratio, uint8_t* mask, int64_t* ids, int64_t width,
                             uint8_t* vl_mask, int64_t* vl_ids, int64_t vl_width, int* counts, void* stream) {
  const char* what = "op_mask_words";
  OP_CHECK_ARG(L >= 1 && L <= MK_MAX, "%s: L = %lld tokens per row, need 1 ... %d", what, (long long)L, MK_MAX);
  OP_CHECK_ARG(B >= 0 && B <= 0x7FFFFFFF, "%s: B = %lld, need 0 ... 2^31 - 1", what, (long long)B);
  OP_CHECK_ARG(ld >= L, "%s: ld = %lld < L = %lld", what, (long long)ld, (long long)L);
  OP_CHECK_ARG(vocab >= 1, "%s: vocab = %lld, need >= 1", what, (long long)vocab);
  OP_CHECK_ARG(p >= 0.f && p <= 1.f, "%s: p = %g, need 0 ... 1", what, (double)p);
  OP_CHECK_ARG(width >= 0 && width <= L + 1, "%s: width = %lld, need 0 ... L + 1 = %lld", what, (long long)width, (long long)(L + 1));
  const bool vl = vl_mask || vl_ids || keys_b;
  if (vl) {
    OP_CHECK_ARG(vl_ratio >= 0.0 && vl_ratio <= 1.0, "%s: vl_ratio = %g, need 0 ... 1", what, vl_ratio);
    OP_CHECK_ARG(vl_width >= 0 && vl_width <= L + 1, "%s: vl_width = %lld, need 0 ... L + 1 = %lld", what, (long long)vl_width, (long long)(L + 1));
  }
  if (B == 0) return OP_OK;
  OP_CHECK_ARG(src_tokens && table && keys_a && mask && (ids || width == 0) && counts &&
                   (!vl || (keys_b && vl_mask && (vl_ids || vl_width == 0))),
               "%s: null pointer", what);
  OP_CHECK_ARG(mk_aligned(src_tokens, 8) && mk_aligned(keys_a, 4) && mk_aligned(keys_b, 4) && mk_aligned(ids, 8) && mk_aligned(vl_ids, 8) &&
                   mk_aligned(counts, 4),
               "%s: tokens and ids must be 8-byte aligned, keys and counts 4-byte aligned", what);
  hipLaunchKernelGGL(mask_words_kernel, dim3((unsigned)B, vl ? 2 : 1), dim3(MK_THREADS), 0, (hipStream_t)stream, src_tokens, ld, B, (int)L, pad, table,
                     vocab, keys_a, keys_b, p, vl_ratio, mask, ids, (int)width, vl_mask, vl_ids, (int)vl_width, counts);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

extern "C" int op_mask_blocks(const int* rows, const int* rows_host, const int* centers, int64_t Kmax, const int* keys, int64_t Tmax, int64_t B,
                              int64_t length, uint8_t* mask, int64_t* ids, int64_t width, void* stream) {
  const char* what = "op_mask_blocks";
  OP_CHECK_ARG(Tmax >= 1 && Tmax <= MK_MAX, "%s: Tmax = %lld frames, need 1 ... %d", what, (long long)Tmax, MK_MAX);
  OP_CHECK_ARG(Kmax >= 0 && Kmax <= MK_MAX, "%s: Kmax = %lld centres, need 0 ... %d", what, (long long)Kmax, MK_MAX);
  OP_CHECK_ARG(B >= 0 && B <= 0x7FFFFFFF, "%s: B = %lld, need 0 ... 2^31 - 1", what, (long long)B);
  OP_CHECK_ARG(length >= 1 && length <= MK_MAX, "%s: length = %lld, need 1 ... %d", what, (long long)length, MK_MAX);
  OP_CHECK_ARG(width >= 1 && width <= Tmax + 1, "%s: width = %lld, need 1 ... Tmax + 1 = %lld", what, (long long)width, (long long)(Tmax + 1));
  if (B == 0) return OP_OK;
  OP_CHECK_ARG(rows && rows_host && keys && mask && ids && (centers || Kmax == 0), "%s: null pointer", what);
  OP_CHECK_ARG(mk_aligned(rows, 4) && mk_aligned(rows_host, 4) && mk_aligned(centers, 4) && mk_aligned(keys, 4) && mk_aligned(ids, 8),
               "%s: rows, centers and keys must be 4-byte aligned, ids 8-byte aligned", what);
  for (int64_t b = 0; b < B; ++b) {
    const int T = rows_host[3 * b], K = rows_host[3 * b + 1], target = rows_host[3 * b + 2];
    OP_CHECK_ARG(T >= 0 && T <= Tmax && K >= 0 && K <= Kmax && target >= 0 && target <= T && (T > 0 || K == 0),
                 "%s: row %lld (T %d, K %d, target %d): need 0 <= T <= Tmax = %lld, 0 <= K <= Kmax = %lld (0 when T is 0), 0 <= target <= T", what,
                 (long long)b, T, K, target, (long long)Tmax, (long long)Kmax);
    OP_CHECK_ARG((int64_t)T + 1 - target <= width, "%s: row %lld keeps %d positions, width = %lld", what, (long long)b, T + 1 - target,
                 (long long)width);
  }
  hipLaunchKernelGGL(mask_blocks_kernel, dim3((unsigned)B), dim3(MK_THREADS), 0, (hipStream_t)stream, rows, centers, (int)Kmax, keys, (int)Tmax,
                     (int)length, mask, ids, (int)width);
  OP_LAUNCH_CHECK();
  return OP_OK;
}
