// Average precision per class for the MAP metric (include/onepeace_hip.h: op_average_precision).  Replaces the host path of the
// reference's MAP (one_peace/metrics/map.py:35-44: torch.sigmoid(preds).cpu().numpy(), then sklearn's average_precision_score(targets,
// preds, average=None) -- a device-to-host copy of the [N, C] scores and one host sort per class) with a sort-free count on the device:
//
//   AP_c = (1 / P_c) sum over positives i of TP_c(i) / CNT_c(i),   CNT_c(i) = #{j : s_jc >= s_ic},   TP_c(i) = #{j : y_jc = 1, s_jc >= s_ic}
//
// which is sklearn's sum over thresholds of (recall step) x precision with tied scores sharing one threshold.  The counts are integers;
// the only rounding is in the P_c fp64 divisions, their sum and the last division.
//
// ap_prepare_kernel: workgroup = 64 rows x 64 classes.  It reads scores and targets coalesced along the classes, turns them through LDS and
//   writes, class-major, the ordered uint32 key of every score (st_ordered of retrieval.hip: integer order = fp32 order, -0 = +0) and one
//   64-bit word of target bits per (class, 64 rows).
// ap_count_kernel: workgroup = (class, group of 64 positives); four waves.  It finds its positives from the class's target bits (popcount
//   prefix: the g-th group holds the positives of rank 64 g ... 64 g + 63 in sample order), takes one positive per lane -- the same 64 in
//   every wave -- and stages the class's keys through LDS in chunks of AP_CHUNK, next to a copy that holds 0 where the target is 0 (0 is
//   below the key of every float, so it is never counted).  Each wave scans a quarter of the chunk; all lanes read the same key (an LDS
//   broadcast) and the work is two integer compare-and-adds per pair.  The waves' counts are added in LDS (integers), wave 0 forms the 64
//   quotients, sums them with a shuffle butterfly and writes one fp64 partial per group.
// ap_finish_kernel: one thread per class adds the class's partials in group order and divides by P_c.
// The order of every floating-point sum is fixed by the class's own column: no floating-point atomics, nothing depends on C, on the row
// strides or on the launch geometry, so two runs -- and a column computed alone -- give the same bits.
#include "common.h"

#include <algorithm>

namespace {

constexpr int AP_THREADS = 256;
constexpr int AP_TILE = 64;              // rows and classes per transpose tile; rows per word of target bits; positives per group
constexpr int AP_PITCH = AP_TILE + 1;    // LDS tile pitch in dwords: column reads fall on distinct banks
constexpr int AP_CHUNK = 2048;           // keys staged per round: 512 per wave
constexpr int AP_TARGET_GROUPS = 4096;   // workgroups the counting grid aims for
constexpr int64_t AP_MAX_C = 65535;

__device__ __forceinline__ uint32_t ap_ordered(float s) {
  uint32_t u = __float_as_uint(s);
  if (__builtin_isnan(s)) u = 0x7fc00000u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__global__ __launch_bounds__(AP_THREADS) void ap_prepare_kernel(const float* __restrict__ scores, int64_t lds_, const uint8_t* __restrict__ targets,
                                                                int64_t ldt, int64_t N, int64_t C, int64_t W, uint32_t* __restrict__ keys,
                                                                uint64_t* __restrict__ mask) {
  __shared__ uint32_t tk[AP_TILE * AP_PITCH];
  __shared__ uint32_t ty[AP_TILE * AP_PITCH];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t n0 = (int64_t)blockIdx.x * AP_TILE, c0 = (int64_t)blockIdx.y * AP_TILE;
  {
    const int64_t cls = c0 + lane;
    for (int r = wave; r < AP_TILE; r += 4) {
      const int64_t row = n0 + r;
      const bool in = row < N && cls < C;
      tk[r * AP_PITCH + lane] = in ? ap_ordered(scores[row * lds_ + cls]) : 0u;
      ty[r * AP_PITCH + lane] = in ? (uint32_t)targets[row * ldt + cls] : 0u;
    }
  }
  __syncthreads();
  const int64_t row = n0 + lane;
  for (int cc = wave; cc < AP_TILE; cc += 4) {
    const int64_t cls = c0 + cc;
    if (cls >= C) break;  // uniform in the wave
    const uint64_t bits = __ballot(ty[lane * AP_PITCH + cc] != 0u);  // rows >= N hold 0
    if (row < N) keys[cls * N + row] = tk[lane * AP_PITCH + cc];
    if (lane == 0) mask[cls * W + blockIdx.x] = bits;
  }
}

__global__ __launch_bounds__(AP_THREADS) void ap_count_kernel(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ mask, int64_t N,
                                                              int64_t W, double* __restrict__ partial, int* __restrict__ npos) {
  __shared__ __align__(16) uint32_t sk[AP_CHUNK];
  __shared__ __align__(16) uint32_t sp[AP_CHUNK];
  __shared__ int wtot[4];
  __shared__ int sel[AP_TILE];
  __shared__ int red[4][AP_TILE][2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t c = blockIdx.x;
  const uint32_t* __restrict__ K = keys + c * N;
  const uint64_t* __restrict__ M = mask + c * W;

  // thread t owns the words [w0, w1) of the class's target bits; base = the number of positives in front of them
  const int64_t wpt = (W + AP_THREADS - 1) / AP_THREADS;
  const int64_t w0 = std::min<int64_t>(W, tid * wpt), w1 = std::min<int64_t>(W, w0 + wpt);
  int mine = 0;
  for (int64_t w = w0; w < w1; ++w) mine += __popcll(M[w]);
  int inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int v = __shfl_up(inc, o);
    if (lane >= o) inc += v;
  }
  if (lane == 63) wtot[wave] = inc;
  __syncthreads();
  int base = inc - mine;
  for (int w = 0; w < wave; ++w) base += wtot[w];
  const int P = wtot[0] + wtot[1] + wtot[2] + wtot[3];
  if (blockIdx.y == 0 && tid == 0) npos[c] = P;

  for (int64_t g = blockIdx.y; g * AP_TILE < P; g += gridDim.y) {
    const int r0 = (int)(g * AP_TILE), r1 = std::min(P, r0 + AP_TILE);
    if (base < r1 && base + mine > r0) {
      int rank = base;
      for (int64_t w = w0; w < w1 && rank < r1; ++w) {
        uint64_t bits = M[w];
        const int n = __popcll(bits);
        if (rank + n <= r0) {
          rank += n;
          continue;
        }
        while (bits) {
          const int b = __builtin_ctzll(bits);
          bits &= bits - 1;
          if (rank >= r0 && rank < r1) sel[rank - r0] = (int)(w * AP_TILE + b);
          ++rank;
        }
      }
    }
    __syncthreads();
    const bool valid = lane < r1 - r0;
    const uint32_t ki = valid ? K[sel[lane]] : 0xffffffffu;
    int cnt = 0, tp = 0;
    for (int64_t j0 = 0; j0 < N; j0 += AP_CHUNK) {
      if (j0) __syncthreads();  // the previous chunk's reads are done
      for (int r = tid; r < AP_CHUNK; r += AP_THREADS) {
        const int64_t j = j0 + r;  // the 64 lanes of a wave share one word of target bits
        const bool in = j < N;
        const uint32_t k = in ? K[j] : 0u;
        const bool y = in && ((M[j >> 6] >> (j & 63)) & 1ull);
        sk[r] = k;
        sp[r] = y ? k : 0u;
      }
      __syncthreads();
      const int q0 = wave * (AP_CHUNK / 4);
      const int q1 = (int)std::min<int64_t>(q0 + AP_CHUNK / 4, (N - j0 + 3) & ~int64_t(3));  // the tail is padded with 0 up to the chunk
      for (int q = q0; q < q1; q += 4) {
        const u32x4 a = *reinterpret_cast<const u32x4*>(sk + q);
        const u32x4 b = *reinterpret_cast<const u32x4*>(sp + q);
        cnt += (int)(a.x >= ki) + (int)(a.y >= ki) + (int)(a.z >= ki) + (int)(a.w >= ki);
        tp += (int)(b.x >= ki) + (int)(b.y >= ki) + (int)(b.z >= ki) + (int)(b.w >= ki);
      }
    }
    red[wave][lane][0] = cnt;
    red[wave][lane][1] = tp;
    __syncthreads();
    if (wave == 0) {
      const int CNT = red[0][lane][0] + red[1][lane][0] + red[2][lane][0] + red[3][lane][0];
      const int TP = red[0][lane][1] + red[1][lane][1] + red[2][lane][1] + red[3][lane][1];
      double term = valid ? (double)TP / (double)CNT : 0.0;  // CNT >= 1: a positive counts itself
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o);
      if (lane == 0) partial[c * W + g] = term;
    }
    __syncthreads();  // sel, red and the staging buffers are free again
  }
}

__global__ __launch_bounds__(AP_THREADS) void ap_finish_kernel(const double* __restrict__ partial, const int* __restrict__ npos, int64_t C,
                                                               int64_t W, double* __restrict__ ap) {
  const int64_t c = (int64_t)blockIdx.x * AP_THREADS + threadIdx.x;
  if (c >= C) return;
  const int P = npos[c];
  const int groups = (P + AP_TILE - 1) / AP_TILE;
  double s = 0.0;
  for (int g = 0; g < groups; ++g) s += partial[c * W + g];
  ap[c] = P ? s / (double)P : 0.0;
}

int64_t ap_words(int64_t N) { return (N + AP_TILE - 1) / AP_TILE; }

}  // namespace

extern "C" int64_t op_average_precision_workspace_bytes(int64_t N, int64_t C) {
  if (N <= 0 || C <= 0) return 0;
  return 4 * N * C + 16 * C * ap_words(N);
}

extern "C" int op_average_precision(const float* scores, int64_t ld_scores, const uint8_t* targets, int64_t ld_targets, int64_t N, int64_t C,
                                    double* ap, int* npos, void* workspace, int64_t workspace_bytes, void* stream) {
  OP_CHECK_ARG(N >= 1 && N < (int64_t(1) << 31), "op_average_precision: N = %lld, need 1 <= N < 2^31", (long long)N);
  OP_CHECK_ARG(C >= 1 && C <= AP_MAX_C, "op_average_precision: C = %lld, need 1 <= C <= %lld", (long long)C, (long long)AP_MAX_C);
  OP_CHECK_ARG(ld_scores >= C && ld_targets >= C, "op_average_precision: ld_scores = %lld, ld_targets = %lld, need >= C = %lld",
               (long long)ld_scores, (long long)ld_targets, (long long)C);
  OP_CHECK_ARG(scores && targets && ap && npos && ((uintptr_t)scores & 3) == 0 && ((uintptr_t)ap & 7) == 0 && ((uintptr_t)npos & 3) == 0,
               "op_average_precision: scores, targets, ap, npos must be non-null and aligned to their element size");
  const int64_t W = ap_words(N), need = 4 * N * C + 16 * C * W;
  OP_CHECK_ARG(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0,
               "op_average_precision: N = %lld, C = %lld need %lld workspace bytes (16-aligned), got %lld", (long long)N, (long long)C,
               (long long)need, (long long)workspace_bytes);
  double* partial = (double*)workspace;               // [C][W]
  uint64_t* mask = (uint64_t*)(partial + C * W);      // [C][W]
  uint32_t* keys = (uint32_t*)(mask + C * W);         // [C][N]
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ap_prepare_kernel, dim3((unsigned)W, (unsigned)((C + AP_TILE - 1) / AP_TILE)), dim3(AP_THREADS), 0, st, scores, ld_scores,
                     targets, ld_targets, N, C, W, keys, mask);
  OP_LAUNCH_CHECK();
  const int64_t gy = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(W, 65535), (AP_TARGET_GROUPS + C - 1) / C));
  hipLaunchKernelGGL(ap_count_kernel, dim3((unsigned)C, (unsigned)gy), dim3(AP_THREADS), 0, st, (const uint32_t*)keys, (const uint64_t*)mask, N, W,
                     partial, npos);
  OP_LAUNCH_CHECK();
  hipLaunchKernelGGL(ap_finish_kernel, dim3((unsigned)((C + AP_THREADS - 1) / AP_THREADS)), dim3(AP_THREADS), 0, st, (const double*)partial,
                     (const int*)npos, C, W, ap);
  OP_LAUNCH_CHECK();
  return OP_OK;
}
