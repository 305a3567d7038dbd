// Fine-tuning losses (include/onepeace_hip.h: op_row_loss, op_box_loss): the loss, the logged counter and the gradient of one criterion
// in one pass over the logits, instead of the reference's chain of small torch launches (fp32 log-softmax, gather or multiply, sum,
// exp, argmax, compare, and their backward twins).
//
// row_loss_kernel: one workgroup of 256 lanes per row of logits [B, C] (bf16 or fp32, row stride ld).  The row is read from memory once,
//   with 16-byte vector loads from the first 16-byte boundary of the row on (the up to 7 elements in front of it and the tail behind the
//   last whole vector go one element per lane, so an odd C or a column slice of a wider matrix takes the same code), converted to fp32
//   and staged in LDS; the soft / multi-label target row is staged beside it.  Elements past RL_CAP columns do not fit the stage and are
//   read again from the caches in the later passes.  Pass 0 (the load) finds the row maximum and the arg-max (lowest index on a tie; a
//   NaN ranks above everything, as in torch), pass 1 the sums of the mode, pass 2 writes gscale * d loss / d logits.  Every sum is a lane's
//   strided partial, a shuffle butterfly over the wave and the four waves in order: no floating-point atomics, the same bits every run.
//     hard  (classify_loss.py:62-64)  F.cross_entropy(label_smoothing = eps, reduction = 'sum'), int64 targets, -100 = ignore_index
//     soft  (classify_loss.py:56-60)  sum_c -t_c logp_c, counter sum_c p_c t_c
//     multi (classify_loss.py:51-54)  F.binary_cross_entropy_with_logits(reduction = 'sum'), counter t[argmax]
//     hinge (hinge_loss.py:49-53)     sum_k max(0, margin + x_k - x_target), counter (argmax == target)
//   With m the row maximum, S = sum_c exp(x_c - m): log-probabilities are -(log S + (m - x_c)), a sum of two non-negative terms;
//   S is kept as 1 + S1, S1 the sum without the arg-max column, so that log S and 1 - p_argmax stay precise on a saturated row.
// sum_rows_kernel: one workgroup adds row_loss and row_correct over the rows in a fixed order.
// box_loss_kernel (refcoco_loss.py:36-46): one workgroup; o = sigmoid(logits), sum |o - t| / B + the mean over the valid rows
//   (o_x1 < o_x2 and o_y1 < o_y2) of 1 - GIoU(o_i, t_i) -- only the diagonal of torchvision's generalized_box_iou is ever formed.  The
//   valid rows are counted first; the second phase recomputes each row and writes the gradient through the sigmoid.
#include "common.h"

#include <math.h>

namespace {

constexpr int RL_THREADS = 256;
constexpr int RL_CAP = 4096;  // columns of a row staged in LDS (fp32): 16 KiB for the logits, 16 KiB for a float target row
constexpr int64_t RL_IGNORE = -100;

enum { RL_HARD = 0, RL_SOFT = 1, RL_MULTI = 2, RL_HINGE = 3 };

// K sums over the workgroup: the wave butterfly, then the four waves in order.  red: 4 * K floats, free again on return.
template <int K> __device__ __forceinline__ void block_sum(float (&v)[K], float* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = wave_sum(v[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) red[wave * K + k] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) v[k] = ((red[k] + red[K + k]) + red[2 * K + k]) + red[3 * K + k];
  __syncthreads();
}

// (a, ia) ranks before (b, ib): the greater value, a NaN above every number, the lower index among equals
__device__ __forceinline__ bool rl_before(float a, int ia, float b, int ib) {
  const bool an = __builtin_isnan(a), bn = __builtin_isnan(b);
  if (an || bn) return an && (!bn || ia < ib);
  return a > b || (a == b && ia < ib);
}

template <typename T> struct RlVec;
template <> struct RlVec<bf16_t> { static constexpr int N = 8; };
template <> struct RlVec<float> { static constexpr int N = 4; };

template <typename T> __device__ __forceinline__ void rl_load_vec(const T* p, float (&v)[RlVec<T>::N]);
template <> __device__ __forceinline__ void rl_load_vec<bf16_t>(const bf16_t* p, float (&v)[8]) { Vec8<bf16_t>::load(p, v); }
template <> __device__ __forceinline__ void rl_load_vec<float>(const float* p, float (&v)[4]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = a[i];
}

// Read row[0 .. C) once: `visit(c, value)` for every element, the first RL_CAP of them copied to dst as fp32.
template <typename T, typename F> __device__ __forceinline__ void rl_stage(const T* __restrict__ row, int C, float* dst, F visit) {
  constexpr int V = RlVec<T>::N;
  const int tid = threadIdx.x;
  const int misfit = (int)(((uintptr_t)row & 15) / sizeof(T));   // row is aligned to sizeof(T)
  const int head = min(C, misfit ? (int)(16 / sizeof(T)) - misfit : 0);
  const int nvec = (C - head) / V;
  if (tid < head) {
    const float x = (float)row[tid];
    if (tid < RL_CAP) dst[tid] = x;
    visit(tid, x);
  }
  for (int i = tid; i < nvec; i += RL_THREADS) {
    const int c0 = head + i * V;
    float v[V];
    rl_load_vec<T>(row + c0, v);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if (c0 + j < RL_CAP) dst[c0 + j] = v[j];
      visit(c0 + j, v[j]);
    }
  }
  const int c = head + nvec * V + tid;
  if (c < C) {
    const float x = (float)row[c];
    if (c < RL_CAP) dst[c] = x;
    visit(c, x);
  }
}

template <typename T> __device__ __forceinline__ float rl_get(const float* staged, const T* __restrict__ row, int c) {
  return c < RL_CAP ? staged[c] : (float)row[c];
}

template <typename T, typename TT>
__global__ __launch_bounds__(RL_THREADS) void row_loss_kernel(const T* __restrict__ logits, int64_t ld, const void* __restrict__ targets_,
                                                              int64_t ldt, int C, int mode, float eps, float margin, float gscale,
                                                              float* __restrict__ row_loss, float* __restrict__ row_correct,
                                                              float* __restrict__ dlogits) {
  __shared__ __align__(16) float sx[RL_CAP];
  __shared__ __align__(16) float st[RL_CAP];
  __shared__ float red[4 * 4];
  __shared__ float bestv[4];
  __shared__ int besti[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t r = blockIdx.x;
  const T* __restrict__ x = logits + r * ld;
  const bool dense = mode == RL_SOFT || mode == RL_MULTI;  // a float target row; else one int64 class index
  const TT* __restrict__ t = dense ? (const TT*)targets_ + r * ldt : nullptr;
  float* __restrict__ dx = dlogits ? dlogits + r * (int64_t)C : nullptr;

  // pass 0: the one read of the row; maximum and arg-max
  float bv = 0.f;
  int bi = 0x7fffffff;  // "nothing yet": any element ranks before it
  rl_stage<T>(x, C, sx, [&](int c, float v) {
    if (bi == 0x7fffffff || rl_before(v, c, bv, bi)) {
      bv = v;
      bi = c;
    }
  });
  if (dense) rl_stage<TT>(t, C, st, [](int, float) {});
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(bv, o);
    const int oi = __shfl_xor(bi, o);
    if (oi != 0x7fffffff && (bi == 0x7fffffff || rl_before(ov, oi, bv, bi))) {
      bv = ov;
      bi = oi;
    }
  }
  if (lane == 0) {
    bestv[wave] = bv;
    besti[wave] = bi;
  }
  __syncthreads();  // also: sx and st are complete
  bv = bestv[0];
  bi = besti[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    if (besti[w] != 0x7fffffff && rl_before(bestv[w], besti[w], bv, bi)) {
      bv = bestv[w];
      bi = besti[w];
    }
  }
  const float m = bv;      // C >= 1: wave 0 always holds an element
  const int amax = bi;

  int64_t tgt = 0;
  bool ignore = false, bad = false;
  if (!dense) {
    tgt = ((const int64_t*)targets_)[r];
    ignore = mode == RL_HARD && tgt == RL_IGNORE;
    bad = !ignore && (tgt < 0 || tgt >= C);
  }
  if (ignore || bad) {  // uniform over the workgroup; nothing is read at the target
    if (tid == 0) {
      row_loss[r] = bad ? __builtin_nanf("") : 0.f;
      row_correct[r] = 0.f;
    }
    if (dx)
      for (int c = tid; c < C; c += RL_THREADS) dx[c] = 0.f;
    return;
  }

  // S = 1 + S1 with S1 the sum over every column but the arg-max (whose exponential is exactly 1): log S = log1p(S1) and
  // 1 - p_argmax = S1 / S keep their relative precision when the row saturates (S1 << 1), where S itself rounds at 2^-24.
  if (mode == RL_HARD) {
    float a[2] = {0.f, 0.f};  // S1, sum (m - x_c)
    for (int c = tid; c < C; c += RL_THREADS) {
      const float d = m - rl_get(sx, x, c);
      a[0] += c == amax ? 0.f : expf(-d);
      a[1] += d;
    }
    block_sum<2>(a, red);
    const float S1 = a[0], S = 1.f + S1, logS = log1pf(S1);
    const float xt = rl_get(sx, x, (int)tgt);
    if (tid == 0) {
      float loss = logS + (1.f - eps) * (m - xt);
      if (eps > 0.f) loss += (eps / (float)C) * a[1];
      row_loss[r] = loss;
      row_correct[r] = amax == (int)tgt ? 1.f : 0.f;
    }
    if (dx) {
      const float u = eps / (float)C;
      for (int c = tid; c < C; c += RL_THREADS) {
        float g;
        if (c == amax) g = c == (int)tgt ? eps - S1 / S : 1.f / S;
        else {
          const float p = expf(rl_get(sx, x, c) - m) / S;
          g = c == (int)tgt ? p - (1.f - eps) : p;
        }
        dx[c] = gscale * (g - u);
      }
    }
  } else if (mode == RL_SOFT) {
    float a[4] = {0.f, 0.f, 0.f, 0.f};  // S1, sum t, sum t (m - x), sum t e
    for (int c = tid; c < C; c += RL_THREADS) {
      const float d = m - rl_get(sx, x, c), tc = rl_get(st, t, c);
      const float e = expf(-d);
      a[0] += c == amax ? 0.f : e;
      a[1] += tc;
      a[2] += tc * d;
      a[3] += tc * e;
    }
    block_sum<4>(a, red);
    const float S = 1.f + a[0], tsum = a[1];
    if (tid == 0) {
      row_loss[r] = tsum * log1pf(a[0]) + a[2];
      row_correct[r] = a[3] / S;
    }
    if (dx)
      for (int c = tid; c < C; c += RL_THREADS) dx[c] = gscale * ((expf(rl_get(sx, x, c) - m) / S) * tsum - rl_get(st, t, c));
  } else if (mode == RL_MULTI) {
    float a[1] = {0.f};
    for (int c = tid; c < C; c += RL_THREADS) {
      const float xc = rl_get(sx, x, c), tc = rl_get(st, t, c);
      const float e = expf(-fabsf(xc));
      a[0] += (fmaxf(xc, 0.f) - xc * tc) + log1pf(e);
      if (dx) dx[c] = gscale * ((xc >= 0.f ? 1.f / (1.f + e) : e / (1.f + e)) - tc);
    }
    block_sum<1>(a, red);
    if (tid == 0) {
      row_loss[r] = a[0];
      row_correct[r] = rl_get(st, t, amax);
    }
  } else {  // RL_HINGE
    const float xt = rl_get(sx, x, (int)tgt);
    float a[2] = {0.f, 0.f};  // loss, sum of the subgradients
    for (int c = tid; c < C; c += RL_THREADS) {
      const float h = (margin + rl_get(sx, x, c)) - xt;
      a[0] += h > 0.f ? h : (__builtin_isnan(h) ? h : 0.f);
      a[1] += h > 0.f ? 1.f : (h == 0.f ? 0.5f : 0.f);
    }
    block_sum<2>(a, red);
    if (tid == 0) {
      row_loss[r] = a[0];
      row_correct[r] = amax == (int)tgt ? 1.f : 0.f;
    }
    if (dx)
      for (int c = tid; c < C; c += RL_THREADS) {
        const float h = (margin + rl_get(sx, x, c)) - xt;
        const float g = h > 0.f ? 1.f : (h == 0.f ? 0.5f : 0.f);
        dx[c] = gscale * (c == (int)tgt ? g - a[1] : g);
      }
  }
}

__global__ __launch_bounds__(RL_THREADS) void sum_rows_kernel(const float* __restrict__ row_loss, const float* __restrict__ row_correct,
                                                              int64_t B, float* __restrict__ sums) {
  __shared__ float red[4 * 2];
  float a[2] = {0.f, 0.f};
  for (int64_t r = threadIdx.x; r < B; r += RL_THREADS) {
    a[0] += row_loss[r];
    a[1] += row_correct[r];
  }
  block_sum<2>(a, red);
  if (threadIdx.x == 0) {
    sums[0] = a[0];
    sums[1] = a[1];
  }
}

// ---- boxes ----------------------------------------------------------------------------------------------------------------------
// torch's subgradients: max(a, b) and min(a, b) give 1/2 to each side of a tie, clamp(min = 0) passes the gradient at 0
__device__ __forceinline__ float g_max(float a, float b) { return a > b ? 1.f : (a == b ? 0.5f : 0.f); }  // d max(a, b) / d a
__device__ __forceinline__ float g_min(float a, float b) { return a < b ? 1.f : (a == b ? 0.5f : 0.f); }  // d min(a, b) / d a

struct BoxRow {
  float o[4];
  float l1;      // sum_j |o_j - t_j|
  float sgn[4];  // sign(o_j - t_j), sign(0) = 0
  bool valid;
  float li;      // 1 - GIoU
  float dli[4];  // d li / d o_j
};

template <typename T> __device__ __forceinline__ void box_load(const T* p, float (&v)[4]);
template <> __device__ __forceinline__ void box_load<float>(const float* p, float (&v)[4]) { rl_load_vec<float>(p, v); }
template <> __device__ __forceinline__ void box_load<bf16_t>(const bf16_t* p, float (&v)[4]) {
  const bf16x4 a = *reinterpret_cast<const bf16x4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) v[i] = (float)a[i];
}

template <typename T> __device__ __forceinline__ BoxRow box_row(const T* __restrict__ logits, const float* __restrict__ targets, int64_t r) {
  BoxRow R;
  float x[4], t[4];
  box_load<T>(logits + 4 * r, x);
  box_load<float>(targets + 4 * r, t);
  R.l1 = 0.f;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float e = expf(-fabsf(x[j]));
    R.o[j] = x[j] >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    const float d = R.o[j] - t[j];
    R.l1 += fabsf(d);
    R.sgn[j] = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
  }
  const float* o = R.o;
  R.valid = o[0] < o[2] && o[1] < o[3];
  // torchvision.ops.generalized_box_iou(o, t), entry (i, i)
  const float w1 = o[2] - o[0], h1 = o[3] - o[1];
  const float area1 = w1 * h1, area2 = (t[2] - t[0]) * (t[3] - t[1]);
  const float iw0 = fminf(o[2], t[2]) - fmaxf(o[0], t[0]), ih0 = fminf(o[3], t[3]) - fmaxf(o[1], t[1]);
  const float iw = fmaxf(iw0, 0.f), ih = fmaxf(ih0, 0.f);
  const float inter = iw * ih, uni = (area1 + area2) - inter, iou = inter / uni;
  const float ew0 = fmaxf(o[2], t[2]) - fminf(o[0], t[0]), eh0 = fmaxf(o[3], t[3]) - fminf(o[1], t[1]);
  const float ew = fmaxf(ew0, 0.f), eh = fmaxf(eh0, 0.f);
  const float enc = ew * eh;
  R.li = 1.f - (iou - (enc - uni) / enc);
  // li = 2 - inter / uni - uni / enc
  const float cw = iw0 >= 0.f ? 1.f : 0.f, ch = ih0 >= 0.f ? 1.f : 0.f, cew = ew0 >= 0.f ? 1.f : 0.f, ceh = eh0 >= 0.f ? 1.f : 0.f;
  const float darea[4] = {-h1, -w1, h1, w1};
  const float dinter[4] = {-ih * cw * g_max(o[0], t[0]), -iw * ch * g_max(o[1], t[1]), ih * cw * g_min(o[2], t[2]), iw * ch * g_min(o[3], t[3])};
  const float denc[4] = {-eh * cew * g_min(o[0], t[0]), -ew * ceh * g_min(o[1], t[1]), eh * cew * g_max(o[2], t[2]), ew * ceh * g_max(o[3], t[3])};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float duni = darea[j] - dinter[j];
    const float diou = (dinter[j] * uni - inter * duni) / (uni * uni);
    const float drat = (duni * enc - uni * denc[j]) / (enc * enc);
    R.dli[j] = -diou - drat;
  }
  return R;
}

template <typename T>
__global__ __launch_bounds__(RL_THREADS) void box_loss_kernel(const T* __restrict__ logits, const float* __restrict__ targets, int64_t B,
                                                              float gscale, float* __restrict__ out, float* __restrict__ dlogits) {
  __shared__ float red[4 * 3];
  float a[3] = {0.f, 0.f, 0.f};  // sum |o - t|, sum over the valid rows of 1 - GIoU, the valid rows (integers below 2^24 per lane: exact)
  for (int64_t r = threadIdx.x; r < B; r += RL_THREADS) {
    const BoxRow R = box_row<T>(logits, targets, r);
    a[0] += R.l1;
    if (R.valid) {
      a[1] += R.li;
      a[2] += 1.f;
    }
  }
  block_sum<3>(a, red);
  const float nv = a[2], fb = (float)B;
  if (threadIdx.x == 0) {
    out[0] = a[0] / fb + (nv > 0.f ? a[1] / nv : __builtin_nanf(""));  // the mean of an empty tensor is NaN
    out[1] = nv;
  }
  if (!dlogits) return;
  for (int64_t r = threadIdx.x; r < B; r += RL_THREADS) {
    const BoxRow R = box_row<T>(logits, targets, r);
    f32x4 g;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float dl = R.sgn[j] / fb + (R.valid ? R.dli[j] / nv : 0.f);
      g[j] = gscale * (dl * (R.o[j] * (1.f - R.o[j])));
    }
    *reinterpret_cast<f32x4*>(dlogits + 4 * r) = g;
  }
}

}  // namespace

extern "C" int op_row_loss(const void* logits, int dtype, int64_t ld, const void* targets, int target_dtype, int64_t ld_targets, int64_t B,
                           int64_t C, int mode, float label_smoothing, float margin, float gscale, float* row_loss, float* row_correct,
                           float* dlogits, float* sums, void* stream) {
  OP_CHECK_ARG(mode >= RL_HARD && mode <= RL_HINGE, "op_row_loss: mode = %d, need 0 (hard), 1 (soft), 2 (multi-label) or 3 (hinge)", mode);
  OP_CHECK_ARG(dtype == OP_DT_BF16 || dtype == OP_DT_F32, "op_row_loss: dtype = %d, need 0 (bf16) or 1 (fp32)", dtype);
  const bool dense = mode == RL_SOFT || mode == RL_MULTI;
  OP_CHECK_ARG(!dense || target_dtype == OP_DT_BF16 || target_dtype == OP_DT_F32,
               "op_row_loss: target_dtype = %d, need 0 (bf16) or 1 (fp32) for [B, C] targets", target_dtype);
  OP_CHECK_ARG(B >= 0 && B < (int64_t(1) << 31), "op_row_loss: B = %lld, need 0 <= B < 2^31", (long long)B);
  OP_CHECK_ARG(C >= 1 && C < (int64_t(1) << 31) - 8, "op_row_loss: C = %lld, need 1 <= C < 2^31 - 8", (long long)C);
  OP_CHECK_ARG(ld >= C, "op_row_loss: ld = %lld, need >= C = %lld", (long long)ld, (long long)C);
  OP_CHECK_ARG(!dense || ld_targets >= C, "op_row_loss: ld_targets = %lld, need >= C = %lld", (long long)ld_targets, (long long)C);
  OP_CHECK_ARG(label_smoothing >= 0.f && label_smoothing < 1.f, "op_row_loss: label_smoothing = %g, need 0 <= label_smoothing < 1",
               (double)label_smoothing);
  OP_CHECK_ARG(logits && targets && row_loss && row_correct, "op_row_loss: logits, targets, row_loss and row_correct must be non-null");
  const uintptr_t xal = dtype == OP_DT_BF16 ? 1 : 3, tal = !dense ? 7 : (target_dtype == OP_DT_BF16 ? 1 : 3);
  OP_CHECK_ARG(((uintptr_t)logits & xal) == 0 && ((uintptr_t)targets & tal) == 0 && ((uintptr_t)row_loss & 3) == 0 &&
                   ((uintptr_t)row_correct & 3) == 0 && ((uintptr_t)dlogits & 3) == 0 && ((uintptr_t)sums & 3) == 0,
               "op_row_loss: every pointer must be aligned to its element size");
  if (B == 0) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)B), block(RL_THREADS);
  const int rc = op_with_bool(dtype == OP_DT_BF16, [&](auto xb) {
    return op_with_bool(dense && target_dtype == OP_DT_BF16, [&](auto tb) {
      typedef op_elem_t<decltype(xb)::value> T;
      hipLaunchKernelGGL((row_loss_kernel<T, op_elem_t<decltype(tb)::value>>), grid, block, 0, st, (const T*)logits, ld, targets, ld_targets,
                         (int)C, mode, label_smoothing, margin, gscale, row_loss, row_correct, dlogits);
      OP_LAUNCH_CHECK();
      return OP_OK;
    });
  });
  if (rc != OP_OK) return rc;
  if (sums) {
    hipLaunchKernelGGL(sum_rows_kernel, dim3(1), block, 0, st, (const float*)row_loss, (const float*)row_correct, B, sums);
    OP_LAUNCH_CHECK();
  }
  return OP_OK;
}

extern "C" int op_box_loss(const void* logits, int dtype, const float* targets, int64_t B, float gscale, float* out, float* dlogits,
                           void* stream) {
  OP_CHECK_ARG(dtype == OP_DT_BF16 || dtype == OP_DT_F32, "op_box_loss: dtype = %d, need 0 (bf16) or 1 (fp32)", dtype);
  OP_CHECK_ARG(B >= 0 && B < (int64_t(1) << 24), "op_box_loss: B = %lld, need 0 <= B < 2^24", (long long)B);
  OP_CHECK_ARG(logits && targets && out, "op_box_loss: logits, targets and out must be non-null");
  OP_CHECK_ARG(((uintptr_t)logits & (dtype == OP_DT_BF16 ? 7 : 15)) == 0 && ((uintptr_t)targets & 15) == 0 && ((uintptr_t)out & 3) == 0 &&
                   ((uintptr_t)dlogits & 15) == 0,
               "op_box_loss: logits, targets and dlogits must be aligned to a row of four elements, out to 4 bytes");
  if (B == 0) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == OP_DT_BF16)
    hipLaunchKernelGGL(box_loss_kernel<bf16_t>, dim3(1), dim3(RL_THREADS), 0, st, (const bf16_t*)logits, targets, B, gscale, out, dlogits);
  else
    hipLaunchKernelGGL(box_loss_kernel<float>, dim3(1), dim3(RL_THREADS), 0, st, (const float*)logits, targets, B, gscale, out, dlogits);
  OP_LAUNCH_CHECK();
  return OP_OK;
}
