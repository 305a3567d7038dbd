// HBM-bound helper kernels of the ONE-PEACE hot path (gfx950): transposes, column reductions, GeGLU backward,
// layer-scale/drop-path residual backward, L2-normalise, InfoNCE rows, AdamW, relative-position bias tables.
// All move 16-byte vectors per lane, accumulate in fp32 and are deterministic (two-stage reductions, no
// floating-point atomics except the relative-position table scatter which is documented below).
#include "common.h"
#include <string.h>

namespace {

constexpr int CS_MAX_PARTS = 256;

// ------------------------------------------------------------------------------------------------------------
// bf16 2-D transpose  out[c][r] = in[r][c]   (64x64 tiles through LDS, 8-byte global accesses on both sides)
// ------------------------------------------------------------------------------------------------------------
// scale (nullable): out[c][r] = bf16(scale[r] * in[r][c]) -- the dgrad copy of a residual branch's last Linear with the layer scale
// folded in (ops._transposed(..., scale=gamma): dx = (rowscale * dout) . (gamma o W), transformer_layer.py:70-88)
__device__ __forceinline__ void transpose_tile(int bx, int by, const bf16_t* __restrict__ in, bf16_t* __restrict__ out,
                                                        int rows, int cols, int64_t ld_in, int64_t ld_out,
                                                        const bf16_t* __restrict__ scale = nullptr) {
  __shared__ bf16_t tile[64][64 + 2];
  const int r0 = by * 64, c0 = bx * 64;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;  // 16 x 16 threads, 4 elements each along the fast axis
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + ty + k * 16, c = c0 + tx * 4;
    if (r < rows) {
      const float sc = scale ? (float)scale[r] : 1.f;
      if (c + 3 < cols && (ld_in & 3) == 0) {
        bf16x4 v = *reinterpret_cast<const bf16x4*>(in + (int64_t)r * ld_in + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) tile[ty + k * 16][tx * 4 + j] = scale ? (bf16_t)(sc * (float)v[j]) : v[j];
      } else {
        for (int j = 0; j < 4; ++j)
          if (c + j < cols) tile[ty + k * 16][tx * 4 + j] = scale ? (bf16_t)(sc * (float)in[(int64_t)r * ld_in + c + j]) : in[(int64_t)r * ld_in + c + j];
      }
    }
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + ty + k * 16, r = r0 + tx * 4;  // output row = input column
    if (c < cols) {
      if (r + 3 < rows && (ld_out & 3) == 0) {
        bf16x4 v;
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = tile[tx * 4 + j][ty + k * 16];
        *reinterpret_cast<bf16x4*>(out + (int64_t)c * ld_out + r) = v;
      } else {
        for (int j = 0; j < 4; ++j)
          if (r + j < rows) out[(int64_t)c * ld_out + r + j] = tile[tx * 4 + j][ty + k * 16];
      }
    }
  }
}


__global__ __launch_bounds__(256) void transpose_kernel(const bf16_t* __restrict__ in, bf16_t* __restrict__ out, int rows, int cols,
                                                        int64_t ld_in, int64_t ld_out, const bf16_t* __restrict__ scale) {
  transpose_tile(blockIdx.x, blockIdx.y, in, out, rows, cols, ld_in, ld_out, scale);
}

// Many transposes in ONE launch (the dgrad copies of all weights after an optimiser step: 520 matrices at 4B).  Descriptor i
// covers tiles [tile0[i], tile0[i+1]) of the launch; a workgroup finds its matrix by binary search.
struct TransposeDesc { const bf16_t* in; bf16_t* out; int rows, cols; int64_t ld_in, ld_out; int tile0, tiles_x; const bf16_t* scale; };
__global__ __launch_bounds__(256) void transpose_batched_kernel(const TransposeDesc* __restrict__ table, int n) {
  const int b = blockIdx.x;
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (table[mid].tile0 <= b) lo = mid; else hi = mid - 1;
  }
  const TransposeDesc d = table[lo];
  const int local = b - d.tile0;
  transpose_tile(local % d.tiles_x, local / d.tiles_x, d.in, d.out, d.rows, d.cols, d.ld_in, d.ld_out, d.scale);
}

// ------------------------------------------------------------------------------------------------------------
// column sums:  part[p][n] = sum over this block's rows of  rs[m] * x[m][n] * (y ? y[m][n] : 1)
// grid = (ceil(N / 512), parts); block 256 = 4 waves x 64 lanes x 8 columns
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void colsum_partial_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ y,
                                                             const float* __restrict__ rowscale, int rps,
                                                             float* __restrict__ part, int64_t M, int N, int64_t ld) {
  __shared__ float red[4][512];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = blockIdx.x * 512 + lane * 8;
  float a[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if (c < N) {
    const int64_t m0 = (int64_t)blockIdx.y * 4 + wid, step = (int64_t)gridDim.y * 4;
    if (!y && !rowscale) {
      // plain column sums (the q / v bias gradients: 2 x 225 MB per layer): FOUR rows in flight per wave -- one load -> add per
      // trip left the kernel at 4.0 TB/s (round 3); the rows are added in the same order as before
      int64_t m = m0;
      for (; m + 3 * step < M; m += 4 * step) {
        typename Vec8<bf16_t>::raw_t r0 = Vec8<bf16_t>::ldraw(x + m * ld + c), r1 = Vec8<bf16_t>::ldraw(x + (m + step) * ld + c),
                                     r2 = Vec8<bf16_t>::ldraw(x + (m + 2 * step) * ld + c), r3 = Vec8<bf16_t>::ldraw(x + (m + 3 * step) * ld + c);
        float v0[8], v1[8], v2[8], v3[8];
        Vec8<bf16_t>::cvt(r0, v0);
        Vec8<bf16_t>::cvt(r1, v1);
        Vec8<bf16_t>::cvt(r2, v2);
        Vec8<bf16_t>::cvt(r3, v3);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = (((a[j] + v0[j]) + v1[j]) + v2[j]) + v3[j];
      }
      for (; m < M; m += step) {
        float xv[8];
        Vec8<bf16_t>::load(x + m * ld + c, xv);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] += xv[j];
      }
    } else {
      for (int64_t m = m0; m < M; m += step) {
        float xv[8];
        Vec8<bf16_t>::load(x + m * ld + c, xv);
        float s = rowscale ? rowscale[m / rps] : 1.f;
        if (y) {
          float yv[8];
          Vec8<bf16_t>::load(y + m * ld + c, yv);
#pragma unroll
          for (int j = 0; j < 8; ++j) a[j] += s * xv[j] * yv[j];
        } else {
#pragma unroll
          for (int j = 0; j < 8; ++j) a[j] += s * xv[j];
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) red[wid][lane * 8 + j] = a[j];
  __syncthreads();
  for (int i = threadIdx.x; i < 512; i += 256) {
    const int cc = blockIdx.x * 512 + i;
    if (cc < N) part[(int64_t)blockIdx.y * N + cc] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
  }
}

// Layer-scale gradient from the weight gradient's side product (op_gemm_tn_grouped: rowdot) instead of from the branch output.
// grid = ceil(N / 64) blocks of 4 waves: wave w folds slots w, w + 4, ... of its 64 columns (four loads in flight per lane: one thread
// per column walking up to 144 slots one dependent load at a time took 36 us per launch), the four partial sums meet in LDS in a fixed order.
__global__ __launch_bounds__(256) void gamma_grad_finish_kernel(const float* __restrict__ rowdot, int slots,
                                                                const bf16_t* __restrict__ b0, const float* __restrict__ g00,
                                                                const bf16_t* __restrict__ b1, const float* __restrict__ g01,
                                                                const bf16_t* __restrict__ b2, const float* __restrict__ g02,
                                                                bf16_t* __restrict__ dgamma, int N, int accumulate) {
  __shared__ float part[4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int n = blockIdx.x * 64 + lane;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
  if (n < N) {
    int s = w;
    for (; s + 12 < slots; s += 16) {
      a0 += rowdot[(int64_t)s * N + n];
      a1 += rowdot[(int64_t)(s + 4) * N + n];
      a2 += rowdot[(int64_t)(s + 8) * N + n];
      a3 += rowdot[(int64_t)(s + 12) * N + n];
    }
    for (; s < slots; s += 4) a0 += rowdot[(int64_t)s * N + n];
  }
  part[w][lane] = (a0 + a1) + (a2 + a3);
  __syncthreads();
  if (w != 0 || n >= N) return;
  float t = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);  // the UNSCALED gradient's side product: exact for any gamma, also 0
  if (g00) t += (b0 ? (float)b0[n] : 0.f) * g00[n];
  if (g01) t += (b1 ? (float)b1[n] : 0.f) * g01[n];
  if (g02) t += (b2 ? (float)b2[n] : 0.f) * g02[n];
  dgamma[n] = (bf16_t)(t + (accumulate ? (float)dgamma[n] : 0.f));
}

// ------------------------------------------------------------------------------------------------------------
// residual-branch backward in one pass (transformer_layer.py:70-88):  out = resid + rs[m] * gamma[n] * y[m][n]
//   dbranch[m][n] = rs[m] * gamma[n] * dout[m][n]
//   part[0][p][n] = sum_rows rs * dout * y        (-> dgamma)
//   part[1][p][n] = sum_rows rs * dout            (-> dbias of the branch's last Linear, times gamma in the fold)
// grid = (ceil(N / 512), parts); block 256 = 4 waves x 64 lanes x 8 columns; two rows in flight per wave.
// SKIP (rs given): the multiplier of a row is read a trip BEFORE the row; where it is 0 nothing of dout / y is loaded, dbranch gets +0 and
// the partial sums get nothing -- the dense kernel multiplies that row by the exact zero.  (A wave walks one row and the loop holds
// no barrier.)
// ------------------------------------------------------------------------------------------------------------
template <bool SKIP>
__global__ __launch_bounds__(256) void resid_bwd_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ y,
                                                        const bf16_t* __restrict__ gamma, const float* __restrict__ rowscale,
                                                        int rps, bf16_t* __restrict__ dbranch, float* __restrict__ part,
                                                        int64_t M, int N, const int* __restrict__ rows) {
  // rows (nullable, ABI 9): row m of dout is row rows[m] of a LARGER matrix (< 0: no row -- reads as zeros); dbranch / y stay packed
  __shared__ float red[4][512];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int c = blockIdx.x * 512 + lane * 8;
  float ag[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ab[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float gv[8] = {1, 1, 1, 1, 1, 1, 1, 1};
  if (c < N) {
    if (gamma) Vec8<bf16_t>::load(gamma + c, gv);
    const int64_t step = (int64_t)gridDim.y * 4;
    const int64_t mfirst = (int64_t)blockIdx.y * 4 + wid;
    // (table entries of the NEXT trip are requested before this trip's rows are used: in one trip, entry -> row is an L2 latency per trip)
    int64_t e0 = (rows && mfirst < M) ? rows[mfirst] : mfirst, e1 = (rows && mfirst + step < M) ? rows[mfirst + step] : mfirst + step;
    float n0 = 1.f, n1 = 1.f;  // SKIP: the multipliers of the next trip's two rows, requested a trip ahead like the table entries
    if constexpr (SKIP) {
      if (mfirst < M) n0 = rowscale[mfirst / rps];
      if (mfirst + step < M) n1 = rowscale[(mfirst + step) / rps];
    }
    for (int64_t m = mfirst; m < M; m += 2 * step) {
      const int64_t m2 = m + step;
      const bool two = m2 < M;
      const int64_t s0 = e0, s1 = two ? e1 : -1;
      const int64_t mn = m + 2 * step;
      if (rows) {
        if (mn < M) e0 = rows[mn];
        if (mn + step < M) e1 = rows[mn + step];
      } else {
        e0 = mn;
        e1 = mn + step;
      }
      const bf16x8 zero8 = {(bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f, (bf16_t)0.f};
      const float sc0 = n0, sc1 = n1;
      if constexpr (SKIP) {
        if (mn < M) n0 = rowscale[mn / rps];
        if (mn + step < M) n1 = rowscale[(mn + step) / rps];
      }
      const bool live0 = !SKIP || sc0 != 0.f, live1 = two && (!SKIP || sc1 != 0.f);
      bf16x8 d0 = (s0 >= 0 && live0) ? Vec8<bf16_t>::ldraw(dout + s0 * N + c) : zero8, d1, y0, y1;
      if (y && live0) y0 = Vec8<bf16_t>::ldraw(y + m * N + c);
      if (live1) {
        d1 = s1 >= 0 ? Vec8<bf16_t>::ldraw(dout + s1 * N + c) : zero8;
        if (y) y1 = Vec8<bf16_t>::ldraw(y + m2 * N + c);
      }
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (h == 1 && !two) break;
        const int64_t mm = h == 0 ? m : m2;
        if (SKIP && !(h == 0 ? live0 : live1)) {
          *reinterpret_cast<bf16x8*>(dbranch + mm * N + c) = zero8;
          continue;
        }
        float d[8], o[8];
        Vec8<bf16_t>::cvt(h == 0 ? d0 : d1, d);
        const float sc = SKIP ? (h == 0 ? sc0 : sc1) : (rowscale ? rowscale[mm / rps] : 1.f);
        if (y) {
          float yv[8];
          Vec8<bf16_t>::cvt(h == 0 ? y0 : y1, yv);
#pragma unroll
          for (int j = 0; j < 8; ++j) ag[j] += sc * d[j] * yv[j];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float t = sc * d[j];
          ab[j] += t;
          o[j] = t * gv[j];
        }
        Vec8<bf16_t>::store(dbranch + mm * N + c, o);
      }
    }
  }
  if (part == nullptr) return;  // uniform
#pragma unroll
  for (int pass = 0; pass < 2; ++pass) {
    if (pass == 0 && y == nullptr) continue;  // uniform
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 8; ++j) red[wid][lane * 8 + j] = pass == 0 ? ag[j] : ab[j];
    __syncthreads();
    float* dst = part + ((int64_t)pass * gridDim.y + blockIdx.y) * N;
    for (int i = threadIdx.x; i < 512; i += 256) {
      const int cc = blockIdx.x * 512 + i;
      if (cc < N) dst[cc] = red[0][i] + red[1][i] + red[2][i] + red[3][i];
    }
  }
}

// ------------------------------------------------------------------------------------------------------------
// GeGLU backward (transformer_layer.py:64-67):  g = gelu(h0) * h1
//   dh0 = dg * h1 * gelu'(h0),  dh1 = dg * gelu(h0)
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void geglu_bwd_kernel(const bf16_t* __restrict__ dg, const bf16_t* __restrict__ h0,
                                                        const bf16_t* __restrict__ h1, bf16_t* __restrict__ dh0,
                                                        bf16_t* __restrict__ dh1, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    float g[8], a[8], b[8], o0[8], o1[8];
    Vec8<bf16_t>::load(dg + i * 8, g);
    Vec8<bf16_t>::load(h0 + i * 8, a);
    Vec8<bf16_t>::load(h1 + i * 8, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float cdf, pdf;
      gelu_parts(a[j], cdf, pdf);
      o0[j] = g[j] * b[j] * (cdf + a[j] * pdf);
      o1[j] = g[j] * a[j] * cdf;
    }
    Vec8<bf16_t>::store(dh0 + i * 8, o0);
    Vec8<bf16_t>::store(dh1 + i * 8, o1);
  }
}

// ------------------------------------------------------------------------------------------------------------
// residual/layer-scale backward (transformer_layer.py:70-88):  out = resid + rs[m] * gamma[n] * y[m][n]
//   dy[m][n] = rs[m] * gamma[n] * dout[m][n]   (written to dbranch)
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void scale_rows_kernel(const bf16_t* __restrict__ dout, const bf16_t* __restrict__ gamma,
                                                         const float* __restrict__ rowscale, int rps,
                                                         bf16_t* __restrict__ dbranch, int64_t M, int N) {
  const int n8 = N / 8;
  const int64_t total = M * n8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t m = i / n8;
    const int c = (int)(i - m * n8) * 8;
    float d[8], gv[8];
    Vec8<bf16_t>::load(dout + m * N + c, d);
    const float s = rowscale ? rowscale[m / rps] : 1.f;
    if (gamma) {
      Vec8<bf16_t>::load(gamma + c, gv);
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] *= s * gv[j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] *= s;
    }
    Vec8<bf16_t>::store(dbranch + m * N + c, d);
  }
}

// ------------------------------------------------------------------------------------------------------------
// F.normalize(x, dim=1) (one_peace_retrieval.py:112): y = x / max(||x||, eps); one wave per row
// ------------------------------------------------------------------------------------------------------------
template <typename TO>
__global__ __launch_bounds__(256) void l2norm_fwd_kernel(const bf16_t* __restrict__ x, TO* __restrict__ y,
                                                         float* __restrict__ inv_norm, int rows, int cols, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float ss = 0.f;
  for (int c = lane * 8; c < cols; c += 512) {
    float v[8];
    Vec8<bf16_t>::load(x + (int64_t)row * cols + c, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) ss += v[j] * v[j];
  }
  ss = wave_sum(ss);
  const float nrm = sqrtf(ss);
  const float inv = 1.f / fmaxf(nrm, eps);
  for (int c = lane * 8; c < cols; c += 512) {
    float v[8];
    Vec8<bf16_t>::load(x + (int64_t)row * cols + c, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] *= inv;
    Vec8<TO>::store(y + (int64_t)row * cols + c, v);
  }
  if (lane == 0 && inv_norm) inv_norm[row] = nrm < eps ? -inv : inv;  // negative: the eps clamp was taken
}

// dx = inv * (dy - y * <y, dy>) while ||x|| >= eps.  Below eps the denominator is the constant eps (clamp_min passes no
// gradient), so dx = dy / eps: the forward marks such rows with a negative inv_norm and the projection term is dropped.
template <typename TY>
__global__ __launch_bounds__(256) void l2norm_bwd_kernel(const TY* __restrict__ dy, const TY* __restrict__ y,
                                                         const float* __restrict__ inv_norm, bf16_t* __restrict__ dx,
                                                         int rows, int cols) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float dot = 0.f;
  for (int c = lane * 8; c < cols; c += 512) {
    float a[8], b[8];
    Vec8<TY>::load(dy + (int64_t)row * cols + c, a);
    Vec8<TY>::load(y + (int64_t)row * cols + c, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) dot += a[j] * b[j];
  }
  dot = wave_sum(dot);
  float inv = inv_norm[row];
  if (inv < 0.f) {  // clamped row
    inv = -inv;
    dot = 0.f;
  }
  for (int c = lane * 8; c < cols; c += 512) {
    float a[8], b[8];
    Vec8<TY>::load(dy + (int64_t)row * cols + c, a);
    Vec8<TY>::load(y + (int64_t)row * cols + c, b);
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = inv * (a[j] - b[j] * dot);
    Vec8<bf16_t>::store(dx + (int64_t)row * cols + c, a);
  }
}

// ------------------------------------------------------------------------------------------------------------
// InfoNCE rows (image_text_pretrain_loss.py:164-185 + adjust_label_smoothed_nll_loss :17-27).
// One workgroup per row of sim [rows][n] (fp32).  Writes the row loss, the argmax hit, <dsim, sim> (for the
// logit-scale gradient) and overwrites sim with d(loss_row)/d(sim) * gscale.
//   loss_row = -(1-eps-e)*lp[t] - e*sum_j lp[j],  e = eps/(n-1),  lp = sim - lse
//   d/ds_k   = p_k*((1-eps-e) + n*e) - (1-eps-e)*[k==t] - e
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float block_sum_256(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(256) void infonce_rows_kernel(float* __restrict__ sim, int n, int64_t ld, int target0,
                                                           float eps_ls, float gscale, float* __restrict__ row_loss,
                                                           float* __restrict__ row_hit, float* __restrict__ row_dot,
                                                           int write_grad) {
  __shared__ float red[4];
  __shared__ float redv[4];
  __shared__ int redi[4];
  const int row = blockIdx.x;
  float* s = sim + (int64_t)row * ld;
  const int tgt = target0 + row;
  float mx = -INFINITY;
  int amax = 0x7fffffff;
  float sum = 0.f;
  for (int k = threadIdx.x; k < n; k += 256) {
    const float v = s[k];
    sum += v;
    if (v > mx) { mx = v; amax = k; }  // first maximum within this thread's increasing k
  }
  // block arg-max (ties -> smallest index, as torch.argmax on CPU returns the first maximal element)
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o);
    const int oi = __shfl_xor(amax, o);
    if (om > mx || (om == mx && oi < amax)) { mx = om; amax = oi; }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { redv[threadIdx.x >> 6] = mx; redi[threadIdx.x >> 6] = amax; }
  __syncthreads();
  mx = redv[0]; amax = redi[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (redv[w] > mx || (redv[w] == mx && redi[w] < amax)) { mx = redv[w]; amax = redi[w]; }
  const float ssum = block_sum_256(sum, red);
  float ex = 0.f;
  for (int k = threadIdx.x; k < n; k += 256) ex += __expf(s[k] - mx);
  const float lse = mx + logf(block_sum_256(ex, red));
  const float e = (eps_ls != 0.f) ? eps_ls / (float)(n - 1) : 0.f;
  const float wt = 1.f - eps_ls - e;
  const float st = s[tgt];
  const float loss = -wt * (st - lse) - e * (ssum - (float)n * lse);
  float dot = 0.f;
  if (write_grad) {
    const float pk_coef = wt + (float)n * e;
    __syncthreads();
    for (int k = threadIdx.x; k < n; k += 256) {
      const float v = s[k];
      float d = __expf(v - lse) * pk_coef - e - (k == tgt ? wt : 0.f);
      d *= gscale;
      dot += d * v;
      s[k] = d;
    }
    dot = block_sum_256(dot, red);
  }
  if (threadIdx.x == 0) {
    row_loss[row] = loss;
    row_hit[row] = (amax == tgt) ? 1.f : 0.f;
    row_dot[row] = dot;
  }
}

// ------------------------------------------------------------------------------------------------------------
// Exponential moving average of the weights in fp32 (the reference's EMAModule with ema_fp32: true; the rule is the one of
// fairseq/modules/ema_module.py:101-127: ema.mul_(decay); ema.add_(param.to(ema.dtype), alpha=1 - decay)):
//   e' = fmaf(take, p, fl32(keep * e))       keep = float(decay), take = float(1 - decay), p the bf16 parameter as stored
// which is bit for bit what torch computes for the two lines on a CPU.  The product and the fma are written out and contraction is
// switched off around them, so no compiler setting turns the two roundings into another pair.  keep = 0, take = 1 gives e' = p.
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float ema_rule(float e, float p, float keep, float take) {
#pragma clang fp contract(off)
  return __builtin_fmaf(take, p, __fmul_rn(keep, e));
}

// The stand-alone pass.  Algorithmic bytes: 10 B/param (e r+w 8, p r 2).
__global__ __launch_bounds__(256) void ema_step_kernel(float* __restrict__ e, const bf16_t* __restrict__ p, int64_t n8, float keep,
                                                       float take) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    float ev[8], pv[8];
    Vec8<float>::load(e + i * 8, ev);
    Vec8<bf16_t>::load(p + i * 8, pv);
#pragma unroll
    for (int j = 0; j < 8; ++j) ev[j] = ema_rule(ev[j], pv[j], keep, take);
    Vec8<float>::store(e + i * 8, ev);
  }
}

// ------------------------------------------------------------------------------------------------------------
// AdamW as the reference does it (one_peace/optim/adam.py:186-253): fp32 math on bf16 params, decoupled decay applied to the
// parameter before the Adam update, eps added to sqrt(v).  ONE kernel template states the update; three switches select what is read
// and written around it, so p, master, m and v cannot depend on them.  What a switch leaves unused arrives as null or 0, never read.
//   GROUPS  the flat buffer is partitioned into parameter groups (trainer.py:265-278, utils/layer_decay.py:34-77:
//           "layer_<id>_<decay|no_decay>" groups with their own lr_scale and weight decay; optim/base_optimizer.py:8-14 sets
//           lr_g = lr * lr_scale_g): group g owns the 8-element vectors [end8[g-1], end8[g]).  ONE launch for all groups: the group
//           of a vector is found by binary search in a table staged in LDS (<= 256 groups), and re-used while consecutive vectors
//           stay in it; step_size and decay_mul are formed per group in fp32 on the device.  Without GROUPS both arrive as scalars
//           that the host formed (op_adamw_step), and there is no table and no search.
//   MASTER  an fp32 master copy of the parameters (the reference's `bf16: true` without `memory_efficient_bf16`:
//           trainer.py:297-307 -> optim/fp16_optimizer.py: Adam runs on fp32_params, _sync_fp32_params_to_fp16 casts them back).
//           The master takes the place of float(p): it is read, updated and stored in fp32, and p receives the round-to-nearest-even
//           bf16 of the value just stored.  p is never read, so an update below half a bf16 spacing accumulates in the master
//           instead of being rounded away every step.
//   EMA     the EMA pass folded in: one more fp32 stream e, and after the update ema_rule with the value the bf16 store of p
//           rounds to -- also with a master: the reference's EMA reads the model, never the optimiser's fp32 copy.
// first8 (runtime): the kernel may run over a RANGE of the flat buffer (op_adamw_step_shard: the optimiser state sharded over the
// data-parallel ranks).  Every pointer then arrives at the range's first vector and is indexed from 0; first8, the global index of
// that vector, is added to the loop index for the group lookup alone, so the table stays the global one and an element's update
// does not depend on where the range starts.  The whole-buffer entries pass 0.
// Algorithmic bytes per parameter: 22 plain or with GROUPS alone (p r+w 4, g r 2, m and v r+w 16); 28 with MASTER (master r+w 8,
// g r 2, m and v r+w 16, p w 2); with EMA 30 without the master (22 + e r+w 8) and 36 with it (28 + 8).
// Non-finite gradients with clipping on: a NaN anywhere in the gradient buffer makes the norm NaN, the clip coefficient NaN
// (fminf would have returned 1 and stepped every other parameter with the unclipped gradient) and with it EVERY parameter and
// moment of the step, as optim.TorchAdamW's clamp does, and with every parameter every element of e; an infinite norm gives
// coefficient 0, and only the infinite elements turn NaN.  The reference raises before its optimiser step instead
// (trainer.py:830-837): the norm is what a loop checks.
// ------------------------------------------------------------------------------------------------------------
// grad_scale times the reference's clip coefficient (fairseq/utils.py:393-397: clamp(max_norm / (norm + 1e-6), max=1), norm =
// |grad_scale| sqrt(sqnorm)).  torch's clamp, not fminf: a NaN coefficient stays NaN.  Formed in fp64 and rounded ONCE: every
// gradient is multiplied by this number and v by its square, so the four fp32 roundings of sqrtf, the sum, the quotient and the
// product reached v doubled (measured: 1.19 x the bound tests/adamw_ref.py derives for v).  A handful of fp64 operations per thread.
__device__ __forceinline__ float clipped_grad_scale(float grad_scale, const float* __restrict__ sqnorm, float clip_norm) {
  if (sqnorm == nullptr || !(clip_norm > 0.f)) return grad_scale;
  const double norm = fabs((double)grad_scale) * sqrt((double)*sqnorm);
  const double c = (double)clip_norm / (norm + 1e-6);
  return (c < 1.0 || c != c) ? (float)((double)grad_scale * c) : grad_scale;
}

constexpr int ADAM_MAX_GROUPS = 256;
template <bool GROUPS, bool MASTER, bool EMA>
__global__ __launch_bounds__(256) void adamw_kernel(bf16_t* __restrict__ p, float* __restrict__ master,
                                                    const bf16_t* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                    float* __restrict__ e, int64_t n8, const int64_t* __restrict__ end8,
                                                    const float* __restrict__ lr_scale, const float* __restrict__ wd,
                                                    int n_groups, float lr, float bias_corr, float step_size, float decay_mul,
                                                    float beta1, float beta2, float eps, float grad_scale,
                                                    const float* __restrict__ sqnorm, float clip_norm, float keep, float take,
                                                    int64_t first8) {
  __shared__ int64_t s_end[ADAM_MAX_GROUPS];  // unused, and not allocated, without GROUPS
  __shared__ float s_step[ADAM_MAX_GROUPS], s_decay[ADAM_MAX_GROUPS];
  if constexpr (GROUPS) {
    for (int i = threadIdx.x; i < n_groups; i += 256) {
      const float lr_g = lr * lr_scale[i];
      s_end[i] = end8[i];
      s_step[i] = lr_g * bias_corr;          // lr_g * sqrt(1 - beta2^t) / (1 - beta1^t)
      s_decay[i] = 1.f - wd[i] * lr_g;       // p <- p - wd * lr_g * p, before the Adam update (adam.py:243-246)
    }
    __syncthreads();
  }
  grad_scale = clipped_grad_scale(grad_scale, sqnorm, clip_norm);
  int grp = 0;
  int64_t lo = 0, hi = GROUPS ? s_end[0] : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    if constexpr (GROUPS) {
      const int64_t gi = i + first8;  // the vector's place in the whole flat buffer: what the table speaks of
      if (gi < lo || gi >= hi) {  // first group whose end is > gi
        int a = 0, b = n_groups - 1;
        while (a < b) {
          const int mid = (a + b) >> 1;
          if (s_end[mid] > gi) b = mid; else a = mid + 1;
        }
        grp = a;
        lo = grp ? s_end[grp - 1] : 0;
        hi = s_end[grp];
      }
      step_size = s_step[grp], decay_mul = s_decay[grp];
    }
    float pv[8], gv[8], mv[8], vv[8], ev[8];
    if constexpr (MASTER) Vec8<float>::load(master + i * 8, pv);
    else Vec8<bf16_t>::load(p + i * 8, pv);
    Vec8<bf16_t>::load(g + i * 8, gv);
    Vec8<float>::load(m + i * 8, mv);
    Vec8<float>::load(v + i * 8, vv);
    if constexpr (EMA) Vec8<float>::load(e + i * 8, ev);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float gr = gv[j] * grad_scale;
      mv[j] = mv[j] * beta1 + (1.f - beta1) * gr;
      vv[j] = vv[j] * beta2 + (1.f - beta2) * gr * gr;
      const float denom = sqrtf(vv[j]) + eps;
      pv[j] = pv[j] * decay_mul - step_size * (mv[j] / denom);
      if constexpr (EMA) ev[j] = ema_rule(ev[j], (float)(bf16_t)pv[j], keep, take);  // the value the store below rounds to
    }
    if constexpr (MASTER) Vec8<float>::store(master + i * 8, pv);
    Vec8<bf16_t>::store(p + i * 8, pv);  // with MASTER: bf16(master'), round to nearest even: the reference's _sync_fp32_params_to_fp16
    Vec8<float>::store(m + i * 8, mv);
    Vec8<float>::store(v + i * 8, vv);
    if constexpr (EMA) Vec8<float>::store(e + i * 8, ev);
  }
}

// sum of squares, stage 1: one partial per workgroup (grid-stride over 8-element vectors); stage 2 folds the partials
__global__ __launch_bounds__(256) void sqnorm_partial_kernel(const bf16_t* __restrict__ x, int64_t n8, float* __restrict__ part) {
  __shared__ float red[4];
  float a = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    float v[8];
    Vec8<bf16_t>::load(x + i * 8, v);
#pragma unroll
    for (int j = 0; j < 8; ++j) a += v[j] * v[j];
  }
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}
__global__ __launch_bounds__(256) void sqnorm_final_kernel(const float* __restrict__ part, int n, float* __restrict__ out) {
  __shared__ float red[4];
  float a = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) a += part[i];
  a = wave_sum(a);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = red[0] + red[1] + red[2] + red[3];
}

// ------------------------------------------------------------------------------------------------------------
// Relative-position bias (adapter/image.py:164-171, text.py:76-83, audio.py:117-124):
// bias[h][i][j] = table[bucket[i][j]][h].  The reference expands this to [B, heads, S, S] per forward; here it
// is built ONCE per table as [heads][S][Spad] bf16 and shared by every sample (attention reads it from L2).
// Columns j >= S are zero-filled (the attention kernels mask them by index).
// ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void relpos_build_kernel(const bf16_t* __restrict__ table, const int* __restrict__ bucket,
                                                           int64_t bucket_ld, bf16_t* __restrict__ out, int heads, int S,
                                                           int Spad, int transposed) {
  const int64_t total = (int64_t)S * Spad;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int i = (int)(idx / Spad), j = (int)(idx - (int64_t)i * Spad);
    if (j < S) {
      const int b = transposed ? bucket[(int64_t)j * bucket_ld + i] : bucket[(int64_t)i * bucket_ld + j];
      for (int h = 0; h < heads; ++h) out[((int64_t)h * S + i) * Spad + j] = table[(int64_t)b * heads + h];
    } else {
      for (int h = 0; h < heads; ++h) out[((int64_t)h * S + i) * Spad + j] = (bf16_t)0.f;
    }
  }
}

// dtable[r][h] = sum over the positions (i, j) with bucket[i][j] == r of dbias[h][i][j], in a fixed order (no atomics: the same bits
// every run).  The caller lists the positions p = i*S + j grouped by bucket (`pos`) and cuts every bucket's list into segments of at
// most a few dozen positions (`seg`: segment t = pos[seg[t] .. seg[t+1])); pass 1 sums each segment per head, pass 2 sums each
// bucket's segments (`bucket_seg`: bucket r = segments bucket_seg[r] .. bucket_seg[r+1]) -- the cross-modal bucket of a joint
// stream holds 10^5 positions, so one thread per bucket would serialise it.
__global__ __launch_bounds__(256) void relpos_seg_sum_kernel(const float* __restrict__ dbias, const int* __restrict__ pos,
                                                             const int* __restrict__ seg, float* __restrict__ partial, int nseg,
                                                             int heads, int S, int Spad) {
  const int64_t total = (int64_t)nseg * heads;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int t = (int)(idx / heads), h = (int)(idx - (int64_t)t * heads);
    const float* d = dbias + (int64_t)h * S * Spad;
    float s = 0.f;
    for (int k = seg[t], e = seg[t + 1]; k < e; ++k) {
      const int p = pos[k], i = p / S;
      s += d[(int64_t)i * Spad + (p - i * S)];
    }
    partial[idx] = s;
  }
}

__global__ __launch_bounds__(256) void relpos_seg_fold_kernel(const float* __restrict__ partial, const int* __restrict__ bucket_seg,
                                                              float* __restrict__ dtable, int num_rel, int heads) {
  const int64_t total = (int64_t)num_rel * heads;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int r = (int)(idx / heads), h = (int)(idx - (int64_t)r * heads);
    float s = 0.f;
    for (int t = bucket_seg[r], e = bucket_seg[r + 1]; t < e; ++t) s += partial[(int64_t)t * heads + h];
    dtable[idx] = s;
  }
}

// Per-sample bias images of the masked-pretraining passes (adapter/image.py:188-204,229-246: the adapters gather a different
// token subset per sample, and with it rows AND columns of the dense [B, heads, S, S] bias): here straight from the table,
//   out[b][h][i][j] = table[bucket[ids[b][i]][ids[b][j]]][h]   (ids = position ids of the K kept tokens of sample b)
// so neither the dense bias nor its gathers are ever materialised.  transposed: out[b][h][j][i] holds that value.
__global__ __launch_bounds__(256) void relpos_build_ids_kernel(const bf16_t* __restrict__ table, const int* __restrict__ bucket,
                                                               int64_t bucket_ld, const int* __restrict__ ids, bf16_t* __restrict__ out,
                                                               int B, int heads, int K, int Kpad, int transposed) {
  const int64_t total = (int64_t)B * K * Kpad;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int j = (int)(idx % Kpad);
    const int64_t bi = idx / Kpad;
    const int i = (int)(bi % K), b = (int)(bi / K);
    bf16_t* o = out + (((int64_t)b * heads) * K + i) * Kpad + j;
    if (j < K) {
      const int pi = ids[(int64_t)b * K + i], pj = ids[(int64_t)b * K + j];
      const int bk = transposed ? bucket[(int64_t)pj * bucket_ld + pi] : bucket[(int64_t)pi * bucket_ld + pj];
      for (int h = 0; h < heads; ++h) o[(int64_t)h * K * Kpad] = table[(int64_t)bk * heads + h];
    } else {
      for (int h = 0; h < heads; ++h) o[(int64_t)h * K * Kpad] = (bf16_t)0.f;
    }
  }
}

// Stage 1 of the table gradient of per-sample images: dense[h][ids[b][i]][ids[b][j]] += dbias[b][h][i][j] -- the per-sample
// slabs are folded into ONE full-sequence image (heads x Sfull x Sfull addresses: little contention), which op_relpos_bias_bwd
// then sums onto the table.  (fp32 atomics: the samples that share a position add in no fixed order.)  (Adding the slabs straight onto the table was 29 ms per call: ten million
// fp32 atomics on a few thousand addresses.)
__global__ __launch_bounds__(256) void relpos_fold_ids_kernel(const float* __restrict__ dbias, const int* __restrict__ ids,
                                                              float* __restrict__ dense, int B, int heads, int K, int Kpad, int Sfull) {
  const int64_t total = (int64_t)B * heads * K * K;
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (int64_t)gridDim.x * 256) {
    const int j = (int)(idx % K);
    int64_t r = idx / K;
    const int i = (int)(r % K);
    r /= K;
    const int h = (int)(r % heads), b = (int)(r / heads);
    const float v = dbias[((((int64_t)b * heads) + h) * K + i) * Kpad + j];
    atomicAdd(&dense[((int64_t)h * Sfull + ids[(int64_t)b * K + i]) * Sfull + ids[(int64_t)b * K + j]], v);
  }
}

inline int ew_grid(int64_t work_items) {
  int64_t b = (work_items + 255) / 256;
  if (b > 2048) b = 2048;
  if (b < 1) b = 1;
  return (int)b;
}

// ------------------------------------------------------------------------------------------------------------
// Stochastic depth without the multiplications by zero (transformer_layer.py:78-88: a dropped sample's branch output is
// multiplied by 0 before it is added to the residual).  The rows of the samples a residual branch KEEPS are packed into a
// smaller matrix, the branch runs on that, and its result is merged back into the full activation matrix:
//   gather:  dst[seg.dst_row0 + j*S + t] = src[seg.src_row0 + kept[j]*S + t]   j < n_kept;  the rest of the segment's dst rows = 0
//            (each segment is padded to a multiple of 64 rows: the weight-gradient kernels want K % 64 == 0, and 0-rows add 0)
//   merge:   out[r] = upd[seg.dst_row0 + inv[sample]*S + t]  if the sample of row r is kept (inv >= 0), else base[r]
// One wave per row, 16-byte vectors; `list` holds the int32 kept[] lists (gather) or inv[] lists (merge) of the segments.
// ------------------------------------------------------------------------------------------------------------
struct RowsSeg { int64_t src_row0, dst_row0; int S, n_kept, dst_rows, n_samples, list_off, pad_; };
struct RowsSegs { int nseg, pad_; RowsSeg seg[4]; };

__global__ __launch_bounds__(256) void rows_gather_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                                          const int* __restrict__ list, const RowsSegs d, int64_t dst_total, int cols) {
  const int lane = threadIdx.x & 63;
  const int n8 = cols / 8;
  for (int64_t rc = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); rc < dst_total; rc += (int64_t)gridDim.x * 4) {
    int64_t from = -1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < d.nseg && rc >= d.seg[i].dst_row0 && rc < d.seg[i].dst_row0 + d.seg[i].dst_rows) {
        const int local = (int)(rc - d.seg[i].dst_row0);
        const int j = local / d.seg[i].S;
        if (j < d.seg[i].n_kept) from = d.seg[i].src_row0 + (int64_t)list[d.seg[i].list_off + j] * d.seg[i].S + (local - j * d.seg[i].S);
      }
    }
    bf16x8* o = reinterpret_cast<bf16x8*>(dst + rc * cols);
    if (from >= 0) {
      const bf16x8* in = reinterpret_cast<const bf16x8*>(src + from * cols);
      for (int c = lane; c < n8; c += 64) o[c] = in[c];
    } else {
      bf16x8 z;
#pragma unroll
      for (int k = 0; k < 8; ++k) z[k] = (bf16_t)0.f;
      for (int c = lane; c < n8; c += 64) o[c] = z;
    }
  }
}

__global__ __launch_bounds__(256) void rows_merge_kernel(const bf16_t* __restrict__ base, const bf16_t* __restrict__ upd,
                                                         bf16_t* __restrict__ out, const int* __restrict__ list, const RowsSegs d,
                                                         int64_t total, int cols) {
  const int lane = threadIdx.x & 63;
  const int n8 = cols / 8;
  for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < total; r += (int64_t)gridDim.x * 4) {
    int64_t from = -1;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (i < d.nseg && r >= d.seg[i].src_row0 && r < d.seg[i].src_row0 + (int64_t)d.seg[i].n_samples * d.seg[i].S) {
        const int local = (int)(r - d.seg[i].src_row0);
        const int smp = local / d.seg[i].S;
        const int j = list[d.seg[i].list_off + smp];
        if (j >= 0) from = d.seg[i].dst_row0 + (int64_t)j * d.seg[i].S + (local - smp * d.seg[i].S);
      }
    }
    if (from < 0 && out == base) continue;  // in place: rows of dropped samples stay what they are
    if (from >= 0 && upd == nullptr) continue;  // (ABI 9) no packed matrix: only the rows of dropped samples are copied
    const bf16x8* in = reinterpret_cast<const bf16x8*>(from >= 0 ? upd + from * cols : base + r * cols);
    bf16x8* o = reinterpret_cast<bf16x8*>(out + r * cols);
    for (int c = lane; c < n8; c += 64) o[c] = in[c];
  }
}

// packed row -> row of the full matrix (-1: a surplus row of a rounded-up segment): what op_rows_gather reads, as a table for the kernels
// that read / write THROUGH it (ABI 9: op_layernorm_*, op_resid_bwd, the residual epilogue of op_gemm_nt)
__global__ __launch_bounds__(256) void rows_map_kernel(int* __restrict__ map, const int* __restrict__ list, const RowsSegs d, int64_t dst_total) {
  const int64_t rc = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (rc >= dst_total) return;
  int64_t from = -1;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i < d.nseg && rc >= d.seg[i].dst_row0 && rc < d.seg[i].dst_row0 + d.seg[i].dst_rows) {
      const int local = (int)(rc - d.seg[i].dst_row0);
      const int j = local / d.seg[i].S;
      if (j < d.seg[i].n_kept) from = d.seg[i].src_row0 + (int64_t)list[d.seg[i].list_off + j] * d.seg[i].S + (local - j * d.seg[i].S);
    }
  }
  map[rc] = (int)from;
}

// Live K-tile lists for the weight gradients of a residual branch whose dropped samples have an all-zero gradient (op_resid_bwd wrote
// ps * dout with ps = 0): problem p covers the rows [row0, row0 + 64 * ntiles) of the row matrix; its list names, in ascending order,
// the 64-row tiles that hold at least one row of a sample with ps != 0.  One workgroup per problem; the flags of 256 tiles at a time
// are compacted in order (ballot + the counts of the waves before).
constexpr int LK_MAX_SEG = 4, LK_MAX_PROB = 8;
struct LiveTilesArgs {
  int nseg;
  struct { const float* ps; int64_t row0; int S, B; } seg[LK_MAX_SEG];  // rows [row0, row0 + S * B); row r belongs to sample (r - row0) / S
  struct { int64_t row0; int ntiles; int* list; int* count; } prob[LK_MAX_PROB];
};

__global__ __launch_bounds__(256) void live_ktiles_kernel(const LiveTilesArgs a) {
  __shared__ int wave_n[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t prow0 = a.prob[blockIdx.x].row0;
  const int ntiles = a.prob[blockIdx.x].ntiles;
  int* __restrict__ list = a.prob[blockIdx.x].list;
  int base = 0;  // (uniform) live tiles before this chunk
  for (int c = 0; c < ntiles; c += 256) {
    const int t = c + tid;
    bool live = false;
    if (t < ntiles) {
      const int64_t r0 = prow0 + (int64_t)t * 64, r1 = r0 + 64;
#pragma unroll
      for (int i = 0; i < LK_MAX_SEG; ++i) {
        if (i >= a.nseg) continue;
        const int64_t lo = r0 > a.seg[i].row0 ? r0 : a.seg[i].row0;
        const int64_t end = a.seg[i].row0 + (int64_t)a.seg[i].S * a.seg[i].B;
        const int64_t hi = r1 < end ? r1 : end;
        if (lo >= hi) continue;
        if (a.seg[i].ps == nullptr) { live = true; continue; }
        const int s0 = (int)((lo - a.seg[i].row0) / a.seg[i].S), s1 = (int)((hi - 1 - a.seg[i].row0) / a.seg[i].S);
        for (int sm = s0; sm <= s1; ++sm) live = live || a.seg[i].ps[sm] != 0.f;
      }
    }
    const unsigned long long m = __ballot(live);
    if (lane == 0) wave_n[wid] = __popcll(m);
    __syncthreads();
    int before = base;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      if (w < wid) before += wave_n[w];
      base += wave_n[w];
    }
    if (live) list[before + __popcll(m & ((1ull << lane) - 1ull))] = t;
    __syncthreads();
  }
  if (tid == 0) *a.prob[blockIdx.x].count = base;
}

// Window lists for the INPUT-gradient GEMMs of such a branch (consumer: op_gemm_nt_grouped_windows), and the zero rows those launches
// no longer write.  A segment is cut into UNITS: wps > 0 -- a unit is a sample, and a kept sample (ps != 0) is listed as wps windows of
// 256 rows from its first row on (odd: they leave out each sample's last row, and the rows S - 1, 2 S - 1, ... of ALL samples are listed
// as strided windows, 256 samples each); wps == 0 -- a unit is an aligned 256-row tile of the segment, listed when one of its rows
// belongs to a kept sample.  A segment feeds up to two lists (the launch of its own rows and a grouped launch, with its problem index there); an
// entry is two words: prob << 28 | (row - base), rows << 16 | row stride.  Grid: x = unit (all segments, then one workgroup per LIST that builds it: ordered ballot
// compaction, segment by segment), y = MW_PIECE-row piece of the unit: the pieces of a unit that is NOT listed write +0 into their rows of
// every output matrix (16-byte stores; the host checks cols % 8 == 0 and ld % 8 == 0) -- or, for an output with a source matrix (the
// residual output of a FORWARD branch: the dense epilogue gives fma(0, y, res) = res there), a copy of the source's rows.
constexpr int MW_MAX_SEG = 4, MW_MAX_OUT = 4, MW_MAX_LIST = 4;
constexpr int MW_PIECE = 16;  // rows a workgroup zero-fills: 64-row pieces left one workgroup per CU busy (1.4 TB/s on the FFN outputs)
struct MWindowsArgs {
  int nseg, nout, nlist, nunits;
  struct { const float* ps; int64_t row0; int S, B, wps, odd, pstride, unit0, units; int list[2], prob[2]; int64_t base[2]; } seg[MW_MAX_SEG];
  struct { bf16_t* ptr; int64_t ld; int cols; const bf16_t* src; int64_t lds; } out[MW_MAX_OUT];  // src (forward, op_live_mwindows_fwd): rows to copy instead of +0
  struct { int* list; int* count; } lists[MW_MAX_LIST];
};

template <class Seg>
__device__ __forceinline__ bool mw_unit_live(const Seg& sg, int u) {
  if (sg.ps == nullptr) return true;
  if (sg.wps > 0) return sg.ps[(int64_t)u * sg.pstride] != 0.f;
  const int64_t lo = (int64_t)u * 256, hi = min(lo + 256, (int64_t)sg.S * sg.B);
  bool live = false;
  for (int sm = (int)(lo / sg.S); sm <= (int)((hi - 1) / sg.S); ++sm) live = live || sg.ps[(int64_t)sm * sg.pstride] != 0.f;
  return live;
}

__global__ __launch_bounds__(256) void live_mwindows_kernel(const MWindowsArgs a) {
  __shared__ int wave_n[4];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  if ((int)blockIdx.x >= a.nunits) {  // ---- list blockIdx.x - nunits ----
    if (blockIdx.y != 0) return;
    {
      const int l = (int)blockIdx.x - a.nunits;
      int base = 0;  // (uniform) entries of list l so far
      for (int i = 0; i < a.nseg; ++i) {
        for (int k = 0; k < 2; ++k) {
          if (a.seg[i].list[k] != l) continue;
          const int per = a.seg[i].wps > 0 ? a.seg[i].wps : 1;
          for (int c = 0; c < a.seg[i].units; c += 256) {
            const int u = c + tid;
            const bool live = u < a.seg[i].units && mw_unit_live(a.seg[i], u);
            const unsigned long long m = __ballot(live);
            if (lane == 0) wave_n[wid] = __popcll(m);
            __syncthreads();
            int before = base;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              if (w < wid) before += wave_n[w] * per;
              base += wave_n[w] * per;
            }
            if (live) {
              const int64_t first = a.seg[i].row0 - a.seg[i].base[k] + (int64_t)u * (a.seg[i].wps > 0 ? a.seg[i].S : 256);
              int* dst = a.lists[l].list + 2 * (before + __popcll(m & ((1ull << lane) - 1ull)) * per);
              for (int w = 0; w < per; ++w) {
                dst[2 * w] = (a.seg[i].prob[k] << 28) | (int)(first + w * 256);
                dst[2 * w + 1] = (256 << 16) | 1;
              }
            }
            __syncthreads();
          }
          if (a.seg[i].odd) {  // the last row of EVERY sample (a dropped one: zeros in, zeros out), 256 samples to a window
            const int nw = (a.seg[i].B + 255) / 256;
            if (tid < nw) {
              int* dst = a.lists[l].list + 2 * (base + tid);
              dst[0] = (a.seg[i].prob[k] << 28) | (int)(a.seg[i].row0 - a.seg[i].base[k] + (int64_t)tid * 256 * a.seg[i].S + a.seg[i].S - 1);
              dst[1] = (min(256, a.seg[i].B - tid * 256) << 16) | a.seg[i].S;
            }
            base += nw;
          }
        }
      }
      if (tid == 0) *a.lists[l].count = base;
    }
    return;
  }
  // ---- zero rows: unit blockIdx.x of segment i, rows [blockIdx.y * MW_PIECE, + MW_PIECE) of it ----
  int i = 0;
#pragma unroll
  for (int j = 1; j < MW_MAX_SEG; ++j)
    if (j < a.nseg && (int)blockIdx.x >= a.seg[j].unit0) i = j;
  const int u = (int)blockIdx.x - a.seg[i].unit0;
  const int64_t seg_rows = (int64_t)a.seg[i].S * a.seg[i].B;
  const int64_t ubeg = (int64_t)u * (a.seg[i].wps > 0 ? a.seg[i].S : 256);
  const int64_t uend = min(ubeg + (a.seg[i].wps > 0 ? a.seg[i].S : 256), seg_rows);
  const int64_t r0 = ubeg + (int64_t)blockIdx.y * MW_PIECE, r1 = min(r0 + MW_PIECE, uend);
  if (r0 >= r1 || mw_unit_live(a.seg[i], u)) return;
  const int nrows = (int)(r1 - r0);
  for (int o = 0; o < a.nout; ++o) {
    const int c8 = a.out[o].cols >> 3;
    bf16_t* base = a.out[o].ptr + (a.seg[i].row0 + r0) * a.out[o].ld;
    const bf16_t* src = a.out[o].src;
    if (src) src += (a.seg[i].row0 + r0) * a.out[o].lds;
    for (int r = wid; r < nrows; r += 4)  // a wave per row: 1 KiB contiguous per store instruction
      for (int c = lane; c < c8; c += 64)
        *reinterpret_cast<uint4*>(base + (int64_t)r * a.out[o].ld + c * 8) =
            src ? *reinterpret_cast<const uint4*>(src + (int64_t)r * a.out[o].lds + c * 8) : make_uint4(0u, 0u, 0u, 0u);
  }
}

}  // namespace

extern "C" {

int op_transpose_scaled(const void* in, void* out, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out, const void* scale,
                        void* stream) {
  OP_CHECK_ARG(in && out && rows >= 0 && cols >= 0, "transpose: bad args");
  if (rows == 0 || cols == 0) return OP_OK;
  dim3 grid(ceil_div(cols, 64), ceil_div(rows, 64));
  hipLaunchKernelGGL(transpose_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)in, (bf16_t*)out, (int)rows,
                     (int)cols, ld_in, ld_out, (const bf16_t*)scale);
  OP_LAUNCH_CHECK();
  return OP_OK;
}
int op_transpose(const void* in, void* out, int64_t rows, int64_t cols, int64_t ld_in, int64_t ld_out, void* stream) {
  return op_transpose_scaled(in, out, rows, cols, ld_in, ld_out, nullptr, stream);
}

// Batched transposes: `table` is a DEVICE array of n descriptors {in, out, rows, cols, ld_in, ld_out, tile0, tiles_x}
// (struct TransposeDesc, 56 bytes: two pointers, two int32, two int64, two int32, one pointer; tile0 = running sum of
// ceil(cols/64)*ceil(rows/64), tiles_x = ceil(cols/64), scale = nullable bf16 [rows] row scales of `in`); total_tiles = the sum over all descriptors.
int op_transpose_batched(const void* table, int64_t n, int64_t total_tiles, void* stream) {
  OP_CHECK_ARG(table && n > 0 && total_tiles > 0, "transpose_batched: bad args");
  hipLaunchKernelGGL(transpose_batched_kernel, dim3((unsigned)total_tiles), dim3(256), 0, (hipStream_t)stream,
                     (const TransposeDesc*)table, (int)n);
  OP_LAUNCH_CHECK();
  return OP_OK;
}
int64_t op_transpose_desc_bytes(void) { return (int64_t)sizeof(TransposeDesc); }

int64_t op_colsum_workspace_bytes(int64_t N) { return (int64_t)CS_MAX_PARTS * N * (int64_t)sizeof(float); }

// out[n] = (accumulate ? out[n] : 0) + mul[n] * sum_m rowscale[m/rps] * x[m][n] * (y ? y[m][n] : 1)
// out_dtype: 0 bf16, 1 f32.  y, rowscale, mul nullable.
int op_colsum(const void* x, const void* y, const float* rowscale, int64_t rows_per_sample, const void* mul, void* out,
              void* workspace, int64_t M, int64_t N, int accumulate, int out_dtype, void* stream) {
  OP_CHECK_ARG(x && out && workspace, "colsum: null pointer");
  OP_CHECK_ARG(N > 0 && N % 8 == 0, "colsum: N must be a multiple of 8");
  hipStream_t s = (hipStream_t)stream;
  int parts = (int)((M + 63) / 64);
  if (parts > CS_MAX_PARTS) parts = CS_MAX_PARTS;
  if (parts < 1) parts = 1;
  dim3 grid(ceil_div(N, 512), parts);
  hipLaunchKernelGGL(colsum_partial_kernel, grid, dim3(256), 0, s, (const bf16_t*)x, (const bf16_t*)y, rowscale,
                     (int)(rows_per_sample > 0 ? rows_per_sample : 1), (float*)workspace, M, (int)N, N);
  OP_LAUNCH_CHECK();
  if (out_dtype == OP_DT_BF16)
    hipLaunchKernelGGL((partials_reduce_kernel<bf16_t>), dim3(ceil_div(N, 32)), dim3(256), 0, s, (const float*)workspace, parts,
                       N, (int)N, (const bf16_t*)mul, (bf16_t*)out, accumulate);
  else
    hipLaunchKernelGGL((partials_reduce_kernel<float>), dim3(ceil_div(N, 32)), dim3(256), 0, s, (const float*)workspace, parts,
                       N, (int)N, (const bf16_t*)mul, (float*)out, accumulate);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

int64_t op_resid_bwd_workspace_bytes(int64_t N) { return 2 * (int64_t)CS_MAX_PARTS * N * (int64_t)sizeof(float); }

// One pass over the gradient of  out = resid + rowscale[m/rps] * gamma[n] * y[m][n]  (transformer_layer.py:70-88,
// y = the branch's last Linear output incl. its bias):
//   dbranch = rowscale * gamma * dout;  dgamma (+)= sum_m rowscale * dout * y;  dbias (+)= sum_m dbranch
// gamma, rowscale, y/dgamma, dbias nullable; dgamma/dbias are bf16 [N]; accumulate: add into them instead of overwriting.
static int resid_bwd_impl(const void* dout, const void* y, const void* gamma, const float* rowscale, int64_t rows_per_sample,
                          void* dbranch, void* dgamma, void* dbias, float* g0, void* workspace, int64_t M, int64_t N, int accumulate,
                          const int* dout_rows, int skip_zero_rows, void* stream) {
  OP_CHECK_ARG(dout && dbranch, "resid_bwd: null pointer");
  OP_CHECK_ARG(N > 0 && N % 8 == 0, "resid_bwd: N must be a multiple of 8");
  OP_CHECK_ARG(!dgamma || y, "resid_bwd: dgamma needs y");
  OP_CHECK_ARG(!(dgamma && g0), "resid_bwd: g0 (dbranch without gamma) and dgamma (from y) are alternatives");
  OP_CHECK_ARG(!(dgamma || dbias || g0) || workspace, "resid_bwd: dgamma/dbias/g0 requested without workspace");
  if (M == 0) {  // the sum over no rows is zero: g0 and the non-accumulating dgamma / dbias are cleared, accumulating ones stay
    if (g0) (void)hipMemsetAsync(g0, 0, (size_t)N * sizeof(float), (hipStream_t)stream);
    if (!accumulate) {
      if (dgamma) (void)hipMemsetAsync(dgamma, 0, (size_t)N * sizeof(bf16_t), (hipStream_t)stream);
      if (dbias) (void)hipMemsetAsync(dbias, 0, (size_t)N * sizeof(bf16_t), (hipStream_t)stream);
    }
    return OP_OK;
  }
  hipStream_t s = (hipStream_t)stream;
  int parts = (int)((M + 63) / 64);
  if (parts > CS_MAX_PARTS) parts = CS_MAX_PARTS;
  if (parts < 1) parts = 1;
  float* ws = (dgamma || dbias || g0) ? (float*)workspace : nullptr;
  // (ABI 8) g0 wanted = the layer-scale gradient comes from the weight gradient: dbranch stays WITHOUT gamma (the weight-gradient and
  // input-gradient GEMMs carry it: op_gemm_tn_grouped's rscale, op_transpose_scaled), dbias still gets it in the fold
  op_with_bool(skip_zero_rows != 0 && rowscale != nullptr, [&](auto skip) {
    hipLaunchKernelGGL(resid_bwd_kernel<decltype(skip)::value>, dim3(ceil_div(N, 512), parts), dim3(256), 0, s, (const bf16_t*)dout,
                       (const bf16_t*)(dgamma ? y : nullptr), (const bf16_t*)(g0 ? nullptr : gamma), rowscale,
                       (int)(rows_per_sample > 0 ? rows_per_sample : 1), (bf16_t*)dbranch, ws, M, (int)N, dout_rows);
    return OP_OK;
  });
  OP_LAUNCH_CHECK();
  if (ws) {
    // job 0: dgamma from sum rs*dout*y; job 1: dbias = gamma * sum rs*dout; job 2 (g0): the same partials without gamma, fp32
    hipLaunchKernelGGL((partials_reduce3_kernel<bf16_t>), dim3(ceil_div(N, 32), g0 ? 3 : 2), dim3(256), 0, s, ws,
                       ws + (int64_t)parts * N, ws + (int64_t)parts * N, (const bf16_t*)nullptr, (const bf16_t*)gamma,
                       (const bf16_t*)nullptr, (bf16_t*)dgamma, (bf16_t*)dbias, (bf16_t*)nullptr, parts, N, (int)N,
                       accumulate, g0);
    OP_LAUNCH_CHECK();
  }
  return OP_OK;
}

int op_resid_bwd(const void* dout, const void* y, const void* gamma, const float* rowscale, int64_t rows_per_sample,
                 void* dbranch, void* dgamma, void* dbias, float* g0, void* workspace, int64_t M, int64_t N, int accumulate,
                 const int* dout_rows, void* stream) {
  return resid_bwd_impl(dout, y, gamma, rowscale, rows_per_sample, dbranch, dgamma, dbias, g0, workspace, M, N, accumulate, dout_rows, 0,
                        stream);
}

// (additive: op_abi_version() stays 10) op_resid_bwd that does not read the rows its multiplier zeroes: where rowscale[m / rps] == 0
// nothing of dout / y is loaded, dbranch gets +0 and the column sums no contribution (op_resid_bwd: +-0 * dout, NaN for a non-finite
// dout).  Every other row and the column sums have op_resid_bwd's bits.  rowscale null: op_resid_bwd.
int op_resid_bwd_skip(const void* dout, const void* y, const void* gamma, const float* rowscale, int64_t rows_per_sample,
                      void* dbranch, void* dgamma, void* dbias, float* g0, void* workspace, int64_t M, int64_t N, int accumulate,
                      const int* dout_rows, void* stream) {
  return resid_bwd_impl(dout, y, gamma, rowscale, rows_per_sample, dbranch, dgamma, dbias, g0, workspace, M, N, accumulate, dout_rows, 1,
                        stream);
}

// dgamma[n] (+)= sum_s rowdot[s][n] + sum_i b_i[n] * g0_i[n]  (see include/onepeace_hip.h)
int op_gamma_grad_finish(const float* rowdot, int64_t slots, const void* b0, const float* g00, const void* b1, const float* g01,
                         const void* b2, const float* g02, void* dgamma, int64_t N, int accumulate, void* stream) {
  OP_CHECK_ARG(rowdot && dgamma && N > 0 && slots > 0, "gamma_grad_finish: null pointer");
  hipLaunchKernelGGL(gamma_grad_finish_kernel, dim3(ceil_div(N, 64)), dim3(256), 0, (hipStream_t)stream, rowdot, (int)slots,
                     (const bf16_t*)b0, g00, (const bf16_t*)b1, g01, (const bf16_t*)b2, g02, (bf16_t*)dgamma, (int)N, accumulate);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// Column sums of x [M, n_seg * seg_cols] (row stride = n_seg * seg_cols) delivered per segment: out_i (bf16 [seg_cols],
// nullable = skip) (+)= sum_m x[m][i * seg_cols + n].  The q/k/v bias gradients of the fused projection
// (multihead_attention.py:57-62: k_proj has no bias -> its slot is null).  n_seg <= 3.
int op_colsum_segments(const void* x, void* out0, void* out1, void* out2, void* workspace, int64_t M, int64_t n_seg,
                       int64_t seg_cols, int accumulate, void* stream) {
  OP_CHECK_ARG(x && workspace, "colsum_segments: null pointer");
  OP_CHECK_ARG(n_seg >= 1 && n_seg <= 3 && seg_cols > 0 && seg_cols % 8 == 0, "colsum_segments: bad segments");
  hipStream_t s = (hipStream_t)stream;
  const int64_t N = n_seg * seg_cols;
  int parts = (int)((M + 63) / 64);
  if (parts > CS_MAX_PARTS) parts = CS_MAX_PARTS;
  if (parts < 1) parts = 1;
  // only the segments that have a consumer are read (k_proj has no bias: a third of the q|k|v gradient stays untouched)
  void* outs[3] = {out0, out1, out2};
  const float* ws = (const float*)workspace;
  for (int i = 0; i < (int)n_seg; ++i) {
    if (outs[i] == nullptr) continue;
    hipLaunchKernelGGL(colsum_partial_kernel, dim3(ceil_div(seg_cols, 512), parts), dim3(256), 0, s,
                       (const bf16_t*)x + i * seg_cols, (const bf16_t*)nullptr, (const float*)nullptr, 1,
                       (float*)workspace + (int64_t)i * parts * seg_cols, M, (int)seg_cols, N);
    OP_LAUNCH_CHECK();
  }
  const int64_t st = (int64_t)parts * seg_cols;
  hipLaunchKernelGGL((partials_reduce3_kernel<bf16_t>), dim3(ceil_div(seg_cols, 32), (int)n_seg), dim3(256), 0, s, ws, ws + st,
                     ws + 2 * st, (const bf16_t*)nullptr, (const bf16_t*)nullptr, (const bf16_t*)nullptr, (bf16_t*)out0,
                     (bf16_t*)out1, (bf16_t*)out2, parts, seg_cols, (int)seg_cols, accumulate);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

int op_geglu_bwd(const void* dg, const void* h0, const void* h1, void* dh0, void* dh1, int64_t numel, void* stream) {
  OP_CHECK_ARG(dg && h0 && h1 && dh0 && dh1, "geglu_bwd: null pointer");
  OP_CHECK_ARG(numel % 8 == 0, "geglu_bwd: numel must be a multiple of 8");
  if (numel == 0) return OP_OK;
  hipLaunchKernelGGL(geglu_bwd_kernel, dim3(ew_grid(numel / 8)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dg,
                     (const bf16_t*)h0, (const bf16_t*)h1, (bf16_t*)dh0, (bf16_t*)dh1, numel / 8);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// dbranch[m][n] = rowscale[m/rps] * gamma[n] * dout[m][n]   (gamma, rowscale nullable)
int op_scale_rows(const void* dout, const void* gamma, const float* rowscale, int64_t rows_per_sample, void* dbranch,
                  int64_t M, int64_t N, void* stream) {
  OP_CHECK_ARG(dout && dbranch, "scale_rows: null pointer");
  OP_CHECK_ARG(N % 8 == 0, "scale_rows: N must be a multiple of 8");
  if (M == 0) return OP_OK;
  hipLaunchKernelGGL(scale_rows_kernel, dim3(ew_grid(M * (N / 8))), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)dout,
                     (const bf16_t*)gamma, rowscale, (int)(rows_per_sample > 0 ? rows_per_sample : 1), (bf16_t*)dbranch, M,
                     (int)N);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// y (out_dtype 0 bf16 / 1 f32) = x / max(||x||_2, eps) per row; inv_norm[rows] saved for the backward, negated where
// ||x||_2 < eps
int op_l2norm_fwd(const void* x, void* y, float* inv_norm, int64_t rows, int64_t cols, float eps, int out_dtype, void* stream) {
  OP_CHECK_ARG(x && y && cols % 8 == 0, "l2norm_fwd: bad args");
  if (rows == 0) return OP_OK;
  if (out_dtype == OP_DT_BF16)
    hipLaunchKernelGGL((l2norm_fwd_kernel<bf16_t>), dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, (bf16_t*)y, inv_norm, (int)rows, (int)cols, eps);
  else
    hipLaunchKernelGGL((l2norm_fwd_kernel<float>), dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)x, (float*)y, inv_norm, (int)rows, (int)cols, eps);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

int op_l2norm_bwd(const void* dy, const void* y, const float* inv_norm, void* dx, int64_t rows, int64_t cols, int y_dtype,
                  void* stream) {
  OP_CHECK_ARG(dy && y && inv_norm && dx && cols % 8 == 0, "l2norm_bwd: bad args");
  if (rows == 0) return OP_OK;
  if (y_dtype == OP_DT_BF16)
    hipLaunchKernelGGL((l2norm_bwd_kernel<bf16_t>), dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)dy, (const bf16_t*)y, inv_norm, (bf16_t*)dx, (int)rows, (int)cols);
  else
    hipLaunchKernelGGL((l2norm_bwd_kernel<float>), dim3(ceil_div(rows, 4)), dim3(256), 0, (hipStream_t)stream,
                       (const float*)dy, (const float*)y, inv_norm, (bf16_t*)dx, (int)rows, (int)cols);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// sim [rows][n] fp32 (ld) is overwritten by gscale * d loss_row / d sim when write_grad != 0.
int op_infonce_rows(float* sim, int64_t rows, int64_t n, int64_t ld, int64_t target0, float label_smoothing, float gscale,
                    float* row_loss, float* row_hit, float* row_dot, int write_grad, void* stream) {
  OP_CHECK_ARG(sim && row_loss && row_hit && row_dot, "infonce_rows: null pointer");
  OP_CHECK_ARG(n >= 2 && target0 >= 0 && target0 + rows <= n, "infonce_rows: targets out of range");
  if (rows == 0) return OP_OK;
  hipLaunchKernelGGL(infonce_rows_kernel, dim3((int)rows), dim3(256), 0, (hipStream_t)stream, sim, (int)n, ld, (int)target0,
                     label_smoothing, gscale, row_loss, row_hit, row_dot, write_grad);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// out[0] = sum of squares of a bf16 vector (fp32, deterministic two-stage fold): the global gradient norm of
// fairseq/utils.py:349-391 over the flat gradient buffer.  workspace: 1024 floats.  numel % 8 == 0.
int op_sqnorm(const void* x, int64_t numel, float* workspace, float* out, void* stream) {
  OP_CHECK_ARG(x && workspace && out && numel % 8 == 0, "sqnorm: bad args");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sqnorm_partial_kernel, dim3(1024), dim3(256), 0, s, (const bf16_t*)x, numel / 8, workspace);
  OP_LAUNCH_CHECK();
  hipLaunchKernelGGL(sqnorm_final_kernel, dim3(1), dim3(256), 0, s, (const float*)workspace, 1024, out);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// What the five op_adamw_step* entries share: the argument checks (messages carry the entry's prefix `who`), the bias correction
// and the launch of adamw_kernel<groups, master != NULL, ema != NULL>.  An entry that requires master or ema checks that itself.
// Without groups step_size and decay_mul are formed here, step_size in fp64 and rounded once; with groups the device forms them.
// numel is the length of what the pointers address and first8 the global index of its first vector (0 but for op_adamw_step_shard).
static int adamw_launch(const char* who, bool groups, void* p, float* master, const void* g, float* m, float* v, float* ema,
                        int64_t numel, int64_t first8, const int64_t* group_end8, const float* group_lr_scale,
                        const float* group_weight_decay, int64_t n_groups, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int64_t step, float grad_scale, const float* grad_sqnorm, float clip_norm, float ema_keep,
                        float ema_take, void* stream) {
  OP_CHECK_ARG(p && g && m && v && (!groups || (group_end8 && group_lr_scale && group_weight_decay)), "%s: null pointer", who);
  OP_CHECK_ARG(numel % 8 == 0 && step >= 1 && (!groups || (n_groups >= 1 && n_groups <= ADAM_MAX_GROUPS)),
               groups ? "%s: numel %% 8 == 0, step >= 1, 1 <= n_groups <= %d required" : "%s: numel must be a multiple of 8 and step >= 1",
               who, ADAM_MAX_GROUPS);
  OP_CHECK_ARG(!master || !ema || ema + numel <= master || master + numel <= ema, "%s: ema overlaps master", who);
  if (numel == 0) return OP_OK;
  const double bc1 = 1.0 - pow((double)beta1, (double)step);
  const double bc2 = 1.0 - pow((double)beta2, (double)step);
  const float bias_corr = groups ? (float)(sqrt(bc2) / bc1) : 0.f;
  const float step_size = groups ? 0.f : (float)((double)lr * sqrt(bc2) / bc1);
  const float decay_mul = groups ? 0.f : 1.f - weight_decay * lr;
  static constexpr decltype(&adamw_kernel<true, false, false>) with_groups[] = {  // [master + 2 ema]; with the plain kernel: all five
      adamw_kernel<true, false, false>, adamw_kernel<true, true, false>, adamw_kernel<true, false, true>, adamw_kernel<true, true, true>};
  hipLaunchKernelGGL((groups ? with_groups[(master != nullptr) + 2 * (ema != nullptr)] : adamw_kernel<false, false, false>),
                     dim3(ew_grid(numel / 8)), dim3(256), 0, (hipStream_t)stream, (bf16_t*)p, master, (const bf16_t*)g, m, v, ema,
                     numel / 8, group_end8, group_lr_scale, group_weight_decay, (int)n_groups, lr, bias_corr, step_size, decay_mul,
                     beta1, beta2, eps, grad_scale, grad_sqnorm, clip_norm, ema_keep, ema_take, first8);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// One AdamW update over a flat bf16 parameter range (numel % 8 == 0).  step >= 1.  The gradient is multiplied by
// grad_scale (1/world after a SUM all-reduce, trainer.py:917-923) and, when grad_sqnorm (device scalar = sum of squares of
// the UNSCALED gradients of ALL ranges, op_sqnorm) and clip_norm > 0 are given, by the reference's clip coefficient
// (trainer.py:929, fairseq/utils.py:393-397) -- computed on the device, no host synchronisation.
int op_adamw_step(void* p, const void* g, float* m, float* v, int64_t numel, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int64_t step, float grad_scale, const float* grad_sqnorm, float clip_norm,
                  void* stream) {
  return adamw_launch("adamw", false, p, nullptr, g, m, v, nullptr, numel, 0, nullptr, nullptr, nullptr, 0, lr, beta1, beta2, eps,
                      weight_decay, step, grad_scale, grad_sqnorm, clip_norm, 0.f, 0.f, stream);
}

// AdamW over a flat buffer partitioned into n_groups (<= 256) contiguous parameter groups in ONE launch: group g covers
// elements [8 * group_end8[g-1], 8 * group_end8[g]) (device table, ascending, last entry = numel / 8) and uses
// lr * group_lr_scale[g] and group_weight_decay[g] (device tables; they are static, the scheduled lr is the scalar argument).
// Same update rule, clip handling and byte traffic as op_adamw_step.
int op_adamw_step_groups(void* p, const void* g, float* m, float* v, int64_t numel, const int64_t* group_end8,
                         const float* group_lr_scale, const float* group_weight_decay, int64_t n_groups, float lr, float beta1,
                         float beta2, float eps, int64_t step, float grad_scale, const float* grad_sqnorm, float clip_norm,
                         void* stream) {
  return adamw_launch("adamw_groups", true, p, nullptr, g, m, v, nullptr, numel, 0, group_end8, group_lr_scale, group_weight_decay,
                      n_groups, lr, beta1, beta2, eps, 0.f, step, grad_scale, grad_sqnorm, clip_norm, 0.f, 0.f, stream);
}

// op_adamw_step_groups with an fp32 master copy (include/onepeace_hip.h): master is read and written, p only written
// (= bf16(master)), 28 B/param.  Same tables, clip handling and argument checks, plus master != NULL.
int op_adamw_step_groups_master(void* p, float* master, const void* g, float* m, float* v, int64_t numel,
                                const int64_t* group_end8, const float* group_lr_scale, const float* group_weight_decay,
                                int64_t n_groups, float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale,
                                const float* grad_sqnorm, float clip_norm, void* stream) {
  OP_CHECK_ARG(master, "adamw_groups_master: null pointer");
  return adamw_launch("adamw_groups_master", true, p, master, g, m, v, nullptr, numel, 0, group_end8, group_lr_scale,
                      group_weight_decay, n_groups, lr, beta1, beta2, eps, 0.f, step, grad_scale, grad_sqnorm, clip_norm, 0.f, 0.f,
                      stream);
}

// One EMA update of a flat fp32 shadow from the flat bf16 parameters (include/onepeace_hip.h): 10 B/param.
int op_ema_step(float* ema, const void* p, int64_t numel, float keep, float take, void* stream) {
  OP_CHECK_ARG(ema && p, "ema_step: null pointer");
  OP_CHECK_ARG(numel % 8 == 0, "ema_step: numel must be a multiple of 8");
  if (numel == 0) return OP_OK;
  hipLaunchKernelGGL(ema_step_kernel, dim3(ew_grid(numel / 8)), dim3(256), 0, (hipStream_t)stream, ema, (const bf16_t*)p, numel / 8,
                     keep, take);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// op_adamw_step_groups (master == NULL) or op_adamw_step_groups_master followed by op_ema_step on the new p, in ONE launch:
// 30 / 36 B/param instead of 22 + 10 / 28 + 10.  Same tables, clip handling and argument checks; ema != NULL and apart from master.
int op_adamw_step_groups_ema(void* p, float* master, const void* g, float* m, float* v, float* ema, int64_t numel,
                             const int64_t* group_end8, const float* group_lr_scale, const float* group_weight_decay,
                             int64_t n_groups, float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale,
                             const float* grad_sqnorm, float clip_norm, float ema_keep, float ema_take, void* stream) {
  OP_CHECK_ARG(ema, "adamw_groups_ema: null pointer");
  return adamw_launch("adamw_groups_ema", true, p, master, g, m, v, ema, numel, 0, group_end8, group_lr_scale, group_weight_decay,
                      n_groups, lr, beta1, beta2, eps, 0.f, step, grad_scale, grad_sqnorm, clip_norm, ema_keep, ema_take, stream);
}

// The grouped step over ONE RANGE of the flat buffers (include/onepeace_hip.h): p and g are the bases of the full buffers, m, v,
// master and ema belong to the range alone.  The same kernel and the same global tables as the whole-buffer entries; only the
// pointers are moved to the range here, and the kernel learns where it starts.  The range checks come before any pointer is moved.
int op_adamw_step_shard(void* p, const void* g, int64_t numel, int64_t first8, int64_t count8, float* m, float* v, float* master,
                        float* ema, const int64_t* group_end8, const float* group_lr_scale, const float* group_weight_decay,
                        int64_t n_groups, float lr, float beta1, float beta2, float eps, int64_t step, float grad_scale,
                        const float* grad_sqnorm, float clip_norm, float ema_keep, float ema_take, void* stream) {
  OP_CHECK_ARG(p && g, "adamw_shard: null pointer");
  OP_CHECK_ARG(numel >= 0 && numel % 8 == 0, "adamw_shard: numel must be a multiple of 8");
  OP_CHECK_ARG(first8 >= 0 && count8 >= 0 && first8 <= numel / 8 && count8 <= numel / 8 - first8,
               "adamw_shard: the range [first8, first8 + count8) must lie inside [0, numel / 8)");
  return adamw_launch("adamw_shard", true, (bf16_t*)p + first8 * 8, master, (const bf16_t*)g + first8 * 8, m, v, ema, count8 * 8,
                      first8, group_end8, group_lr_scale, group_weight_decay, n_groups, lr, beta1, beta2, eps, 0.f, step, grad_scale,
                      grad_sqnorm, clip_norm, ema_keep, ema_take, stream);
}

// transposed != 0 writes out[h][key][query] (the image the dK/dV kernel reads) instead of out[h][query][key]
int op_relpos_bias_build(const void* table, const int* bucket, int64_t bucket_ld, void* out, int64_t heads, int64_t S,
                         int64_t Spad, int transposed, void* stream) {
  OP_CHECK_ARG(table && bucket && out && Spad >= S && Spad % 8 == 0, "relpos_bias_build: bad args");
  hipLaunchKernelGGL(relpos_build_kernel, dim3(ew_grid(S * Spad)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)table,
                     bucket, bucket_ld, (bf16_t*)out, (int)heads, (int)S, (int)Spad, transposed);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// Per-sample images from position ids: out [B][heads][K][Kpad] bf16 (pad columns zero), ids [B][K] int32 (valid positions;
// the caller maps padding to a valid id and masks it through key_pad, as the reference does: adapter/image.py:241-246).
int op_relpos_bias_build_ids(const void* table, const int* bucket, int64_t bucket_ld, const int* ids, void* out, int64_t B,
                             int64_t heads, int64_t K, int64_t Kpad, int transposed, void* stream) {
  OP_CHECK_ARG(table && bucket && ids && out && B > 0 && K > 0 && Kpad >= K && Kpad % 8 == 0, "relpos_bias_build_ids: bad args");
  hipLaunchKernelGGL(relpos_build_ids_kernel, dim3(ew_grid(B * K * Kpad)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)table,
                     bucket, bucket_ld, ids, (bf16_t*)out, (int)B, (int)heads, (int)K, (int)Kpad, transposed);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// Stage 1 of the table gradient from the per-sample bias gradients dbias [B][heads][K][Kpad] fp32 (one slab per sample from
// op_attn_bwd; columns j >= K are not read): the slabs are added into dense_ws, fp32 [heads][Sfull][Sfull] scratch, ZEROED by the
// caller, Sfull = extent of the bucket table the ids index.  op_relpos_bias_bwd (S = Spad = Sfull) then sums dense_ws onto the
// table; it OVERWRITES dtable [num_rel][heads] fp32 (include/onepeace_hip.h), so only dense_ws has to be zeroed.
int op_relpos_bias_fold_ids(const float* dbias, const int* ids, float* dense_ws, int64_t Sfull, int64_t B, int64_t heads, int64_t K,
                            int64_t Kpad, void* stream) {
  OP_CHECK_ARG(dbias && ids && dense_ws && B > 0 && K > 0 && Sfull > 0, "relpos_bias_fold_ids: bad args");
  hipLaunchKernelGGL(relpos_fold_ids_kernel, dim3(ew_grid(B * heads * K * K)), dim3(256), 0, (hipStream_t)stream, dbias, ids, dense_ws,
                     (int)B, (int)heads, (int)K, (int)Kpad, (int)Sfull);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

int op_relpos_bias_bwd(const float* dbias, int64_t S, int64_t Spad, const int* pos, const int* seg, int64_t nseg, const int* bucket_seg,
                       int64_t num_rel, float* partial_ws, float* dtable, int64_t heads, void* stream) {
  OP_CHECK_ARG(dbias && pos && seg && bucket_seg && dtable && (partial_ws || nseg == 0), "relpos_bias_bwd: null pointer");
  OP_CHECK_ARG(S > 0 && Spad >= S && num_rel > 0 && heads > 0 && nseg >= 0 && S * S < (1ll << 31), "relpos_bias_bwd: bad sizes");
  hipStream_t s = (hipStream_t)stream;
  if (nseg > 0)
    hipLaunchKernelGGL(relpos_seg_sum_kernel, dim3(ew_grid(nseg * heads)), dim3(256), 0, s, dbias, pos, seg, partial_ws, (int)nseg,
                       (int)heads, (int)S, (int)Spad);
  hipLaunchKernelGGL(relpos_seg_fold_kernel, dim3(ew_grid(num_rel * heads)), dim3(256), 0, s, (const float*)partial_ws, bucket_seg,
                     dtable, (int)num_rel, (int)heads);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// Row packing of the samples a stochastic-depth branch keeps (see rows_gather_kernel).  Per segment i < nseg (<= 4), host arrays:
// src_row0 (first row of the segment in the full matrix), dst_row0 (first row in the packed matrix), S (rows per sample),
// n_kept, dst_rows (n_kept * S rounded up by the caller; the surplus rows are written as zeros), n_samples, list_off (where the
// segment's list starts in `list`).  `list` (device int32): gather: the kept sample numbers in ascending order; merge: for every
// sample of the segment its position among the kept ones or -1.  cols % 8 == 0, rows 16-byte aligned.
static int rows_segs(RowsSegs& d, int64_t nseg, const int64_t* src_row0, const int64_t* dst_row0, const int64_t* S, const int64_t* n_kept,
                     const int64_t* dst_rows, const int64_t* n_samples, const int64_t* list_off) {
  if (nseg < 1 || nseg > 4 || !src_row0 || !dst_row0 || !S || !n_kept || !dst_rows || !n_samples || !list_off) return 0;
  memset(&d, 0, sizeof(d));
  d.nseg = (int)nseg;
  for (int i = 0; i < (int)nseg; ++i) {
    if (S[i] < 1 || n_kept[i] < 0 || n_kept[i] > n_samples[i] || dst_rows[i] < n_kept[i] * S[i]) return 0;
    d.seg[i].src_row0 = src_row0[i]; d.seg[i].dst_row0 = dst_row0[i]; d.seg[i].S = (int)S[i]; d.seg[i].n_kept = (int)n_kept[i];
    d.seg[i].dst_rows = (int)dst_rows[i]; d.seg[i].n_samples = (int)n_samples[i]; d.seg[i].list_off = (int)list_off[i];
  }
  return 1;
}

int op_rows_gather(const void* src, void* dst, const int* list, int64_t nseg, const int64_t* src_row0, const int64_t* dst_row0,
                   const int64_t* S, const int64_t* n_kept, const int64_t* dst_rows, const int64_t* n_samples, const int64_t* list_off,
                   int64_t dst_total, int64_t cols, void* stream) {
  RowsSegs d;
  OP_CHECK_ARG(src && dst && list && cols > 0 && cols % 8 == 0, "rows_gather: bad argument");
  OP_CHECK_ARG(rows_segs(d, nseg, src_row0, dst_row0, S, n_kept, dst_rows, n_samples, list_off), "rows_gather: bad segment table");
  if (dst_total == 0) return OP_OK;
  int64_t nb = (dst_total + 3) / 4;
  if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(rows_gather_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)src, (bf16_t*)dst, list, d,
                     dst_total, (int)cols);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// out may be `base` itself (then only the rows of kept samples are written).
int op_rows_merge(const void* base, const void* upd, void* out, const int* list, int64_t nseg, const int64_t* src_row0,
                  const int64_t* dst_row0, const int64_t* S, const int64_t* n_kept, const int64_t* dst_rows, const int64_t* n_samples,
                  const int64_t* list_off, int64_t total, int64_t cols, void* stream) {
  RowsSegs d;
  OP_CHECK_ARG(base && out && list && cols > 0 && cols % 8 == 0, "rows_merge: bad argument");
  OP_CHECK_ARG(upd || out != base, "rows_merge: without upd (copy of the dropped samples' rows) out must not be base");
  OP_CHECK_ARG(rows_segs(d, nseg, src_row0, dst_row0, S, n_kept, dst_rows, n_samples, list_off), "rows_merge: bad segment table");
  if (total == 0) return OP_OK;
  int64_t nb = (total + 3) / 4;
  if (nb > 8192) nb = 8192;
  hipLaunchKernelGGL(rows_merge_kernel, dim3((int)nb), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)base, (const bf16_t*)upd,
                     (bf16_t*)out, list, d, total, (int)cols);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// (ABI 9) map[r] = the row of the full matrix packed row r stands for (op_rows_gather's source row), -1 for the surplus rows.
int op_rows_map(int* map, const int* list, int64_t nseg, const int64_t* src_row0, const int64_t* dst_row0, const int64_t* S,
                const int64_t* n_kept, const int64_t* dst_rows, const int64_t* n_samples, const int64_t* list_off, int64_t dst_total,
                void* stream) {
  RowsSegs d;
  OP_CHECK_ARG(map && list, "rows_map: null pointer");
  OP_CHECK_ARG(rows_segs(d, nseg, src_row0, dst_row0, S, n_kept, dst_rows, n_samples, list_off), "rows_map: bad segment table");
  if (dst_total == 0) return OP_OK;
  hipLaunchKernelGGL(rows_map_kernel, dim3((int)((dst_total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, map, list, d, dst_total);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// Live K-tile lists of up to 8 weight-gradient problems over one row matrix, ONE launch, no host synchronisation (see
// live_ktiles_kernel; consumer: op_gemm_tn_grouped_lists).  Segments (HOST arrays of nseg <= 4 entries): rows [row0_i, row0_i + S_i * B_i)
// belong to B_i samples of S_i rows with the DEVICE multipliers ps_i (fp32 [B_i]; a null entry: every sample kept); rows of no segment
// belong to no sample.  Problems (HOST arrays of nprob entries): rows [prob_row0_p, prob_row0_p + prob_rows_p), prob_rows_p % 64 == 0;
// ktiles[p]: DEVICE int32 [prob_rows_p / 64] receives the ascending indices (relative to prob_row0_p) of the 64-row tiles with a row of
// a sample whose ps != 0, n_ktiles[p]: DEVICE int32 their number.
int op_live_ktiles(int64_t nseg, const float* const* ps, const int64_t* row0, const int64_t* S, const int64_t* B, int64_t nprob,
                   const int64_t* prob_row0, const int64_t* prob_rows, int32_t* const* ktiles, int32_t* const* n_ktiles, void* stream) {
  OP_CHECK_ARG(nseg >= 1 && nseg <= LK_MAX_SEG && nprob >= 1 && nprob <= LK_MAX_PROB, "live_ktiles: %lld segments (1 ... %d), %lld problems (1 ... %d)",
               (long long)nseg, LK_MAX_SEG, (long long)nprob, LK_MAX_PROB);
  OP_CHECK_ARG(ps && row0 && S && B && prob_row0 && prob_rows && ktiles && n_ktiles, "live_ktiles: null pointer");
  LiveTilesArgs a;
  memset(&a, 0, sizeof(a));
  a.nseg = (int)nseg;
  for (int i = 0; i < (int)nseg; ++i) {
    OP_CHECK_ARG(row0[i] >= 0 && S[i] >= 1 && B[i] >= 1 && S[i] < ((int64_t)1 << 31) && B[i] < ((int64_t)1 << 31), "live_ktiles: bad segment %d", i);
    a.seg[i].ps = ps[i]; a.seg[i].row0 = row0[i]; a.seg[i].S = (int)S[i]; a.seg[i].B = (int)B[i];
  }
  for (int p = 0; p < (int)nprob; ++p) {
    OP_CHECK_ARG(prob_row0[p] >= 0 && prob_rows[p] >= 64 && prob_rows[p] % 64 == 0 && prob_rows[p] / 64 < ((int64_t)1 << 31) && ktiles[p] && n_ktiles[p],
                 "live_ktiles: bad problem %d", p);
    a.prob[p].row0 = prob_row0[p]; a.prob[p].ntiles = (int)(prob_rows[p] / 64); a.prob[p].list = ktiles[p]; a.prob[p].count = n_ktiles[p];
  }
  hipLaunchKernelGGL(live_ktiles_kernel, dim3((int)nprob), dim3(256), 0, (hipStream_t)stream, a);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

// (additive: op_abi_version() stays 10) Window lists for the input-gradient GEMMs of a residual branch (op_gemm_nt_grouped_windows) and the zero rows they leave
// out, ONE launch, no host synchronisation (see live_mwindows_kernel).  Segments as in op_live_ktiles (HOST arrays of nseg <= 4 entries),
// plus per segment ps_stride (sample b has the multiplier ps[b * ps_stride]: a per-row vector serves with ps_stride = S) and wps: > 0 -- every kept sample is listed as wps windows of 256 rows from its first row on (the caller picks this
// where a sample nearly fills them; odd[i] != 0: and every sample's LAST row, kept or not, is listed in strided windows of 256 samples
// -- for S = 256 n + 1); 0 -- the aligned 256-row tiles of the segment that hold a row of a kept sample.  seg_list /
// seg_prob / seg_base (nseg x 2): the up to two lists a segment feeds (-1: none), the problem index its entries carry there and the
// row of the row matrix at which that problem's operand starts (<= row0; an entry is two words, prob << 28 | row - base and rows << 16 | row stride).  Lists (HOST arrays of
// nlist <= 4): windows[l] DEVICE int32 [2 * max_windows[l]], n_windows[l] DEVICE int32 [1]; the order is segment by segment, ascending.
// Outputs (nout <= 4, may be 0): bf16 matrices of out_rows[o] rows PARALLEL to the row matrix (row stride out_ld[o], out_cols[o]
// columns, both % 8 == 0); the rows of every unit (sample / tile) that is not listed are set to +0 in all of them.  A row that only a
// neighbour's window reaches is zeroed here and written again by the GEMM, which runs later on the stream.
static int live_mwindows_impl(int64_t nseg, const float* const* ps, const int64_t* ps_stride, const int64_t* row0, const int64_t* S, const int64_t* B,
                              const int64_t* wps, const int64_t* odd, const int64_t* seg_list, const int64_t* seg_prob, const int64_t* seg_base, int64_t nlist,
                              int32_t* const* windows,
                              int32_t* const* n_windows, const int64_t* max_windows, int64_t nout, void* const* out, const int64_t* out_ld,
                              const int64_t* out_cols, const int64_t* out_rows, const void* const* out_src, const int64_t* out_src_ld, void* stream) {
  OP_CHECK_ARG(nseg >= 1 && nseg <= MW_MAX_SEG && nlist >= 1 && nlist <= MW_MAX_LIST && nout >= 0 && nout <= MW_MAX_OUT,
               "live_mwindows: %lld segments (1 ... %d), %lld lists (1 ... %d), %lld outputs (0 ... %d)", (long long)nseg, MW_MAX_SEG,
               (long long)nlist, MW_MAX_LIST, (long long)nout, MW_MAX_OUT);
  OP_CHECK_ARG(ps && ps_stride && row0 && S && B && wps && odd && seg_list && seg_prob && seg_base && windows && n_windows && max_windows &&
               (nout == 0 || (out && out_ld && out_cols && out_rows)), "live_mwindows: null pointer");
  MWindowsArgs a;
  memset(&a, 0, sizeof(a));
  a.nseg = (int)nseg; a.nout = (int)nout; a.nlist = (int)nlist;
  int64_t need[MW_MAX_LIST] = {0, 0, 0, 0}, last_row = 0, unit_rows = 1;
  int units = 0;
  for (int i = 0; i < (int)nseg; ++i) {
    OP_CHECK_ARG(row0[i] >= 0 && S[i] >= 1 && B[i] >= 1 && S[i] * B[i] < ((int64_t)1 << 27) && row0[i] < ((int64_t)1 << 40) && wps[i] >= 0 && ps_stride[i] >= 1 && ps_stride[i] < ((int64_t)1 << 31) &&
                 wps[i] <= 64 && (wps[i] == 0 || S[i] <= ((int64_t)1 << 19)) &&
                 (odd[i] == 0 || (wps[i] > 0 && S[i] < 65536 && B[i] <= 65536)), "live_mwindows: bad segment %d", i);
    auto& sg = a.seg[i];
    sg.ps = ps[i]; sg.row0 = row0[i]; sg.S = (int)S[i]; sg.B = (int)B[i]; sg.wps = (int)wps[i]; sg.odd = odd[i] != 0; sg.pstride = (int)ps_stride[i];
    sg.unit0 = units;
    sg.units = sg.wps > 0 ? sg.B : (int)((S[i] * B[i] + 255) / 256);
    units += sg.units;
    if (row0[i] + S[i] * B[i] > last_row) last_row = row0[i] + S[i] * B[i];
    if ((sg.wps > 0 ? S[i] : 256) > unit_rows) unit_rows = sg.wps > 0 ? S[i] : 256;
    for (int k = 0; k < 2; ++k) {
      const int64_t l = seg_list[i * 2 + k];
      sg.list[k] = (int)l;
      if (l < 0) { sg.list[k] = -1; continue; }
      OP_CHECK_ARG(l < nlist && seg_prob[i * 2 + k] >= 0 && seg_prob[i * 2 + k] <= 2 && seg_base[i * 2 + k] >= 0 &&
                   seg_base[i * 2 + k] <= row0[i] && row0[i] - seg_base[i * 2 + k] + S[i] * B[i] + 256 * wps[i] < ((int64_t)1 << 28),
                   "live_mwindows: segment %d: bad list reference %d", i, k);
      sg.prob[k] = (int)seg_prob[i * 2 + k]; sg.base[k] = seg_base[i * 2 + k];
      need[l] += (int64_t)sg.units * (sg.wps > 0 ? sg.wps : 1) + (sg.odd ? (sg.B + 255) / 256 : 0);
    }
  }
  a.nunits = units;
  for (int l = 0; l < (int)nlist; ++l) {
    OP_CHECK_ARG(windows[l] && n_windows[l] && max_windows[l] >= need[l], "live_mwindows: list %d: null, or room for %lld entries (%lld needed)", l,
                 (long long)max_windows[l], (long long)need[l]);
    a.lists[l].list = windows[l]; a.lists[l].count = n_windows[l];
  }
  for (int o = 0; o < (int)nout; ++o) {
    OP_CHECK_ARG(out[o] && ((uintptr_t)out[o] & 15) == 0 && out_cols[o] >= 8 && out_cols[o] % 8 == 0 && out_ld[o] % 8 == 0 && out_ld[o] >= out_cols[o] && out_rows[o] >= last_row &&
                 out_cols[o] < ((int64_t)1 << 31), "live_mwindows: output %d: null or not 16-byte aligned, cols / ld %% 8, or fewer than %lld rows", o, (long long)last_row);
    a.out[o].ptr = (bf16_t*)out[o]; a.out[o].ld = out_ld[o]; a.out[o].cols = (int)out_cols[o];
    if (out_src && out_src[o]) {  // (the source has the output's rows and columns; it must not be the output itself or overlap it)
      OP_CHECK_ARG(out_src_ld && ((uintptr_t)out_src[o] & 15) == 0 && out_src_ld[o] % 8 == 0 && out_src_ld[o] >= out_cols[o] && out_src[o] != out[o],
                   "live_mwindows: source of output %d: not 16-byte aligned, ld %% 8 or ld < cols, or the output itself", o);
      a.out[o].src = (const bf16_t*)out_src[o]; a.out[o].lds = out_src_ld[o];
    }
  }
  hipLaunchKernelGGL(live_mwindows_kernel, dim3(units + (int)nlist, (int)((unit_rows + MW_PIECE - 1) / MW_PIECE)), dim3(256), 0, (hipStream_t)stream, a);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

int op_live_mwindows(int64_t nseg, const float* const* ps, const int64_t* ps_stride, const int64_t* row0, const int64_t* S, const int64_t* B,
                     const int64_t* wps, const int64_t* odd, const int64_t* seg_list, const int64_t* seg_prob, const int64_t* seg_base, int64_t nlist,
                     int32_t* const* windows,
                     int32_t* const* n_windows, const int64_t* max_windows, int64_t nout, void* const* out, const int64_t* out_ld,
                     const int64_t* out_cols, const int64_t* out_rows, void* stream) {
  return live_mwindows_impl(nseg, ps, ps_stride, row0, S, B, wps, odd, seg_list, seg_prob, seg_base, nlist, windows, n_windows, max_windows, nout,
                            out, out_ld, out_cols, out_rows, nullptr, nullptr, stream);
}

// (additive: op_abi_version() stays 10) op_live_mwindows for the FORWARD launches of a residual branch (op_gemm_nt_grouped_windows_fwd):
// the same lists by the same rule, and per output a source matrix out_src[o] (row stride out_src_ld[o] % 8 == 0, 16-byte aligned; null: +0
// as above) whose rows are COPIED into the rows no window covers -- the residual output of the branch takes the residual input there,
// which is what the dense epilogue's fma(0, y, res) gives for a dropped sample; a plain output (q | k | v, h0 | h1) takes +0.
int op_live_mwindows_fwd(int64_t nseg, const float* const* ps, const int64_t* ps_stride, const int64_t* row0, const int64_t* S, const int64_t* B,
                         const int64_t* wps, const int64_t* odd, const int64_t* seg_list, const int64_t* seg_prob, const int64_t* seg_base,
                         int64_t nlist, int32_t* const* windows, int32_t* const* n_windows, const int64_t* max_windows, int64_t nout,
                         void* const* out, const int64_t* out_ld, const int64_t* out_cols, const int64_t* out_rows,
                         const void* const* out_src, const int64_t* out_src_ld, void* stream) {
  OP_CHECK_ARG(nout >= 1 && out_src && out_src_ld, "live_mwindows_fwd: outputs with their source array (entries may be null)");
  return live_mwindows_impl(nseg, ps, ps_stride, row0, S, B, wps, odd, seg_list, seg_prob, seg_base, nlist, windows, n_windows, max_windows, nout,
                            out, out_ld, out_cols, out_rows, out_src, out_src_ld, stream);
}

}  // extern "C"
