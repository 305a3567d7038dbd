// Photometric train transforms on the resized uint8 batch (include/onepeace_hip.h: op_image_color_jitter, op_image_gaussian_blur,
// op_image_normalize_flip).  Replaces the host PIL steps that sit between the resize and ToTensor in the reference's train transforms:
// RandomDistortion = torchvision ColorJitter (utils/transforms.py:144-157; data/vl_data/nlvr2_dataset.py:33-42,
// data/vision_data/image_classify_dataset.py:54-64) and GaussianBlur (utils/transforms.py:160-188; data/vl_data/refcoco_dataset.py:31-36),
// bit for bit.  All three entries work on dense uint8 [B, S, S, 3], S a multiple of 16 in [16, 1024].
//
// ColorJitter is PIL.ImageEnhance: every enhancer is Image.blend(degenerate, image, factor), per byte
//   t = fadd_rn((float)d, fmul_rn(f, (float)(p - d))), two rounded fp32 operations (never an fma); (uint8)t for 0 <= f <= 1, else clipped
//   to 0 ... 255 first.  For 0 <= f <= 1, t lies between d and p, so the clip changes nothing there and ONE clipped form serves both.
// Degenerates: brightness 0; saturation L of the pixel, L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16; contrast the image's rounded mean
// of L, m = (2 sum + count) / (2 count), over the image as it is when the contrast op runs.
// pm_luma_sum_kernel: images with a contrast op only; applies the ops before it per pixel and adds L into sums[image] -- integer atomics,
// the result does not depend on the order.  pm_jitter_kernel: the whole chain per pixel in registers, 16 pixels = 48 bytes = three
// 16-byte loads and stores per work item; an image without an op returns before it reads anything.
//
// GaussianBlur is ImageFilter.GaussianBlur: three extended box blurs along x, then three along y (BoxBlur.c), each from the uint8 result
// of the one before: out[x] = (acc ww + far fw + 2^23) >> 24 in 32-bit unsigned arithmetic, acc = the sum of in[clamp(x + i)], |i| <= R,
// far = in[clamp(x - R - 1)] + in[clamp(x + R + 1)]; R, ww, fw per image from the host (imageprep.gaussian_box_params).
// pm_blur_rows_kernel: workgroup = (image, tile of whole rows); the tile is staged in LDS, the three x passes ping-pong between two LDS
// buffers with a barrier between them, then the tile is written back.  pm_blur_cols_kernel: the same for a strip of columns over all S
// rows.  A workgroup overwrites only what it alone reads, and has read all of it before its first store: that is what makes in place safe.
// A work item of a pass owns 16 consecutive outputs of one line and channel and slides the window sum (integers: exact).
// LDS: two buffers of PM_TILE_BYTES = 12 KiB = 24 KiB per workgroup.  The figure relied on (MI355X microarchitecture guide, "LDS per CU"):
// 160 KiB per CU, all of which one workgroup may declare -- 24 KiB leaves room for 6 workgroups per CU.  At S = 1024 a row tile is 4 rows
// (4 x 3072 B) and a column strip 4 pixels wide (1024 x 12 B).
#include "common.h"
#include "image_store.h"
#include "photometric_blend.h"

#include <algorithm>
#include <cmath>

namespace {

constexpr int PM_THREADS = 256;
constexpr int PM_MAX_S = 1024;
constexpr int PM_MAX_R = 32;
constexpr int PM_TILE_BYTES = 12288;  // one LDS buffer: 4 rows of 1024 pixels, or 1024 rows of 4 pixels
constexpr int PM_SEG = 16;            // outputs per work item of a blur pass (S % 16 == 0)
constexpr int PM_PIX = 16;            // pixels per work item of the jitter kernels: 48 bytes
constexpr int PM_BRIGHTNESS = 1, PM_CONTRAST = 2, PM_SATURATION = 3;

struct PmChain { int op[3]; float f[3]; };

__device__ __forceinline__ PmChain pm_chain(const int* __restrict__ ops, const float* __restrict__ factor, int64_t img) {
  return {{ops[3 * img], ops[3 * img + 1], ops[3 * img + 2]}, {factor[3 * img], factor[3 * img + 1], factor[3 * img + 2]}};
}

__device__ __forceinline__ int pm_luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16; }

// ops [0, n) of the chain on one pixel; m = the contrast mean (used only when a contrast op is among them)
__device__ __forceinline__ void pm_apply(const PmChain& c, int n, int m, int (&px)[3]) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const int op = k < n ? c.op[k] : 0;
    if (op == 0) continue;
    const int d = op == PM_SATURATION ? pm_luma(px[0], px[1], px[2]) : (op == PM_CONTRAST ? m : 0);
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) px[ch] = pm_blend(d, px[ch], c.f[k]);
  }
}

struct PmBytes48 { u32x4 v[3]; };

__device__ __forceinline__ PmBytes48 pm_load48(const uint8_t* p) {
  const u32x4* q = reinterpret_cast<const u32x4*>(p);
  return {{q[0], q[1], q[2]}};
}
__device__ __forceinline__ int pm_byte(const PmBytes48& b, int i) { return (int)((b.v[i >> 4][(i >> 2) & 3] >> ((i & 3) * 8)) & 255u); }

// position of the contrast op in the chain, or -1
__device__ __forceinline__ int pm_contrast_pos(const PmChain& c) {
  return c.op[0] == PM_CONTRAST ? 0 : (c.op[1] == PM_CONTRAST ? 1 : (c.op[2] == PM_CONTRAST ? 2 : -1));
}

__global__ __launch_bounds__(PM_THREADS) void pm_luma_sum_kernel(const uint8_t* __restrict__ img, int S, const int* __restrict__ ops,
                                                                 const float* __restrict__ factor, unsigned* __restrict__ sums) {
  const int64_t b = blockIdx.y;
  const PmChain c = pm_chain(ops, factor, b);
  const int pos = pm_contrast_pos(c);
  if (pos < 0) return;  // uniform: this image needs no mean
  const int items = S * S / PM_PIX;
  const uint8_t* base = img + b * S * S * 3;
  unsigned part = 0;
  for (int it = blockIdx.x * PM_THREADS + threadIdx.x; it < items; it += gridDim.x * PM_THREADS) {
    const PmBytes48 v = pm_load48(base + (int64_t)it * (PM_PIX * 3));
#pragma unroll
    for (int j = 0; j < PM_PIX; ++j) {
      int px[3] = {pm_byte(v, 3 * j), pm_byte(v, 3 * j + 1), pm_byte(v, 3 * j + 2)};
      pm_apply(c, pos, 0, px);
      part += (unsigned)pm_luma(px[0], px[1], px[2]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) part += (unsigned)__shfl_xor((int)part, o);
  if ((threadIdx.x & 63) == 0 && part != 0) atomicAdd(sums + b, part);
}

// in place: every load of a work item precedes its stores, and no other work item touches its 48 bytes
__global__ __launch_bounds__(PM_THREADS) void pm_jitter_kernel(uint8_t* img, int S, const int* __restrict__ ops,
                                                               const float* __restrict__ factor, const unsigned* __restrict__ sums) {
  const int64_t b = blockIdx.y;
  const PmChain c = pm_chain(ops, factor, b);
  if ((c.op[0] | c.op[1] | c.op[2]) == 0) return;  // uniform: an image with no op is neither read nor written
  const unsigned count = (unsigned)(S * S);
  const int m = pm_contrast_pos(c) >= 0 ? (int)((2u * sums[b] + count) / (2u * count)) : 0;  // sum < 2^28: no overflow
  const int items = S * S / PM_PIX;
  uint8_t* base = img + b * S * S * 3;
  for (int it = blockIdx.x * PM_THREADS + threadIdx.x; it < items; it += gridDim.x * PM_THREADS) {
    uint8_t* p = base + (int64_t)it * (PM_PIX * 3);
    const PmBytes48 v = pm_load48(p);
    unsigned w[12] = {};
#pragma unroll
    for (int j = 0; j < PM_PIX; ++j) {
      int px[3] = {pm_byte(v, 3 * j), pm_byte(v, 3 * j + 1), pm_byte(v, 3 * j + 2)};
      pm_apply(c, 3, m, px);
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) {
        const int i = 3 * j + ch;
        w[i >> 2] |= (unsigned)px[ch] << ((i & 3) * 8);
      }
    }
    u32x4* q = reinterpret_cast<u32x4*>(p);
    q[0] = (u32x4){w[0], w[1], w[2], w[3]};
    q[1] = (u32x4){w[4], w[5], w[6], w[7]};
    q[2] = (u32x4){w[8], w[9], w[10], w[11]};
  }
}

// One extended box blur over `lines` lines of `size` samples each, from LDS buffer `in` to `out`.  Sample x of line l is the byte at
// line_off(l) + x * stride.  Work item = (line, segment of PM_SEG outputs): window sum once, then slid.
template <bool ROWS>
__device__ __forceinline__ void pm_box_pass(const uint8_t* in, uint8_t* out, int lines, int size, int row_bytes, int stride, int R,
                                            unsigned ww, unsigned fw) {
  const int segs = size / PM_SEG;
  for (int it = threadIdx.x; it < lines * segs; it += PM_THREADS) {
    const int l = it % lines, x0 = (it / lines) * PM_SEG;
    const int off = ROWS ? (l / 3) * row_bytes + l % 3 : l;  // rows: line = (row, channel); columns: line = byte column of the strip
    const uint8_t* src = in + off;
    uint8_t* dst = out + off;
    const int last = size - 1;
    int acc = 0;
    for (int i = -R; i <= R; ++i) acc += src[min(max(x0 + i, 0), last) * stride];
#pragma unroll 4
    for (int x = x0; x < x0 + PM_SEG; ++x) {
      const int enter = src[min(x + R + 1, last) * stride];
      const unsigned far = (unsigned)(src[max(x - R - 1, 0) * stride] + enter);
      dst[x * stride] = (uint8_t)(((unsigned)acc * ww + far * fw + (1u << 23)) >> 24);
      acc += enter - src[max(x - R, 0) * stride];
    }
  }
}

// the three passes: a -> b -> a -> b; the result is in b
template <bool ROWS>
__device__ __forceinline__ void pm_three_passes(uint8_t* a, uint8_t* b, int lines, int size, int row_bytes, int stride, int R, unsigned ww,
                                                unsigned fw) {
  __syncthreads();
  pm_box_pass<ROWS>(a, b, lines, size, row_bytes, stride, R, ww, fw);
  __syncthreads();
  pm_box_pass<ROWS>(b, a, lines, size, row_bytes, stride, R, ww, fw);
  __syncthreads();
  pm_box_pass<ROWS>(a, b, lines, size, row_bytes, stride, R, ww, fw);
  __syncthreads();
}

// rows per tile of the row kernel / pixels per strip of the column kernel: what fits PM_TILE_BYTES (strips in whole groups of 4 pixels =
// 3 dwords per row)
inline int pm_tile_rows(int S) { return std::max(1, std::min(S, PM_TILE_BYTES / (S * 3))); }
inline int pm_strip_cols(int S) { return std::min(S, (PM_TILE_BYTES / (S * 3)) & ~3); }

__global__ __launch_bounds__(PM_THREADS) void pm_blur_rows_kernel(uint8_t* img, int S, int tile_rows, const int* __restrict__ Rt,
                                                                  const unsigned* __restrict__ wwt, const unsigned* __restrict__ fwt,
                                                                  const uint8_t* __restrict__ on) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][PM_TILE_BYTES];
  const int64_t b = blockIdx.y;
  if (on[b] == 0) return;  // uniform: not blurred, not touched
  const int R = Rt[b];
  const unsigned ww = wwt[b], fw = fwt[b];
  const int r0 = blockIdx.x * tile_rows, nr = min(tile_rows, S - r0), row_bytes = S * 3;
  uint8_t* g = img + (b * S + r0) * row_bytes;  // the tile's rows are contiguous: nr * row_bytes bytes, a multiple of 16
  const int vecs = nr * row_bytes / 16;
  for (int i = threadIdx.x; i < vecs; i += PM_THREADS)
    reinterpret_cast<u32x4*>(lds[0])[i] = reinterpret_cast<const u32x4*>(g)[i];
  pm_three_passes<true>(lds[0], lds[1], nr * 3, S, row_bytes, 3, R, ww, fw);
  for (int i = threadIdx.x; i < vecs; i += PM_THREADS)
    reinterpret_cast<u32x4*>(g)[i] = reinterpret_cast<const u32x4*>(lds[1])[i];
}

__global__ __launch_bounds__(PM_THREADS) void pm_blur_cols_kernel(uint8_t* img, int S, int strip_cols, const int* __restrict__ Rt,
                                                                  const unsigned* __restrict__ wwt, const unsigned* __restrict__ fwt,
                                                                  const uint8_t* __restrict__ on) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][PM_TILE_BYTES];
  const int64_t b = blockIdx.y;
  if (on[b] == 0) return;
  const int R = Rt[b];
  const unsigned ww = wwt[b], fw = fwt[b];
  const int c0 = blockIdx.x * strip_cols, nc = min(strip_cols, S - c0);
  const int strip_bytes = nc * 3, dw = strip_bytes / 4;  // nc % 4 == 0: whole dwords, dword-aligned in every row
  uint8_t* g = img + (b * S * S + c0) * 3;
  for (int i = threadIdx.x; i < S * dw; i += PM_THREADS) {
    const int y = i / dw, k = i % dw;
    reinterpret_cast<unsigned*>(lds[0])[i] = reinterpret_cast<const unsigned*>(g + (int64_t)y * S * 3)[k];
  }
  pm_three_passes<false>(lds[0], lds[1], strip_bytes, S, 0, strip_bytes, R, ww, fw);
  for (int i = threadIdx.x; i < S * dw; i += PM_THREADS) {
    const int y = i / dw, k = i % dw;
    reinterpret_cast<unsigned*>(g + (int64_t)y * S * 3)[k] = reinterpret_cast<const unsigned*>(lds[1])[i];
  }
}

// uint8 [B, S, S, 3] -> [B, 3, S, S]: work item = (row, 4 columns) = 12 bytes = 3 aligned dwords, then the store of the resize kernel
template <int OUT>
__global__ __launch_bounds__(PM_THREADS) void pm_normalize_flip_kernel(const uint8_t* __restrict__ src, void* __restrict__ out, int S,
                                                                       IrNorm nm, const uint8_t* __restrict__ flip) {
  const int64_t img = blockIdx.y;
  const bool flipped = flip != nullptr && flip[img] != 0;  // uniform
  const int G = S / 4;
  for (int it = blockIdx.x * PM_THREADS + threadIdx.x; it < G * S; it += gridDim.x * PM_THREADS) {
    const int g = it % G, y = it / G;
    const unsigned* q = reinterpret_cast<const unsigned*>(src + ((img * S + y) * S + g * 4) * 3);
    const unsigned d0 = q[0], d1 = q[1], d2 = q[2];
    int u[4][3] = {{(int)(d0 & 255), (int)((d0 >> 8) & 255), (int)((d0 >> 16) & 255)},
                   {(int)(d0 >> 24), (int)(d1 & 255), (int)((d1 >> 8) & 255)},
                   {(int)((d1 >> 16) & 255), (int)(d1 >> 24), (int)(d2 & 255)},
                   {(int)((d2 >> 8) & 255), (int)((d2 >> 16) & 255), (int)(d2 >> 24)}};
    ir_store_group<OUT>(out, u, img, y, g, G, S, nm, flipped);
  }
}

int pm_check_batch(const char* what, const void* img, int64_t B, int64_t S) {
  OP_CHECK_ARG(S >= 16 && S <= PM_MAX_S && S % 16 == 0, "%s: S = %lld, need a multiple of 16 in [16, %d]", what, (long long)S, PM_MAX_S);
  OP_CHECK_ARG(B >= 0 && B <= 65535, "%s: B = %lld, need 0 ... 65535", what, (long long)B);
  OP_CHECK_ARG(B == 0 || (img && ((uintptr_t)img & 15) == 0), "%s: the image batch must be a 16-byte aligned device pointer", what);
  return OP_OK;
}

// blocks along x for a grid-stride pass of `items` work items per image: enough to cover them, at most ~4096 workgroups in all
unsigned pm_blocks(int64_t items, int64_t B) {
  const int64_t need = (items + PM_THREADS - 1) / PM_THREADS;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(need, std::max<int64_t>(1, 4096 / B)));
}

}  // namespace

extern "C" int op_image_color_jitter(void* img, int64_t B, int64_t S, const int* ops, const float* factor, const int* ops_host,
                                     const float* factor_host, unsigned* sums, void* stream) {
  if (int rc = pm_check_batch("op_image_color_jitter", img, B, S)) return rc;
  if (B == 0) return OP_OK;
  OP_CHECK_ARG(ops && factor && ops_host && factor_host && sums, "op_image_color_jitter: null pointer");
  OP_CHECK_ARG(((uintptr_t)ops & 3) == 0 && ((uintptr_t)factor & 3) == 0 && ((uintptr_t)sums & 3) == 0 && ((uintptr_t)ops_host & 3) == 0 &&
                   ((uintptr_t)factor_host & 3) == 0,
               "op_image_color_jitter: ops, factor and sums must be 4-byte aligned");
  bool any = false, any_contrast = false;
  for (int64_t i = 0; i < B; ++i) {
    int contrasts = 0;
    for (int k = 0; k < 3; ++k) {
      const int op = ops_host[3 * i + k];
      const float f = factor_host[3 * i + k];
      OP_CHECK_ARG(op >= 0 && op <= PM_SATURATION, "op_image_color_jitter: image %lld: op %d, need 0 (none), 1 (brightness), 2 (contrast) or 3 (saturation)",
                   (long long)i, op);
      OP_CHECK_ARG(std::isfinite(f) && f >= 0.0f, "op_image_color_jitter: image %lld: factor %g, need a finite value >= 0", (long long)i,
                   (double)f);
      any |= op != 0;
      contrasts += op == PM_CONTRAST;
    }
    OP_CHECK_ARG(contrasts <= 1, "op_image_color_jitter: image %lld has %d contrast ops, need at most one", (long long)i, contrasts);
    any_contrast |= contrasts != 0;
  }
  if (!any) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(pm_blocks(S * S / PM_PIX, B), (unsigned)B);
  if (any_contrast) {
    hipError_t e = hipMemsetAsync(sums, 0, (size_t)B * sizeof(unsigned), st);
    if (e != hipSuccess) {
      op_set_error("op_image_color_jitter: hipMemsetAsync failed: %s", hipGetErrorString(e));
      return (int)e;
    }
    hipLaunchKernelGGL(pm_luma_sum_kernel, grid, dim3(PM_THREADS), 0, st, (const uint8_t*)img, (int)S, ops, factor, sums);
    OP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(pm_jitter_kernel, grid, dim3(PM_THREADS), 0, st, (uint8_t*)img, (int)S, ops, factor, (const unsigned*)sums);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

extern "C" int op_image_gaussian_blur(void* img, int64_t B, int64_t S, const int* R, const unsigned* ww, const unsigned* fw,
                                      const uint8_t* on, const int* R_host, const uint8_t* on_host, void* stream) {
  if (int rc = pm_check_batch("op_image_gaussian_blur", img, B, S)) return rc;
  if (B == 0) return OP_OK;
  OP_CHECK_ARG(R && ww && fw && on && R_host && on_host, "op_image_gaussian_blur: null pointer");
  OP_CHECK_ARG(((uintptr_t)R & 3) == 0 && ((uintptr_t)ww & 3) == 0 && ((uintptr_t)fw & 3) == 0 && ((uintptr_t)R_host & 3) == 0,
               "op_image_gaussian_blur: R, ww and fw must be 4-byte aligned");
  bool any = false;
  for (int64_t i = 0; i < B; ++i) {
    if (!on_host[i]) continue;
    any = true;
    OP_CHECK_ARG(R_host[i] >= 0 && R_host[i] <= PM_MAX_R, "op_image_gaussian_blur: image %lld: box radius %d, need 0 ... %d", (long long)i,
                 R_host[i], PM_MAX_R);
  }
  if (!any) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  const int tile_rows = pm_tile_rows((int)S), strip_cols = pm_strip_cols((int)S);
  hipLaunchKernelGGL(pm_blur_rows_kernel, dim3((unsigned)((S + tile_rows - 1) / tile_rows), (unsigned)B), dim3(PM_THREADS), 0, st,
                     (uint8_t*)img, (int)S, tile_rows, R, ww, fw, on);
  OP_LAUNCH_CHECK();
  hipLaunchKernelGGL(pm_blur_cols_kernel, dim3((unsigned)((S + strip_cols - 1) / strip_cols), (unsigned)B), dim3(PM_THREADS), 0, st,
                     (uint8_t*)img, (int)S, strip_cols, R, ww, fw, on);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

extern "C" int op_image_normalize_flip(const void* src, int64_t B, int64_t S, const float* mean, const float* stdev, void* out, int out_dtype,
                                       const uint8_t* flip, void* stream) {
  if (int rc = pm_check_batch("op_image_normalize_flip", src, B, S)) return rc;
  OP_CHECK_ARG(out_dtype == OP_DT_BF16 || out_dtype == OP_DT_F32, "op_image_normalize_flip: out_dtype = %d, need 0 (bf16) or 1 (f32)", out_dtype);
  OP_CHECK_ARG(mean && stdev, "op_image_normalize_flip: mean / stdev (host float[3]) are required");
  if (B == 0) return OP_OK;
  OP_CHECK_ARG(out && ((uintptr_t)out & 15) == 0, "op_image_normalize_flip: out must be a 16-byte aligned device pointer");
  const int64_t in_bytes = B * S * S * 3, out_bytes = in_bytes * (out_dtype == OP_DT_BF16 ? 2 : 4);
  const uintptr_t sa = (uintptr_t)src, oa = (uintptr_t)out;
  OP_CHECK_ARG(sa + in_bytes <= oa || oa + out_bytes <= sa, "op_image_normalize_flip: out must not overlap src");
  IrNorm nm;
  for (int c = 0; c < 3; ++c) nm.mean[c] = mean[c], nm.stdev[c] = stdev[c];
  const dim3 grid(pm_blocks(S * S / 4, B), (unsigned)B);
  hipStream_t st = (hipStream_t)stream;
  if (out_dtype == OP_DT_BF16)
    hipLaunchKernelGGL(pm_normalize_flip_kernel<OP_DT_BF16>, grid, dim3(PM_THREADS), 0, st, (const uint8_t*)src, out, (int)S, nm, flip);
  else
    hipLaunchKernelGGL(pm_normalize_flip_kernel<OP_DT_F32>, grid, dim3(PM_THREADS), 0, st, (const uint8_t*)src, out, (int)S, nm, flip);
  OP_LAUNCH_CHECK();
  return OP_OK;
}
