// RandAugment and RandomErasing of timm's create_transform as the reference's image-classification fine-tune calls it
// (data/vision_data/image_classify_dataset.py:65-77: auto_augment='rand-m9-mstd0.5-inc1', interpolation='bicubic', re_prob=0.25,
// re_mode='pixel'), on the device (include/onepeace_hip.h: op_image_randaug_layer, op_image_erase).  timm's RandAugment ops are Pillow
// calls on the resized uint8 image; every op here gives Pillow's bytes.  The batch is the dense uint8 [B, S, S, 3] the resize writes.
//
// op_image_randaug_layer applies ONE layer: one op per image (op int32 [B], arg fp64 [B, 6]).
//   ra_hist_kernel   images with AutoContrast / Equalize only: the three 256-bin channel histograms, counted in LDS and added to
//                    hist[image] with integer atomics -- the result does not depend on the order.  A bin holds at most S S <= 2^20.
//   ra_apply_kernel  pointwise ops (1 ... 6): every workgroup builds its image's three 256-entry LUTs in LDS (ImageOps.autocontrast /
//                    equalize from the histogram; invert, posterize, solarize, solarize-add from the byte), then maps 16 pixels = 48 bytes
//                    per work item in place.  Neighbourhood ops read the batch and write the scratch: Sharpness (ImageFilter.SMOOTH in
//                    integers, then the Image.blend of photometric_blend.h) and Affine (Geometry.c: affine_transform +
//                    bicubic_filter32RGB in fp64, one rounding per C operation), 4 pixels = three dwords per work item.
//   ra_copy_back_kernel  the images of the neighbourhood ops, scratch -> batch, 16 bytes per work item.
// An image with op 0 is neither read nor written by any of them.
//
// The fp64 arithmetic of Affine and of the AutoContrast LUT must round after every product and sum as Pillow's C does: it is written as
// plain products and sums under `#pragma clang fp contract(off)` (csrc/photometric_blend.h records why not __dmul_rn / __dadd_rn).
//
// op_image_erase is RandomErasing's store: x[i, :, top:top+h, left:left+w] = noise_i.view(3, h, w).to(x.dtype), one launch for the batch.
#include "common.h"
#include "photometric_blend.h"

#include <algorithm>
#include <cfloat>
#include <cmath>

namespace {

constexpr int RA_THREADS = 256;
constexpr int RA_MAX_S = 1024;
constexpr int RA_PIX = 16;  // pixels per work item of the pointwise pass: 48 bytes
constexpr int RA_BINS = 3 * 256;
constexpr int RA_ERASE_MAX_S = 16384;  // 3 S S < 2^31
enum : int {
  RA_NONE = 0, RA_AUTOCONTRAST = 1, RA_EQUALIZE = 2, RA_INVERT = 3, RA_POSTERIZE = 4, RA_SOLARIZE = 5, RA_SOLARIZE_ADD = 6,
  RA_COLOR = 7, RA_CONTRAST = 8, RA_BRIGHTNESS = 9,  // op_image_color_jitter's; refused here
  RA_SHARPNESS = 10, RA_AFFINE = 11
};

struct RaFill { int c[3]; };
struct RaBytes48 { u32x4 v[3]; };

__device__ __forceinline__ RaBytes48 ra_load48(const uint8_t* p) {
  const u32x4* q = reinterpret_cast<const u32x4*>(p);
  return {{q[0], q[1], q[2]}};
}
__device__ __forceinline__ int ra_byte(const RaBytes48& b, int i) { return (int)((b.v[i >> 4][(i >> 2) & 3] >> ((i & 3) * 8)) & 255u); }

__host__ __device__ inline bool ra_uses_hist(int op) { return op == RA_AUTOCONTRAST || op == RA_EQUALIZE; }
__host__ __device__ inline bool ra_uses_scratch(int op) { return op == RA_SHARPNESS || op == RA_AFFINE; }

__global__ __launch_bounds__(RA_THREADS) void ra_hist_kernel(const uint8_t* __restrict__ img, int S, const int* __restrict__ ops,
                                                             unsigned* __restrict__ hist) {
  __shared__ unsigned h[RA_BINS];
  const int64_t b = blockIdx.y;
  if (!ra_uses_hist(ops[b])) return;  // uniform
  for (int i = threadIdx.x; i < RA_BINS; i += RA_THREADS) h[i] = 0;
  __syncthreads();
  const int items = S * S / RA_PIX;
  const uint8_t* base = img + b * S * S * 3;
  for (int it = blockIdx.x * RA_THREADS + threadIdx.x; it < items; it += gridDim.x * RA_THREADS) {
    const RaBytes48 v = ra_load48(base + (int64_t)it * (RA_PIX * 3));
#pragma unroll
    for (int i = 0; i < RA_PIX * 3; ++i) atomicAdd(&h[(i % 3) * 256 + ra_byte(v, i)], 1u);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < RA_BINS; i += RA_THREADS)
    if (h[i] != 0) atomicAdd(hist + b * RA_BINS + i, h[i]);
}

// ImageOps.autocontrast, entry i of a channel whose first / last non-empty bins are lo < hi
__device__ __forceinline__ int ra_autocontrast_entry(int i, int lo, int hi) {
#pragma clang fp contract(off)
  const double scale = 255.0 / (double)(hi - lo);
  const double offset = (double)(-lo) * scale;
  const double prod = (double)i * scale;
  const double v = prod + offset;
  return min(max((int)v, 0), 255);
}

// invert, posterize, solarize, solarize-add of byte p; a = the op's integer argument
__device__ __forceinline__ int ra_point(int op, int p, int a) {
  switch (op) {
    case RA_INVERT: return 255 - p;
    case RA_POSTERIZE: return p & ~((1 << (8 - a)) - 1) & 255;
    case RA_SOLARIZE: return p < a ? p : 255 - p;
    case RA_SOLARIZE_ADD: return p < 128 ? min(255, p + a) : p;
    default: return p;
  }
}

// The three LUTs of the image's pointwise op into lut[3][256]; h is LDS scratch of RA_BINS counters.  All threads of the workgroup call it.
__device__ __forceinline__ void ra_build_lut(int op, int a, int S, const unsigned* __restrict__ hist, unsigned* h, int* bounds, uint8_t* lut) {
  const int t = threadIdx.x;  // RA_THREADS == 256: thread t owns bin t of the three channels
  if (!ra_uses_hist(op)) {
#pragma unroll
    for (int c = 0; c < 3; ++c) lut[c * 256 + t] = (uint8_t)ra_point(op, t, a);
    __syncthreads();
    return;
  }
  if (t < 3) bounds[t] = 255, bounds[3 + t] = 0;  // first / last non-empty bin per channel
  unsigned own[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) own[c] = h[c * 256 + t] = hist[c * 256 + t];
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c)
    if (own[c] != 0) atomicMin(&bounds[c], t), atomicMax(&bounds[3 + c], t);
  __syncthreads();
  if (op == RA_AUTOCONTRAST) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int lo = bounds[c], hi = bounds[3 + c];
      lut[c * 256 + t] = (uint8_t)(hi <= lo ? t : ra_autocontrast_entry(t, lo, hi));
    }
    __syncthreads();
    return;
  }
  // Equalize: n_i = step / 2 + the counts below bin i -- an inclusive scan of the three channels in LDS, minus the bin itself
  for (int off = 1; off < 256; off <<= 1) {
    unsigned add[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) add[c] = t >= off ? h[c * 256 + t - off] : 0u;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c * 256 + t] += add[c];
    __syncthreads();
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int lo = bounds[c], hi = bounds[3 + c];
    const unsigned total = h[c * 256 + 255];                                    // = S S
    const unsigned last = h[c * 256 + hi] - (hi > 0 ? h[c * 256 + hi - 1] : 0u);  // the count of the last non-empty bin
    const unsigned step = hi <= lo ? 0u : (total - last) / 255u;
    const unsigned below = h[c * 256 + t] - own[c];
    lut[c * 256 + t] = (uint8_t)(step == 0 ? (unsigned)t : min(255u, (step / 2 + below) / step));
  }
  __syncthreads();
}

// ImageFilter.SMOOTH of channel byte (x, y, ch): (2 s + 13) / 26, s = the 3 x 3 sum with centre weight 5; the border is copied
__device__ __forceinline__ int ra_smooth(const uint8_t* __restrict__ src, int S, int x, int y, int ch, int p) {
  if (x == 0 || y == 0 || x == S - 1 || y == S - 1) return p;
  int s = 4 * p;
#pragma unroll
  for (int dy = -1; dy <= 1; ++dy) {
    const uint8_t* row = src + ((int64_t)(y + dy) * S + x) * 3 + ch;
    s += row[-3] + row[0] + row[3];
  }
  return (2 * s + 13) / 26;
}

// Geometry.c BICUBIC(v, v1, v2, v3, v4, d)
__device__ __forceinline__ double ra_cub(double v1, double v2, double v3, double v4, double d) {
#pragma clang fp contract(off)
  const double p1 = v2;
  const double p2 = -v1 + v3;
  const double p3 = 2 * (v1 - v2) + v3 - v4;
  const double p4 = -v1 + v2 - v3 + v4;
  return p1 + d * (p2 + d * (p3 + d * p4));
}

// output pixel (x, y) of Image.transform(AFFINE, a, BICUBIC, fillcolor): every index is clamped into the image before it is read
__device__ __forceinline__ void ra_affine_pixel(const uint8_t* __restrict__ src, int S, const double (&a)[6], int x, int y, const RaFill& fill,
                                                int (&out)[3]) {
#pragma clang fp contract(off)
  const double xc = (double)x + 0.5, yc = (double)y + 0.5;
  double xin = a[0] * xc + a[1] * yc + a[2];
  double yin = a[3] * xc + a[4] * yc + a[5];
  const double size = (double)S;
  if (!(xin >= 0.0 && xin < size && yin >= 0.0 && yin < size)) {
    out[0] = fill.c[0], out[1] = fill.c[1], out[2] = fill.c[2];
    return;
  }
  xin -= 0.5;
  yin -= 0.5;
  const double fx = floor(xin), fy = floor(yin);  // in [-1, S - 1]
  const double dx = xin - fx, dy = yin - fy;
  const int ix = (int)fx - 1, iy = (int)fy - 1;
  int col[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) col[i] = min(max(ix + i, 0), S - 1) * 3;
  double r[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int yy = iy + j;
    if (j == 0 || (yy >= 0 && yy < S)) {  // row 0 is read at its clamped index; a later row outside the image repeats the one before
      const uint8_t* row = src + (int64_t)min(max(yy, 0), S - 1) * S * 3;
#pragma unroll
      for (int c = 0; c < 3; ++c)
        r[c][j] = ra_cub((double)row[col[0] + c], (double)row[col[1] + c], (double)row[col[2] + c], (double)row[col[3] + c], dx);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) r[c][j] = r[c][j > 0 ? j - 1 : 0];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const double v = ra_cub(r[c][0], r[c][1], r[c][2], r[c][3], dy);
    out[c] = v <= 0.0 ? 0 : (v >= 255.0 ? 255 : (int)v);  // truncated, not rounded
  }
}

// img and scratch never alias (checked on the host); the pointwise ops read and write img, every load of a work item before its stores
__global__ __launch_bounds__(RA_THREADS) void ra_apply_kernel(uint8_t* img, uint8_t* __restrict__ scratch, int S, const int* __restrict__ ops,
                                                              const double* __restrict__ arg, const unsigned* __restrict__ hist, RaFill fill) {
  __shared__ unsigned h[RA_BINS];
  __shared__ int bounds[6];
  __shared__ uint8_t lut[RA_BINS];
  const int64_t b = blockIdx.y;
  const int op = ops[b];
  if (op == RA_NONE) return;  // uniform: neither read nor written
  uint8_t* base = img + b * S * S * 3;
  if (!ra_uses_scratch(op)) {
    ra_build_lut(op, (int)arg[6 * b], S, hist + b * RA_BINS, h, bounds, lut);
    const int items = S * S / RA_PIX;
    for (int it = blockIdx.x * RA_THREADS + threadIdx.x; it < items; it += gridDim.x * RA_THREADS) {
      uint8_t* p = base + (int64_t)it * (RA_PIX * 3);
      const RaBytes48 v = ra_load48(p);
      unsigned w[12] = {};
#pragma unroll
      for (int i = 0; i < RA_PIX * 3; ++i) w[i >> 2] |= (unsigned)lut[(i % 3) * 256 + ra_byte(v, i)] << ((i & 3) * 8);
      u32x4* q = reinterpret_cast<u32x4*>(p);
      q[0] = (u32x4){w[0], w[1], w[2], w[3]};
      q[1] = (u32x4){w[4], w[5], w[6], w[7]};
      q[2] = (u32x4){w[8], w[9], w[10], w[11]};
    }
    return;
  }
  // neighbourhood ops: work item = (row, 4 columns) = 12 bytes = 3 aligned dwords of the scratch
  uint8_t* dst = scratch + b * S * S * 3;
  const int G = S / 4;
  const float f = (float)arg[6 * b];
  double a[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) a[k] = arg[6 * b + k];
  for (int it = blockIdx.x * RA_THREADS + threadIdx.x; it < G * S; it += gridDim.x * RA_THREADS) {
    const int g = it % G, y = it / G;
    unsigned w[3] = {};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int x = g * 4 + j;
      int px[3];
      if (op == RA_SHARPNESS) {
        const uint8_t* p = base + ((int64_t)y * S + x) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) px[c] = pm_blend(ra_smooth(base, S, x, y, c, p[c]), p[c], f);
      } else {
        ra_affine_pixel(base, S, a, x, y, fill, px);
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int i = 3 * j + c;
        w[i >> 2] |= (unsigned)px[c] << ((i & 3) * 8);
      }
    }
    unsigned* q = reinterpret_cast<unsigned*>(dst + ((int64_t)y * S + g * 4) * 3);
    q[0] = w[0], q[1] = w[1], q[2] = w[2];
  }
}

__global__ __launch_bounds__(RA_THREADS) void ra_copy_back_kernel(uint8_t* __restrict__ img, const uint8_t* __restrict__ scratch, int S,
                                                                  const int* __restrict__ ops) {
  const int64_t b = blockIdx.y;
  if (!ra_uses_scratch(ops[b])) return;  // uniform
  const int vecs = S * S * 3 / 16;
  u32x4* d = reinterpret_cast<u32x4*>(img + b * S * S * 3);
  const u32x4* s = reinterpret_cast<const u32x4*>(scratch + b * S * S * 3);
  for (int i = blockIdx.x * RA_THREADS + threadIdx.x; i < vecs; i += gridDim.x * RA_THREADS) d[i] = s[i];
}

template <typename T>
__global__ __launch_bounds__(RA_THREADS) void ra_erase_kernel(T* __restrict__ x, int S, const int* __restrict__ box,
                                                              const float* __restrict__ noise, const int64_t* __restrict__ noise_off) {
  const int64_t b = blockIdx.y;
  const int top = box[4 * b], left = box[4 * b + 1], h = box[4 * b + 2], w = box[4 * b + 3];
  if (h <= 0 || w <= 0) return;  // uniform: untouched
  const int n = 3 * h * w;       // < 3 S S < 2^31
  const float* src = noise + noise_off[b];
  T* xb = x + b * 3 * S * S;
  for (int e = blockIdx.x * RA_THREADS + threadIdx.x; e < n; e += gridDim.x * RA_THREADS) {
    const int q = e % w, t = e / w, r = t % h, c = t / h;
    xb[((int64_t)c * S + top + r) * S + left + q] = (T)src[e];
  }
}

// blocks along x for a grid-stride pass of `items` work items per image: enough to cover them, at most ~4096 workgroups in all
unsigned ra_blocks(int64_t items, int64_t B) {
  const int64_t need = (items + RA_THREADS - 1) / RA_THREADS;
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(need, std::max<int64_t>(1, 4096 / B)));
}

bool ra_whole(double v, double lo, double hi) { return std::isfinite(v) && v >= lo && v <= hi && v == std::floor(v); }

}  // namespace

extern "C" int op_image_randaug_layer(void* img, int64_t B, int64_t S, const int* op, const double* arg, const int* op_host,
                                      const double* arg_host, const uint8_t* fill, unsigned* hist, void* scratch, void* stream) {
  const char* what = "op_image_randaug_layer";
  OP_CHECK_ARG(S >= 16 && S <= RA_MAX_S && S % 16 == 0, "%s: S = %lld, need a multiple of 16 in [16, %d]", what, (long long)S, RA_MAX_S);
  OP_CHECK_ARG(B >= 0 && B <= 65535, "%s: B = %lld, need 0 ... 65535", what, (long long)B);
  if (B == 0) return OP_OK;
  OP_CHECK_ARG(img && ((uintptr_t)img & 15) == 0 && scratch && ((uintptr_t)scratch & 15) == 0,
               "%s: the image batch and the scratch must be 16-byte aligned device pointers", what);
  OP_CHECK_ARG(op && arg && op_host && arg_host && fill && hist, "%s: null pointer", what);
  OP_CHECK_ARG(((uintptr_t)op & 3) == 0 && ((uintptr_t)op_host & 3) == 0 && ((uintptr_t)hist & 3) == 0 && ((uintptr_t)arg & 7) == 0 &&
                   ((uintptr_t)arg_host & 7) == 0,
               "%s: op and hist must be 4-byte aligned, arg 8-byte aligned", what);
  const int64_t bytes = B * S * S * 3;
  const uintptr_t ia = (uintptr_t)img, sa = (uintptr_t)scratch;
  OP_CHECK_ARG(ia + bytes <= sa || sa + bytes <= ia, "%s: the scratch must not overlap the image batch", what);
  bool any = false, any_hist = false, any_scratch = false;
  for (int64_t i = 0; i < B; ++i) {
    const int o = op_host[i];
    const double* a = arg_host + 6 * i;
    OP_CHECK_ARG(!(o >= RA_COLOR && o <= RA_BRIGHTNESS),
                 "%s: image %lld: op %d (Color / Contrast / Brightness) belongs to op_image_color_jitter", what, (long long)i, o);
    OP_CHECK_ARG(o >= RA_NONE && o <= RA_AFFINE, "%s: image %lld: op %d, need 0 ... 6, 10 or 11", what, (long long)i, o);
    if (o == RA_POSTERIZE) OP_CHECK_ARG(ra_whole(a[0], 0, 7), "%s: image %lld: posterize bits %g, need an integer in 0 ... 7", what, (long long)i, a[0]);
    if (o == RA_SOLARIZE) OP_CHECK_ARG(ra_whole(a[0], 0, 256), "%s: image %lld: solarize threshold %g, need an integer in 0 ... 256", what, (long long)i, a[0]);
    if (o == RA_SOLARIZE_ADD) OP_CHECK_ARG(ra_whole(a[0], 0, 255), "%s: image %lld: solarize-add %g, need an integer in 0 ... 255", what, (long long)i, a[0]);
    if (o == RA_SHARPNESS)
      OP_CHECK_ARG(std::isfinite(a[0]) && a[0] >= 0.0 && a[0] <= (double)FLT_MAX, "%s: image %lld: sharpness factor %g, need a finite value >= 0", what,
                   (long long)i, a[0]);
    if (o == RA_AFFINE)
      for (int k = 0; k < 6; ++k) OP_CHECK_ARG(std::isfinite(a[k]), "%s: image %lld: affine coefficient %d is not finite", what, (long long)i, k);
    any |= o != RA_NONE;
    any_hist |= ra_uses_hist(o);
    any_scratch |= ra_uses_scratch(o);
  }
  if (!any) return OP_OK;
  hipStream_t st = (hipStream_t)stream;
  if (any_hist) {
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)B * RA_BINS * sizeof(unsigned), st);
    if (e != hipSuccess) {
      op_set_error("%s: hipMemsetAsync failed: %s", what, hipGetErrorString(e));
      return (int)e;
    }
    hipLaunchKernelGGL(ra_hist_kernel, dim3(ra_blocks(S * S / RA_PIX, B), (unsigned)B), dim3(RA_THREADS), 0, st, (const uint8_t*)img, (int)S, op, hist);
    OP_LAUNCH_CHECK();
  }
  const RaFill fl = {{fill[0], fill[1], fill[2]}};
  // the neighbourhood ops have S S / 4 work items per image, the pointwise ones S S / 16: the grid covers the larger count that occurs
  const int64_t items = any_scratch ? S * S / 4 : S * S / RA_PIX;
  hipLaunchKernelGGL(ra_apply_kernel, dim3(ra_blocks(items, B), (unsigned)B), dim3(RA_THREADS), 0, st, (uint8_t*)img, (uint8_t*)scratch, (int)S, op,
                     arg, (const unsigned*)hist, fl);
  OP_LAUNCH_CHECK();
  if (any_scratch) {
    hipLaunchKernelGGL(ra_copy_back_kernel, dim3(ra_blocks(S * S * 3 / 16, B), (unsigned)B), dim3(RA_THREADS), 0, st, (uint8_t*)img,
                       (const uint8_t*)scratch, (int)S, op);
    OP_LAUNCH_CHECK();
  }
  return OP_OK;
}

extern "C" int op_image_erase(void* x, int dtype, int64_t B, int64_t S, const int* box, const int* box_host, const float* noise,
                              const int64_t* noise_off, void* stream) {
  const char* what = "op_image_erase";
  OP_CHECK_ARG(dtype == OP_DT_BF16 || dtype == OP_DT_F32, "%s: dtype = %d, need 0 (bf16) or 1 (f32)", what, dtype);
  OP_CHECK_ARG(S >= 1 && S <= RA_ERASE_MAX_S, "%s: S = %lld, need 1 ... %d", what, (long long)S, RA_ERASE_MAX_S);
  OP_CHECK_ARG(B >= 0 && B <= 65535, "%s: B = %lld, need 0 ... 65535", what, (long long)B);
  if (B == 0) return OP_OK;
  OP_CHECK_ARG(x && box && box_host && noise_off, "%s: null pointer", what);
  OP_CHECK_ARG(((uintptr_t)x & (dtype == OP_DT_BF16 ? 1 : 3)) == 0 && ((uintptr_t)box & 3) == 0 && ((uintptr_t)box_host & 3) == 0 &&
                   ((uintptr_t)noise & 3) == 0 && ((uintptr_t)noise_off & 7) == 0,
               "%s: x, box, noise and noise_off must be aligned to their element size", what);
  int64_t most = 0;
  for (int64_t i = 0; i < B; ++i) {
    const int top = box_host[4 * i], left = box_host[4 * i + 1], h = box_host[4 * i + 2], w = box_host[4 * i + 3];
    if (h == 0) continue;
    OP_CHECK_ARG(h > 0 && w > 0 && top >= 0 && left >= 0 && (int64_t)top + h <= S && (int64_t)left + w <= S,
                 "%s: box %lld (top %d, left %d, h %d, w %d) is empty or outside the %lld x %lld image", what, (long long)i, top, left, h, w,
                 (long long)S, (long long)S);
    most = std::max<int64_t>(most, 3 * (int64_t)h * w);
  }
  if (most == 0) return OP_OK;
  OP_CHECK_ARG(noise, "%s: null pointer", what);
  const dim3 grid(ra_blocks(most, B), (unsigned)B);
  return op_with_bool(dtype == OP_DT_BF16, [&](auto bf) {
    using T = op_elem_t<decltype(bf)::value>;
    hipLaunchKernelGGL(ra_erase_kernel<T>, grid, dim3(RA_THREADS), 0, (hipStream_t)stream, (T*)x, (int)S, box, noise, noise_off);
    OP_LAUNCH_CHECK();
    return OP_OK;
  });
}
