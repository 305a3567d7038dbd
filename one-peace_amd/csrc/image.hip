// Image pre-processing of the hub (include/onepeace_hip.h: op_image_resize_normalize).  Replaces the host transform of
// one_peace/models/one_peace/hub_interface.py:94-101 -- Resize((S, S), BICUBIC) on a PIL RGB image, ToTensor, Normalize with the CLIP
// mean / std of data/base_dataset.py:23-24 -- for a batch of decoded uint8 images of different sizes, bit for bit.
//
// The resize is Pillow's Image.resize for 8-bit images (src/libImaging/Resample.c): 22-bit fixed-point filter weights built on the
// host (one-peace_amd/imageprep.py: bicubic_coeffs), a horizontal pass over only the source rows the vertical filter reads into a uint8
// intermediate (clip8((acc + 2^21) >> 22)), then the vertical pass in the same rounding.  Integer accumulation: the result does not
// depend on the launch shape.
//
// ir_horizontal_kernel: workgroup = (image, tile of IR_ROWS_H intermediate rows); work item = (output column, 4 rows), so one load of
// the column's weights serves four rows.  Per 4 taps a lane reads the 12 source bytes of 4 RGB pixels as 4 dwords from the dword
// boundary below them and splits them with v_alignbyte; the window may reach 13 bytes past the image, hence the 16-byte slack the
// caller keeps behind the last image.
// ir_vertical_kernel: workgroup = (image, tile of IR_ROWS_V output rows); work item = (output row, 4 columns): per tap 12 bytes (3
// aligned dwords) of the intermediate, then ToTensor / Normalize in torchvision's fp32 order ((u / 255 - mean) / std, IEEE divisions)
// and the cast (bf16 by round-to-nearest-even, as torch's .to(bfloat16)), or the uint8 HWC pixels themselves.
// PIL runs the vertical pass first for an image more than 100 times taller than wide that shrinks vertically (vfirst = 1; PIL/Image.py,
// resize).  Such an image is narrow: its first pass filters the source columns into an [S, W, 3] intermediate and its second the
// intermediate's rows, both with plain byte loads (the `vfirst` branches of the two kernels).
// The training / evaluation geometry needs no arithmetic of its own (op_image_resize_normalize_flip): RandomResizedCrop
// (data/pretrain_data/image_text_pretrain_dataset.py:46-53) and Resize + CenterCrop (data/vision_data/image_classify_dataset.py:78-84) are
// shifted / windowed coefficient records built on the host, and RandomHorizontalFlip (image_classify_dataset.py:59, nlvr2_dataset.py:37) is a
// per-image flag under which the vertical kernel stores its 4-column group mirrored.
#include "common.h"
#include "image_store.h"

#include <algorithm>

namespace {

constexpr int IR_THREADS = 256;
constexpr int IR_ROWS_H = 16;  // intermediate rows per workgroup, horizontal pass (work items of 4 rows)
constexpr int IR_ROWS_V = 16;  // output rows per workgroup, vertical pass (S is a multiple of 16)
constexpr int IR_DESC = 11;    // int64 per image: src_off, H, W, cx_off, kx, cy_off, ky, tmp_off, row0, rows, vfirst
constexpr int IR_PREC = 22;
constexpr int IR_MAX_S = 1024;
constexpr int IR_SLACK = 16;

__device__ __forceinline__ int ir_clip8(int acc) { return min(max(acc >> IR_PREC, 0), 255); }

// the 12 bytes at `byte` (any alignment) as 3 dwords, from the 4 dwords starting at the dword boundary below it
__device__ __forceinline__ void ir_load12(const uint8_t* base, int64_t byte, unsigned& d0, unsigned& d1, unsigned& d2) {
  const unsigned* p = reinterpret_cast<const unsigned*>(base + (byte & ~int64_t(3)));
  const unsigned sh = (unsigned)(byte & 3);
  const unsigned u0 = p[0], u1 = p[1], u2 = p[2], u3 = p[3];
  d0 = __builtin_amdgcn_alignbyte(u1, u0, sh);
  d1 = __builtin_amdgcn_alignbyte(u2, u1, sh);
  d2 = __builtin_amdgcn_alignbyte(u3, u2, sh);
}

// pixel x weight on the 24-bit multiplier (full rate; v_mul_lo_u32 is quarter rate): |w| <= 2^22 + 1 and pixels <= 255 fit it
__device__ __forceinline__ int ir_mul(unsigned px, int w) { return __mul24((int)px, w); }

// acc[c] += w[j] * channel c of pixel j, for the 4 RGB pixels packed in d0..d2
__device__ __forceinline__ void ir_mac4(int (&acc)[3], unsigned d0, unsigned d1, unsigned d2, const int (&w)[4]) {
  acc[0] += ir_mul(d0 & 255, w[0]) + ir_mul(d0 >> 24, w[1]) + ir_mul((d1 >> 16) & 255, w[2]) + ir_mul((d2 >> 8) & 255, w[3]);
  acc[1] += ir_mul((d0 >> 8) & 255, w[0]) + ir_mul(d1 & 255, w[1]) + ir_mul(d1 >> 24, w[2]) + ir_mul((d2 >> 16) & 255, w[3]);
  acc[2] += ir_mul((d0 >> 16) & 255, w[0]) + ir_mul((d1 >> 8) & 255, w[1]) + ir_mul(d2 & 255, w[2]) + ir_mul(d2 >> 24, w[3]);
}

__global__ __launch_bounds__(IR_THREADS) void ir_horizontal_kernel(const uint8_t* __restrict__ src, const int64_t* __restrict__ desc,
                                                                   const int* __restrict__ coef, uint8_t* __restrict__ tmp, int S) {
  const int64_t* d = desc + (int64_t)blockIdx.y * IR_DESC;
  const int64_t src_off = d[0], H = d[1], W = d[2], cx_off = d[3], tmp_off = d[7], row0 = d[8], rows = d[9];
  const int kx = (int)d[4];
  const int64_t r_begin = (int64_t)blockIdx.x * IR_ROWS_H;
  if (r_begin >= rows) return;
  const int nr = (int)min((int64_t)IR_ROWS_H, rows - r_begin);
  if (d[10]) {  // vertical pass first: intermediate rows r_begin ... of the S output rows, all W columns
    const int64_t cy_off = d[5];
    const int ky = (int)d[6];
    for (int64_t it = threadIdx.x; it < W * nr; it += IR_THREADS) {
      const int64_t x = it % W, r = r_begin + it / W;
      const int* c = coef + cy_off + r * (4 + ky);
      const int64_t ymin = min(max((int64_t)c[0], int64_t(0)), H - 1);
      const int n = (int)min(max((int64_t)c[1], int64_t(0)), min((int64_t)ky, H - ymin));
      int acc[3] = {1 << (IR_PREC - 1), 1 << (IR_PREC - 1), 1 << (IR_PREC - 1)};
      for (int t = 0; t < n; ++t) {
        const uint8_t* q = src + src_off + ((ymin + t) * W + x) * 3;
        const int w = c[4 + t];
        acc[0] += ir_mul(q[0], w);
        acc[1] += ir_mul(q[1], w);
        acc[2] += ir_mul(q[2], w);
      }
      uint8_t* q = tmp + tmp_off + (r * W + x) * 3;
      q[0] = (uint8_t)ir_clip8(acc[0]);
      q[1] = (uint8_t)ir_clip8(acc[1]);
      q[2] = (uint8_t)ir_clip8(acc[2]);
    }
    return;
  }
  for (int it = threadIdx.x; it < S * (IR_ROWS_H / 4); it += IR_THREADS) {
    const int o = it % S, r_first = (it / S) * 4;
    if (r_first >= nr) break;  // items of later row groups are further along
    const int* c = coef + cx_off + (int64_t)o * (4 + kx);
    const int xmin = (int)min(max((int64_t)c[0], int64_t(0)), W - 1);
    const int n = (int)min(max((int64_t)c[1], int64_t(0)), min((int64_t)kx, W - xmin));
    int64_t base[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {  // rows past the tile re-read its last row; their results are not stored
      const int64_t sr = min(row0 + r_begin + min(r_first + j, nr - 1), H - 1);
      base[j] = src_off + (sr * W + xmin) * 3;
    }
    int acc[4][3];
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << (IR_PREC - 1);
    for (int t = 0; t < n; t += 4) {
      const int4 w4 = *reinterpret_cast<const int4*>(c + 4 + t);
      const int w[4] = {w4.x, t + 1 < n ? w4.y : 0, t + 2 < n ? w4.z : 0, t + 3 < n ? w4.w : 0};
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        unsigned d0, d1, d2;
        ir_load12(src, base[j] + 3 * t, d0, d1, d2);
        ir_mac4(acc[j], d0, d1, d2, w);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (r_first + j < nr) {
        uint8_t* q = tmp + tmp_off + ((r_begin + r_first + j) * S + o) * 3;
        q[0] = (uint8_t)ir_clip8(acc[j][0]);
        q[1] = (uint8_t)ir_clip8(acc[j][1]);
        q[2] = (uint8_t)ir_clip8(acc[j][2]);
      }
    }
  }
}

template <int OUT>
__global__ __launch_bounds__(IR_THREADS) void ir_vertical_kernel(const uint8_t* __restrict__ tmp, const int64_t* __restrict__ desc,
                                                                 const int* __restrict__ coef, void* __restrict__ out, int S, IrNorm nm,
                                                                 const uint8_t* __restrict__ flip) {
  const int img = blockIdx.y;
  const int64_t* d = desc + (int64_t)img * IR_DESC;
  const int64_t W = d[2], cx_off = d[3], cy_off = d[5], tmp_off = d[7], row0 = d[8], rows = d[9];
  const int kx = (int)d[4], ky = (int)d[6];
  const bool vfirst = d[10] != 0;
  const bool flipped = flip != nullptr && flip[img] != 0;  // uniform: RandomHorizontalFlip of this image
  const int G = S / 4;
  for (int it = threadIdx.x; it < G * IR_ROWS_V; it += IR_THREADS) {
    const int g = it % G, y = blockIdx.x * IR_ROWS_V + it / G;
    int u[4][3];
    if (vfirst) {  // horizontal pass over row y of the [S, W, 3] intermediate
#pragma unroll
      for (int x = 0; x < 4; ++x) {
        const int* c = coef + cx_off + (int64_t)(g * 4 + x) * (4 + kx);
        const int64_t xmin = min(max((int64_t)c[0], int64_t(0)), W - 1);
        const int n = (int)min(max((int64_t)c[1], int64_t(0)), min((int64_t)kx, W - xmin));
        int acc[3] = {1 << (IR_PREC - 1), 1 << (IR_PREC - 1), 1 << (IR_PREC - 1)};
        for (int t = 0; t < n; ++t) {
          const uint8_t* q = tmp + tmp_off + ((int64_t)y * W + xmin + t) * 3;
          const int w = c[4 + t];
          acc[0] += ir_mul(q[0], w);
          acc[1] += ir_mul(q[1], w);
          acc[2] += ir_mul(q[2], w);
        }
        u[x][0] = ir_clip8(acc[0]);
        u[x][1] = ir_clip8(acc[1]);
        u[x][2] = ir_clip8(acc[2]);
      }
    } else {
      const int* c = coef + cy_off + (int64_t)y * (4 + ky);
      const int64_t ymin = min(max((int64_t)c[0] - row0, int64_t(0)), rows - 1);
      const int n = (int)min(max((int64_t)c[1], int64_t(0)), min((int64_t)ky, rows - ymin));
      const uint8_t* p = tmp + tmp_off + (ymin * S + g * 4) * 3;
      int acc[4][3];
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 1 << (IR_PREC - 1);
      for (int t = 0; t < n; t += 4) {
        const int4 w4 = *reinterpret_cast<const int4*>(c + 4 + t);
        const int w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          if (t + j < n) {
            const unsigned* q = reinterpret_cast<const unsigned*>(p + (int64_t)(t + j) * S * 3);
            const unsigned d0 = q[0], d1 = q[1], d2 = q[2];
            const unsigned px[4][3] = {{d0 & 255, (d0 >> 8) & 255, (d0 >> 16) & 255}, {d0 >> 24, d1 & 255, (d1 >> 8) & 255},
                                       {(d1 >> 16) & 255, d1 >> 24, d2 & 255}, {(d2 >> 8) & 255, (d2 >> 16) & 255, d2 >> 24}};
#pragma unroll
            for (int x = 0; x < 4; ++x)
#pragma unroll
              for (int ch = 0; ch < 3; ++ch) acc[x][ch] += ir_mul(px[x][ch], w[j]);
          }
        }
      }
#pragma unroll
      for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) u[x][ch] = ir_clip8(acc[x][ch]);
      }
    ir_store_group<OUT>(out, u, img, y, g, G, S, nm, flipped);
  }
}

}  // namespace

// op_image_resize_normalize plus RandomHorizontalFlip (image_classify_dataset.py:59, nlvr2_dataset.py:37): flip = device uint8 [B], non-zero =
// this image's columns are stored mirrored; NULL = no image is.  Crops and centre crops need nothing here: they are tables (imageprep.py).
// Additive: op_abi_version() stays 10.
extern "C" int op_image_resize_normalize_flip(const void* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int64_t B,
                                              const int* coef, int64_t coef_count, int64_t S, const float* mean, const float* stdev,
                                              void* out, int out_dtype, void* workspace, int64_t workspace_bytes, const uint8_t* flip,
                                              void* stream) {
  OP_CHECK_ARG(S >= 16 && S <= IR_MAX_S && S % 16 == 0, "op_image_resize_normalize: S = %lld, need a multiple of 16 in [16, %d]",
               (long long)S, IR_MAX_S);
  OP_CHECK_ARG(B >= 0 && B <= 65535, "op_image_resize_normalize: B = %lld, need 0 ... 65535", (long long)B);
  OP_CHECK_ARG(out_dtype == OP_DT_BF16 || out_dtype == OP_DT_F32 || out_dtype == IR_OUT_U8,
               "op_image_resize_normalize: out_dtype = %d, need 0 (bf16), 1 (f32) or 2 (uint8 HWC)", out_dtype);
  OP_CHECK_ARG(out_dtype == IR_OUT_U8 || (mean && stdev), "op_image_resize_normalize: mean / stdev (host float[3]) are required");
  if (B == 0) return OP_OK;
  OP_CHECK_ARG(src && desc && desc_host && coef && out && workspace, "op_image_resize_normalize: null pointer");
  OP_CHECK_ARG(((uintptr_t)src & 15) == 0 && ((uintptr_t)coef & 15) == 0 && ((uintptr_t)out & 15) == 0 &&
                   ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)desc & 7) == 0,
               "op_image_resize_normalize: src, coef, out and workspace must be 16-byte aligned, desc 8-byte aligned");
  int64_t max_tiles = 0;
  for (int64_t i = 0; i < B; ++i) {
    const int64_t* d = desc_host + i * IR_DESC;
    const int64_t src_off = d[0], H = d[1], W = d[2], cx_off = d[3], kx = d[4], cy_off = d[5], ky = d[6], tmp_off = d[7], row0 = d[8],
                  rows = d[9], vfirst = d[10];
    OP_CHECK_ARG(H >= 1 && W >= 1 && H < (int64_t(1) << 30) && W < (int64_t(1) << 30) && H * W < (int64_t(1) << 40),
                 "op_image_resize_normalize: image %lld is %lld x %lld, need H, W >= 1", (long long)i, (long long)H, (long long)W);
    OP_CHECK_ARG(src_off >= 0 && src_off + 3 * H * W + IR_SLACK <= src_bytes,
                 "op_image_resize_normalize: image %lld (offset %lld, %lld x %lld) and %d readable bytes behind it overrun src (%lld bytes)",
                 (long long)i, (long long)src_off, (long long)H, (long long)W, IR_SLACK, (long long)src_bytes);
    OP_CHECK_ARG(kx >= 4 && ky >= 4 && kx % 4 == 0 && ky % 4 == 0 && kx < (1 << 24) && ky < (1 << 24),
                 "op_image_resize_normalize: image %lld: weights per record %lld / %lld, need multiples of 4", (long long)i,
                 (long long)kx, (long long)ky);
    OP_CHECK_ARG(cx_off >= 0 && cy_off >= 0 && cx_off % 4 == 0 && cy_off % 4 == 0 && cx_off + S * (4 + kx) <= coef_count &&
                     cy_off + S * (4 + ky) <= coef_count,
                 "op_image_resize_normalize: image %lld: coefficient records at %lld / %lld (multiples of 4) overrun coef (%lld ints)",
                 (long long)i, (long long)cx_off, (long long)cy_off, (long long)coef_count);
    OP_CHECK_ARG(vfirst == 0 || vfirst == 1, "op_image_resize_normalize: image %lld: vfirst = %lld", (long long)i, (long long)vfirst);
    OP_CHECK_ARG(vfirst ? (row0 == 0 && rows == S) : (row0 >= 0 && rows >= 1 && row0 + rows <= H),
                 "op_image_resize_normalize: image %lld: rows %lld + %lld outside 0 ... %lld (vertical pass first: 0 + S)", (long long)i,
                 (long long)row0, (long long)rows, (long long)H);
    const int64_t tmp_bytes = rows * (vfirst ? W : S) * 3;
    OP_CHECK_ARG(tmp_off >= 0 && tmp_off % 16 == 0 && tmp_off + tmp_bytes <= workspace_bytes,
                 "op_image_resize_normalize: image %lld: intermediate at %lld (16-aligned) of %lld bytes overruns the workspace (%lld)",
                 (long long)i, (long long)tmp_off, (long long)tmp_bytes, (long long)workspace_bytes);
    max_tiles = std::max(max_tiles, (rows + IR_ROWS_H - 1) / IR_ROWS_H);
  }
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(ir_horizontal_kernel, dim3((unsigned)max_tiles, (unsigned)B), dim3(IR_THREADS), 0, st, (const uint8_t*)src, desc,
                     coef, (uint8_t*)workspace, (int)S);
  OP_LAUNCH_CHECK();
  IrNorm nm = {};
  if (out_dtype != IR_OUT_U8)
    for (int c = 0; c < 3; ++c) nm.mean[c] = mean[c], nm.stdev[c] = stdev[c];
  const dim3 grid((unsigned)(S / IR_ROWS_V), (unsigned)B);
  const uint8_t* t = (const uint8_t*)workspace;
  if (out_dtype == OP_DT_BF16)
    hipLaunchKernelGGL(ir_vertical_kernel<OP_DT_BF16>, grid, dim3(IR_THREADS), 0, st, t, desc, coef, out, (int)S, nm, flip);
  else if (out_dtype == OP_DT_F32)
    hipLaunchKernelGGL(ir_vertical_kernel<OP_DT_F32>, grid, dim3(IR_THREADS), 0, st, t, desc, coef, out, (int)S, nm, flip);
  else
    hipLaunchKernelGGL(ir_vertical_kernel<IR_OUT_U8>, grid, dim3(IR_THREADS), 0, st, t, desc, coef, out, (int)S, nm, flip);
  OP_LAUNCH_CHECK();
  return OP_OK;
}

extern "C" int op_image_resize_normalize(const void* src, int64_t src_bytes, const int64_t* desc, const int64_t* desc_host, int64_t B,
                                         const int* coef, int64_t coef_count, int64_t S, const float* mean, const float* stdev,
                                         void* out, int out_dtype, void* workspace, int64_t workspace_bytes, void* stream) {
  return op_image_resize_normalize_flip(src, src_bytes, desc, desc_host, B, coef, coef_count, S, mean, stdev, out, out_dtype, workspace,
                                        workspace_bytes, nullptr, stream);
}
