// Batch augmentation of the image-classification fine-tune (include/onepeace_hip.h: op_mix_images).  Replaces the full-batch torch passes of
// timm's Mixup / CutMix as the reference uses them (data/vision_data/image_classify_dataset.py:46-51, 117-130): x.mul_(lam).add_(x.flip(0)
// .mul_(1 - lam)) for Mixup, x[:, :, yl:yh, xl:xh] = x.flip(0)[:, :, yl:yh, xl:xh] for CutMix, per batch, per element or per pair.
//
// mix_images_kernel: sample i is mixed with its partner j = B - 1 - i, both read from the ORIGINAL batch.  blockIdx.y = the pair (i, j),
// i <= j; a work item owns the same 8 elements (16 bytes of bf16, two 16-byte vectors of fp32) of sample i and of sample j: it reads both,
// then writes both, so the launch may run in place without a clone and without any order between workgroups.  The middle sample of an odd
// batch is its own partner: read once, mixed with itself.  W % 8 == 0 keeps the 8 elements inside one image row, so the CutMix test is one
// row compare and 8 column compares.  One read and one write of the batch; the per-sample tables are uniform (scalar) loads.
// Mixup is fadd_rn(fmul_rn(x_i, lam), fmul_rn(x_j, 1 - lam)): two rounded fp32 products and one rounded sum, torch's statement bit for bit --
// the contraction into an fma is switched off for this file's arithmetic, an fma differs on about 38 % of random elements.
#include "common.h"

#include <algorithm>

namespace {

constexpr int MIX_THREADS = 256;
constexpr int MIX_BLOCKS = 4096;  // launch cap (guideline: ~2048 ... 4096 workgroups for a streaming pass); grid-stride behind it

struct MixRow { int kind; float lam, oml; int yl, yh, xl, xh; };

__device__ __forceinline__ MixRow mix_row(const int* kind, const float* lam, const float* oml, const int* box, int64_t s) {
  return {kind[s], lam[s], oml[s], box[4 * s], box[4 * s + 1], box[4 * s + 2], box[4 * s + 3]};
}

// the 8 output elements of the sample `r` describes: a = its own elements, b = its partner's; (y, x0) = row and first column of the 8
__device__ __forceinline__ void mix8(const MixRow& r, const float (&a)[8], const float (&b)[8], int y, int x0, float (&o)[8]) {
#pragma clang fp contract(off)
  if (r.kind == 1) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const float pa = a[k] * r.lam, pb = b[k] * r.oml;
      o[k] = pa + pb;
    }
  } else if (r.kind == 2) {
    const bool row_in = y >= r.yl && y < r.yh;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = (row_in && x0 + k >= r.xl && x0 + k < r.xh) ? b[k] : a[k];
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = a[k];
  }
}

// x and out may be the same buffer (TI == TO): no __restrict__, every load of a work item precedes its stores
template <typename TI, typename TO>
__global__ __launch_bounds__(MIX_THREADS) void mix_images_kernel(const TI* x, TO* out, int64_t B, int64_t CHW, int H, int W, const int* kind,
                                                                 const float* lam, const float* oml, const int* box) {
  const int64_t i = blockIdx.y, j = B - 1 - i;
  const MixRow ri = mix_row(kind, lam, oml, box, i), rj = mix_row(kind, lam, oml, box, j);
  const int64_t nvec = CHW / 8;
  for (int64_t v = (int64_t)blockIdx.x * MIX_THREADS + threadIdx.x; v < nvec; v += (int64_t)gridDim.x * MIX_THREADS) {
    const int64_t e = v * 8;
    const unsigned e32 = (unsigned)e;  // CHW < 2^31: 32-bit divisions
    const int x0 = (int)(e32 % (unsigned)W), y = (int)((e32 / (unsigned)W) % (unsigned)H);
    float a[8], b[8], oi[8], oj[8];
    if (i == j) {
      Vec8<TI>::load(x + i * CHW + e, a);
      mix8(ri, a, a, y, x0, oi);
      Vec8<TO>::store(out + i * CHW + e, oi);
    } else {
      const typename Vec8<TI>::raw_t va = Vec8<TI>::ldraw(x + i * CHW + e), vb = Vec8<TI>::ldraw(x + j * CHW + e);
      Vec8<TI>::cvt(va, a);
      Vec8<TI>::cvt(vb, b);
      mix8(ri, a, b, y, x0, oi);
      mix8(rj, b, a, y, x0, oj);
      Vec8<TO>::store(out + i * CHW + e, oi);
      Vec8<TO>::store(out + j * CHW + e, oj);
    }
  }
}

}  // namespace

extern "C" int op_mix_images(const void* x, void* out, int in_dtype, int out_dtype, int64_t B, int64_t CHW, int64_t H, int64_t W,
                             const int* kind, const float* lam, const float* one_minus_lam, const int* box, void* stream) {
  OP_CHECK_ARG((in_dtype == OP_DT_BF16 || in_dtype == OP_DT_F32) && (out_dtype == OP_DT_BF16 || out_dtype == OP_DT_F32),
               "op_mix_images: in_dtype = %d, out_dtype = %d, need 0 (bf16) or 1 (f32)", in_dtype, out_dtype);
  OP_CHECK_ARG(B >= 0 && B <= 2 * 65535, "op_mix_images: B = %lld, need 0 ... %d", (long long)B, 2 * 65535);
  OP_CHECK_ARG(H >= 1 && W >= 1 && H < (int64_t(1) << 30) && W < (int64_t(1) << 30) && CHW >= H * W && CHW % (H * W) == 0 &&
                   CHW < (int64_t(1) << 31),
               "op_mix_images: CHW = %lld is not a positive multiple of H x W = %lld x %lld below 2^31", (long long)CHW, (long long)H,
               (long long)W);
  if (B == 0) return OP_OK;
  OP_CHECK_ARG(x && out && kind && lam && one_minus_lam && box, "op_mix_images: null pointer");
  OP_CHECK_ARG(((uintptr_t)kind & 3) == 0 && ((uintptr_t)lam & 3) == 0 && ((uintptr_t)one_minus_lam & 3) == 0 && ((uintptr_t)box & 3) == 0,
               "op_mix_images: kind, lam, one_minus_lam and box must be 4-byte aligned");
  const int64_t in_bytes = B * CHW * (in_dtype == OP_DT_BF16 ? 2 : 4), out_bytes = B * CHW * (out_dtype == OP_DT_BF16 ? 2 : 4);
  const uintptr_t xa = (uintptr_t)x, oa = (uintptr_t)out;
  OP_CHECK_ARG((xa == oa && in_dtype == out_dtype) || xa + in_bytes <= oa || oa + out_bytes <= xa,
               "op_mix_images: out must be x itself (with the same dtype) or must not overlap it");
  if (W % 8 != 0 || CHW % 8 != 0 || (xa & 15) != 0 || (oa & 15) != 0) {
    op_set_error("op_mix_images: W = %lld and CHW = %lld must be multiples of 8 and x, out 16-byte aligned (not supported)", (long long)W,
                 (long long)CHW);
    return OP_ENOTSUP;
  }
  const int64_t pairs = (B + 1) / 2, blocks = (CHW / 8 + MIX_THREADS - 1) / MIX_THREADS;
  const dim3 grid((unsigned)std::min<int64_t>(blocks, std::max<int64_t>(1, MIX_BLOCKS / pairs)), (unsigned)pairs);
  return op_with_bool(in_dtype == OP_DT_BF16, [&](auto ib) {
    return op_with_bool(out_dtype == OP_DT_BF16, [&](auto ob) {
      using TI = op_elem_t<decltype(ib)::value>;
      using TO = op_elem_t<decltype(ob)::value>;
      hipLaunchKernelGGL((mix_images_kernel<TI, TO>), grid, dim3(MIX_THREADS), 0, (hipStream_t)stream, (const TI*)x, (TO*)out, B, CHW,
                         (int)H, (int)W, kind, lam, one_minus_lam, box);
      OP_LAUNCH_CHECK();
      return OP_OK;
    });
  });
}
