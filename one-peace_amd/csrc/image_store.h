// The store of the image kernels (csrc/image.hip: ir_vertical_kernel; csrc/photometric.hip: pm_normalize_flip_kernel): RandomHorizontalFlip,
// ToTensor / Normalize in torchvision's fp32 order and the cast, for one group of 4 adjacent pixels.  ONE definition, so that the resize
// route and the photometric route (resize to uint8, jitter, blur, then this) cannot drift apart.
#pragma once
#include "common.h"

constexpr int IR_OUT_U8 = 2;  // out_dtype of the image entries besides OP_DT_BF16 / OP_DT_F32: the uint8 HWC pixels themselves

struct IrNorm { float mean[3], stdev[3]; };

// u[x][ch]: the 4 pixels of column group g (columns 4 g ... 4 g + 3) of row y of image img, G = S / 4 groups per row.  OUT = OP_DT_BF16 /
// OP_DT_F32: out [B, 3, S, S], (u / 255 - mean) / stdev with IEEE divisions, bf16 by round-to-nearest-even (torch's .to(bfloat16));
// OUT = IR_OUT_U8: out uint8 [B, S, S, 3], the pixels themselves.
template <int OUT>
__device__ __forceinline__ void ir_store_group(void* __restrict__ out, int (&u)[4][3], int64_t img, int y, int g, int G, int S,
                                               const IrNorm& nm, bool flipped) {
  // a flipped image writes column S - 1 - x: the 4-column group goes to group G - 1 - g with its columns reversed (same vector stores)
  const int go = flipped ? G - 1 - g : g;
  if (flipped) {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      const int a = u[0][ch], b = u[1][ch];
      u[0][ch] = u[3][ch], u[1][ch] = u[2][ch], u[2][ch] = b, u[3][ch] = a;
    }
  }
  if constexpr (OUT == IR_OUT_U8) {
    unsigned* q = reinterpret_cast<unsigned*>(reinterpret_cast<uint8_t*>(out) + ((img * S + y) * S + go * 4) * 3);
    q[0] = (unsigned)u[0][0] | (unsigned)u[0][1] << 8 | (unsigned)u[0][2] << 16 | (unsigned)u[1][0] << 24;
    q[1] = (unsigned)u[1][1] | (unsigned)u[1][2] << 8 | (unsigned)u[2][0] << 16 | (unsigned)u[2][1] << 24;
    q[2] = (unsigned)u[2][2] | (unsigned)u[3][0] << 8 | (unsigned)u[3][1] << 16 | (unsigned)u[3][2] << 24;
  } else {
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      float v[4];
#pragma unroll
      for (int x = 0; x < 4; ++x) v[x] = ((float)u[x][ch] / 255.0f - nm.mean[ch]) / nm.stdev[ch];  // torchvision's order, IEEE
      const int64_t e = ((img * 3 + ch) * S + y) * S + go * 4;
      if constexpr (OUT == OP_DT_BF16) {
        bf16x4 r;
#pragma unroll
        for (int x = 0; x < 4; ++x) r[x] = (bf16_t)v[x];
        *reinterpret_cast<bf16x4*>(reinterpret_cast<bf16_t*>(out) + e) = r;
      } else {
        *reinterpret_cast<f32x4*>(reinterpret_cast<float*>(out) + e) = (f32x4){v[0], v[1], v[2], v[3]};
      }
    }
  }
}
