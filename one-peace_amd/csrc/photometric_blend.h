// Image.blend of PIL for one byte: the one device function behind every ImageEnhance step (csrc/photometric.hip: brightness, contrast,
// saturation; csrc/randaugment.hip: sharpness).
#pragma once
#include "common.h"

// Image.blend(d, p, f) for one byte: fadd_rn(d, fmul_rn(f, p - d)).  Written as a plain product and sum under contract(off), as
// csrc/augment.hip does: __fmul_rn / __fadd_rn are inlined header functions whose * and + the compiler still contracts into an fma (it did:
// v_fma_f32 in the listing, and about 0.5 % of random bytes off PIL); the pragma binds only what is written here.
__device__ __forceinline__ int pm_blend(int d, int p, float f) {
#pragma clang fp contract(off)
  const float prod = f * (float)(p - d);
  const float t = (float)d + prod;
  return (int)fminf(fmaxf(t, 0.0f), 255.0f);
}
