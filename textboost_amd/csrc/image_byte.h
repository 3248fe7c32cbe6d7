// The byte rule of a decoded image, shared by `vae_image_rgbx_kernel` (elementwise.hip) and `tile_blend_kernel` (canvas.hip) so that a
// one-tile canvas has the bytes of `decode_rgbx`.  Per channel uint8(rint(clamp(x / 2 + 0.5, 0, 1) * 255)): x / 2 is exact, so the fma rounds once
// like the two torch ops; the product with 255 is rounded on its own before rint (half-way cases would flip otherwise); NaN -> 0.
#pragma once
#include "common.h"

__device__ __forceinline__ uint32_t image_byte(float x) {
  const float v = fmaf(x, 0.5f, 0.5f);
  const float c = v > 0.f ? fminf(v, 1.f) : 0.f;   // NaN compares false
  return (uint32_t)rintf(__fmul_rn(c, 255.f));
}
