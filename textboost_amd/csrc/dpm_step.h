// The arithmetic of one guided DPM-Solver++(2M) update on one latent element, shared by `dpm_step_kernel` (elementwise.hip: text-to-image)
// and `dpm_step_blend_kernel` (edit.hip: image editing) so that both produce the same bits:
//   eps = e_u + g (e_c - e_u) ;  m0 = (x - sigma_t eps) / alpha_t ;  xn = ca x + cb m0 + cc m_prev
#pragma once
#include "common.h"

__device__ __forceinline__ void dpm_update(float eu, float ec, float xv, float mp, float g, float alpha_t, float sigma_t, float ca, float cb,
                                           float cc, float& m0, float& xn) {
  const float eps = eu + g * (ec - eu);
  m0 = (xv - sigma_t * eps) / alpha_t;
  xn = ca * xv + cb * m0 + cc * mp;
}
