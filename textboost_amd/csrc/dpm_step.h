// The arithmetic of one guided DPM-Solver++(2M) update on one latent element, shared by `dpm_step_kernel` (elementwise.hip: text-to-image),
// `dpm_step_blend_kernel` (edit.hip: image editing) and `canvas_step_kernel` (canvas.hip: the MultiDiffusion canvas) so that all produce
// the same bits:
//   eps = e_u + g (e_c - e_u) ;  m0 = (x - sigma_t eps) / alpha_t ;  xn = ca x + cb m0 + cc m_prev
// in two halves, because the canvas averages the guided eps of its windows before it takes the one update.
//
// Every multiply-add is spelled out.  Left to the compiler, which products fuse depends on the code around the expression (the canvas kernel
// got ca x + fma(cb, m0, cc m_prev) where the step kernels get fma(cc, m_prev, fma(ca, x, cb m0))), and the kernels would disagree in the last
// bit.  The spelling is the one the step kernels have always compiled to, so their results do not change.
#pragma once
#include "common.h"

__device__ __forceinline__ float guided_eps(float eu, float ec, float g) { return fmaf(g, ec - eu, eu); }

__device__ __forceinline__ void dpm_update_eps(float eps, float xv, float mp, float alpha_t, float sigma_t, float ca, float cb, float cc,
                                               float& m0, float& xn) {
  m0 = fmaf(-sigma_t, eps, xv) / alpha_t;
  xn = fmaf(cc, mp, fmaf(ca, xv, __fmul_rn(cb, m0)));
}

__device__ __forceinline__ void dpm_update(float eu, float ec, float xv, float mp, float g, float alpha_t, float sigma_t, float ca, float cb,
                                           float cc, float& m0, float& xn) {
  dpm_update_eps(guided_eps(eu, ec, g), xv, mp, alpha_t, sigma_t, ca, cb, cc, m0, xn);
}
