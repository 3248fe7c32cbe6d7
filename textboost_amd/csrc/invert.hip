// Editing a real photo by its prompt (inference.py --invert-image; `HipSampler.invert`, `HipSampler.denoise(pin=...)`): the walk
// from the photo's latents up the noise schedule (DDIM inversion with guidance), and the solver step that keeps the source rows -- and, under a
// mask, the kept cells of the edited rows -- on that walk while the rest is denoised beside them.  Both are elementwise on 64 KB per image;
// they exist so that inversion and the pinned step launch what text-to-image launches, with no host round trip.
#include "common.h"
#include "dpm_step.h"
#include "../../include/textboost_hip.h"

namespace {

// element i of x [B, n_per_b]:  eps = e_u + g (e_c - e_u) ;  xn = cx x + ce eps ;  x <- xn, x2 <- half(xn) twice, traj[i] <- xn (traj may be NULL)
__global__ __launch_bounds__(256) void invert_step_kernel(float* __restrict__ x, const f16* __restrict__ e, f16* __restrict__ x2,
                                                          float* __restrict__ traj, int64_t tot, float g, float cx, float ce) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= tot) return;
  const float eu = (float)e[i], ec = (float)e[tot + i];
  const float eps = eu + g * (ec - eu);
  float xn = cx * x[i] + ce * eps;
  // x2 must be the rounding of the fp32 value that x holds: see dpm_step_blend_kernel (edit.hip) on v_fma_mixlo_f16
  asm volatile("" : "+v"(xn));
  x[i] = xn;
  if (traj) traj[i] = xn;
  x2[i] = (f16)xn;
  x2[tot + i] = (f16)xn;
}

// `dpm_step_kernel` (elementwise.hip) through the shared `dpm_update`, then the select.  blockIdx.y = image b, blockIdx.x * 256 + lane = element j
// of its n_per_b = C * hw latents (NCHW), so cell j % hw of the mask, which channels and rows share:
//   b <  n_src:  x[b, j] <- pin[j]
//   b >= n_src:  x[b, j] <- (mask == NULL || mask[j % hw]) ? (the step's x) : pin[j]
// m_prev gets the row's own unpinned data prediction everywhere, x2 the 16-bit x twice (see below for which rounding).
__global__ __launch_bounds__(256) void dpm_step_pin_kernel(float* __restrict__ x, const f16* __restrict__ e, float* __restrict__ m_prev,
                                                           f16* __restrict__ x2, int64_t n_per_b, int B, float g, float alpha_t, float sigma_t,
                                                           float ca, float cb, float cc, const float* __restrict__ pin, int n_src,
                                                           const uint8_t* __restrict__ mask, int hw) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_per_b) return;
  const int b = blockIdx.y;
  const int64_t tot = n_per_b * B;
  const int64_t i = (int64_t)b * n_per_b + j;
  float m0, xn;
  dpm_update((float)e[i], (float)e[tot + i], x[i], m_prev[i], g, alpha_t, sigma_t, ca, cb, cc, m0, xn);
  m_prev[i] = m0;
  const bool step = b >= n_src && (mask == nullptr || mask[j % hw] != 0);
  // An unpinned element carries `dpm_step_kernel`'s bits in x2 as well, so that an unpinned row feeds the next UNet call what text-to-image
  // feeds it: the conversion of xn is written as there and left to the compiler as there (in the fp16 build it folds into the update's last
  // fma, v_fma_mixlo_f16: one rounding of the exact fma, which is half(x) except on ties of the double rounding).  A pinned element is
  // half(pin), the rounding of the fp32 value stored in x.
  // The empty statement keeps the compiler from moving the select in front of the conversion (convert(select) would round the stored fp32
  // value in every element and lose the fold).  tests/test_gpu_invert.py holds x2 against tb_dpm_step's bits in both builds.
  const float p = pin[j];
  f16 hs = (f16)xn;
  asm volatile("" : "+v"(hs));
  const f16 h = step ? hs : (f16)p;
  x[i] = step ? xn : p;
  x2[i] = h;
  x2[tot + i] = h;
}

}  // namespace

extern "C" int tb_invert_step(float* x, const void* eps2, void* x2, float* traj_out, int64_t n_per_b, int B, float guidance, float cx, float ce,
                              tb_stream_t stream) {
  (void)hipGetLastError();  // drop any stale (non-sticky) error left by an earlier runtime call
  if (!x || !eps2 || !x2 || n_per_b <= 0 || B <= 0 || B > 65535) return TB_EINVAL;
  const int64_t tot = n_per_b * B;
  hipLaunchKernelGGL(invert_step_kernel, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, (const f16*)eps2, (f16*)x2, traj_out, tot, guidance,
                     cx, ce);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_dpm_step_pin(float* x, const void* eps2, float* m_prev, void* x2, int64_t n_per_b, int B, float guidance, float alpha_t,
                               float sigma_t, float ca, float cb, float cc, const float* pin, int n_src, const uint8_t* mask, int hw,
                               tb_stream_t stream) {
  (void)hipGetLastError();
  if (!x || !eps2 || !m_prev || !x2 || !pin || n_per_b <= 0 || B <= 0 || B > 65535 || alpha_t == 0.f || n_src < 0 || n_src > B || hw <= 0 ||
      n_per_b % hw != 0)
    return TB_EINVAL;
  hipLaunchKernelGGL(dpm_step_pin_kernel, dim3((unsigned)((n_per_b + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, x,
                     (const f16*)eps2, m_prev, (f16*)x2, n_per_b, B, guidance, alpha_t, sigma_t, ca, cb, cc, pin, n_src, mask, hw);
  TB_CHECK_LAUNCH();
  return TB_OK;
}
