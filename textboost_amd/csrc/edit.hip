// Image editing with a trained run (textboost_amd/edit.py, inference.py --init-image / --mask): the sampler step that keeps
// the unmasked part of an encoded photo on the schedule, and the paste of the decoded region back into the photo.
#include "common.h"
#include "dpm_step.h"
#include "../../include/textboost_hip.h"

namespace {

// `dpm_step_kernel` (elementwise.hip) plus the inpainting select, one launch per step.  blockIdx.y = image b, blockIdx.x * 256 + lane = element
// j of its n_per_b = C * hw latents (NCHW), so cell j % hw of the mask, which channels and images share:
//   x[b, j] <- mask[j % hw] ? (the step's x) : keep_a z0[j] + keep_s noise[b, j]      (the photo's latents at the NEXT step's noise level)
// m_prev gets the unblended data prediction, x2 = half(x) twice, as there.  With (keep_a, keep_s) = (1, 0) a kept element is z0 exactly.
__global__ __launch_bounds__(256) void dpm_step_blend_kernel(float* __restrict__ x, const f16* __restrict__ e, float* __restrict__ m_prev,
                                                             f16* __restrict__ x2, int64_t n_per_b, int B, float g, float alpha_t,
                                                             float sigma_t, float ca, float cb, float cc, const float* __restrict__ z0,
                                                             const float* __restrict__ noise, const uint8_t* __restrict__ mask, int hw,
                                                             float keep_a, float keep_s) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_per_b) return;
  const int64_t tot = n_per_b * B;
  const int64_t i = (int64_t)blockIdx.y * n_per_b + j;
  float m0, xn;
  dpm_update((float)e[i], (float)e[tot + i], x[i], m_prev[i], g, alpha_t, sigma_t, ca, cb, cc, m0, xn);
  m_prev[i] = m0;
  const float kept = keep_a * z0[j] + keep_s * noise[i];
  float xo = mask[j % hw] ? xn : kept;
  // x2 must be the rounding of the fp32 value that x holds (a kept latent is the photo's in both): behind this empty statement the compiler
  // cannot fold the conversion into the fma above (v_fma_mixlo_f16 rounds the exact fma once, which differs on ties)
  asm volatile("" : "+v"(xo));
  x[i] = xo;
  x2[i] = (f16)xo;
  x2[tot + i] = (f16)xo;
}

// dst[y][x] = mask[y][x] ? gen[y][x] : orig[y][x] on resident RGBX images (one uint32 per pixel), mask u8
__global__ __launch_bounds__(256) void img_paste_kernel(const uint32_t* __restrict__ gen, int64_t gstride, const uint32_t* __restrict__ orig,
                                                        int64_t ostride, const uint8_t* __restrict__ mask, int64_t mstride,
                                                        uint32_t* __restrict__ dst, int64_t dstride, int w, int h) {
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= w || y >= h) return;
  dst[y * dstride + x] = mask[y * mstride + x] ? gen[y * gstride + x] : orig[y * ostride + x];
}

}  // namespace

extern "C" int tb_dpm_step_blend(float* x, const void* eps2, float* m_prev, void* x2, int64_t n_per_b, int B, float guidance, float alpha_t,
                                 float sigma_t, float ca, float cb, float cc, const float* z0, const float* noise, const uint8_t* mask,
                                 int hw, float keep_a, float keep_s, tb_stream_t stream) {
  (void)hipGetLastError();  // drop any stale (non-sticky) error left by an earlier runtime call
  if (!x || !eps2 || !m_prev || !x2 || !z0 || !noise || !mask || n_per_b <= 0 || B <= 0 || B > 65535 || alpha_t == 0.f || hw <= 0 ||
      n_per_b % hw != 0)
    return TB_EINVAL;
  hipLaunchKernelGGL(dpm_step_blend_kernel, dim3((unsigned)((n_per_b + 255) / 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, x,
                     (const f16*)eps2, m_prev, (f16*)x2, n_per_b, B, guidance, alpha_t, sigma_t, ca, cb, cc, z0, noise, mask, hw, keep_a,
                     keep_s);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_img_paste(const uint32_t* gen, int64_t gstride, const uint32_t* orig, int64_t ostride, const uint8_t* mask, int64_t mstride,
                            uint32_t* dst, int64_t dstride, int w, int h, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!gen || !orig || !mask || !dst || w <= 0 || h <= 0 || gstride < w || ostride < w || mstride < w || dstride < w) return TB_EINVAL;
  hipLaunchKernelGGL(img_paste_kernel, dim3((w + 63) / 64, (h + 3) / 4), dim3(64, 4), 0, (hipStream_t)stream, gen, gstride, orig, ostride, mask,
                     mstride, dst, dstride, w, h);
  TB_CHECK_LAUNCH();
  return TB_OK;
}
