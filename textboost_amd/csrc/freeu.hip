// FreeU (inference.py --freeu; HipUNet.enable_freeu): in front of the resnets of the first two decoder stages the hidden half
// of the concat input is amplified and the lowest spatial frequencies of the skip half are damped, in place on the concat buffer.
//
// The skip filter is diffusers' fourier_filter(x, threshold = 1, scale = s): it scales the frequencies {0, -1} x {0, -1} of every
// (image, channel) plane.  That is at most 7 real moments per plane (the sum, and a cosine and a sine moment of three frequencies), so no FFT
// is run: one workgroup owns (image, 64 channels), sums the moments and then corrects its own elements.  NHWC rows are channel-contiguous,
// so the 64 lanes of a wave run along the channels (one 128-byte row segment per load) and the four waves take the pixels p = wave, wave + 4,
// ...; a lane adds its pixels in ascending order and the four wave partials are added in wave order: a repeat is bit-identical.  Element
// loads are 2 bytes per lane: a concat view starts at any even column of a row of any stride, so nothing wider is aligned in general, and the
// whole launch moves 1-2 MB per image out of L2.  The twiddles come from four LDS tables (cos / sin of 2 pi h / H and 2 pi w / W, sincospif);
// the diagonal frequency is their product form.
//
// The scalar backbone (x[:, : hc / 2] *= b) rides in the same launch as further workgroups behind the skip slabs.  The structure backbone
// needs the channel mean of every pixel and its range over the image before the first element changes: one workgroup of 16 waves per image
// keeps the mean map in LDS (hence H * W <= 4096), one wave per pixel, lanes along channels.
#include "common.h"
#include "../../include/textboost_hip.h"
#include <math.h>

namespace {

const int MAX_SIDE = 256;      // LDS twiddle tables
const int MAX_PIXELS = 4096;   // LDS mean map of the structure backbone
const int MAX_CH = 1 << 20;

// grid (skip slabs + hidden slabs, B), 256 threads.  blockIdx.x < skip_slabs: the filter on skip channels [64 x, 64 x + 64); behind them the
// scalar backbone on hidden channels.  g = (s - 1) / (H W).
__global__ __launch_bounds__(256) void freeu_kernel(f16* __restrict__ x, int64_t ld, int H, int W, int hc, int sc, int skip_slabs, float b,
                                                    float g) {
  __shared__ float tw[4][MAX_SIDE];   // cos a_h, sin a_h, cos b_w, sin b_w
  __shared__ float red[4][7][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int HW = H * W;
  f16* img = x + (int64_t)blockIdx.y * HW * ld;
  if ((int)blockIdx.x >= skip_slabs) {   // (uniform over the workgroup)
    const int c = ((int)blockIdx.x - skip_slabs) * 64 + lane;
    if (c < hc / 2)
      for (int p = wave; p < HW; p += 4) {
        f16* e = img + (int64_t)p * ld + c;
        *e = (f16)((float)*e * b);
      }
    return;
  }
  for (int i = threadIdx.x; i < H; i += 256) sincospif(2.f * (float)i / (float)H, &tw[1][i], &tw[0][i]);
  for (int i = threadIdx.x; i < W; i += 256) sincospif(2.f * (float)i / (float)W, &tw[3][i], &tw[2][i]);
  __syncthreads();
  const int c = (int)blockIdx.x * 64 + lane;
  const bool on = c < sc;
  f16* col = img + hc + c;
  float m[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (on)
    for (int p = wave; p < HW; p += 4) {
      const int h = p / W, w = p - h * W;
      const float v = (float)col[(int64_t)p * ld];
      const float ca = tw[0][h], sa = tw[1][h], cb = tw[2][w], sb = tw[3][w];
      m[0] += v;
      m[1] += v * ca;
      m[2] += v * sa;
      m[3] += v * cb;
      m[4] += v * sb;
      m[5] += v * (ca * cb - sa * sb);
      m[6] += v * (sa * cb + ca * sb);
    }
#pragma unroll
  for (int k = 0; k < 7; ++k) red[wave][k][lane] = m[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 7; ++k) m[k] = ((red[0][k][lane] + red[1][k][lane]) + red[2][k][lane]) + red[3][k][lane];
  if (!on) return;
  // an axis of length 1 has the frequency 0 only: its -1 would count the same bin again
  const float wa = H > 1 ? 1.f : 0.f, wb = W > 1 ? 1.f : 0.f, wab = wa * wb;
  for (int p = wave; p < HW; p += 4) {
    const int h = p / W, w = p - h * W;
    f16* e = col + (int64_t)p * ld;
    const float ca = tw[0][h], sa = tw[1][h], cb = tw[2][w], sb = tw[3][w];
    float t = m[0];
    t += wa * (m[1] * ca + m[2] * sa);
    t += wb * (m[3] * cb + m[4] * sb);
    t += wab * (m[5] * (ca * cb - sa * sb) + m[6] * (sa * cb + ca * sb));
    *e = (f16)((float)*e + g * t);
  }
}

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}

// grid (B), 1024 threads = 16 waves; wave k owns the pixels p = k, k + 16, ...
__global__ __launch_bounds__(1024) void freeu_structure_kernel(f16* __restrict__ x, int64_t ld, int HW, int hc, float b) {
  __shared__ float mean[MAX_PIXELS];
  __shared__ float lo_s[16], hi_s[16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  f16* img = x + (int64_t)blockIdx.x * HW * ld;
  for (int p = wave; p < HW; p += 16) {
    const f16* row = img + (int64_t)p * ld;
    float a = 0.f;
    for (int c = lane; c < hc; c += 64) a += (float)row[c];
    a = wave_sum(a);
    if (lane == 0) mean[p] = a / (float)hc;
  }
  __syncthreads();
  float lo = INFINITY, hi = -INFINITY;
  for (int p = threadIdx.x; p < HW; p += 1024) {
    lo = fminf(lo, mean[p]);
    hi = fmaxf(hi, mean[p]);
  }
  lo = wave_min(lo);
  hi = wave_max(hi);
  if (lane == 0) {
    lo_s[wave] = lo;
    hi_s[wave] = hi;
  }
  __syncthreads();
  lo = lo_s[0];
  hi = hi_s[0];
#pragma unroll
  for (int k = 1; k < 16; ++k) {
    lo = fminf(lo, lo_s[k]);
    hi = fmaxf(hi, hi_s[k]);
  }
  const float range = hi - lo;
  // every read of the hidden columns lies in front of the barriers above; from here on a wave writes the rows it owns
  for (int p = wave; p < HW; p += 16) {
    const float n = range > 0.f ? (mean[p] - lo) / range : 0.f;   // a constant map: the published code divides by zero here
    const float f = (b - 1.f) * n + 1.f;
    f16* row = img + (int64_t)p * ld;
    for (int c = lane; c < hc / 2; c += 64) row[c] = (f16)((float)row[c] * f);
  }
}

}  // namespace

extern "C" int tb_freeu(void* x, int64_t ld, int B, int H, int W, int hc, int sc, float b, float s, int mode, tb_stream_t stream) {
  (void)hipGetLastError();  // drop any stale (non-sticky) error left by an earlier runtime call
  if (!x || B <= 0 || H <= 0 || W <= 0 || hc <= 0 || (hc & 1) || sc <= 0 || !isfinite(b) || !isfinite(s)) return TB_EINVAL;
  if (mode != TB_FREEU_SCALAR && mode != TB_FREEU_STRUCTURE) return TB_EINVAL;
  if (B > 65535 || H > MAX_SIDE || W > MAX_SIDE || H * W > MAX_PIXELS || hc > MAX_CH || sc > MAX_CH || ld < (int64_t)hc + sc) return TB_EINVAL;
  if (mode == TB_FREEU_STRUCTURE && b != 1.f) {
    hipLaunchKernelGGL(freeu_structure_kernel, dim3((unsigned)B), dim3(1024), 0, (hipStream_t)stream, (f16*)x, ld, H * W, hc, b);
    TB_CHECK_LAUNCH();
  }
  const int skip_slabs = s != 1.f ? (sc + 63) / 64 : 0;
  const int hid_slabs = (mode == TB_FREEU_SCALAR && b != 1.f) ? (hc / 2 + 63) / 64 : 0;
  if (skip_slabs + hid_slabs > 0) {
    const float g = (float)(((double)s - 1.0) / ((double)H * (double)W));
    hipLaunchKernelGGL(freeu_kernel, dim3((unsigned)(skip_slabs + hid_slabs), (unsigned)B), dim3(256), 0, (hipStream_t)stream, (f16*)x, ld, H,
                       W, hc, sc, skip_slabs, b, g);
    TB_CHECK_LAUNCH();
  }
  return TB_OK;
}
