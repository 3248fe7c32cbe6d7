// Prompt-to-prompt LocalBlend (inference.py --blend WORD ...; textboost_amd/local_blend.py; Hertz et al. 2022): the edited
// image of a prompt-to-prompt pair keeps the source image's latents except where the named words have attended so far.
//   A_r[t][s]  = the accumulator of tb_attn_token_maps for conditional row r: the head-and-layer mean of the level-2 cross-attention
//                probabilities, summed over the steps run so far                              (r = the pair's source row, its edited row)
//   m_r[s]     = sum of A_r[p][s] over the row's word positions p, in table order            (fp32 adds; nothing to contract)
//   P_r        = 3 x 3 max of m_r, stride 1, windows clipped at the borders                  mx_r = max_s P_r[s] = max_s m_r[s]
//   bit_r[s]   = P_r[s] > fl32(th mx_r)                                                      (one rounded multiply, strict compare)
//   mask[y][x] = (bit_src | bit_edit)[y / (h / h_l)][x / (w / w_l)]  [& limit[y][x] != 0]    (nearest upsampling commutes with all of the above)
//
//   * tb_blend_mask             one workgroup per pair: the two word-sum maps in the LDS, the stencil, the threshold, the upsampled bytes
//   * tb_dpm_step_local_blend   tb_dpm_step for all rows, then x_edit <- mask ? x_edit : x_src against the source row's value of the same step
//
// `acc` must be finite: the maxima are taken with fmaxf, which drops a NaN where the host restatement (numpy's max) would propagate it.
//
// Ownership.  Every output byte / element has one owning lane, maxima are exact in any order and the cell count is an integer: no atomics,
// no read-back, a relaunch is bit-identical.  Both are small kernels (the mask is 4 KB per pair, the step 64 KB per image); they exist so
// that the whole edit stays on the device and captures into one graph.
#include <cmath>

#include "common.h"
#include "dpm_step.h"
#include "../../include/textboost_hip.h"

namespace {

constexpr int LB_THREADS = 256;
constexpr int LB_MAX_HW = 2048;   // positions of the coarse map (two fp32 images and one byte image of it in the LDS: 18 KB)
constexpr int LB_MAX_T = 128;     // prompt tokens (tb_attn_token_maps' limit)
constexpr int LB_MAX_P = 16;      // word positions per row

__global__ __launch_bounds__(LB_THREADS) void blend_mask_kernel(const float* __restrict__ acc, const int32_t* __restrict__ words, int n, int T,
                                                                int hl, int wl, int h, int w, int n_pos, float th,
                                                                const uint8_t* __restrict__ limit, uint8_t* __restrict__ mask,
                                                                int32_t* __restrict__ area) {
  // (all LDS in the dynamic region, every carve a multiple of 16 bytes)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int HW = hl * wl, HWp = (HW + 3) & ~3;
  float* m = reinterpret_cast<float*>(smem_raw);                 // [2][HWp] the word-sum maps: source row, edited row
  float* red = m + 2 * HWp;                                      // [8] per-wave maxima of the two rows
  int* cnt = reinterpret_cast<int*>(red + 8);                    // [4] per-wave cell counts
  uint8_t* bits = reinterpret_cast<uint8_t*>(cnt + 4);           // [HW] bit_src | bit_edit
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6, pair = blockIdx.x;

  // ---- the word sums of both rows, and each row's maximum (= the maximum of its pooled map)
  float mx[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int row = pair + r * n;
    const float* A = acc + (int64_t)row * T * HW;
    int J[LB_MAX_P];   // the row's table, read once (block-uniform); entries past n_pos and positions outside [0, T) become -1
#pragma unroll
    for (int p = 0; p < LB_MAX_P; ++p) {
      const int j = p < n_pos ? words[(int64_t)row * n_pos + p] : -1;
      J[p] = j < T ? j : -1;
    }
    float v = -INFINITY;
    for (int s = t; s < HW; s += LB_THREADS) {
      float sum = 0.f;
#pragma unroll
      for (int p = 0; p < LB_MAX_P; ++p)   // table order
        if (J[p] >= 0) sum += A[(int64_t)J[p] * HW + s];
      m[r * HWp + s] = sum;
      v = fmaxf(v, sum);
    }
    v = wave_max(v);
    if (lane == 0) red[r * 4 + wave] = v;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < 2; ++r) mx[r] = fmaxf(fmaxf(red[r * 4], red[r * 4 + 1]), fmaxf(red[r * 4 + 2], red[r * 4 + 3]));
  const float thr0 = __fmul_rn(th, mx[0]), thr1 = __fmul_rn(th, mx[1]);

  // ---- 3 x 3 max with clipped windows, the strict compare, the union of the two rows
  for (int s = t; s < HW; s += LB_THREADS) {
    const int y = s / wl, x = s - y * wl;
    const int y0 = y > 0 ? y - 1 : 0, y1 = y < hl - 1 ? y + 1 : hl - 1, x0 = x > 0 ? x - 1 : 0, x1 = x < wl - 1 ? x + 1 : wl - 1;
    float p0 = m[y * wl + x], p1 = m[HWp + y * wl + x];
    for (int yy = y0; yy <= y1; ++yy)
      for (int xx = x0; xx <= x1; ++xx) {
        p0 = fmaxf(p0, m[yy * wl + xx]);
        p1 = fmaxf(p1, m[HWp + yy * wl + xx]);
      }
    bits[s] = (uint8_t)((p0 > thr0) | (p1 > thr1));
  }
  __syncthreads();

  // ---- nearest upsampling to the latent grid, the limit, one byte per lane; the cell count
  const int fy = h / hl, fx = w / wl;
  const int64_t hw = (int64_t)h * w;
  uint8_t* out = mask + (int64_t)pair * hw;
  int c = 0;
  for (int64_t i = t; i < hw; i += LB_THREADS) {
    const int y = (int)(i / w), x = (int)(i - (int64_t)y * w);
    bool on = bits[(y / fy) * wl + x / fx] != 0;
    if (limit) on = on && limit[i] != 0;
    out[i] = on ? 255 : 0;
    c += on ? 1 : 0;
  }
  if (area) {   // (block-uniform)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) cnt[wave] = c;
    __syncthreads();
    if (t == 0) area[pair] = cnt[0] + cnt[1] + cnt[2] + cnt[3];
  }
}

// `dpm_step_kernel` (elementwise.hip) through the shared `dpm_update` for both rows of a pair, then the select.  blockIdx.y = pair p (source
// row p, edited row p + B / 2), blockIdx.x * 256 + lane = element j of a row's n_per_b = C * hw latents (NCHW), so cell j % hw of the pair's
// mask, which the channels share.  The lane owns element j of BOTH rows: it reads no x another lane writes.
//   x[p, j]         <- the step's x
//   x[p + B/2, j]   <- mask[p][j % hw] ? (the step's x) : x[p, j] (the new one)
// m_prev gets every row's own unblended data prediction.
__global__ __launch_bounds__(256) void dpm_step_local_blend_kernel(float* __restrict__ x, const f16* __restrict__ e, float* __restrict__ m_prev,
                                                                   f16* __restrict__ x2, int64_t n_per_b, int B, float g, float alpha_t,
                                                                   float sigma_t, float ca, float cb, float cc,
                                                                   const uint8_t* __restrict__ mask, int hw) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= n_per_b) return;
  const int p = blockIdx.y, n = B / 2;
  const int64_t tot = n_per_b * B;
  const int64_t is = (int64_t)p * n_per_b + j, ie = (int64_t)(p + n) * n_per_b + j;
  float m0s, xs, m0e, xe;
  dpm_update((float)e[is], (float)e[tot + is], x[is], m_prev[is], g, alpha_t, sigma_t, ca, cb, cc, m0s, xs);
  dpm_update((float)e[ie], (float)e[tot + ie], x[ie], m_prev[ie], g, alpha_t, sigma_t, ca, cb, cc, m0e, xe);
  m_prev[is] = m0s;
  m_prev[ie] = m0e;
  const bool keep = mask[(int64_t)p * hw + j % hw] != 0;
  // x2 carries `dpm_step_kernel`'s bits: of the row's own step where it is kept, of the SOURCE row's step where it is blended -- so that a
  // row feeds the next UNet call what text-to-image feeds it, and an all-zero mask makes the edited row the source row in x and x2.  Both
  // conversions are written as there and left to the compiler as there (in the fp16 build each folds into its update's last fma,
  // v_fma_mixlo_f16: one rounding of the exact fma, which is half(x) except on ties of the double rounding).  The empty statements keep the
  // compiler from moving the select in front of the conversions (see dpm_step_pin_kernel, invert.hip); tests/test_gpu_blend.py holds x2
  // against tb_dpm_step's bits in both builds.
  f16 hs = (f16)xs, he = (f16)xe;
  asm volatile("" : "+v"(hs));
  asm volatile("" : "+v"(he));
  const f16 h = keep ? he : hs;
  x[is] = xs;
  x[ie] = keep ? xe : xs;
  x2[is] = hs;
  x2[tot + is] = hs;
  x2[ie] = h;
  x2[tot + ie] = h;
}

}  // namespace

extern "C" int tb_blend_mask(const float* acc, const int32_t* words, int n, int T, int hl, int wl, int h, int w, int n_pos, float th,
                             const uint8_t* limit, uint8_t* mask, int32_t* area, tb_stream_t stream) {
  (void)hipGetLastError();  // drop any stale (non-sticky) error left by an earlier runtime call
  if (!acc || !words || !mask || n <= 0 || n > (1 << 20) || T < 2 || T > LB_MAX_T || hl <= 0 || wl <= 0 || (int64_t)hl * wl > LB_MAX_HW ||
      n_pos < 1 || n_pos > LB_MAX_P || h <= 0 || w <= 0 || h % hl != 0 || w % wl != 0 || (int64_t)h * w > (1 << 24) || !std::isfinite(th))
    return TB_EINVAL;
  const int HWp = (hl * wl + 3) & ~3;
  const size_t lds = (size_t)2 * HWp * sizeof(float) + 8 * sizeof(float) + 4 * sizeof(int) + (size_t)HWp;
  hipLaunchKernelGGL(blend_mask_kernel, dim3((unsigned)n), dim3(LB_THREADS), lds, (hipStream_t)stream, acc, words, n, T, hl, wl, h, w, n_pos, th,
                     limit, mask, area);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_dpm_step_local_blend(float* x, const void* eps2, float* m_prev, void* x2, int64_t n_per_b, int B, float guidance,
                                       float alpha_t, float sigma_t, float ca, float cb, float cc, const uint8_t* mask, int hw,
                                       tb_stream_t stream) {
  (void)hipGetLastError();
  if (!x || !eps2 || !m_prev || !x2 || !mask || n_per_b <= 0 || B <= 0 || B > 65535 || B % 2 != 0 || alpha_t == 0.f || hw <= 0 ||
      n_per_b % hw != 0)
    return TB_EINVAL;
  hipLaunchKernelGGL(dpm_step_local_blend_kernel, dim3((unsigned)((n_per_b + 255) / 256), (unsigned)(B / 2)), dim3(256), 0, (hipStream_t)stream,
                     x, (const f16*)eps2, m_prev, (f16*)x2, n_per_b, B, guidance, alpha_t, sigma_t, ca, cb, cc, mask, hw);
  TB_CHECK_LAUNCH();
  return TB_OK;
}
