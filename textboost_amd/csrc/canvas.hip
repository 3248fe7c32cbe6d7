// MultiDiffusion canvas (inference.py --width / --height; textboost_amd/canvas.py, `HipSampler.denoise_canvas`, `Pipeline.canvas_images`;
// DESIGN.md 24): a latent larger than the model's square is denoised as overlapping model-sized windows whose guided noise predictions are
// averaged where they overlap, and decoded as VAE tiles feathered in pixel space.  The UNet and the decoder run the shapes they are tuned
// for; the three kernels here are the glue: crop the windows out of the canvas, average and take the ONE solver step on the canvas, blend
// the decoded tiles.  Each moves a few hundred KB to a few tens of MB once, with one owner per output element (gathers, no atomics), so
// all three are bound by launch latency at the small end and by HBM traffic at the large end; there is nothing to tile or stage.
//
// A window's origin is any cell (the last window of an axis is clamped to the edge), so a crop row is S contiguous elements at an
// arbitrary, unaligned offset: the canvas side is read with per-lane scalar loads, consecutive lanes on consecutive addresses within a
// row (coalesced up to the row ends), and the window / tile side, which is aligned and dense, takes the stores (gather) or is read once
// per covering window (step, blend).  No vector loads on the canvas side: their alignment would depend on the table.
#include "common.h"
#include "dpm_step.h"
#include "image_byte.h"
#include "../../include/textboost_hip.h"

namespace {

// origin k of a device table, clamped so that [o, o + S) lies inside the axis whatever the table holds (`span` = L - S >= 0)
__device__ __forceinline__ int origin(const int32_t* __restrict__ t, int k, int span) { return min(max(t[k], 0), span); }

// blockIdx.y = row r of the chunk, blockIdx.x * 256 + lane = element j of its [4, S, S] crop.  Rows past the pair list repeat the last pair.
template <bool FROM_H>
__global__ __launch_bounds__(256) void canvas_gather_kernel(const float* __restrict__ x, const f16* __restrict__ xh, f16* __restrict__ x2,
                                                            int Hc, int Wc, int S, const int32_t* __restrict__ oy, int ny,
                                                            const int32_t* __restrict__ ox, int nx, int Bu, int64_t first_pair,
                                                            int64_t npairs) {
  const int per = 4 * S * S;
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= per) return;
  const int r = blockIdx.y;
  const int64_t p = min(first_pair + r, npairs - 1);
  const int nw = ny * nx;
  const int64_t img = p / nw;
  const int k = (int)(p % nw);
  const int iy = k / nx, ix = k % nx;
  const int c = j / (S * S), rem = j % (S * S);
  const int y = origin(oy, iy, Hc - S) + rem / S, xx = origin(ox, ix, Wc - S) + rem % S;
  const int64_t src = ((img * 4 + c) * Hc + y) * Wc + xx;
  const f16 h = FROM_H ? xh[src] : (f16)x[src];
  x2[(int64_t)r * per + j] = h;
  x2[(int64_t)(Bu + r) * per + j] = h;
}

// blockIdx.y = img * 4 + c, blockIdx.x * 256 + lane = cell (y, x) of the canvas.  The covering windows of a cell are a contiguous run of each
// sorted table; the tables are short (13 entries for a 2048-pixel side at the default stride) and every lane of a wave reads the same entry.
template <bool XH>
__global__ __launch_bounds__(256) void canvas_step_kernel(float* __restrict__ x, const f16* __restrict__ e, float* __restrict__ m_prev,
                                                          f16* __restrict__ xh, int Hc, int Wc, int S, const int32_t* __restrict__ oy, int ny,
                                                          const int32_t* __restrict__ ox, int nx, int Bu, float g, float alpha_t,
                                                          float sigma_t, float ca, float cb, float cc) {
  const int cell = blockIdx.x * 256 + threadIdx.x;
  if (cell >= Hc * Wc) return;
  const int y = cell / Wc, xx = cell % Wc;
  const int64_t img = blockIdx.y / 4;
  const int c = blockIdx.y % 4;
  const int64_t per = (int64_t)4 * S * S;
  float sum = 0.f;
  int cnt = 0;
  for (int iy = 0; iy < ny; ++iy) {
    const int o = origin(oy, iy, Hc - S);
    if (o > y) break;
    if (y - o >= S) continue;
    for (int ix = 0; ix < nx; ++ix) {
      const int q = origin(ox, ix, Wc - S);
      if (q > xx) break;
      if (xx - q >= S) continue;
      const int64_t p = (img * ny + iy) * nx + ix;     // a valid pair: the unused rows of a ragged last chunk are never addressed
      const int64_t row = (p / Bu) * 2 * Bu + p % Bu;
      const int64_t at = row * per + ((int64_t)c * S + (y - o)) * S + (xx - q);
      const float eg = guided_eps((float)e[at], (float)e[at + (int64_t)Bu * per], g);
      sum = cnt ? sum + eg : eg;
      ++cnt;
    }
  }
  if (!cnt) return;     // (only a device table that disagrees with the checked host table leaves a cell uncovered)
  const float eps = sum / (float)cnt;
  const int64_t i = (int64_t)blockIdx.y * Hc * Wc + cell;
  float m0, xn;
  dpm_update_eps(eps, x[i], m_prev[i], alpha_t, sigma_t, ca, cb, cc, m0, xn);
  m_prev[i] = m0;
  x[i] = xn;
  if (XH) xh[i] = (f16)xn;     // written as in dpm_step_kernel, so that the compiler folds it as there (v_fma_mixlo_f16 in the fp16 build)
}

// the feather of one axis: 1 inside the tile, ramping down to 1 / R over the R pixels next to an edge that another tile continues
__device__ __forceinline__ float axis_weight(int t, int O, int P, int Lp, int R) {
  const int lo = (O == 0) ? R : min(t - O + 1, R);
  const int hi = (O + P == Lp) ? R : min(O + P - t, R);
  return (float)min(lo, hi) / (float)R;
}

// blockIdx.y = image, blockIdx.x * 256 + lane = pixel (y, x).  NCHW stores are coalesced per channel plane, the RGBX store per pixel.
__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ tiles, int64_t ld, float* __restrict__ image,
                                                         uint32_t* __restrict__ rgbx, int Hp, int Wp, int P, const int32_t* __restrict__ ty,
                                                         int nty, const int32_t* __restrict__ tx, int ntx, int R) {
  const int pix = blockIdx.x * 256 + threadIdx.x;
  if (pix >= Hp * Wp) return;
  const int y = pix / Wp, xx = pix % Wp;
  const int64_t img = blockIdx.y;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, ws = 0.f;
  for (int iy = 0; iy < nty; ++iy) {
    const int O = origin(ty, iy, Hp - P);
    if (O > y) break;
    if (y - O >= P) continue;
    const float wy = axis_weight(y, O, P, Hp, R);
    for (int ix = 0; ix < ntx; ++ix) {
      const int Q = origin(tx, ix, Wp - P);
      if (Q > xx) break;
      if (xx - Q >= P) continue;
      const float w = wy * axis_weight(xx, Q, P, Wp, R);
      const int64_t t = (img * nty + iy) * ntx + ix;
      const float* v = tiles + ((t * P + (y - O)) * P + (xx - Q)) * ld;
      a0 += w * v[0];
      a1 += w * v[1];
      a2 += w * v[2];
      ws += w;
    }
  }
  if (!(ws > 0.f)) return;
  const float r = a0 / ws, g = a1 / ws, b = a2 / ws;
  if (image) {
    const int64_t plane = (int64_t)Hp * Wp;
    float* o = image + img * 3 * plane + pix;
    o[0] = fminf(fmaxf(r * 0.5f + 0.5f, 0.f), 1.f);
    o[plane] = fminf(fmaxf(g * 0.5f + 0.5f, 0.f), 1.f);
    o[2 * plane] = fminf(fmaxf(b * 0.5f + 0.5f, 0.f), 1.f);
  }
  if (rgbx) rgbx[img * Hp * Wp + pix] = image_byte(r) | (image_byte(g) << 8) | (image_byte(b) << 16);
}

// a host table of window origins: first 0, last L - S, strictly increasing, no gap
bool table_ok(const int32_t* t, int n, int L, int S) {
  if (!t || n <= 0 || S <= 0 || L < S || t[0] != 0 || t[n - 1] != L - S) return false;
  for (int k = 0; k + 1 < n; ++k)
    if (t[k + 1] <= t[k] || t[k + 1] - t[k] > S) return false;
  return true;
}

const int MAX_SIDE = 1 << 14;   // cells or pixels per axis: keeps every per-image index inside int32

}  // namespace

extern "C" int tb_canvas_gather(const float* x, const void* xh, void* x2, int n, int Hc, int Wc, int S, const int32_t* oy_dev,
                                const int32_t* oy_host, int ny, const int32_t* ox_dev, const int32_t* ox_host, int nx, int Bu, int chunk,
                                tb_stream_t stream) {
  (void)hipGetLastError();  // drop any stale (non-sticky) error left by an earlier runtime call
  if (!x || !x2 || !oy_dev || !ox_dev || n <= 0 || Bu <= 0 || Bu > 65535 || chunk < 0 || Hc > MAX_SIDE || Wc > MAX_SIDE) return TB_EINVAL;
  if (!table_ok(oy_host, ny, Hc, S) || !table_ok(ox_host, nx, Wc, S)) return TB_EINVAL;
  const int64_t npairs = (int64_t)n * ny * nx, first = (int64_t)chunk * Bu;
  if (first >= npairs) return TB_EINVAL;
  const dim3 grid((unsigned)((4 * S * S + 255) / 256), (unsigned)Bu);
  if (xh)
    hipLaunchKernelGGL(canvas_gather_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, (const f16*)xh, (f16*)x2, Hc, Wc, S, oy_dev, ny,
                       ox_dev, nx, Bu, first, npairs);
  else
    hipLaunchKernelGGL(canvas_gather_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, (const f16*)xh, (f16*)x2, Hc, Wc, S, oy_dev, ny,
                       ox_dev, nx, Bu, first, npairs);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_canvas_step(float* x, const void* eps_all, float* m_prev, void* xh, int n, int Hc, int Wc, int S, const int32_t* oy_dev,
                              const int32_t* oy_host, int ny, const int32_t* ox_dev, const int32_t* ox_host, int nx, int Bu, float guidance,
                              float alpha_t, float sigma_t, float ca, float cb, float cc, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!x || !eps_all || !m_prev || !oy_dev || !ox_dev || n <= 0 || 4 * (int64_t)n > 65535 || Bu <= 0 || Bu > 65535 || alpha_t == 0.f ||
      Hc > MAX_SIDE || Wc > MAX_SIDE)
    return TB_EINVAL;
  if (!table_ok(oy_host, ny, Hc, S) || !table_ok(ox_host, nx, Wc, S)) return TB_EINVAL;
  const dim3 grid((unsigned)(((int64_t)Hc * Wc + 255) / 256), (unsigned)(4 * n));
  if (xh)
    hipLaunchKernelGGL(canvas_step_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, (const f16*)eps_all, m_prev, (f16*)xh, Hc, Wc, S,
                       oy_dev, ny, ox_dev, nx, Bu, guidance, alpha_t, sigma_t, ca, cb, cc);
  else
    hipLaunchKernelGGL(canvas_step_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, (const f16*)eps_all, m_prev, (f16*)xh, Hc, Wc, S,
                       oy_dev, ny, ox_dev, nx, Bu, guidance, alpha_t, sigma_t, ca, cb, cc);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_tile_blend(const float* tiles, int64_t ld, float* image, uint32_t* rgbx, int n, int Hp, int Wp, int P, const int32_t* ty_dev,
                             const int32_t* ty_host, int nty, const int32_t* tx_dev, const int32_t* tx_host, int ntx, int ramp,
                             tb_stream_t stream) {
  (void)hipGetLastError();
  if (!tiles || (!image && !rgbx) || !ty_dev || !tx_dev || ld < 3 || n <= 0 || n > 65535 || ramp < 1 || Hp > MAX_SIDE || Wp > MAX_SIDE)
    return TB_EINVAL;
  if (!table_ok(ty_host, nty, Hp, P) || !table_ok(tx_host, ntx, Wp, P)) return TB_EINVAL;
  const dim3 grid((unsigned)(((int64_t)Hp * Wp + 255) / 256), (unsigned)n);
  hipLaunchKernelGGL(tile_blend_kernel, grid, dim3(256), 0, (hipStream_t)stream, tiles, ld, image, rgbx, Hp, Wp, P, ty_dev, nty, tx_dev, ntx,
                     ramp);
  TB_CHECK_LAUNCH();
  return TB_OK;
}
