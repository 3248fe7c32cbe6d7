// Subject masks from cross-attention (textboost_amd/auto_mask.py, make_masks.py, inference.py --mask auto:WORD): the chain from
// the accumulators of an `AttnMapRecorder` to mask bytes at the photo's pixel size,
//     word map + bilinear resize -> min / max -> 256-bin histogram -> Otsu threshold -> mask bytes -> square dilation,
// six entry points on one stream with no host read in between.  Everything is fp32 / u8 / u32 (and float64 inside the Otsu criterion):
// nothing here depends on the build's 16-bit type.  Every output element has one owner or is an integer sum, so a repeated launch gives the
// same bits.
#include "common.h"
#include "../../include/textboost_hip.h"

namespace {

constexpr int AMK_THREADS = 256;
constexpr int AMK_MAX_TOKENS = 128;    // csrc/attn_maps.hip: the recorder's limit
constexpr int AMK_MAX_MAP = 128;       // h, w of one accumulator: a band of map rows lives in LDS (at most 128 x 128 floats = 64 KiB)
constexpr int AMK_BAND = 4;            // output rows per workgroup of the resize
constexpr int AMK_RANGE_BLOCKS = 256;  // partial (min, max) pairs of the two-stage range: ws holds 2 * AMK_RANGE_BLOCKS floats
constexpr int AMK_HIST_BLOCKS = 256;
constexpr int AMK_TILE = 64;           // the dilation's output tile (AMK_TILE x AMK_TILE pixels per workgroup)
constexpr int AMK_MAX_RADIUS = 64;

struct word_positions {
  int32_t p[AMK_MAX_TOKENS];
};

// F.interpolate(mode="bilinear", align_corners=False) along one axis: output index d of `out` from `in` samples -> the lower source index and
// the weight of the upper neighbour.  The coordinate is formed in float64 (the fp32 form loses up to `in` ulps of the weight); the weight is
// rounded to fp32 once.
__device__ __forceinline__ void bilinear_source(int d, int in, int out, int& i0, int& i1, float& l1) {
  double s = ((double)d + 0.5) * ((double)in / (double)out) - 0.5;
  s = s < 0.0 ? 0.0 : s;
  i0 = (int)s;
  i0 = i0 > in - 1 ? in - 1 : i0;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l1 = (float)(s - (double)i0);
}

// One workgroup owns AMK_BAND output rows.  Stage 1: the rows [r0, r1] of the word map m that those output rows read, summed over images and
// word positions in index order into LDS.  Stage 2: one thread per output pixel interpolates from LDS and writes (or adds to) its element.
__global__ __launch_bounds__(AMK_THREADS) void map_word_upsample_kernel(const float* __restrict__ acc, int nb, int T, int h, int w,
                                                                        word_positions pos, int npos, float weight,
                                                                        float* __restrict__ score, int H, int W, int accumulate) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  float* m = reinterpret_cast<float*>(smem_raw);
  const int y0 = blockIdx.x * AMK_BAND, y1 = min(H, y0 + AMK_BAND);
  int r0, r1, t0, t1;
  float lf;
  bilinear_source(y0, h, H, r0, t0, lf);
  bilinear_source(y1 - 1, h, H, t1, r1, lf);
  const int nrows = r1 - r0 + 1;
  const int64_t hw = (int64_t)h * w;
  for (int idx = threadIdx.x; idx < nrows * w; idx += AMK_THREADS) {
    const float* src = acc + (int64_t)r0 * w + idx;
    float s = 0.f;
    for (int b = 0; b < nb; ++b)
      for (int p = 0; p < npos; ++p) s = __fadd_rn(s, src[((int64_t)b * T + pos.p[p]) * hw]);
    m[idx] = s;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < (y1 - y0) * W; idx += AMK_THREADS) {
    const int yy = idx / W, x = idx - yy * W, y = y0 + yy;
    int i0, i1, j0, j1;
    float ly, lx;
    bilinear_source(y, h, H, i0, i1, ly);
    bilinear_source(x, w, W, j0, j1, lx);
    const float* a = m + (i0 - r0) * w;
    const float* b = m + (i1 - r0) * w;
    const float top = __fadd_rn(__fmul_rn(1.f - lx, a[j0]), __fmul_rn(lx, a[j1]));
    const float bot = __fadd_rn(__fmul_rn(1.f - lx, b[j0]), __fmul_rn(lx, b[j1]));
    const float v = __fmul_rn(weight, __fadd_rn(__fmul_rn(1.f - ly, top), __fmul_rn(ly, bot)));
    float* o = score + (int64_t)y * W + x;
    *o = accumulate ? __fadd_rn(*o, v) : v;
  }
}

// ---- min / max --------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void block_min_max(float& lo, float& hi, float* red /* 8 floats of LDS */) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o, 64));
    hi = fmaxf(hi, __shfl_xor(hi, o, 64));
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = lo;
    red[4 + (threadIdx.x >> 6)] = hi;
  }
  __syncthreads();
  lo = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  hi = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
}

// (min, max) of x[0 .. n) over the whole grid's stride -> out[2 * blockIdx.x .. + 2).  16-byte loads over the aligned middle of the array.
__global__ __launch_bounds__(AMK_THREADS) void range_partial_kernel(const float* __restrict__ x, int64_t n, float* __restrict__ out) {
  __shared__ float red[8];
  float lo = INFINITY, hi = -INFINITY;
  const int64_t head = min(n, (int64_t)((4 - (((uintptr_t)x >> 2) & 3)) & 3));     // scalars in front of the first 16-byte boundary
  const int64_t n4 = (n - head) >> 2;
  const int64_t tid = (int64_t)blockIdx.x * AMK_THREADS + threadIdx.x, step = (int64_t)gridDim.x * AMK_THREADS;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x + head);
  for (int64_t i = tid; i < n4; i += step) {
    const f32x4 v = x4[i];
    lo = fminf(fminf(lo, v[0]), fminf(fminf(v[1], v[2]), v[3]));
    hi = fmaxf(fmaxf(hi, v[0]), fmaxf(fmaxf(v[1], v[2]), v[3]));
  }
  const int64_t tail = head + 4 * n4;                                              // the scalars behind the last whole float4
  for (int64_t i = tid; i < head + (n - tail); i += step) {
    const float v = x[i < head ? i : tail + (i - head)];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  block_min_max(lo, hi, red);
  if (threadIdx.x == 0) {
    out[2 * blockIdx.x] = lo;
    out[2 * blockIdx.x + 1] = hi;
  }
}

__global__ __launch_bounds__(AMK_THREADS) void range_final_kernel(const float* __restrict__ part, int nparts, float* __restrict__ minmax) {
  __shared__ float red[8];
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < nparts; i += AMK_THREADS) {
    lo = fminf(lo, part[2 * i]);
    hi = fmaxf(hi, part[2 * i + 1]);
  }
  block_min_max(lo, hi, red);
  if (threadIdx.x == 0) {
    minmax[0] = lo;
    minmax[1] = hi;
  }
}

// ---- histogram / threshold / mask -------------------------------------------------------------------------------------------------------
// the normalised score: one rounded subtraction and one rounded division (hi == lo: 0)
__device__ __forceinline__ float normalised(float s, float lo, float hi) {
  return hi == lo ? 0.f : __fdiv_rn(__fsub_rn(s, lo), __fsub_rn(hi, lo));
}

__global__ __launch_bounds__(AMK_THREADS) void hist_clear_kernel(uint32_t* __restrict__ hist) { hist[threadIdx.x] = 0u; }

__global__ __launch_bounds__(AMK_THREADS) void score_hist_kernel(const float* __restrict__ score, int64_t n, const float* __restrict__ minmax,
                                                                 uint32_t* __restrict__ hist) {
  __shared__ uint32_t bins[256];
  bins[threadIdx.x] = 0u;
  __syncthreads();
  const float lo = minmax[0], hi = minmax[1];
  for (int64_t i = (int64_t)blockIdx.x * AMK_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * AMK_THREADS) {
    const float t = normalised(score[i], lo, hi);
    int b = (int)__fmul_rn(t, 256.0f);
    b = b > 255 ? 255 : (b < 0 ? 0 : b);
    atomicAdd(&bins[b], 1u);
  }
  __syncthreads();
  const uint32_t c = bins[threadIdx.x];
  if (c) atomicAdd(&hist[threadIdx.x], c);
}

// One workgroup, thread k = candidate threshold k.  The prefix sums are exact integers; the criterion is float64 with every operation
// rounded on its own (no contraction), so the numpy float64 restatement gives the same numbers.
__global__ __launch_bounds__(256) void otsu_threshold_kernel(const uint32_t* __restrict__ hist, float* __restrict__ thr) {
  __shared__ unsigned long long w0s[256], s0s[256];
  __shared__ double cs[256];
  __shared__ int ks[256];
  const int k = threadIdx.x;
  w0s[k] = hist[k];
  __syncthreads();
  if (k == 0) {
    unsigned long long cw = 0, cv = 0;
    for (int i = 0; i < 256; ++i) {
      const unsigned long long hi = w0s[i];
      cw += hi;
      cv += hi * (unsigned long long)i;
      w0s[i] = cw;
      s0s[i] = cv;
    }
  }
  __syncthreads();
  const unsigned long long N = w0s[255], S = s0s[255], w0 = w0s[k], s0 = s0s[k];
  double c = -1.0;
  if (w0 > 0 && w0 < N) {
    const double num = __dsub_rn(__dmul_rn((double)S, (double)w0), __dmul_rn((double)N, (double)s0));
    c = __ddiv_rn(__dmul_rn(num, num), __dmul_rn((double)w0, (double)(N - w0)));
  }
  cs[k] = c;
  ks[k] = k;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {     // the maximal criterion, the smaller k on a tie
    if (k < o) {
      const double c2 = cs[k + o];
      const int k2 = ks[k + o];
      if (c2 > cs[k] || (c2 == cs[k] && k2 < ks[k])) {
        cs[k] = c2;
        ks[k] = k2;
      }
    }
    __syncthreads();
  }
  if (k == 0) {
    const int best = cs[0] >= 0.0 ? ks[0] : 255;     // no k splits the mass (one occupied bin, or an empty histogram): nothing is foreground
    thr[0] = (float)(best + 1) * (1.0f / 256.0f);
    thr[1] = (float)best;
  }
}

__global__ __launch_bounds__(AMK_THREADS) void mask_from_score_kernel(const float* __restrict__ score, const float* __restrict__ minmax,
                                                                      const float* __restrict__ thr, uint8_t* __restrict__ mask, int64_t n,
                                                                      int soft) {
  const int64_t i = (int64_t)blockIdx.x * AMK_THREADS + threadIdx.x;
  if (i >= n) return;
  const float t = normalised(score[i], minmax[0], minmax[1]);
  if (soft) {
    const float c = fminf(fmaxf(t, 0.f), 1.f);
    mask[i] = (uint8_t)rintf(__fmul_rn(255.0f, c));
  } else {
    mask[i] = t >= thr[0] ? 255 : 0;
  }
}

// ---- dilation ---------------------------------------------------------------------------------------------------------------------------
// One workgroup owns an AMK_TILE x AMK_TILE output tile: the tile plus a halo of r pixels goes to LDS (0 outside the image: the neutral element
// of the maximum, so the square is clipped at the borders), then a row pass into a second LDS image and a column pass to the output.
__global__ __launch_bounds__(AMK_THREADS) void mask_dilate_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, int W, int H, int r) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int side = AMK_TILE + 2 * r;
  uint8_t* tile = smem_raw;                 // [side][side]
  uint8_t* rows = smem_raw + side * side;   // [side][AMK_TILE]
  const int x0 = blockIdx.x * AMK_TILE, y0 = blockIdx.y * AMK_TILE;
  for (int idx = threadIdx.x; idx < side * side; idx += AMK_THREADS) {
    const int ty = idx / side, tx = idx - ty * side, x = x0 - r + tx, y = y0 - r + ty;
    tile[idx] = (x >= 0 && x < W && y >= 0 && y < H) ? in[(int64_t)y * W + x] : (uint8_t)0;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < side * AMK_TILE; idx += AMK_THREADS) {
    const int ty = idx / AMK_TILE, tx = idx - ty * AMK_TILE;
    const uint8_t* p = tile + ty * side + tx;
    uint8_t v = 0;
    for (int d = 0; d <= 2 * r; ++d) v = p[d] > v ? p[d] : v;
    rows[idx] = v;
  }
  __syncthreads();
  for (int idx = threadIdx.x; idx < AMK_TILE * AMK_TILE; idx += AMK_THREADS) {
    const int ty = idx / AMK_TILE, tx = idx - ty * AMK_TILE, x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) continue;
    const uint8_t* p = rows + ty * AMK_TILE + tx;
    uint8_t v = 0;
    for (int d = 0; d <= 2 * r; ++d) v = p[d * AMK_TILE] > v ? p[d * AMK_TILE] : v;
    out[(int64_t)y * W + x] = v;
  }
}

}  // namespace

extern "C" int tb_map_word_upsample(const float* acc, int nb, int T, int h, int w, const int32_t* positions, int npos, float weight, float* score,
                                    int H, int W, int accumulate, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!acc || !positions || !score || nb < 1 || T < 1 || T > AMK_MAX_TOKENS || npos < 1 || npos > T) return TB_EINVAL;
  if (h < 1 || w < 1 || h > AMK_MAX_MAP || w > AMK_MAX_MAP || H < 1 || W < 1 || (accumulate != 0 && accumulate != 1)) return TB_EINVAL;
  if ((int64_t)H * W > 0x7fffffff) return TB_EINVAL;
  word_positions pos;
  for (int p = 0; p < npos; ++p) {
    if (positions[p] < 0 || positions[p] >= T) return TB_EINVAL;
    pos.p[p] = positions[p];
  }
  for (int p = npos; p < AMK_MAX_TOKENS; ++p) pos.p[p] = 0;
  // map rows one band of output rows can read: AMK_BAND - 1 steps of h / H between its first and last source row, plus both neighbours
  int64_t rows = ((int64_t)(AMK_BAND - 1) * h + H - 1) / H + 3;
  rows = rows > h ? h : rows;
  const size_t lds = (size_t)rows * w * sizeof(float);
  hipLaunchKernelGGL(map_word_upsample_kernel, dim3((unsigned)((H + AMK_BAND - 1) / AMK_BAND)), dim3(AMK_THREADS), lds, (hipStream_t)stream, acc,
                     nb, T, h, w, pos, npos, weight, score, H, W, accumulate);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_score_range(const float* score, int64_t n, float* minmax, float* ws, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!score || !minmax || n < 1) return TB_EINVAL;
  int64_t blocks = ws ? (n + 4 * AMK_THREADS - 1) / (4 * AMK_THREADS) : 1;
  blocks = blocks > AMK_RANGE_BLOCKS ? AMK_RANGE_BLOCKS : blocks;
  if (blocks == 1) {      // one workgroup writes the result itself
    hipLaunchKernelGGL(range_partial_kernel, dim3(1), dim3(AMK_THREADS), 0, (hipStream_t)stream, score, n, minmax);
    TB_CHECK_LAUNCH();
    return TB_OK;
  }
  hipLaunchKernelGGL(range_partial_kernel, dim3((unsigned)blocks), dim3(AMK_THREADS), 0, (hipStream_t)stream, score, n, ws);
  TB_CHECK_LAUNCH();
  hipLaunchKernelGGL(range_final_kernel, dim3(1), dim3(AMK_THREADS), 0, (hipStream_t)stream, (const float*)ws, (int)blocks, minmax);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_score_hist(const float* score, int64_t n, const float* minmax, uint32_t* hist, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!score || !minmax || !hist || n < 1) return TB_EINVAL;
  hipLaunchKernelGGL(hist_clear_kernel, dim3(1), dim3(AMK_THREADS), 0, (hipStream_t)stream, hist);
  TB_CHECK_LAUNCH();
  int64_t blocks = (n + 8 * AMK_THREADS - 1) / (8 * AMK_THREADS);
  blocks = blocks > AMK_HIST_BLOCKS ? AMK_HIST_BLOCKS : blocks;
  hipLaunchKernelGGL(score_hist_kernel, dim3((unsigned)blocks), dim3(AMK_THREADS), 0, (hipStream_t)stream, score, n, minmax, hist);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_otsu_threshold(const uint32_t* hist, float* thr, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!hist || !thr) return TB_EINVAL;
  hipLaunchKernelGGL(otsu_threshold_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, hist, thr);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_mask_from_score(const float* score, const float* minmax, const float* thr, uint8_t* mask, int64_t n, int soft,
                                  tb_stream_t stream) {
  (void)hipGetLastError();
  if (!score || !minmax || !thr || !mask || n < 1 || (soft != 0 && soft != 1)) return TB_EINVAL;
  const int64_t blocks = (n + AMK_THREADS - 1) / AMK_THREADS;
  if (blocks > 0x7fffffff) return TB_EINVAL;
  hipLaunchKernelGGL(mask_from_score_kernel, dim3((unsigned)blocks), dim3(AMK_THREADS), 0, (hipStream_t)stream, score, minmax, thr, mask, n, soft);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_mask_dilate(const uint8_t* in, uint8_t* out, int W, int H, int radius, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!in || !out || in == out || W < 1 || H < 1 || radius < 0 || radius > AMK_MAX_RADIUS) return TB_EINVAL;
  const int gx = (W + AMK_TILE - 1) / AMK_TILE, gy = (H + AMK_TILE - 1) / AMK_TILE;
  if (gy > 65535) return TB_EINVAL;
  const int side = AMK_TILE + 2 * radius;
  const size_t lds = (size_t)side * side + (size_t)side * AMK_TILE;     // <= 192 * 192 + 192 * 64 = 49152 bytes
  hipLaunchKernelGGL(mask_dilate_kernel, dim3(gx, gy), dim3(AMK_THREADS), lds, (hipStream_t)stream, in, out, W, H, radius);
  TB_CHECK_LAUNCH();
  return TB_OK;
}
