// Attend-and-Excite (inference.py --excite): a training-free guidance that nudges the latents until every named word owns
// a strongly attended patch of the level-2 cross-attention maps.
//   A[j][s]   = mean over the supervised layers and their heads of softmax_j(scale q_s . k_j)      (accumulated by tb_attn_token_maps)
//   pt_j[s]   = softmax over j in [1, last) of 100 A[j][s]            M_w[s] = sum_{j in J_w} pt_j[s]
//   G_w       = M_w * (3 x 3 Gaussian, sigma 0.5, reflect padding)    l_w = max(0, 1 - max_s G_w[s])      L = max_w l_w
//
//   * tb_excite_loss    one workgroup per image: L, the worst word, the <= 9 positions whose taps feed its arg-max, and loss_scale dL/dA there
//   * tb_excite_bwd     one wave per (image, selected position, head): recomputes that query row's softmax and ADDS the gradient to its dQ row
//   * tb_excite_update  x -= (step / loss_scale) g per image, only where every element of g is finite (reduce, then apply)
//
// Ownership.  Every output element has one owning thread and nothing is accumulated with atomics: a relaunch is bit-identical.  The loss kernel
// works in double behind the fp32 maps (its arithmetic is a few thousand exponentials per image): the arg-max and the tie rule -- lowest word,
// lowest position -- then depend on the inputs alone, and the outputs are rounded to fp32 once.
#include <cmath>
#include <vector>

#include "common.h"
#include "../../include/textboost_hip.h"

namespace {

constexpr int EX_THREADS = 256;
constexpr int EX_MAX_HW = 2048;   // positions of a supervised map (three double images of it in the LDS: 48 KB)
constexpr int EX_MAX_T = 128;     // prompt tokens (tb_attn_token_maps' limit)
constexpr int EX_MAX_W = 8;       // words
constexpr int EX_MAX_P = 16;      // token positions per word
constexpr int EX_SEL = 9;         // selected positions per image: the 3 x 3 taps of the arg-max, reflect-folded

__device__ __forceinline__ int ex_reflect(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * n - 2 - i : i); }

// (value, index) arg-max with the tie rule "lowest index": is (ov, oi) better than (v, i)?
__device__ __forceinline__ bool ex_better(double ov, int oi, double v, int i) { return ov > v || (ov == v && oi < i); }

// the token set of word `wi` of image b as a 128-bit mask; positions outside [1, lst) (the -1 padding included) are not members
__device__ __forceinline__ void ex_word_mask(const int32_t* __restrict__ words, int Pn, int lst, uint64_t& lo, uint64_t& hi) {
  lo = 0, hi = 0;
  for (int p = 0; p < Pn; ++p) {
    const int j = words[p];
    if (j >= 1 && j < lst) {
      if (j < 64) lo |= 1ull << j;
      else hi |= 1ull << (j - 64);
    }
  }
}
__device__ __forceinline__ bool ex_member(uint64_t lo, uint64_t hi, int j) { return ((j < 64 ? lo >> j : hi >> (j - 64)) & 1ull) != 0; }

__global__ __launch_bounds__(EX_THREADS) void excite_loss_kernel(const float* __restrict__ A, const int32_t* __restrict__ last,
                                                                 const int32_t* __restrict__ words, int T, int h, int w, int Wn, int Pn,
                                                                 float loss_scale, double k0, double k1, float* __restrict__ loss,
                                                                 int32_t* __restrict__ word,
                                                                 int32_t* __restrict__ sel, float* __restrict__ dA) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  __shared__ double redv[4];
  __shared__ int redi[4];
  __shared__ double msel[EX_SEL];
  const int HW = h * w, t = threadIdx.x, lane = t & 63, wave = t >> 6, b = blockIdx.x;
  double* mx = reinterpret_cast<double*>(smem_raw);   // [HW] max_j A[j][s]
  double* inv = mx + HW;                               // [HW] 1 / sum_j exp(100 (A[j][s] - mx[s]))
  double* M = inv + HW;                                // [HW] the current word's map
  const float* Ab = A + (int64_t)b * T * HW;
  int lst = last[b];
  lst = lst < 1 ? 1 : (lst > T ? T : lst);
  // ---- the token softmax of every position: one lane walks its position's tokens in order
  for (int s = t; s < HW; s += EX_THREADS) {
    float m = -INFINITY;
    for (int j = 1; j < lst; ++j) m = fmaxf(m, Ab[(int64_t)j * HW + s]);
    double sum = 0.0;
    for (int j = 1; j < lst; ++j) sum += exp(100.0 * ((double)Ab[(int64_t)j * HW + s] - (double)m));
    mx[s] = (double)m;
    inv[s] = 1.0 / sum;
  }
  // ---- the words in order: map, 3 x 3 Gaussian, spatial arg-max; the worst word so far is kept (a later word must be strictly worse)
  // (k0, k1: the centre and the side tap of the Gaussian, [e^-2, 1, e^-2] / (1 + 2 e^-2), computed once on the host)
  int best_w = -1, best_s = 0;
  double best_l = 0.0;
  for (int wi = 0; wi < Wn; ++wi) {
    uint64_t lo, hi;
    ex_word_mask(words + ((int64_t)b * Wn + wi) * Pn, Pn, lst, lo, hi);
    if ((lo | hi) == 0) continue;   // (block-uniform: the table is the same for every thread)
    __syncthreads();                // the previous word's map has been read (first word: the statistics are written)
    for (int s = t; s < HW; s += EX_THREADS) {
      double acc = 0.0;
      for (int j = 1; j < lst; ++j)
        if (ex_member(lo, hi, j)) acc += exp(100.0 * ((double)Ab[(int64_t)j * HW + s] - mx[s])) * inv[s];
      M[s] = acc;
    }
    __syncthreads();
    double v = -1.0;
    int vi = 0x7fffffff;
    for (int s = t; s < HW; s += EX_THREADS) {
      const int y = s / w, x = s - y * w;
      double g = 0.0;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx)
          // (no fused multiply-add: the nine taps of a constant map then add up to the same value at every position, and to exactly what
          // the row-major float64 restatement gets -- ties and l = 0 are decided by the inputs, not by the contraction the compiler picks)
          g = __dadd_rn(g, __dmul_rn(__dmul_rn(dy ? k1 : k0, dx ? k1 : k0), M[ex_reflect(y + dy, h) * w + ex_reflect(x + dx, w)]));
      if (ex_better(g, s, v, vi)) v = g, vi = s;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double ov = __shfl_xor(v, o, 64);
      const int oi = __shfl_xor(vi, o, 64);
      if (ex_better(ov, oi, v, vi)) v = ov, vi = oi;
    }
    if (lane == 0) redv[wave] = v, redi[wave] = vi;
    __syncthreads();
    v = redv[0], vi = redi[0];
#pragma unroll
    for (int q = 1; q < 4; ++q)
      if (ex_better(redv[q], redi[q], v, vi)) v = redv[q], vi = redi[q];
    const double l = v < 1.0 ? 1.0 - v : 0.0;
    if (best_w < 0 || l > best_l) best_w = wi, best_s = vi, best_l = l;
  }
  // ---- the selection: the taps of the arg-max of the worst word, folded by the reflection, in ascending position order
  int spos[EX_SEL];
  double kap[EX_SEL];
  int nsel = 0;
  if (best_w >= 0 && best_l > 0.0) {
    const int y = best_s / w, x = best_s - y * w;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        const int p = ex_reflect(y + dy, h) * w + ex_reflect(x + dx, w);
        const double kw = (dy ? k1 : k0) * (dx ? k1 : k0);
        int i = 0;
        while (i < nsel && spos[i] != p) ++i;
        if (i == nsel) spos[nsel] = p, kap[nsel] = kw, ++nsel;
        else kap[i] += kw;
      }
    for (int i = 1; i < nsel; ++i)   // insertion sort, <= 9 entries
      for (int q = i; q > 0 && spos[q - 1] > spos[q]; --q) {
        const int ts = spos[q]; spos[q] = spos[q - 1]; spos[q - 1] = ts;
        const double tk = kap[q]; kap[q] = kap[q - 1]; kap[q - 1] = tk;
      }
  }
  uint64_t lo = 0, hi = 0;
  if (nsel) ex_word_mask(words + ((int64_t)b * Wn + best_w) * Pn, Pn, lst, lo, hi);
  __syncthreads();
  if (t < nsel) {   // M of the worst word at the selected positions (its map in the LDS has been overwritten by later words)
    const int s = spos[t];
    double acc = 0.0;
    for (int j = 1; j < lst; ++j)
      if (ex_member(lo, hi, j)) acc += exp(100.0 * ((double)Ab[(int64_t)j * HW + s] - mx[s])) * inv[s];
    msel[t] = acc;
  }
  __syncthreads();
  if (t == 0) {
    loss[b] = (float)best_l;
    word[b] = best_w;
  }
  if (t < EX_SEL) sel[(int64_t)b * EX_SEL + t] = t < nsel ? spos[t] : -1;
  float* dAb = dA + (int64_t)b * EX_SEL * T;
  for (int u = t; u < EX_SEL * T; u += EX_THREADS) {
    const int i = u / T, j = u - i * T;
    double d = 0.0;
    if (i < nsel && j >= 1 && j < lst) {
      // (spos / kap are indexed by a run-time i: a small select chain instead of scratch memory)
      int s = 0;
      double kw = 0.0;
#pragma unroll
      for (int q = 0; q < EX_SEL; ++q)
        if (q == i) s = spos[q], kw = kap[q];
      const double p = exp(100.0 * ((double)Ab[(int64_t)j * HW + s] - mx[s])) * inv[s];
      d = -100.0 * (double)loss_scale * kw * p * ((ex_member(lo, hi, j) ? 1.0 : 0.0) - msel[i]);
    }
    dAb[u] = (float)d;
  }
}

// One wave per (selected slot, head, image).  Lane l owns keys l and l + 64 in the softmax, head-dim elements l, l + 64, l + 128 in the sum over
// the keys; scores and that sum are accumulated in double (77 x 160 products per wave: nothing), the softmax itself is fp32.
__global__ __launch_bounds__(64) void excite_bwd_kernel(const f16* __restrict__ Q, int64_t ldq, const f16* __restrict__ K, int64_t ldk,
                                                        f16* __restrict__ dQ, int64_t lddq, const int32_t* __restrict__ sel,
                                                        const float* __restrict__ dA, int Sq, int Skv, int hd, float scale, float coef, int b0) {
  __shared__ float qs[160];
  __shared__ float ds[128];
  const int lane = threadIdx.x, slot = blockIdx.x, hh = blockIdx.y, bi = blockIdx.z, b = b0 + bi;
  const int s = sel[(int64_t)bi * EX_SEL + slot];
  if (s < 0 || s >= Sq) return;   // (block-uniform)
  const f16* q = Q + ((int64_t)b * Sq + s) * ldq + hh * hd;
  const f16* Kg = K + (int64_t)b * Skv * ldk + hh * hd;
  const float* dAr = dA + ((int64_t)bi * EX_SEL + slot) * Skv;
  for (int d = lane; d < hd; d += 64) qs[d] = (float)q[d];
  __syncthreads();
  float sc[2], da[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int j = lane + 64 * r;
    double acc = 0.0;
    if (j < Skv) {
      const f16* kj = Kg + (int64_t)j * ldk;
      for (int d = 0; d < hd; ++d) acc += (double)qs[d] * (double)(float)kj[d];
    }
    sc[r] = j < Skv ? scale * (float)acc : -INFINITY;
    da[r] = j < Skv ? coef * dAr[j] : 0.f;
  }
  const float m = wave_max(fmaxf(sc[0], sc[1]));
  float e[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) e[r] = lane + 64 * r < Skv ? expf(sc[r] - m) : 0.f;
  const float inv = 1.0f / wave_sum(e[0] + e[1]);
  const float p0 = e[0] * inv, p1 = e[1] * inv;
  const float dot = wave_sum(p0 * da[0] + p1 * da[1]);
  ds[lane] = p0 * (da[0] - dot);
  ds[lane + 64] = p1 * (da[1] - dot);
  __syncthreads();
  f16* dq = dQ + ((int64_t)b * Sq + s) * lddq + hh * hd;
  for (int d = lane; d < hd; d += 64) {
    double acc = 0.0;
    for (int j = 0; j < Skv; ++j) acc += (double)ds[j] * (double)(float)Kg[(int64_t)j * ldk + d];
    const float add = scale * (float)acc;
    if (add != 0.f) dq[d] = (f16)((float)dq[d] + add);   // (a zero addend stores nothing: -0 stays -0)
  }
}

// stage 1: bad[b] = (step[b] != 0 and some element of g[b] is not finite).  One workgroup per image, no atomics.
__global__ __launch_bounds__(256) void excite_flag_kernel(const f16* __restrict__ g, const float* __restrict__ step, int64_t n,
                                                          int32_t* __restrict__ bad) {
  const int b = blockIdx.x;
  const f16* gb = g + (int64_t)b * n;
  int any = 0;
  if (step[b] != 0.f)
    for (int64_t i = threadIdx.x; i < n; i += 256) {
      const float v = (float)gb[i];
      any |= !(fabsf(v) <= 3.4028234664e38f);   // inf and NaN
    }
  any = __syncthreads_or(any);
  if (threadIdx.x == 0) bad[b] = any ? 1 : 0;
}

// stage 2: the update of the images stage 1 passed; an image with step 0 is not written at all
__global__ __launch_bounds__(256) void excite_apply_kernel(float* __restrict__ x, const f16* __restrict__ g, const float* __restrict__ step,
                                                           const int32_t* __restrict__ bad, f16* __restrict__ x2, int64_t n, int B,
                                                           float loss_scale) {
  const int b = blockIdx.y;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float st = step[b];
  if (i >= n || st == 0.f || bad[b]) return;
  const float c = st / loss_scale;
  const int64_t at = (int64_t)b * n + i;
  float xn = __fsub_rn(x[at], __fmul_rn(c, (float)g[at]));
  asm volatile("" : "+v"(xn));   // x2 = the rounding of the fp32 value x holds: the conversion must not fold into the arithmetic (edit.hip)
  x[at] = xn;
  x2[at] = (f16)xn;
  x2[(int64_t)B * n + at] = (f16)xn;
}

}  // namespace

extern "C" int tb_excite_loss(const float* A, const int32_t* last, const int32_t* words, int nb, int T, int h, int w, int n_words, int n_pos,
                              float loss_scale, int check, float* loss, int32_t* word, int32_t* sel, float* dA, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!A || !last || !words || !loss || !word || !sel || !dA) return TB_EINVAL;
  if (nb < 1 || nb > 65535 || T < 2 || T > EX_MAX_T || h < 2 || w < 2 || (int64_t)h * w > EX_MAX_HW) return TB_EINVAL;
  if (n_words < 1 || n_words > EX_MAX_W || n_pos < 1 || n_pos > EX_MAX_P || !(loss_scale > 0.f) || (check != 0 && check != 1)) return TB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  if (check) {
    // The tables live on the device.  check = 1 (outside a stream capture only) reads them back and refuses a `last` outside [1, T] and a
    // position that is neither -1 nor in [1, last); with check = 0 the kernel ignores such a position.
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) return TB_ELAUNCH;
    if (cap != hipStreamCaptureStatusNone) return TB_EINVAL;
    std::vector<int32_t> hl((size_t)nb), hw_((size_t)nb * n_words * n_pos);
    if (hipMemcpyAsync(hl.data(), last, hl.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipMemcpyAsync(hw_.data(), words, hw_.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      tb_last_hip_error_code_ = (int)hipGetLastError();
      return TB_ELAUNCH;
    }
    for (int b = 0; b < nb; ++b) {
      if (hl[b] < 1 || hl[b] > T) return TB_EINVAL;
      for (int i = 0; i < n_words * n_pos; ++i) {
        const int32_t j = hw_[(size_t)b * n_words * n_pos + i];
        if (j != -1 && (j < 1 || j >= hl[b])) return TB_EINVAL;
      }
    }
  }
  const size_t lds = (size_t)3 * h * w * sizeof(double);
  const double e2 = std::exp(-2.0), k1 = e2 / (1.0 + 2.0 * e2), k0 = 1.0 / (1.0 + 2.0 * e2);
  hipLaunchKernelGGL(excite_loss_kernel, dim3((unsigned)nb), dim3(EX_THREADS), lds, s, A, last, words, T, h, w, n_words, n_pos, loss_scale, k0, k1,
                     loss, word, sel, dA);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_excite_bwd(const tb_attn_desc* d, int dtype, int b0, int nb, const int32_t* sel, const float* dA, float coef,
                             tb_stream_t stream) {
  (void)hipGetLastError();
  if (!d || !d->Q || !d->K || !d->dQ || !sel || !dA || dtype != TB_F16) return TB_EINVAL;
  if (d->B < 1 || d->H < 1 || d->H > 65535 || d->Sq < 1 || d->Skv < 1 || d->Skv > EX_MAX_T) return TB_EINVAL;
  if (d->hd < 8 || d->hd % 8 != 0 || d->hd > 160) return TB_EINVAL;
  if (b0 < 0 || nb < 1 || nb > 65535 || (int64_t)b0 + nb > d->B || !(coef == coef)) return TB_EINVAL;
  const int64_t C = (int64_t)d->H * d->hd;
  if (d->ldq < C || d->ldk < C || d->lddq < C) return TB_EINVAL;
  hipLaunchKernelGGL(excite_bwd_kernel, dim3(EX_SEL, (unsigned)d->H, (unsigned)nb), dim3(64), 0, (hipStream_t)stream, (const f16*)d->Q, d->ldq,
                     (const f16*)d->K, d->ldk, (f16*)d->dQ, d->lddq, sel, dA, d->Sq, d->Skv, d->hd, d->scale, coef, b0);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_excite_update(float* x, const void* g, const float* step, void* x2, int32_t* bad, int64_t n_per_b, int B, float loss_scale,
                                tb_stream_t stream) {
  (void)hipGetLastError();
  if (!x || !g || !step || !x2 || !bad || n_per_b <= 0 || B <= 0 || B > 65535 || !(loss_scale > 0.f)) return TB_EINVAL;
  const int64_t blocks = (n_per_b + 255) / 256;
  if (blocks > 0x7fffffff) return TB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(excite_flag_kernel, dim3((unsigned)B), dim3(256), 0, s, (const f16*)g, step, n_per_b, bad);
  TB_CHECK_LAUNCH();
  hipLaunchKernelGGL(excite_apply_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, s, x, (const f16*)g, step, bad, (f16*)x2, n_per_b, B,
                     loss_scale);
  TB_CHECK_LAUNCH();
  return TB_OK;
}
