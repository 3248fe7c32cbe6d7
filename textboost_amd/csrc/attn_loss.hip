// Cross-attention localisation loss (--attn_loss_weight): a training loss that tells the placeholder token where to attend.
//   p_{b,h,s,j} = softmax_j(scale q_{b,h,s} . k_{b,h,j})         P_J = sum_j tok_w[b,j] p_j         A_{b,s} = (1/H) sum_h P_J
//   L_layer = sum_b sum_s g[b,s] A_{b,s}                         (g from tb_attn_loss_coef: negative on the subject, positive off it)
//   ds_j = p_j (c g_s / H) (tok_w_j - P_J)       dq_s += scale sum_j ds_j k_j       dk_j += scale sum_s ds_{s,j} q_s
//
//   * tb_attn_loss_coef   latent-grid target [B, 1, h, w] -> g [B, (h/f)(w/f)]: one workgroup per sample, box means and sums in double
//   * tb_attn_loss_bwd    recomputes the layer's softmax (as tb_attn_token_maps does) and ADDS the gradient into dQ / dK; writes the partial
//                         sums of the loss into the layer's slot of the workspace
//   * tb_attn_loss_final  adds the partials of all slots in a fixed order -> state[TB_ST_LOSS_ATTN]
//
// Ownership (tb_attn_loss_bwd).  One workgroup (four waves) owns one (batch, head) and walks its queries in blocks of 64: every dQ element is
// written once by one lane, dK stays in that workgroup's accumulators over all query blocks and is written once at the end.  No atomics, no
// second stage: eager launches and graph replays are bit-identical.  The default layers (Sq = 256, 8 heads, B = 8) give 64 workgroups of four
// blocks each: the launch is latency-bound either way, and a query-split dK would add a workspace pass per layer for nothing.
//
// Tile plan.  K_h lies in LDS twice, [keys][hd] and transposed [hd][keys]; so does each 64-query block of Q_h.
//   phase A  (wave w: queries 32 (w & 1) ..)  S^T = K Q^T on 32 x 32 x 16 MFMA tiles as in attn_maps.hip: the QUERY on the lane, the keys in the
//            registers, so max, sum, P_J and w = g_s p_j (tok_w_j - P_J) are in-lane fp32 arithmetic.  The accumulator registers are, as they
//            stand, the A operand of dQ = W K (the contraction index of an MFMA may be permuted as long as both operands agree: element e of
//            k-step t is key 16 t + 8 (e >> 2) + (e & 3) + 4 hi, which K^T serves as two 8-byte LDS reads).  The two waves of a query half
//            share its d-tiles.  (m, 1 / sum, P_J, g_s) of every query go to LDS for phase B.
//   phase B  (wave w: key tile w)  S = Q K^T, the KEY on the lane and the queries in the registers, softmax from the stored statistics; the
//            registers are the A operand of dK = W^T Q against Q^T from LDS.  dK: 5 d-tiles x 16 accumulator registers per lane.
// W is the only inexact MFMA operand (q, k are the 16-bit operands themselves).  It enters as THREE 16-bit terms (hi + mid + lo, 24 bits and
// more: fp16 terms carry 11 bits and are pre-scaled by 2^10 against the subnormal range, bf16 terms 8 bits), so the contractions see fp32 data
// and the result's error is that of an fp32 evaluation; the uniform factor c scale loss_scale / H is applied in fp32 behind the MFMAs.
#include "common.h"
#include "../../include/textboost_hip.h"

namespace {

constexpr int AL_BQ = 64;         // queries per block
constexpr int AL_MAX_KV = 128;    // keys: at most four 32-row tiles, one per wave in phase B
constexpr int AL_THREADS = 256;
constexpr int AL_MAX_DT = 5;      // 32-wide tiles of the head dim (hd <= 160)
#ifdef TB_BF16
constexpr float AL_PRE = 1.f;     // bf16 has fp32's exponent range
#else
constexpr float AL_PRE = 1024.f;  // |g u| 2^10 < 65504 for |g| < 63 (tb_attn_loss_coef gives |g| <= 1), and the third term reaches 2^-34
#endif

template <bool ALIGNED>
__device__ __forceinline__ f16x8 al_load8(const f16* src) {
  if constexpr (ALIGNED) return *(const f16x8*)src;
  f16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = src[e];
  return v;
}

// x = a + b + c up to 2^-24 |x| (and better), each term one 16-bit float.  x is pinned to ONE register value first: it arrives as a product, and
// with contraction allowed the compiler may round that product to 16 bits twice, once fused (from the exact product) for the stored term and
// once from the rounded fp32 value for the residual.  Where the product lies within an fp32 ulp of a 16-bit tie the two differ by a whole
// 16-bit ulp, and the terms no longer add up to x (seen on one key of one test case: 2^-10 relative on that key's dK row).
__device__ __forceinline__ void al_split3(float x, f16& a, f16& b, f16& c) {
  asm("" : "+v"(x));
  a = (f16)x;
  float r = x - (float)a;
  b = (f16)r;
  r -= (float)b;
  c = (f16)r;
}

// eight contraction elements of a transposed LDS image for k-step t of a 32-element tile: [16 t + 4 hi, +4) and [16 t + 8 + 4 hi, +4)
__device__ __forceinline__ f16x8 al_perm8(const f16* p) {
  const f16x4 lo = *(const f16x4*)p, hi = *(const f16x4*)(p + 8);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

struct AlLds {
  int pitch, kpitch, qpitch, hdp, nkt;
  size_t kl, ktl, ql, qtl, st, tokw, red, total;   // byte offsets
};

__host__ __device__ inline AlLds al_layout(int Skv, int hd) {
  AlLds L;
  L.nkt = (Skv + 31) >> 5;
  L.hdp = (hd + 31) & ~31;
  L.pitch = L.hdp + 8;            // halfs; rows 16-byte aligned
  L.kpitch = L.nkt * 32 + 8;
  L.qpitch = AL_BQ + 8;
  size_t o = 0;
  L.kl = o;   o += (size_t)L.nkt * 32 * L.pitch * 2;
  L.ktl = o;  o += (size_t)L.hdp * L.kpitch * 2;
  L.ql = o;   o += (size_t)AL_BQ * L.pitch * 2;
  L.qtl = o;  o += (size_t)L.hdp * L.qpitch * 2;
  L.st = o;   o += (size_t)AL_BQ * 16;
  L.tokw = o; o += (size_t)AL_MAX_KV * 4;
  L.red = o;  o += 16;
  L.total = o;                    // <= 43008 + 43520 + 21504 + 23040 + 1024 + 512 + 16 = 132624 bytes
  return L;
}

// rows [r0, r0 + nrows) of a [*, hd] slice -> LDS image [nrows][pitch] and its transpose [hdp][tpitch]; rows >= nvalid and columns >= hd are zero.
// The loads are unconditional (an invalid unit reads the slice's first row and discards it): see attn_maps.hip.
template <bool ALIGNED>
__device__ __forceinline__ void al_stage(const f16* __restrict__ src, int64_t ld, int r0, int nvalid, int nrows, int hd, int hdp, f16* img, int pitch,
                                         f16* timg, int tpitch, int t) {
  const int chunks = hdp >> 3, units = nrows * chunks;
  for (int u0 = t; u0 < units; u0 += 4 * AL_THREADS) {
    f16x8 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = u0 + i * AL_THREADS, row = u / chunks, c = (u - row * chunks) * 8;
      const bool valid = u < units && c < hd && r0 + row < nvalid;
      const f16x8 x = al_load8<ALIGNED>(valid ? src + (int64_t)(r0 + row) * ld + c : src);
      v[i] = valid ? x : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int u = u0 + i * AL_THREADS, row = u / chunks, c = (u - row * chunks) * 8;
      if (u < units) {
        *(f16x8*)(img + row * pitch + c) = v[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) timg[(c + e) * tpitch + row] = v[i][e];
      }
    }
  }
}

template <bool ALIGNED>
__global__ __launch_bounds__(AL_THREADS) void attn_loss_bwd_kernel(const f16* __restrict__ Q, int64_t ldq, const f16* __restrict__ K, int64_t ldk,
                                                                   f16* __restrict__ dQ, int64_t lddq, f16* __restrict__ dK, int64_t lddk,
                                                                   const float* __restrict__ tok_w, const float* __restrict__ g,
                                                                   const float* __restrict__ loss_scale, float* __restrict__ part, int H, int Sq,
                                                                   int Skv, int hd, float scale_log2e, float cfac, int64_t tail) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const AlLds L = al_layout(Skv, hd);
  f16* Kl = reinterpret_cast<f16*>(smem_raw + L.kl);
  f16* Ktl = reinterpret_cast<f16*>(smem_raw + L.ktl);
  f16* Ql = reinterpret_cast<f16*>(smem_raw + L.ql);
  f16* Qtl = reinterpret_cast<f16*>(smem_raw + L.qtl);
  float4* st = reinterpret_cast<float4*>(smem_raw + L.st);
  float* tokw = reinterpret_cast<float*>(smem_raw + L.tokw);
  float* red = reinterpret_cast<float*>(smem_raw + L.red);
  const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nkt = L.nkt, hdp = L.hdp, pitch = L.pitch, kpitch = L.kpitch, qpitch = L.qpitch;
  const int hd16 = (hd + 15) & ~15, ndt = hdp >> 5;
  const int bh = blockIdx.x, b = bh / H, h = bh - b * H;
  const f16* Qg = Q + (int64_t)b * Sq * ldq + h * hd;
  const f16* Kg = K + (int64_t)b * Skv * ldk + h * hd;
  f16* dQg = dQ + (int64_t)b * Sq * lddq + h * hd;
  f16* dKg = dK + (int64_t)b * Skv * lddk + h * hd;
  const float* gb = g + (int64_t)b * Sq;

  if (bh == 0)   // the tail of a slot wider than this layer's B * H: tb_attn_loss_final adds whole slots
    for (int64_t i = t; i < tail; i += AL_THREADS) part[(int64_t)gridDim.x + i] = 0.f;
  int any = 0;
  if (t < AL_MAX_KV) {
    const float w = t < Skv ? tok_w[(int64_t)b * Skv + t] : 0.f;
    tokw[t] = w;
    any = w != 0.f;
  }
  // a sample without a placeholder token: zero loss, and dQ / dK stay as they are, bit for bit
  if (!__syncthreads_or(any)) {
    if (t == 0) part[bh] = 0.f;
    return;
  }
  al_stage<ALIGNED>(Kg, ldk, 0, Skv, nkt * 32, hd, hdp, Kl, pitch, Ktl, kpitch, t);
  const float cf = cfac * (loss_scale ? loss_scale[0] : 1.f);

  const int qh = wave & 1, dpar = wave >> 1;   // phase A: query half, and which of its d-tiles
  f32x16 dkacc[AL_MAX_DT];                     // phase B: key tile `wave`, [d-tile][register]
#pragma unroll
  for (int dt = 0; dt < AL_MAX_DT; ++dt)
#pragma unroll
    for (int r = 0; r < 16; ++r) dkacc[dt][r] = 0.f;
  float lossacc = 0.f;

  for (int s0 = 0; s0 < Sq; s0 += AL_BQ) {
    __syncthreads();                           // the previous block's Q images and statistics have been read
    al_stage<ALIGNED>(Qg, ldq, s0, Sq, AL_BQ, hd, hdp, Ql, pitch, Qtl, qpitch, t);
    __syncthreads();
    // ---- phase A: lane (l31, hi) holds query qh * 32 + l31 and keys kt * 32 + mfma32_row(r, hi)
    {
      f32x16 acc[4];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[kt][r] = 0.f;
      for (int ks = 0; ks < hd16; ks += 16) {
        const f16x8 qf = *(const f16x8*)(Ql + (qh * 32 + l31) * pitch + ks + 8 * hi);
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
          if (kt < nkt) {
            const f16x8 kf = *(const f16x8*)(Kl + (kt * 32 + l31) * pitch + ks + 8 * hi);
            acc[kt] = TB_MFMA_32x32x16(kf, qf, acc[kt]);
          }
      }
      float m = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
        if (kt < nkt)
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (kt * 32 + mfma32_row(r, hi) < Skv) m = fmaxf(m, acc[kt][r]);
      m = fmaxf(m, __shfl_xor(m, 32, 64));     // (key 0 is in the hi = 0 half: finite after the exchange)
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
        if (kt < nkt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const bool ok = kt * 32 + mfma32_row(r, hi) < Skv;
            const float e = ok ? __builtin_amdgcn_exp2f((acc[kt][r] - m) * scale_log2e) : 0.f;
            acc[kt][r] = e;
            sum += e;
          }
      sum += __shfl_xor(sum, 32, 64);
      const float inv = 1.0f / sum;
      float pj = 0.f;
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
        if (kt < nkt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float p = acc[kt][r] * inv;
            acc[kt][r] = p;
            pj = __fmaf_rn(tokw[kt * 32 + mfma32_row(r, hi)], p, pj);
          }
      pj += __shfl_xor(pj, 32, 64);
      const int sq = s0 + qh * 32 + l31;
      const float gq = sq < Sq ? gb[sq] : 0.f;  // a query past the end: w = 0, nothing reaches dK
      if (dpar == 0 && hi == 0) {
        st[qh * 32 + l31] = make_float4(m, inv, pj, gq);
        lossacc = __fmaf_rn(gq, pj, lossacc);
      }
      // w = g_s p_j (tok_w_j - P_J) as three 16-bit terms, already in the A-operand order of dQ = W K
      f16x8 wt[3][4][2];
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
        if (kt < nkt)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const float w = (gq * AL_PRE) * (acc[kt][r] * (tokw[kt * 32 + mfma32_row(r, hi)] - pj));
            f16 a, bb, c;
            al_split3(w, a, bb, c);
            wt[0][kt][r >> 3][r & 7] = a;
            wt[1][kt][r >> 3][r & 7] = bb;
            wt[2][kt][r >> 3][r & 7] = c;
          }
      for (int dt = dpar; dt < ndt; dt += 2) {
        f32x16 o;
#pragma unroll
        for (int r = 0; r < 16; ++r) o[r] = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
          if (kt < nkt)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
              const f16x8 kf = al_perm8(Ktl + (dt * 32 + l31) * kpitch + kt * 32 + 16 * tt + 4 * hi);
#pragma unroll
              for (int term = 0; term < 3; ++term) o = TB_MFMA_32x32x16(wt[term][kt][tt], kf, o);
            }
        // o: query qh * 32 + mfma32_row(r, hi) (rows), head-dim element dt * 32 + l31 (this lane)
        const int d = dt * 32 + l31;
        if (d < hd) {
          float old[16];
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int s = s0 + qh * 32 + mfma32_row(r, hi);
            old[r] = (float)dQg[(int64_t)(s < Sq ? s : Sq - 1) * lddq + d];
          }
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int s = s0 + qh * 32 + mfma32_row(r, hi);
            const float add = cf * o[r];
            if (s < Sq && add != 0.f) dQg[(int64_t)s * lddq + d] = (f16)(old[r] + add);   // (a zero addend stores nothing: -0 stays -0)
          }
        }
      }
    }
    __syncthreads();                           // the block's statistics are in LDS
    // ---- phase B: lane (l31, hi) holds key wave * 32 + l31 and queries sub * 32 + mfma32_row(r, hi)
    if (wave < nkt) {
      const int key = wave * 32 + l31;
      const bool kvalid = key < Skv;
      const float tw = tokw[key & (AL_MAX_KV - 1)];
      for (int sub = 0; sub < 2; ++sub) {
        if (s0 + sub * 32 >= Sq) break;
        f32x16 sacc;
#pragma unroll
        for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
        for (int ks = 0; ks < hd16; ks += 16) {
          const f16x8 qf = *(const f16x8*)(Ql + (sub * 32 + l31) * pitch + ks + 8 * hi);
          const f16x8 kf = *(const f16x8*)(Kl + (wave * 32 + l31) * pitch + ks + 8 * hi);
          sacc = TB_MFMA_32x32x16(qf, kf, sacc);
        }
        f16x8 wt[3][2];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float4 s4 = st[sub * 32 + mfma32_row(r, hi)];   // (m, 1 / sum, P_J, g) of the query
          const float p = kvalid ? __builtin_amdgcn_exp2f((sacc[r] - s4.x) * scale_log2e) * s4.y : 0.f;
          const float w = (s4.w * AL_PRE) * (p * (tw - s4.z));
          f16 a, bb, c;
          al_split3(w, a, bb, c);
          wt[0][r >> 3][r & 7] = a;
          wt[1][r >> 3][r & 7] = bb;
          wt[2][r >> 3][r & 7] = c;
        }
#pragma unroll
        for (int dt = 0; dt < AL_MAX_DT; ++dt)
          if (dt < ndt)
#pragma unroll
            for (int tt = 0; tt < 2; ++tt) {
              const f16x8 qf = al_perm8(Qtl + (dt * 32 + l31) * qpitch + sub * 32 + 16 * tt + 4 * hi);
#pragma unroll
              for (int term = 0; term < 3; ++term) dkacc[dt] = TB_MFMA_32x32x16(wt[term][tt], qf, dkacc[dt]);
            }
      }
    }
  }
  // ---- dK: key wave * 32 + mfma32_row(r, hi) (rows), head-dim element dt * 32 + l31 (this lane)
  if (wave < nkt) {
#pragma unroll
    for (int dt = 0; dt < AL_MAX_DT; ++dt) {
      const int d = dt * 32 + l31;
      if (dt < ndt && d < hd) {
        float old[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = wave * 32 + mfma32_row(r, hi);
          old[r] = (float)dKg[(int64_t)(key < Skv ? key : 0) * lddk + d];
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = wave * 32 + mfma32_row(r, hi);
          const float add = cf * dkacc[dt][r];
          if (key < Skv && add != 0.f) dKg[(int64_t)key * lddk + d] = (f16)(old[r] + add);
        }
      }
    }
  }
  // ---- sum_s g_s P_J of this (batch, head), over 1 / H: waves 0 and 1 hold the terms
  lossacc = wave_sum(lossacc);
  if (lane == 0) red[wave] = lossacc;
  __syncthreads();
  if (t == 0) part[bh] = (red[0] + red[1]) / (float)H;
}

// One workgroup per sample.  m = box mean (f x f) of the target, fg = sum m, bg = n - fg, g = (1 - m) / max(bg, 1) - m / max(fg, 1): sums and
// the quotient in double in a fixed order, one rounding to fp32 at the end.
__global__ __launch_bounds__(256) void attn_loss_coef_kernel(const float* __restrict__ target, int h, int w, int f, float* __restrict__ g) {
  __shared__ double redd[4];
  const int b = blockIdx.x, oh = h / f, ow = w / f, n = oh * ow;
  const float* tb = target + (int64_t)b * h * w;
  const double inv_area = 1.0 / ((double)f * (double)f);
  double fg = 0.0;
  for (int s = threadIdx.x; s < n; s += 256) {
    const int oy = s / ow, ox = s - oy * ow;
    double a = 0.0;
    for (int y = 0; y < f; ++y)
      for (int x = 0; x < f; ++x) a += (double)tb[(int64_t)(oy * f + y) * w + ox * f + x];
    fg += a * inv_area;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) fg += __shfl_xor(fg, o, 64);
  if ((threadIdx.x & 63) == 0) redd[threadIdx.x >> 6] = fg;
  __syncthreads();
  fg = (redd[0] + redd[1]) + (redd[2] + redd[3]);
  const double bg = (double)n - fg;
  const double ifg = 1.0 / (fg > 1.0 ? fg : 1.0), ibg = 1.0 / (bg > 1.0 ? bg : 1.0);
  for (int s = threadIdx.x; s < n; s += 256) {
    const int oy = s / ow, ox = s - oy * ow;
    double a = 0.0;
    for (int y = 0; y < f; ++y)
      for (int x = 0; x < f; ++x) a += (double)tb[(int64_t)(oy * f + y) * w + ox * f + x];
    const double m = a * inv_area;
    g[(int64_t)b * n + s] = (float)((1.0 - m) * ibg - m * ifg);
  }
}

// One wave: lane l adds elements l, l + 64, ... in double, then the lanes meet in a fixed order.
__global__ __launch_bounds__(64) void attn_loss_final_kernel(const float* __restrict__ part, int64_t n, float norm, float* __restrict__ out) {
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += 64) acc += (double)part[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (threadIdx.x == 0) out[0] = (float)(acc * (double)norm);
}

}  // namespace

extern "C" int tb_attn_loss_coef(const float* target, int B, int h, int w, int f, float* g, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!target || !g || B < 1 || B > 65535 || h < 1 || w < 1 || f < 1 || f > 64 || h % f || w % f) return TB_EINVAL;
  if ((int64_t)h * w > (1 << 30)) return TB_EINVAL;
  hipLaunchKernelGGL(attn_loss_coef_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, target, h, w, f, g);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int64_t tb_attn_loss_workspace_bytes(int B, int H, int n_slots) {
  if (B < 1 || H < 1 || n_slots < 1) return TB_EINVAL;
  return (int64_t)n_slots * B * H * (int64_t)sizeof(float);
}

extern "C" int tb_attn_loss_bwd(const tb_attn_desc* d, int dtype, const float* tok_w, const float* g, float coef, const float* loss_scale,
                                float* ws, int64_t ws_bytes, int slot, int64_t slot_floats, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!d || !d->Q || !d->K || !d->dQ || !d->dK || !tok_w || !g || !ws || dtype != TB_F16) return TB_EINVAL;
  if (d->B < 1 || d->H < 1 || d->Sq < 1 || d->Skv < 1 || d->Skv > AL_MAX_KV) return TB_EINVAL;
  if (d->hd < 8 || d->hd % 8 != 0 || d->hd > 160) return TB_EINVAL;
  const int64_t C = (int64_t)d->H * d->hd, BH = (int64_t)d->B * d->H;
  if (d->ldq < C || d->ldk < C || d->lddq < C || d->lddk < C || BH > 0x7fffffff) return TB_EINVAL;
  if (slot < 0 || slot_floats < BH || ws_bytes < ((int64_t)slot + 1) * slot_floats * (int64_t)sizeof(float)) return TB_EINVAL;
  if (!(coef == coef)) return TB_EINVAL;
  const AlLds L = al_layout(d->Skv, d->hd);
  const bool aligned = (((uintptr_t)d->Q | (uintptr_t)d->K) & 15) == 0 && d->ldq % 8 == 0 && d->ldk % 8 == 0;
  static bool attr_done = false;
  if (!attr_done) {
    if (hipFuncSetAttribute((const void*)attn_loss_bwd_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)attn_loss_bwd_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, 136 * 1024) != hipSuccess)
      return TB_ELAUNCH;
    attr_done = true;
  }
  float* part = ws + (int64_t)slot * slot_floats;
  hipStream_t s = (hipStream_t)stream;
  const float scale_log2e = d->scale * 1.4426950408889634f;
  const float cfac = (float)((double)coef * (double)d->scale / ((double)d->H * (double)AL_PRE));
  if (aligned)
    hipLaunchKernelGGL(attn_loss_bwd_kernel<true>, dim3((unsigned)BH), dim3(AL_THREADS), L.total, s, (const f16*)d->Q, d->ldq, (const f16*)d->K,
                       d->ldk, (f16*)d->dQ, d->lddq, (f16*)d->dK, d->lddk, tok_w, g, loss_scale, part, d->H, d->Sq, d->Skv, d->hd, scale_log2e, cfac,
                       slot_floats - BH);
  else
    hipLaunchKernelGGL(attn_loss_bwd_kernel<false>, dim3((unsigned)BH), dim3(AL_THREADS), L.total, s, (const f16*)d->Q, d->ldq, (const f16*)d->K,
                       d->ldk, (f16*)d->dQ, d->lddq, (f16*)d->dK, d->lddk, tok_w, g, loss_scale, part, d->H, d->Sq, d->Skv, d->hd, scale_log2e, cfac,
                       slot_floats - BH);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_attn_loss_final(const float* ws, int n_slots, int64_t slot_floats, float norm, float* out, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!ws || !out || n_slots < 1 || slot_floats < 1) return TB_EINVAL;
  hipLaunchKernelGGL(attn_loss_final_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, ws, (int64_t)n_slots * slot_floats, norm, out);
  TB_CHECK_LAUNCH();
  return TB_OK;
}
