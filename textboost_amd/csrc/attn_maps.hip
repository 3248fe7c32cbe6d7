// Token attention maps: the cross-attention PROBABILITIES the flash forward never materialises, summed over heads, one image per prompt token.
//     maps[b - b0][j][s] (+)= w * sum_h softmax_j(scale * q_{b,h,s} . k_{b,h,j})            fp32 [nb, Skv, Sq]
// The kernel computes its own softmax (all keys of a query fit one tile, Skv <= 128), so it depends neither on the forward's LSE nor on which
// forward variant ran.  One workgroup (two waves) owns 64 queries of one image for ALL heads and ALL keys: no atomics, `accumulate` is a
// read-modify-write by the owner, and a launch is bit-reproducible.
//
// Tile plan.  Per head the workgroup stages K_h [32 * ceil(Skv / 32)][hd] and Q_h [64][hd] into LDS (zero rows / zero columns up to the next
// multiple of 16 of hd; 16-byte loads when every operand row is 16-byte aligned, a 2-byte-load instance otherwise: any ldq / ldk).  Each wave computes
// S^T = K Q^T for its 32 queries as up to four 32 x 32 MFMA tiles (A = K rows, B = Q rows, both read "row with the contraction index
// contiguous"): the accumulator then holds the QUERY on the lane and the KEYS in the registers, so max and sum over the keys are in-lane
// reductions over <= 64 registers plus one exchange between the two lane halves, and a store of one register is 32 consecutive floats of
// one token's image.  Probabilities and the head sum never leave fp32 registers; the denominator is summed with compensation (below).
#include "common.h"
#include "../../include/textboost_hip.h"

namespace {

constexpr int AM_BQ = 64;        // queries per workgroup (32 per wave)
constexpr int AM_MAX_KV = 128;   // keys: at most four 32-row tiles
constexpr int AM_THREADS = 128;

// 8 halfs of a row: one 16-byte load when every row of the operands is 16-byte aligned (ALIGNED, decided by the host), 2-byte loads otherwise
template <bool ALIGNED>
__device__ __forceinline__ f16x8 load8(const f16* src) {
  if constexpr (ALIGNED) return *(const f16x8*)src;
  f16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = src[e];
  return v;
}

template <bool ALIGNED>
__global__ __launch_bounds__(AM_THREADS) void attn_token_maps_kernel(const f16* __restrict__ Q, int64_t ldq, const f16* __restrict__ K, int64_t ldk,
                                                                     float* __restrict__ maps, int H, int Sq, int Skv, int hd, float scale_log2e,
                                                                     int b0, float w, int accumulate) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nkt = (Skv + 31) >> 5;                 // key tiles (1..4)
  const int hdp = (hd + 15) & ~15, chunks = hdp >> 3;
  const int pitch = hdp + 8;                       // halfs: rows of 32 m + 16 bytes, 16-byte aligned
  f16* Kl = reinterpret_cast<f16*>(smem_raw);      // [nkt * 32][pitch]
  f16* Ql = Kl + nkt * 32 * pitch;                 // [AM_BQ][pitch]
  const int nrows = nkt * 32 + AM_BQ;
  const int bi = blockIdx.y, b = b0 + bi, s0 = blockIdx.x * AM_BQ;
  const f16* Qg = Q + (int64_t)b * Sq * ldq;
  const f16* Kg = K + (int64_t)b * Skv * ldk;

  f32x16 msum[4];                                  // sum over heads of the probabilities: [key tile][register]
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int r = 0; r < 16; ++r) msum[kt][r] = 0.f;

  for (int h = 0; h < H; ++h) {
    __syncthreads();                               // the previous head's fragments have been read
    // K rows and Q rows are one LDS image [nkt * 32 + AM_BQ][pitch]: one loop over (row, 8-half chunk) units, four loads in flight per thread.
    // The loads are unconditional (a unit that loads nothing reads the image's first K row and discards it): a branch around a load makes
    // the compiler wait for it before the next one, and the loop then pays the global latency once per unit.
    for (int u0 = t; u0 < nrows * chunks; u0 += 4 * AM_THREADS) {
      f16x8 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int u = u0 + i * AM_THREADS, row = u / chunks, c = (u - row * chunks) * 8, qrow = s0 + row - nkt * 32;
        const bool isk = row < Skv, isq = row >= nkt * 32 && qrow < Sq;
        const bool valid = u < nrows * chunks && c < hd && (isk || isq);
        const f16* src = isk ? Kg + (int64_t)row * ldk + h * hd + c : Qg + (int64_t)qrow * ldq + h * hd + c;
        const f16x8 x = load8<ALIGNED>(valid ? src : Kg);
        v[i] = valid ? x : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int u = u0 + i * AM_THREADS, row = u / chunks, c = (u - row * chunks) * 8;
        if (u < nrows * chunks) *(f16x8*)(Kl + row * pitch + c) = v[i];
      }
    }
    __syncthreads();
    // S^T tiles: lane (l31, hi) ends with query wave * 32 + l31 and keys kt * 32 + mfma32_row(r, hi)
    f32x16 acc[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[kt][r] = 0.f;
    for (int ks = 0; ks < hdp; ks += 16) {
      const f16x8 qf = *(const f16x8*)(Ql + (wave * 32 + l31) * pitch + ks + 8 * hi);
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
        if (kt < nkt) {
          const f16x8 kf = *(const f16x8*)(Kl + (kt * 32 + l31) * pitch + ks + 8 * hi);
          acc[kt] = TB_MFMA_32x32x16(kf, qf, acc[kt]);
        }
    }
    // softmax over the keys of this lane's query (keys >= Skv masked)
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
      if (kt < nkt)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kt * 32 + mfma32_row(r, hi) < Skv) m = fmaxf(m, acc[kt][r]);
    m = fmaxf(m, __shfl_xor(m, 32, 64));           // (Skv >= 1: key 0 is in the hi = 0 half, so m is finite after the exchange)
    // The denominator as an unevaluated pair sum_hi + sum_lo (TwoSum per term, then across the two lane halves: both halves end with the same
    // pair), and each probability corrected by its residual e - p * sum: a plain fp32 sum of up to 128 terms and one rounded reciprocal put
    // the SAME relative error (1e-7 measured) on every probability of a query, which shows as sum_j p_j != 1.
    float s = 0.f, c = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
      if (kt < nkt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const bool ok = kt * 32 + mfma32_row(r, hi) < Skv;
          const float e = ok ? __builtin_amdgcn_exp2f((acc[kt][r] - m) * scale_log2e) : 0.f;
          acc[kt][r] = e;
          const float ts = s + e, bp = ts - s;
          c += (s - (ts - bp)) + (e - bp);
          s = ts;
        }
    {
      const float s2 = __shfl_xor(s, 32, 64), c2 = __shfl_xor(c, 32, 64);
      const float ts = s + s2, bp = ts - s;
      c = (c + c2) + ((s - (ts - bp)) + (s2 - bp));
      s = ts;
    }
    const float sum_hi = s + c, sum_lo = (s - sum_hi) + c;
    const float inv = 1.0f / sum_hi;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
      if (kt < nkt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float e = acc[kt][r], p = e * inv;
          const float res = __fmaf_rn(-p, sum_lo, __fmaf_rn(-p, sum_hi, e));
          msum[kt][r] += __fmaf_rn(res, inv, p);
        }
  }
  // epilogue: one register = 32 consecutive queries of one token's image.  (w * sum) is rounded BEFORE it is added to the old value, so two
  // accumulating launches on zeros give exactly twice one overwriting launch.
  const int s = s0 + wave * 32 + l31;
  if (s < Sq) {
    float* out = maps + (int64_t)bi * Skv * Sq + s;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
      if (kt < nkt) {
        float old[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) old[r] = 0.f;
        if (accumulate) {   // the tile's 16 old values in flight together (a masked-off key re-reads key 0's)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int key = kt * 32 + mfma32_row(r, hi);
            old[r] = out[(int64_t)(key < Skv ? key : 0) * Sq];
          }
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kt * 32 + mfma32_row(r, hi);
          if (key < Skv) out[(int64_t)key * Sq] = __fadd_rn(old[r], __fmul_rn(w, msum[kt][r]));
        }
      }
  }
}

}  // namespace

extern "C" int tb_attn_token_maps(const tb_attn_desc* d, int dtype, int b0, int nb, float w, int accumulate, float* maps, tb_stream_t stream) {
  if (!d || !maps || !d->Q || !d->K || dtype != TB_F16) return TB_EINVAL;
  if (d->B < 1 || d->H < 1 || d->Sq < 1 || d->Skv < 1 || d->Skv > AM_MAX_KV) return TB_EINVAL;
  if (d->hd < 8 || d->hd % 8 != 0 || d->hd > 160) return TB_EINVAL;
  if (b0 < 0 || nb < 1 || (int64_t)b0 + nb > d->B || (accumulate != 0 && accumulate != 1)) return TB_EINVAL;
  const int64_t C = (int64_t)d->H * d->hd;
  if (d->ldq < C || d->ldk < C) return TB_EINVAL;
  const int64_t qblocks = ((int64_t)d->Sq + AM_BQ - 1) / AM_BQ;
  if (qblocks > 0x7fffffff || nb > 65535) return TB_EINVAL;
  const int nkt = (d->Skv + 31) / 32, hdp = (d->hd + 15) & ~15;
  const size_t lds = (size_t)(nkt * 32 + AM_BQ) * (hdp + 8) * sizeof(f16);   // <= 192 * 168 * 2 = 64512 bytes
  // every (row, 8-half chunk) of Q and K 16-byte aligned?  (hd % 8 == 0: the chunks are, when the rows are)
  const bool aligned = (((uintptr_t)d->Q | (uintptr_t)d->K) & 15) == 0 && d->ldq % 8 == 0 && d->ldk % 8 == 0;
  const dim3 grid((unsigned)qblocks, (unsigned)nb);
  const float scale_log2e = d->scale * 1.4426950408889634f;
  if (aligned)
    hipLaunchKernelGGL(attn_token_maps_kernel<true>, grid, dim3(AM_THREADS), lds, (hipStream_t)stream, (const f16*)d->Q, d->ldq, (const f16*)d->K,
                       d->ldk, maps, d->H, d->Sq, d->Skv, d->hd, scale_log2e, b0, w, accumulate);
  else
    hipLaunchKernelGGL(attn_token_maps_kernel<false>, grid, dim3(AM_THREADS), lds, (hipStream_t)stream, (const f16*)d->Q, d->ldq, (const f16*)d->K,
                       d->ldk, maps, d->H, d->Sq, d->Skv, d->hd, scale_log2e, b0, w, accumulate);
  TB_CHECK_LAUNCH();
  return TB_OK;
}
