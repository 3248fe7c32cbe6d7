// Regional cross-attention forward: tb_attention_fwd's O = softmax(scale Q K^T + m) V for a short key sequence (the prompt, Skv <= 128) with a
// region mask m in {0, -inf} that is never materialised:
//     m[s][j] = 0     if key_region[b][j] < 0                               (the key is unrestricted)
//             = 0     if bit key_region[b][j] of query_regions[s] is set    (query s lies inside the key's region)
//             = -inf  otherwise                                             (the probability is an exact zero)
// One workgroup (four waves) owns qtiles * 128 queries of one (batch, head).  The K image [keys][hd] and the TRANSPOSED V image [hd][keys] of
// ALL keys are staged once (zero rows / columns up to the tile sizes; 16-byte loads when every operand row is 16-byte aligned, a 2-byte
// instance otherwise), beside one shift count per key: the region index, 32 for an unrestricted key, 33 for a key past Skv.  Each wave walks
// its 32-query tiles with no barrier: S^T = K Q^T on the 32 x 32 x 16 MFMA puts the QUERY on the lane and the KEYS in the registers, so the
// mask is one 32-bit load per lane (the query's region bits, bit 32 set on top) and one 64-bit shift + select per score, the softmax is a
// single in-lane pass plus one exchange between the two lane halves, and O^T = V^T P^T takes P from the same registers.  The keys of the V^T
// image are stored in the order the accumulator registers hold them (vt_pos), so a V^T fragment is one 16-byte LDS read.
// No atomics; every output element has one owner and depends on its own query only: a repeated launch is bit-identical, and rows whose
// query lies outside a key's region do not depend on that key's K / V rows at all (p = 0 exactly, 0 * v adds nothing).
// The key-tile count and the head-dim steps are RUN-TIME guards around statically unrolled tile loops (three instances by head dim).  Making
// them template parameters was tried: the compiler then hoists the loop-invariant K fragments out of the query-tile loop and spills
// (100 .. 950 bytes of scratch per lane in every instance), so the guards stay; DESIGN.md 19 states what they cost.
#include "common.h"
#include "../../include/textboost_hip.h"

#include <vector>

namespace {

constexpr int RA_MAX_KV = 128;   // keys: at most four 32-row tiles
constexpr int RA_THREADS = 256;  // four waves, 32 queries each per tile
constexpr float RA_LOG2E = 1.4426950408889634f;
constexpr int RA_SH_FREE = 32, RA_SH_NONE = 33;   // shift counts of an unrestricted key / of no key (bit 33 of the query word is never set)

template <bool ALIGNED>
__device__ __forceinline__ f16x8 ra_load8(const f16* src) {
  if constexpr (ALIGNED) return *(const f16x8*)src;
  f16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = src[e];
  return v;
}

// position of key j inside its group of 16 in the V^T image: the contraction index 8 * hi + e of the MFMA's B operand (P) is accumulator
// register 8 * jj + e, i.e. key 16 * jj + 8 * (e >> 2) + 4 * hi + (e & 3)
__device__ __forceinline__ int vt_pos(int j) { return (j & ~15) + 8 * ((j >> 2) & 1) + 4 * ((j >> 3) & 1) + (j & 3); }

template <int DT, bool ALIGNED>
__global__ __launch_bounds__(RA_THREADS) void attn_region_fwd_kernel(const tb_attn_desc p, const int32_t* __restrict__ key_region,
                                                                     const uint32_t* __restrict__ query_regions, int qtiles, int bands, int remap) {
  constexpr int KS = 2 * DT;                       // 16-wide contraction steps of the head dim
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int nkt = (p.Skv + 31) >> 5;               // key tiles (1..4)
  const int hd = p.hd, hdp = (hd + 15) & ~15, dt = (hd + 31) >> 5;
  const int kpitch = hdp + 8, vpitch = nkt * 32 + 8;   // halfs: rows of 32 m + 16 bytes
  f16* Kl = reinterpret_cast<f16*>(smem_raw);      // [nkt * 32][kpitch]
  f16* Vt = Kl + nkt * 32 * kpitch;                // [DT * 32][vpitch]
  int* shl = reinterpret_cast<int*>(Vt + DT * 32 * vpitch);   // [nkt * 32]
  // workgroup -> (query band, head, batch): the H heads of one band read and write the same cache lines of Q and O, so with `remap` XCD i
  // takes the (band, batch) pairs i, i + 8, .. and runs their heads back to back (the pairing of the short-key flash forward)
  int b, h, band;
  {
    const int lin = blockIdx.x, H = p.H;
    int xb;
    if (remap) {
      const int xcd = lin & 7, k = lin >> 3;
      xb = (k / H) * 8 + xcd;
      h = k - (k / H) * H;
    } else {
      xb = lin / H;
      h = lin - xb * H;
    }
    band = xb % bands;
    b = xb / bands;
  }
  const int qblk = band * 128 * qtiles;
  const f16* Qg = (const f16*)p.Q + (int64_t)b * p.Sq * p.ldq + h * hd;
  const f16* Kg = (const f16*)p.K + (int64_t)b * p.Skv * p.ldk + h * hd;
  const f16* Vg = (const f16*)p.V + (int64_t)b * p.Skv * p.ldv + h * hd;

  auto load_q = [&](f16x8 (&qf)[KS], int q) {
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int c = 16 * j + 8 * hi;
      const bool valid = q < p.Sq && c < hd;
      const f16x8 x = ra_load8<ALIGNED>(valid ? Qg + (int64_t)q * p.ldq + c : Kg);
      qf[j] = valid ? x : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
  };
  // the first tile's Q fragments are requested before the staging: their latency hides under it
  f16x8 qf[KS];
  load_q(qf, qblk + wave * 32 + l31);
  uint32_t qbits;
  {
    const int q = qblk + wave * 32 + l31;
    qbits = query_regions[q < p.Sq ? q : 0];
  }

  // ---- staging: K rows, V columns, shift counts.  Loads are unconditional (an invalid unit re-reads the first K row and discards it)
  {
    const int kchunks = hdp >> 3, nk = nkt * 32 * kchunks;
    for (int u0 = t; u0 < nk; u0 += 4 * RA_THREADS) {
      f16x8 v[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int u = u0 + i * RA_THREADS, row = u / kchunks, c = (u - row * kchunks) * 8;
        const bool valid = u < nk && row < p.Skv && c < hd;
        const f16x8 x = ra_load8<ALIGNED>(valid ? Kg + (int64_t)row * p.ldk + c : Kg);
        v[i] = valid ? x : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int u = u0 + i * RA_THREADS, row = u / kchunks, c = (u - row * kchunks) * 8;
        if (u < nk) *(f16x8*)(Kl + row * kpitch + c) = v[i];
      }
    }
    // V: consecutive threads take consecutive KEYS of one 8-column chunk, so the eight 2-byte stores of a wave go to 16 different keys' slots
    constexpr int vchunks = DT * 4;
    const int nv = nkt * 32 * vchunks;
    for (int u0 = t; u0 < nv; u0 += 2 * RA_THREADS) {
      f16x8 v[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int u = u0 + i * RA_THREADS, ch = u / (nkt * 32), row = u - ch * (nkt * 32), c = ch * 8;
        const bool valid = u < nv && row < p.Skv && c < hd;
        const f16x8 x = ra_load8<ALIGNED>(valid ? Vg + (int64_t)row * p.ldv + c : Kg);
        v[i] = valid ? x : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int u = u0 + i * RA_THREADS, ch = u / (nkt * 32), row = u - ch * (nkt * 32), c = ch * 8;
        if (u < nv) {
          f16* dst = Vt + c * vpitch + vt_pos(row);
#pragma unroll
          for (int e = 0; e < 8; ++e) dst[e * vpitch] = v[i][e];
        }
      }
    }
    if (t < nkt * 32) {
      int sh = RA_SH_NONE;
      if (t < p.Skv) {
        const int kr = key_region[(int64_t)b * p.Skv + t];
        sh = kr < 0 ? RA_SH_FREE : (kr < 32 ? kr : RA_SH_NONE);
      }
      shl[t] = sh;
    }
  }
  __syncthreads();

  const float c2 = p.scale * RA_LOG2E;             // scores go to the log2 domain in fp32, after the MFMA
  for (int qt = 0; qt < qtiles; ++qt) {
    const int q = qblk + (qt * 4 + wave) * 32 + l31;
    const uint64_t qword = (uint64_t)qbits | (1ull << 32);
    // S^T tiles: lane (l31, hi) ends with query q and keys kt * 32 + mfma32_row(r, hi)
    f32x16 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kt][r] = 0.f;
#pragma unroll
    for (int j = 0; j < KS; ++j)
      if (16 * j < hdp) {
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
          if (kt < nkt) {
            const f16x8 kf = *(const f16x8*)(Kl + (kt * 32 + l31) * kpitch + 16 * j + 8 * hi);
            s[kt] = TB_MFMA_32x32x16(kf, qf[j], s[kt]);
          }
      }
    // the next tile's Q fragments and region bits, under this tile's softmax
    if (qt + 1 < qtiles) {
      const int qn = q + 128;
      load_q(qf, qn);
      qbits = query_regions[qn < p.Sq ? qn : 0];
    }
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
      if (kt < nkt)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int4 sh = *(const int4*)(shl + kt * 32 + 8 * g + 4 * hi);   // keys mfma32_row(4 g .. 4 g + 3, hi)
          const int shv[4] = {sh.x, sh.y, sh.z, sh.w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const bool ok = (qword >> shv[e]) & 1;   // (unsigned: bit 31 is a region like any other)
            const float v = ok ? s[kt][4 * g + e] * c2 : -INFINITY;
            s[kt][4 * g + e] = v;
            mx = fmaxf(mx, v);
          }
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mref = mx == -INFINITY ? 0.f : mx;   // a query with every key masked: all p = exp2(-inf) = 0, no NaN
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
      if (kt < nkt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pv = __builtin_amdgcn_exp2f(s[kt][r] - mref);
          s[kt][r] = pv;
          l += pv;
        }
    f32x16 o[DT];
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[d][r] = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
      if (kt < nkt) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          f16x8 pf;
#pragma unroll
          for (int e = 0; e < 8; ++e) pf[e] = (f16)s[kt][8 * jj + e];
#pragma unroll
          for (int d = 0; d < DT; ++d)
            if (d < dt) {
              const f16x8 vf = *(const f16x8*)(Vt + (d * 32 + l31) * vpitch + kt * 32 + 16 * jj + 8 * hi);
              o[d] = TB_MFMA_32x32x16(vf, pf, o[d]);
            }
        }
      }
    l += __shfl_xor(l, 32, 64);
    if (q < p.Sq) {
      const float inv = l > 0.f ? 1.f / l : 0.f;
      f16* Og = (f16*)p.O + ((int64_t)b * p.Sq + q) * p.ldo + h * hd;
#pragma unroll
      for (int d = 0; d < DT; ++d)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int col = d * 32 + 8 * r4 + 4 * hi;   // 4 consecutive head-dim columns
          if (col < hd) {
            f16x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (f16)(o[d][4 * r4 + e] * inv);
            if constexpr (ALIGNED) {
              *(f16x4*)(Og + col) = v;
            } else {
#pragma unroll
              for (int e = 0; e < 4; ++e) Og[col + e] = v[e];
            }
          }
        }
      if (p.LSE && hi == 0) p.LSE[((int64_t)b * p.H + h) * p.Sq + q] = l > 0.f ? mx * (1.f / RA_LOG2E) + logf(l) : -INFINITY;
    }
  }
}

template <int DT>
int ra_launch(const tb_attn_desc& d, const int32_t* key_region, const uint32_t* query_regions, bool aligned, int qtiles, int bands, int remap,
              size_t lds, unsigned grid, hipStream_t s) {
  static bool attr_done = false;   // (per DT: one static per instantiation)
  if (!attr_done) {
    if (hipFuncSetAttribute((const void*)attn_region_fwd_kernel<DT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)attn_region_fwd_kernel<DT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess)
      return TB_ELAUNCH;
    attr_done = true;
  }
  if (aligned)
    hipLaunchKernelGGL((attn_region_fwd_kernel<DT, true>), dim3(grid), dim3(RA_THREADS), lds, s, d, key_region, query_regions, qtiles, bands, remap);
  else
    hipLaunchKernelGGL((attn_region_fwd_kernel<DT, false>), dim3(grid), dim3(RA_THREADS), lds, s, d, key_region, query_regions, qtiles, bands, remap);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

}  // namespace

extern "C" int tb_attention_region_fwd(const tb_attn_desc* d, int dtype, const int32_t* key_region, const uint32_t* query_regions,
                                       tb_stream_t stream) {
  (void)hipGetLastError();
  if (!d || !d->Q || !d->K || !d->V || !d->O || !key_region || !query_regions || dtype != TB_F16 || d->causal != 0) return TB_EINVAL;
  if (d->B < 1 || d->H < 1 || d->Sq < 1 || d->Skv < 1 || d->Skv > RA_MAX_KV) return TB_EINVAL;
  if (d->hd < 8 || d->hd % 8 != 0 || d->hd > 160) return TB_EINVAL;
  const int64_t C = (int64_t)d->H * d->hd;
  if (d->ldq < C || d->ldk < C || d->ldv < C || d->ldo < C) return TB_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  // The region indices live on the device.  Outside a stream capture they are read back and checked (a few KB behind the work already queued
  // on the stream); inside one nothing may synchronise, and the kernel itself treats an index >= 32 as a region no query belongs to.
  {
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess) return TB_ELAUNCH;
    if (cap == hipStreamCaptureStatusNone) {
      std::vector<int32_t> host((size_t)d->B * d->Skv);
      if (hipMemcpyAsync(host.data(), key_region, host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
          hipStreamSynchronize(s) != hipSuccess) {
        tb_last_hip_error_code_ = (int)hipGetLastError();
        return TB_ELAUNCH;
      }
      for (int32_t r : host)
        if (r >= 32) return TB_EINVAL;
    }
  }
  // queries per workgroup: 512 / 256 while that still leaves two workgroups per CU, else 128
  const int64_t BH = (int64_t)d->B * d->H;
  int qtiles = 4;
  while (qtiles > 1 && (((int64_t)d->Sq + 128 * qtiles - 1) / (128 * qtiles)) * BH < 512) qtiles >>= 1;
  const int64_t bands = ((int64_t)d->Sq + 128 * qtiles - 1) / (128 * qtiles);
  if (bands * BH > 0x7fffffff) return TB_EINVAL;
  const int remap = ((bands * d->B) & 7) == 0;
  const int nkt = (d->Skv + 31) / 32, hdp = (d->hd + 15) & ~15;
  const int DT = d->hd <= 64 ? 2 : (d->hd <= 96 ? 3 : 5);
  const size_t lds = ((size_t)nkt * 32 * (hdp + 8) + (size_t)DT * 32 * (nkt * 32 + 8)) * sizeof(f16) + (size_t)nkt * 32 * sizeof(int);   // <= 87040 bytes
  const bool aligned = (((uintptr_t)d->Q | (uintptr_t)d->K | (uintptr_t)d->V | (uintptr_t)d->O) & 15) == 0 && d->ldq % 8 == 0 && d->ldk % 8 == 0 &&
                       d->ldv % 8 == 0 && d->ldo % 8 == 0;
  const unsigned grid = (unsigned)(bands * BH);
  if (DT == 2) return ra_launch<2>(*d, key_region, query_regions, aligned, qtiles, (int)bands, remap, lds, grid, s);
  if (DT == 3) return ra_launch<3>(*d, key_region, query_regions, aligned, qtiles, (int)bands, remap, lds, grid, s);
  return ra_launch<5>(*d, key_region, query_regions, aligned, qtiles, (int)bands, remap, lds, grid, s);
}
