// Two-term short-key attention forward (prompt-to-prompt editing):
//     O = softmax(scale1 Q1 K1^T) V1 + softmax(scale2 Q2 K2^T) V2
// Each softmax is normalised over its own keys (Skv <= 128 per term), the sum is taken in fp32 and rounded once.  The second term is optional.
// The structure is csrc/region_attn.hip's: one workgroup (four waves) owns 128 queries of one (batch, head); the K image [keys][hd] and the
// TRANSPOSED V image [hd][keys] of ALL keys of a term sit in LDS (zero rows / columns up to the tile sizes; 16-byte loads when every operand row
// is 16-byte aligned, a 2-byte instance otherwise); S^T = K Q^T on the 32 x 32 x 16 MFMA puts the QUERY on the lane and the KEYS in the
// registers, so the softmax is a single in-lane pass plus one exchange between the two lane halves, and O^T = V^T P^T takes P from the same
// registers.  The keys of the V^T image are stored in the order the accumulator registers hold them (vt_pos): a V^T fragment is one 16-byte
// LDS read.
// The two terms are two PHASES over the same LDS: four key images at hd = 160 would not fit a CU.  Phase 1 restages K2 / V2 over K1 / V1
// behind a barrier; the fp32 O accumulators stay live across the phases, which is why a wave owns ONE 32-query tile (region_attn.hip walks
// up to four: its accumulators die with each tile).  P is normalised (p / l) BEFORE it is rounded to 16 bits, so both terms accumulate into
// the same registers with no rescaling and the output is one rounding of the fp32 sum.
// No atomics; every output element has one owner and depends on its own query only: a repeated launch is bit-identical.  Nothing is read
// back to the host.  As in region_attn.hip the key-tile count and the head-dim steps are run-time guards around statically unrolled loops.
#include "common.h"
#include "../../include/textboost_hip.h"

namespace {

constexpr int PA_MAX_KV = 128;   // keys per term: at most four 32-row tiles
constexpr int PA_THREADS = 256;  // four waves, 32 queries each
constexpr float PA_LOG2E = 1.4426950408889634f;

struct pa_term {
  const f16* Q;
  const f16* K;
  const f16* V;
  int64_t ldq, ldk, ldv;
  int Skv;
  float scale;
};

struct pa_args {
  pa_term t0, t1;
  f16* O;
  int64_t ldo;
  int B, H, Sq, hd, nterms, bands, remap;
};

template <bool ALIGNED>
__device__ __forceinline__ f16x8 pa_load8(const f16* src) {
  if constexpr (ALIGNED) return *(const f16x8*)src;
  f16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = src[e];
  return v;
}

// position of key j inside its group of 16 in the V^T image: the contraction index 8 * hi + e of the MFMA's B operand (P) is accumulator
// register 8 * jj + e, i.e. key 16 * jj + 8 * (e >> 2) + 4 * hi + (e & 3)
__device__ __forceinline__ int pa_vt_pos(int j) { return (j & ~15) + 8 * ((j >> 2) & 1) + 4 * ((j >> 3) & 1) + (j & 3); }

template <int DT, bool ALIGNED>
__global__ __launch_bounds__(PA_THREADS) __attribute__((amdgpu_waves_per_eu(2))) void attn_dual_fwd_kernel(const pa_args p) {
  constexpr int KS = 2 * DT;                       // 16-wide contraction steps of the head dim
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int t = threadIdx.x, lane = t & 63, l31 = lane & 31, hi = lane >> 5;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int hd = p.hd, hdp = (hd + 15) & ~15, dt = (hd + 31) >> 5;
  const int kpitch = hdp + 8;                      // halfs: rows of 32 m + 16 bytes
  // workgroup -> (query band, head, batch), the pairing of region_attn.hip: with `remap` XCD i takes the (band, batch) pairs i, i + 8, .. and
  // runs their heads back to back (they read and write the same cache lines of Q and O)
  int b, h, band;
  {
    const int lin = blockIdx.x, H = p.H;
    int xb;
    if (p.remap) {
      const int xcd = lin & 7, k = lin >> 3;
      xb = (k / H) * 8 + xcd;
      h = k - (k / H) * H;
    } else {
      xb = lin / H;
      h = lin - xb * H;
    }
    band = xb % p.bands;
    b = xb / p.bands;
  }
  const int q = band * 128 + wave * 32 + l31;

  f32x16 o[DT];
#pragma unroll
  for (int d = 0; d < DT; ++d)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[d][r] = 0.f;

  for (int ph = 0; ph < p.nterms; ++ph) {
    const int Skv = ph ? p.t1.Skv : p.t0.Skv;
    const int64_t ldq = ph ? p.t1.ldq : p.t0.ldq, ldk = ph ? p.t1.ldk : p.t0.ldk, ldv = ph ? p.t1.ldv : p.t0.ldv;
    const f16* Qg = (ph ? p.t1.Q : p.t0.Q) + (int64_t)b * p.Sq * ldq + h * hd;
    const f16* Kg = (ph ? p.t1.K : p.t0.K) + (int64_t)b * Skv * ldk + h * hd;
    const f16* Vg = (ph ? p.t1.V : p.t0.V) + (int64_t)b * Skv * ldv + h * hd;
    const float c2 = (ph ? p.t1.scale : p.t0.scale) * PA_LOG2E;   // scores go to the log2 domain in fp32, after the MFMA
    const int nkt = (Skv + 31) >> 5;               // key tiles (1..4)
    const int vpitch = nkt * 32 + 8;
    f16* Kl = reinterpret_cast<f16*>(smem_raw);    // [nkt * 32][kpitch]
    f16* Vt = Kl + nkt * 32 * kpitch;              // [DT * 32][vpitch]

    // this term's Q fragments are requested before the staging: their latency hides under it
    f16x8 qf[KS];
#pragma unroll
    for (int j = 0; j < KS; ++j) {
      const int c = 16 * j + 8 * hi;
      const bool valid = q < p.Sq && c < hd;
      const f16x8 x = pa_load8<ALIGNED>(valid ? Qg + (int64_t)q * ldq + c : Kg);
      qf[j] = valid ? x : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }

    if (ph) __syncthreads();                       // every wave has finished reading the first term's images
    // ---- staging: K rows, V columns.  Loads are unconditional (an invalid unit re-reads the first K row and discards it)
    {
      const int kchunks = hdp >> 3, nk = nkt * 32 * kchunks;
      for (int u0 = t; u0 < nk; u0 += 4 * PA_THREADS) {
        f16x8 v[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int u = u0 + i * PA_THREADS, row = u / kchunks, c = (u - row * kchunks) * 8;
          const bool valid = u < nk && row < Skv && c < hd;
          const f16x8 x = pa_load8<ALIGNED>(valid ? Kg + (int64_t)row * ldk + c : Kg);
          v[i] = valid ? x : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int u = u0 + i * PA_THREADS, row = u / kchunks, c = (u - row * kchunks) * 8;
          if (u < nk) *(f16x8*)(Kl + row * kpitch + c) = v[i];
        }
      }
      // V: consecutive threads take consecutive KEYS of one 8-column chunk, so the eight 2-byte stores of a wave go to 16 different keys' slots
      constexpr int vchunks = DT * 4;
      const int nv = nkt * 32 * vchunks;
      for (int u0 = t; u0 < nv; u0 += 2 * PA_THREADS) {
        f16x8 v[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int u = u0 + i * PA_THREADS, ch = u / (nkt * 32), row = u - ch * (nkt * 32), c = ch * 8;
          const bool valid = u < nv && row < Skv && c < hd;
          const f16x8 x = pa_load8<ALIGNED>(valid ? Vg + (int64_t)row * ldv + c : Kg);
          v[i] = valid ? x : f16x8{0, 0, 0, 0, 0, 0, 0, 0};
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int u = u0 + i * PA_THREADS, ch = u / (nkt * 32), row = u - ch * (nkt * 32), c = ch * 8;
          if (u < nv) {
            f16* dst = Vt + c * vpitch + pa_vt_pos(row);
#pragma unroll
            for (int e = 0; e < 8; ++e) dst[e * vpitch] = v[i][e];
          }
        }
      }
    }
    __syncthreads();

    // S^T tiles: lane (l31, hi) ends with query q and keys kt * 32 + 8 * (r >> 2) + 4 * hi + (r & 3)
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
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
      if (kt < nkt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int key = kt * 32 + 8 * (r >> 2) + 4 * hi + (r & 3);
          const float v = key < Skv ? s[kt][r] * c2 : -INFINITY;   // the zero rows past Skv are no keys
          s[kt][r] = v;
          mx = fmaxf(mx, v);
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));          // (finite: Skv >= 1)
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
      if (kt < nkt)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float pv = __builtin_amdgcn_exp2f(s[kt][r] - mx);
          s[kt][r] = pv;
          l += pv;
        }
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.f / l;                       // l >= 1: the row maximum contributes exp2(0)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
      if (kt < nkt) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
          f16x8 pf;
#pragma unroll
          for (int e = 0; e < 8; ++e) pf[e] = (f16)(s[kt][8 * jj + e] * inv);   // normalised, then rounded
#pragma unroll
          for (int d = 0; d < DT; ++d)
            if (d < dt) {
              const f16x8 vf = *(const f16x8*)(Vt + (d * 32 + l31) * vpitch + kt * 32 + 16 * jj + 8 * hi);
              o[d] = TB_MFMA_32x32x16(vf, pf, o[d]);
            }
        }
      }
  }

  if (q < p.Sq) {
    f16* Og = p.O + ((int64_t)b * p.Sq + q) * p.ldo + h * hd;
#pragma unroll
    for (int d = 0; d < DT; ++d)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const int col = d * 32 + 8 * r4 + 4 * hi;   // 4 consecutive head-dim columns
        if (col < hd) {
          f16x4 v;
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = (f16)o[d][4 * r4 + e];
          if constexpr (ALIGNED) {
            *(f16x4*)(Og + col) = v;
          } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) Og[col + e] = v[e];
          }
        }
      }
  }
}

template <int DT>
int pa_launch(const pa_args& a, bool aligned, size_t lds, unsigned grid, hipStream_t s) {
  static bool attr_done = false;   // (per DT: one static per instantiation)
  if (!attr_done) {
    if (hipFuncSetAttribute((const void*)attn_dual_fwd_kernel<DT, true>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess ||
        hipFuncSetAttribute((const void*)attn_dual_fwd_kernel<DT, false>, hipFuncAttributeMaxDynamicSharedMemorySize, 96 * 1024) != hipSuccess)
      return TB_ELAUNCH;
    attr_done = true;
  }
  if (aligned)
    hipLaunchKernelGGL((attn_dual_fwd_kernel<DT, true>), dim3(grid), dim3(PA_THREADS), lds, s, a);
  else
    hipLaunchKernelGGL((attn_dual_fwd_kernel<DT, false>), dim3(grid), dim3(PA_THREADS), lds, s, a);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

bool pa_term_ok(const tb_attn_desc* d, int64_t C) {
  return d->Q && d->K && d->V && d->causal == 0 && d->Skv >= 1 && d->Skv <= PA_MAX_KV && d->ldq >= C && d->ldk >= C && d->ldv >= C;
}

pa_term pa_make_term(const tb_attn_desc* d) {
  return pa_term{(const f16*)d->Q, (const f16*)d->K, (const f16*)d->V, d->ldq, d->ldk, d->ldv, d->Skv, d->scale};
}

bool pa_term_aligned(const tb_attn_desc* d) {
  return (((uintptr_t)d->Q | (uintptr_t)d->K | (uintptr_t)d->V) & 15) == 0 && d->ldq % 8 == 0 && d->ldk % 8 == 0 && d->ldv % 8 == 0;
}

}  // namespace

extern "C" int tb_attention_dual_fwd(const tb_attn_desc* d1, const tb_attn_desc* d2, int dtype, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!d1 || !d1->O || dtype != TB_F16) return TB_EINVAL;
  if (d1->B < 1 || d1->H < 1 || d1->Sq < 1) return TB_EINVAL;
  if (d1->hd < 8 || d1->hd % 8 != 0 || d1->hd > 160) return TB_EINVAL;
  const int64_t C = (int64_t)d1->H * d1->hd;
  if (!pa_term_ok(d1, C) || d1->ldo < C) return TB_EINVAL;
  if (d2 && (d2->B != d1->B || d2->H != d1->H || d2->Sq != d1->Sq || d2->hd != d1->hd || !pa_term_ok(d2, C))) return TB_EINVAL;
  const int64_t BH = (int64_t)d1->B * d1->H;
  const int64_t bands = ((int64_t)d1->Sq + 127) / 128;
  if (bands * BH > 0x7fffffff) return TB_EINVAL;
  pa_args a;
  a.t0 = pa_make_term(d1);
  a.t1 = d2 ? pa_make_term(d2) : a.t0;
  a.O = (f16*)d1->O;
  a.ldo = d1->ldo;
  a.B = d1->B, a.H = d1->H, a.Sq = d1->Sq, a.hd = d1->hd;
  a.nterms = d2 ? 2 : 1;
  a.bands = (int)bands;
  a.remap = ((bands * d1->B) & 7) == 0;
  const int skv_max = d2 && d2->Skv > d1->Skv ? d2->Skv : d1->Skv;
  const int nkt = (skv_max + 31) / 32, hdp = (d1->hd + 15) & ~15;
  const int DT = d1->hd <= 64 ? 2 : (d1->hd <= 96 ? 3 : 5);
  const size_t lds = ((size_t)nkt * 32 * (hdp + 8) + (size_t)DT * 32 * (nkt * 32 + 8)) * sizeof(f16);   // <= 86528 bytes: two workgroups per CU
  const bool aligned = pa_term_aligned(d1) && (!d2 || pa_term_aligned(d2)) && ((uintptr_t)d1->O & 15) == 0 && d1->ldo % 8 == 0;
  const unsigned grid = (unsigned)(bands * BH);
  hipStream_t s = (hipStream_t)stream;
  if (DT == 2) return pa_launch<2>(a, aligned, lds, grid, s);
  if (DT == 3) return pa_launch<3>(a, aligned, lds, grid, s);
  return pa_launch<5>(a, aligned, lds, grid, s);
}
