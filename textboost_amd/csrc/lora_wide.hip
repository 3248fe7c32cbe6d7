// Text-encoder LoRA at ranks 9 .. 64 (--lora_rank 16 / 32 / 64): operand packing and the adapter weight gradients on the matrix cores.
// The rank <= 8 kernels of text_small.hip keep RR accumulators per element on the vector ALUs; at r = 64 that is a 0.5 GFLOP product per layer.
//
// Layout ("wide"): adapter p (q, k, v) owns columns [p*rp, p*rp + r) of t / dt, rp = r rounded up to 32, so that every 32-wide MFMA tile lies
// inside ONE adapter; the total width Rp is P*rp rounded up to the GEMMs' K granularity (64).  Padding columns / rows are zero.  The down
// projection, the dt product and both K-extended qkv products are plain tb_gemm calls on the packed operands; what no GEMM here does is the
// contraction over the ROW index M = B*77 of the two weight gradients:
//   dB[(p*D + n)*r + j] += scaling * sum_m dY[m, p*D + n] * t[m, p*rp + j]
//   dA[(p*r + j)*K + k] +=           sum_m dt[m, p*rp + j] * x[m, k]
#include "common.h"
#include "../../include/textboost_hip.h"

namespace {

// ---- one launch packs the operands of ALL layers (the stacks are contiguous over layers), TW = f16 or float (the fp32 mode):
//   Ap [l][c, k]  = A[l][(p*r + j)*K + k]               c = p*rp + j, j < r; else 0   ([Rp, K]: weight of the down projection)
//   W2 [l][n, c]  = scaling * B[l][n*r + j]             n in adapter p's rows, c = p*rp + j, j < r; else 0   ([P*D, Rp])
//   W2t[l][c, n]  = W2[l][n, c]                         ([Rp, P*D]: weight of the dt product; optional)
//   W2d[l][k, c]  = Ap[l][c, k]                         ([K, Rp]: second K-source of the qkv dgrad product)
template <typename TW>
__global__ __launch_bounds__(256) void lora_wide_pack_kernel(const float* __restrict__ A, const float* __restrict__ Bcat, TW* __restrict__ Ap,
                                                             TW* __restrict__ W2, TW* __restrict__ W2t, TW* __restrict__ W2d, int D, int K, int r,
                                                             int rp, int Rp, int P, int layers, float scaling) {
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nb = (int64_t)layers * P * D * Rp, na = (int64_t)layers * Rp * K;
  if (idx < nb) {
    const int64_t n = idx / Rp;  // row over layers * P * D
    const int c = (int)(idx - n * Rp);
    const int p = (int)((n / D) % P);
    const int j = c - p * rp;
    const float v = (j >= 0 && j < r) ? scaling * Bcat[n * r + j] : 0.f;
    W2[idx] = (TW)v;
    if (W2t) {
      const int64_t l = n / ((int64_t)P * D), nl = n - l * P * D;
      W2t[(l * Rp + c) * ((int64_t)P * D) + nl] = (TW)v;
    }
  } else if (idx < nb + na) {
    const int64_t i = idx - nb;
    const int64_t lc = i / K;  // layer * Rp + c
    const int k = (int)(i - lc * K);
    const int64_t l = lc / Rp;
    const int c = (int)(lc - l * Rp);
    const int p = c / rp, j = c - p * rp;
    const float v = (p < P && j < r) ? A[((l * P + p) * r + j) * K + k] : 0.f;
    Ap[i] = (TW)v;
    W2d[(l * K + k) * Rp + c] = (TW)v;
  }
}

// ---- the two weight gradients in one launch: one 32 x 32 output tile per workgroup, C[i, j] = sum_m Lm[m, c0 + i] * Sm[m, s0 + j].
//   blocks [0, nB)        dB tiles: Lm = dY (32 of adapter p's output columns), Sm = t  (32 of adapter p's rank columns)
//   blocks [nB, nB + nA)  dA tiles: Lm = dt (32 rank columns of one adapter),  Sm = x  (32 input columns)
// The workgroup walks ALL of M in 64-row slabs: both [64 rows][32 columns] slabs are staged row-major in LDS (64-byte rows: the four rows a
// transposing read touches per 16-lane group cover all 64 banks once), wave w multiplies rows 16 w .. 16 w + 15 of every slab -- m is the MFMA's k
// index, so both fragments come through ds_read_b64_tr_b16 -- and the four waves' accumulators are added in wave order through LDS: fp32
// accumulation in a fixed order, no atomics.  Rows >= M are zero-filled in LDS.  Every lane runs every transposing read (EXEC all ones: no
// early return, no lane-dependent branch around them); all LDS is one static array, so every address below is 8-byte aligned.
constexpr int LW_TILE = 32, LW_SLAB = 64, LW_ROWB = 64 /* bytes per image row */, LW_IMG = LW_SLAB * LW_ROWB;

__device__ __forceinline__ f16x4 lw_tr_read(uint32_t addr) {
  f16x4 v;
  asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr) : "memory");
  return v;
}

__global__ __launch_bounds__(256) void lora_wide_wgrad_kernel(const f16* __restrict__ dY, int64_t lddy, const f16* __restrict__ x, int64_t ldx,
                                                              const f16* __restrict__ t, int64_t ldt, const f16* __restrict__ dt, int64_t lddt,
                                                              float* __restrict__ dA, float* __restrict__ dB, int64_t M, int D, int K, int r,
                                                              int rp, int P, float scaling, int nB) {
  __shared__ __attribute__((aligned(16))) unsigned char lw_smem[4 * 16 * 64 * 4];   // the walk: two slab images (8 KiB); then 4 waves x 16 x 64 floats
  static_assert(sizeof(lw_smem) >= 2 * LW_IMG, "slab images fit");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int jt_n = rp / LW_TILE;   // rank tiles per adapter
  // ---- tile (block-uniform)
  const bool is_b = (int)blockIdx.x < nB;
  const f16 *Lm, *Sm;
  int64_t ldl, lds_, c0, s0;
  int p, j0;          // adapter, first rank column of the tile inside it
  int64_t o0;         // dB: first output column n0 (over P*D); dA: first input column k0
  if (is_b) {
    const int b = (int)blockIdx.x;
    const int nt = b / jt_n, jt = b - nt * jt_n;
    o0 = (int64_t)nt * LW_TILE;
    p = (int)(o0 / D), j0 = jt * LW_TILE;
    Lm = dY, ldl = lddy, c0 = o0;
    Sm = t, lds_ = ldt, s0 = (int64_t)p * rp + j0;
  } else {
    const int b = (int)blockIdx.x - nB;
    const int kt_n = K / LW_TILE;
    const int ct = b / kt_n, kt = b - ct * kt_n;   // ct: 32-column tile of dt over P * rp
    o0 = (int64_t)kt * LW_TILE;
    p = ct / jt_n, j0 = (ct - p * jt_n) * LW_TILE;
    Lm = dt, ldl = lddt, c0 = (int64_t)ct * LW_TILE;
    Sm = x, lds_ = ldx, s0 = o0;
  }
  // ---- staging: thread -> row tid / 4, 16-byte chunk tid % 4 of both slabs
  const int srow = tid >> 2, sch = tid & 3;
  const f16* lp = Lm + c0 + sch * 8;
  const f16* sp = Sm + s0 + sch * 8;
  const f16x8 z8 = {0, 0, 0, 0, 0, 0, 0, 0};
  f16x8 lv, sv;
  auto load_slab = [&](int64_t m0) {
    const int64_t m = m0 + srow;
    const bool ok = m < M;
    lv = ok ? *(const f16x8*)(lp + m * ldl) : z8;
    sv = ok ? *(const f16x8*)(sp + m * lds_) : z8;
  };
  // ---- transposing reads: the 16-lane group g = lane / 16 fetches the block [rows 16 wave + 8 (lane / 32) + 4 u + (0..3)][columns 16 (g & 1) + (0..15)];
  // lane 4 q + pp of the group supplies row q, columns 4 pp .. 4 pp + 3 and receives column (lane % 16), rows 0..3 -> elements 4 u .. 4 u + 3 of the
  // 32x32x16 fragment of tile column lane % 32, k = 8 (lane / 32) + 4 u + e
  typedef __attribute__((address_space(3))) void* lptr_t;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(lptr_t)lw_smem;
  const int li = lane & 15, q = li >> 2, pp = li & 3;
  const uint32_t ta = lds0 + (uint32_t)((wave * 16 + 8 * (lane >> 5) + q) * LW_ROWB + (16 * ((lane >> 4) & 1) + 4 * pp) * 2);
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  load_slab(0);
  for (int64_t m0 = 0; m0 < M; m0 += LW_SLAB) {
    __syncthreads();  // the previous slab's fragment reads are done
    *(f16x8*)(lw_smem + srow * LW_ROWB + sch * 16) = lv;
    *(f16x8*)(lw_smem + LW_IMG + srow * LW_ROWB + sch * 16) = sv;
    __syncthreads();
    if (m0 + LW_SLAB < M) load_slab(m0 + LW_SLAB);   // (block-uniform) the next slab's loads fly under this slab's product
    f16x4 a0 = lw_tr_read(ta), a1 = lw_tr_read(ta + 4 * LW_ROWB);
    f16x4 b0 = lw_tr_read(ta + LW_IMG), b1 = lw_tr_read(ta + LW_IMG + 4 * LW_ROWB);
    // inline-asm reads are not counted by the compiler; the wait takes the four fragments as operands so that no use of them can move above it
    asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(a0), "+v"(a1), "+v"(b0), "+v"(b1)::"memory");
    f16x8 af, bf;
#pragma unroll
    for (int e = 0; e < 4; ++e) af[e] = a0[e], af[4 + e] = a1[e], bf[e] = b0[e], bf[4 + e] = b1[e];
    acc = TB_MFMA_32x32x16(af, bf, acc);
  }
  // ---- the four waves' partial tiles, added in wave order
  __syncthreads();
  float* red = (float*)lw_smem;   // [wave][register][lane]
#pragma unroll
  for (int e = 0; e < 16; ++e) red[(wave * 16 + e) * 64 + lane] = acc[e];
  __syncthreads();
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int e = tid + 256 * u;          // register e / 64 of lane e % 64
    const float v = ((red[e] + red[1024 + e]) + red[2048 + e]) + red[3072 + e];
    const int ln = e & 63, reg = e >> 6;
    const int col = ln & 31, row = mfma32_row(reg, ln >> 5);
    if (is_b) {  // C[i = output column, j = rank column]: rows of r floats (4-byte stores: r may be odd)
      if (j0 + col < r) dB[(o0 + row) * r + j0 + col] += v * scaling;
    } else {     // C[i = rank column, j = input column]
      if (j0 + row < r) dA[((int64_t)p * r + j0 + row) * K + o0 + col] += v;
    }
  }
}

}  // namespace

#define GRID1D(n) dim3((unsigned)(((n) + 255) / 256))

static bool lw_dims_ok(int r, int rp, int P) { return r > 0 && rp >= r && rp % LW_TILE == 0 && rp <= 64 && P > 0; }

extern "C" int tb_lora_wide_pack(const float* A, const float* Bcat, void* a_pad, void* w2_fwd, void* w2_t, void* w2_dgrad, int dtype, int D,
                                 int K, int r, int rp, int Rp, int P, int layers, float scaling, tb_stream_t stream) {
  (void)hipGetLastError();  // drop any stale (non-sticky) error left by an earlier runtime call
  if (!A || !Bcat || !a_pad || !w2_fwd || !w2_dgrad || !lw_dims_ok(r, rp, P) || Rp < P * rp || layers <= 0 || D <= 0 || K <= 0) return TB_EINVAL;
  const int64_t n = (int64_t)layers * ((int64_t)P * D + K) * Rp;
  if (dtype == TB_F16)
    hipLaunchKernelGGL(lora_wide_pack_kernel<f16>, GRID1D(n), dim3(256), 0, (hipStream_t)stream, A, Bcat, (f16*)a_pad, (f16*)w2_fwd, (f16*)w2_t,
                       (f16*)w2_dgrad, D, K, r, rp, Rp, P, layers, scaling);
  else if (dtype == TB_F32)
    hipLaunchKernelGGL(lora_wide_pack_kernel<float>, GRID1D(n), dim3(256), 0, (hipStream_t)stream, A, Bcat, (float*)a_pad, (float*)w2_fwd,
                       (float*)w2_t, (float*)w2_dgrad, D, K, r, rp, Rp, P, layers, scaling);
  else
    return TB_EINVAL;
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int tb_lora_wide_wgrad(const void* dY, int64_t lddy, const void* x, int64_t ldx, const void* t, int64_t ldt, const void* dt,
                                  int64_t lddt, float* dA, float* dB, int64_t M, int D, int K, int r, int rp, int P, float scaling,
                                  tb_stream_t stream) {
  (void)hipGetLastError();  // drop any stale (non-sticky) error left by an earlier runtime call
  if (!dY || !x || !t || !dt || !dA || !dB || !lw_dims_ok(r, rp, P) || M <= 0 || D <= 0 || K <= 0) return TB_EINVAL;
  if (D % LW_TILE || K % LW_TILE) return TB_EINVAL;                       // tiles inside one adapter / inside the row
  if (lddy % 8 || ldx % 8 || ldt % 8 || lddt % 8) return TB_EINVAL;       // 16-byte vector loads
  if (((uintptr_t)dY) % 16 || ((uintptr_t)x) % 16 || ((uintptr_t)t) % 16 || ((uintptr_t)dt) % 16) return TB_EINVAL;
  if (lddy < (int64_t)P * D || ldx < K || ldt < (int64_t)P * rp || lddt < (int64_t)P * rp) return TB_EINVAL;
  const int nB = (P * D / LW_TILE) * (rp / LW_TILE), nA = (P * rp / LW_TILE) * (K / LW_TILE);
  hipLaunchKernelGGL(lora_wide_wgrad_kernel, dim3(nB + nA), dim3(256), 0, (hipStream_t)stream, (const f16*)dY, lddy, (const f16*)x, ldx,
                     (const f16*)t, ldt, (const f16*)dt, lddt, dA, dB, M, D, K, r, rp, P, scaling, nB);
  TB_CHECK_LAUNCH();
  return TB_OK;
}
