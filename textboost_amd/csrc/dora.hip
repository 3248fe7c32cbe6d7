// Text-encoder DoRA (--use_dora): weight-decomposed LoRA, a learned per-output-row magnitude m on top of the low-rank direction
// (peft 0.13.2 DoraLinearLayer).  For one adapted Linear, W [N, K], A [r, K], B [N, r], s = lora_alpha / r:
//   n_j = || W_j + s (B A)_j ||_2        a CONSTANT of the backward (peft detaches it)          c_j = m_j / n_j
//   u   = x W^T + s (x A^T) B^T          what the two-source GEMM computes, stored in the operand type
//   y   = c (.) u + b                    then the Linear's own epilogue (residual / activation + saved pre-activation)
//   dU  = dY (.) c                       feeds every existing adapter / dgrad kernel in dY's place
//   dm_j += (1 / n_j) sum_i dY_ij u_ij
// Three kernels: the row norms of all layers of one module (once per optimizer step), the forward application behind the GEMM that wrote u
// (student rows only: the frozen rows behind them take c = 1), and the backward's scale + column reduction.  Every sum is fp32 in a fixed
// order -- per thread sequentially, across lanes by xor shuffles, across waves / row lanes through LDS in index order -- and nothing here
// uses an atomic: two launches give the same bits.
#include "common.h"
#include "../../include/textboost_hip.h"

namespace {

// ---- 8 consecutive elements as floats, 16-byte accesses (callers check: columns % 8 == 0, pitches % 8 == 0, 16-byte aligned bases)
__device__ __forceinline__ void load8(const f16* p, float* v) {
  const f16x8 x = *(const f16x8*)p;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (float)x[e];
}
__device__ __forceinline__ void load8(const float* p, float* v) {
  const f32x4 a = *(const f32x4*)p, b = *(const f32x4*)(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[e] = a[e];
    v[4 + e] = b[e];
  }
}
__device__ __forceinline__ void store8(f16* p, const float* v) {
  f16x8 x;
#pragma unroll
  for (int e = 0; e < 8; ++e) x[e] = (f16)v[e];
  *(f16x8*)p = x;
}
__device__ __forceinline__ void store8(float* p, const float* v) {
  f32x4 a, b;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    a[e] = v[e];
    b[e] = v[4 + e];
  }
  *(f32x4*)p = a;
  *(f32x4*)(p + 4) = b;
}
__device__ __forceinline__ void load2(const f16* p, float& a, float& b) {
  const f16x2 x = *(const f16x2*)p;
  a = (float)x[0];
  b = (float)x[1];
}
__device__ __forceinline__ void load2(const float* p, float& a, float& b) {
  const float2 x = *(const float2*)p;
  a = x.x;
  b = x.y;
}

// ---- kernel 1: n [layers][N] = row norms of W + s B A, c = m / n.  N = P * D; adapter p owns rows [p D, (p + 1) D) and A rows [p r, (p + 1) r).
// One workgroup per (16 rows, layer): thread t owns the column pairs 2 t + 512 i, forms the 16 x 2 products (B A) from the tile's B rows in LDS
// (broadcast reads) and A from global (shared by all row tiles: L2), adds the stored W and squares.  W is read once, 4 bytes per lane.
constexpr int DN_ROWS = 16;
template <typename TW>
__global__ __launch_bounds__(256) void dora_norms_kernel(const void* const* __restrict__ Wp, const float* __restrict__ A,
                                                         const float* __restrict__ Bcat, const float* __restrict__ m, float* __restrict__ n_out,
                                                         float* __restrict__ c_out, int D, int K, int r, int P, float scaling) {
  __shared__ __attribute__((aligned(16))) float Bs[DN_ROWS][64];
  __shared__ float red[4][DN_ROWS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int layer = blockIdx.y;
  const int64_t N = (int64_t)P * D;
  const int64_t j0 = (int64_t)blockIdx.x * DN_ROWS;   // first row of the tile (D % 16 == 0: one adapter per tile)
  const int p = (int)(j0 / D);
  const TW* W = (const TW*)Wp[layer] + j0 * K;
  const float* Al = A + ((int64_t)layer * P + p) * r * K;
  const float* Bl = Bcat + ((int64_t)layer * N + j0) * r;
  const int r4 = (r + 3) & ~3;
  for (int i = tid; i < DN_ROWS * 64; i += 256) {
    const int jj = i >> 6, q = i & 63;
    Bs[jj][q] = q < r ? scaling * Bl[jj * r + q] : 0.f;
  }
  __syncthreads();
  float ss[DN_ROWS];
#pragma unroll
  for (int jj = 0; jj < DN_ROWS; ++jj) ss[jj] = 0.f;
  for (int k = 2 * tid; k < K; k += 512) {
    float d0[DN_ROWS], d1[DN_ROWS];
#pragma unroll
    for (int jj = 0; jj < DN_ROWS; ++jj) d0[jj] = d1[jj] = 0.f;
    for (int rc = 0; rc < r4; rc += 4) {
      float a0[4], a1[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        a0[q] = a1[q] = 0.f;
        if (rc + q < r) load2(Al + (int64_t)(rc + q) * K + k, a0[q], a1[q]);
      }
#pragma unroll
      for (int jj = 0; jj < DN_ROWS; ++jj) {
        const f32x4 b = *(const f32x4*)&Bs[jj][rc];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          d0[jj] = fmaf(b[q], a0[q], d0[jj]);
          d1[jj] = fmaf(b[q], a1[q], d1[jj]);
        }
      }
    }
#pragma unroll
    for (int jj = 0; jj < DN_ROWS; ++jj) {
      float w0, w1;
      load2(W + (int64_t)jj * K + k, w0, w1);
      w0 += d0[jj];
      w1 += d1[jj];
      ss[jj] = fmaf(w0, w0, ss[jj]);
      ss[jj] = fmaf(w1, w1, ss[jj]);
    }
  }
#pragma unroll
  for (int jj = 0; jj < DN_ROWS; ++jj) {
    const float v = wave_sum(ss[jj]);
    if (lane == 0) red[wave][jj] = v;
  }
  __syncthreads();
  if (tid < DN_ROWS) {
    const float nn = sqrtf(((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid]);
    const int64_t o = (int64_t)layer * N + j0 + tid;
    n_out[o] = nn;
    if (c_out) c_out[o] = m[o] / nn;
  }
}

// ---- kernel 2: y[i, :] = epilogue(c (.) u[i, :] + b) for rows i < Ms, epilogue(u[i, :] + b) for the frozen rows behind them.
// ACT 0: plain (+ the fp32 residual R when given); ACT 1 / 2: quick_gelu / erf gelu of the value rounded to the operand type, which is also
// stored as the pre-activation -- the arithmetic of tb_gemm's epilogue.  One (row, 8 columns) unit per thread, grid-stride.
template <typename TU, typename TY, int ACT>
__global__ __launch_bounds__(256) void dora_apply_kernel(const TU* __restrict__ u, int64_t ldu, const float* __restrict__ c,
                                                         const float* __restrict__ bias, int64_t M, int64_t Ms, int N,
                                                         const float* __restrict__ R, int64_t ldr, TY* __restrict__ y, int64_t ldy,
                                                         TU* __restrict__ pre, int64_t ldpre) {
  const int n8 = N >> 3;
  const int64_t units = M * n8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < units; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / n8;
    const int col = (int)(i - row * n8) << 3;
    float v[8], cs[8], b[8];
    load8(u + row * ldu + col, v);
    load8(bias + col, b);
    if (row < Ms) {
      load8(c + col, cs);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = fmaf(cs[e], v[e], b[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += b[e];
    }
    if (R) {
      float rr[8];
      load8(R + row * ldr + col, rr);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] += rr[e];
    }
    if (ACT != 0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = (float)(TU)v[e];
      if (pre) store8(pre + row * ldpre + col, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) v[e] = ACT == 1 ? quick_gelu_f(v[e]) : gelu_erf_f(v[e]);
    }
    store8(y + row * ldy + col, v);
  }
}

// ---- kernel 3: dU = dY (.) c and dm[j] += (1 / n[j]) sum_i dY[i, j] u[i, j].  One workgroup of 1024 threads per 64 columns walks ALL M rows: thread
// (cg = tid & 7, rl = tid >> 3) owns columns 8 cg .. 8 cg + 7 of rows rl, rl + 128, ... (sequential fp32 sums); the 128 row lanes are added through
// LDS in index order, 32 at a time and then the four partial sums.  A wave instruction touches 8 rows x 128 (256) contiguous bytes.  The launch is
// latency-bound (12 .. 48 workgroups): sixteen waves per workgroup keep each thread's walk at M / 128 iterations.
constexpr int DB_LANES = 128;
template <typename T>
__global__ __launch_bounds__(1024) void dora_bwd_kernel(const T* __restrict__ dY, int64_t lddy, const T* __restrict__ u, int64_t ldu,
                                                        const float* __restrict__ c, const float* __restrict__ nrm, T* __restrict__ dU,
                                                        int64_t lddu, float* __restrict__ dm, int64_t M, int N) {
  __shared__ float red[DB_LANES][65];
  __shared__ float red2[4][64];
  const int tid = threadIdx.x, cg = tid & 7, rl = tid >> 3;
  const int col = blockIdx.x * 64 + cg * 8;
  float acc[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) acc[e] = 0.f;
  if (col < N) {   // (N % 8 == 0: a unit is inside the matrix or wholly outside)
    float cs[8];
    load8(c + col, cs);
    for (int64_t row = rl; row < M; row += DB_LANES) {
      float g[8], uu[8];
      load8(dY + row * lddy + col, g);
      load8(u + row * ldu + col, uu);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        acc[e] = fmaf(g[e], uu[e], acc[e]);
        g[e] *= cs[e];
      }
      store8(dU + row * lddu + col, g);
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[rl][cg * 8 + e] = acc[e];
  __syncthreads();
  if (tid < 256) {
    const int q = tid >> 6, j = tid & 63;
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < 32; ++i) s += red[q * 32 + i][j];
    red2[q][j] = s;
  }
  __syncthreads();
  if (tid < 64) {
    const int j = blockIdx.x * 64 + tid;
    if (j < N) dm[j] += (((red2[0][tid] + red2[1][tid]) + red2[2][tid]) + red2[3][tid]) / nrm[j];
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int tb_dora_norms(const void* const* Wp, int dtype, const float* A, const float* Bcat, const float* m, float* n_out, float* c_out,
                             int D, int K, int r, int P, int layers, float scaling, tb_stream_t stream) {
  if (!Wp || !A || !Bcat || !n_out || (c_out && !m)) return TB_EINVAL;
  if (D <= 0 || D % DN_ROWS || K <= 0 || K % 2 || r < 1 || r > 64 || P < 1 || layers < 1) return TB_EINVAL;
  if (dtype != TB_F16 && dtype != TB_F32) return TB_EINVAL;
  const dim3 grid((unsigned)((int64_t)P * D / DN_ROWS), (unsigned)layers);
  if (dtype == TB_F32)
    hipLaunchKernelGGL(dora_norms_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, Wp, A, Bcat, m, n_out, c_out, D, K, r, P, scaling);
  else
    hipLaunchKernelGGL(dora_norms_kernel<f16>, grid, dim3(256), 0, (hipStream_t)stream, Wp, A, Bcat, m, n_out, c_out, D, K, r, P, scaling);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

namespace {
template <typename TU, typename TY>
int dora_apply_launch(const void* u, int64_t ldu, const float* c, const float* bias, int64_t M, int64_t Ms, int N, int act, const float* R,
                      int64_t ldr, void* y, int64_t ldy, void* pre, int64_t ldpre, hipStream_t st) {
  const int64_t units = M * (N >> 3);
  const unsigned grid = (unsigned)((units + 255) / 256 < 2048 ? (units + 255) / 256 : 2048);
#define TB_DORA_APPLY(ACT)                                                                                                              \
  hipLaunchKernelGGL((dora_apply_kernel<TU, TY, ACT>), dim3(grid), dim3(256), 0, st, (const TU*)u, ldu, c, bias, M, Ms, N, R, ldr, (TY*)y, \
                     ldy, (TU*)pre, ldpre)
  if (act == TB_ACT_NONE) TB_DORA_APPLY(0);
  else if (act == TB_ACT_QUICK_GELU) TB_DORA_APPLY(1);
  else TB_DORA_APPLY(2);
#undef TB_DORA_APPLY
  TB_CHECK_LAUNCH();
  return TB_OK;
}
}  // namespace

extern "C" int tb_dora_apply(const void* u, int64_t ldu, int dtype, const float* c, const float* bias, int64_t M, int64_t Ms, int N, int act,
                             const float* R, int64_t ldr, void* y, int64_t ldy, int y_dtype, void* pre, int64_t ldpre, tb_stream_t stream) {
  if (!u || !c || !bias || !y || M <= 0 || Ms < 0 || Ms > M || N <= 0 || N % 8) return TB_EINVAL;
  if (dtype != TB_F16 && dtype != TB_F32) return TB_EINVAL;
  if (y_dtype != TB_F32 && y_dtype != dtype) return TB_EINVAL;
  if (act != TB_ACT_NONE && act != TB_ACT_QUICK_GELU && act != TB_ACT_GELU) return TB_EINVAL;
  if (act != TB_ACT_NONE && (R || y_dtype != dtype)) return TB_EINVAL;   // the activation's output is an operand of the next Linear
  if (act == TB_ACT_NONE && pre) return TB_EINVAL;
  const int ua = dtype == TB_F32 ? 4 : 8, ya = y_dtype == TB_F32 ? 4 : 8;   // pitch granularity of a 16-byte access
  if (ldu % ua || ldy % ya || !al16(u) || !al16(y) || !al16(c) || !al16(bias)) return TB_EINVAL;
  if (R && (ldr % 4 || !al16(R))) return TB_EINVAL;
  if (pre && (ldpre % ua || !al16(pre))) return TB_EINVAL;
  hipStream_t st = (hipStream_t)stream;
  if (dtype == TB_F32) return dora_apply_launch<float, float>(u, ldu, c, bias, M, Ms, N, act, R, ldr, y, ldy, pre, ldpre, st);
  if (y_dtype == TB_F32) return dora_apply_launch<f16, float>(u, ldu, c, bias, M, Ms, N, act, R, ldr, y, ldy, pre, ldpre, st);
  return dora_apply_launch<f16, f16>(u, ldu, c, bias, M, Ms, N, act, R, ldr, y, ldy, pre, ldpre, st);
}

extern "C" int tb_dora_bwd(const void* dY, int64_t lddy, const void* u, int64_t ldu, int dtype, const float* c, const float* n, void* dU,
                           int64_t lddu, float* dm, int64_t M, int N, tb_stream_t stream) {
  if (!dY || !u || !c || !n || !dU || !dm || M <= 0 || N <= 0 || N % 8) return TB_EINVAL;
  if (dtype != TB_F16 && dtype != TB_F32) return TB_EINVAL;
  const int a = dtype == TB_F32 ? 4 : 8;
  if (lddy % a || ldu % a || lddu % a || !al16(dY) || !al16(u) || !al16(dU) || !al16(c)) return TB_EINVAL;
  const dim3 grid((unsigned)((N + 63) / 64));
  if (dtype == TB_F32)
    hipLaunchKernelGGL(dora_bwd_kernel<float>, grid, dim3(1024), 0, (hipStream_t)stream, (const float*)dY, lddy, (const float*)u, ldu, c, n,
                       (float*)dU, lddu, dm, M, N);
  else
    hipLaunchKernelGGL(dora_bwd_kernel<f16>, grid, dim3(1024), 0, (hipStream_t)stream, (const f16*)dY, lddy, (const f16*)u, ldu, c, n,
                       (f16*)dU, lddu, dm, M, N);
  TB_CHECK_LAUNCH();
  return TB_OK;
}
