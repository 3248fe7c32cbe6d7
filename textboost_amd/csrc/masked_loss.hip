// Masked denoising loss (--instance_mask_dir): the subject mask of a training image weights the MSE of the step, so that the background of the
// single instance image stays out of the gradient.  The reference has the slot (train_textboost.py:1086-1088, dataset.py:367-370) and nothing
// that fills it; DESIGN.md section 16 states the two deviations from its dead line (division by C * W_b, and max(W_b, 1)).
//
//   * tb_img_to_loss_weight  crop of a resident grey RGBX mask image (image.hip's layout: one dword per pixel, R in the low byte) ->
//                            cell x cell box mean of the R byte -> fp32 [out_h, out_w] latent-sized weights, bit-exact with numpy float32
//   * tb_mse_loss_weighted(_f32)  loss = (1/B) sum_b [ sum_{c,y,x} w_b (pred - target)^2 / (C max(W_b, 1)) ],  W_b = sum_{y,x} w_b, and
//                            dpred = loss_scale * dloss/dpred; two launches, a deterministic two-stage reduction with no atomics
#include "../../include/textboost_hip.h"
#include "common.h"

// tb_img_to_loss_weight's arithmetic is pinned operation by operation (numpy float32 rounds each one): no FMA contraction in this file
#pragma clang fp contract(off)

namespace {

// A block is 64 x 4 threads: thread (tx, ty) sums the `cell` pixels of crop column bx * cpb * cell + tx under output row by * 4 + ty (a wave reads
// one contiguous 256-byte row segment per load, as everywhere in image.hip), the column sums meet in LDS, and thread tx < cpb adds the `cell`
// columns of its output cell.  cpb = 64 / cell cells per block row, so that no cell straddles two blocks.  All sums are exact integers.
__global__ __launch_bounds__(256) void loss_weight_kernel(const uint32_t* __restrict__ src, int64_t sstride, int x0, int y0, int out_h, int out_w,
                                                          int cell, float floor_w, float* __restrict__ dst) {
  __shared__ int col[4][64];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int cpb = 64 / cell;
  const int oy = blockIdx.y * 4 + ty;
  const int cx = blockIdx.x * cpb * cell + tx;  // crop column
  int s = 0;
  if (tx < cpb * cell && cx < out_w * cell && oy < out_h) {
    const uint32_t* p = src + (int64_t)(y0 + oy * cell) * sstride + x0 + cx;
    for (int j = 0; j < cell; ++j) s += (int)(p[(int64_t)j * sstride] & 255u);
  }
  col[ty][tx] = s;
  __syncthreads();
  const int ox = blockIdx.x * cpb + tx;
  if (tx < cpb && ox < out_w && oy < out_h) {
    int S = 0;
    for (int j = 0; j < cell; ++j) S += col[ty][tx * cell + j];
    const float m = (float)S / (float)(255 * cell * cell);
    const float scale = 1.f - floor_w;
    const float sm = scale * m;  // rounds on its own (contraction is off)
    dst[(int64_t)oy * out_w + ox] = floor_w + sm;
  }
}

// First stage.  Grid (P, B): block (p, b) owns elements [p, p + P, ...) * 256 of sample b's C * hw.  Every block of a sample first adds up the
// sample's hw weights itself (hw is 4096 at 512^2: 16 L2-resident loads per thread, cheaper than a third launch), in double, so that W_b is
// the correctly rounded sum and the gradient carries four fp32 roundings only: pred - target, w * d, the coefficient, and their product.
template <typename TP>
__global__ __launch_bounds__(256) void wmse_partial_kernel(const TP* __restrict__ pred, const float* __restrict__ target,
                                                           const float* __restrict__ weight, float* __restrict__ dpred,
                                                           const float* __restrict__ loss_scale, int B, int C, int hw, float* __restrict__ part,
                                                           float* __restrict__ inv_den) {
  __shared__ double redd[4];
  __shared__ float red[4];
  const int b = blockIdx.y, P = gridDim.x;
  const float* wb = weight + (int64_t)b * hw;
  double ws = 0.0;
  for (int i = threadIdx.x; i < hw; i += 256) ws += (double)wb[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ws += __shfl_xor(ws, o, 64);
  if ((threadIdx.x & 63) == 0) redd[threadIdx.x >> 6] = ws;
  __syncthreads();
  const double W = ((redd[0] + redd[1]) + (redd[2] + redd[3]));
  const double den = (double)C * (W > 1.0 ? W : 1.0);  // max(W_b, 1): one latent pixel's worth of weight
  const float gcoef = (float)(2.0 * (double)(loss_scale ? loss_scale[0] : 1.f) / ((double)B * den));
  const int64_t n = (int64_t)C * hw, base = (int64_t)b * n;
  float a = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)P * 256) {
    const float d = (float)pred[base + i] - target[base + i];
    const float wd = wb[i % hw] * d;
    a += wd * d;
    dpred[base + i] = gcoef * wd;
  }
  a = block_sum_256(a, red);
  if (threadIdx.x == 0) {
    part[(int64_t)b * P + blockIdx.x] = a;
    if (blockIdx.x == 0) inv_den[b] = (float)(1.0 / den);
  }
}

// Second stage, one wave: lane l adds the partials of samples l, l + 64, ... in a fixed order.
__global__ __launch_bounds__(64) void wmse_final_kernel(const float* __restrict__ part, const float* __restrict__ inv_den, int B, int P,
                                                        float* __restrict__ loss_out) {
  double acc = 0.0;
  for (int b = threadIdx.x; b < B; b += 64) {
    double s = 0.0;
    for (int p = 0; p < P; ++p) s += (double)part[(int64_t)b * P + p];
    acc += s * (double)inv_den[b];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if (threadIdx.x == 0) loss_out[0] = (float)(acc / (double)B);
}

int wmse_blocks(int C, int h, int w) {
  const int64_t n = (int64_t)C * h * w;
  int64_t P = (n + 1023) / 1024;
  return (int)(P > 16 ? 16 : P < 1 ? 1 : P);
}

template <typename TP>
int wmse_launch(const TP* pred, const float* target, const float* weight, float* dpred, float* loss_out, const float* loss_scale, int B, int C,
                int h, int w, float* ws, int64_t ws_bytes, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!pred || !target || !weight || !dpred || !loss_out || !ws || B <= 0 || B > 65535 || C <= 0 || h <= 0 || w <= 0) return TB_EINVAL;
  if ((int64_t)h * w > (1 << 30) || (int64_t)C * h * w > ((int64_t)1 << 40)) return TB_EINVAL;
  if (ws_bytes < tb_mse_loss_weighted_workspace_bytes(B, C, h, w)) return TB_EINVAL;
  const int P = wmse_blocks(C, h, w);
  float* part = ws;
  float* inv_den = ws + (int64_t)B * P;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(wmse_partial_kernel<TP>, dim3(P, B), dim3(256), 0, s, pred, target, weight, dpred, loss_scale, B, C, h * w, part, inv_den);
  hipLaunchKernelGGL(wmse_final_kernel, dim3(1), dim3(64), 0, s, part, inv_den, B, P, loss_out);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

}  // namespace

extern "C" int tb_img_to_loss_weight(const uint32_t* src, int64_t sstride, int sw, int sh, int x0, int y0, int out_h, int out_w, int cell,
                                     float floor_w, float* dst, tb_stream_t stream) {
  (void)hipGetLastError();
  if (!src || !dst || sw <= 0 || sh <= 0 || out_h <= 0 || out_w <= 0 || cell <= 0 || cell > 64 || sstride < sw) return TB_EINVAL;
  if (!(floor_w >= 0.f && floor_w < 1.f)) return TB_EINVAL;
  if (x0 < 0 || y0 < 0 || (int64_t)x0 + (int64_t)cell * out_w > sw || (int64_t)y0 + (int64_t)cell * out_h > sh) return TB_EINVAL;
  const int cpb = 64 / cell;
  hipLaunchKernelGGL(loss_weight_kernel, dim3((out_w + cpb - 1) / cpb, (out_h + 3) / 4), dim3(64, 4), 0, (hipStream_t)stream, src, sstride, x0,
                     y0, out_h, out_w, cell, floor_w, dst);
  TB_CHECK_LAUNCH();
  return TB_OK;
}

extern "C" int64_t tb_mse_loss_weighted_workspace_bytes(int B, int C, int h, int w) {
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0) return TB_EINVAL;
  return (int64_t)B * (wmse_blocks(C, h, w) + 1) * (int64_t)sizeof(float);
}

extern "C" int tb_mse_loss_weighted(const void* pred, const float* target, const float* weight, float* dpred, float* loss_out,
                                    const float* loss_scale, int B, int C, int h, int w, float* ws, int64_t ws_bytes, tb_stream_t stream) {
  return wmse_launch((const f16*)pred, target, weight, dpred, loss_out, loss_scale, B, C, h, w, ws, ws_bytes, stream);
}

extern "C" int tb_mse_loss_weighted_f32(const float* pred, const float* target, const float* weight, float* dpred, float* loss_out,
                                        const float* loss_scale, int B, int C, int h, int w, float* ws, int64_t ws_bytes, tb_stream_t stream) {
  return wmse_launch(pred, target, weight, dpred, loss_out, loss_scale, B, C, h, w, ws, ws_bytes, stream);
}
