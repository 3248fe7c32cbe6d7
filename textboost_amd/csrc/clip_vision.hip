// CLIP ViT patch embedding (textboost_amd/clip_score.py: the image tower of the CLIP-T / CLIP-I evaluation).
//
// `vision_model.embeddings` of transformers' CLIPVisionModel on the resident RGBX u8 images of augment.py, CLIP's Normalize included:
//     h0[b, 0]     = class_embedding + pos[0]
//     h0[b, 1 + p] = conv2d(normalise(image b), W, stride = patch)[p] + pos[1 + p]
// as ONE implicit GEMM on v_mfma_f32_16x16x32 (no im2col buffer in HBM).  The normalisation (x / 255 - mean_c) / std_c is folded into the
// packed weight by the host (clip_score.pack_patch_weight): W'[n, k] = W[n, c, ky, kx] / (255 std_c) in the build's 16-bit type, bias[n] =
// -sum W mean_c / std_c in fp32, so the A operand is the raw byte, exact in fp16 and bf16.  K runs in the pixel layout's order,
// k = (ky * patch + kx) * 4 + byte (R, G, B, X): a lane's 8 consecutive k are two neighbouring pixels of one patch row (patch is even, so a
// group never straddles rows).  The X byte meets a zero weight column, so whatever it holds adds exact zeros.  K is padded to the MFMA step
// with zero columns of W' (those k are never read from the image).
//
// Block = 4 waves = 64 patch rows x 64 channels; a wave owns 16 rows and four 16 x 16 accumulators.  Fragments come straight from global
// memory (a patch row is 56 contiguous bytes; W' is 1.6 MB and stays in L2): this layer is < 1 % of the tower's FLOPs, so it is kept simple.
#include "../../include/textboost_hip.h"
#include "common.h"

namespace {

__device__ __forceinline__ void bytes_to_half4(uint32_t v, f16x8& a, int o) {
  a[o + 0] = (f16)(float)(v & 255u);
  a[o + 1] = (f16)(float)((v >> 8) & 255u);
  a[o + 2] = (f16)(float)((v >> 16) & 255u);
  a[o + 3] = (f16)(float)(v >> 24);
}

__global__ __launch_bounds__(256) void clip_patch_embed_kernel(const uint32_t* __restrict__ img, int64_t img_stride, int64_t row_stride,
                                                               int B, int npx, int patch, const f16* __restrict__ W, int64_t ldw, int K,
                                                               int Kp, const float* __restrict__ bias, const float* __restrict__ cls,
                                                               const float* __restrict__ pos, float* __restrict__ out, int64_t ldo, int D) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int P = npx * npx;
  const int64_t M = (int64_t)B * P;
  const int64_t m0 = (int64_t)blockIdx.x * 64 + wave * 16;
  const int n0 = blockIdx.y * 64;

  // class rows: written once per image by the first row of blocks
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < B * 64; i += 256) {
      const int b = i >> 6, n = n0 + (i & 63);
      if (n < D) out[(int64_t)b * (1 + P) * ldo + n] = cls[n] + pos[n];
    }
  }

  // A fragment of this lane: patch row m0 + (lane & 15), k = k0 + 8 (lane >> 4) + j
  const int64_t m = m0 + (lane & 15);
  const bool mvalid = m < M;
  const uint32_t* base = img;
  if (mvalid) {
    const int b = (int)(m / P), p = (int)(m % P);
    base = img + b * img_stride + (int64_t)(p / npx) * patch * row_stride + (int64_t)(p % npx) * patch;
  }
  const int kq = 8 * (lane >> 4);
  const int krow = 4 * patch;  // k per patch row
  const f16* wrow = W + (int64_t)(n0 + (lane & 15)) * ldw + kq;
  f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  const f16x8 zero8 = {};
  for (int k0 = 0; k0 < Kp; k0 += 32) {
    const int k = k0 + kq;
    f16x8 a = zero8;
    if (mvalid && k < K) {
      const int ky = k / krow, kx = (k - ky * krow) >> 2;
      const uint32_t* src = base + ky * row_stride + kx;
      bytes_to_half4(src[0], a, 0);
      bytes_to_half4(src[1], a, 4);
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
      if (n0 + 16 * t < D) {  // D % 16 == 0: uniform across the wave
        const f16x8 w = *(const f16x8*)(wrow + (int64_t)16 * t * ldw + k0);
        acc[t] = TB_MFMA_16x16x32(a, w, acc[t]);
      }
    }
  }

  // C/D: register r of lane l is row 4 (l >> 4) + r, column l & 15 of the 16 x 16 tile
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int n = n0 + 16 * t + (lane & 15);
    if (n >= D) continue;
    const float bn = bias[n];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t row = m0 + 4 * (lane >> 4) + r;
      if (row >= M) continue;
      const int b = (int)(row / P), p = (int)(row % P);
      out[((int64_t)b * (1 + P) + 1 + p) * ldo + n] = (acc[t][r] + bn) + pos[(int64_t)(1 + p) * D + n];
    }
  }
}

}  // namespace

extern "C" int tb_clip_patch_embed(const uint32_t* img, int64_t img_stride, int64_t row_stride, int B, int S, int patch, const void* w,
                                   int64_t ldw, int Kp, const float* bias, const float* cls, const float* pos, float* out, int64_t ldo, int D,
                                   tb_stream_t stream) {
  (void)hipGetLastError();  // drop any stale (non-sticky) error left by an earlier runtime call
  if (!img || !w || !bias || !cls || !pos || !out) return TB_EINVAL;
  if (B <= 0 || S <= 0 || patch <= 0 || patch % 2 || S % patch || D <= 0 || D % 16) return TB_EINVAL;
  const int K = 4 * patch * patch;
  if (Kp < K || Kp % 32 || ldw < Kp || ldw % 8 || ((uintptr_t)w) % 16 || ldo < D) return TB_EINVAL;
  if (row_stride < S || img_stride < (int64_t)(S - 1) * row_stride + S) return TB_EINVAL;
  const int npx = S / patch;
  const int64_t M = (int64_t)B * npx * npx;
  dim3 grid((unsigned)((M + 63) / 64), (unsigned)((D + 63) / 64));
  hipLaunchKernelGGL(clip_patch_embed_kernel, grid, dim3(256), 0, (hipStream_t)stream, img, img_stride, row_stride, B, npx, patch,
                     (const f16*)w, ldw, K, Kp, bias, cls, pos, out, ldo, D);
  TB_CHECK_LAUNCH();
  return TB_OK;
}
