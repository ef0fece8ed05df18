// The two FIR resamplers of the k-diffusion UNet (MonsterDiffusion: base/layers.py:208-241), 16-bit NHWC, C a multiple of 8:
//   pmi_fir_down2   reflect-pad 1, depthwise 4x4 kernel k k^T with k = [1, 3, 3, 1] / 8, stride 2        [N, H, W, C] -> [N, H/2, W/2, C]
//   pmi_fir_up2     reflect-pad 1, conv_transpose2d with (2k)(2k)^T, stride 2, padding 3                  [N, H, W, C] -> [N, 2H, 2W, C]
// Per axis the transposed convolution is out[2y] = 1/4 x[refl(y - 1)] + 3/4 x[y], out[2y + 1] = 3/4 x[y] + 1/4 x[refl(y + 1)]: bilinear x2
// in the interior, but the border row is REFLECTED (x[-1] = x[1]), not clamped -- pmi_upsample_bilinear2 is a different operator there.
// The reflection is index arithmetic (no padded copy).  HBM-bound streaming kernels: one thread per output pixel and 8 channels, 16-byte
// loads and stores, every tap weight (1, 3, 9 over 64 resp. 16) exact in fp32, fp32 sums, one rounding at the store.
#include "common.h"
#include "launch_util.h"
#include "../../include/perceptor_hip.h"

namespace {

// index -1 .. n of an axis of n >= 2 samples under reflect padding by one
__device__ __forceinline__ int refl(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }

template <typename T>
__global__ __launch_bounds__(256) void fir_down2_kernel(const u16* __restrict__ x, u16* __restrict__ y, int N, int H, int W, int C) {
  const int C8 = C >> 3, Ho = H / 2, Wo = W / 2;
  const int64_t total = (int64_t)N * Ho * Wo * C8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(i % C8);
    const int64_t pix = i / C8;
    const int n = (int)(pix / ((int64_t)Ho * Wo));
    const int rem = (int)(pix - (int64_t)n * Ho * Wo);
    const int oy = rem / Wo, ox = rem - oy * Wo;
    const u16* b = x + (int64_t)n * H * W * C + c8 * 8;
    int col[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) col[t] = refl(2 * ox - 1 + t, W);
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const u16* row = b + (int64_t)refl(2 * oy - 1 + r, H) * W * C;
      const float wr = (r == 0 || r == 3) ? 1.f : 3.f;
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float f[8];
        unpack8<T>(*(const uint4*)(row + (int64_t)col[t] * C), f);
        const float wgt = wr * ((t == 0 || t == 3) ? 1.f : 3.f) * 0.015625f;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += wgt * f[e];
      }
    }
    *(uint4*)(y + pix * C + c8 * 8) = pack8<T>(o);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void fir_up2_kernel(const u16* __restrict__ x, u16* __restrict__ y, int N, int H, int W, int C) {
  const int C8 = C >> 3, Ho = H * 2, Wo = W * 2;
  const int64_t total = (int64_t)N * Ho * Wo * C8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(i % C8);
    const int64_t pix = i / C8;
    const int n = (int)(pix / ((int64_t)Ho * Wo));
    const int rem = (int)(pix - (int64_t)n * Ho * Wo);
    const int oy = rem / Wo, ox = rem - oy * Wo;
    const int iy = oy >> 1, ix = ox >> 1;
    const int y1 = refl((oy & 1) ? iy + 1 : iy - 1, H);       // the 1/4 neighbour of each axis
    const int x1 = refl((ox & 1) ? ix + 1 : ix - 1, W);
    const u16* b = x + (int64_t)n * H * W * C + c8 * 8;
    float a00[8], a01[8], a10[8], a11[8], o[8];
    unpack8<T>(*(const uint4*)(b + ((int64_t)iy * W + ix) * C), a00);
    unpack8<T>(*(const uint4*)(b + ((int64_t)iy * W + x1) * C), a01);
    unpack8<T>(*(const uint4*)(b + ((int64_t)y1 * W + ix) * C), a10);
    unpack8<T>(*(const uint4*)(b + ((int64_t)y1 * W + x1) * C), a11);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.5625f * a00[e] + 0.1875f * a01[e] + 0.1875f * a10[e] + 0.0625f * a11[e];
    *(uint4*)(y + pix * C + c8 * 8) = pack8<T>(o);
  }
}

}  // namespace

#define ST ((hipStream_t)s)

extern "C" int pmi_fir_down2(const void* x, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!x || !y || N <= 0 || H < 2 || W < 2 || (H & 1) || (W & 1) || C <= 0 || (C & 7) || (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16)) return PMI_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)y) & 15)) return PMI_ERR_ARG;
  dim3 grid(grid_256((int64_t)N * (H / 2) * (W / 2) * (C / 8))), block(256);
  if (dtype == PMI_DT_BF16) hipLaunchKernelGGL(fir_down2_kernel<BF16>, grid, block, 0, ST, (const u16*)x, (u16*)y, N, H, W, C);
  else hipLaunchKernelGGL(fir_down2_kernel<F16>, grid, block, 0, ST, (const u16*)x, (u16*)y, N, H, W, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_fir_up2(const void* x, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!x || !y || N <= 0 || H < 2 || W < 2 || C <= 0 || (C & 7) || (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16)) return PMI_ERR_ARG;
  if ((((uintptr_t)x | (uintptr_t)y) & 15)) return PMI_ERR_ARG;
  dim3 grid(grid_256((int64_t)N * H * W * 4 * (C / 8))), block(256);
  if (dtype == PMI_DT_BF16) hipLaunchKernelGGL(fir_up2_kernel<BF16>, grid, block, 0, ST, (const u16*)x, (u16*)y, N, H, W, C);
  else hipLaunchKernelGGL(fir_up2_kernel<F16>, grid, block, 0, ST, (const u16*)x, (u16*)y, N, H, W, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
