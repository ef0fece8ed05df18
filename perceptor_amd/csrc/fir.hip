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

// ---- adjoints (the input gradient of MonsterEngine) -------------------------------------------------------------------------------------
// Exact transposes of the two operators above, reflection included, in gather form: one thread per dx pixel and 8 channels, no atomics.
// Per axis an input index i receives a fixed set of taps, held as (index, weight) slots whose weight is 0 where the tap does not exist:
//   down (H even, Ho = H / 2; weights over 8):  3 dy[i >> 1];  1 dy[i odd ? (i + 1) / 2 : i / 2 - 1] where that output exists;
//                                               the folds: 1 dy[0] into i = 1 (padded -1), 1 dy[Ho - 1] into i = H - 2 (padded H)
//   up   (dy has 2H rows; weights over 4):      3 dy[2i], 3 dy[2i + 1];  1 dy[2i + 2] (i < H - 1), 1 dy[2i - 1] (i > 0);
//                                               the folds: 1 dy[0] into i = 1, 1 dy[2H - 1] into i = H - 2 (both at H = 3: six terms)
// The 2-D operator is the outer product; every weight (1, 3, 9 over 64 resp. 16) times a 16-bit value is exact in fp32.
struct tap { int idx; float w; };

__device__ __forceinline__ void down_bwd_taps(int i, int n, tap t[3]) {
  const int no = n >> 1, odd = i & 1;
  t[0].idx = i >> 1; t[0].w = 3.f;
  const int o1 = odd ? (i + 1) >> 1 : (i >> 1) - 1;
  const bool v1 = o1 >= 0 && o1 < no;
  t[1].idx = v1 ? o1 : 0; t[1].w = v1 ? 1.f : 0.f;
  const bool f0 = i == 1, f1 = i == n - 2;                   // never both: n is even
  t[2].idx = f1 ? no - 1 : 0; t[2].w = (f0 || f1) ? 1.f : 0.f;
}

__device__ __forceinline__ void up_bwd_taps(int i, int n, tap t[6]) {
  t[0].idx = 2 * i; t[0].w = 3.f;
  t[1].idx = 2 * i + 1; t[1].w = 3.f;
  t[2].idx = i < n - 1 ? 2 * i + 2 : 0; t[2].w = i < n - 1 ? 1.f : 0.f;
  t[3].idx = i > 0 ? 2 * i - 1 : 0; t[3].w = i > 0 ? 1.f : 0.f;
  t[4].idx = 0; t[4].w = i == 1 ? 1.f : 0.f;
  t[5].idx = 2 * n - 1; t[5].w = i == n - 2 ? 1.f : 0.f;
}

// dy [N, Hs, Ws, C] -> dx [N, H, W, C]; UP: Hs = 2H with six slots per axis and weights over 16, else Hs = H / 2, three slots, over 64
template <typename T, bool UP>
__global__ __launch_bounds__(256) void fir_bwd_kernel(const u16* __restrict__ dy, u16* __restrict__ dx, int N, int H, int W, int C) {
  constexpr int S = UP ? 6 : 3;
  constexpr float unit = UP ? 0.0625f : 0.015625f;
  const int C8 = C >> 3, Hs = UP ? 2 * H : H / 2, Ws = UP ? 2 * W : W / 2;
  const int64_t total = (int64_t)N * H * W * C8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c8 = (int)(i % C8);
    const int64_t pix = i / C8;
    const int n = (int)(pix / ((int64_t)H * W));
    const int rem = (int)(pix - (int64_t)n * H * W);
    const int iy = rem / W, ix = rem - iy * W;
    tap ty[S], tx[S];
    if (UP) { up_bwd_taps(iy, H, ty); up_bwd_taps(ix, W, tx); }
    else { down_bwd_taps(iy, H, ty); down_bwd_taps(ix, W, tx); }
    const u16* b = dy + (int64_t)n * Hs * Ws * C + c8 * 8;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
#pragma unroll
    for (int r = 0; r < S; ++r) {
      if (ty[r].w == 0.f) continue;
      const u16* row = b + (int64_t)ty[r].idx * Ws * C;
#pragma unroll
      for (int t = 0; t < S; ++t) {
        if (tx[t].w == 0.f) continue;
        float f[8];
        unpack8<T>(*(const uint4*)(row + (int64_t)tx[t].idx * C), f);
        const float wgt = ty[r].w * tx[t].w * unit;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] += wgt * f[e];
      }
    }
    *(uint4*)(dx + pix * C + c8 * 8) = pack8<T>(o);
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

template <bool UP>
static int fir_bwd(const void* dy, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!dy || !dx || N <= 0 || H < 2 || W < 2 || (!UP && ((H & 1) || (W & 1))) || C <= 0 || (C & 7) || (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16)) return PMI_ERR_ARG;
  if ((((uintptr_t)dy | (uintptr_t)dx) & 15)) return PMI_ERR_ARG;
  dim3 grid(grid_256((int64_t)N * H * W * (C / 8))), block(256);
  if (dtype == PMI_DT_BF16) hipLaunchKernelGGL((fir_bwd_kernel<BF16, UP>), grid, block, 0, ST, (const u16*)dy, (u16*)dx, N, H, W, C);
  else hipLaunchKernelGGL((fir_bwd_kernel<F16, UP>), grid, block, 0, ST, (const u16*)dy, (u16*)dx, N, H, W, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_fir_down2_bwd(const void* dy, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  return fir_bwd<false>(dy, dx, N, H, W, C, dtype, s);
}

extern "C" int pmi_fir_up2_bwd(const void* dy, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  return fir_bwd<true>(dy, dx, N, H, W, C, dtype, s);
}

// ---- the 8-tap "cubic" resamplers of the DeepImagePrior skip network (deep_image_prior/updown.py) ----------------------------------------------
//   pmi_fir8_down2   reflect-pad 3, depthwise 8x8 kernel k k^T, k = [-3, -9, 29, 111, 111, 29, -9, -3] / 256, stride 2   [N, H, W, C] -> [N, H/2, W/2, C]
//   pmi_fir8_up2     reflect-pad 2, conv_transpose2d with (2k)(2k)^T, stride 2, padding 7                               [N, H, W, C] -> [N, 2H, 2W, C]
// Per axis: down[o] = sum_t k[t] x[refl(2o - 3 + t)];  up[2m] = sum_d 2k[7 - 2d] x[refl(m + d - 2)],  up[2m + 1] = sum_d 2k[6 - 2d] x[refl(m + d - 1)].
// The long-kernel siblings of the 4-tap kernels above: reflection as index arithmetic, one thread per output pixel and 4 channels (C a multiple
// of 4: the network's 4-channel skip shares them), fp32 sums, one rounding at the store.  The source of down2 and the destination of down2_bwd
// may carry a one-pixel ring ([N, H + 2, W + 2, C], interior H x W): the 3x3 convolutions beside them run on ringed tensors.
// Adjoints in gather form: an input index i is read through the padded positions u = i, u = -i (1 <= i <= pad) and u = 2(n - 1) - i (when
// that lies in n .. n + pad - 1); each u collects the outputs whose taps reach it.  No atomics.
namespace {

__constant__ float k8[8] = {-0.01171875f, -0.03515625f, 0.11328125f, 0.43359375f, 0.43359375f, 0.11328125f, -0.03515625f, -0.01171875f};

__device__ __forceinline__ int refl_n(int i, int n) { return i < 0 ? -i : (i >= n ? 2 * (n - 1) - i : i); }
__device__ __forceinline__ int64_t ring_off(int n, int y, int x, int H, int W, int r, int C) {
  return (((int64_t)n * (H + 2 * r) + (y + r)) * (W + 2 * r) + (x + r)) * C;
}
template <typename T>
__device__ __forceinline__ void ld4(const u16* p, float* f) {
  const uint2 v = *(const uint2*)p;
  f[0] = T::to_f((u16)(v.x & 0xffff)); f[1] = T::to_f((u16)(v.x >> 16));
  f[2] = T::to_f((u16)(v.y & 0xffff)); f[3] = T::to_f((u16)(v.y >> 16));
}

template <typename T>
__global__ __launch_bounds__(256) void fir8_down2_kernel(const u16* __restrict__ x, int xr, u16* __restrict__ y, int N, int H, int W, int C) {
  const int G = C >> 2, Ho = H / 2, Wo = W / 2;
  const int64_t total = (int64_t)N * Ho * Wo * G;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % G);
    const int64_t pix = i / G;
    const int n = (int)(pix / ((int64_t)Ho * Wo)), rem = (int)(pix - (int64_t)n * Ho * Wo), oy = rem / Wo, ox = rem - oy * Wo;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < 8; ++r) {
      const int iy = refl_n(2 * oy - 3 + r, H);
#pragma unroll
      for (int t = 0; t < 8; ++t) {
        float f[4];
        ld4<T>(x + ring_off(n, iy, refl_n(2 * ox - 3 + t, W), H, W, xr, C) + 4 * g, f);
        const float wgt = k8[r] * k8[t];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf(wgt, f[e], o[e]);
      }
    }
    *(uint2*)(y + pix * C + 4 * g) = pack4<T>(o[0], o[1], o[2], o[3]);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void fir8_up2_kernel(const u16* __restrict__ x, u16* __restrict__ y, int N, int H, int W, int C) {
  const int G = C >> 2, Ho = 2 * H, Wo = 2 * W;
  const int64_t total = (int64_t)N * Ho * Wo * G;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % G);
    const int64_t pix = i / G;
    const int n = (int)(pix / ((int64_t)Ho * Wo)), rem = (int)(pix - (int64_t)n * Ho * Wo), oy = rem / Wo, ox = rem - oy * Wo;
    const int py = oy & 1, px = ox & 1, my = oy >> 1, mx = ox >> 1;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 4; ++a) {
      const int iy = refl_n(my + a - 2 + py, H);
      const float wy = 2.f * k8[7 - py - 2 * a];
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        float f[4];
        ld4<T>(x + (((int64_t)n * H + iy) * W + refl_n(mx + b - 2 + px, W)) * C + 4 * g, f);
        const float wgt = wy * (2.f * k8[7 - px - 2 * b]);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf(wgt, f[e], o[e]);
      }
    }
    *(uint2*)(y + pix * C + 4 * g) = pack4<T>(o[0], o[1], o[2], o[3]);
  }
}

// (index, weight) of every output that reads input i of an axis of n samples; at most 12 (down) or 24 (up) entries
template <bool UP>
__device__ __forceinline__ int fir8_bwd_taps(int i, int n, int* idx, float* w) {
  constexpr int PAD = UP ? 2 : 3;
  const int hi = 2 * (n - 1) - i;
  const int u[3] = {i, -i, hi};
  const bool v[3] = {true, i >= 1 && i <= PAD, hi >= n && hi <= n + PAD - 1};
  int cnt = 0;
  for (int c = 0; c < 3; ++c) {
    if (!v[c]) continue;
    if (UP) {
      for (int d = 0; d < 4; ++d) {
        const int m0 = u[c] - d + 2, m1 = u[c] - d + 1;
        if (m0 >= 0 && m0 < n) { idx[cnt] = 2 * m0; w[cnt] = 2.f * k8[7 - 2 * d]; ++cnt; }
        if (m1 >= 0 && m1 < n) { idx[cnt] = 2 * m1 + 1; w[cnt] = 2.f * k8[6 - 2 * d]; ++cnt; }
      }
    } else {
      for (int t = 0; t < 8; ++t) {
        const int q = u[c] + 3 - t;
        if (q < 0 || (q & 1) || (q >> 1) >= n / 2) continue;
        idx[cnt] = q >> 1; w[cnt] = k8[t]; ++cnt;
      }
    }
  }
  return cnt;
}

// dy [N, Hs, Ws, C] (Hs = 2H up, H / 2 down) -> dx with ring dxr, interior [N, H, W, C]
template <typename T, bool UP>
__global__ __launch_bounds__(256) void fir8_bwd_kernel(const u16* __restrict__ dy, u16* __restrict__ dx, int dxr, int N, int H, int W, int C) {
  constexpr int S = UP ? 24 : 12;
  const int G = C >> 2, Hs = UP ? 2 * H : H / 2, Ws = UP ? 2 * W : W / 2;
  const int64_t total = (int64_t)N * H * W * G;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % G);
    const int64_t pix = i / G;
    const int n = (int)(pix / ((int64_t)H * W)), rem = (int)(pix - (int64_t)n * H * W), iy = rem / W, ix = rem - iy * W;
    int yi[S], xi[S];
    float yw[S], xw[S];
    const int ny = fir8_bwd_taps<UP>(iy, H, yi, yw), nx = fir8_bwd_taps<UP>(ix, W, xi, xw);
    const u16* b = dy + (int64_t)n * Hs * Ws * C + 4 * g;
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < ny; ++r) {
      const u16* row = b + (int64_t)yi[r] * Ws * C;
      for (int t = 0; t < nx; ++t) {
        float f[4];
        ld4<T>(row + (int64_t)xi[t] * C, f);
        const float wgt = yw[r] * xw[t];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = fmaf(wgt, f[e], o[e]);
      }
    }
    *(uint2*)(dx + ring_off(n, iy, ix, H, W, dxr, C) + 4 * g) = pack4<T>(o[0], o[1], o[2], o[3]);
  }
}

inline bool fir8_ok(const void* a, const void* b, int N, int H, int W, int C, int ring, int dtype, int hmin, bool even) {
  return a && b && N > 0 && H >= hmin && W >= hmin && !(even && ((H & 1) || (W & 1))) && C > 0 && !(C & 3) && (ring == 0 || ring == 1) &&
         (int64_t)N * (2 * H + 2) * (2 * W + 2) < (1ll << 31) && !(((uintptr_t)a | (uintptr_t)b) & 7) && (dtype == PMI_DT_F16 || dtype == PMI_DT_BF16);
}

}  // namespace

extern "C" int pmi_fir8_down2(const void* x, int x_ring, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!fir8_ok(x, y, N, H, W, C, x_ring, dtype, 4, true)) return PMI_ERR_ARG;
  dim3 grid(grid_256((int64_t)N * (H / 2) * (W / 2) * (C / 4))), block(256);
  if (dtype == PMI_DT_BF16) hipLaunchKernelGGL(fir8_down2_kernel<BF16>, grid, block, 0, ST, (const u16*)x, x_ring, (u16*)y, N, H, W, C);
  else hipLaunchKernelGGL(fir8_down2_kernel<F16>, grid, block, 0, ST, (const u16*)x, x_ring, (u16*)y, N, H, W, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_fir8_up2(const void* x, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!fir8_ok(x, y, N, H, W, C, 0, dtype, 3, false)) return PMI_ERR_ARG;
  dim3 grid(grid_256((int64_t)N * H * W * 4 * (C / 4))), block(256);
  if (dtype == PMI_DT_BF16) hipLaunchKernelGGL(fir8_up2_kernel<BF16>, grid, block, 0, ST, (const u16*)x, (u16*)y, N, H, W, C);
  else hipLaunchKernelGGL(fir8_up2_kernel<F16>, grid, block, 0, ST, (const u16*)x, (u16*)y, N, H, W, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_fir8_down2_bwd(const void* dy, void* dx, int dx_ring, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!fir8_ok(dy, dx, N, H, W, C, dx_ring, dtype, 4, true)) return PMI_ERR_ARG;
  dim3 grid(grid_256((int64_t)N * H * W * (C / 4))), block(256);
  if (dtype == PMI_DT_BF16) hipLaunchKernelGGL((fir8_bwd_kernel<BF16, false>), grid, block, 0, ST, (const u16*)dy, (u16*)dx, dx_ring, N, H, W, C);
  else hipLaunchKernelGGL((fir8_bwd_kernel<F16, false>), grid, block, 0, ST, (const u16*)dy, (u16*)dx, dx_ring, N, H, W, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_fir8_up2_bwd(const void* dy, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!fir8_ok(dy, dx, N, H, W, C, 0, dtype, 3, false)) return PMI_ERR_ARG;
  dim3 grid(grid_256((int64_t)N * H * W * (C / 4))), block(256);
  if (dtype == PMI_DT_BF16) hipLaunchKernelGGL((fir8_bwd_kernel<BF16, true>), grid, block, 0, ST, (const u16*)dy, (u16*)dx, 0, N, H, W, C);
  else hipLaunchKernelGGL((fir8_bwd_kernel<F16, true>), grid, block, 0, ST, (const u16*)dy, (u16*)dx, 0, N, H, W, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
