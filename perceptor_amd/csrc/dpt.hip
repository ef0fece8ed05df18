// Memory-bound kernels of the DPT depth decoder (engine/dpt.py), between the convolutions that pmi_igemm runs:
//   pmi_bilinear2_ac_fwd/_bwd   F.interpolate(scale_factor=2, mode="bilinear", align_corners=True) (+ an addend on the output grid) and its exact
//                               adjoint in gather form.  The source coordinate of output row oy is oy (H - 1) / (2H - 1): its integer part and its
//                               fraction come from ONE integer division, so the weights carry a single fp32 rounding and both directions use
//                               the same weights (the adjoint identity holds to rounding of the sums only).
//   pmi_depth_to_space / pmi_space_to_depth   [N, H, W, (ky, kx, c)] <-> [N, kH, kW, c], k in {2, 4}: the layout half of ConvTranspose2d(kernel = stride = k)
//                               (the other half is one GEMM to k k C columns) plus its bias; the inverse is the adjoint's first step.
//   pmi_dpt_tap_split / _join   fp32 residual-stream tap [N, T, W] -> 16-bit patch rows [N P, W] + 16-bit class rows [N, W]; and the fp32 gradient rows
//                               back into one [N, T, W] tensor.   pmi_dpt_tap_add: a + b in fp32 and its 16-bit copy (a tap's gradient joining the walk).
//   pmi_dpt_colsum              per-image column sums of a 16-bit [N][P][W] into fp32 [N][W]: four row slices per workgroup, summed in a fixed order.
//   pmi_dpt_relu_bwd            dz = g (y > 0) (+ r): the mask is STRICTLY positive (a ReLU output is never negative, so y >= 0 would pass everything).
//   pmi_dpt_head_fwd/_bwd       the 32 -> 1 convolution, its ReLU and the sign: out = -relu(w . h + b) fp32; dh = -scale dout (z > 0) w (h > 0), 16-bit.
// 16-bit NHWC behind dtype (0 f16 / 1 bf16), fp32 arithmetic, one rounding at the store.  No atomics: two runs are bit-equal.
#include "common.h"
#include "launch_util.h"
#include "../../include/perceptor_hip.h"

namespace {

// align_corners=True source of output index o on an axis of L inputs and 2L outputs: i0, i1 and the weight of i1 (the weight of i0 is 1 - l1)
struct AcSrc { int i0, i1; float l1; };
__device__ __forceinline__ AcSrc ac_src(int o, int L) {
  const int den = 2 * L - 1, num = o * (L - 1);          // (L = 1: num = 0, den = 1)
  AcSrc s;
  s.i0 = num / den;
  s.i1 = s.i0 + (s.i0 < L - 1 ? 1 : 0);
  s.l1 = (float)(num - s.i0 * den) / (float)den;
  return s;
}

template <typename T>
__global__ __launch_bounds__(256) void bilinear_fwd_kernel(const u16* __restrict__ x, const u16* __restrict__ r, u16* __restrict__ y, int N, int H,
                                                           int W, int C) {
  const int c8 = C / 8, Ho = 2 * H, Wo = 2 * W;
  const int64_t total = (int64_t)N * Ho * Wo * c8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % c8) * 8;
    int64_t p = i / c8;
    const int ox = (int)(p % Wo); p /= Wo;
    const int oy = (int)(p % Ho);
    const int n = (int)(p / Ho);
    const AcSrc sy = ac_src(oy, H), sx = ac_src(ox, W);
    const u16* base = x + (int64_t)n * H * W * C + c;
    float a[8], b[8], cc[8], d[8], o[8];
    unpack8<T>(*(const uint4*)(base + ((int64_t)sy.i0 * W + sx.i0) * C), a);
    unpack8<T>(*(const uint4*)(base + ((int64_t)sy.i0 * W + sx.i1) * C), b);
    unpack8<T>(*(const uint4*)(base + ((int64_t)sy.i1 * W + sx.i0) * C), cc);
    unpack8<T>(*(const uint4*)(base + ((int64_t)sy.i1 * W + sx.i1) * C), d);
    const float lx1 = sx.l1, lx0 = 1.f - lx1, ly1 = sy.l1, ly0 = 1.f - ly1;
    const int64_t at = (((int64_t)n * Ho + oy) * Wo + ox) * C + c;
    float add[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (r) unpack8<T>(*(const uint4*)(r + at), add);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = ly0 * (lx0 * a[e] + lx1 * b[e]) + ly1 * (lx0 * cc[e] + lx1 * d[e]) + add[e];
    *(uint4*)(y + at) = pack8<T>(o);
  }
}

// weight with which output index o reads input index i (0 for most o)
__device__ __forceinline__ float ac_weight(int o, int i, int L) {
  const AcSrc s = ac_src(o, L);
  return (s.i0 == i ? 1.f - s.l1 : 0.f) + (s.i1 == i ? s.l1 : 0.f);
}

template <typename T>
__global__ __launch_bounds__(256) void bilinear_bwd_kernel(const u16* __restrict__ g, u16* __restrict__ dx, int N, int H, int W, int C) {
  const int c8 = C / 8, Ho = 2 * H, Wo = 2 * W;
  const int64_t total = (int64_t)N * H * W * c8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % c8) * 8;
    int64_t p = i / c8;
    const int ix = (int)(p % W); p /= W;
    const int iy = (int)(p % H);
    const int n = (int)(p / H);
    // every output index that can read input index j lies in [2j - 3, 2j + 4] (|o (L-1)/(2L-1) - j| < 1), clamped to the grid
    const int y0 = max(0, 2 * iy - 3), y1 = min(Ho - 1, 2 * iy + 4), x0 = max(0, 2 * ix - 3), x1 = min(Wo - 1, 2 * ix + 4);
    float wx[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wx[k] = (x0 + k <= x1) ? ac_weight(x0 + k, ix, W) : 0.f;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const u16* base = g + (int64_t)n * Ho * Wo * C + c;
    for (int oy = y0; oy <= y1; ++oy) {
      const float wy = ac_weight(oy, iy, H);
      if (wy == 0.f) continue;
      float row[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        if (wx[k] != 0.f) {
          float v[8];
          unpack8<T>(*(const uint4*)(base + ((int64_t)oy * Wo + (x0 + k)) * C), v);
#pragma unroll
          for (int e = 0; e < 8; ++e) row[e] = fmaf(wx[k], v[e], row[e]);
        }
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf(wy, row[e], acc[e]);
    }
    *(uint4*)(dx + (((int64_t)n * H + iy) * W + ix) * C + c) = pack8<T>(acc);
  }
}

// to_space: x [N, H, W, k k C] -> y [N, kH, kW, C] (+ bias[c]);  otherwise y [N, kH, kW, C] -> x-shaped
template <typename T, bool TO_SPACE>
__global__ __launch_bounds__(256) void depth_space_kernel(const u16* __restrict__ src, const float* __restrict__ bias, u16* __restrict__ dst, int N,
                                                          int H, int W, int C, int k) {
  const int c8 = C / 8, Ho = k * H, Wo = k * W;
  const int64_t total = (int64_t)N * Ho * Wo * c8;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % c8) * 8;
    int64_t p = i / c8;
    const int ox = (int)(p % Wo); p /= Wo;
    const int oy = (int)(p % Ho);
    const int n = (int)(p / Ho);
    const int y = oy / k, ky = oy - y * k, x = ox / k, kx = ox - x * k;
    const int64_t deep = ((((int64_t)n * H + y) * W + x) * (k * k) + (ky * k + kx)) * C + c;
    const int64_t wide = (((int64_t)n * Ho + oy) * Wo + ox) * C + c;
    if (TO_SPACE) {
      uint4 v = *(const uint4*)(src + deep);
      if (bias) {
        float f[8];
        unpack8<T>(v, f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] += bias[c + e];
        v = pack8<T>(f);
      }
      *(uint4*)(dst + wide) = v;
    } else {
      *(uint4*)(dst + deep) = *(const uint4*)(src + wide);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void tap_split_kernel(const float* __restrict__ x, u16* __restrict__ tok, u16* __restrict__ cls, int N, int Tk,
                                                        int W) {
  const int w4 = W / 4;
  const int64_t total = (int64_t)N * Tk * w4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % w4) * 4;
    const int64_t row = i / w4;
    const int t = (int)(row % Tk);
    const int n = (int)(row / Tk);
    const float4 v = *(const float4*)(x + row * W + c);
    u16* dst = t == 0 ? cls + (int64_t)n * W + c : tok + ((int64_t)n * (Tk - 1) + (t - 1)) * W + c;
    *(uint2*)dst = pack4<T>(v.x, v.y, v.z, v.w);
  }
}

__global__ __launch_bounds__(256) void tap_join_kernel(const float* __restrict__ d_tok, const float* __restrict__ d_cls, float* __restrict__ out,
                                                       int N, int T, int W) {
  const int w4 = W / 4;
  const int64_t total = (int64_t)N * T * w4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % w4) * 4;
    const int64_t row = i / w4;
    const int t = (int)(row % T);
    const int n = (int)(row / T);
    const float* src = t == 0 ? d_cls + (int64_t)n * W + c : d_tok + ((int64_t)n * (T - 1) + (t - 1)) * W + c;
    *(float4*)(out + row * W + c) = *(const float4*)src;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void tap_add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out32,
                                                      u16* __restrict__ out16, int64_t n4) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
    const float4 u = ((const float4*)a)[i], v = ((const float4*)b)[i];
    const float4 s = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
    ((float4*)out32)[i] = s;
    ((uint2*)out16)[i] = pack4<T>(s.x, s.y, s.z, s.w);
  }
}

// workgroup (n, 128-column group): lane = a column pair, the four waves take rows p = wave, wave + 4, ...; then (s0 + s1) + (s2 + s3)
template <typename T>
__global__ __launch_bounds__(256) void colsum_kernel(const u16* __restrict__ x, float* __restrict__ out, int N, int P, int W) {
  __shared__ float red[4][128];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = blockIdx.y, col = blockIdx.x * 128 + 2 * lane;
  float s0 = 0.f, s1 = 0.f;
  if (col < W) {
    const u16* base = x + (int64_t)n * P * W + col;
    for (int p = wave; p < P; p += 4) {
      const uint32_t v = *(const uint32_t*)(base + (int64_t)p * W);
      s0 += T::to_f((u16)(v & 0xffff));
      s1 += T::to_f((u16)(v >> 16));
    }
  }
  red[wave][2 * lane] = s0;
  red[wave][2 * lane + 1] = s1;
  __syncthreads();
  if (wave == 0 && col < W) {
    float* o = out + (int64_t)n * W + col;
    o[0] = (red[0][2 * lane] + red[1][2 * lane]) + (red[2][2 * lane] + red[3][2 * lane]);
    o[1] = (red[0][2 * lane + 1] + red[1][2 * lane + 1]) + (red[2][2 * lane + 1] + red[3][2 * lane + 1]);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void relu_bwd_kernel(const u16* __restrict__ g, const u16* __restrict__ y, const u16* __restrict__ r,
                                                       u16* __restrict__ dz, int64_t n8) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n8; i += (int64_t)gridDim.x * 256) {
    float gv[8], yv[8], rv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, o[8];
    unpack8<T>(((const uint4*)g)[i], gv);
    unpack8<T>(((const uint4*)y)[i], yv);
    if (r) unpack8<T>(((const uint4*)r)[i], rv);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (yv[e] > 0.f ? gv[e] : 0.f) + rv[e];
    ((uint4*)dz)[i] = pack8<T>(o);
  }
}

constexpr int HEAD_C = 32;

template <typename T>
__global__ __launch_bounds__(256) void head_fwd_kernel(const u16* __restrict__ h, const float* __restrict__ w, const float* __restrict__ b,
                                                       float* __restrict__ out, int64_t P) {
  float wr[HEAD_C];
#pragma unroll
  for (int c = 0; c < HEAD_C; ++c) wr[c] = w[c];
  const float bias = b[0];
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    float z = 0.f;
#pragma unroll
    for (int c = 0; c < HEAD_C; c += 8) {
      float f[8];
      unpack8<T>(*(const uint4*)(h + p * HEAD_C + c), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) z = fmaf(f[e], wr[c + e], z);
    }
    z += bias;
    out[p] = -(z > 0.f ? z : (z == z ? 0.f : z));          // -relu(z); a NaN stays a NaN
  }
}

// z > 0 exactly where out < 0 (out = -relu(z))
template <typename T>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out, const u16* __restrict__ h,
                                                       const float* __restrict__ w, u16* __restrict__ dh, int64_t P, float scale) {
  float wr[HEAD_C];
#pragma unroll
  for (int c = 0; c < HEAD_C; ++c) wr[c] = w[c];
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const float d = out[p] < 0.f ? -scale * dout[p] : 0.f;
#pragma unroll
    for (int c = 0; c < HEAD_C; c += 8) {
      float f[8], o[8];
      unpack8<T>(*(const uint4*)(h + p * HEAD_C + c), f);
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = f[e] > 0.f ? d * wr[c + e] : 0.f;
      *(uint4*)(dh + p * HEAD_C + c) = pack8<T>(o);
    }
  }
}

constexpr int AC_MAX = 16384;          // ac_src multiplies an output index (< 2 AC_MAX) by L - 1 in 32 bits
inline bool dt_ok(int dtype) { return dtype == PMI_DT_F16 || dtype == PMI_DT_BF16; }
// every extent of the LARGER grid (scale k per axis) at most 2^20 and its element count below 2^40: the index arithmetic is 64-bit
inline bool map_ok(int N, int H, int W, int C, int k) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7) || H > (1 << 20) / k || W > (1 << 20) / k || N > (1 << 20) || C > (1 << 20)) return false;
  return (int64_t)N * (k * H) * ((int64_t)k * W) <= (1ll << 40) / C;
}
inline bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }
inline bool rows_ok(int N, int T, int W) { return N > 0 && T >= 2 && W > 0 && (W & 3) == 0 && N <= (1 << 20) && T <= (1 << 20) && W <= (1 << 20); }

}  // namespace

#define ST ((hipStream_t)s)
#define DPT_LAUNCH(K, grid, block, ...)                                                       \
  do {                                                                                        \
    if (dtype == PMI_DT_BF16) hipLaunchKernelGGL((K<BF16>), grid, block, 0, ST, __VA_ARGS__); \
    else hipLaunchKernelGGL((K<F16>), grid, block, 0, ST, __VA_ARGS__);                       \
  } while (0)

extern "C" int pmi_bilinear2_ac_fwd(const void* x, const void* r, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!x || !y || !map_ok(N, H, W, C, 2) || H > AC_MAX || W > AC_MAX || !dt_ok(dtype) || !aligned16(x) || !aligned16(y) || !aligned16(r))
    return PMI_ERR_ARG;
  DPT_LAUNCH(bilinear_fwd_kernel, dim3(grid_256((int64_t)N * 4 * H * W * (C / 8))), dim3(256), (const u16*)x, (const u16*)r, (u16*)y, N, H, W, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_bilinear2_ac_bwd(const void* g, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!g || !dx || !map_ok(N, H, W, C, 2) || H > AC_MAX || W > AC_MAX || !dt_ok(dtype) || !aligned16(g) || !aligned16(dx)) return PMI_ERR_ARG;
  DPT_LAUNCH(bilinear_bwd_kernel, dim3(grid_256((int64_t)N * H * W * (C / 8))), dim3(256), (const u16*)g, (u16*)dx, N, H, W, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_depth_to_space(const void* x, const float* bias, void* y, int N, int H, int W, int C, int k, int dtype, pmi_stream_t s) {
  if (!x || !y || (k != 2 && k != 4) || !map_ok(N, H, W, C, k) || !dt_ok(dtype) || !aligned16(x) || !aligned16(y)) return PMI_ERR_ARG;
  const dim3 grid(grid_256((int64_t)N * k * k * H * W * (C / 8)));
  if (dtype == PMI_DT_BF16) hipLaunchKernelGGL((depth_space_kernel<BF16, true>), grid, dim3(256), 0, ST, (const u16*)x, bias, (u16*)y, N, H, W, C, k);
  else hipLaunchKernelGGL((depth_space_kernel<F16, true>), grid, dim3(256), 0, ST, (const u16*)x, bias, (u16*)y, N, H, W, C, k);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_space_to_depth(const void* y, void* x, int N, int H, int W, int C, int k, int dtype, pmi_stream_t s) {
  if (!x || !y || (k != 2 && k != 4) || !map_ok(N, H, W, C, k) || !dt_ok(dtype) || !aligned16(x) || !aligned16(y)) return PMI_ERR_ARG;
  const dim3 grid(grid_256((int64_t)N * k * k * H * W * (C / 8)));
  if (dtype == PMI_DT_BF16)
    hipLaunchKernelGGL((depth_space_kernel<BF16, false>), grid, dim3(256), 0, ST, (const u16*)y, (const float*)nullptr, (u16*)x, N, H, W, C, k);
  else hipLaunchKernelGGL((depth_space_kernel<F16, false>), grid, dim3(256), 0, ST, (const u16*)y, (const float*)nullptr, (u16*)x, N, H, W, C, k);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dpt_tap_split(const float* x, void* tok, void* cls, int N, int T, int W, int dtype, pmi_stream_t s) {
  if (!x || !tok || !cls || !rows_ok(N, T, W) || !dt_ok(dtype) || !aligned16(x) || !aligned16(tok) || !aligned16(cls)) return PMI_ERR_ARG;
  DPT_LAUNCH(tap_split_kernel, dim3(grid_256((int64_t)N * T * (W / 4))), dim3(256), x, (u16*)tok, (u16*)cls, N, T, W);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dpt_tap_join(const float* d_tok, const float* d_cls, float* out, int N, int T, int W, pmi_stream_t s) {
  if (!d_tok || !d_cls || !out || !rows_ok(N, T, W) || !aligned16(d_tok) || !aligned16(d_cls) || !aligned16(out)) return PMI_ERR_ARG;
  hipLaunchKernelGGL(tap_join_kernel, dim3(grid_256((int64_t)N * T * (W / 4))), dim3(256), 0, ST, d_tok, d_cls, out, N, T, W);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dpt_tap_add(const float* a, const float* b, float* out32, void* out16, int64_t n, int dtype, pmi_stream_t s) {
  if (!a || !b || !out32 || !out16 || n <= 0 || (n & 3) || !dt_ok(dtype) || !aligned16(a) || !aligned16(b) || !aligned16(out32) || !aligned16(out16))
    return PMI_ERR_ARG;
  DPT_LAUNCH(tap_add_kernel, dim3(grid_256(n / 4)), dim3(256), a, b, out32, (u16*)out16, n / 4);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dpt_colsum(const void* x, float* out, int N, int P, int W, int dtype, pmi_stream_t s) {
  if (!x || !out || N <= 0 || P <= 0 || W <= 0 || (W & 1) || N > 65535 || P > (1 << 20) || W > (1 << 20) || !dt_ok(dtype) || ((uintptr_t)x & 3))
    return PMI_ERR_ARG;
  DPT_LAUNCH(colsum_kernel, dim3((W + 127) / 128, N), dim3(256), (const u16*)x, out, N, P, W);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dpt_relu_bwd(const void* g, const void* y, const void* r, void* dz, int64_t n, int dtype, pmi_stream_t s) {
  if (!g || !y || !dz || n <= 0 || (n & 7) || !dt_ok(dtype) || !aligned16(g) || !aligned16(y) || !aligned16(r) || !aligned16(dz)) return PMI_ERR_ARG;
  DPT_LAUNCH(relu_bwd_kernel, dim3(grid_256(n / 8)), dim3(256), (const u16*)g, (const u16*)y, (const u16*)r, (u16*)dz, n / 8);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dpt_head_fwd(const void* h, const float* w, const float* b, float* out, int64_t P, int dtype, pmi_stream_t s) {
  if (!h || !w || !b || !out || P <= 0 || P > (1ll << 40) || !dt_ok(dtype) || !aligned16(h) || !al4(w) || !al4(b) || !al4(out)) return PMI_ERR_ARG;
  DPT_LAUNCH(head_fwd_kernel, dim3(grid_256(P)), dim3(256), (const u16*)h, w, b, out, P);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dpt_head_bwd(const float* dout, const float* out, const void* h, const float* w, void* dh, int64_t P, float scale, int dtype,
                                pmi_stream_t s) {
  if (!dout || !out || !h || !w || !dh || P <= 0 || P > (1ll << 40) || !finite_f(scale) || !dt_ok(dtype) || !aligned16(h) || !aligned16(dh) ||
      !al4(dout) || !al4(out) || !al4(w))
    return PMI_ERR_ARG;
  DPT_LAUNCH(head_bwd_kernel, dim3(grid_256(P)), dim3(256), dout, out, (const u16*)h, w, (u16*)dh, P, scale);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
