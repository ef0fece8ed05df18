// CLIP ModifiedResNet image tower (open_clip / OpenAI-CLIP RN50 .. RN50x64): the kernels the convolutions around them do not cover.
// Every convolution (BatchNorm folded), its input gradient, the pools and the ReLU masks run on pmi_igemm / pmi_avgpool2(_bwd) /
// pmi_act_fwd / pmi_act_bwd; this file adds
//   pmi_rn_stage_input / _bwd   resized NCHW fp32 image -> (x - mean) / std as 16-bit NHWC with 8 channels (3 + zero padding),
//                               the stem convolution's input; the adjoint takes its fp32 dX back to an NCHW gradient
//   pmi_rn_tokens / _bwd        AttentionPool2d's token matrix: [mean of the HW pixels | the pixels] + positional_embedding
//   pmi_rn_attn_fwd / _bwd      AttentionPool2d's single-query multi-head attention (the mean token is the only query) and its gradient
// The attention kernels are memory-bound (T x C x 2 values per image): one workgroup per (image, head) reads its K | V slice once,
// keeps the T <= RN_TMAX scores / probabilities in LDS and writes no T x T or transposed buffer.
#include "../../include/perceptor_hip.h"
#include "common.h"
#include "launch_util.h"

#define RN_TMAX 1024
#define RN_HEAD 64

namespace {

// ---- stem input staging ------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void rn_stage_input_kernel(const float* __restrict__ img, const float* __restrict__ mean,
                                                             const float* __restrict__ stdv, u16* __restrict__ out, int N, int HW) {
  const int64_t total = (int64_t)N * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int n = (int)(i / HW), p = (int)(i - (int64_t)n * HW);
    float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = (img[((int64_t)n * 3 + c) * HW + p] - mean[c]) / stdv[c];
    *(uint4*)(out + i * 8) = pack8<T>(f);
  }
}

__global__ __launch_bounds__(256) void rn_stage_input_bwd_kernel(const float* __restrict__ dx, int ldc, const float* __restrict__ stdv,
                                                                 float* __restrict__ dimg, int N, int HW, float mul) {
  const int64_t total = (int64_t)N * 3 * HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t nc = i / HW;
    const int p = (int)(i - nc * HW), c = (int)(nc % 3), n = (int)(nc / 3);
    dimg[i] = dx[((int64_t)n * HW + p) * ldc + c] / stdv[c] * mul;
  }
}

// ---- attention-pool tokens ---------------------------------------------------------------------------------------------------
// tok[n][0] = mean_p x[n][p] + pos[0], tok[n][1 + p] = x[n][p] + pos[1 + p]; the mean in fp32, each value rounded once
template <typename T>
__global__ __launch_bounds__(256) void rn_tokens_kernel(const u16* __restrict__ x, const float* __restrict__ pos, u16* __restrict__ tok,
                                                        int N, int HW, int C) {
  const int C8 = C >> 3, Tn = HW + 1;
  const int64_t total = (int64_t)N * Tn * C8;
  const float inv = 1.f / (float)HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C8) * 8;
    const int64_t r = i / C8;
    const int t = (int)(r % Tn), n = (int)(r / Tn);
    float f[8];
    if (t == 0) {
      float s[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const u16* xp = x + (int64_t)n * HW * C + c;
      for (int p = 0; p < HW; ++p) {
        unpack8<T>(*(const uint4*)(xp + (int64_t)p * C), f);
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] += f[e];
      }
#pragma unroll
      for (int e = 0; e < 8; ++e) f[e] = s[e] * inv;
    } else {
      unpack8<T>(*(const uint4*)(x + ((int64_t)n * HW + t - 1) * C + c), f);
    }
    const float* pp = pos + (int64_t)t * C + c;
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] += pp[e];
    *(uint4*)(tok + r * C + c) = pack8<T>(f);
  }
}

// adjoint of the token matrix: dx[n][p] = dtok[n][1 + p] + (dtok[n][0] + dq0[n]) / HW (dq0: the query path's gradient of row 0, fp32, optional)
template <typename T>
__global__ __launch_bounds__(256) void rn_tokens_bwd_kernel(const u16* __restrict__ dtok, const float* __restrict__ dq0, u16* __restrict__ dx,
                                                            int N, int HW, int C) {
  const int C8 = C >> 3, Tn = HW + 1;
  const int64_t total = (int64_t)N * HW * C8;
  const float inv = 1.f / (float)HW;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = (int)(i % C8) * 8;
    const int64_t r = i / C8;
    const int p = (int)(r % HW), n = (int)(r / HW);
    float f[8], g[8];
    unpack8<T>(*(const uint4*)(dtok + ((int64_t)n * Tn + 1 + p) * C + c), f);
    unpack8<T>(*(const uint4*)(dtok + (int64_t)n * Tn * C + c), g);
    if (dq0) {
#pragma unroll
      for (int e = 0; e < 8; ++e) g[e] += dq0[(int64_t)n * C + c + e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) f[e] += g[e] * inv;
    *(uint4*)(dx + r * C + c) = pack8<T>(f);
  }
}

// ---- single-query attention --------------------------------------------------------------------------------------------------
// block-wide reductions of 256 threads (4 waves); `w` is a 4-float LDS scratch that is free on entry
__device__ __forceinline__ float block_max(float v, float* w) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(w[0], w[1]), fmaxf(w[2], w[3]));
}
__device__ __forceinline__ float block_sum(float v, float* w) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = v;
  __syncthreads();
  return (w[0] + w[1]) + (w[2] + w[3]);
}

// dot of a 64-value 16-bit row with 64 floats in LDS (every lane reads the same LDS words: broadcast)
template <typename T>
__device__ __forceinline__ float dot64(const u16* __restrict__ row, const float* v) {
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float f[8];
    unpack8<T>(*(const uint4*)(row + 8 * j), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) s += v[8 * j + e] * f[e];
  }
  return s;
}

// out[d] = sum_t w[t] rows[t][d] for the 64 columns of one head: thread = (t group of 32, 8 columns), then a 32-way LDS reduction
template <typename T>
__device__ __forceinline__ float weighted_rows64(const u16* __restrict__ rows, int64_t ld, const float* w, int Tn, float (*red)[RN_HEAD + 1]) {
  const int tid = threadIdx.x, d8 = tid & 7, tg = tid >> 3;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int t = tg; t < Tn; t += 32) {
    float f[8];
    unpack8<T>(*(const uint4*)(rows + (int64_t)t * ld + d8 * 8), f);
    const float p = w[t];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += p * f[e];
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) red[tg][d8 * 8 + e] = acc[e];
  __syncthreads();
  float s = 0.f;
  if (tid < RN_HEAD) {
#pragma unroll 8
    for (int g = 0; g < 32; ++g) s += red[g][tid];
  }
  return s;
}

// q [N][C] (the projected mean token), kv [N*Tn][2C] (K | V) -> o [N][C], P [N*heads][Tn] fp32 (kept for the backward)
template <typename T>
__global__ __launch_bounds__(256) void rn_attn_fwd_kernel(const u16* __restrict__ q, const u16* __restrict__ kv, u16* __restrict__ o,
                                                          float* __restrict__ P, int Tn, int C, int heads, float scale) {
  __shared__ float sq[RN_HEAD];
  __shared__ float sp[RN_TMAX];
  __shared__ float red[32][RN_HEAD + 1];
  __shared__ float w0[4], w1[4];
  const int bh = blockIdx.x, n = bh / heads, h = bh - n * heads, tid = threadIdx.x;
  if (tid < RN_HEAD) sq[tid] = T::to_f(q[(int64_t)n * C + h * RN_HEAD + tid]) * scale;
  __syncthreads();
  const int64_t ld = 2 * (int64_t)C;
  const u16* kb = kv + (int64_t)n * Tn * ld + h * RN_HEAD;
  float m = -INFINITY;
  for (int t = tid; t < Tn; t += 256) {
    const float s = dot64<T>(kb + (int64_t)t * ld, sq);
    sp[t] = s;
    m = fmaxf(m, s);
  }
  m = block_max(m, w0);
  float l = 0.f;
  for (int t = tid; t < Tn; t += 256) {
    const float e = __expf(sp[t] - m);
    sp[t] = e;
    l += e;
  }
  const float inv = 1.f / block_sum(l, w1);
  float* Pr = P + (int64_t)bh * Tn;
  for (int t = tid; t < Tn; t += 256) {
    const float p = sp[t] * inv;
    sp[t] = p;
    Pr[t] = p;
  }
  __syncthreads();
  const float s = weighted_rows64<T>(kb + C, ld, sp, Tn, red);
  if (tid < RN_HEAD) o[(int64_t)n * C + h * RN_HEAD + tid] = T::from_f(s);
}

// dO [N][C] -> dq [N][C] (gradient of the projected query, before the scale), dkv [N*Tn][2C] (dK | dV)
template <typename T>
__global__ __launch_bounds__(256) void rn_attn_bwd_kernel(const u16* __restrict__ q, const u16* __restrict__ kv, const float* __restrict__ P,
                                                          const u16* __restrict__ dout, u16* __restrict__ dq, u16* __restrict__ dkv,
                                                          int Tn, int C, int heads, float scale) {
  __shared__ float sq[RN_HEAD], sdo[RN_HEAD];
  __shared__ float sds[RN_TMAX];
  __shared__ float red[32][RN_HEAD + 1];
  __shared__ float w0[4];
  const int bh = blockIdx.x, n = bh / heads, h = bh - n * heads, tid = threadIdx.x;
  if (tid < RN_HEAD) {
    sq[tid] = T::to_f(q[(int64_t)n * C + h * RN_HEAD + tid]);
    sdo[tid] = T::to_f(dout[(int64_t)n * C + h * RN_HEAD + tid]);
  }
  __syncthreads();
  const int64_t ld = 2 * (int64_t)C;
  const u16* kb = kv + (int64_t)n * Tn * ld + h * RN_HEAD;
  const float* Pr = P + (int64_t)bh * Tn;
  float dl = 0.f;
  for (int t = tid; t < Tn; t += 256) {
    const float dp = dot64<T>(kb + C + (int64_t)t * ld, sdo);          // dP[t] = dO . V[t]
    sds[t] = dp;
    dl += Pr[t] * dp;
  }
  const float delta = block_sum(dl, w0);                                // sum_t P dP = dO . O
  u16* db = dkv + (int64_t)n * Tn * ld + h * RN_HEAD;
  for (int t = tid; t < Tn; t += 256) {
    const float p = Pr[t];
    const float ds = p * (sds[t] - delta) * scale;
    sds[t] = ds;
    u16* dk = db + (int64_t)t * ld;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a[8], b[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) { a[e] = ds * sq[8 * j + e]; b[e] = p * sdo[8 * j + e]; }
      *(uint4*)(dk + 8 * j) = pack8<T>(a);                               // dK[t] = dS[t] q
      *(uint4*)(dk + C + 8 * j) = pack8<T>(b);                           // dV[t] = P[t] dO
    }
  }
  __syncthreads();
  const float s = weighted_rows64<T>(kb, ld, sds, Tn, red);             // dq = sum_t dS[t] K[t]
  if (tid < RN_HEAD) dq[(int64_t)n * C + h * RN_HEAD + tid] = T::from_f(s);
}

}  // namespace

#define ST ((hipStream_t)s)
#define BY_DTYPE(KERN, GRID, ...)                                                                  \
  do {                                                                                             \
    if (dtype == PMI_DT_BF16) hipLaunchKernelGGL(KERN<BF16>, GRID, dim3(256), 0, ST, __VA_ARGS__); \
    else hipLaunchKernelGGL(KERN<F16>, GRID, dim3(256), 0, ST, __VA_ARGS__);                       \
  } while (0)
#define RN_DTYPE_OK(dt) ((dt) == PMI_DT_F16 || (dt) == PMI_DT_BF16)

extern "C" int pmi_rn_stage_input(const float* img, const float* mean, const float* stdv, void* out, int N, int H, int W, int dtype,
                                  pmi_stream_t s) {
  if (!img || !mean || !stdv || !out || N <= 0 || H <= 0 || W <= 0 || !RN_DTYPE_OK(dtype)) return PMI_ERR_ARG;
  BY_DTYPE(rn_stage_input_kernel, dim3(grid_256((int64_t)N * H * W)), img, mean, stdv, (u16*)out, N, H * W);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_rn_stage_input_bwd(const float* dx, int ldc, const float* stdv, float* dimg, int N, int H, int W, float mul, pmi_stream_t s) {
  if (!dx || !stdv || !dimg || N <= 0 || H <= 0 || W <= 0 || ldc < 3) return PMI_ERR_ARG;
  hipLaunchKernelGGL(rn_stage_input_bwd_kernel, dim3(grid_256((int64_t)N * 3 * H * W)), dim3(256), 0, ST, dx, ldc, stdv, dimg, N, H * W, mul);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_rn_tokens(const void* x, const float* pos, void* tok, int N, int HW, int C, int dtype, pmi_stream_t s) {
  if (!x || !pos || !tok || N <= 0 || HW <= 0 || C <= 0 || (C & 7) || !RN_DTYPE_OK(dtype)) return PMI_ERR_ARG;
  BY_DTYPE(rn_tokens_kernel, dim3(grid_256((int64_t)N * (HW + 1) * (C / 8))), (const u16*)x, pos, (u16*)tok, N, HW, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_rn_tokens_bwd(const void* dtok, const float* dq0, void* dx, int N, int HW, int C, int dtype, pmi_stream_t s) {
  if (!dtok || !dx || N <= 0 || HW <= 0 || C <= 0 || (C & 7) || !RN_DTYPE_OK(dtype)) return PMI_ERR_ARG;
  BY_DTYPE(rn_tokens_bwd_kernel, dim3(grid_256((int64_t)N * HW * (C / 8))), (const u16*)dtok, dq0, (u16*)dx, N, HW, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_rn_attn_fwd(const void* q, const void* kv, void* o, float* P, int N, int Tn, int C, int heads, float scale, int dtype,
                               pmi_stream_t s) {
  if (!q || !kv || !o || !P || N <= 0 || Tn <= 0 || Tn > RN_TMAX || heads <= 0 || C != heads * RN_HEAD || !RN_DTYPE_OK(dtype)) return PMI_ERR_ARG;
  BY_DTYPE(rn_attn_fwd_kernel, dim3(N * heads), (const u16*)q, (const u16*)kv, (u16*)o, P, Tn, C, heads, scale);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_rn_attn_bwd(const void* q, const void* kv, const float* P, const void* dout, void* dq, void* dkv, int N, int Tn, int C,
                               int heads, float scale, int dtype, pmi_stream_t s) {
  if (!q || !kv || !P || !dout || !dq || !dkv || N <= 0 || Tn <= 0 || Tn > RN_TMAX || heads <= 0 || C != heads * RN_HEAD || !RN_DTYPE_OK(dtype))
    return PMI_ERR_ARG;
  BY_DTYPE(rn_attn_bwd_kernel, dim3(N * heads), (const u16*)q, (const u16*)kv, P, (const u16*)dout, (u16*)dq, (u16*)dkv, Tn, C, heads, scale);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
