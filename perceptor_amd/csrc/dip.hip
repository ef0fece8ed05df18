// Training-mode kernels of the DeepImagePrior skip network (engine/dip.py): the first kernels here that differentiate a network to its WEIGHTS.
//   pmi_dip_pack_w         fp32 [Cout, Cin, kh, kw] parameters -> the 16-bit forward packing B[n_p][tap][cin_p] of pmi_igemm and the transposed,
//                          tap-reversed packing of the input-gradient convolution, on the device, every forward (nothing derived is cached)
//   pmi_dip_wgrad          dW[co][ci][ky][kx] = sum_{n,y,x} dY[n,y,x,co] Xpad[n,y+ky,x+kx,ci] and db = sum dY: a GEMM whose reduction runs over the
//                          pixels.  Cout > 4: mfma_f32_32x32x16 on [pixel][channel] LDS tiles read with ds_read_b64_tr_b16 (both operands are
//                          pixel-major, the reduction index is the slow axis of both); Cout <= 4 (the 4-channel skip and the 3-channel head): a
//                          plain fp32 reduction, one thread per input channel.  Both write fp32 slabs per pixel range; one fixed-order reduce sums
//                          them into PyTorch's layout.  No floating-point atomics: two runs agree bit for bit.
//   pmi_dip_bn_stats       BatchNorm2d batch statistics of an NHWC tensor: per-workgroup partial sums, the mean, a CENTRED second pass for the
//                          variance (no E[x^2] - E[x]^2), then 1/sigma and the running statistics (momentum, unbiased variance)
//   pmi_dip_bn_apply       y = act(a x + b), a = gamma / sigma, b = beta - mean a, act in {none, LeakyReLU 0.2}; the destination may be a channel
//                          slice of a wider tensor and may carry a reflected one-pixel ring
//   pmi_dip_bn_bwd         sum dy' and sum dy' xhat (dy' = dy act'), dgamma, dbeta, then dx = gamma / sigma (dy' - mean(dy') - xhat mean(dy' xhat))
//   pmi_dip_reflect_pad    the one-pixel reflected ring of a 3x3 convolution's input;  pmi_dip_pad_fold: its adjoint (ring rows added onto their mirrors)
//   pmi_dip_head_fwd/_bwd  1x1 convolution to <= 4 channels with fp32 weights, bias, the decorrelated-colour matrix and the sigmoid, NCHW fp32 out;
//                          backward: sigmoid', the matrix transpose, the 16-bit NHWC dY (8 channels, zero padded) the weight gradient reads
// Tensors: NHWC 16-bit (bf16 / f16 behind dtype), C a multiple of 4, 8-byte vectors.  A tensor "with ring r" is [N, H + 2r, W + 2r, ld] whose
// interior is the H x W map.  Statistics, parameters and their gradients are fp32.
#include "common.h"
#include "launch_util.h"
#include "../../include/perceptor_hip.h"

namespace {

__device__ __forceinline__ int64_t pix_off(int n, int y, int x, int H, int W, int r, int ld) {
  return (((int64_t)n * (H + 2 * r) + (y + r)) * (W + 2 * r) + (x + r)) * ld;
}

template <typename T>
__device__ __forceinline__ void load4(const u16* p, float* f) {
  const uint2 v = *(const uint2*)p;
  f[0] = T::to_f((u16)(v.x & 0xffff)); f[1] = T::to_f((u16)(v.x >> 16));
  f[2] = T::to_f((u16)(v.y & 0xffff)); f[3] = T::to_f((u16)(v.y >> 16));
}
template <typename T>
__device__ __forceinline__ void store4(u16* p, const float* f) { *(uint2*)p = pack4<T>(f[0], f[1], f[2], f[3]); }

__device__ __forceinline__ float lrelu_slope(float pre, int act) { return (act && !(pre > 0.f)) ? 0.2f : 1.f; }

// ---- weight packing -----------------------------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void pack_w_kernel(const float* __restrict__ w, u16* __restrict__ fwd, u16* __restrict__ dxp, int Cout, int Cin,
                                                     int taps, int n_p, int cin_p, int rows_p, int cout_p) {
  const int64_t tf = (int64_t)n_p * taps * cin_p, td = dxp ? (int64_t)rows_p * taps * cout_p : 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < tf + td; i += (int64_t)gridDim.x * 256) {
    if (i < tf) {
      const int ci = (int)(i % cin_p), t = (int)((i / cin_p) % taps), co = (int)(i / ((int64_t)cin_p * taps));
      fwd[i] = T::from_f((co < Cout && ci < Cin) ? w[((int64_t)co * Cin + ci) * taps + t] : 0.f);
    } else {
      const int64_t j = i - tf;
      const int co = (int)(j % cout_p), t = (int)((j / cout_p) % taps), ci = (int)(j / ((int64_t)cout_p * taps));
      dxp[j] = T::from_f((co < Cout && ci < Cin) ? w[((int64_t)co * Cin + ci) * taps + (taps - 1 - t)] : 0.f);
    }
  }
}

// ---- weight gradient ----------------------------------------------------------------------------------------------------------------------
// Workgroup = 4 waves = a 64 (co) x 64 (ci of one tap) tile, 32 pixels per step.  The step's dY and X rows go to two [32 pixel][64 channel] LDS
// images (pitch 72 elements = 144 B: 8-byte aligned blocks for the transposed read).  mfma_f32_32x32x16 takes A[row = co][k = pixel] and
// B[k = pixel][col = ci] with lane (r = l & 31, h = l >> 5) holding k = 8h .. 8h + 7: each 16-lane group g reads, twice, the 4-pixel x
// 16-channel block (pixels 16 ks + 8 (g >> 1) + {0, 4} .., channels 16 (g & 1) ..) transposed -- lane 4q + p supplies row q, channels 4p .. 4p + 3
// and lane i receives channel i of the four pixels.  Every lane runs every read (EXEC all ones): tiles are padded with zeros, never masked.
constexpr int WG_KT = 32, WG_LD = 72;
typedef short dip_s4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ uint4 tr_frag(const u16* p) {       // pixels r0 .. r0 + 3 at p, r0 + 4 .. r0 + 7 four rows further
  typedef __attribute__((address_space(3))) dip_s4* lds_s4;
  const dip_s4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)p);
  const dip_s4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(p + 4 * WG_LD));
  const uint2 ua = __builtin_bit_cast(uint2, a), ub = __builtin_bit_cast(uint2, b);
  return make_uint4(ua.x, ua.y, ub.x, ub.y);
}

template <typename T>
__global__ __launch_bounds__(256) void wgrad_mfma_kernel(const u16* __restrict__ dy, int ldy, int dyr, const u16* __restrict__ x, int ldx, int xr,
                                                         float* __restrict__ slabs, float* __restrict__ bslabs, int N, int H, int W, int Cout,
                                                         int Cin, int taps, int steps_per, int nsteps) {
  __shared__ __align__(16) u16 sa[WG_KT * WG_LD];
  __shared__ __align__(16) u16 sb[WG_KT * WG_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nct = (Cin + 63) / 64;
  const int tap = blockIdx.y / nct, ct = blockIdx.y % nct, split = blockIdx.z;
  const int ky = taps == 9 ? tap / 3 : xr, kx = taps == 9 ? tap % 3 : xr;      // raw coordinates in X's (H + 2 xr) x (W + 2 xr) grid
  const int co0 = blockIdx.x * 64, ci0 = ct * 64;
  const int cout8 = (Cout + 7) & ~7, cin8 = (Cin + 7) & ~7;
  const int64_t P = (int64_t)N * H * W;
  const int s0 = split * steps_per, s1 = min(nsteps, s0 + steps_per);
  const int prow = tid >> 3, pch = (tid & 7) * 8;
  const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3, wm = wave & 1, wn = wave >> 1;
  const int a_off = (8 * (g >> 1) + q) * WG_LD + 32 * wm + 16 * (g & 1) + 4 * pp;
  const int b_off = (8 * (g >> 1) + q) * WG_LD + 32 * wn + 16 * (g & 1) + 4 * pp;
  const bool do_bias = blockIdx.y == 0 && tid < 64;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  float bsum = 0.f;
  for (int s = s0; s < s1; ++s) {
    const int64_t p = (int64_t)s * WG_KT + prow;
    uint4 va = make_uint4(0, 0, 0, 0), vb = make_uint4(0, 0, 0, 0);
    if (p < P) {
      const int n = (int)(p / ((int64_t)H * W)), rem = (int)(p - (int64_t)n * H * W), y = rem / W, xx = rem - y * W;
      if (co0 + pch + 8 <= cout8) va = *(const uint4*)(dy + pix_off(n, y, xx, H, W, dyr, ldy) + co0 + pch);
      if (ci0 + pch + 8 <= cin8)
        vb = *(const uint4*)(x + (((int64_t)n * (H + 2 * xr) + (y + ky)) * (W + 2 * xr) + (xx + kx)) * ldx + ci0 + pch);
    }
    __syncthreads();
    *(uint4*)(sa + prow * WG_LD + pch) = va;
    *(uint4*)(sb + prow * WG_LD + pch) = vb;
    __syncthreads();
    if (do_bias) {
#pragma unroll 8
      for (int r = 0; r < WG_KT; ++r) bsum += T::to_f(sa[r * WG_LD + tid]);
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const uint4 fa = tr_frag(sa + a_off + 16 * ks * WG_LD);
      const uint4 fb = tr_frag(sb + b_off + 16 * ks * WG_LD);
      acc = T::mfma32(fa, fb, acc);
    }
  }
  float* slab = slabs + (int64_t)split * Cout * taps * Cin;
  const int ci = ci0 + 32 * wn + (lane & 31);
#pragma unroll
  for (int reg = 0; reg < 16; ++reg) {
    const int co = co0 + 32 * wm + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
    if (co < Cout && ci < Cin) slab[((int64_t)co * taps + tap) * Cin + ci] = acc[reg];
  }
  if (do_bias && co0 + tid < Cout) bslabs[(int64_t)split * Cout + co0 + tid] = bsum;
}

// Cout <= 4: grid (splits, taps); one thread per input channel walks the split's pixels
template <typename T>
__global__ __launch_bounds__(256) void wgrad_small_kernel(const u16* __restrict__ dy, int ldy, int dyr, const u16* __restrict__ x, int ldx, int xr,
                                                          float* __restrict__ slabs, float* __restrict__ bslabs, int N, int H, int W, int Cout,
                                                          int Cin, int taps, int pix_per) {
  const int split = blockIdx.x, tap = blockIdx.y, tid = threadIdx.x;
  const int ky = taps == 9 ? tap / 3 : xr, kx = taps == 9 ? tap % 3 : xr;
  const int64_t P = (int64_t)N * H * W;
  const int64_t p0 = (int64_t)split * pix_per, p1 = min(P, p0 + pix_per);
  float* slab = slabs + (int64_t)split * Cout * taps * Cin;
  for (int ci = tid; ci < Cin; ci += 256) {
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int64_t p = p0; p < p1; ++p) {
      const int n = (int)(p / ((int64_t)H * W)), rem = (int)(p - (int64_t)n * H * W), y = rem / W, xx = rem - y * W;
      const u16* d = dy + pix_off(n, y, xx, H, W, dyr, ldy);
      const float xv = T::to_f(x[(((int64_t)n * (H + 2 * xr) + (y + ky)) * (W + 2 * xr) + (xx + kx)) * ldx + ci]);
#pragma unroll
      for (int co = 0; co < 4; ++co)
        if (co < Cout) acc[co] = fmaf(T::to_f(d[co]), xv, acc[co]);
    }
#pragma unroll
    for (int co = 0; co < 4; ++co)
      if (co < Cout) slab[((int64_t)co * taps + tap) * Cin + ci] = acc[co];
  }
  if (tap == 0 && tid < Cout) {
    float bsum = 0.f;
    for (int64_t p = p0; p < p1; ++p) {
      const int n = (int)(p / ((int64_t)H * W)), rem = (int)(p - (int64_t)n * H * W), y = rem / W, xx = rem - y * W;
      bsum += T::to_f(dy[pix_off(n, y, xx, H, W, dyr, ldy) + tid]);
    }
    bslabs[(int64_t)split * Cout + tid] = bsum;
  }
}

// slabs [splits][Cout][taps][Cin] -> dW [Cout][Cin][taps] (PyTorch's layout) and db [Cout], summed in split order, times alpha
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ slabs, const float* __restrict__ bslabs, float* __restrict__ dW,
                                                           float* __restrict__ db, int Cout, int Cin, int taps, int splits, float alpha) {
  const int64_t nw = (int64_t)Cout * Cin * taps, total = nw + (db ? Cout : 0);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    float s = 0.f;
    if (i < nw) {
      const int tap = (int)(i % taps), ci = (int)((i / taps) % Cin), co = (int)(i / ((int64_t)taps * Cin));
      const int64_t src = ((int64_t)co * taps + tap) * Cin + ci;
      for (int k = 0; k < splits; ++k) s += slabs[k * nw + src];
      dW[i] = alpha * s;
    } else {
      for (int k = 0; k < splits; ++k) s += bslabs[(int64_t)k * Cout + (i - nw)];
      db[i - nw] = alpha * s;
    }
  }
}

// ---- BatchNorm, training mode ---------------------------------------------------------------------------------------------------------------
// Column reductions: thread (g = tid % G, r = tid / G) takes channels 4g .. 4g + 3 of every R-th pixel of the workgroup's range, G = C / 4,
// R = 256 / G; the R rows meet in LDS and thread g adds them in row order.  part: [blocks][C] (x ncomp).
template <typename T, int MODE = 0>     // 0: sum x   1: sum (x - mean)^2
__global__ __launch_bounds__(256) void bn_part_kernel(const u16* __restrict__ x, int ldx, int xr, const float* __restrict__ mean,
                                                      float* __restrict__ part, int N, int H, int W, int C, int pix_per) {
  __shared__ float red[256 * 4];
  const int tid = threadIdx.x, G = C >> 2, R = 256 / G, g = tid % G, r = tid / G;
  const int64_t P = (int64_t)N * H * W, p0 = (int64_t)blockIdx.x * pix_per, p1 = min(P, p0 + pix_per);
  float a[4] = {0.f, 0.f, 0.f, 0.f}, m[4] = {0.f, 0.f, 0.f, 0.f};
  if (MODE == 1) {
#pragma unroll
    for (int e = 0; e < 4; ++e) m[e] = mean[4 * g + e];
  }
  if (r < R) {
    for (int64_t p = p0 + r; p < p1; p += R) {
      const int n = (int)(p / ((int64_t)H * W)), rem = (int)(p - (int64_t)n * H * W), y = rem / W, xx = rem - y * W;
      float f[4];
      load4<T>(x + pix_off(n, y, xx, H, W, xr, ldx) + 4 * g, f);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (MODE == 0) a[e] += f[e];
        else { const float d = f[e] - m[e]; a[e] = fmaf(d, d, a[e]); }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) red[tid * 4 + e] = a[e];
  __syncthreads();
  if (tid < G) {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      float s = 0.f;
      for (int rr = 0; rr < R; ++rr) s += red[(rr * G + tid) * 4 + e];
      part[(int64_t)blockIdx.x * C + 4 * tid + e] = s;
    }
  }
}

__global__ __launch_bounds__(256) void bn_mean_kernel(const float* __restrict__ part, float* __restrict__ mean, int C, int nblk, float inv_p) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * C + c];
  mean[c] = s * inv_p;
}

__global__ __launch_bounds__(256) void bn_var_kernel(const float* __restrict__ part, const float* __restrict__ mean, float* __restrict__ rstd,
                                                     float* __restrict__ rmean, float* __restrict__ rvar, int C, int nblk, float inv_p,
                                                     float unbias, float momentum, float eps) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float s = 0.f;
  for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * C + c];
  const float var = s * inv_p;
  rstd[c] = 1.f / sqrtf(var + eps);
  if (rmean) rmean[c] = (1.f - momentum) * rmean[c] + momentum * mean[c];
  if (rvar) rvar[c] = (1.f - momentum) * rvar[c] + momentum * (var * unbias);
}

// one thread per destination pixel (ring included) and 4 channels
template <typename T>
__global__ __launch_bounds__(256) void bn_apply_kernel(const u16* __restrict__ x, int ldx, int xr, const float* __restrict__ mean,
                                                       const float* __restrict__ rstd, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       u16* __restrict__ y, int ldy, int yr, int N, int H, int W, int C, int act) {
  const int G = C >> 2, Hd = H + 2 * yr, Wd = W + 2 * yr;
  const int64_t total = (int64_t)N * Hd * Wd * G;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % G);
    const int64_t pix = i / G;
    const int n = (int)(pix / ((int64_t)Hd * Wd)), rem = (int)(pix - (int64_t)n * Hd * Wd), yd = rem / Wd, xd = rem - yd * Wd;
    int ys = yd - yr, xs = xd - yr;
    ys = ys < 0 ? -ys : (ys >= H ? 2 * (H - 1) - ys : ys);
    xs = xs < 0 ? -xs : (xs >= W ? 2 * (W - 1) - xs : xs);
    float f[4];
    load4<T>(x + pix_off(n, ys, xs, H, W, xr, ldx) + 4 * g, f);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * g + e;
      const float a = gamma[c] * rstd[c], b = fmaf(-mean[c], a, beta[c]);
      const float v = fmaf(a, f[e], b);
      f[e] = v * lrelu_slope(v, act);
    }
    store4<T>(y + pix * ldy + 4 * g, f);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_part_kernel(const u16* __restrict__ x, int ldx, int xr, const u16* __restrict__ dy, int lddy,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ part,
                                                          int N, int H, int W, int C, int act, int pix_per) {
  __shared__ float red[256 * 8];
  const int tid = threadIdx.x, G = C >> 2, R = 256 / G, g = tid % G, r = tid / G;
  const int64_t P = (int64_t)N * H * W, p0 = (int64_t)blockIdx.x * pix_per, p1 = min(P, p0 + pix_per);
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f}, m[4], rs[4], ca[4], cb[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int c = 4 * g + e;
    m[e] = mean[c]; rs[e] = rstd[c]; ca[e] = gamma[c] * rs[e]; cb[e] = fmaf(-m[e], ca[e], beta[c]);
  }
  if (r < R) {
    for (int64_t p = p0 + r; p < p1; p += R) {
      const int n = (int)(p / ((int64_t)H * W)), rem = (int)(p - (int64_t)n * H * W), y = rem / W, xx = rem - y * W;
      float f[4], d[4];
      load4<T>(x + pix_off(n, y, xx, H, W, xr, ldx) + 4 * g, f);
      load4<T>(dy + p * lddy + 4 * g, d);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float gg = d[e] * lrelu_slope(fmaf(ca[e], f[e], cb[e]), act);
        s1[e] += gg;
        s2[e] = fmaf(gg, (f[e] - m[e]) * rs[e], s2[e]);
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) { red[tid * 8 + e] = s1[e]; red[tid * 8 + 4 + e] = s2[e]; }
  __syncthreads();
  if (tid < G) {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float s = 0.f;
      for (int rr = 0; rr < R; ++rr) s += red[(rr * G + tid) * 8 + e];
      part[((int64_t)blockIdx.x * 2 + (e >> 2)) * C + 4 * tid + (e & 3)] = s;
    }
  }
}

// sums [2][C] = (sum dy', sum dy' xhat); dbeta = alpha sum dy', dgamma = alpha sum dy' xhat
__global__ __launch_bounds__(256) void bn_bwd_final_kernel(const float* __restrict__ part, float* __restrict__ sums, float* __restrict__ dgamma,
                                                           float* __restrict__ dbeta, int C, int nblk, float alpha) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= C) return;
  float a = 0.f, b = 0.f;
  for (int k = 0; k < nblk; ++k) { a += part[((int64_t)k * 2) * C + c]; b += part[((int64_t)k * 2 + 1) * C + c]; }
  sums[c] = a; sums[C + c] = b;
  if (dbeta) dbeta[c] = alpha * a;
  if (dgamma) dgamma[c] = alpha * b;
}

// dx written to the interior of a destination with ring dxr (the ring itself is the caller's zeros)
template <typename T>
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const u16* __restrict__ x, int ldx, int xr, const u16* __restrict__ dy, int lddy,
                                                           const float* __restrict__ mean, const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ sums, u16* __restrict__ dx, int lddx, int dxr, int N, int H,
                                                           int W, int C, int act, float inv_p) {
  const int G = C >> 2;
  const int64_t total = (int64_t)N * H * W * G;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % G);
    const int64_t p = i / G;
    const int n = (int)(p / ((int64_t)H * W)), rem = (int)(p - (int64_t)n * H * W), y = rem / W, xx = rem - y * W;
    float f[4], d[4];
    load4<T>(x + pix_off(n, y, xx, H, W, xr, ldx) + 4 * g, f);
    load4<T>(dy + p * lddy + 4 * g, d);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int c = 4 * g + e;
      const float m = mean[c], rs = rstd[c], a = gamma[c] * rs, b = fmaf(-m, a, beta[c]);
      const float gg = d[e] * lrelu_slope(fmaf(a, f[e], b), act), xh = (f[e] - m) * rs;
      f[e] = a * (gg - sums[c] * inv_p - xh * (sums[C + c] * inv_p));
    }
    store4<T>(dx + pix_off(n, y, xx, H, W, dxr, lddx) + 4 * g, f);
  }
}

// ---- the reflected ring of a 3x3 convolution's input and its adjoint -------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void reflect_pad_kernel(const u16* __restrict__ x, u16* __restrict__ y, int N, int H, int W, int C) {
  const int G = C >> 2, Hd = H + 2, Wd = W + 2;
  const int64_t total = (int64_t)N * Hd * Wd * G;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % G);
    const int64_t pix = i / G;
    const int n = (int)(pix / ((int64_t)Hd * Wd)), rem = (int)(pix - (int64_t)n * Hd * Wd), yd = rem / Wd, xd = rem - yd * Wd;
    int ys = yd - 1, xs = xd - 1;
    ys = ys < 0 ? -ys : (ys >= H ? 2 * (H - 1) - ys : ys);
    xs = xs < 0 ? -xs : (xs >= W ? 2 * (W - 1) - xs : xs);
    *(uint2*)(y + pix * C + 4 * g) = *(const uint2*)(x + pix_off(n, ys, xs, H, W, 0, C) + 4 * g);
  }
}

// dx[y][x] = sum of the padded gradient over every padded position that mirrors onto (y, x): itself, padded row -1 onto row 1, padded row H onto
// row H - 2 (both at H = 3), the same per column; + add.  fp32 sum of at most 9 + 1 terms, one rounding.
template <typename T>
__global__ __launch_bounds__(256) void pad_fold_kernel(const u16* __restrict__ gp, const u16* __restrict__ add, u16* __restrict__ dx, int N, int H,
                                                       int W, int C) {
  const int G = C >> 2;
  const int64_t total = (int64_t)N * H * W * G;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int g = (int)(i % G);
    const int64_t p = i / G;
    const int n = (int)(p / ((int64_t)H * W)), rem = (int)(p - (int64_t)n * H * W), y = rem / W, xx = rem - y * W;
    const int uy[3] = {y, -1, H}, ux[3] = {xx, -1, W};
    const bool vy[3] = {true, y == 1, y == H - 2}, vx[3] = {true, xx == 1, xx == W - 2};
    float o[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      if (!vy[a]) continue;
#pragma unroll
      for (int b = 0; b < 3; ++b) {
        if (!vx[b]) continue;
        float f[4];
        load4<T>(gp + pix_off(n, uy[a], ux[b], H, W, 1, C) + 4 * g, f);
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] += f[e];
      }
    }
    if (add) {
      float f[4];
      load4<T>(add + p * C + 4 * g, f);
#pragma unroll
      for (int e = 0; e < 4; ++e) o[e] += f[e];
    }
    store4<T>(dx + p * C + 4 * g, o);
  }
}

// ---- output head -------------------------------------------------------------------------------------------------------------------------------
constexpr int HEAD_MAX_CIN = 512;

template <typename T>
__global__ __launch_bounds__(256) void head_fwd_kernel(const u16* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                       const float* __restrict__ cm, float* __restrict__ out, int N, int HW, int Cin, int Cout,
                                                       int sigmoid) {
  __shared__ float sw[4 * HEAD_MAX_CIN];
  for (int i = threadIdx.x; i < Cout * Cin; i += 256) sw[i] = w[i];
  __syncthreads();
  const int64_t P = (int64_t)N * HW;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    const u16* row = x + p * Cin;
    for (int c = 0; c < Cin; c += 8) {
      float f[8];
      unpack8<T>(*(const uint4*)(row + c), f);
#pragma unroll
      for (int co = 0; co < 4; ++co) {
        if (co < Cout) {
#pragma unroll
          for (int e = 0; e < 8; ++e) z[co] = fmaf(f[e], sw[co * Cin + c + e], z[co]);
        }
      }
    }
#pragma unroll
    for (int co = 0; co < 4; ++co)
      if (co < Cout) z[co] += bias[co];
    float r[4] = {z[0], z[1], z[2], z[3]};
    if (cm) {                                    // einsum("nchw,cd->ndhw"): r[d] = sum_c z[c] cm[c][d], 3 channels
#pragma unroll
      for (int d = 0; d < 3; ++d) r[d] = fmaf(z[2], cm[6 + d], fmaf(z[1], cm[3 + d], z[0] * cm[d]));
    }
    const int n = (int)(p / HW), hw = (int)(p - (int64_t)n * HW);
#pragma unroll
    for (int d = 0; d < 4; ++d)
      if (d < Cout) out[((int64_t)n * Cout + d) * HW + hw] = sigmoid ? 1.f / (1.f + expf(-r[d])) : r[d];
  }
}

// dz [P][8] 16-bit = scale * cm (dout sigmoid'), channels Cout .. 7 zero
template <typename T>
__global__ __launch_bounds__(256) void head_bwd_kernel(const float* __restrict__ dout, const float* __restrict__ out, const float* __restrict__ cm,
                                                       u16* __restrict__ dz, int N, int HW, int Cout, int sigmoid, float scale) {
  const int64_t P = (int64_t)N * HW;
  for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < P; p += (int64_t)gridDim.x * 256) {
    const int n = (int)(p / HW), hw = (int)(p - (int64_t)n * HW);
    float dr[4] = {0.f, 0.f, 0.f, 0.f}, o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      if (d < Cout) {
        const int64_t at = ((int64_t)n * Cout + d) * HW + hw;
        const float s = out[at];
        dr[d] = dout[at] * (sigmoid ? s * (1.f - s) : 1.f);
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c < Cout) o[c] = scale * (cm ? fmaf(dr[2], cm[3 * c + 2], fmaf(dr[1], cm[3 * c + 1], dr[0] * cm[3 * c])) : dr[c]);
    }
    *(uint4*)(dz + p * 8) = pack8<T>(o);
  }
}

inline bool dt_ok(int dtype) { return dtype == PMI_DT_F16 || dtype == PMI_DT_BF16; }
inline bool al8(const void* p) { return ((uintptr_t)p & 7) == 0; }
inline bool grid_ok(int N, int H, int W) { return N > 0 && H > 0 && W > 0 && (int64_t)N * (H + 2) * (W + 2) < (1ll << 31); }
inline int bn_blocks(int64_t P) { const int64_t b = (P + 63) / 64; return (int)(b < 1 ? 1 : (b > 256 ? 256 : b)); }

}  // namespace

#define ST ((hipStream_t)s)
#define DIP_LAUNCH(K, grid, block, ...)                                                       \
  do {                                                                                        \
    if (dtype == PMI_DT_BF16) hipLaunchKernelGGL((K<BF16>), grid, block, 0, ST, __VA_ARGS__); \
    else hipLaunchKernelGGL((K<F16>), grid, block, 0, ST, __VA_ARGS__);                       \
  } while (0)

extern "C" int pmi_dip_pack_w(const float* w, void* fwd, void* dxp, int Cout, int Cin, int taps, int n_p, int cin_p, int rows_p, int cout_p,
                              int dtype, pmi_stream_t s) {
  if (!w || !fwd || Cout <= 0 || Cin <= 0 || (taps != 1 && taps != 9) || n_p < Cout || cin_p < Cin || !dt_ok(dtype)) return PMI_ERR_ARG;
  if (dxp && (rows_p < Cin || cout_p < Cout)) return PMI_ERR_ARG;
  const int64_t total = (int64_t)n_p * taps * cin_p + (dxp ? (int64_t)rows_p * taps * cout_p : 0);
  dim3 grid(grid_256(total)), block(256);
  DIP_LAUNCH(pack_w_kernel, grid, block, w, (u16*)fwd, (u16*)dxp, Cout, Cin, taps, n_p, cin_p, rows_p, cout_p);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

// pixel ranges the reduction is split into: enough workgroups to fill the device, never more than there are 32-pixel steps (MFMA route) or
// 64-pixel ranges (plain route), at most 64
extern "C" int pmi_dip_wgrad_splits(int64_t P, int Cout, int Cin, int taps) {
  if (P <= 0 || Cout <= 0 || Cin <= 0 || (taps != 1 && taps != 9)) return PMI_ERR_ARG;
  int64_t want, most;
  if (Cout <= 4) { want = 256 / taps; most = (P + 63) / 64; }
  else { const int64_t tiles = (int64_t)((Cout + 63) / 64) * taps * ((Cin + 63) / 64); want = (1024 + tiles - 1) / tiles; most = (P + WG_KT - 1) / WG_KT; }
  int64_t k = want < most ? want : most;
  k = k > 64 ? 64 : k;
  return (int)(k < 1 ? 1 : k);
}

extern "C" int pmi_dip_wgrad(const void* dy, int ldy, int dy_ring, const void* x, int ldx, int x_ring, float* slabs, float* dW, float* db, int N,
                             int H, int W, int Cout, int Cin, int taps, int splits, float alpha, int dtype, pmi_stream_t s) {
  if (!dy || !x || !slabs || !dW || !grid_ok(N, H, W) || Cout <= 0 || Cin <= 0 || (taps != 1 && taps != 9) || !dt_ok(dtype)) return PMI_ERR_ARG;
  if ((dy_ring != 0 && dy_ring != 1) || (x_ring != 0 && x_ring != 1) || (taps == 9 && x_ring != 1) || ldy < Cout || ldx < Cin) return PMI_ERR_ARG;
  const int64_t P = (int64_t)N * H * W;
  if (splits != pmi_dip_wgrad_splits(P, Cout, Cin, taps)) return PMI_ERR_ARG;
  float* bslabs = slabs + (int64_t)splits * Cout * Cin * taps;
  if (Cout <= 4) {
    const int pix_per = (int)((P + splits - 1) / splits);
    DIP_LAUNCH(wgrad_small_kernel, dim3(splits, taps), dim3(256), (const u16*)dy, ldy, dy_ring, (const u16*)x, ldx, x_ring, slabs, bslabs, N, H, W,
               Cout, Cin, taps, pix_per);
  } else {
    // 16-byte rows: whole 8-channel chunks up to the rounded channel count must lie inside a row
    if (!aligned16(dy) || !aligned16(x) || (ldy & 7) || (ldx & 7) || ldy < ((Cout + 7) & ~7) || ldx < ((Cin + 7) & ~7)) return PMI_ERR_ARG;
    const int nsteps = (int)((P + WG_KT - 1) / WG_KT), steps_per = (nsteps + splits - 1) / splits;
    dim3 grid((Cout + 63) / 64, taps * ((Cin + 63) / 64), splits);
    DIP_LAUNCH(wgrad_mfma_kernel, grid, dim3(256), (const u16*)dy, ldy, dy_ring, (const u16*)x, ldx, x_ring, slabs, bslabs, N, H, W, Cout, Cin,
               taps, steps_per, nsteps);
  }
  PMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(wgrad_reduce_kernel, dim3(grid_256((int64_t)Cout * Cin * taps + Cout)), dim3(256), 0, ST, slabs, bslabs, dW, db, Cout, Cin,
                     taps, splits, alpha);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dip_bn_blocks(int64_t P) { return P <= 0 ? PMI_ERR_ARG : bn_blocks(P); }

static bool bn_args_ok(const void* x, int ldx, int ring, int N, int H, int W, int C, int dtype) {
  return x && grid_ok(N, H, W) && C > 0 && !(C & 3) && C <= 1024 && ldx >= C && !(ldx & 3) && al8(x) && (ring == 0 || ring == 1) && dt_ok(dtype);
}

extern "C" int pmi_dip_bn_stats(const void* x, int ldx, int x_ring, float* part, float* mean, float* rstd, float* running_mean, float* running_var,
                                int N, int H, int W, int C, float momentum, float eps, int dtype, pmi_stream_t s) {
  if (!bn_args_ok(x, ldx, x_ring, N, H, W, C, dtype) || !part || !mean || !rstd || !(eps > 0.f)) return PMI_ERR_ARG;
  const int64_t P = (int64_t)N * H * W;
  if (P < 2) return PMI_ERR_ARG;                 // the unbiased variance of one sample does not exist (torch raises as well)
  const int nblk = bn_blocks(P), pix_per = (int)((P + nblk - 1) / nblk), cb = (C + 255) / 256;
  const float inv_p = (float)(1.0 / (double)P), unbias = (float)((double)P / (double)(P - 1));
  DIP_LAUNCH(bn_part_kernel, dim3(nblk), dim3(256), (const u16*)x, ldx, x_ring, (const float*)nullptr, part, N, H, W, C, pix_per);
  PMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_mean_kernel, dim3(cb), dim3(256), 0, ST, part, mean, C, nblk, inv_p);
  PMI_CHECK_LAUNCH();
  if (dtype == PMI_DT_BF16) hipLaunchKernelGGL((bn_part_kernel<BF16, 1>), dim3(nblk), dim3(256), 0, ST, (const u16*)x, ldx, x_ring, mean, part, N, H, W, C, pix_per);
  else hipLaunchKernelGGL((bn_part_kernel<F16, 1>), dim3(nblk), dim3(256), 0, ST, (const u16*)x, ldx, x_ring, mean, part, N, H, W, C, pix_per);
  PMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_var_kernel, dim3(cb), dim3(256), 0, ST, part, mean, rstd, running_mean, running_var, C, nblk, inv_p, unbias, momentum, eps);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dip_bn_apply(const void* x, int ldx, int x_ring, const float* mean, const float* rstd, const float* gamma, const float* beta,
                                void* y, int ldy, int y_ring, int N, int H, int W, int C, int act, int dtype, pmi_stream_t s) {
  if (!bn_args_ok(x, ldx, x_ring, N, H, W, C, dtype) || !mean || !rstd || !gamma || !beta || !y || !al8(y) || ldy < C || (ldy & 3)) return PMI_ERR_ARG;
  if ((y_ring != 0 && y_ring != 1) || (y_ring && (H < 2 || W < 2)) || (act != 0 && act != 1)) return PMI_ERR_ARG;
  dim3 grid(grid_256((int64_t)N * (H + 2 * y_ring) * (W + 2 * y_ring) * (C / 4))), block(256);
  DIP_LAUNCH(bn_apply_kernel, grid, block, (const u16*)x, ldx, x_ring, mean, rstd, gamma, beta, (u16*)y, ldy, y_ring, N, H, W, C, act);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dip_bn_bwd(const void* x, int ldx, int x_ring, const void* dy, int lddy, const float* mean, const float* rstd, const float* gamma,
                              const float* beta, float* part, float* sums, float* dgamma, float* dbeta, void* dx, int lddx, int dx_ring, int N, int H,
                              int W, int C, int act, float alpha, int dtype, pmi_stream_t s) {
  if (!bn_args_ok(x, ldx, x_ring, N, H, W, C, dtype) || !dy || !al8(dy) || lddy < C || (lddy & 3) || !mean || !rstd || !gamma || !beta || !part || !sums)
    return PMI_ERR_ARG;
  if (!dx || !al8(dx) || lddx < C || (lddx & 3) || (dx_ring != 0 && dx_ring != 1) || (act != 0 && act != 1)) return PMI_ERR_ARG;
  const int64_t P = (int64_t)N * H * W;
  const int nblk = bn_blocks(P), pix_per = (int)((P + nblk - 1) / nblk);
  DIP_LAUNCH(bn_bwd_part_kernel, dim3(nblk), dim3(256), (const u16*)x, ldx, x_ring, (const u16*)dy, lddy, mean, rstd, gamma, beta, part, N, H, W, C,
             act, pix_per);
  PMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(bn_bwd_final_kernel, dim3((C + 255) / 256), dim3(256), 0, ST, part, sums, dgamma, dbeta, C, nblk, alpha);
  PMI_CHECK_LAUNCH();
  DIP_LAUNCH(bn_bwd_apply_kernel, dim3(grid_256(P * (C / 4))), dim3(256), (const u16*)x, ldx, x_ring, (const u16*)dy, lddy, mean, rstd, gamma, beta,
             sums, (u16*)dx, lddx, dx_ring, N, H, W, C, act, (float)(1.0 / (double)P));
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dip_reflect_pad(const void* x, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!x || !y || !grid_ok(N, H, W) || H < 2 || W < 2 || C <= 0 || (C & 3) || !al8(x) || !al8(y) || !dt_ok(dtype)) return PMI_ERR_ARG;
  DIP_LAUNCH(reflect_pad_kernel, dim3(grid_256((int64_t)N * (H + 2) * (W + 2) * (C / 4))), dim3(256), (const u16*)x, (u16*)y, N, H, W, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dip_pad_fold(const void* gp, const void* add, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!gp || !dx || !grid_ok(N, H, W) || H < 2 || W < 2 || C <= 0 || (C & 3) || !al8(gp) || !al8(dx) || !al8(add) || !dt_ok(dtype)) return PMI_ERR_ARG;
  DIP_LAUNCH(pad_fold_kernel, dim3(grid_256((int64_t)N * H * W * (C / 4))), dim3(256), (const u16*)gp, (const u16*)add, (u16*)dx, N, H, W, C);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dip_head_fwd(const void* x, const float* w, const float* bias, const float* cm, float* out, int N, int HW, int Cin, int Cout,
                                int sigmoid, int dtype, pmi_stream_t s) {
  if (!x || !w || !bias || !out || N <= 0 || HW <= 0 || (int64_t)N * HW >= (1ll << 31) || Cin <= 0 || (Cin & 7) || Cin > HEAD_MAX_CIN || Cout < 1 ||
      Cout > 4 || (cm && Cout != 3) || !aligned16(x) || !dt_ok(dtype))
    return PMI_ERR_ARG;
  DIP_LAUNCH(head_fwd_kernel, dim3(grid_256((int64_t)N * HW)), dim3(256), (const u16*)x, w, bias, cm, out, N, HW, Cin, Cout, sigmoid);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_dip_head_bwd(const float* dout, const float* out, const float* cm, void* dz, int N, int HW, int Cout, int sigmoid, float scale,
                                int dtype, pmi_stream_t s) {
  if (!dout || !out || !dz || N <= 0 || HW <= 0 || (int64_t)N * HW >= (1ll << 31) || Cout < 1 || Cout > 4 || (cm && Cout != 3) || !aligned16(dz) ||
      !dt_ok(dtype))
    return PMI_ERR_ARG;
  DIP_LAUNCH(head_bwd_kernel, dim3(grid_256((int64_t)N * HW)), dim3(256), dout, out, cm, (u16*)dz, N, HW, Cout, sigmoid, scale);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
