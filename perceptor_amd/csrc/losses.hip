// Guidance losses beside the spherical CLIP loss (perceptor/losses/__init__.py), fp32 in and out, each with its gradient:
//   pmi_head_loss     linear probe on the tower's un-normalised embedding      reference: losses/simulacra_aesthetic.py:36-41 over
//                     (Simulacra rating, AVA logit / expected / probability)   models/simulacra_aesthetic/simulacra_aesthetic.py:58-60;
//                                                                              losses/aesthetic_visual_assessment.py:39-51
//   pmi_smoothness    total variation of an NCHW image                         losses/smoothness.py:5-10
//   pmi_sqdiff_loss   mean squared difference, the tail of the resize loss     losses/resize.py:14-18
// No atomics: every scalar is a two-stage sum in a fixed order (per-thread strided terms, wave shuffle tree, per-block slot in the caller's
// `partial` workspace, then one workgroup over the slots), so a result has the same bits on every run.  The image-sized kernels are
// HBM-bound streams: 16 bytes per lane where rows allow it (W % 4 == 0 / 16-byte aligned pointers), 4-byte coalesced otherwise.
//
// pmi_head_loss, mode 2 ("expected"): the reference multiplies softmax(l) by arange(1, K + 1), subtracts the target from EACH of the K
// products and takes the mean of their squares over N * K values -- it never sums the K products into an expectation.  That is kept.
#include "../../include/perceptor_hip.h"
#include "common.h"
#include "launch_util.h"

namespace {

constexpr int LB = 1024;     // first-level slots (workgroups) of the image-sized reductions
constexpr int HEAD_KMAX = 16, HEAD_DMAX = 4096;

// ------------------------------------------------------------------------------------------------------------------ head loss
// One workgroup per sample.  e = emb / max(|emb|, 1e-12); l[k] = sq * W[k].e + b[k] (sq = sqrt(D) in mode 0, else 1);
// term = this sample's share of the loss before mult / n_total; demb = c * (I - e e^T) sq W^T (dterm/dl) / |emb|, c = mult * gscale / n_total.
__global__ __launch_bounds__(256) void head_loss_kernel(const float* __restrict__ emb, const float* __restrict__ W, const float* __restrict__ b,
                                                        float* __restrict__ demb, float* __restrict__ out, float* __restrict__ partial,
                                                        int K, int D, int mode, float target, int tidx, float sq, float c) {
  __shared__ float e_s[HEAD_DMAX], g_s[HEAD_DMAX];
  __shared__ float l_s[HEAD_KMAX];
  __shared__ float red[4];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const float* row = emb + (int64_t)n * D;
  float s = 0.f;
  for (int d = tid; d < D; d += 256) { const float v = row[d]; s += v * v; }
  const float nrm = fmaxf(sqrtf(block_sum_256(s, red)), 1e-12f);
  for (int d = tid; d < D; d += 256) e_s[d] = row[d] / nrm;
  __syncthreads();
  for (int k = wid; k < K; k += 4) {
    float q = 0.f;
    for (int d = lane; d < D; d += 64) q += W[(int64_t)k * D + d] * e_s[d];
    q = wave_sum(q);
    if (lane == 0) l_s[k] = sq * q + b[k];
  }
  __syncthreads();
  // K <= 16 values: every thread works them out for itself (no further exchange)
  float l[HEAD_KMAX], dl[HEAD_KMAX];
#pragma unroll
  for (int k = 0; k < HEAD_KMAX; ++k) { l[k] = k < K ? l_s[k] : -__builtin_inff(); dl[k] = 0.f; }
  float term = 0.f;
  if (mode == 0) {
    const float df = l[0] - target;
    term = df * df;
    dl[0] = 2.f * df;
  } else if (mode == 1) {
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k)
      if (k == tidx) { term = -0.01f * l[k]; dl[k] = -0.01f; }
  } else {
    float m = l[0];
#pragma unroll
    for (int k = 1; k < HEAD_KMAX; ++k) m = fmaxf(m, l[k]);
    float p[HEAD_KMAX], z = 0.f;
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k) { p[k] = k < K ? expf(l[k] - m) : 0.f; z += p[k]; }
    float gp[HEAD_KMAX], pg = 0.f;            // gp = dterm / dp
    const float c2 = 0.01f / (float)K;
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k) {
      p[k] /= z;
      gp[k] = 0.f;
      if (mode == 2) {
        if (k < K) { const float f = p[k] * (float)(k + 1) - target; term += c2 * f * f; gp[k] = 2.f * c2 * f * (float)(k + 1); }
      } else if (k == tidx) {
        term = -p[k]; gp[k] = -1.f;
      }
      pg += p[k] * gp[k];
    }
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k) dl[k] = p[k] * (gp[k] - pg);
  }
  if (tid < K) {
    float v = 0.f;
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k) if (k == tid) v = l[k];
    out[(int64_t)n * K + tid] = v;
  }
  if (tid == 0) partial[n] = term;
  float dot = 0.f;
  for (int d = tid; d < D; d += 256) {
    float ge = 0.f;
#pragma unroll
    for (int k = 0; k < HEAD_KMAX; ++k) if (k < K) ge += dl[k] * W[(int64_t)k * D + d];
    ge *= sq;
    g_s[d] = ge;
    dot += e_s[d] * ge;
  }
  dot = block_sum_256(dot, red);
  const float cn = c / nrm;
  for (int d = tid; d < D; d += 256) demb[(int64_t)n * D + d] = cn * (g_s[d] - e_s[d] * dot);
}

// loss = scale * sum_n partial[n]: thread t adds n = t, t + 256, ... in order, then the fixed tree
__global__ __launch_bounds__(256) void head_final_kernel(const float* __restrict__ partial, int N, float* __restrict__ loss, float scale) {
  __shared__ float red[4];
  float v = 0.f;
  for (int n = threadIdx.x; n < N; n += 256) v += partial[n];
  v = block_sum_256(v, red);
  if (threadIdx.x == 0) loss[0] = v * scale;
}

// ------------------------------------------------------------------------------------------------------------------ smoothness
// V values per thread along W (V = 4 needs W % 4 == 0, so a group never crosses a row, and 16-byte aligned pointers).  Each value reads its
// four neighbours; a missing neighbour contributes nothing.  The forward differences (down, right) are the loss terms, so each is counted once.
template <int V>
__global__ __launch_bounds__(256) void smoothness_kernel(const float* __restrict__ x, float* __restrict__ grad, float* __restrict__ partial,
                                                         int64_t units, int H, int W, float gh, float gw) {
  __shared__ float red[4];
  float sh = 0.f, sw = 0.f;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
    const int64_t base = u * V, r = base / W;
    const int w0 = (int)(base - r * W), h = (int)(r % H);
    const bool has_up = h > 0, has_dn = h < H - 1;
    float c[V], up[V], dn[V], g[V];
    if constexpr (V == 4) {
      const float4 cv = *(const float4*)(x + base);
      c[0] = cv.x; c[1] = cv.y; c[2] = cv.z; c[3] = cv.w;
      if (has_up) { const float4 t = *(const float4*)(x + base - W); up[0] = t.x; up[1] = t.y; up[2] = t.z; up[3] = t.w; }
      if (has_dn) { const float4 t = *(const float4*)(x + base + W); dn[0] = t.x; dn[1] = t.y; dn[2] = t.z; dn[3] = t.w; }
    } else {
      c[0] = x[base];
      if (has_up) up[0] = x[base - W];
      if (has_dn) dn[0] = x[base + W];
    }
    const bool has_l = w0 > 0, has_r = w0 + V < W;
    const float xl = has_l ? x[base - 1] : 0.f, xr = has_r ? x[base + V] : 0.f;
#pragma unroll
    for (int e = 0; e < V; ++e) {
      float dv = 0.f, dh = 0.f;
      if (has_up) dv = c[e] - up[e];
      if (has_dn) { const float f = dn[e] - c[e]; sh += f * f; dv -= f; }
      if (e > 0) dh = c[e] - c[e - 1]; else if (has_l) dh = c[e] - xl;
      if (e + 1 < V) { const float f = c[e + 1] - c[e]; sw += f * f; dh -= f; }
      else if (has_r) { const float f = xr - c[e]; sw += f * f; dh -= f; }
      g[e] = gh * dv + gw * dh;
    }
    if constexpr (V == 4) *(float4*)(grad + base) = make_float4(g[0], g[1], g[2], g[3]);
    else grad[base] = g[0];
  }
  sh = block_sum_256(sh, red);
  sw = block_sum_256(sw, red);
  if (threadIdx.x == 0) { partial[2 * blockIdx.x] = sh; partial[2 * blockIdx.x + 1] = sw; }
}

// out = s0 * sum_j partial[stride * j] (+ s1 * sum_j partial[stride * j + 1] when stride == 2), j < nblk <= LB
__global__ __launch_bounds__(LB) void slots_final_kernel(const float* __restrict__ partial, int nblk, int stride, float* __restrict__ out,
                                                         float s0, float s1) {
  __shared__ float r0[LB / 64], r1[LB / 64];
  const int t = threadIdx.x;
  float a = t < nblk ? partial[stride * t] : 0.f;
  float b = (t < nblk && stride == 2) ? partial[2 * t + 1] : 0.f;
  a = wave_sum(a); b = wave_sum(b);
  if ((t & 63) == 0) { r0[t >> 6] = a; r1[t >> 6] = b; }
  __syncthreads();
  if (t == 0) {
    float sa = 0.f, sb = 0.f;
    for (int i = 0; i < LB / 64; ++i) { sa += r0[i]; sb += r1[i]; }
    out[0] = stride == 2 ? sa * s0 + sb * s1 : sa * s0;
  }
}

// ------------------------------------------------------------------------------------------------------------------ squared difference
// unit u covers elements [4u, 4u + 4): one 16-byte access per tensor when `vec` and the unit is whole, else element by element (the tail)
__global__ __launch_bounds__(256) void sqdiff_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ g,
                                                     float* __restrict__ partial, int64_t count, int vec, float gc) {
  __shared__ float red[4];
  const int64_t units = (count + 3) >> 2;
  float acc = 0.f;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
    const int64_t base = u * 4;
    if (vec && base + 4 <= count) {
      const float4 av = *(const float4*)(a + base), bv = *(const float4*)(b + base);
      const float d0 = av.x - bv.x, d1 = av.y - bv.y, d2 = av.z - bv.z, d3 = av.w - bv.w;
      acc += d0 * d0; acc += d1 * d1; acc += d2 * d2; acc += d3 * d3;
      *(float4*)(g + base) = make_float4(gc * d0, gc * d1, gc * d2, gc * d3);
    } else {
      for (int64_t i = base; i < count && i < base + 4; ++i) {
        const float d = a[i] - b[i];
        acc += d * d;
        g[i] = gc * d;
      }
    }
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

}  // namespace

#define ST ((hipStream_t)s)

// partial: N floats of workspace
extern "C" int pmi_head_loss(const float* emb, const float* W, const float* b, float* loss, float* demb, float* out, float* partial, int N,
                             int K, int D, int mode, float target, int n_total, float mult, float gscale, pmi_stream_t s) {
  if (!emb || !W || !b || !loss || !demb || !out || !partial || N <= 0 || K <= 0 || K > HEAD_KMAX || D <= 0 || D > HEAD_DMAX ||
      n_total < N || mode < 0 || mode > 3 || !(target == target))
    return PMI_ERR_ARG;
  if (mode == 0 && K != 1) return PMI_ERR_ARG;
  int tidx = -1;
  if (mode == 1 || mode == 3) {                 // the target selects a class: an integer in 1 .. K
    if (!(target >= 1.f && target <= (float)K) || target != (float)(int)target) return PMI_ERR_ARG;
    tidx = (int)target - 1;
  }
  const float sq = mode == 0 ? (float)sqrt((double)D) : 1.f;
  const float c = (float)((double)mult * (double)gscale / (double)n_total);
  hipLaunchKernelGGL(head_loss_kernel, dim3(N), dim3(256), 0, ST, emb, W, b, demb, out, partial, K, D, mode, target, tidx, sq, c);
  PMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(head_final_kernel, dim3(1), dim3(256), 0, ST, partial, N, loss, (float)((double)mult / (double)n_total));
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

// partial: 2048 floats of workspace
extern "C" int pmi_smoothness(const float* x, float* loss, float* grad, float* partial, int N, int C, int H, int W, int n_total, float gscale,
                              pmi_stream_t s) {
  if (!x || !loss || !grad || !partial || N <= 0 || C <= 0 || H < 2 || W < 2 || n_total < N) return PMI_ERR_ARG;
  const int64_t total = (int64_t)N * C * H * W;
  if (total >= ((int64_t)1 << 40)) return PMI_ERR_ARG;
  const double inv_h = 1.0 / ((double)n_total * C * (double)(H - 1) * W), inv_w = 1.0 / ((double)n_total * C * (double)H * (W - 1));
  const float gh = (float)(2.0 * gscale * inv_h), gw = (float)(2.0 * gscale * inv_w);
  const bool vec = W % 4 == 0 && aligned16(x) && aligned16(grad);
  const int64_t units = vec ? total / 4 : total;
  const unsigned nblk = grid_256(units, LB);
  if (vec) hipLaunchKernelGGL(smoothness_kernel<4>, dim3(nblk), dim3(256), 0, ST, x, grad, partial, units, H, W, gh, gw);
  else hipLaunchKernelGGL(smoothness_kernel<1>, dim3(nblk), dim3(256), 0, ST, x, grad, partial, units, H, W, gh, gw);
  PMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(slots_final_kernel, dim3(1), dim3(LB), 0, ST, partial, (int)nblk, 2, loss, (float)inv_h, (float)inv_w);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

// partial: 1024 floats of workspace
extern "C" int pmi_sqdiff_loss(const float* a, const float* b, float* loss, float* g, float* partial, int64_t count, int64_t n_total_count,
                               pmi_stream_t s) {
  if (!a || !b || !loss || !g || !partial || count <= 0 || count >= ((int64_t)1 << 40) || n_total_count < count) return PMI_ERR_ARG;
  const double inv = 1.0 / (double)n_total_count;
  const int vec = aligned16(a) && aligned16(b) && aligned16(g);
  const unsigned nblk = grid_256((count + 3) >> 2, LB);
  hipLaunchKernelGGL(sqdiff_kernel, dim3(nblk), dim3(256), 0, ST, a, b, g, partial, count, vec, (float)(2.0 * inv));
  PMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(slots_final_kernel, dim3(1), dim3(LB), 0, ST, partial, (int)nblk, 1, loss, (float)inv, 0.f);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
