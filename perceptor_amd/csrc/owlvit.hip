// OWL-ViT detection heads on the ViT tower's last hidden state (engine/owlvit.py; reference perceptor/models/owlvit/modeling_owlvit.py).
//
// merge fwd : post_layernorm on all T rows -> patch rows times the class-token row -> layer_norm; image_feats as fp32 and as the 16-bit
//             GEMM operand, mean / rstd of both norms kept.  One launch, one wave per patch row (the class row's LayerNorm is recomputed
//             by every wave: one more W-float read that hits L2, against a second launch and a round trip through HBM).
// merge bwd : the exact adjoint, to all T rows of the hidden state.  The class row's gradient is a sum over the image's P patch rows:
//             phase 1 writes one partial row per workgroup (OWL_ROWS patch rows, summed in a fixed order), phase 2 sums an image's
//             partials in block order and applies the class row's LayerNorm adjoint.  No atomics: two runs are bit-equal.
// class head: logits = (e / (|e| + 1e-6) . q + shift) (elu(scale) + 1) per (row, query) from the packed GEMM output [e | shift | scale],
//             and the map dlogits -> gradient of that GEMM output as the 16-bit operand of the transposed-weight GEMM.  The Q x D query
//             block sits in LDS, staged once per workgroup.
// top-k loss: one workgroup per (image, query): log-softmax over the P tokens, k rounds of arg-max, the loss partial and dlogits.
// box out   : dense2 (W -> 4) + box bias + sigmoid, one wave per row.
//
// Everything is fp32 arithmetic on the vector ALU: per row the heads are O(W) work next to the tower's GEMMs.
#include "common.h"
#include "launch_util.h"
#include "../../include/perceptor_hip.h"

#include <math.h>

namespace {

constexpr int OWL_V4 = 8;        // float4 per lane of a row held in registers: W <= 64 * 4 * 8 = 2048
constexpr int OWL_ROWS = 8;      // patch rows per workgroup of the merge backward (two per wave)
constexpr int OWL_E = 16;        // class-embedding values per lane: D <= 1024
constexpr int OWL_QD_MAX = 12288;   // floats of LDS for the query block (48 KB)
constexpr int OWL_LROWS = 16;    // rows per workgroup of the class-head kernels (four per wave): one LDS fill per 16 rows
constexpr int OWL_K_MAX = 64;
constexpr int OWL_P_MAX = 16256;   // P floats + 304 B of static LDS stay inside 64 KB per workgroup

__device__ __forceinline__ float4 f4(float v) { return make_float4(v, v, v, v); }
__device__ __forceinline__ float hsum(float4 a) { return (a.x + a.y) + (a.z + a.w); }

// lane's columns of a W-float row: c = (i * 64 + lane) * 4, i < OWL_V4; columns at or past W read as zero
__device__ __forceinline__ void row_load(const float* __restrict__ p, int W, int lane, float4* v) {
#pragma unroll
  for (int i = 0; i < OWL_V4; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = c < W ? *(const float4*)(p + c) : f4(0.f);
  }
}

// mean over the row of the lane's values (zeros past W add nothing)
__device__ __forceinline__ float row_mean(const float4* v, int W) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < OWL_V4; ++i) s += hsum(v[i]);
  return wave_sum(s) / W;
}

// two-pass LayerNorm statistics (as pmi_layernorm_fwd)
__device__ __forceinline__ void row_stats(const float4* v, int W, int lane, float eps, float& mean, float& rstd) {
  mean = row_mean(v, W);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < OWL_V4; ++i)
    if ((i * 64 + lane) * 4 < W) { const float4 d = v[i] - f4(mean); s += hsum(d * d); }
  rstd = rsqrtf(wave_sum(s) / W + eps);
}

// v <- (v - mean) rstd gamma + beta on the valid columns, zero past W
__device__ __forceinline__ void row_affine(float4* v, int W, int lane, float mean, float rstd, const float* __restrict__ gamma,
                                           const float* __restrict__ beta) {
#pragma unroll
  for (int i = 0; i < OWL_V4; ++i) {
    const int c = (i * 64 + lane) * 4;
    v[i] = c < W ? (v[i] - f4(mean)) * f4(rstd) * *(const float4*)(gamma + c) + *(const float4*)(beta + c) : f4(0.f);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void owl_merge_ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ g1,
                                                               const float* __restrict__ b1, const float* __restrict__ g2,
                                                               const float* __restrict__ b2, float* __restrict__ f32o, u16* __restrict__ f16o,
                                                               float* __restrict__ mean1, float* __restrict__ rstd1,
                                                               float* __restrict__ mean2, float* __restrict__ rstd2, int N, int Tn, int W, float eps) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, P = Tn - 1;
  const int64_t r = (int64_t)blockIdx.x * 4 + wv;
  if (r >= (int64_t)N * P) return;       // wave-uniform; the kernel has no barrier
  const int64_t n = r / P;
  const int p = (int)(r % P);
  const float* xc = x + n * Tn * W;
  float4 a[OWL_V4], c[OWL_V4];
  float m0, r0, m1, r1, m2, r2;
  row_load(xc, W, lane, a);
  row_stats(a, W, lane, eps, m0, r0);
  row_load(xc + (int64_t)(p + 1) * W, W, lane, c);
  row_stats(c, W, lane, eps, m1, r1);
  if (lane == 0) {
    mean1[n * Tn + p + 1] = m1; rstd1[n * Tn + p + 1] = r1;
    if (p == 0) { mean1[n * Tn] = m0; rstd1[n * Tn] = r0; }
  }
  row_affine(a, W, lane, m0, r0, g1, b1);
  row_affine(c, W, lane, m1, r1, g1, b1);
#pragma unroll
  for (int i = 0; i < OWL_V4; ++i) c[i] = c[i] * a[i];
  row_stats(c, W, lane, eps, m2, r2);
  if (lane == 0) { mean2[r] = m2; rstd2[r] = r2; }
  row_affine(c, W, lane, m2, r2, g2, b2);
#pragma unroll
  for (int i = 0; i < OWL_V4; ++i) {
    const int col = (i * 64 + lane) * 4;
    if (col < W) {
      *(float4*)(f32o + r * W + col) = c[i];
      *(uint2*)(f16o + r * W + col) = pack4<T>(c[i].x, c[i].y, c[i].z, c[i].w);
    }
  }
}

// LayerNorm input gradient of one row held in registers: dy <- rstd (gy - mean(gy) - xh mean(gy xh)), gy = dy gamma; xh = the normalised row
__device__ __forceinline__ void row_ln_vjp(float4* dy, const float4* xh, int W, int lane, float rstd, const float* __restrict__ gamma) {
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < OWL_V4; ++i) {
    const int c = (i * 64 + lane) * 4;
    dy[i] = c < W ? dy[i] * *(const float4*)(gamma + c) : f4(0.f);
    s1 += hsum(dy[i]);
    s2 += hsum(dy[i] * xh[i]);
  }
  s1 = wave_sum(s1) / W; s2 = wave_sum(s2) / W;
#pragma unroll
  for (int i = 0; i < OWL_V4; ++i) {
    const int c = (i * 64 + lane) * 4;
    dy[i] = c < W ? f4(rstd) * (dy[i] - f4(s1) - xh[i] * f4(s2)) : f4(0.f);
  }
}

// phase 1: workgroup (n, blk) owns patch rows blk * OWL_ROWS .. + OWL_ROWS - 1 of image n; wave v takes rows v and v + 4 of them, in that
// order.  dx of the patch rows is final; the class row's share dm * y goes to part[(n * nblk + blk)][W], the four waves added in wave order.
__global__ __launch_bounds__(256) void owl_merge_ln_bwd_kernel(const float* __restrict__ df, const float* __restrict__ x,
                                                               const float* __restrict__ g1, const float* __restrict__ b1,
                                                               const float* __restrict__ g2, const float* __restrict__ mean1,
                                                               const float* __restrict__ rstd1, const float* __restrict__ mean2,
                                                               const float* __restrict__ rstd2, float* __restrict__ dx,
                                                               float* __restrict__ part, int N, int Tn, int W, int nblk) {
  extern __shared__ __attribute__((aligned(16))) float acc_s[];          // [4][W]
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, P = Tn - 1;
  const int64_t n = blockIdx.x / nblk;
  const int blk = blockIdx.x % nblk;
  const float* xc = x + n * Tn * W;
  float4 y0[OWL_V4], acc[OWL_V4];
  row_load(xc, W, lane, y0);
  row_affine(y0, W, lane, mean1[n * Tn], rstd1[n * Tn], g1, b1);
#pragma unroll
  for (int i = 0; i < OWL_V4; ++i) acc[i] = f4(0.f);
  for (int j = wv; j < OWL_ROWS; j += 4) {
    const int p = blk * OWL_ROWS + j;
    if (p >= P) break;                   // wave-uniform; no barrier inside the loop
    const int64_t r = n * P + p, t = n * Tn + p + 1;
    const float m1 = mean1[t], r1 = rstd1[t], m2 = mean2[r], r2 = rstd2[r];
    float4 xh[OWL_V4], d[OWL_V4];
    row_load(xc + (int64_t)(p + 1) * W, W, lane, xh);
    row_load(df + r * W, W, lane, d);
    // xh = normalised row, y = xh gamma + beta, m = y y0, mh = (m - m2) r2; layer_norm's vjp gives dm
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < OWL_V4; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < W) {
        xh[i] = (xh[i] - f4(m1)) * f4(r1);
        const float4 y = xh[i] * *(const float4*)(g1 + c) + *(const float4*)(b1 + c);
        const float4 mh = (y * y0[i] - f4(m2)) * f4(r2);
        d[i] = d[i] * *(const float4*)(g2 + c);
        s1 += hsum(d[i]);
        s2 += hsum(d[i] * mh);
      } else {
        xh[i] = f4(0.f); d[i] = f4(0.f);
      }
    }
    s1 = wave_sum(s1) / W; s2 = wave_sum(s2) / W;
#pragma unroll
    for (int i = 0; i < OWL_V4; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < W) {
        const float4 y = xh[i] * *(const float4*)(g1 + c) + *(const float4*)(b1 + c);
        const float4 mh = (y * y0[i] - f4(m2)) * f4(r2);
        const float4 dm = f4(r2) * (d[i] - f4(s1) - mh * f4(s2));
        acc[i] = acc[i] + dm * y;
        d[i] = dm * y0[i];
      }
    }
    row_ln_vjp(d, xh, W, lane, r1, g1);
#pragma unroll
    for (int i = 0; i < OWL_V4; ++i) {
      const int c = (i * 64 + lane) * 4;
      if (c < W) *(float4*)(dx + t * W + c) = d[i];
    }
  }
#pragma unroll
  for (int i = 0; i < OWL_V4; ++i) {
    const int c = (i * 64 + lane) * 4;
    if (c < W) *(float4*)(acc_s + wv * W + c) = acc[i];
  }
  __syncthreads();
  float* po = part + ((int64_t)n * nblk + blk) * W;
  for (int c = threadIdx.x; c < W; c += 256) po[c] = (acc_s[c] + acc_s[W + c]) + (acc_s[2 * W + c] + acc_s[3 * W + c]);
}

// phase 2: one workgroup per image: the class row's dy = sum of its nblk partial rows in block order, then post_layernorm's adjoint
__global__ __launch_bounds__(256) void owl_merge_cls_bwd_kernel(const float* __restrict__ part, const float* __restrict__ x,
                                                                const float* __restrict__ g1, const float* __restrict__ mean1,
                                                                const float* __restrict__ rstd1, float* __restrict__ dx, int Tn, int W, int nblk) {
  __shared__ float red[4];
  const int64_t n = blockIdx.x;
  const float m0 = mean1[n * Tn], r0 = rstd1[n * Tn];
  float gy[OWL_V4], xh[OWL_V4];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int i = 0; i < OWL_V4; ++i) {
    const int c = threadIdx.x + 256 * i;
    gy[i] = 0.f; xh[i] = 0.f;
    if (c < W) {
      float s = 0.f;
      for (int b = 0; b < nblk; ++b) s += part[(n * nblk + b) * W + c];
      gy[i] = s * g1[c];
      xh[i] = (x[n * Tn * W + c] - m0) * r0;
      s1 += gy[i];
      s2 += gy[i] * xh[i];
    }
  }
  s1 = block_sum_256(s1, red) / W;
  s2 = block_sum_256(s2, red) / W;
#pragma unroll
  for (int i = 0; i < OWL_V4; ++i) {
    const int c = threadIdx.x + 256 * i;
    if (c < W) dx[n * Tn * W + c] = r0 * (gy[i] - s1 - xh[i] * s2);
  }
}

// elu(s) + 1 = exp(s) for s <= 0: written so, the small values keep their relative accuracy (expm1(s) + 1 cancels to an absolute 2^-24)
__device__ __forceinline__ float elu1(float s) { return s > 0.f ? s + 1.f : expf(s); }
__device__ __forceinline__ float elu1_grad(float s) { return s > 0.f ? 1.f : expf(s); }

__global__ __launch_bounds__(256) void owl_class_logits_fwd_kernel(const float* __restrict__ g, int ldg, const float* __restrict__ q,
                                                                   float* __restrict__ logits, float* __restrict__ ce, int64_t M, int D, int Q) {
  extern __shared__ __attribute__((aligned(16))) float qs[];             // [Q][D]
  for (int i = threadIdx.x; i < Q * D; i += 256) qs[i] = q[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = wv; j < OWL_LROWS; j += 4) {
    const int64_t r = (int64_t)blockIdx.x * OWL_LROWS + j;
    if (r >= M) break;                   // wave-uniform; no barrier inside the loop
    const float* row = g + r * ldg;
    float e[OWL_E];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < OWL_E; ++i) {
      const int c = lane + 64 * i;
      e[i] = c < D ? row[c] : 0.f;
      ss += e[i] * e[i];
    }
    const float inv = 1.f / (sqrtf(wave_sum(ss)) + 1e-6f);
#pragma unroll
    for (int i = 0; i < OWL_E; ++i) {
      const int c = lane + 64 * i;
      e[i] *= inv;
      if (c < D) ce[r * D + c] = e[i];
    }
    const float sh = row[D], sc = elu1(row[D + 1]);
    for (int k = 0; k < Q; ++k) {
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < OWL_E; ++i) {
        const int c = lane + 64 * i;
        if (c < D) dot = fmaf(e[i], qs[k * D + c], dot);
      }
      dot = wave_sum(dot);
      if (lane == 0) logits[r * Q + k] = (dot + sh) * sc;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void owl_class_logits_bwd_kernel(const float* __restrict__ dl, const float* __restrict__ g, int ldg,
                                                                   const float* __restrict__ q, u16* __restrict__ dg, int64_t M, int D, int Q) {
  extern __shared__ __attribute__((aligned(16))) float qs[];
  for (int i = threadIdx.x; i < Q * D; i += 256) qs[i] = q[i];
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int j = wv; j < OWL_LROWS; j += 4) {
    const int64_t r = (int64_t)blockIdx.x * OWL_LROWS + j;
    if (r >= M) break;
    const float* row = g + r * ldg;
    float e[OWL_E], de[OWL_E];
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < OWL_E; ++i) {
      const int c = lane + 64 * i;
      e[i] = c < D ? row[c] : 0.f;
      de[i] = 0.f;
      ss += e[i] * e[i];
    }
    const float nrm = sqrtf(wave_sum(ss)), inv = 1.f / (nrm + 1e-6f);
    const float sh = row[D], s = row[D + 1], sc = elu1(s);
    float dsh = 0.f, dsc = 0.f;
    for (int k = 0; k < Q; ++k) {
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < OWL_E; ++i) {
        const int c = lane + 64 * i;
        if (c < D) dot = fmaf(e[i], qs[k * D + c], dot);
      }
      dot = wave_sum(dot) * inv;
      const float d = dl[r * Q + k];
      dsh += d * sc;
      dsc += d * (dot + sh);
#pragma unroll
      for (int i = 0; i < OWL_E; ++i) {
        const int c = lane + 64 * i;
        if (c < D) de[i] = fmaf(d * sc, qs[k * D + c], de[i]);
      }
    }
    // e_hat = e inv, inv = 1 / (|e| + 1e-6):  d e = de inv - e (de . e) inv^2 / |e|
    float t = 0.f;
#pragma unroll
    for (int i = 0; i < OWL_E; ++i) t = fmaf(de[i], e[i], t);
    t = wave_sum(t);
    const float back = nrm > 0.f ? t * inv * inv / nrm : 0.f;
    u16* out = dg + r * ldg;
#pragma unroll
    for (int i = 0; i < OWL_E; ++i) {
      const int c = lane + 64 * i;
      if (c < D) out[c] = T::from_f(de[i] * inv - e[i] * back);
    }
    for (int c = D + lane; c < ldg; c += 64)     // shift, scale, then the GEMM's zero padding
      out[c] = T::from_f(c == D ? dsh : (c == D + 1 ? dsc * elu1_grad(s) : 0.f));
  }
}

// (value, index) arg-max over the workgroup; ties go to the lower index.  rv / ri = 4 slots of LDS each.
__device__ __forceinline__ void block_argmax(float& v, int& i, float* rv, int* ri) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (ov > v || (ov == v && oi < i)) { v = ov; i = oi; }
  }
  __syncthreads();
  if ((threadIdx.x & 63) == 0) { rv[threadIdx.x >> 6] = v; ri[threadIdx.x >> 6] = i; }
  __syncthreads();
  v = rv[0]; i = ri[0];
#pragma unroll
  for (int w = 1; w < 4; ++w)
    if (rv[w] > v || (rv[w] == v && ri[w] < i)) { v = rv[w]; i = ri[w]; }
}

__global__ __launch_bounds__(256) void owl_topk_loss_kernel(const float* __restrict__ logits, const float* __restrict__ w,
                                                            float* __restrict__ dlogits, float* __restrict__ partial, int N, int P, int Q, int k,
                                                            float mul) {
  extern __shared__ __attribute__((aligned(16))) float ls[];             // [P]: the column, selected entries replaced by -inf
  __shared__ float red[4], rv[4];
  __shared__ int ri[4], sel[OWL_K_MAX];
  const int n = blockIdx.x / Q, qi = blockIdx.x % Q, tid = threadIdx.x;
  const float* col = logits + (int64_t)n * P * Q + qi;
  float mx = -INFINITY;
  for (int p = tid; p < P; p += 256) {
    const float v = col[(int64_t)p * Q];
    ls[p] = v;
    mx = fmaxf(mx, v);
  }
  mx = wave_max(mx);
  if ((tid & 63) == 0) rv[tid >> 6] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(rv[0], rv[1]), fmaxf(rv[2], rv[3]));
  float se = 0.f;
  for (int p = tid; p < P; p += 256) se += expf(ls[p] - mx);
  const float lse = mx + logf(block_sum_256(se, red));
  const int ke = k < P ? k : P;
  float picked = 0.f;                    // thread 0: sum over the selected set of the log-softmax, in selection order
  for (int j = 0; j < ke; ++j) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int p = tid; p < P; p += 256) {
      const float v = ls[p];
      if (v > bv || (v == bv && p < bi)) { bv = v; bi = p; }
    }
    block_argmax(bv, bi, rv, ri);        // (its leading barrier orders the scan after the previous round's update of ls)
    if (tid == 0) {
      sel[j] = bi < P ? bi : -1;         // a column of NaN selects nothing
      if (bi < P) { picked += bv - lse; ls[bi] = -INFINITY; }
    }
    __syncthreads();
  }
  const float coef = -0.01f * w[qi] / ((float)N * (float)ke);
  if (tid == 0) partial[blockIdx.x] = coef * picked;
  for (int p = tid; p < P; p += 256) {
    const float sm = expf(col[(int64_t)p * Q] - lse);
    float ind = 0.f;
    for (int j = 0; j < ke; ++j) ind = sel[j] == p ? 1.f : ind;
    dlogits[((int64_t)n * P + p) * Q + qi] = coef * mul * (ind - (float)ke * sm);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void owl_box_out_kernel(const u16* __restrict__ h, int ldh, const float* __restrict__ w2,
                                                          const float* __restrict__ b2, const float* __restrict__ bias, float* __restrict__ boxes,
                                                          int64_t M, int P, int W) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wv;
  if (r >= M) return;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int c = lane * 8; c < W; c += 512) {
    float v[8];
    unpack8<T>(*(const uint4*)(h + r * ldh + c), v);
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const float4 wa = *(const float4*)(w2 + (int64_t)o * W + c), wb = *(const float4*)(w2 + (int64_t)o * W + c + 4);
      acc[o] += (v[0] * wa.x + v[1] * wa.y + v[2] * wa.z + v[3] * wa.w) + (v[4] * wb.x + v[5] * wb.y + v[6] * wb.z + v[7] * wb.w);
    }
  }
#pragma unroll
  for (int o = 0; o < 4; ++o) acc[o] = wave_sum(acc[o]);
  if (lane == 0) {
    const float4 bb = *(const float4*)(bias + (r % P) * 4);
    const float z[4] = {acc[0] + b2[0] + bb.x, acc[1] + b2[1] + bb.y, acc[2] + b2[2] + bb.z, acc[3] + b2[3] + bb.w};
    *(float4*)(boxes + r * 4) = make_float4(1.f / (1.f + expf(-z[0])), 1.f / (1.f + expf(-z[1])), 1.f / (1.f + expf(-z[2])), 1.f / (1.f + expf(-z[3])));
  }
}

bool merge_shape_ok(int N, int T, int W) { return N > 0 && T > 1 && W > 0 && W % 4 == 0 && W <= 64 * 4 * OWL_V4; }
bool class_shape_ok(int64_t M, int D, int Q, int ldg) {
  return M > 0 && D > 0 && D <= 64 * OWL_E && Q > 0 && (int64_t)Q * D <= OWL_QD_MAX && ldg >= D + 2 && (M + OWL_LROWS - 1) / OWL_LROWS <= 0x7fffffffll;
}

}  // namespace

#define ST ((hipStream_t)s)

extern "C" int pmi_owl_merge_ln_fwd(const float* x, const float* g1, const float* b1, const float* g2, const float* b2, float* feats32,
                                    void* feats16, float* mean_rstd1, float* mean_rstd2, int N, int T, int W, float eps, int dtype,
                                    pmi_stream_t s) {
  if (!x || !g1 || !b1 || !g2 || !b2 || !feats32 || !feats16 || !mean_rstd1 || !mean_rstd2) return PMI_ERR_ARG;
  if (!merge_shape_ok(N, T, W) || !(eps > 0.f) || (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16)) return PMI_ERR_ARG;
  if (!aligned16(x) || !aligned16(g1) || !aligned16(b1) || !aligned16(g2) || !aligned16(b2) || !aligned16(feats32) || !aligned16(feats16)) return PMI_ERR_ARG;
  const int64_t M1 = (int64_t)N * T, M2 = (int64_t)N * (T - 1);
  if ((M2 + 3) / 4 > 0x7fffffffll) return PMI_ERR_ARG;
  const dim3 grid((unsigned)((M2 + 3) / 4)), block(256);
  if (dtype == PMI_DT_BF16)
    hipLaunchKernelGGL(owl_merge_ln_fwd_kernel<BF16>, grid, block, 0, ST, x, g1, b1, g2, b2, feats32, (u16*)feats16, mean_rstd1, mean_rstd1 + M1,
                       mean_rstd2, mean_rstd2 + M2, N, T, W, eps);
  else
    hipLaunchKernelGGL(owl_merge_ln_fwd_kernel<F16>, grid, block, 0, ST, x, g1, b1, g2, b2, feats32, (u16*)feats16, mean_rstd1, mean_rstd1 + M1,
                       mean_rstd2, mean_rstd2 + M2, N, T, W, eps);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_owl_merge_bwd_blocks(int T) { return T > 1 ? (T - 1 + OWL_ROWS - 1) / OWL_ROWS : 0; }

extern "C" int pmi_owl_merge_ln_bwd(const float* dfeats, const float* x, const float* g1, const float* b1, const float* g2,
                                    const float* mean_rstd1, const float* mean_rstd2, float* dx, float* partials, int N, int T, int W,
                                    pmi_stream_t s) {
  if (!dfeats || !x || !g1 || !b1 || !g2 || !mean_rstd1 || !mean_rstd2 || !dx || !partials) return PMI_ERR_ARG;
  if (!merge_shape_ok(N, T, W)) return PMI_ERR_ARG;
  if (!aligned16(dfeats) || !aligned16(x) || !aligned16(g1) || !aligned16(b1) || !aligned16(g2) || !aligned16(dx)) return PMI_ERR_ARG;
  const int nblk = pmi_owl_merge_bwd_blocks(T);
  const int64_t M1 = (int64_t)N * T, M2 = (int64_t)N * (T - 1);
  if ((int64_t)N * nblk > 0x7fffffffll) return PMI_ERR_ARG;
  hipLaunchKernelGGL(owl_merge_ln_bwd_kernel, dim3((unsigned)(N * nblk)), dim3(256), (size_t)4 * W * sizeof(float), ST, dfeats, x, g1, b1, g2,
                     mean_rstd1, mean_rstd1 + M1, mean_rstd2, mean_rstd2 + M2, dx, partials, N, T, W, nblk);
  PMI_CHECK_LAUNCH();
  hipLaunchKernelGGL(owl_merge_cls_bwd_kernel, dim3((unsigned)N), dim3(256), 0, ST, partials, x, g1, mean_rstd1, mean_rstd1 + M1, dx, T, W, nblk);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_owl_class_logits_fwd(const float* g, int ldg, const float* q, float* logits, float* class_embeds, int64_t M, int D, int Q,
                                        pmi_stream_t s) {
  if (!g || !q || !logits || !class_embeds || !class_shape_ok(M, D, Q, ldg)) return PMI_ERR_ARG;
  hipLaunchKernelGGL(owl_class_logits_fwd_kernel, dim3((unsigned)((M + OWL_LROWS - 1) / OWL_LROWS)), dim3(256), (size_t)Q * D * sizeof(float), ST,
                     g, ldg, q, logits, class_embeds, M, D, Q);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_owl_class_logits_bwd(const float* dlogits, const float* g, int ldg, const float* q, void* dg, int64_t M, int D, int Q,
                                        int dtype, pmi_stream_t s) {
  if (!dlogits || !g || !q || !dg || !class_shape_ok(M, D, Q, ldg) || (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16)) return PMI_ERR_ARG;
  const dim3 grid((unsigned)((M + OWL_LROWS - 1) / OWL_LROWS)), block(256);
  const size_t lds = (size_t)Q * D * sizeof(float);
  if (dtype == PMI_DT_BF16)
    hipLaunchKernelGGL(owl_class_logits_bwd_kernel<BF16>, grid, block, lds, ST, dlogits, g, ldg, q, (u16*)dg, M, D, Q);
  else
    hipLaunchKernelGGL(owl_class_logits_bwd_kernel<F16>, grid, block, lds, ST, dlogits, g, ldg, q, (u16*)dg, M, D, Q);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_owl_topk_loss(const float* logits, const float* weights, float* dlogits, float* partials, int N, int P, int Q, int k,
                                 float mul, pmi_stream_t s) {
  if (!logits || !weights || !dlogits || !partials) return PMI_ERR_ARG;
  if (N <= 0 || P <= 0 || P > OWL_P_MAX || Q <= 0 || k <= 0 || k > OWL_K_MAX || !finite_f(mul) || (int64_t)N * Q > 0x7fffffffll) return PMI_ERR_ARG;
  hipLaunchKernelGGL(owl_topk_loss_kernel, dim3((unsigned)(N * Q)), dim3(256), (size_t)P * sizeof(float), ST, logits, weights, dlogits, partials,
                     N, P, Q, k, mul);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_owl_box_out(const void* h, int ldh, const float* w2, const float* b2, const float* box_bias, float* boxes, int64_t M, int P,
                               int W, int dtype, pmi_stream_t s) {
  if (!h || !w2 || !b2 || !box_bias || !boxes) return PMI_ERR_ARG;
  if (M <= 0 || P <= 0 || W <= 0 || W % 8 || ldh < W || ldh % 8 || (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16)) return PMI_ERR_ARG;
  if (!aligned16(h) || !aligned16(w2) || !aligned16(box_bias) || !aligned16(boxes) || (M + 3) / 4 > 0x7fffffffll) return PMI_ERR_ARG;
  const dim3 grid((unsigned)((M + 3) / 4)), block(256);
  if (dtype == PMI_DT_BF16)
    hipLaunchKernelGGL(owl_box_out_kernel<BF16>, grid, block, 0, ST, (const u16*)h, ldh, w2, b2, box_bias, boxes, M, P, W);
  else
    hipLaunchKernelGGL(owl_box_out_kernel<F16>, grid, block, 0, ST, (const u16*)h, ldh, w2, b2, box_bias, boxes, M, P, W);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
