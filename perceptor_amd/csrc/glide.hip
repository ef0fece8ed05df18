// GLIDE CLIP image tower: the patch stem in one launch per direction (engine/glide.py; reference perceptor/models/glide_clip/encoders.py).
//
// forward : Normalize on the 0..255 scale -> 4x4 stride-4 patch convolution (K = 48) -> + positions, token 0 = row ts[n] of the timestep
//           table -> LayerNorm.  Writes x0 (pre-LayerNorm, kept for the backward), x (the residual stream) and mean / rstd.
// backward: LayerNorm input gradient -> W^T -> un-patchify with the Normalize adjoint, to the image.  Token 0's row is dropped.
//
// All arithmetic is fp32 on the vector ALU: at K = 48 the tower's stem is 19 MFLOP per sample and an MFMA tile would be mostly padding.
// A workgroup owns GL_TOK consecutive token rows and streams the [W][48] weight panel from L2 (147 KB at W = 768: LDS-resident it would
// allow no second workgroup on the CU and cost one LDS fill per 8 rows of work; read straight from L2 each panel byte is loaded once per
// workgroup and the CU keeps several workgroups in flight).  LayerNorm needs a whole W row, so the row tile is never split across workgroups.
#include "common.h"
#include "launch_util.h"
#include "../../include/perceptor_hip.h"

namespace {

constexpr int GL_P = 4;                  // patch edge
constexpr int GL_K = 3 * GL_P * GL_P;    // 48
constexpr int GL_TOK = 8;                // token rows per workgroup
constexpr int GL_MAXC = 8;               // channels per thread: W <= 256 * 8

// sum over the 256-thread workgroup of GL_TOK values per thread; red = 4 * GL_TOK floats of LDS
__device__ __forceinline__ void block_sum_tok(float* v, float* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int t = 0; t < GL_TOK; ++t) v[t] = wave_sum(v[t]);
  __syncthreads();
  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < GL_TOK; ++t) red[wv * GL_TOK + t] = v[t];
  }
  __syncthreads();
#pragma unroll
  for (int t = 0; t < GL_TOK; ++t) v[t] = (red[t] + red[GL_TOK + t]) + (red[2 * GL_TOK + t] + red[3 * GL_TOK + t]);
}

// Thread tid owns channels j = tid + 256 c.  Its weight row w[j][0..47] is 12 float4 loads of one contiguous 192 B run (a wave's 64 rows
// are one 12 KB run: every byte fetched is used, from L1 after the first touch) and stays in registers over the tile's 8 rows; the rows'
// 48 normalised pixels sit in LDS and are read as wave-uniform (broadcast) b128.  Channels go three at a time, so one broadcast read
// feeds 12 FMAs and the loop is bound by the vector ALU, not by LDS.
__global__ __launch_bounds__(256) void glide_embed_fwd_kernel(const float* __restrict__ img, const float* __restrict__ mean,
                                                              const float* __restrict__ stdv, const float* __restrict__ w,
                                                              const int64_t* __restrict__ ts, const float* __restrict__ w_t,
                                                              const float* __restrict__ pos, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, float* __restrict__ x0,
                                                              float* __restrict__ x, float* __restrict__ mean_o, float* __restrict__ rstd_o,
                                                              int N, int R, int W, int n_timestep, float eps) {
  __shared__ __attribute__((aligned(16))) float a_s[GL_TOK][GL_K];
  __shared__ float red[4 * GL_TOK];
  __shared__ int64_t trow[GL_TOK];       // row of w_t for a token-0 row, -1 for a patch row
  const int G = R / GL_P, T = G * G + 1;
  const int64_t M = (int64_t)N * T, r0 = (int64_t)blockIdx.x * GL_TOK;
  const int tid = threadIdx.x;
  // ---- stage the tile's normalised patches: one thread per (row, channel, patch line), a 16-byte load each
  if (tid < GL_TOK * 3 * GL_P) {
    const int tok = tid / (3 * GL_P), c = (tid / GL_P) % 3, py = tid % GL_P;
    const int64_t r = r0 + tok;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < M) {
      const int n = (int)(r / T), t = (int)(r % T);
      if (t > 0) {
        const int gy = (t - 1) / G, gx = (t - 1) % G;
        const float4 p = *(const float4*)(img + (((int64_t)n * 3 + c) * R + gy * GL_P + py) * R + gx * GL_P);
        const float m = mean[c], s = stdv[c];
        v = make_float4((255.f * p.x - m) / s, (255.f * p.y - m) / s, (255.f * p.z - m) / s, (255.f * p.w - m) / s);
      }
    }
    *(float4*)&a_s[tok][c * GL_P * GL_P + py * GL_P] = v;
  }
  if (tid < GL_TOK) {
    const int64_t r = r0 + tid;
    int64_t row = -1;
    if (r < M && r % T == 0) {
      row = ts[r / T];
      row = row < 0 ? 0 : (row >= n_timestep ? n_timestep - 1 : row);      // never read outside the table
    }
    trow[tid] = row;
  }
  __syncthreads();
  // ---- patch projection
  float acc[GL_MAXC][GL_TOK];
#pragma unroll
  for (int c = 0; c < GL_MAXC; ++c)
#pragma unroll
    for (int t = 0; t < GL_TOK; ++t) acc[c][t] = 0.f;
#pragma unroll
  for (int c0 = 0; c0 < GL_MAXC; c0 += 3) {
    if (c0 * 256 < W) {                  // workgroup-uniform
      float4 wr[3][GL_K / 4];
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int q = 0; q < GL_K / 4; ++q) {
          const int j = tid + 256 * (c0 + i);
          wr[i][q] = (c0 + i < GL_MAXC && j < W) ? *(const float4*)(w + (int64_t)j * GL_K + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
      for (int t = 0; t < GL_TOK; ++t)
#pragma unroll
        for (int q = 0; q < GL_K / 4; ++q) {
          const float4 a = *(const float4*)&a_s[t][4 * q];
#pragma unroll
          for (int i = 0; i < 3; ++i)
            if (c0 + i < GL_MAXC) {
              float s = acc[c0 + i][t];
              s = fmaf(a.x, wr[i][q].x, s); s = fmaf(a.y, wr[i][q].y, s); s = fmaf(a.z, wr[i][q].z, s); s = fmaf(a.w, wr[i][q].w, s);
              acc[c0 + i][t] = s;
            }
        }
    }
  }
  // ---- x0 = projection (or the timestep row) + position; LayerNorm over the row (two-pass, as pmi_layernorm_fwd)
  float s1[GL_TOK], s2[GL_TOK];
#pragma unroll
  for (int t = 0; t < GL_TOK; ++t) {
    s1[t] = 0.f;
    const int64_t r = r0 + t;
    if (r >= M) continue;                // workgroup-uniform
    const int tt = (int)(r % T);
    const int64_t tr = trow[t];
#pragma unroll
    for (int c = 0; c < GL_MAXC; ++c) {
      const int j = tid + 256 * c;
      if (j < W) {
        const float v = (tr >= 0 ? w_t[tr * W + j] : acc[c][t]) + pos[(int64_t)tt * W + j];
        acc[c][t] = v;
        x0[r * W + j] = v;
        s1[t] += v;
      }
    }
  }
  block_sum_tok(s1, red);
#pragma unroll
  for (int t = 0; t < GL_TOK; ++t) {
    s1[t] /= W;
    s2[t] = 0.f;
#pragma unroll
    for (int c = 0; c < GL_MAXC; ++c)
      if (tid + 256 * c < W) { const float d = acc[c][t] - s1[t]; s2[t] += d * d; }
  }
  block_sum_tok(s2, red);
#pragma unroll
  for (int t = 0; t < GL_TOK; ++t) {
    const int64_t r = r0 + t;
    if (r >= M) continue;
    const float rstd = rsqrtf(s2[t] / W + eps);
    if (tid == 0) { mean_o[r] = s1[t]; rstd_o[r] = rstd; }
#pragma unroll
    for (int c = 0; c < GL_MAXC; ++c) {
      const int j = tid + 256 * c;
      if (j < W) x[r * W + j] = (acc[c][t] - s1[t]) * rstd * gamma[j] + beta[j];
    }
  }
}

// A workgroup owns GL_TOK consecutive patch rows.  Phase 1: one wave per row, the LayerNorm input gradient (pmi_layernorm_bwd's
// arithmetic) into LDS.  Phase 2: lane k < 48 of wave v sums W[j][k] * dx[j] over the v-th quarter of j for all 8 rows -- the weight
// loads are 192 B contiguous per j and each feeds 8 FMAs, dx comes as broadcast b128.  Phase 3: the four partial sums meet in LDS and
// one thread per (row, channel, patch line) stores 16 bytes of the image gradient: every pixel belongs to exactly one patch.
__global__ __launch_bounds__(256) void glide_embed_bwd_kernel(const float* __restrict__ g, const float* __restrict__ x0,
                                                              const float* __restrict__ gamma, const float* __restrict__ mean_i,
                                                              const float* __restrict__ rstd_i, const float* __restrict__ w,
                                                              const float* __restrict__ stdv, float* __restrict__ dimg,
                                                              int N, int R, int W, float mul) {
  extern __shared__ __attribute__((aligned(16))) float dx_s[];          // [GL_TOK][W], then [4][GL_TOK][GL_K]
  const int G = R / GL_P, T = G * G + 1;
  const int64_t Q = (int64_t)N * G * G, q0 = (int64_t)blockIdx.x * GL_TOK;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  for (int tok = wv; tok < GL_TOK; tok += 4) {
    const int64_t q = q0 + tok;
    float* dxr = dx_s + tok * W;
    if (q >= Q) {                        // wave-uniform
      for (int c = lane * 4; c < W; c += 256) *(float4*)(dxr + c) = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    const int64_t r = (q / (G * G)) * T + 1 + q % (G * G);
    const float* gr = g + r * W;
    const float* xr = x0 + r * W;
    const float mean = mean_i[r], rstd = rstd_i[r];
    float s1 = 0.f, s2 = 0.f;
    for (int c = lane * 4; c < W; c += 256) {
      const float4 d = *(const float4*)(gr + c), gm = *(const float4*)(gamma + c), xv = *(const float4*)(xr + c);
      const float4 gy = make_float4(d.x * gm.x, d.y * gm.y, d.z * gm.z, d.w * gm.w);
      const float4 xh = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd, (xv.w - mean) * rstd);
      s1 += gy.x + gy.y + gy.z + gy.w;
      s2 += gy.x * xh.x + gy.y * xh.y + gy.z * xh.z + gy.w * xh.w;
    }
    s1 = wave_sum(s1) / W; s2 = wave_sum(s2) / W;
    for (int c = lane * 4; c < W; c += 256) {
      const float4 d = *(const float4*)(gr + c), gm = *(const float4*)(gamma + c), xv = *(const float4*)(xr + c);
      const float4 gy = make_float4(d.x * gm.x, d.y * gm.y, d.z * gm.z, d.w * gm.w);
      const float4 xh = make_float4((xv.x - mean) * rstd, (xv.y - mean) * rstd, (xv.z - mean) * rstd, (xv.w - mean) * rstd);
      *(float4*)(dxr + c) = make_float4(rstd * (gy.x - s1 - xh.x * s2), rstd * (gy.y - s1 - xh.y * s2),
                                        rstd * (gy.z - s1 - xh.z * s2), rstd * (gy.w - s1 - xh.w * s2));
    }
  }
  __syncthreads();
  float acc[GL_TOK];
#pragma unroll
  for (int t = 0; t < GL_TOK; ++t) acc[t] = 0.f;
  if (lane < GL_K) {
    const int jq = W / 4;                // W % 64 == 0: a multiple of 16
    for (int j = wv * jq; j < (wv + 1) * jq; j += 4) {
      const float w0 = w[(int64_t)j * GL_K + lane], w1 = w[(int64_t)(j + 1) * GL_K + lane];
      const float w2 = w[(int64_t)(j + 2) * GL_K + lane], w3 = w[(int64_t)(j + 3) * GL_K + lane];
#pragma unroll
      for (int t = 0; t < GL_TOK; ++t) {
        const float4 d = *(const float4*)(dx_s + t * W + j);
        float s = acc[t];
        s = fmaf(w0, d.x, s); s = fmaf(w1, d.y, s); s = fmaf(w2, d.z, s); s = fmaf(w3, d.w, s);
        acc[t] = s;
      }
    }
  }
  __syncthreads();                       // dx is dead: its LDS now holds the four partial sums
  if (lane < GL_K) {
#pragma unroll
    for (int t = 0; t < GL_TOK; ++t) dx_s[(wv * GL_TOK + t) * GL_K + lane] = acc[t];
  }
  __syncthreads();
  if (tid < GL_TOK * 3 * GL_P) {
    const int tok = tid / (3 * GL_P), c = (tid / GL_P) % 3, py = tid % GL_P;
    const int64_t q = q0 + tok;
    if (q < Q) {
      const int k = c * GL_P * GL_P + py * GL_P;
      float4 v = *(const float4*)(dx_s + tok * GL_K + k);
#pragma unroll
      for (int p = 1; p < 4; ++p) {
        const float4 u = *(const float4*)(dx_s + (p * GL_TOK + tok) * GL_K + k);
        v.x += u.x; v.y += u.y; v.z += u.z; v.w += u.w;
      }
      const float sc = mul * 255.f / stdv[c];
      const int n = (int)(q / (G * G)), pp = (int)(q % (G * G)), gy = pp / G, gx = pp % G;
      *(float4*)(dimg + (((int64_t)n * 3 + c) * R + gy * GL_P + py) * R + gx * GL_P) = make_float4(v.x * sc, v.y * sc, v.z * sc, v.w * sc);
    }
  }
}

bool glide_shape_ok(int N, int R, int P, int W) {
  return N > 0 && R > 0 && P == GL_P && R % P == 0 && W > 0 && W % 64 == 0 && W <= 256 * GL_MAXC;
}

}  // namespace

#define ST ((hipStream_t)s)

extern "C" int pmi_glide_embed_fwd(const float* img, const float* mean, const float* stdv, const float* w, const int64_t* ts, const float* w_t,
                                   const float* pos, const float* gamma, const float* beta, float* x0, float* x, float* mean_rstd,
                                   int N, int R, int P, int W, int n_timestep, float eps, pmi_stream_t s) {
  if (!img || !mean || !stdv || !w || !ts || !w_t || !pos || !gamma || !beta || !x0 || !x || !mean_rstd) return PMI_ERR_ARG;
  if (!glide_shape_ok(N, R, P, W) || n_timestep <= 0 || !aligned16(img) || !aligned16(w)) return PMI_ERR_ARG;
  const int64_t M = (int64_t)N * ((R / P) * (R / P) + 1);
  if ((M + GL_TOK - 1) / GL_TOK > 0x7fffffffll) return PMI_ERR_ARG;
  hipLaunchKernelGGL(glide_embed_fwd_kernel, dim3((unsigned)((M + GL_TOK - 1) / GL_TOK)), dim3(256), 0, ST, img, mean, stdv, w, ts, w_t, pos,
                     gamma, beta, x0, x, mean_rstd, mean_rstd + M, N, R, W, n_timestep, eps);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_glide_embed_bwd(const float* g, const float* x0, const float* gamma, const float* mean_rstd, const float* w,
                                   const float* stdv, float* dimg, int N, int R, int P, int W, float mul, pmi_stream_t s) {
  if (!g || !x0 || !gamma || !mean_rstd || !w || !stdv || !dimg) return PMI_ERR_ARG;
  if (!glide_shape_ok(N, R, P, W) || !finite_f(mul) || !aligned16(g) || !aligned16(x0) || !aligned16(gamma) || !aligned16(dimg)) return PMI_ERR_ARG;
  const int G = R / P;
  const int64_t M = (int64_t)N * (G * G + 1), Q = (int64_t)N * G * G;
  if ((Q + GL_TOK - 1) / GL_TOK > 0x7fffffffll) return PMI_ERR_ARG;
  const size_t a = (size_t)GL_TOK * W * sizeof(float), b = (size_t)4 * GL_TOK * GL_K * sizeof(float);
  hipLaunchKernelGGL(glide_embed_bwd_kernel, dim3((unsigned)((Q + GL_TOK - 1) / GL_TOK)), dim3(256), a > b ? a : b, ST, g, x0, gamma, mean_rstd,
                     mean_rstd + M, w, stdv, dimg, N, R, W, mul);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
