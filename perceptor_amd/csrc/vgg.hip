// VGG-19 feature tower pieces and the style-transfer loss (perceptor/losses/style_transfer.py), 16-bit NHWC activations, fp32 accumulation:
//   pmi_maxpool2 / pmi_maxpool2_bwd   nn.MaxPool2d(2, 2) and its adjoint fused with the ReLU mask of the pooled tensor
//   pmi_gram                          G[(n,c),(m,d)] = scale * sum_p f[n,p,c] f[m,p,d]: both MFMA operands are transposed reads of the
//                                     same NHWC tensor (K runs along the pixels), split-K into a workspace, fixed-order reduce, mirrored
//   pmi_style_level                   mean|fa - fb|, mean|Ga - Gb| and S = sign(Ga - Gb) of one level
//   pmi_gram_bwd                      the level's gradient to fa: an MFMA GEMM with M = pixels, K = N*C gathered across the samples,
//                                     and one fused epilogue (sign term, coefficients, incoming gradient, ReLU mask, one 16-bit store)
// No atomics anywhere: scalars are two-stage sums through per-workgroup slots, the Gram's split-K slabs are added in slab order.
//
// The transposes: the Gram kernel stages [64 pixels][64 channels] blocks and writes them to the LDS as [channel][pixel], so each lane's
// fragment (one channel, 8 consecutive pixels) is one 16-byte LDS read.  The backward GEMM needs no transpose: its A operand (a pixel's
// channels of sample m) and its B operand (a row of S + S^T, the exact small integers -2 .. 2, written once per call into the caller's
// T workspace) are both K-contiguous, staged through the LDS with coalesced 16-byte loads.
#include "../../include/perceptor_hip.h"
#include "common.h"
#include "launch_util.h"

namespace {

constexpr int SLOTS = 1024;          // first-level slots of each scalar reduction
constexpr int GT = 64;               // Gram output tile (rows and columns) per workgroup
constexpr int GK = 64;               // pixels per staged K step
constexpr int GLD = GK + 8;          // LDS row pitch in elements: 144 bytes, 16-byte aligned rows
constexpr int GRAM_MAX_SPLITS = 32;

// ------------------------------------------------------------------------------------------------------------------ max pool
// one thread: 8 channels of one 2x2 window
template <typename T>
__global__ __launch_bounds__(256) void maxpool2_kernel(const u16* __restrict__ x, u16* __restrict__ y, int64_t units, int Ho, int Wo, int C) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= units) return;
  const int cg = C >> 3;
  const int g = (int)(u % cg);
  int64_t q = u / cg;
  const int wo = (int)(q % Wo); q /= Wo;
  const int ho = (int)(q % Ho);
  const int64_t n = q / Ho;
  const int W = 2 * Wo;
  const u16* src = x + (((n * 2 * Ho + 2 * ho) * W + 2 * wo) * (int64_t)C + 8 * g);
  const uint4 v[4] = {*(const uint4*)src, *(const uint4*)(src + C), *(const uint4*)(src + (int64_t)W * C), *(const uint4*)(src + (int64_t)W * C + C)};
  u16 out[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    u16 bb = 0; float bv = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t w = ((const uint32_t*)&v[k])[e >> 1];
      const u16 b = (u16)((e & 1) ? (w >> 16) : (w & 0xffff));
      const float f = T::to_f(b);
      if (k == 0 || f > bv) { bv = f; bb = b; }      // strict: the first maximum in row-major order wins
    }
    out[e] = bb;
  }
  *(uint4*)(y + u * 8) = make_uint4(out[0] | ((uint32_t)out[1] << 16), out[2] | ((uint32_t)out[3] << 16), out[4] | ((uint32_t)out[5] << 16),
                                    out[6] | ((uint32_t)out[7] << 16));
}

// dx[window position] = dy where the position is the window's first maximum and x > 0 there, else 0: the route is recomputed from x
template <typename T>
__global__ __launch_bounds__(256) void maxpool2_bwd_kernel(const u16* __restrict__ dy, const u16* __restrict__ x, u16* __restrict__ dx,
                                                           int64_t units, int Ho, int Wo, int C) {
  const int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (u >= units) return;
  const int cg = C >> 3;
  const int g = (int)(u % cg);
  int64_t q = u / cg;
  const int wo = (int)(q % Wo); q /= Wo;
  const int ho = (int)(q % Ho);
  const int64_t n = q / Ho;
  const int W = 2 * Wo;
  const int64_t base = ((n * 2 * Ho + 2 * ho) * W + 2 * wo) * (int64_t)C + 8 * g;
  const int64_t off[4] = {0, C, (int64_t)W * C, (int64_t)W * C + C};
  uint4 v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k] = *(const uint4*)(x + base + off[k]);
  const uint4 d = *(const uint4*)(dy + u * 8);
  u16 o[4][8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    int bk = 0; float bv = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t w = ((const uint32_t*)&v[k])[e >> 1];
      const float f = T::to_f((u16)((e & 1) ? (w >> 16) : (w & 0xffff)));
      if (k == 0 || f > bv) { bv = f; bk = k; }
    }
    const uint32_t dw = ((const uint32_t*)&d)[e >> 1];
    const u16 db = (u16)((e & 1) ? (dw >> 16) : (dw & 0xffff));
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k][e] = (k == bk && bv > 0.f) ? db : (u16)0;
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    *(uint4*)(dx + base + off[k]) = make_uint4(o[k][0] | ((uint32_t)o[k][1] << 16), o[k][2] | ((uint32_t)o[k][3] << 16),
                                               o[k][4] | ((uint32_t)o[k][5] << 16), o[k][6] | ((uint32_t)o[k][7] << 16));
}

// ------------------------------------------------------------------------------------------------------------------ Gram
// Workgroup (t, s): the 64 x 64 tile t of the upper block triangle over the pixels of split s -> ws[s][row][col].  Four waves, one 32 x 32
// quadrant each (mfma 32x32x16: lane (r, h) holds A[row r][k = 8h + j], B[k = 8h + j][col r]; D: col = lane & 31,
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)).
template <typename T>
__global__ __launch_bounds__(256) void gram_kernel(const u16* __restrict__ f, float* __restrict__ ws, int HW, int C, int R, int ntile,
                                                   int steps_per_split) {
  __shared__ __attribute__((aligned(16))) u16 As[GT * GLD];
  __shared__ __attribute__((aligned(16))) u16 Bs[GT * GLD];
  int ti = 0, rem = blockIdx.x;                     // tile index -> (ti <= tj)
  while (rem >= ntile - ti) { rem -= ntile - ti; ++ti; }
  const int tj = ti + rem;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;
  const int p_begin = blockIdx.y * steps_per_split * GK;
  const int p_end = min(HW, p_begin + steps_per_split * GK);
  f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;
  for (int p0 = p_begin; p0 < p_end; p0 += GK) {
    __syncthreads();
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int idx = tid + 256 * it, pl = idx >> 3, grp = idx & 7, p = p0 + pl;
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const int row = (side ? tj : ti) * GT + grp * 8;     // 8 rows = 8 channels of one sample (C % 8 == 0)
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row < R && p < p_end) {                          // tail pixels and rows past N*C are masked, not read
          const int n = row / C, c = row - n * C;
          v = *(const uint4*)(f + ((int64_t)n * HW + p) * C + c);
        }
        u16* dst = (side ? Bs : As) + (grp * 8) * GLD + pl;
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          dst[(2 * e) * GLD] = (u16)(w[e] & 0xffff);
          dst[(2 * e + 1) * GLD] = (u16)(w[e] >> 16);
        }
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < GK / 16; ++ks) {
      const uint4 a = *(const uint4*)(As + (wr * 32 + r) * GLD + ks * 16 + 8 * h);
      const uint4 b = *(const uint4*)(Bs + (wc * 32 + r) * GLD + ks * 16 + 8 * h);
      acc = T::mfma32(a, b, acc);
    }
  }
  float* out = ws + (int64_t)blockIdx.y * R * R;
  const int col = tj * GT + wc * 32 + r;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = ti * GT + wr * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
    if (row < R && col < R) out[(int64_t)row * R + col] = acc[i];
  }
}

// G[i][j] = G[j][i] = scale * (ws[0][i][j] + ws[1][i][j] + ...), i <= j: the slabs in order, the mirror written from the same value
__global__ __launch_bounds__(256) void gram_reduce_kernel(const float* __restrict__ ws, float* __restrict__ G, int R, int splits, float scale) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)R * R) return;
  const int i = (int)(e / R), j = (int)(e - (int64_t)i * R);
  if (i > j) return;
  float v = 0.f;
  for (int s = 0; s < splits; ++s) v += ws[(int64_t)s * R * R + e];
  v *= scale;
  G[e] = v;
  G[(int64_t)j * R + i] = v;
}

// ------------------------------------------------------------------------------------------------------------------ level sums
template <typename T>
__global__ __launch_bounds__(256) void feat_l1_kernel(const u16* __restrict__ a, const u16* __restrict__ b, float* __restrict__ partial,
                                                      int64_t units) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
    float fa[8], fb[8];
    unpack8<T>(*(const uint4*)(a + u * 8), fa);
    unpack8<T>(*(const uint4*)(b + u * 8), fb);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc += fabsf(fa[e] - fb[e]);
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

template <typename T>
__global__ __launch_bounds__(256) void gram_l1_sign_kernel(const float* __restrict__ Ga, const float* __restrict__ Gb, u16* __restrict__ S,
                                                           float* __restrict__ partial, int64_t units) {
  __shared__ float red[4];
  const u16 one = T::from_f(1.f), mone = T::from_f(-1.f);
  float acc = 0.f;
  for (int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (int64_t)gridDim.x * 256) {
    const float4 x = *(const float4*)(Ga + u * 4), y = *(const float4*)(Gb + u * 4);
    const float d[4] = {x.x - y.x, x.y - y.y, x.z - y.z, x.w - y.w};
    u16 s[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) { acc += fabsf(d[e]); s[e] = d[e] > 0.f ? one : (d[e] < 0.f ? mone : (u16)0); }
    *(uint2*)(S + u * 4) = make_uint2(s[0] | ((uint32_t)s[1] << 16), s[2] | ((uint32_t)s[3] << 16));
  }
  acc = block_sum_256(acc, red);
  if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}

// loss2[0] = s0 * sum partial[0 .. n0), loss2[1] = s1 * sum partial[SLOTS .. SLOTS + n1): thread t owns slot t, then the fixed tree
__global__ __launch_bounds__(SLOTS) void level_final_kernel(const float* __restrict__ partial, int n0, int n1, float* __restrict__ loss2,
                                                            float s0, float s1) {
  __shared__ float r0[SLOTS / 64], r1[SLOTS / 64];
  const int t = threadIdx.x;
  float a = t < n0 ? partial[t] : 0.f;
  float b = t < n1 ? partial[SLOTS + t] : 0.f;
  a = wave_sum(a); b = wave_sum(b);
  if ((t & 63) == 0) { r0[t >> 6] = a; r1[t >> 6] = b; }
  __syncthreads();
  if (t == 0) {
    float sa = 0.f, sb = 0.f;
    for (int i = 0; i < SLOTS / 64; ++i) { sa += r0[i]; sb += r1[i]; }
    loss2[0] = sa * s0;
    loss2[1] = sb * s1;
  }
}

// ------------------------------------------------------------------------------------------------------------------ Gram backward
// T = S + S^T as 16-bit values (the exact integers -2 .. 2): the B operand of the level-gradient GEMM
template <typename T>
__global__ __launch_bounds__(256) void sign_sum_kernel(const u16* __restrict__ S, u16* __restrict__ Tm, int R) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)R * R) return;
  const int i = (int)(e / R), j = (int)(e - (int64_t)i * R);
  Tm[e] = T::from_f(T::to_f(S[e]) + T::to_f(S[(int64_t)j * R + i]));
}

// Workgroup (bx, by, n): BP = 128 pixels x BC = 64 channels of sample n.  acc[p][c] = sum_k fa[m(k), p, d(k)] * T[(n, c), k], k = (m, d)
// over all N*C rows.  Both operands are K-contiguous in memory (a pixel's channels; a row of T), so a K chunk of 64 is staged with
// coalesced 16-byte loads (8 consecutive lanes per 128-byte row piece) into [row][64 + 8] LDS images and every fragment is one
// ds_read_b128.  Four waves: wave (wr, wc) owns pixels 64 wr .. + 64 (two 32 x 32 tiles) and channels 32 wc .. + 32.
constexpr int BP = 128, BC = 64, BK = 64, BLD = BK + 8;
template <typename T>
__global__ __launch_bounds__(256) void gram_bwd_kernel(const u16* __restrict__ fa, const u16* __restrict__ fb, const u16* __restrict__ Tm,
                                                       const u16* __restrict__ g_in, u16* __restrict__ dF, int HW, int C, int R,
                                                       float c_feat, float c_gram, float gscale) {
  __shared__ __attribute__((aligned(16))) u16 As[BP * BLD];
  __shared__ __attribute__((aligned(16))) u16 Bs[BC * BLD];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, r = lane & 31, h = lane >> 5;
  const int wr = wv >> 1, wc = wv & 1;
  const int n = blockIdx.z, p0 = blockIdx.x * BP, c0 = blockIdx.y * BC;
  f32x16 acc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) acc[t][i] = 0.f;
  const int ch = tid & 7;                                     // 16-byte piece of the 128-byte K chunk
  for (int k0 = 0; k0 < R; k0 += BK) {
    const int kk = k0 + 8 * ch;                               // 8 consecutive k: 8 channels of one sample (C % 8 == 0, R % 16 == 0)
    const bool k_ok = kk < R;
    const int m = k_ok ? kk / C : 0, d = kk - m * C;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < BP / 32; ++it) {
      const int row = (tid >> 3) + 32 * it, p = p0 + row;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (k_ok && p < HW) v = *(const uint4*)(fa + ((int64_t)m * HW + p) * C + d);
      *(uint4*)(As + row * BLD + 8 * ch) = v;
    }
#pragma unroll
    for (int it = 0; it < BC / 32; ++it) {
      const int row = (tid >> 3) + 32 * it, c = c0 + row;
      uint4 v = make_uint4(0, 0, 0, 0);
      if (k_ok && c < C) v = *(const uint4*)(Tm + ((int64_t)n * C + c) * R + kk);
      *(uint4*)(Bs + row * BLD + 8 * ch) = v;
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      const uint4 b = *(const uint4*)(Bs + (wc * 32 + r) * BLD + ks * 16 + 8 * h);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const uint4 a = *(const uint4*)(As + (wr * 64 + t * 32 + r) * BLD + ks * 16 + 8 * h);
        acc[t] = T::mfma32(a, b, acc[t]);
      }
    }
  }
  const int c = c0 + wc * 32 + r;
  if (c >= C) return;
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int p = p0 + wr * 64 + t * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
      if (p >= HW) continue;
      const int64_t off = ((int64_t)n * HW + p) * C + c;
      const float a = T::to_f(fa[off]), bb = T::to_f(fb[off]);
      const float sg = a > bb ? 1.f : (a < bb ? -1.f : 0.f);
      float v = gscale * (c_feat * sg + c_gram * acc[t][i]);
      if (g_in) v += T::to_f(g_in[off]);
      dF[off] = T::from_f(a > 0.f ? v : 0.f);
    }
}

inline int gram_splits(int R, int HW) {
  const int nt = (R + GT - 1) / GT, tiles = nt * (nt + 1) / 2, steps = (HW + GK - 1) / GK;
  int s = 512 / tiles;
  if (s < 1) s = 1;
  if (s > steps) s = steps;
  if (s > GRAM_MAX_SPLITS) s = GRAM_MAX_SPLITS;
  return s;
}
inline bool level_args_ok(int N, int HW, int C) {
  return N > 0 && HW > 0 && C > 0 && C % 16 == 0 && (int64_t)N * C <= 8192 && (int64_t)N * HW * C < ((int64_t)1 << 31);
}
inline bool pool_args_ok(int N, int H, int W, int C) {
  return N > 0 && H > 0 && W > 0 && C > 0 && H % 2 == 0 && W % 2 == 0 && C % 8 == 0 && (int64_t)N * H * W * C < ((int64_t)1 << 40);
}

}  // namespace

#define ST ((hipStream_t)s)
#define BY_DTYPE(KERNEL, GRID, ...)                                                                              \
  do {                                                                                                           \
    if (dtype == PMI_DT_F16) hipLaunchKernelGGL(KERNEL<F16>, GRID, dim3(256), 0, ST, __VA_ARGS__);               \
    else hipLaunchKernelGGL(KERNEL<BF16>, GRID, dim3(256), 0, ST, __VA_ARGS__);                                  \
    PMI_CHECK_LAUNCH();                                                                                          \
  } while (0)

extern "C" int pmi_maxpool2(const void* x, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!x || !y || !pool_args_ok(N, H, W, C) || (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16)) return PMI_ERR_ARG;
  const int64_t units = (int64_t)N * (H / 2) * (W / 2) * (C / 8);
  BY_DTYPE(maxpool2_kernel, dim3((unsigned)((units + 255) / 256)), (const u16*)x, (u16*)y, units, H / 2, W / 2, C);
  return PMI_OK;
}

extern "C" int pmi_maxpool2_bwd(const void* dy, const void* x, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s) {
  if (!dy || !x || !dx || !pool_args_ok(N, H, W, C) || (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16)) return PMI_ERR_ARG;
  const int64_t units = (int64_t)N * (H / 2) * (W / 2) * (C / 8);
  BY_DTYPE(maxpool2_bwd_kernel, dim3((unsigned)((units + 255) / 256)), (const u16*)dy, (const u16*)x, (u16*)dx, units, H / 2, W / 2, C);
  return PMI_OK;
}

extern "C" int pmi_gram_workspace(int N, int HW, int C) {
  if (!level_args_ok(N, HW, C)) return PMI_ERR_ARG;
  const int64_t R = (int64_t)N * C, fl = R * R * gram_splits((int)R, HW);
  return fl < ((int64_t)1 << 31) ? (int)fl : PMI_ERR_ARG;
}

extern "C" int pmi_gram(const void* f, float* G, float* ws, int N, int HW, int C, float scale, int dtype, pmi_stream_t s) {
  if (!f || !G || !ws || !level_args_ok(N, HW, C) || (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16) || !(scale == scale)) return PMI_ERR_ARG;
  if (pmi_gram_workspace(N, HW, C) < 0) return PMI_ERR_ARG;
  const int R = N * C, nt = (R + GT - 1) / GT, splits = gram_splits(R, HW);
  const int steps = (HW + GK - 1) / GK, sps = (steps + splits - 1) / splits;
  const int used = (steps + sps - 1) / sps;                 // every launched split owns at least one step, so every slab read is written
  BY_DTYPE(gram_kernel, dim3(nt * (nt + 1) / 2, used), (const u16*)f, ws, HW, C, R, nt, sps);
  hipLaunchKernelGGL(gram_reduce_kernel, dim3((unsigned)(((int64_t)R * R + 255) / 256)), dim3(256), 0, ST, ws, G, R, used, scale);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

// partial: 2048 floats of workspace
extern "C" int pmi_style_level(const void* fa, const void* fb, const float* Ga, const float* Gb, void* S, float* loss2, float* partial,
                               int N, int HW, int C, int dtype, pmi_stream_t s) {
  if (!fa || !fb || !Ga || !Gb || !S || !loss2 || !partial || !level_args_ok(N, HW, C) || (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16))
    return PMI_ERR_ARG;
  const int64_t count = (int64_t)N * HW * C, R = (int64_t)N * C;
  const unsigned n0 = grid_256(count / 8, SLOTS), n1 = grid_256(R * R / 4, SLOTS);
  BY_DTYPE(feat_l1_kernel, dim3(n0), (const u16*)fa, (const u16*)fb, partial, count / 8);
  BY_DTYPE(gram_l1_sign_kernel, dim3(n1), Ga, Gb, (u16*)S, partial + SLOTS, R * R / 4);
  hipLaunchKernelGGL(level_final_kernel, dim3(1), dim3(SLOTS), 0, ST, partial, (int)n0, (int)n1, loss2, (float)(1.0 / (double)count),
                     (float)(1.0 / ((double)R * (double)R)));
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_gram_bwd(const void* fa, const void* fb, const void* S, void* T, const void* g_in, void* dF, int N, int HW, int C,
                            float c_feat, float c_gram, float gscale, int dtype, pmi_stream_t s) {
  if (!fa || !fb || !S || !T || !dF || !level_args_ok(N, HW, C) || (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16) || !(c_feat == c_feat) ||
      !(c_gram == c_gram) || !(gscale == gscale))
    return PMI_ERR_ARG;
  const int R = N * C;
  BY_DTYPE(sign_sum_kernel, dim3((unsigned)(((int64_t)R * R + 255) / 256)), (const u16*)S, (u16*)T, R);
  BY_DTYPE(gram_bwd_kernel, dim3((HW + BP - 1) / BP, (C + BC - 1) / BC, N), (const u16*)fa, (const u16*)fb, (const u16*)T, (const u16*)g_in,
           (u16*)dF, HW, C, R, c_feat, c_gram, gscale);
  return PMI_OK;
}
