// One level of the LPIPS distance (lpips 0.1: NetLinLayer over unit-normalised features) and its adjoint, 16-bit NHWC features, fp32
// arithmetic, no atomics:
//   pmi_lpips_level      s[n][p] = sum_c w_c (fa_c / (|fa| + eps) - fb_c / (|fb| + eps))^2, the norms |fa|, |fb| (kept for the backward) and
//                        mean[n] = sum_p s[n][p] / HW (two-stage sum through per-workgroup slots, fixed order)
//   pmi_lpips_level_bwd  with ua = fa / (na + eps), q_c = 2 r w_c (ua_c - ub_c):  dfa = q / (na + eps) - fa (fa . q) / (na (na + eps)^2),
//                        dFa = (fa > 0) (gscale dfa + g_in_a); side b is the same with a and b swapped; either side or both per launch
// Both are memory bound.  A lane owns 8 consecutive channels of one pixel (one 16-byte load per side), C / 8 consecutive lanes form a pixel
// group (8 pixels per wave at C = 64, one at C = 512; C = 48 gives groups of six lanes and four idle lanes per wave), and a pixel's values
// stay in registers between the norm reduction, the fa . q reduction and the store: every feature element is read once per launch.
// Group sums: a xor butterfly when the group size is a power of two, else every lane adds its group's lanes in lane order; either way all
// lanes of a group hold the same bits.  Differences of two products round each product first (mul_rn: never contracted into an FMA), so
// the level and its adjoint are bit-symmetric under a swap of the sides and exactly zero for fa == fb.
#include "../../include/perceptor_hip.h"
#include "common.h"
#include "launch_util.h"

namespace {

constexpr int LP_SLOTS = 512;        // first-level slots per sample of the mean
constexpr float LP_EPS = 1e-10f;

// a * b rounded to fp32 on its own.  A plain product (also HIP's __fmul_rn, which is one) may be contracted into an FMA with the subtraction
// that follows: fma(a, ia, -(b * ib)) is the rounding residual of b * ib, not 0, when a == b and ia == ib.
__device__ __forceinline__ float mul_rn(float a, float b) {
  float r;
  asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}

// sum over the G consecutive lanes starting at lane `base` (G even, 2 .. 64; groups never straddle a wave)
__device__ __forceinline__ float group_sum(float v, int G, int base, bool pow2) {
  if (pow2) {
    for (int o = G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
  }
  float acc = 0.f;
  for (int j = 0; j < G; ++j) acc += __shfl(v, base + j);
  return acc;
}

struct Geometry {
  int G, ppw;        // lanes per pixel, pixels per wave
  bool pow2;
};
__device__ __forceinline__ Geometry geometry(int C) {
  Geometry g;
  g.G = C >> 3;
  g.ppw = 64 / g.G;
  g.pow2 = (g.G & (g.G - 1)) == 0;
  return g;
}

// grid (x, N): workgroup x of sample n walks pixel tiles of 4 * ppw pixels with stride gridDim.x
template <typename T>
__global__ __launch_bounds__(256) void lpips_level_kernel(const u16* __restrict__ fa, const u16* __restrict__ fb, const float* __restrict__ w,
                                                          float* __restrict__ s, float* __restrict__ na, float* __restrict__ nb,
                                                          float* __restrict__ partial, int HW, int C) {
  __shared__ float red[4];
  const Geometry g = geometry(C);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int pl = lane / g.G, cl = lane - pl * g.G, base = pl * g.G;
  const bool live = pl < g.ppw;                          // the idle lanes of a non-power-of-two group size
  const int n = blockIdx.y, tile = 4 * g.ppw;
  float wl[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) wl[e] = (w && live) ? w[8 * cl + e] : 1.f;
  float acc = 0.f;
  for (int p0 = blockIdx.x * tile; p0 < HW; p0 += gridDim.x * tile) {      // uniform per workgroup: the shuffles see every lane
    const int p = p0 + wv * g.ppw + pl;
    const bool ok = live && p < HW;
    const int64_t pix = (int64_t)n * HW + p;
    float a[8], b[8];
    uint4 va = make_uint4(0, 0, 0, 0), vb = make_uint4(0, 0, 0, 0);
    if (ok) {
      va = *(const uint4*)(fa + pix * C + 8 * cl);
      vb = *(const uint4*)(fb + pix * C + 8 * cl);
    }
    unpack8<T>(va, a);
    unpack8<T>(vb, b);
    float ssa = 0.f, ssb = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) { ssa += a[e] * a[e]; ssb += b[e] * b[e]; }
    const float ra = sqrtf(group_sum(ssa, g.G, base, g.pow2)), rb = sqrtf(group_sum(ssb, g.G, base, g.pow2));
    const float ia = 1.f / (ra + LP_EPS), ib = 1.f / (rb + LP_EPS);
    float t = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d = mul_rn(a[e], ia) - mul_rn(b[e], ib);      // both products rounded: swapping a and b negates d exactly
      t += wl[e] * (d * d);
    }
    t = group_sum(t, g.G, base, g.pow2);
    if (ok && cl == 0) {
      s[pix] = t;
      na[pix] = ra;
      nb[pix] = rb;
      acc += t;
    }
  }
  if (partial) {
    acc = block_sum_256(acc, red);
    if (threadIdx.x == 0) partial[(int64_t)n * LP_SLOTS + blockIdx.x] = acc;
  }
}

// mean[n] = scale * sum of partial[n][0 .. nslots): thread t owns slots t and t + 256, then the fixed tree
__global__ __launch_bounds__(256) void lpips_mean_kernel(const float* __restrict__ partial, int nslots, float* __restrict__ mean, float scale) {
  __shared__ float red[4];
  const int t = threadIdx.x;
  const float* row = partial + (int64_t)blockIdx.x * LP_SLOTS;
  float v = (t < nslots ? row[t] : 0.f) + (t + 256 < nslots ? row[t + 256] : 0.f);
  v = block_sum_256(v, red);
  if (t == 0) mean[blockIdx.x] = v * scale;
}

// grid (x, N), one tile per workgroup
template <typename T>
__global__ __launch_bounds__(256) void lpips_level_bwd_kernel(const u16* __restrict__ fa, const u16* __restrict__ fb, const float* __restrict__ w,
                                                              const float* __restrict__ na, const float* __restrict__ nb,
                                                              const float* __restrict__ r, const u16* __restrict__ gia,
                                                              const u16* __restrict__ gib, u16* __restrict__ dFa, u16* __restrict__ dFb, int HW,
                                                              int C, float gscale) {
  const Geometry g = geometry(C);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int pl = lane / g.G, cl = lane - pl * g.G, base = pl * g.G;
  const bool live = pl < g.ppw;
  const int n = blockIdx.y;
  const int p = blockIdx.x * 4 * g.ppw + wv * g.ppw + pl;
  const bool ok = live && p < HW;
  const int64_t pix = (int64_t)n * HW + p, off = pix * C + 8 * cl;
  float a[8], b[8], q[8];
  uint4 va = make_uint4(0, 0, 0, 0), vb = make_uint4(0, 0, 0, 0);
  float ra = 0.f, rb = 0.f, rr = 0.f;
  if (ok) {
    va = *(const uint4*)(fa + off);
    vb = *(const uint4*)(fb + off);
    ra = na[pix]; rb = nb[pix]; rr = r[pix];
  }
  unpack8<T>(va, a);
  unpack8<T>(vb, b);
  const float ia = 1.f / (ra + LP_EPS), ib = 1.f / (rb + LP_EPS);
  float da = 0.f, db = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float we = (w && live) ? w[8 * cl + e] : 1.f;
    q[e] = 2.f * rr * we * (mul_rn(a[e], ia) - mul_rn(b[e], ib));
    da += a[e] * q[e];
    db += b[e] * q[e];
  }
  da = group_sum(da, g.G, base, g.pow2);                 // fa . q  (before the bounds exit: the shuffles see every lane)
  db = group_sum(db, g.G, base, g.pow2);                 // fb . q  (side b's q is -q)
  if (!ok) return;
  if (dFa) {
    const float pa = ra > 0.f ? da * ia * ia / ra : 0.f;  // an all-zero pixel: the gradient is defined as 0 (the mask below does it)
    float in[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, o[8];
    if (gia) unpack8<T>(*(const uint4*)(gia + off), in);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = a[e] > 0.f ? gscale * (mul_rn(q[e], ia) - mul_rn(a[e], pa)) + in[e] : 0.f;
    *(uint4*)(dFa + off) = pack8<T>(o);
  }
  if (dFb) {
    const float pb = rb > 0.f ? db * ib * ib / rb : 0.f;
    float in[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, o[8];
    if (gib) unpack8<T>(*(const uint4*)(gib + off), in);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = b[e] > 0.f ? gscale * (mul_rn(b[e], pb) - mul_rn(q[e], ib)) + in[e] : 0.f;
    *(uint4*)(dFb + off) = pack8<T>(o);
  }
}

inline bool lpips_args_ok(int N, int HW, int C, int dtype) {
  return N > 0 && N <= 65535 && HW > 0 && C >= 16 && C % 16 == 0 && C <= 512 && (int64_t)N * HW * C < ((int64_t)1 << 40) &&
         (dtype == PMI_DT_F16 || dtype == PMI_DT_BF16);
}

}  // namespace

#define ST ((hipStream_t)s)

extern "C" int pmi_lpips_level(const void* fa, const void* fb, const float* w, float* s_out, float* na, float* nb, float* mean, float* partial,
                               int N, int HW, int C, int dtype, pmi_stream_t s) {
  if (!fa || !fb || !s_out || !na || !nb || (mean && !partial) || !lpips_args_ok(N, HW, C, dtype) || !aligned16(fa) || !aligned16(fb))
    return PMI_ERR_ARG;
  const int tile = 4 * (64 / (C / 8));
  const int64_t tiles = ((int64_t)HW + tile - 1) / tile;
  const int gx = (int)(tiles < LP_SLOTS ? tiles : LP_SLOTS);
  float* part = mean ? partial : nullptr;
  if (dtype == PMI_DT_F16)
    hipLaunchKernelGGL(lpips_level_kernel<F16>, dim3(gx, N), dim3(256), 0, ST, (const u16*)fa, (const u16*)fb, w, s_out, na, nb, part, HW, C);
  else
    hipLaunchKernelGGL(lpips_level_kernel<BF16>, dim3(gx, N), dim3(256), 0, ST, (const u16*)fa, (const u16*)fb, w, s_out, na, nb, part, HW, C);
  PMI_CHECK_LAUNCH();
  if (mean) {
    hipLaunchKernelGGL(lpips_mean_kernel, dim3(N), dim3(256), 0, ST, partial, gx, mean, (float)(1.0 / (double)HW));
    PMI_CHECK_LAUNCH();
  }
  return PMI_OK;
}

extern "C" int pmi_lpips_level_bwd(const void* fa, const void* fb, const float* w, const float* na, const float* nb, const float* r,
                                   const void* g_in_a, const void* g_in_b, void* dFa, void* dFb, int N, int HW, int C, float gscale,
                                   int dtype, pmi_stream_t s) {
  if (!fa || !fb || !na || !nb || !r || (!dFa && !dFb) || !lpips_args_ok(N, HW, C, dtype) || !finite_f(gscale) || !aligned16(fa) ||
      !aligned16(fb) || !aligned16(g_in_a) || !aligned16(g_in_b) || !aligned16(dFa) || !aligned16(dFb))
    return PMI_ERR_ARG;
  const int tile = 4 * (64 / (C / 8));
  const int64_t tiles = ((int64_t)HW + tile - 1) / tile;
  if (tiles > 0x7fffffff) return PMI_ERR_ARG;
  const dim3 grid((unsigned)tiles, N);
  if (dtype == PMI_DT_F16)
    hipLaunchKernelGGL(lpips_level_bwd_kernel<F16>, grid, dim3(256), 0, ST, (const u16*)fa, (const u16*)fb, w, na, nb, r, (const u16*)g_in_a,
                       (const u16*)g_in_b, (u16*)dFa, (u16*)dFb, HW, C, gscale);
  else
    hipLaunchKernelGGL(lpips_level_bwd_kernel<BF16>, grid, dim3(256), 0, ST, (const u16*)fa, (const u16*)fb, w, na, nb, r, (const u16*)g_in_a,
                       (const u16*)g_in_b, (u16*)dFa, (u16*)dFb, HW, C, gscale);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
