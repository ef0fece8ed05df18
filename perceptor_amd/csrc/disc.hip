// Kernels of the Real-ESRGAN U-Net discriminator's image gradient (engine/disc.py; perceptor/losses/super_resolution/
// unet_discriminator_sn.py:34-63).
//
// pmi_convt4x4s2: the input gradient of Conv2d(Cin, Cout, 4, 2, 1, bias=False), a transposed 4x4 / stride-2 / pad-1 convolution, taken by
// output parity: the hi-resolution pixel (2p + a, 2q + b) receives the four taps ky = 3 - 2u (a = 0) or 2 - 2u (a = 1), kx alike, from the
// low-resolution gradient at (p + a - 1 + u, q + b - 1 + v), u, v in {0, 1}; outside the low-resolution image the gradient is zero:
//   acc[n, 2p+a, 2q+b, ci] = sum_{u, v} sum_co W[co, ci, ky(a, u), kx(b, v)] g[n, p+a-1+u, q+b-1+v, co]
//   D = (acc + R) * (Y >= 0 ? 1 : slope)            fp32 throughout, ONE rounding to 16 bit at the store (none for an fp32 D)
// R is the gradient that reaches the same tensor through the U-Net skip, Y the stored LeakyReLU output the convolution read: one launch
// yields the gradient at the previous pre-activation.
//
// Workgroup: one phase (a, b) of 8 x 32 low-resolution pixels of one image, 64 (or 32) of the Cin output channels, four waves; the phase,
// the channel group and the image are blockIdx.z.  The (8 + 1) x (32 + 1) patch of the phase goes through the LDS once, in 32-channel
// chunks of Cout (96-byte pixel pitch: the 16 lanes of every ds_read_b128 lane group land on 16 distinct 16-byte slots, as rrdb.hip);
// pixels outside the image are buffer loads with an out-of-range offset, which return zeros, so tiles need no branch and any h, w >= 1 is
// taken.  The weights are read from L2 in fragment order (the host packs them per phase: engine/disc.py, pack_convt_weights) and stay in
// registers across the wave's four 16-pixel blocks.  The MFMA is v_mfma_f32_16x16x32 with the weights as the A operand (rows = output
// channels) and the pixels as the B operand, so a lane ends up with 4 consecutive channels of one pixel: R, Y and the store are 8 bytes
// per lane (16 for fp32).  The image index comes from blockIdx.z: no load and no store crosses an image.
//
// pmi_lrelu_bwd, pmi_lrelu_add: the LeakyReLU masks and activations that no convolution epilogue covers.  pmi_mean_f32: the mean of the
// fp32 logit map in a fixed two-stage order (256 contiguous ranges, then one tree), so two runs are bit-equal.
#include "../../include/perceptor_hip.h"
#include "common.h"
#include "launch_util.h"

namespace {

constexpr int TH = 8, TW = 32;                 // low-resolution tile of one phase
constexpr int PH = TH + 1, PW = TW + 1;        // its patch: rows p + a - 1 + u, columns q + b - 1 + v
constexpr int PP = 48;                         // LDS pixel pitch in elements (96 bytes) for a 32-channel chunk
constexpr int NPIECE = PH * PW * 4;            // 16-byte pieces of one chunk of the patch
constexpr int NLOAD = (NPIECE + 255) / 256;    // per thread

template <typename T, int NB, bool F32>
__global__ __launch_bounds__(256) void convt4x4s2_kernel(const u16* G, int ldg, int nchunk, const uint4* __restrict__ Wp, void* Dv, int ldd,
                                                         const u16* R, int ldr, const u16* Y, int ldy, float slope, int h, int w, int ngroups) {
  __shared__ __attribute__((aligned(16))) u16 patch[PH * PW * PP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4, p16 = lane & 15;
  int z = blockIdx.z;
  const int cg = z % ngroups;
  z /= ngroups;
  const int phase = z & 3, img = z >> 2, a = phase >> 1, b = phase & 1;
  const int ty0 = blockIdx.y * TH, tx0 = blockIdx.x * TW;
  const int64_t img_elems = (int64_t)h * w * ldg;
  const __amdgpu_buffer_rsrc_t gr = make_rsrc(G + img * img_elems, img_elems * 2);

  // byte offsets of this thread's pieces of the patch inside the image (the same for every chunk)
  uint32_t src[NLOAD];
  int dst[NLOAD];
#pragma unroll
  for (int it = 0; it < NLOAD; ++it) {
    const int idx = tid + 256 * it, pp = idx >> 2, piece = idx & 3;
    const int py = pp / PW, px = pp - py * PW;
    const int gy = ty0 + a - 1 + py, gx = tx0 + b - 1 + px;
    const bool ok = idx < NPIECE && gy >= 0 && gy < h && gx >= 0 && gx < w;
    src[it] = ok ? (uint32_t)(((gy * w + gx) * ldg + piece * 8) * 2) : PMI_BUF_OOB;
    dst[it] = idx < NPIECE ? pp * PP + piece * 8 : -1;
  }

  f32x4 acc[4][NB];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

  uint4 stage[NLOAD];
#pragma unroll
  for (int it = 0; it < NLOAD; ++it) stage[it] = buf_load16(gr, src[it], 0);

  // packed weights: [Cin / 16][phase][Cout / 32][u v][lane] fragments of 8 values
  const uint4* wbase = Wp + ((int64_t)(cg * NB) * 4 + phase) * nchunk * 256 + lane;
  const int64_t wnb = (int64_t)4 * nchunk * 256;           // fragments from one 16-channel block to the next
  for (int c = 0; c < nchunk; ++c) {
    __syncthreads();                                     // the previous chunk's fragment reads are done
#pragma unroll
    for (int it = 0; it < NLOAD; ++it)
      if (dst[it] >= 0) *(uint4*)(patch + dst[it]) = stage[it];
    __syncthreads();
    if (c + 1 < nchunk) {                                // in flight during this chunk's MFMAs
#pragma unroll
      for (int it = 0; it < NLOAD; ++it) stage[it] = buf_load16(gr, src[it], (uint32_t)(c + 1) * 64u);
    }
    const uint4* wc = wbase + (int64_t)c * 256;
#pragma unroll
    for (int uv = 0; uv < 4; ++uv) {
      const int u = uv >> 1, v = uv & 1;
      uint4 wf[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) wf[nb] = wc[nb * wnb + uv * 64];
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        const int row = 2 * wv + (mb >> 1) + u, col = 16 * (mb & 1) + p16 + v;
        const uint4 xf = *(const uint4*)(patch + (row * PW + col) * PP + 8 * q);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = T::mfma16(wf[nb], xf, acc[mb][nb]);
      }
    }
  }

  // D tile of one MFMA: column (lane & 15) = pixel, rows 4 (lane >> 4) + r = output channels
  const int H2 = 2 * h, W2 = 2 * w;
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    const int p = ty0 + 2 * wv + (mb >> 1), qx = tx0 + 16 * (mb & 1) + p16;
    if (p >= h || qx >= w) continue;
    const int64_t pix = ((int64_t)img * H2 + 2 * p + a) * W2 + 2 * qx + b;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int n0 = (cg * NB + nb) * 16 + 4 * q;
      float v[4] = {acc[mb][nb][0], acc[mb][nb][1], acc[mb][nb][2], acc[mb][nb][3]};
      if (R) {
        const uint2 r = *(const uint2*)(R + pix * ldr + n0);
        v[0] += T::to_f((u16)(r.x & 0xffff)); v[1] += T::to_f((u16)(r.x >> 16));
        v[2] += T::to_f((u16)(r.y & 0xffff)); v[3] += T::to_f((u16)(r.y >> 16));
      }
      if (Y) {
        const uint2 y = *(const uint2*)(Y + pix * ldy + n0);
        const float f[4] = {T::to_f((u16)(y.x & 0xffff)), T::to_f((u16)(y.x >> 16)), T::to_f((u16)(y.y & 0xffff)), T::to_f((u16)(y.y >> 16))};
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = f[e] >= 0.f ? v[e] : slope * v[e];
      }
      if constexpr (F32) *(float4*)((float*)Dv + pix * ldd + n0) = make_float4(v[0], v[1], v[2], v[3]);
      else *(uint2*)((u16*)Dv + pix * ldd + n0) = pack4<T>(v[0], v[1], v[2], v[3]);
    }
  }
}

// dz = (g + g2) * (y >= 0 ? 1 : slope); g2 optional
template <typename T>
__global__ __launch_bounds__(256) void lrelu_bwd_kernel(const u16* __restrict__ g, const u16* __restrict__ g2, const u16* __restrict__ y,
                                                        u16* __restrict__ dz, int64_t n, float slope) {
  const int64_t n8 = n >> 3, t = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  for (int64_t i = t; i < n8; i += step) {
    float a[8], b[8], f[8];
    unpack8<T>(((const uint4*)g)[i], a);
    unpack8<T>(((const uint4*)y)[i], f);
    if (g2) {
      unpack8<T>(((const uint4*)g2)[i], b);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += b[e];
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = f[e] >= 0.f ? a[e] : slope * a[e];
    ((uint4*)dz)[i] = pack8<T>(a);
  }
  const int64_t i = n8 * 8 + t;                           // the tail that is no whole vector
  if (i < n) {
    float a = T::to_f(g[i]);
    if (g2) a += T::to_f(g2[i]);
    dz[i] = T::from_f(T::to_f(y[i]) >= 0.f ? a : slope * a);
  }
}

// y = lrelu(z) + r; r optional
template <typename T>
__global__ __launch_bounds__(256) void lrelu_add_kernel(const u16* __restrict__ zp, const u16* __restrict__ r, u16* __restrict__ y, int64_t n,
                                                        float slope) {
  const int64_t n8 = n >> 3, t = (int64_t)blockIdx.x * 256 + threadIdx.x, step = (int64_t)gridDim.x * 256;
  for (int64_t i = t; i < n8; i += step) {
    float a[8], b[8];
    unpack8<T>(((const uint4*)zp)[i], a);
#pragma unroll
    for (int e = 0; e < 8; ++e) a[e] = a[e] >= 0.f ? a[e] : slope * a[e];
    if (r) {
      unpack8<T>(((const uint4*)r)[i], b);
#pragma unroll
      for (int e = 0; e < 8; ++e) a[e] += b[e];
    }
    ((uint4*)y)[i] = pack8<T>(a);
  }
  const int64_t i = n8 * 8 + t;
  if (i < n) {
    float a = T::to_f(zp[i]);
    a = a >= 0.f ? a : slope * a;
    if (r) a += T::to_f(r[i]);
    y[i] = T::from_f(a);
  }
}

// fixed tree over the 256 values of a workgroup
__device__ __forceinline__ float block_sum256(float v, float* sh) {
  sh[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

constexpr int MEAN_PARTS = 256;

__global__ __launch_bounds__(256) void mean_stage1_kernel(const float* __restrict__ x, float* __restrict__ partial, int64_t n, int64_t per) {
  __shared__ float sh[256];
  const int64_t lo = (int64_t)blockIdx.x * per, hi = lo + per < n ? lo + per : n;
  float s = 0.f;
  for (int64_t i = lo + threadIdx.x; i < hi; i += 256) s += x[i];
  s = block_sum256(s, sh);
  if (threadIdx.x == 0) partial[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void mean_stage2_kernel(const float* __restrict__ partial, float* __restrict__ out, float scale) {
  __shared__ float sh[256];
  const float s = block_sum256(partial[threadIdx.x], sh);
  if (threadIdx.x == 0) out[0] = s * scale;
}

}  // namespace

extern "C" int pmi_convt4x4s2_eligible(int Cout, int Cin, int ldg, int ldd, int ldr, int ldy, int images, int h, int w, int dtype) {
  if (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16) return 0;
  if (Cout < 32 || Cout > 512 || Cout % 32 || Cin < 32 || Cin % 32 || Cin > 4096) return 0;
  if (images < 1 || h < 1 || w < 1 || h > 16384 || w > 16384) return 0;
  if (ldg < Cout || ldg % 8 || ldd < Cin || ldd % 8) return 0;
  if (ldr < 0 || ldr % 8 || ldy < 0 || ldy % 8) return 0;                          // 0: that operand is absent
  if ((ldr && ldr < Cin) || (ldy && ldy < Cin)) return 0;
  const int ngroups = Cin % 64 ? Cin / 32 : Cin / 64;
  if ((int64_t)images * 4 * ngroups > 65535 || (h + TH - 1) / TH > 65535) return 0;
  if ((int64_t)h * w * ldg * 2 > 0x7ffffff0ll) return 0;                           // one image of g is one buffer resource
  return 1;
}

extern "C" int pmi_convt4x4s2(const void* G, int ldg, int Cout, const void* Wp, int Cin, void* D, int ldd, const void* R, int ldr,
                              const void* Y, int ldy, float slope, int out_f32, int images, int h, int w, int dtype, pmi_stream_t s) {
  if (!G || !Wp || !D) return PMI_ERR_ARG;
  if (out_f32 != 0 && out_f32 != 1) return PMI_ERR_ARG;
  if (!pmi_convt4x4s2_eligible(Cout, Cin, ldg, ldd, R ? ldr : 0, Y ? ldy : 0, images, h, w, dtype)) return PMI_ERR_ARG;
  if ((R && ldr < Cin) || (Y && ldy < Cin)) return PMI_ERR_ARG;
  if (((uintptr_t)G | (uintptr_t)Wp | (uintptr_t)D | (uintptr_t)R | (uintptr_t)Y) & 15) return PMI_ERR_ARG;
  if (!finite_f(slope)) return PMI_ERR_ARG;
  const int nb = Cin % 64 ? 2 : 4, ngroups = Cin / (16 * nb);
  const dim3 grid((w + TW - 1) / TW, (h + TH - 1) / TH, images * 4 * ngroups);
#define CONVT_LAUNCH(TT, NBV, F32V)                                                                                                    \
  hipLaunchKernelGGL((convt4x4s2_kernel<TT, NBV, F32V>), grid, dim3(256), 0, (hipStream_t)s, (const u16*)G, ldg, Cout / 32, (const uint4*)Wp, \
                     D, ldd, (const u16*)R, ldr, (const u16*)Y, ldy, slope, h, w, ngroups)
#define CONVT_NB(TT, F32V) do { if (nb == 2) CONVT_LAUNCH(TT, 2, F32V); else CONVT_LAUNCH(TT, 4, F32V); } while (0)
  if (dtype == PMI_DT_F16) { if (out_f32) CONVT_NB(F16, true); else CONVT_NB(F16, false); }
  else { if (out_f32) CONVT_NB(BF16, true); else CONVT_NB(BF16, false); }
#undef CONVT_NB
#undef CONVT_LAUNCH
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_lrelu_bwd(const void* g, const void* g2, const void* y, void* dz, int64_t n, float slope, int dtype, pmi_stream_t s) {
  if (!g || !y || !dz || n < 1 || !finite_f(slope)) return PMI_ERR_ARG;
  if (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16) return PMI_ERR_ARG;
  if (((uintptr_t)g | (uintptr_t)g2 | (uintptr_t)y | (uintptr_t)dz) & 15) return PMI_ERR_ARG;
  if (dtype == PMI_DT_F16)
    hipLaunchKernelGGL(lrelu_bwd_kernel<F16>, dim3(grid_256(n >> 3)), dim3(256), 0, (hipStream_t)s, (const u16*)g, (const u16*)g2, (const u16*)y, (u16*)dz, n, slope);
  else
    hipLaunchKernelGGL(lrelu_bwd_kernel<BF16>, dim3(grid_256(n >> 3)), dim3(256), 0, (hipStream_t)s, (const u16*)g, (const u16*)g2, (const u16*)y, (u16*)dz, n, slope);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_lrelu_add(const void* z, const void* r, void* y, int64_t n, float slope, int dtype, pmi_stream_t s) {
  if (!z || !y || n < 1 || !finite_f(slope)) return PMI_ERR_ARG;
  if (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16) return PMI_ERR_ARG;
  if (((uintptr_t)z | (uintptr_t)r | (uintptr_t)y) & 15) return PMI_ERR_ARG;
  if (dtype == PMI_DT_F16)
    hipLaunchKernelGGL(lrelu_add_kernel<F16>, dim3(grid_256(n >> 3)), dim3(256), 0, (hipStream_t)s, (const u16*)z, (const u16*)r, (u16*)y, n, slope);
  else
    hipLaunchKernelGGL(lrelu_add_kernel<BF16>, dim3(grid_256(n >> 3)), dim3(256), 0, (hipStream_t)s, (const u16*)z, (const u16*)r, (u16*)y, n, slope);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_mean_f32(const float* x, float* partial, float* out, int64_t n, float scale, pmi_stream_t s) {
  if (!x || !partial || !out || n < 1 || !finite_f(scale)) return PMI_ERR_ARG;
  if (((uintptr_t)x | (uintptr_t)partial | (uintptr_t)out) & 3) return PMI_ERR_ARG;
  const int64_t per = (n + MEAN_PARTS - 1) / MEAN_PARTS;
  hipLaunchKernelGGL(mean_stage1_kernel, dim3(MEAN_PARTS), dim3(256), 0, (hipStream_t)s, x, partial, n, per);
  hipLaunchKernelGGL(mean_stage2_kernel, dim3(1), dim3(256), 0, (hipStream_t)s, (const float*)partial, out, scale);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
