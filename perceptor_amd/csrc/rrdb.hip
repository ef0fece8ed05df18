// The dense-block convolution of Real-ESRGAN's RRDBNet (perceptor/models/super_resolution/custom_rrdbnet_arch.py:9-127): one 3x3, pad-1,
// stride-1 convolution over a channel PREFIX of a 16-bit NHWC buffer that writes a channel SLICE of a buffer (possibly the same one), with
// bias, LeakyReLU, the scaled residuals and the nearest x2 up-sampling of the tail folded in:
//   z = sum_{tap, c < Cin} X[pix + tap][c] W[n][tap][c] + bias[n]      zero padding; up = 1: X is read at (y >> 1, x >> 1) of the half-size grid
//   a = z >= 0 ? z : slope z
//   D[pix][n] = beta (alpha a + R1[pix][n]) + R2[pix][n]               fp32 throughout, ONE rounding to 16 bit at the store
//
// Workgroup: 8 x 32 output pixels of one image, all N (32 or 64) output channels, four waves.  The (8 + 2) x (32 + 2) halo patch goes through
// the LDS in 32-channel chunks (96-byte pixel pitch: the 16 lanes of every ds_read_b128 lane group land on 16 distinct 16-byte slots);
// pixels outside the image are buffer loads with an out-of-range offset, which return zeros, so the tails need no branch.  The weights are
// read straight from L2 in fragment order (one convolution's weights are at most 221 KB) and stay in registers across the wave's four
// 16-pixel blocks.  Each wave owns ALL N columns of its 64 pixels (two tile rows): an LDS fragment feeds N / 16 MFMAs and no accumulator
// is shared between waves.  The MFMA is v_mfma_f32_16x16x32 with the weights as the A operand (rows = output channels) and the pixels as
// the B operand, so a lane ends up with 4 consecutive output channels of one pixel: residual loads and the store are 8 bytes per lane.
//
// Aliasing: the kernel reads channels [0, Cin) of X, N channels of R1 / R2, and writes exactly the N channels of D's slice at pixels inside
// the image -- D may be channels [Cin, Cin + N) of the buffer X points into, and R1 may be X itself.  The image index is blockIdx.z: no
// halo read and no store crosses an image boundary.
#include "../../include/perceptor_hip.h"
#include "common.h"
#include "launch_util.h"

namespace {

constexpr int TH = 8, TW = 32;                 // output tile
constexpr int PH = TH + 2, PW = TW + 2;        // halo patch
constexpr int PP = 48;                         // LDS pixel pitch in elements (96 bytes) for a 32-channel chunk
constexpr int NPIECE = PH * PW * 4;            // 16-byte pieces of one chunk of the patch
constexpr int NLOAD = (NPIECE + 255) / 256;    // per thread

template <typename T, int NB>
__global__ __launch_bounds__(256) void rdb_conv_kernel(const u16* X, int ldx, int nchunk, const uint4* __restrict__ Wp,
                                                       const float* __restrict__ bias, u16* D, int ldd, const u16* R1, int ldr1, const u16* R2,
                                                       int ldr2, float alpha, float beta, float slope, int up, int H, int W) {
  __shared__ __attribute__((aligned(16))) u16 patch[PH * PW * PP];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, q = lane >> 4, p16 = lane & 15;
  const int img = blockIdx.z, ty0 = blockIdx.y * TH, tx0 = blockIdx.x * TW;
  const int Hi = up ? H >> 1 : H, Wi = up ? W >> 1 : W;
  const int64_t img_elems = (int64_t)Hi * Wi * ldx;
  const __amdgpu_buffer_rsrc_t xr = make_rsrc(X + img * img_elems, img_elems * 2);

  // byte offsets of this thread's pieces of the patch inside the image (the same for every chunk)
  uint32_t src[NLOAD];
  int dst[NLOAD];
#pragma unroll
  for (int it = 0; it < NLOAD; ++it) {
    const int idx = tid + 256 * it, pp = idx >> 2, piece = idx & 3;
    const int py = pp / PW, px = pp - py * PW;
    int gy = ty0 - 1 + py, gx = tx0 - 1 + px;
    const bool ok = idx < NPIECE && gy >= 0 && gy < H && gx >= 0 && gx < W;
    if (up) { gy >>= 1; gx >>= 1; }
    src[it] = ok ? (uint32_t)(((gy * Wi + gx) * ldx + piece * 8) * 2) : PMI_BUF_OOB;
    dst[it] = idx < NPIECE ? pp * PP + piece * 8 : -1;
  }

  f32x4 acc[4][NB];
#pragma unroll
  for (int mb = 0; mb < 4; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = (f32x4){0.f, 0.f, 0.f, 0.f};

  uint4 stage[NLOAD];
#pragma unroll
  for (int it = 0; it < NLOAD; ++it) stage[it] = buf_load16(xr, src[it], 0);

  for (int c = 0; c < nchunk; ++c) {
    __syncthreads();                                     // the previous chunk's fragment reads are done
#pragma unroll
    for (int it = 0; it < NLOAD; ++it)
      if (dst[it] >= 0) *(uint4*)(patch + dst[it]) = stage[it];
    __syncthreads();
    if (c + 1 < nchunk) {                                // in flight during this chunk's MFMAs
#pragma unroll
      for (int it = 0; it < NLOAD; ++it) stage[it] = buf_load16(xr, src[it], (uint32_t)(c + 1) * 64u);
    }
    const uint4* wc = Wp + (int64_t)c * 9 * NB * 64 + lane;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      const int dy = tap / 3, dx = tap - 3 * dy;
      uint4 wf[NB];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) wf[nb] = wc[(tap * NB + nb) * 64];
#pragma unroll
      for (int mb = 0; mb < 4; ++mb) {
        const int row = 2 * wv + (mb >> 1) + dy, col = 16 * (mb & 1) + p16 + dx;
        const uint4 xf = *(const uint4*)(patch + (row * PW + col) * PP + 8 * q);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = T::mfma16(wf[nb], xf, acc[mb][nb]);
      }
    }
  }

  // D tile of one MFMA: column (lane & 15) = pixel, rows 4 (lane >> 4) + r = output channels
#pragma unroll
  for (int mb = 0; mb < 4; ++mb) {
    const int y = ty0 + 2 * wv + (mb >> 1), x = tx0 + 16 * (mb & 1) + p16;
    if (y >= H || x >= W) continue;
    const int64_t pix = ((int64_t)img * H + y) * W + x;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      const int n0 = nb * 16 + 4 * q;
      const float4 b = *(const float4*)(bias + n0);
      float v[4] = {acc[mb][nb][0] + b.x, acc[mb][nb][1] + b.y, acc[mb][nb][2] + b.z, acc[mb][nb][3] + b.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = alpha * (v[e] >= 0.f ? v[e] : slope * v[e]);
      if (R1) {
        const uint2 r = *(const uint2*)(R1 + pix * ldr1 + n0);
        v[0] += T::to_f((u16)(r.x & 0xffff)); v[1] += T::to_f((u16)(r.x >> 16));
        v[2] += T::to_f((u16)(r.y & 0xffff)); v[3] += T::to_f((u16)(r.y >> 16));
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] *= beta;
      if (R2) {
        const uint2 r = *(const uint2*)(R2 + pix * ldr2 + n0);
        v[0] += T::to_f((u16)(r.x & 0xffff)); v[1] += T::to_f((u16)(r.x >> 16));
        v[2] += T::to_f((u16)(r.y & 0xffff)); v[3] += T::to_f((u16)(r.y >> 16));
      }
      *(uint2*)(D + pix * ldd + n0) = pack4<T>(v[0], v[1], v[2], v[3]);
    }
  }
}

}  // namespace

extern "C" int pmi_rdb_conv3x3_eligible(int Cin, int N, int ldx, int ldd, int ldr1, int ldr2, int up, int images, int H, int W, int dtype) {
  if (dtype != PMI_DT_F16 && dtype != PMI_DT_BF16) return 0;
  if (Cin < 32 || Cin > 192 || Cin % 32 || (N != 32 && N != 64)) return 0;
  if (up != 0 && up != 1) return 0;
  if (images < 1 || images > 65535 || H < 1 || W < 1 || (up && ((H | W) & 1))) return 0;
  if (ldx < Cin || ldx % 8 || ldd < N || ldd % 8) return 0;
  if (ldr1 < 0 || ldr1 % 8 || ldr2 < 0 || ldr2 % 8) return 0;                      // 0: that residual is absent
  if ((ldr1 && ldr1 < N) || (ldr2 && ldr2 < N)) return 0;
  if ((H + TH - 1) / TH > 65535) return 0;
  const int64_t Hi = up ? H / 2 : H, Wi = up ? W / 2 : W;
  if (Hi * Wi * ldx * 2 > 0x7ffffff0ll) return 0;                                   // one image of X is one buffer resource
  return 1;
}

extern "C" int pmi_rdb_conv3x3(const void* X, int ldx, int Cin, const void* Wp, const float* bias, int N, void* D, int ldd, const void* R1,
                               int ldr1, const void* R2, int ldr2, float alpha, float beta, float slope, int up, int images, int H, int W,
                               int dtype, pmi_stream_t s) {
  if (!X || !Wp || !bias || !D) return PMI_ERR_ARG;
  if (!pmi_rdb_conv3x3_eligible(Cin, N, ldx, ldd, R1 ? ldr1 : 0, R2 ? ldr2 : 0, up, images, H, W, dtype)) return PMI_ERR_ARG;
  if ((R1 && ldr1 < N) || (R2 && ldr2 < N)) return PMI_ERR_ARG;
  if (((uintptr_t)X | (uintptr_t)Wp | (uintptr_t)bias | (uintptr_t)D | (uintptr_t)R1 | (uintptr_t)R2) & 15) return PMI_ERR_ARG;
  if (!finite_f(alpha) || !finite_f(beta) || !finite_f(slope)) return PMI_ERR_ARG;
  const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH, images);
#define RDB_LAUNCH(TT, NBV)                                                                                                             \
  hipLaunchKernelGGL((rdb_conv_kernel<TT, NBV>), grid, dim3(256), 0, (hipStream_t)s, (const u16*)X, ldx, Cin / 32, (const uint4*)Wp, bias, \
                     (u16*)D, ldd, (const u16*)R1, ldr1, (const u16*)R2, ldr2, alpha, beta, slope, up, H, W)
  if (dtype == PMI_DT_F16) { if (N == 32) RDB_LAUNCH(F16, 2); else RDB_LAUNCH(F16, 4); }
  else { if (N == 32) RDB_LAUNCH(BF16, 2); else RDB_LAUNCH(BF16, 4); }
#undef RDB_LAUNCH
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
