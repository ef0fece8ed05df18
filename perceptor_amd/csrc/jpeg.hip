// The differentiable JPEG codec behind drawers.JPEG (perceptor/drawers/jpeg/{compression,decompression,utils}.py), fp32 throughout:
//   pmi_jpeg_decode      quantised 8x8 DCT coefficients of Y, Cb, Cr (4:2:0) -> RGB images in [0, 1]      (decompress_jpeg.forward)
//   pmi_jpeg_decode_bwd  its exact adjoint with respect to the three coefficient tensors
//   pmi_jpeg_encode      RGB images -> coefficients, optionally with the cubic "differentiable rounding"     (compress_jpeg.forward)
// One launch each.  Layout: y [N][(H/8)(W/8)][8][8], cb / cr [N][(H/16)(W/16)][8][8], blocks row-major over the block grid, first index
// inside a block = row = the vertical frequency; images [N][3][H][W]; H and W multiples of 16.
//
// Work split: a 16 x 16 macroblock is six 8 x 8 blocks (four Y, Cb, Cr) and depends on nothing outside itself.  A workgroup of four waves
// covers MBW = 4 macroblocks side by side (16 rows x 64 columns); wave w owns macroblock w and holds its six blocks one value per lane
// (lane = 8 r + c: a coefficient block is one 256-byte load).  The 2-D transforms run separably, two 8-term passes through LDS; the sample
// planes of the 16 x 64 strip live in LDS, and the colour stage walks them with thread t = (row t / 16, pixel quad t % 16), so every image
// row is read and written as 256 contiguous bytes per plane (float4 per thread).  Tables are __constant__; no atomics, no scratch.
//
// The +128 of the chroma IDCT and the -128 of the colour matrix cancel and are never formed (likewise +128 / -128 in the encoder).
#include "common.h"
#include "launch_util.h"
#include "../../include/perceptor_hip.h"

namespace {

constexpr int MBW = 4;            // macroblocks per workgroup = waves per workgroup
constexpr int YS = 72, CS = 40;   // LDS row pitches of the luma / chroma planes: 8 rows of a block column fall into 8 distinct bank groups

// cos(k pi / 16), k = 0 .. 31: the DCT basis cos((2 v + 1) y pi / 16) is COS16[((2 v + 1) y) & 31]
__constant__ float COS16[32] = {
    1.f, 0.980785251f, 0.923879504f, 0.831469595f, 0.707106769f, 0.555570245f, 0.382683426f, 0.195090324f,
    0.f, -0.195090324f, -0.382683426f, -0.555570245f, -0.707106769f, -0.831469595f, -0.923879504f, -0.980785251f,
    -1.f, -0.980785251f, -0.923879504f, -0.831469595f, -0.707106769f, -0.555570245f, -0.382683426f, -0.195090324f,
    0.f, 0.195090324f, 0.382683426f, 0.555570245f, 0.707106769f, 0.831469595f, 0.923879504f, 0.980785251f};

// The Annex K tables in their printed orientation.  The reference multiplies element [i][j] of a block by the TRANSPOSED luma table
// (utils.py:21), so lane (r, c) reads QY[c][r]; the chroma table's 4 x 4 corner is transposed too (utils.py:28-30) and is symmetric.
__constant__ float QY[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                             18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
__constant__ float QC[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
                             99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

struct Tile {
  float a[MBW][6][64];      // per wave and block: dequantised coefficients (decode); rows 0 .. 2*16*CS alias the chroma gradient rows `gc`
  float b[MBW][6][64];      // per wave and block: the result of the first 1-D pass
  float yp[16][YS];         // luma plane of the strip (samples, then their gradient)
  float cp[2][8][CS];       // Cb, Cr planes of the strip (samples, WITHOUT the +128)
};
static_assert(2 * 16 * CS <= MBW * 6 * 64, "gc must fit into Tile::a");

// where a workgroup and its waves stand
struct Place {
  int n, my, mx0;           // sample, macroblock row, first macroblock column
  int wave, lane, r, c;
  bool active;              // this wave's macroblock exists (the last workgroup of a row may be short)
  int64_t yblk[4], cblk;    // block indices (sample included) of the wave's four Y blocks and of its chroma block
};

__device__ __forceinline__ Place place(int H, int W) {
  Place p;
  const int mbx = W >> 4, mby = H >> 4, gx = (mbx + MBW - 1) / MBW;
  int b = blockIdx.x;
  const int g = b % gx; b /= gx;
  p.my = b % mby; p.n = b / mby;
  p.mx0 = g * MBW;
  p.wave = threadIdx.x >> 6; p.lane = threadIdx.x & 63; p.r = p.lane >> 3; p.c = p.lane & 7;
  const int mx = p.mx0 + p.wave;
  p.active = mx < mbx;
  const int64_t ny = (int64_t)(H >> 3) * (W >> 3), nc = (int64_t)mby * mbx;
#pragma unroll
  for (int k = 0; k < 4; ++k) p.yblk[k] = (int64_t)p.n * ny + (int64_t)(2 * p.my + (k >> 1)) * (W >> 3) + 2 * mx + (k & 1);
  p.cblk = (int64_t)p.n * nc + (int64_t)p.my * mbx + mx;
  return p;
}

__device__ __forceinline__ float alpha2(int r, int c) { return (r == 0 ? 0.70710678118654752f : 1.f) * (c == 0 ? 0.70710678118654752f : 1.f); }

// The wave's macroblock: coefficients -> sample planes in LDS.  Every wave of the workgroup calls it (barriers inside); an inactive wave
// writes zeros.  out[u][v] = 0.25 sum_x sum_y (c q f alpha)[x][y] cos((2u+1) x pi/16) cos((2v+1) y pi/16) (+128 for luma).
__device__ __forceinline__ void idct_macroblock(Tile& T, const Place& p, const float* __restrict__ y, const float* __restrict__ cb,
                                                const float* __restrict__ cr, float factor) {
  const int r = p.r, c = p.c, lane = p.lane, w = p.wave;
  float cw[8], rw[8];                                         // cos((2c+1) k pi/16), cos((2r+1) k pi/16)
#pragma unroll
  for (int k = 0; k < 8; ++k) { cw[k] = COS16[((2 * c + 1) * k) & 31]; rw[k] = COS16[((2 * r + 1) * k) & 31]; }
  const float a2 = alpha2(r, c);
  const float dqy = QY[c * 8 + r] * a2 * factor, dqc = QC[c * 8 + r] * a2 * factor;
  float s[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) s[k] = 0.f;
  if (p.active) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s[k] = y[p.yblk[k] * 64 + lane] * dqy;
    s[4] = cb[p.cblk * 64 + lane] * dqc;
    s[5] = cr[p.cblk * 64 + lane] * dqc;
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) T.a[w][k][lane] = s[k];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 6; ++k) {                                // along the second index: t[r][v = c] = sum_y s[r][y] cos((2c+1) y pi/16)
    const float4 lo = *(const float4*)&T.a[w][k][r * 8], hi = *(const float4*)&T.a[w][k][r * 8 + 4];
    float t = lo.x * cw[0];
    t = fmaf(lo.y, cw[1], t); t = fmaf(lo.z, cw[2], t); t = fmaf(lo.w, cw[3], t);
    t = fmaf(hi.x, cw[4], t); t = fmaf(hi.y, cw[5], t); t = fmaf(hi.z, cw[6], t); t = fmaf(hi.w, cw[7], t);
    T.b[w][k][lane] = t;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 6; ++k) {                                // along the first: out[u = r][c] = sum_x t[x][c] cos((2r+1) x pi/16)
    float o = T.b[w][k][c] * rw[0];
#pragma unroll
    for (int x = 1; x < 8; ++x) o = fmaf(T.b[w][k][x * 8 + c], rw[x], o);
    o *= 0.25f;
    if (k < 4) T.yp[8 * (k >> 1) + r][16 * w + 8 * (k & 1) + c] = o + 128.f;
    else T.cp[k - 4][r][8 * w + c] = o;
  }
  __syncthreads();
}

// The transposed transform of the wave's macroblock from the planes in LDS: raw[k] = sum_u sum_v g[u][v] cos((2u+1) r pi/16) cos((2v+1) c pi/16)
// for lane (r, c), the caller scales.  Luma g = T.yp; chroma g[u][v] = gc[.][2u][v] + gc[.][2u + 1][v] (gc holds horizontal pair sums per
// image row).  Blocks outside `want` (bit k) are skipped; `want` is uniform over the workgroup.  Barriers inside.
__device__ __forceinline__ void dct_macroblock(Tile& T, const float (*gc)[16][CS], const Place& p, int want, float raw[6]) {
  const int r = p.r, c = p.c, lane = p.lane, w = p.wave;
  float ru[8], cv[8];                                         // cos((2k+1) r pi/16), cos((2k+1) c pi/16)
#pragma unroll
  for (int k = 0; k < 8; ++k) { ru[k] = COS16[((2 * k + 1) * r) & 31]; cv[k] = COS16[((2 * k + 1) * c) & 31]; }
#pragma unroll
  for (int k = 0; k < 6; ++k) {                                // along the rows: a[x = r][v = c] = sum_u g[u][c] cos((2u+1) r pi/16)
    if (!((want >> k) & 1)) continue;
    float acc = 0.f;
    if (k < 4) {
      const float* g = &T.yp[8 * (k >> 1)][16 * w + 8 * (k & 1) + c];
      acc = g[0] * ru[0];
#pragma unroll
      for (int u = 1; u < 8; ++u) acc = fmaf(g[u * YS], ru[u], acc);
    } else {
      const float* g = &gc[k - 4][0][8 * w + c];
      acc = (g[0] + g[CS]) * ru[0];
#pragma unroll
      for (int u = 1; u < 8; ++u) acc = fmaf(g[2 * u * CS] + g[(2 * u + 1) * CS], ru[u], acc);
    }
    T.b[w][k][lane] = acc;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 6; ++k) {                                // along the columns: raw[r][y = c] = sum_v a[r][v] cos((2v+1) c pi/16)
    raw[k] = 0.f;
    if (!((want >> k) & 1)) continue;
    const float4 lo = *(const float4*)&T.b[w][k][r * 8], hi = *(const float4*)&T.b[w][k][r * 8 + 4];
    float t = lo.x * cv[0];
    t = fmaf(lo.y, cv[1], t); t = fmaf(lo.z, cv[2], t); t = fmaf(lo.w, cv[3], t);
    t = fmaf(hi.x, cv[4], t); t = fmaf(hi.y, cv[5], t); t = fmaf(hi.z, cv[6], t); t = fmaf(hi.w, cv[7], t);
    raw[k] = t;
  }
}

// ycbcr_to_rgb_jpeg (decompression.py:135-147) on samples whose chroma carries no +128; values on the 0 .. 255 scale, before the clamp
__device__ __forceinline__ void ycc_to_rgb(float y, float cb, float cr, float& R, float& G, float& B) {
  R = fmaf(1.402f, cr, y);
  G = fmaf(-0.714136f, cr, fmaf(-0.344136f, cb, y));
  B = fmaf(1.772f, cb, y);
}

__device__ __forceinline__ float comp(const float4& v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

__global__ __launch_bounds__(64 * MBW) void jpeg_decode_kernel(const float* __restrict__ y, const float* __restrict__ cb, const float* __restrict__ cr,
                                                               float factor, float* __restrict__ out, int H, int W) {
  __shared__ Tile T;
  const Place p = place(H, W);
  idct_macroblock(T, p, y, cb, cr, factor);
  const int row = threadIdx.x >> 4, q = threadIdx.x & 15, x0 = p.mx0 * 16 + 4 * q;
  if (x0 >= W) return;
  const float4 yy = *(const float4*)&T.yp[row][4 * q];
  const float2 b2 = *(const float2*)&T.cp[0][row >> 1][2 * q], r2 = *(const float2*)&T.cp[1][row >> 1][2 * q];
  float o[3][4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float R, G, B;
    ycc_to_rgb(comp(yy, i), i < 2 ? b2.x : b2.y, i < 2 ? r2.x : r2.y, R, G, B);
    o[0][i] = fminf(fmaxf(R, 0.f), 255.f) / 255.f;
    o[1][i] = fminf(fmaxf(G, 0.f), 255.f) / 255.f;
    o[2][i] = fminf(fmaxf(B, 0.f), 255.f) / 255.f;
  }
  const int64_t plane = (int64_t)H * W;
  float* dst = out + (int64_t)p.n * 3 * plane + (int64_t)(p.my * 16 + row) * W + x0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) *(float4*)(dst + ch * plane) = make_float4(o[ch][0], o[ch][1], o[ch][2], o[ch][3]);
}

__global__ __launch_bounds__(64 * MBW) void jpeg_decode_bwd_kernel(const float* __restrict__ y, const float* __restrict__ cb, const float* __restrict__ cr,
                                                                   float factor, const float* __restrict__ d_out, float* __restrict__ d_y,
                                                                   float* __restrict__ d_cb, float* __restrict__ d_cr, int H, int W) {
  __shared__ Tile T;
  float (*gc)[16][CS] = (float (*)[16][CS])&T.a[0][0][0];
  const Place p = place(H, W);
  idct_macroblock(T, p, y, cb, cr, factor);                    // the forward's arithmetic: the same clamp decisions
  const int row = threadIdx.x >> 4, q = threadIdx.x & 15, x0 = p.mx0 * 16 + 4 * q;
  {
    float gy[4] = {0.f, 0.f, 0.f, 0.f}, gb[4] = {0.f, 0.f, 0.f, 0.f}, gr[4] = {0.f, 0.f, 0.f, 0.f};
    if (x0 < W) {
      const float4 yy = *(const float4*)&T.yp[row][4 * q];
      const float2 b2 = *(const float2*)&T.cp[0][row >> 1][2 * q], r2 = *(const float2*)&T.cp[1][row >> 1][2 * q];
      const int64_t plane = (int64_t)H * W;
      const float* src = d_out + (int64_t)p.n * 3 * plane + (int64_t)(p.my * 16 + row) * W + x0;
      const float4 dR = *(const float4*)src, dG = *(const float4*)(src + plane), dB = *(const float4*)(src + 2 * plane);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float R, G, B;
        ycc_to_rgb(comp(yy, i), i < 2 ? b2.x : b2.y, i < 2 ? r2.x : r2.y, R, G, B);
        const float gR = (R > 0.f && R < 255.f) ? comp(dR, i) / 255.f : 0.f;
        const float gG = (G > 0.f && G < 255.f) ? comp(dG, i) / 255.f : 0.f;
        const float gB = (B > 0.f && B < 255.f) ? comp(dB, i) / 255.f : 0.f;
        gy[i] = (gR + gG) + gB;
        gb[i] = fmaf(1.772f, gB, -0.344136f * gG);
        gr[i] = fmaf(1.402f, gR, -0.714136f * gG);
      }
    }
    // yp[row][4q ..] is read by this thread alone; the chroma rows go to gc (T.a is dead since the first pass of the IDCT)
    *(float4*)&T.yp[row][4 * q] = make_float4(gy[0], gy[1], gy[2], gy[3]);
    *(float2*)&gc[0][row][2 * q] = make_float2(gb[0] + gb[1], gb[2] + gb[3]);
    *(float2*)&gc[1][row][2 * q] = make_float2(gr[0] + gr[1], gr[2] + gr[3]);
  }
  __syncthreads();
  const int want = (d_y ? 15 : 0) | (d_cb ? 16 : 0) | (d_cr ? 32 : 0);
  float raw[6];
  dct_macroblock(T, gc, p, want, raw);
  if (!p.active) return;
  const float a2 = alpha2(p.r, p.c);
  const float sy = QY[p.c * 8 + p.r] * a2 * factor * 0.25f, sc = QC[p.c * 8 + p.r] * a2 * factor * 0.25f;
  if (d_y) {
#pragma unroll
    for (int k = 0; k < 4; ++k) d_y[p.yblk[k] * 64 + p.lane] = raw[k] * sy;
  }
  if (d_cb) d_cb[p.cblk * 64 + p.lane] = raw[4] * sc;
  if (d_cr) d_cr[p.cblk * 64 + p.lane] = raw[5] * sc;
}

// diff_round (utils.py:34-41): round half to even plus the cube of the remainder
__device__ __forceinline__ float quant_round(float x, int mode) {
  if (!mode) return x;
  const float r = rintf(x), d = x - r;
  return r + d * d * d;
}

__global__ __launch_bounds__(64 * MBW) void jpeg_encode_kernel(const float* __restrict__ img, float factor, int round_mode, float* __restrict__ y,
                                                               float* __restrict__ cb, float* __restrict__ cr, int H, int W) {
  __shared__ Tile T;
  float (*gc)[16][CS] = (float (*)[16][CS])&T.a[0][0][0];
  const Place p = place(H, W);
  const int row = threadIdx.x >> 4, q = threadIdx.x & 15, x0 = p.mx0 * 16 + 4 * q;
  {
    float yy[4] = {0.f, 0.f, 0.f, 0.f}, bb[4] = {0.f, 0.f, 0.f, 0.f}, rr[4] = {0.f, 0.f, 0.f, 0.f};
    if (x0 < W) {
      const int64_t plane = (int64_t)H * W;
      const float* src = img + (int64_t)p.n * 3 * plane + (int64_t)(p.my * 16 + row) * W + x0;
      const float4 vR = *(const float4*)src, vG = *(const float4*)(src + plane), vB = *(const float4*)(src + 2 * plane);
#pragma unroll
      for (int i = 0; i < 4; ++i) {                            // rgb_to_ycbcr_jpeg (compression.py:19-38); chroma without its +128
        const float R = comp(vR, i) * 255.f, G = comp(vG, i) * 255.f, B = comp(vB, i) * 255.f;
        yy[i] = fmaf(0.114f, B, fmaf(0.587f, G, 0.299f * R)) - 128.f;
        bb[i] = fmaf(0.5f, B, fmaf(-0.331264f, G, -0.168736f * R));
        rr[i] = fmaf(-0.081312f, B, fmaf(-0.418688f, G, 0.5f * R));
      }
    }
    *(float4*)&T.yp[row][4 * q] = make_float4(yy[0], yy[1], yy[2], yy[3]);
    *(float2*)&gc[0][row][2 * q] = make_float2(bb[0] + bb[1], bb[2] + bb[3]);
    *(float2*)&gc[1][row][2 * q] = make_float2(rr[0] + rr[1], rr[2] + rr[3]);
  }
  __syncthreads();
  float raw[6];
  dct_macroblock(T, gc, p, 63, raw);
  if (!p.active) return;
  const float a2 = alpha2(p.r, p.c) * 0.25f;
  const float sy = a2 / (QY[p.c * 8 + p.r] * factor), sc = 0.25f * a2 / (QC[p.c * 8 + p.r] * factor);      // 0.25: the 2 x 2 mean
#pragma unroll
  for (int k = 0; k < 4; ++k) y[p.yblk[k] * 64 + p.lane] = quant_round(raw[k] * sy, round_mode);
  cb[p.cblk * 64 + p.lane] = quant_round(raw[4] * sc, round_mode);
  cr[p.cblk * 64 + p.lane] = quant_round(raw[5] * sc, round_mode);
}

// workgroups of the launch, or 0 for a shape the kernels do not take
inline int64_t jpeg_grid(int N, int H, int W) {
  if (N <= 0 || H <= 0 || W <= 0 || (H & 15) || (W & 15)) return 0;
  const int64_t g = (int64_t)N * (H >> 4) * (((W >> 4) + MBW - 1) / MBW);
  return g > 0x7fffffffll ? 0 : g;
}

}  // namespace

#define ST ((hipStream_t)s)

extern "C" int pmi_jpeg_decode(const float* y, const float* cb, const float* cr, float factor, float* out, int N, int H, int W, pmi_stream_t s) {
  const int64_t g = jpeg_grid(N, H, W);
  if (!g || !y || !cb || !cr || !out || !finite_f(factor) || factor <= 0.f) return PMI_ERR_ARG;
  if (!aligned16(y) || !aligned16(cb) || !aligned16(cr) || !aligned16(out)) return PMI_ERR_ARG;
  hipLaunchKernelGGL(jpeg_decode_kernel, dim3((unsigned)g), dim3(64 * MBW), 0, ST, y, cb, cr, factor, out, H, W);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_jpeg_decode_bwd(const float* y, const float* cb, const float* cr, float factor, const float* d_out, float* d_y, float* d_cb,
                                   float* d_cr, int N, int H, int W, pmi_stream_t s) {
  const int64_t g = jpeg_grid(N, H, W);
  if (!g || !y || !cb || !cr || !d_out || !finite_f(factor) || factor <= 0.f) return PMI_ERR_ARG;
  if (!aligned16(y) || !aligned16(cb) || !aligned16(cr) || !aligned16(d_out) || !aligned16(d_y) || !aligned16(d_cb) || !aligned16(d_cr)) return PMI_ERR_ARG;
  if (!d_y && !d_cb && !d_cr) return PMI_OK;
  hipLaunchKernelGGL(jpeg_decode_bwd_kernel, dim3((unsigned)g), dim3(64 * MBW), 0, ST, y, cb, cr, factor, d_out, d_y, d_cb, d_cr, H, W);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_jpeg_encode(const float* images, float factor, int round_mode, float* y, float* cb, float* cr, int N, int H, int W, pmi_stream_t s) {
  const int64_t g = jpeg_grid(N, H, W);
  if (!g || !images || !y || !cb || !cr || !finite_f(factor) || factor <= 0.f || (round_mode != 0 && round_mode != 1)) return PMI_ERR_ARG;
  if (!aligned16(images) || !aligned16(y) || !aligned16(cb) || !aligned16(cr)) return PMI_ERR_ARG;
  hipLaunchKernelGGL(jpeg_encode_kernel, dim3((unsigned)g), dim3(64 * MBW), 0, ST, images, factor, round_mode, y, cb, cr, H, W);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
