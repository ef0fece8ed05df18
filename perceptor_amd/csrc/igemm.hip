// Implicit-GEMM convolution / GEMM for gfx950 on v_mfma_f32_32x32x16_{f16,bf16}.
//
//   D[m][n] = act(alpha * sum_k A(m,k) * B[n][k] + bias[n] + nbias[m/hw][n]) + R[m][n]
//
// Tile 128 (pixels) x 128 (output channels) x 64 (k) per 256-thread workgroup, 4 waves as
// 2 x 2, each wave a 64 x 64 sub-tile = 2 x 2 MFMA blocks of 32 x 32 (fp32 accumulate).
// The product is computed "swapped" (MFMA A operand = weights, B operand = activations) so
// an accumulator lane holds 4 consecutive output channels of one pixel: NHWC epilogue
// stores are 8-byte (16-bit out) or 16-byte (fp32 out) vectors.
// LDS: two stages x (16 KiB activations + 16 KiB weights) = 64 KiB -> 2 workgroups per CU.
// Rows are 128 B (64 k-elements); the 16-byte chunk index is XOR-swizzled with (row>>1)&7
// so both the ds_write_b128 staging and the ds_read_b128 fragment reads are conflict-free.
// Global->LDS goes through registers (gathered addresses + zero fill for the conv halo);
// the loads of k-tile t+1 are issued before the MFMAs of tile t and written after them.
// Conv taps: 9 = 3x3 (dy, dx in -1..1); 16 = the 4x4 stride-2 window (dy, dx in -1..2) of the
// Upsample2D adjoint, whose weights are the 3x3 kernel folded per output phase (engine/sd.py).
// PHASED (taps 9, stride 2, up 2): the adjoint of Downsample2D (pad right / bottom by one, 3x3 stride-2 convolution).  The input is the
// low-resolution gradient [Hin x Win], the output the 2Hin x 2Win one.  Output pixel (2p + a, 2q + b) only meets the kernel taps with
// ky = a, kx = b (mod 2): 4 / 2 / 2 / 1 of them for the phases (0,0) (0,1) (1,0) (1,1), at the input pixels (p - ty, q - tx), ty, tx in
// {0, 1}.  blockIdx.y is the phase (the 4-tap one first): the tap set is workgroup-uniform, a phase is a GEMM of M / 4 rows over its own
// K range of the phase-packed weights (engine/sd.py: pack_downsample_adjoint_weights), and the epilogue scatters a row to its pixel.
// 9 tap-products per 2 x 2 output block instead of the 36 of a 3x3 pass over a zero-inserted gradient.
#include <cstdio>
#include <cstdlib>
#include "common.h"
#include "epilogue.h"
#include "../../include/perceptor_hip.h"

namespace {

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int TILE_BYTES = 128 * 128;        // one operand tile: 128 rows x 128 B
constexpr int STAGE_BYTES = 2 * TILE_BYTES;  // activations + weights

__device__ __forceinline__ int lds_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

template <typename T, bool CONV, bool KFAST, bool PHASED = false>
__global__ __launch_bounds__(256, 2) void igemm_kernel(const pmi_igemm_args a) {
  static_assert(!PHASED || CONV, "the phased geometry is a convolution");
  __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wr = wid >> 1, wc = wid & 1;
#ifdef PMI_STAMPS   // tools/gemm_probe.py --stamps: phase timestamps (100 MHz) per workgroup; a.reserved carries the enable flag
#define GSTAMP(k) do { if (tid == 0 && a.reserved == 77 && a.splitk <= 1) ((long long*)a.ws)[(int64_t)blockIdx.x * 8 + (k)] = (long long)wall_clock64(); } while (0)
#else
#define GSTAMP(k) do {} while (0)
#endif
  GSTAMP(0);
  // PHASED: rows, k range and tap grid of this workgroup's phase (otherwise the whole problem)
  const int ph = PHASED ? (int)blockIdx.y : 0, pa = ph >> 1, pb = ph & 1;
  const int ntx = 2 - pb;                                                     // taps along x: kx in {0, 2} or {1}
  const int Mr = PHASED ? a.M >> 2 : a.M;
  const int Kr = PHASED ? (2 - pa) * ntx * (a.C0 + a.C1) : a.K;
  const int kofs = PHASED ? (ph == 0 ? 0 : 2 + 2 * ph) * (a.C0 + a.C1) : 0;    // first k of the phase: 0, 4, 6, 8 taps in
  const bool up1 = !PHASED && a.up;
  const int tiles_n = (a.N + BN - 1) / BN, tiles_m = (Mr + BM - 1) / BM;
  const int logical = xcd_remap(blockIdx.x, tiles_m * tiles_n);
  // Each XCD (own L2) gets a contiguous range of tiles.  Row-major ranges re-read all of B per XCD, column-major ranges all
  // of A: walk along the shorter operand so the longer one is split across the XCDs (ViT GEMMs: M = 2056, N up to 4096).
  const bool nmajor = Mr < a.N;
  const int m0 = (nmajor ? logical % tiles_m : logical / tiles_n) * BM, n0 = (nmajor ? logical / tiles_m : logical % tiles_n) * BN;

  const u16* A0 = (const u16*)a.A0;
  const u16* A1 = (const u16*)a.A1;
  const u16* Bw = (const u16*)a.B;
  int64_t offD = 0, offR = 0;
  if (a.batch > 1) {
    const int zo = blockIdx.z / a.batch_inner, zi = blockIdx.z % a.batch_inner;
    A0 += zo * a.sA_o + zi * a.sA_i;
    Bw += zo * a.sB_o + zi * a.sB_i;
    offD = zo * a.sD_o + zi * a.sD_i;
    offR = zo * a.sR_o + zi * a.sR_i;
  }

  // ---- per-thread staging coordinates: 4 rows x one 16-byte chunk of each operand tile ----
  const int srow = tid >> 3, sc = tid & 7;
  const int Cin = a.C0 + a.C1;
  const int Hv = up1 ? a.Hin * 2 : a.Hin, Wv = up1 ? a.Win * 2 : a.Win;
  int ys[4], xs[4], nb[4];
  int64_t arow[4];
  int64_t brow[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + srow + 32 * i;
    if (CONV) {
      if (PHASED && m < Mr) {                 // rows of a phase run over the low-resolution grid
        const int hw = a.Hin * a.Win;
        const int img = m / hw, rem = m - img * hw;
        const int y = rem / a.Win;
        ys[i] = y; xs[i] = rem - y * a.Win; nb[i] = img * a.Hin;
      } else if (m < Mr) {
        const int hw = a.H * a.W;
        const int img = m / hw, rem = m - img * hw;
        const int y = rem / a.W, x = rem - y * a.W;
        ys[i] = y * a.stride; xs[i] = x * a.stride; nb[i] = img * a.Hin;
      } else {
        ys[i] = -(1 << 20); xs[i] = 0; nb[i] = 0;
      }
    } else {
      arow[i] = m < Mr ? (int64_t)m : -1;
    }
    const int n = n0 + srow + 32 * i;
    brow[i] = n < a.N ? (int64_t)n * a.ldb : -1;
  }

  uint4 ra0[4], rb0[4], ra1[4], rb1[4];   // two register sets: global loads run two k-tiles ahead of the MFMAs
  int tap_u = 0, ci_u = 0;  // KFAST: uniform (tap, channel) of the next k-tile to load

  // KFAST tiles are read with raw buffer loads (out-of-range offset = zero fill): no divergent branch around a load, so
  // the compiler keeps exact vmcnt counts and the two-tile lookahead survives (see conv3x3.hip).  Bases are moved to the
  // tile's first row / image so 32-bit offsets suffice.
  const int hw_out = PHASED ? a.Hin * a.Win : CONV ? a.H * a.W : 1;
  const int img0 = CONV ? m0 / hw_out : 0;
  const int64_t a_skip = CONV ? (int64_t)img0 * a.Hin * a.Win : (int64_t)m0;            // rows (pixels) in front of the base
  const int64_t a_rows = (CONV ? (int64_t)(Mr / hw_out) * a.Hin * a.Win : (int64_t)a.M) - a_skip;
  const u16* const A0b = A0 + a_skip * a.lda0;
  const u16* const A1b = A1 ? A1 + a_skip * a.lda1 : A0b;
  const int64_t bytesA0 = ((a_rows - 1) * a.lda0 + a.C0) * 2, bytesA1 = A1 ? ((a_rows - 1) * a.lda1 + a.C1) * 2 : 0;
  const int nrows_b = min(BN, a.N - n0);
  const __amdgpu_buffer_rsrc_t rsrc_b = make_rsrc(Bw + (int64_t)n0 * a.ldb, ((int64_t)(nrows_b - 1) * a.ldb + a.K) * 2);
  uint32_t vob[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) vob[i] = (uint32_t)((srow + 32 * i) * a.ldb + sc * 8) * 2u;

  int kt_end = 0;                                        // first k-tile past this workgroup's range (set below)
  auto load_tile = [&](int kt, uint4* ra, uint4* rb) {
    const bool dead = kt >= kt_end;                      // lookahead past the end: zero tiles, no control flow
    if constexpr (KFAST) {
      const int tap = tap_u, cbase = ci_u;
      ci_u += BK;
      if (ci_u >= Cin) { ci_u -= Cin; ++tap_u; }
      const bool second = cbase >= a.C0;               // uniform: C0 is a multiple of BK
      const __amdgpu_buffer_rsrc_t rs = make_rsrc(second ? A1b : A0b, second ? bytesA1 : bytesA0);
      const uint32_t ld2 = (uint32_t)(second ? a.lda1 : a.lda0) * 2u;
      const uint32_t so = (uint32_t)(cbase - (second ? a.C0 : 0)) * 2u;
      int dy = 0, dx = 0;
      if (PHASED) { dy = -(tap >> (ntx - 1)); dx = -(tap & (ntx - 1)); }
      else if (CONV && a.taps == 9) { dy = tap / 3 - 1; dx = tap - (tap / 3) * 3 - 1; }
      if (CONV && a.taps == 16) { dy = (tap >> 2) - 1; dx = (tap & 3) - 1; }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        uint32_t vo;
        if (CONV) {
          int iy = ys[i] + dy, ix = xs[i] + dx;
          const bool ok = iy >= 0 && iy < Hv && ix >= 0 && ix < Wv;
          if (up1) { iy >>= 1; ix >>= 1; }
          vo = ok && !dead ? (uint32_t)((nb[i] - img0 * a.Hin + iy) * a.Win + ix) * ld2 + (uint32_t)sc * 16u : PMI_BUF_OOB;
        } else {
          vo = dead ? PMI_BUF_OOB : (uint32_t)(srow + 32 * i) * ld2 + (uint32_t)sc * 16u;   // rows past M fall outside the resource
        }
        ra[i] = buf_load16(rs, vo, so);
        rb[i] = buf_load16(rsrc_b, dead ? PMI_BUF_OOB : vob[i], (uint32_t)(kt * BK + kofs) * 2u);
      }
      return;
    }
    const int k = kt * BK + sc * 8;
    const bool kok = k < Kr && !dead;
    const int tap = k / Cin, ci = k - tap * Cin;
    const bool second = ci >= a.C0;
    const u16* base = second ? A1 : A0;
    const int ld = second ? a.lda1 : a.lda0;
    const int cc = second ? ci - a.C0 : ci;
    int dy = 0, dx = 0;
    if (PHASED) { dy = -(tap >> (ntx - 1)); dx = -(tap & (ntx - 1)); }
    else if (CONV && a.taps == 9) { dy = tap / 3 - 1; dx = tap - (tap / 3) * 3 - 1; }
    if (CONV && a.taps == 16) { dy = (tap >> 2) - 1; dx = (tap & 3) - 1; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (CONV) {
        int iy = ys[i] + dy, ix = xs[i] + dx;
        if (kok && iy >= 0 && iy < Hv && ix >= 0 && ix < Wv) {
          if (up1) { iy >>= 1; ix >>= 1; }
          v = *(const uint4*)(base + ((int64_t)(nb[i] + iy) * a.Win + ix) * ld + cc);
        }
      } else {
        if (kok && arow[i] >= 0) v = *(const uint4*)(base + arow[i] * ld + cc);
      }
      ra[i] = v;
      uint4 w = make_uint4(0, 0, 0, 0);
      if (kok && brow[i] >= 0) w = *(const uint4*)(Bw + brow[i] + k + kofs);
      rb[i] = w;
    }
  };
  auto store_tile = [&](int stage, const uint4* ra, const uint4* rb) {
    char* sa = smem + stage * STAGE_BYTES;
    char* sb = sa + TILE_BYTES;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int off = lds_off(srow + 32 * i, sc);
      *(uint4*)(sa + off) = ra[i];
      *(uint4*)(sb + off) = rb[i];
    }
  };

  f32x16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk_all = (Kr + BK - 1) / BK;
  const int l31 = lane & 31, lhi = lane >> 5;
  // split-K (grid.z when batch <= 1): this workgroup reduces k-tiles [kt0, kt0 + nk) into its own fp32 slab
  int kt0 = 0, nk = nk_all;
  if (a.splitk > 1) {
    const int per = (nk_all + a.splitk - 1) / a.splitk;
    kt0 = blockIdx.z * per;
    nk = min(per, nk_all - kt0);
    if (KFAST) { tap_u = (kt0 * BK) / Cin; ci_u = kt0 * BK - tap_u * Cin; }
  }

  auto mma_tile = [&](int stage) {
    const char* sa = smem + stage * STAGE_BYTES;
    const char* sb = sa + TILE_BYTES;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const int ch = kk * 2 + lhi;
      uint4 xf[2], wf[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) xf[i] = *(const uint4*)(sa + lds_off(wr * 64 + i * 32 + l31, ch));
#pragma unroll
      for (int j = 0; j < 2; ++j) wf[j] = *(const uint4*)(sb + lds_off(wc * 64 + j * 32 + l31, ch));
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = T::mfma32(wf[j], xf[i], acc[i][j]);
    }
  };

  // Pipeline: LDS holds k-tile t (stage t&1); tile t+1 sits in one register set (loaded during iteration t-1) and the loads
  // of tile t+2 are issued into the other set before the MFMAs of tile t.  A 128x128x64 tile is only 16 MFMAs per wave --
  // one tile of lookahead left every iteration waiting on its own global loads (measured ~3600 cycles per iteration pair
  // against ~1500 for the LDS traffic).
  kt_end = kt0 + nk;
  load_tile(kt0, ra0, rb0);
  load_tile(kt0 + 1, ra1, rb1);
  store_tile(0, ra0, rb0);
  __syncthreads();
  GSTAMP(1);
  for (int kt = 0; kt < nk; kt += 2) {                   // an odd tile count runs one extra all-zero tile
    load_tile(kt0 + kt + 2, ra0, rb0);
    __builtin_amdgcn_sched_barrier(0);     // keep the loads in front of the MFMAs (the scheduler sinks them to their use)
    mma_tile(0);
    __builtin_amdgcn_sched_barrier(0);
    store_tile(1, ra1, rb1);
    __syncthreads();
    load_tile(kt0 + kt + 3, ra1, rb1);
    __builtin_amdgcn_sched_barrier(0);
    mma_tile(1);
    __builtin_amdgcn_sched_barrier(0);
    store_tile(0, ra0, rb0);
    __syncthreads();
  }

  GSTAMP(2);
  if (a.splitk > 1) {   // raw fp32 partial sums; bias / activation / residual happen in splitk_reduce_kernel
    float* slab = (float*)a.ws + (int64_t)blockIdx.z * a.M * a.N;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + wr * 64 + i * 32 + l31;
      if (m >= a.M) continue;
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = n0 + wc * 64 + j * 32 + 4 * lhi + 8 * g;
          if (n < a.N) *(float4*)(slab + (int64_t)m * a.N + n) = make_float4(acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]);
        }
    }
    return;
  }
  // ---- epilogue: lane = pixel (col), registers = 4 consecutive output channels x 4 groups ----
  // row of D that GEMM row m lands in.  PHASED: pixel (2p + pa, 2q + pb) of the high-resolution grid (no residual, per-sample bias or
  // statistics there: pmi_igemm rejects them, so every other use of m below is an unphased one)
  auto orow = [&](int m) -> int64_t {
    if constexpr (PHASED) {
      const int hw = a.Hin * a.Win;
      const int img = m / hw, rem = m - img * hw;
      const int p = rem / a.Win, q = rem - p * a.Win;
      return (int64_t)(img * a.H + 2 * p + pa) * a.W + 2 * q + pb;
    } else {
      return (int64_t)m;
    }
  };
  float* const stat = (float*)smem;            // [2 wave rows][BN][2] per-channel (sum, sumsq) of this tile (main loop is done with LDS)
  // Fast path (16-bit output, 16-byte aligned rows): each wave transposes its 64 x 64 tile through LDS and writes
  // 16 bytes per lane, 8 rows x 128 B per instruction, reading a 16-bit residual the same way.  In the accumulator layout a
  // store instruction covers 32 rows x 16 bytes, which the address coalescer handles several times slower -- decisive for the
  // short-K, store-heavy 1x1 convolutions (M = 2M rows, K = 256..768).
  const bool fast = !a.split_out && !a.out_f32 && !a.res_up && (a.ldd & 7) == 0 && (offD & 7) == 0 && (a.N & 7) == 0 && (((uintptr_t)a.D) & 15) == 0 &&
                    (!a.R || (!a.res_f32 && (a.ldr & 7) == 0 && (offR & 7) == 0 && (((uintptr_t)a.R) & 15) == 0));
  if (fast) {
    constexpr int SROW = 144;                  // staged row: 128 B + 16 B pad
    char* const stg = smem + 2 * 2 * BN * 4 + wid * (64 * SROW);      // behind the two statistics slots
    const int r8 = lane & 7, rp = lane >> 3;   // write-out role: 16-byte chunk r8 of row 8 t + rp
    const float* nbq[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = m0 + wr * 64 + i * 32 + l31;
      nbq[i] = (a.nbias && m < a.M) ? a.nbias + (int64_t)(m / a.hw) * (a.ldnb ? a.ldnb : a.N) : nullptr;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wc * 64 + j * 32 + 4 * lhi + 8 * g;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (a.bias && n < a.N) b = *(const float4*)(a.bias + n);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          float v[4] = {acc[i][j][4 * g] * a.alpha + b.x, acc[i][j][4 * g + 1] * a.alpha + b.y,
                        acc[i][j][4 * g + 2] * a.alpha + b.z, acc[i][j][4 * g + 3] * a.alpha + b.w};
          if (nbq[i] && n < a.N) { const float4 q = *(const float4*)(nbq[i] + n); v[0] += q.x; v[1] += q.y; v[2] += q.z; v[3] += q.w; }
          if (a.act != PMI_ACT_NONE) act_apply_n<4>(v, a.act);
          *(uint2*)(stg + (i * 32 + l31) * SROW + (j * 32 + 8 * g + 4 * lhi) * 2) = pack4<T>(v[0], v[1], v[2], v[3]);
        }
      }
      __builtin_amdgcn_sched_barrier(0);       // one 32-column block of bias loads in flight at a time (register budget)
    }
    const int cl0 = wc * 64 + r8 * 8;          // first of this lane's 8 columns inside the tile
    const bool nok = n0 + cl0 < a.N;
    uint4 rres[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int m = m0 + wr * 64 + 8 * t + rp;
      rres[t] = make_uint4(0, 0, 0, 0);
      if (a.R && nok && m < a.M) rres[t] = *(const uint4*)((const u16*)a.R + offR + (int64_t)m * a.ldr + n0 + cl0);
    }
    float cs[16];                              // [0..7] sums, [8..15] sums of squares of this lane's 8 columns
#pragma unroll
    for (int e = 0; e < 16; ++e) cs[e] = 0.f;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
      const int m = m0 + wr * 64 + 8 * t + rp;
      uint4 v = *(const uint4*)(stg + (8 * t + rp) * SROW + r8 * 16);
      if (a.R || a.stats) {
        float f[8];
        unpack8<T>(v, f);
        if (a.R) {
          float r[8];
          unpack8<T>(rres[t], r);
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] += r[e];
          v = pack8<T>(f);
        }
        if (m < a.M) {
#pragma unroll
          for (int e = 0; e < 8; ++e) { cs[e] += f[e]; cs[8 + e] += f[e] * f[e]; }
        }
      }
      if (nok && m < Mr) *(uint4*)((u16*)a.D + offD + orow(m) * a.ldd + n0 + cl0) = v;
    }
    if (a.stats) {   // butterfly over the 8 lanes that share r8 (lane bits 3..5), halving the live values per step; one slot per wave row
      float b8[8], b4[4], b2[2];
      const bool h3 = lane & 8, h4 = lane & 16, h5 = lane & 32;
#pragma unroll
      for (int k = 0; k < 8; ++k) { const float mine = h3 ? cs[k + 8] : cs[k], other = h3 ? cs[k] : cs[k + 8]; b8[k] = mine + __shfl_xor(other, 8); }
#pragma unroll
      for (int k = 0; k < 4; ++k) { const float mine = h4 ? b8[k + 4] : b8[k], other = h4 ? b8[k] : b8[k + 4]; b4[k] = mine + __shfl_xor(other, 16); }
#pragma unroll
      for (int k = 0; k < 2; ++k) { const float mine = h5 ? b4[k + 2] : b4[k], other = h5 ? b4[k] : b4[k + 2]; b2[k] = mine + __shfl_xor(other, 32); }
      const int e0 = (h4 ? 4 : 0) + (h5 ? 2 : 0);
      float* const slot = stat + wr * 2 * BN;
      slot[2 * (cl0 + e0) + (h3 ? 1 : 0)] = b2[0];
      slot[2 * (cl0 + e0 + 1) + (h3 ? 1 : 0)] = b2[1];
    }
  } else {
  int64_t rrow[2];
  const float* nbp[2];
  int mrow[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + wr * 64 + i * 32 + l31;
    mrow[i] = m;
    rrow[i] = (int64_t)m * a.ldr;
    if (a.R && a.res_up && m < a.M) {
      const int hw = a.H * a.W;
      const int img = m / hw, rem = m - img * hw;
      const int y = rem / a.W, x = rem - y * a.W;
      rrow[i] = ((int64_t)(img * (a.H >> 1) + (y >> 1)) * (a.W >> 1) + (x >> 1)) * a.ldr;
    }
    nbp[i] = (a.nbias && m < a.M) ? a.nbias + (int64_t)(m / a.hw) * (a.ldnb ? a.ldnb : a.N) : nullptr;
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    float ssum[16], ssq[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { ssum[r] = 0.f; ssq[r] = 0.f; }
    // biases and residual pieces of the block are fetched before its first store: loads inside the store loop cannot be
    // hoisted above the preceding stores (may alias) and serialise one round trip per store (see conv3x3.hip)
    float4 rv[2][4], bv[4], nbv[2][4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int n = n0 + wc * 64 + j * 32 + 4 * lhi + 8 * g;
      bv[g] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (a.bias && n < a.N) bv[g] = *(const float4*)(a.bias + n);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        nbv[i][g] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (nbp[i] && n < a.N) nbv[i][g] = *(const float4*)(nbp[i] + n);
      }
    }
    if (a.R) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const int n = n0 + wc * 64 + j * 32 + 4 * lhi + 8 * g;
          rv[i][g] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (mrow[i] >= a.M || n >= a.N) continue;
          if (a.res_f32) {
            rv[i][g] = *(const float4*)((const float*)a.R + offR + rrow[i] + n);
          } else if (a.split_out) {          // hi words in .x/.y, lo words in .z/.w
            const int po = split_off(n, a.split_out);
            const uint2 rh = *(const uint2*)((const u16*)a.R + offR + rrow[i] + po);
            const uint2 rl = *(const uint2*)((const u16*)a.R + offR + rrow[i] + po + a.split_out);
            rv[i][g].x = __builtin_bit_cast(float, rh.x); rv[i][g].y = __builtin_bit_cast(float, rh.y);
            rv[i][g].z = __builtin_bit_cast(float, rl.x); rv[i][g].w = __builtin_bit_cast(float, rl.y);
          } else {
            const uint2 r = *(const uint2*)((const u16*)a.R + offR + rrow[i] + n);
            rv[i][g].x = __builtin_bit_cast(float, r.x); rv[i][g].y = __builtin_bit_cast(float, r.y);
          }
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int m = mrow[i];
      if (m >= Mr) continue;
      const int64_t mo = orow(m);
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int n = n0 + wc * 64 + j * 32 + 4 * lhi + 8 * g;
        if (n >= a.N) continue;
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = acc[i][j][4 * g + e] * a.alpha;
        v[0] += bv[g].x + nbv[i][g].x; v[1] += bv[g].y + nbv[i][g].y; v[2] += bv[g].z + nbv[i][g].z; v[3] += bv[g].w + nbv[i][g].w;
        if (a.act != PMI_ACT_NONE) act_apply_n<4>(v, a.act);
        if (a.R) {
          if (a.res_f32) {
            v[0] += rv[i][g].x; v[1] += rv[i][g].y; v[2] += rv[i][g].z; v[3] += rv[i][g].w;
          } else {
            const uint32_t r0 = __builtin_bit_cast(uint32_t, rv[i][g].x), r1 = __builtin_bit_cast(uint32_t, rv[i][g].y);
            v[0] += T::to_f((u16)(r0 & 0xffff)); v[1] += T::to_f((u16)(r0 >> 16));
            v[2] += T::to_f((u16)(r1 & 0xffff)); v[3] += T::to_f((u16)(r1 >> 16));
            if (a.split_out) {
              const uint32_t l0 = __builtin_bit_cast(uint32_t, rv[i][g].z), l1 = __builtin_bit_cast(uint32_t, rv[i][g].w);
              v[0] += T::to_f((u16)(l0 & 0xffff)); v[1] += T::to_f((u16)(l0 >> 16));
              v[2] += T::to_f((u16)(l1 & 0xffff)); v[3] += T::to_f((u16)(l1 >> 16));
            }
          }
        }
        if (a.split_out) {
          const int64_t o = offD + (int64_t)m * a.ldd + split_off(n, a.split_out);
          const uint2 hi = pack4<T>(v[0], v[1], v[2], v[3]);
          const float l0 = v[0] - T::to_f((u16)(hi.x & 0xffff)), l1 = v[1] - T::to_f((u16)(hi.x >> 16));
          const float l2 = v[2] - T::to_f((u16)(hi.y & 0xffff)), l3 = v[3] - T::to_f((u16)(hi.y >> 16));
          *(uint2*)((u16*)a.D + o) = hi;
          *(uint2*)((u16*)a.D + o + a.split_out) = pack4<T>(l0, l1, l2, l3);
        } else {
        const int64_t o = offD + mo * a.ldd + n;
        if (a.out_f32) *(float4*)((float*)a.D + o) = make_float4(v[0], v[1], v[2], v[3]);
        else *(uint2*)((u16*)a.D + o) = pack4<T>(v[0], v[1], v[2], v[3]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { ssum[4 * g + e] += v[e]; ssq[4 * g + e] += v[e] * v[e]; }
      }
    }
    if (a.stats) stats_block_to_lds(ssum, ssq, stat + wr * 2 * BN, wc * 64 + j * 32, lane);
  }
  }
  if (a.stats) {
    __syncthreads();
    const int img = m0 / a.hw, prow = (m0 - img * a.hw) / BM;
    float* o = a.stats + ((int64_t)(img * a.stats_p + prow) * a.N + n0) * 2;
    for (int c = tid; c < 2 * BN; c += 256)
      if (n0 + (c >> 1) < a.N) o[c] = stat[c] + stat[2 * BN + c];
  }
#ifdef PMI_STAMPS
  __syncthreads();
  GSTAMP(3);
#endif
}

// sum the split-K slabs and apply the fused epilogue (bias, per-sample bias, activation, residual), 4 channels per thread
template <typename T>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const pmi_igemm_args a) {
  const int n4 = a.N >> 2;
  const int64_t total = (int64_t)a.M * n4;
  const float* ws = (const float*)a.ws;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int m = (int)(i / n4), n = (int)(i - (int64_t)m * n4) * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int z = 0; z < a.splitk; ++z) {
      const float4 p = *(const float4*)(ws + ((int64_t)z * a.M + m) * a.N + n);
      s.x += p.x; s.y += p.y; s.z += p.z; s.w += p.w;
    }
    float v[4] = {s.x * a.alpha, s.y * a.alpha, s.z * a.alpha, s.w * a.alpha};
    if (a.bias) { const float4 b = *(const float4*)(a.bias + n); v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w; }
    if (a.nbias) {
      const float4 b = *(const float4*)(a.nbias + (int64_t)(m / a.hw) * (a.ldnb ? a.ldnb : a.N) + n);
      v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
    }
    if (a.act != PMI_ACT_NONE) act_apply_n<4>(v, a.act);
    if (a.R) {
      int64_t rrow = (int64_t)m * a.ldr;
      if (a.res_up) {
        const int hw = a.H * a.W;
        const int img = m / hw, rem = m - img * hw;
        const int y = rem / a.W, x = rem - y * a.W;
        rrow = ((int64_t)(img * (a.H >> 1) + (y >> 1)) * (a.W >> 1) + (x >> 1)) * a.ldr;
      }
      if (a.res_f32) {
        const float4 r = *(const float4*)((const float*)a.R + rrow + n);
        v[0] += r.x; v[1] += r.y; v[2] += r.z; v[3] += r.w;
      } else {
        const int po = a.split_out ? split_off(n, a.split_out) : n;
        const uint2 r = *(const uint2*)((const u16*)a.R + rrow + po);
        v[0] += T::to_f((u16)(r.x & 0xffff)); v[1] += T::to_f((u16)(r.x >> 16));
        v[2] += T::to_f((u16)(r.y & 0xffff)); v[3] += T::to_f((u16)(r.y >> 16));
        if (a.split_out) {
          const uint2 l = *(const uint2*)((const u16*)a.R + rrow + po + a.split_out);
          v[0] += T::to_f((u16)(l.x & 0xffff)); v[1] += T::to_f((u16)(l.x >> 16));
          v[2] += T::to_f((u16)(l.y & 0xffff)); v[3] += T::to_f((u16)(l.y >> 16));
        }
      }
    }
    if (a.split_out) {
      const int64_t o = (int64_t)m * a.ldd + split_off(n, a.split_out);
      const uint2 hi = pack4<T>(v[0], v[1], v[2], v[3]);
      const float l0 = v[0] - T::to_f((u16)(hi.x & 0xffff)), l1 = v[1] - T::to_f((u16)(hi.x >> 16));
      const float l2 = v[2] - T::to_f((u16)(hi.y & 0xffff)), l3 = v[3] - T::to_f((u16)(hi.y >> 16));
      *(uint2*)((u16*)a.D + o) = hi;
      *(uint2*)((u16*)a.D + o + a.split_out) = pack4<T>(l0, l1, l2, l3);
      continue;
    }
    const int64_t o = (int64_t)m * a.ldd + n;
    if (a.out_f32) *(float4*)((float*)a.D + o) = make_float4(v[0], v[1], v[2], v[3]);
    else *(uint2*)((u16*)a.D + o) = pack4<T>(v[0], v[1], v[2], v[3]);
  }
}

template <typename T>
int launch(const pmi_igemm_args& a, hipStream_t s) {
  const bool phased = a.up == 2;          // Downsample2D adjoint: one grid slice of M / 4 rows per output phase
  const int tiles = (((phased ? a.M / 4 : a.M) + BM - 1) / BM) * ((a.N + BN - 1) / BN);
  const dim3 grid(tiles, phased ? 4 : 1, a.batch > 1 ? a.batch : (a.splitk > 1 ? a.splitk : 1)), block(256);
  const bool conv = a.taps != 1 || a.up || a.stride == 2;
  const int Cin = a.C0 + a.C1;
  const bool kfast = (Cin % BK == 0) && (a.C0 % BK == 0);
  if (phased) {
    if (kfast) hipLaunchKernelGGL((igemm_kernel<T, true, true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((igemm_kernel<T, true, false, true>), grid, block, 0, s, a);
  } else if (conv) {
    if (kfast) hipLaunchKernelGGL((igemm_kernel<T, true, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((igemm_kernel<T, true, false>), grid, block, 0, s, a);
  } else {
    if (kfast) hipLaunchKernelGGL((igemm_kernel<T, false, true>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((igemm_kernel<T, false, false>), grid, block, 0, s, a);
  }
  PMI_CHECK_LAUNCH();
  if (a.splitk > 1) {
    const int64_t work = (int64_t)a.M * (a.N / 4);
    const int blocks = (int)((work + 255) / 256 > 4096 ? 4096 : (work + 255) / 256);
    hipLaunchKernelGGL(splitk_reduce_kernel<T>, dim3(blocks), dim3(256), 0, s, a);
    PMI_CHECK_LAUNCH();
  }
  return PMI_OK;
}

}  // namespace

extern "C" int pmi_conv3x3_halo_config(const pmi_igemm_args* a);
int pmi_conv3x3_halo_launch(const pmi_igemm_args* a, int cfg, void* stream);
int pmi_conv3x3_wd_launch(const pmi_igemm_args* a, int cfg, void* stream);   // conv_wd.hip: tile configs 4, 6
int pmi_conv3x3_up_wd_launch(const pmi_igemm_args* a, void* stream);          // conv_up_wd.hip: tile config 9
extern "C" int pmi_gemm_wd_eligible(const pmi_igemm_args* a);                 // gemm_wd.hip: plain GEMMs with fragment-ordered weights
int pmi_gemm_wd_tile_rows(const pmi_igemm_args* a, int splitk);
int pmi_gemm_wd_launch(const pmi_igemm_args* a, void* stream);
void pmi_conv3x3_allow_wd(int v);
void pmi_conv3x3_wd_mf16(int v);
void pmi_conv3x3_wd128(int v);
void pmi_conv3x3_force_config(int cfg);
void pmi_conv3x3_prefer_256(int v);
static int g_allow_halo = 1;
static int g_wd_max_split = 8;      // A/B switch: pmi_set_option(11, n)
// Split-K factor the generic kernel wants for this shape (1 = none): small-M layers (16x16 / 8x8 feature maps) otherwise
// launch far fewer workgroups than the 256 CUs.  The caller then provides ws = S * M * N floats.
int pmi_conv3x3_wd_splitk(const pmi_igemm_args* a, int cfg);        // conv_wd.hip
extern "C" int pmi_igemm_splitk(const pmi_igemm_args* a) {
  if (a->batch > 1 || (a->N & 3) || a->up == 2) return 1;
  if (g_allow_halo) {
    const int halo = pmi_conv3x3_halo_config(a);
    if (halo >= 0) return pmi_conv3x3_wd_splitk(a, halo);
  }
  if (a->act == PMI_ACT_GEGLU) return 1;
  if (a->A1 && a->taps == 1 && pmi_gemm_wd_eligible(a)) return 1;       // two-source weights-direct GEMM (1x1 skip convolutions): no split-K
  if (pmi_gemm_wd_eligible(a)) {    // weights-direct GEMM: fill the 256 CUs with (row tile x 256-column) workgroups; >= 2 chunks of 128 per split
    const int nch = (a->K + 127) / 128;
    int best = 1;
    long best_cost = -1;
    for (int s = 1; s <= g_wd_max_split && nch / s >= 4; s *= 2) {
      const int rows = pmi_gemm_wd_tile_rows(a, s);
      const long wgs = (long)((a->M + rows - 1) / rows) * (a->N < 256 ? 1 : (a->N + 255) / 256) * s;
      // rounds x rows x (chunks + fixed prologue / epilogue share); a split pays for its fp32 slabs and the reduce launch
      const long cost = ((wgs + 255) / 256) * rows * (nch / s + 6) + (s > 1 ? 8L * 144 : 0);
      if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = s; }
    }
    return best;
  }
  const int tiles = ((a->M + BM - 1) / BM) * ((a->N + BN - 1) / BN);
  const int nk = (a->K + BK - 1) / BK;
  if (tiles >= 384 || nk < 16) return 1;     // 2 workgroups fit per CU: below 384 tiles part of the chip idles through a long K loop
  int s = 512 / tiles;
  if (s > nk / 8) s = nk / 8;
  if (s > 16) s = 16;
  return s < 2 ? 1 : s;
}

int pmi_igemm_halo_allowed(void) { return g_allow_halo; }

extern "C" int pmi_igemm_stats_rows(const pmi_igemm_args* a) {
  if (a->batch > 1 || a->splitk > 1 || a->up == 2) return 0;
  const int halo = g_allow_halo ? pmi_conv3x3_halo_config(a) : -1;
  if (a->split_out) return halo >= 6 ? (a->H / 8) * (a->W / 32) : 0;    // split outputs: the weights-direct conv3x3 epilogue only (the generic kernel takes none)
  if (halo == 3) return 0;                                             // few-output-channel config: no statistics epilogue
  if (halo >= 0) return (a->H / (halo == 1 ? 16 : 8)) * (a->W / 32);   // configs 0, 2: 8-row tiles
  if (a->hw > 0 && (a->hw % BM) == 0 && (a->M % a->hw) == 0) return a->hw / BM;
  return 0;
}

void pmi_attn_flash_qt(int v);     // attn_flash.hip
void pmi_attn_flash_kv_chunks(int v);
void pmi_conv3x3_wd_splitk_enable(int v);   // conv_wd.hip
void pmi_gemm_wd_few_wgs(int v);            // gemm_wd.hip
void pmi_conv3x3_wd_smallc(int v);          // conv3x3.hip
void pmi_conv3x3_up_phase(int v);
void pmi_conv3x3_skip_enable(int v);
void pmi_vit_attn_lds(int v);               // attn.hip

extern "C" int pmi_set_option(int key, int value) {
  if (key == 0) { const int old = g_allow_halo; g_allow_halo = value; return old; }
  if (key == 1) { pmi_conv3x3_force_config(value); return 0; }
  if (key == 2) { pmi_conv3x3_prefer_256(value); return 0; }
  if (key == 6) { pmi_conv3x3_allow_wd(value); return 0; }
  if (key == 7) { pmi_conv3x3_wd_mf16(value); return 0; }
  if (key == 8) { pmi_conv3x3_wd128(value); return 0; }
  if (key == 9) { pmi_attn_flash_qt(value); return 0; }
  if (key == 10) { pmi_conv3x3_wd_splitk_enable(value); return 0; }
  if (key == 11) { g_wd_max_split = value; return 0; }
  if (key == 12) { pmi_gemm_wd_few_wgs(value); return 0; }
  if (key == 13) { pmi_conv3x3_wd_smallc(value); return 0; }
  if (key == 14) { pmi_attn_flash_kv_chunks(value); return 0; }
  if (key == 15) { pmi_conv3x3_up_phase(value); return 0; }
  if (key == 16) { pmi_conv3x3_skip_enable(value); return 0; }
  if (key == 17) { pmi_vit_attn_lds(value); return 0; }
  return PMI_ERR_ARG;
}

// PMI_DEBUG=1 in the environment: name the argument check that rejected a call
static int bad_arg(int line) {
  if (getenv("PMI_DEBUG")) fprintf(stderr, "pmi_igemm: argument check at igemm.hip:%d failed\n", line);
  return PMI_ERR_ARG;
}

extern "C" int pmi_igemm(const pmi_igemm_args* a, pmi_stream_t stream) {
  if (!a || !a->A0 || !a->B || !a->D) return bad_arg(__LINE__);
  if (a->M <= 0 || a->N <= 0 || a->K <= 0) return bad_arg(__LINE__);
  if ((a->K & 7) || (a->C0 & 7) || (a->C1 & 7)) return bad_arg(__LINE__);
  // a ragged N (attention scores) is allowed when the 4-wide epilogue vectors stay inside the row pitch
  if ((a->N & 3) && (a->bias || a->nbias || a->R || a->ldd < ((a->N + 3) & ~3))) return bad_arg(__LINE__);
  if ((a->lda0 & 7) || (a->ldb & 7) || (a->ldd & 3)) return bad_arg(__LINE__);
  if (a->C1 > 0 && (!a->A1 || (a->lda1 & 7))) return bad_arg(__LINE__);
  if (a->taps != 1 && a->taps != 9 && a->taps != 16) return bad_arg(__LINE__);
  // taps 16: the 4x4 stride-2 window of the Upsample2D adjoint (rows / columns 2y-1 .. 2y+2 of the high-resolution gradient)
  if (a->taps == 16 && (a->stride != 2 || a->up || a->res_up || a->Hin != 2 * a->H || a->Win != 2 * a->W)) return bad_arg(__LINE__);
  if (a->stride != 1 && a->stride != 2) return bad_arg(__LINE__);
  // up 2: the Downsample2D adjoint by output phase (taps 9 on phase-packed weights, stride 2 = the forward's): one source, M = images x 2Hin x 2Win,
  // and nothing in the epilogue that is indexed by the GEMM row (residual, per-sample bias, statistics, split outputs); no split-K, no batch
  if (a->up == 2 && (a->taps != 9 || a->stride != 2 || a->res_up || a->A1 || a->C1 || a->R || a->nbias || a->stats || a->splitk > 1 || a->batch > 1 ||
                     a->split_out || a->split_in || a->pro_a || a->D2 || a->aux || a->dtype == PMI_DT_F16X2 || (a->M & 3))) return bad_arg(__LINE__);
  if (a->K != a->taps * (a->C0 + a->C1)) return bad_arg(__LINE__);
  if (a->R && (a->ldr & 3)) return bad_arg(__LINE__);
  // (split_out: the group width ops.split_group gives a tensor of N channels -- 32, or N itself for 8 / 16 / 24; the epilogues write 4-channel
  // runs at split_off(n, G), which never straddle a group for G % 4 == 0)
  if (a->split_out && ((a->split_out & 7) || a->split_out > 32 || a->out_f32 || (a->N % a->split_out) || a->batch > 1)) return bad_arg(__LINE__);
  if ((unsigned)a->split_in > 2u) return bad_arg(__LINE__);
  // (a fused prologue over split tensors and the single-operand form split_in = 2 exist in the weights-direct conv3x3 configs only: the
  // check behind the config query below rejects every other route)
  if (a->split_in == 2 && !a->split_out) return bad_arg(__LINE__);
  if (a->nbias && a->hw <= 0) return bad_arg(__LINE__);
  const bool conv = a->taps != 1 || a->up || a->stride == 2;
  if (a->res_up && ((a->H & 1) || (a->W & 1))) return bad_arg(__LINE__);
  if ((conv || a->res_up) && (a->H <= 0 || a->W <= 0 || a->Hin <= 0 || a->Win <= 0 || a->M % (a->H * a->W))) return bad_arg(__LINE__);
  if (a->up && (a->H != 2 * a->Hin || a->W != 2 * a->Win)) return bad_arg(__LINE__);
  if (a->batch > 1 && a->batch_inner <= 0) return bad_arg(__LINE__);
  const int halo = g_allow_halo ? pmi_conv3x3_halo_config(a) : -1;
  if (a->pro_a && (!a->pro_b || halo < 0)) return PMI_ERR_ARG;
  if ((a->split_in == 2 || ((a->split_in || a->split_out) && a->pro_a) || (a->split_out && a->R && a->res_f32)) && halo < 6) return bad_arg(__LINE__);
  if (a->stats && a->stats_p != pmi_igemm_stats_rows(a)) return PMI_ERR_ARG;
  if (a->splitk > 1 && (!a->ws || a->batch > 1 || (halo >= 0 && a->splitk != pmi_conv3x3_wd_splitk(a, halo)) || (a->N & 3) || a->stats)) return PMI_ERR_ARG;
  if (a->act == PMI_ACT_GEGLU && !pmi_gemm_wd_eligible(a)) return bad_arg(__LINE__);     // the gated epilogue exists in the weights-direct GEMM only
  if ((a->D2 || a->aux) && !pmi_gemm_wd_eligible(a)) return bad_arg(__LINE__);           // so do the second output / activation-gradient epilogues: no other kernel would honour them
  if (pmi_gemm_wd_eligible(a) && !((a->nbias || a->res_up) && a->splitk <= 1)) {      // (a per-sample bias / up-sampled residual needs the reduce kernel: split-K only)
    const int rc = pmi_gemm_wd_launch(a, stream);
    if (rc != PMI_OK || a->splitk <= 1 || a->reserved3 == 1) return rc;      // reserved3 = 1: the caller consumes the raw slabs (fused reduce + LayerNorm)
    hipStream_t s = (hipStream_t)stream;             // split-K: the slabs get bias / activation / residual in the reduce kernel
    const int64_t work = (int64_t)a->M * (a->N / 4);
    const int blocks = (int)((work + 255) / 256 > 4096 ? 4096 : (work + 255) / 256);
    if (a->dtype == PMI_DT_BF16) hipLaunchKernelGGL(splitk_reduce_kernel<BF16>, dim3(blocks), dim3(256), 0, s, *a);
    else hipLaunchKernelGGL(splitk_reduce_kernel<F16>, dim3(blocks), dim3(256), 0, s, *a);
    PMI_CHECK_LAUNCH();
    return PMI_OK;
  }
  if (halo == 9) return pmi_conv3x3_up_wd_launch(a, stream);
  if (halo >= 4) {
    const int rc = pmi_conv3x3_wd_launch(a, halo, stream);
    if (rc != PMI_OK || a->splitk <= 1) return rc;
    hipStream_t s = (hipStream_t)stream;             // split-K: bias / per-sample bias / activation / residual in the reduce kernel
    const int64_t work = (int64_t)a->M * (a->N / 4);
    const int blocks = (int)((work + 255) / 256 > 4096 ? 4096 : (work + 255) / 256);
    if (a->dtype == PMI_DT_BF16) hipLaunchKernelGGL(splitk_reduce_kernel<BF16>, dim3(blocks), dim3(256), 0, s, *a);
    else hipLaunchKernelGGL(splitk_reduce_kernel<F16>, dim3(blocks), dim3(256), 0, s, *a);
    PMI_CHECK_LAUNCH();
    return PMI_OK;
  }
  if (halo >= 0) return pmi_conv3x3_halo_launch(a, halo, stream);
  hipStream_t s = (hipStream_t)stream;
  return a->dtype == PMI_DT_BF16 ? launch<BF16>(*a, s) : launch<F16>(*a, s);
}

extern "C" int pmi_abi_version(void) { return 1; }
