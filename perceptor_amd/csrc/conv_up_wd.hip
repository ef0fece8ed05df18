// conv3x3 over a nearest-x2 up-sampled input, by output phase, for gfx950 MFMA (tile config 9) -- the up-sampling ResBlocks' first convolution.
//
// A 3x3 convolution over nearest-x2(x) is four 2x2 convolutions over x itself, one per output parity (a, b): output pixel (2y + a, 2x + b)
// reads the low-resolution rows y + a - 1 + u, u = 0, 1, and columns x + b - 1 + v, v = 0, 1, against sums of the original taps (rows: a = 0:
// w0 | w1 + w2, a = 1: w0 + w1 | w2; the same for the columns; engine/ops.py PackedLinear.frag16_up sums them in fp32 and rounds once).
// That is 16 tap products per low-resolution pixel instead of the 36 that conv_wd.hip's gather route multiplies (its 10 x 34 high-resolution
// patch holds every low-resolution pixel up to four times, each copy through the GroupNorm + SiLU prologue): 4/9 of the MFMAs, a quarter of
// the prologue evaluations per output pixel.  Zero padding where the LOW-resolution index leaves the image is the high-resolution padding.
//
// The kernel is conv_wd.hip's 256-channel 16x16x32 tile (config 6) with that reduction; what is said there about the weight stream, the LDS
// patch layout, the staging plan and the epilogue holds here.  A 512-thread workgroup owns 8 x 32 LOW-resolution positions x one phase x 256
// output channels (wave: 256 positions x 32 channels, 128 accumulator registers).  Per 64-channel chunk the 9 x 33 low-resolution patch this
// phase reads (origin (y0 - 1 + a, x0 - 1 + b): fragment addresses carry no phase term) is staged once, double-buffered, one barrier per chunk.
// A chunk is 8 groups (dx, 32-channel step, half-row) with the two dy taps innermost: 8 rows x 2 taps x 2 channel blocks = 32 MFMAs on 9
// fragment rows; the weights of a (dx, step) pair are 4 fragments (4 KB per wave) in a two-slot ring.
// Workgroup order: phase fastest, then the channel tile, inside xcd_remap -- the four phases of a tile read (nearly) the same patch from one
// XCD's L2.  Grid = images x low-resolution tiles x 4 x Cout / 256: the gather route's workgroup count.
//
// One source, prologue none / GroupNorm-apply + activation, bias and per-sample bias, 16-bit plain output, fused output statistics: partial row
// (low-resolution tile, phase) -> 4 (ty tiles_x + tx) + phase of the (H / 8)(W / 32) rows per image the gather route writes as well.
#include "common.h"
#include "../../include/perceptor_hip.h"

#ifndef UP_FINE
#define UP_FINE 2    // staging VALU instructions the scheduler is asked to place behind each MFMA of a store-slot group (conv_wd.hip: WD_FINE)
#endif
#ifndef UP_FROW
#define UP_FROW 1    // first output row of a store-slot group that takes staging VALU (the coefficient reads issued at the group's top land under row 0)
#endif

namespace {

constexpr int PW = 33, PR = 9;

template <typename T, int PRO>
__global__ __launch_bounds__(512, 2) void conv3x3_up_wd_kernel(const pmi_igemm_args a) {
  constexpr int NW = 8, NT = 512, CK = 64, KS = 2;
  constexpr int PP = PR * PW;                          // patch pixels (297)
  constexpr int CPR = CK / 8;                          // 16-byte staging units per patch pixel
  constexpr int NG = 2 * KS * 2;                       // groups per chunk: 2 dx x k-steps x 2 half-rows
  constexpr int WGC = 2 * KS;                          // weight groups per chunk
  constexpr int NWF = 4;                               // fragments per weight group: 2 dy x 2 channel blocks
  constexpr int GB = NWF * 1024;
  constexpr int NPI = (PP * CPR + NT - 1) / NT;        // staging pieces per thread per chunk (5)
  constexpr int ROW = CK * 2 + 32;                     // patch row pitch (160 B): conflict-free b128 fragment reads
  constexpr int PATCH_BYTES = (NPI * NT / CPR) * ROW;  // padded to whole staging passes
  constexpr int BN = 256, NPX = 256;
  constexpr int SROW = BN * 2 + 16;
  constexpr int EPI_BYTES = NPX * SROW + NW * BN * 8 + BN * 4;
  constexpr int MAXCIN = 2048;
  constexpr int CTAB = MAXCIN + 8;                     // + a unit of eight zeros for padding pixels
  constexpr int COEF_BYTES = PRO ? 2 * CTAB * 4 : 0;
  constexpr int PPIX_BYTES = NPI * NT * 4;
  static_assert(NPI <= NG - 1, "the next patch must be complete before the barrier in the chunk's last group");
  constexpr int BSM_OFF = (2 * PATCH_BYTES + COEF_BYTES + PPIX_BYTES) > (EPI_BYTES - BN * 4) ? (2 * PATCH_BYTES + COEF_BYTES + PPIX_BYTES) : (EPI_BYTES - BN * 4);
  static_assert(BSM_OFF + BN * 4 <= 160 * 1024, "LDS budget");
  // the farthest fragment read: lane 63, last group, row 8
  static_assert(15 * ROW + 48 + 16 + (ROW + 64 + 16 * ROW) + 8 * PW * ROW <= PATCH_BYTES, "fragment reads stay inside a patch buffer");
  __shared__ __attribute__((aligned(16))) char smem[BSM_OFF + BN * 4];
  float* const bsm = (float*)(smem + BSM_OFF);
  float* const coef = (float*)(smem + 2 * PATCH_BYTES);
  int* const ppix_s = (int*)(smem + 2 * PATCH_BYTES + COEF_BYTES);

  const int tid = threadIdx.x, lane = tid & 63;
  if (PRO && tid < 16) coef[(tid >> 3) * CTAB + MAXCIN + (tid & 7)] = 0.f;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wn = wid;

  const int tiles_x = a.Win / 32, tiles_y = a.Hin / 8, tiles_n = a.N / BN;
  const int nimg = a.M / (a.H * a.W);
  int logical = xcd_remap(blockIdx.x, nimg * tiles_y * tiles_x * tiles_n * 4);
  const int phase = logical & 3; logical >>= 2;
  const int tn = logical % tiles_n; logical /= tiles_n;
  const int tx = logical % tiles_x; logical /= tiles_x;
  const int ty = logical % tiles_y;
  const int img = logical / tiles_y;
  const int pa = phase >> 1, pb_ = phase & 1;
  const int y0 = ty * 8, x0 = tx * 32, n0 = tn * BN;    // low-resolution tile origin

#ifdef PMI_STAMPS   // tools/conv_probe.py --stamps
#define STAMP(k) do { if (tid == 0 && a.ws) ((long long*)a.ws)[(int64_t)blockIdx.x * 8 + (k)] = (long long)wall_clock64(); } while (0)
#else
#define STAMP(k) do {} while (0)
#endif
  STAMP(0);
  const int Cin = a.C0;
  const int nchunks = Cin / CK;
  const int sc = tid % CPR;
  const int64_t img_px = (int64_t)a.Hin * a.Win;
  const u16* const A0i = (const u16*)a.A0 + (int64_t)img * img_px * a.lda0;
  const __amdgpu_buffer_rsrc_t rs_a = make_rsrc(A0i, ((img_px - 1) * a.lda0 + a.C0) * 2);
  const uint32_t ld2 = (uint32_t)a.lda0 * 2u;
  // this wave's weight stream: [phase][chunk][dx][step][dy][16-channel block][lane][8] 16-bit, contiguous in loop order
  const int64_t wslab = (int64_t)nchunks * WGC * GB;
  const __amdgpu_buffer_rsrc_t rsrc_w = make_rsrc((const char*)a.Bf + ((int64_t)(tn * NW + wn) * 4 + phase) * wslab, wslab);
  const uint32_t wvo = (uint32_t)lane * 16u;

  // ---- staging plan: source pixel per staged piece, -1 = zero padding (outside the LOW-resolution image) ----
#pragma unroll
  for (int i = 0; i < NPI; ++i) {
    const int pp = tid / CPR + (NT / CPR) * i;
    const int py = pp / PW, px = pp - py * PW;
    const int sy = y0 - 1 + pa + py, sx = x0 - 1 + pb_ + px;
    const bool inside = pp < PP && (unsigned)sy < (unsigned)a.Hin && (unsigned)sx < (unsigned)a.Win;
    ppix_s[i * NT + tid] = inside ? sy * a.Win + sx : -1;
  }

  auto load_piece = [&](int chunk, int pix, bool live) -> uint4 {       // !live: out-of-range offset, zeros, no traffic, no branch
    const uint32_t vo = (pix >= 0 && live) ? (uint32_t)pix * ld2 + (uint32_t)sc * 16u : PMI_BUF_OOB;
    return buf_load16(rs_a, vo, (uint32_t)(chunk * CK) * 2u);
  };
  // (conv_wd.hip: a padding unit reads zero coefficients, act(0 * 0 + 0) = 0; SiLU on coefficients pre-scaled by -log2(e) in five instructions)
  constexpr bool PSILU = PRO == 1 + PMI_ACT_SILU;
  constexpr float NLOG2E = -1.4426950408889634f;
  auto read_coef = [&](int chunk, int pix, float* ga, float* gb) {
    const float* ca = coef + (pix >= 0 ? chunk * CK + sc * 8 : MAXCIN);
    *(float4*)ga = *(const float4*)ca; *(float4*)(ga + 4) = *(const float4*)(ca + 4);
    *(float4*)gb = *(const float4*)(ca + CTAB); *(float4*)(gb + 4) = *(const float4*)(ca + CTAB + 4);
  };
  auto cvt_piece = [&](uint4 pc, int pix, const float* ga, const float* gb, bool mask) -> uint4 {
    if (!PRO) return pc;
    float f[8];
    unpack8<T>(pc, f);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      if constexpr (PSILU) {
        const float u = __builtin_fmaf(f[e], ga[e], gb[e]);
        f[e] = u * __builtin_amdgcn_rcpf(__builtin_fmaf(__builtin_amdgcn_exp2f(u), NLOG2E, NLOG2E));
      } else {
        f[e] = act_apply(f[e] * ga[e] + gb[e], PRO - 1);
      }
    }
    const uint32_t keep = (!mask || pix >= 0) ? 0xffffffffu : 0u;     // the first patch shares one coefficient read between its units: padding masked here
    uint4 v = pack8<T>(f);
    v.x &= keep; v.y &= keep; v.z &= keep; v.w &= keep;
    return v;
  };
  auto write_piece = [&](char* pbuf, int i, const uint4& o) {
    *(uint4*)(pbuf + (tid / CPR) * ROW + sc * 16 + i * (NT / CPR) * ROW) = o;
  };

  f32x4 acc4[8][2][2];                                  // [row][half-row][16-channel block]
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc4[i][(r >> 3) & 1][(r >> 2) & 1][r & 3] = 0.f;

  for (int c = tid; c < BN; c += NT) {                  // (made visible by the prologue's barrier)
    const int n = n0 + c;
    float b = 0.f;
    if (a.bias) b = a.bias[n];
    if (a.nbias) b += a.nbias[(int64_t)img * (a.ldnb ? a.ldnb : a.N) + n];
    bsm[c] = b;
  }

  uint4 wq[2][NWF];                                     // [ring slot][dy x channel block]
  auto load_wg = [&](int slot, int group) {             // groups past the end fall outside the resource: zeros
    const uint32_t vo = wvo + (uint32_t)group * (uint32_t)GB;
#pragma unroll
    for (int f = 0; f < NWF; ++f) wq[slot][f] = buf_load16(rsrc_w, vo + f * 1024u, 0);
  };

  // ---- prologue: patch of chunk 0, the first weight group ----
  load_wg(0, 0);
  {
    uint4 p0[NPI];
    float ga[8], gb[8];
#pragma unroll
    for (int i = 0; i < NPI; ++i) p0[i] = load_piece(0, ppix_s[i * NT + tid], true);
    if (PRO) {
      for (int c = tid; c < Cin; c += NT) {
        coef[c] = a.pro_a[(int64_t)img * Cin + c] * (PSILU ? NLOG2E : 1.f);
        coef[CTAB + c] = a.pro_b[(int64_t)img * Cin + c] * (PSILU ? NLOG2E : 1.f);
      }
      __syncthreads();
      read_coef(0, 0, ga, gb);
    }
#pragma unroll
    for (int i = 0; i < NPI; ++i) write_piece(smem, i, cvt_piece(p0[i], ppix_s[i * NT + tid], ga, gb, true));
  }
  __syncthreads();
  STAMP(1);

  const int frag0 = (lane & 15) * ROW + (lane >> 4) * 16;
  auto goff = [&](int g) -> int { const int q = g >> 1, s = g & 1; return (q / KS) * ROW + (q % KS) * 64 + s * 16 * ROW; };
  // Six fragment registers as a rolling window over the 9 patch rows of a group: row i's MFMAs need rows i and i + 1; once they have issued,
  // row i's register is reloaded -- with row i + 6 of this group (i < 3) or with row i - 3 of the NEXT group (i = 3 .. 7; after the last
  // output row, row 8's register takes the next group's row 5 as well).  Row r of group g therefore sits in register (r + 3 g) % 6; 3 NG is a
  // multiple of 6, so the map repeats per chunk and every index is a compile-time constant.  The chunk's barrier sits in its last group
  // between output rows 2 and 3: the wave's last reads of the current buffer in front of it, the prefetch from the other buffer behind it.
  static_assert((3 * NG) % 6 == 0, "fragment window must repeat per chunk");
  uint4 xf[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) xf[r] = *(const uint4*)(smem + frag0 + r * PW * ROW);
  int pixc = ppix_s[0 * NT + tid];
  uint4 pr = load_piece(nchunks > 1 ? 1 : 0, pixc, nchunks > 1);       // piece 0 of the second chunk's patch
  int pixn = ppix_s[1 * NT + tid];
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    const char* const pb = smem + (chunk & 1) * PATCH_BYTES;
    char* const pn = smem + ((chunk + 1) & 1) * PATCH_BYTES;
    const bool more = chunk + 1 < nchunks;              // past the end the staging runs on zeros into the unused buffer (no branches around loads)
    const int cn = more ? chunk + 1 : chunk;
    const bool more2 = chunk + 2 < nchunks;
    const int cn2 = more2 ? chunk + 2 : chunk;
    const int gbase = chunk * WGC;
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      if (g & 1) load_wg(((g >> 1) + 1) & 1, gbase + (g >> 1) + 1);     // the next (dx, step) pair's weights, in the pair's second group
      const bool store_slot = g < NPI;                  // stores piece g from `pr`, loaded a slot earlier
      const int lp = (g + 1 == NG) ? 0 : g + 1;         // piece whose load is issued in this group
      const bool load_slot = (g + 1 == NG) || lp < NPI;
      float ga[8], gb[8];
      if (PRO && store_slot) read_coef(cn, pixc, ga, gb);
      uint4 prn = pr;
      int pixl = pixc;
      if (load_slot) { prn = load_piece(lp == 0 ? cn2 : cn, pixn, lp == 0 ? more2 : more); pixl = pixn; }
      __builtin_amdgcn_sched_barrier(0);   // keep the global loads in front of the MFMAs
      uint4 po;
      if (store_slot) {
        if (PRO) po = cvt_piece(pr, pixc, ga, gb, false);
        else write_piece(pn, g, pr);
      }
      const char* const cb0 = pb + frag0 + goff(g);
      const char* const nb = (g + 1 < NG ? pb : pn) + frag0 + goff((g + 1) % NG);
      auto rows = [&](int i0, int i1) {
#pragma unroll
        for (int i = i0; i < i1; ++i) {
#pragma unroll
          for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
              acc4[i][g & 1][cb] = T::mfma16(wq[(g >> 1) & 1][dy * 2 + cb], xf[(i + dy + 3 * g) % 6], acc4[i][g & 1][cb]);
          if (i < 3) xf[(i + 3 * g) % 6] = *(const uint4*)(cb0 + (i + 6) * PW * ROW);
          else if (i < 7) xf[(i + 3 * g) % 6] = *(const uint4*)(nb + (i - 3) * PW * ROW);
          else {
            xf[(7 + 3 * g) % 6] = *(const uint4*)(nb + 4 * PW * ROW);
            xf[(8 + 3 * g) % 6] = *(const uint4*)(nb + 5 * PW * ROW);
          }
        }
#pragma unroll
        for (int i = i0; i < i1; ++i) {
          if (UP_FINE && PRO && store_slot && i >= UP_FROW) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
              __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
              __builtin_amdgcn_sched_group_barrier(0x002, UP_FINE, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
          } else {
            __builtin_amdgcn_sched_group_barrier(0x008, 4, 0);   // the MFMAs of output row i
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);   // reload the freed fragment register
          }
        }
      };
      if (g == NG - 1) {
        rows(0, 3);
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
        __builtin_amdgcn_sched_barrier(0);
        rows(3, 8);
      } else {
        rows(0, 8);
      }
      __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);                // row 8's register was freed by the last output row as well
      if (PRO && store_slot) write_piece(pn, g, po);                    // behind the rows: a write in front would hold every fragment read behind it
      int pixn2 = pixn;
      if (load_slot) pixn2 = ppix_s[((lp + 1) % NPI) * NT + tid];
      pr = prn; pixc = pixl; pixn = pixn2;
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  STAMP(2);

  // ---- epilogue: the whole tile goes through LDS once and leaves as full pixel rows (512 contiguous bytes) at (2y + a, 2x + b) ----
  char* const stg = smem;
  float* const stat = (float*)(smem + NPX * SROW);     // [NW][BN][2] (sum, sumsq) partials per write-out wave, summed in a fixed order
  constexpr int LPR = BN / 8;                          // lanes per output pixel row (32)
  constexpr int PPI = 64 / LPR;                        // pixels per store instruction (2)
  constexpr int PXW = NPX / NW;                        // pixels written out by a wave (32: one low-resolution row)
  constexpr int NWI = PXW / PPI;                       // store instructions per wave (16)
  const int q = lane % LPR, psub = lane / LPR;
  const int cl0 = q * 8;
  const __amdgpu_buffer_rsrc_t rs_d = make_rsrc((u16*)a.D + (int64_t)img * a.H * a.W * a.ldd, ((int64_t)(a.H * a.W - 1) * a.ldd + a.N) * 2);
  const uint32_t dvo = (uint32_t)(psub * 2 * a.ldd + n0 + cl0) * 2u;     // the instruction's second pixel: two output columns on
  // (no barrier here: the bias table is the prologue's, and the main loop's last barrier already freed the patch buffers)
  {
    float4 bb[2];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb) bb[cb] = *(const float4*)(bsm + wn * 32 + cb * 16 + 4 * (lane >> 4));
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int sx = 0; sx < 2; ++sx)
#pragma unroll
        for (int cb = 0; cb < 2; ++cb) {
          const int cl = wn * 32 + cb * 16 + 4 * (lane >> 4);
          const float4 b = bb[cb];
          const f32x4 c = acc4[i][sx][cb];
          *(uint2*)(stg + (i * 32 + sx * 16 + (lane & 15)) * SROW + cl * 2) =
              pack4<T>(c[0] * a.alpha + b.x, c[1] * a.alpha + b.y, c[2] * a.alpha + b.z, c[3] * a.alpha + b.w);
        }
  }
  __syncthreads();
  STAMP(6);
  float cs[16];                                        // [0..7] sums, [8..15] sums of squares of this lane's 8 channels
#pragma unroll
  for (int e = 0; e < 16; ++e) cs[e] = 0.f;
  const uint32_t orow = (uint32_t)((2 * (y0 + wid) + pa) * a.W + 2 * x0 + pb_);     // a wave writes out low-resolution row wid of the tile
#pragma unroll
  for (int t = 0; t < NWI; ++t) {
    const int p = wid * PXW + t * PPI + psub;
    const uint4 v = *(const uint4*)(stg + p * SROW + cl0 * 2);
    if (a.stats) {
      float f[8];
      unpack8<T>(v, f);
#pragma unroll
      for (int e = 0; e < 8; ++e) { cs[e] += f[e]; cs[8 + e] += f[e] * f[e]; }
    }
    buf_store16_nt(v, rs_d, dvo, (orow + (uint32_t)(2 * t * PPI)) * (uint32_t)a.ldd * 2u);
  }
  STAMP(7);
  if (a.stats) {
#pragma unroll
    for (int e = 0; e < 16; ++e) cs[e] += __shfl_xor(cs[e], 32);
    if (lane < LPR) {
      float* const slot = stat + (wid * BN + cl0) * 2;
#pragma unroll
      for (int e = 0; e < 8; ++e) { slot[2 * e] = cs[e]; slot[2 * e + 1] = cs[8 + e]; }
    }
    __syncthreads();
    float* o = a.stats + (((int64_t)img * a.stats_p + (ty * tiles_x + tx) * 4 + phase) * a.N + n0) * 2;
    for (int c = tid; c < 2 * BN; c += NT) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < NW; ++w) v += stat[w * 2 * BN + c];
      o[c] = v;
    }
  }
#ifdef PMI_STAMPS
  __syncthreads();
  STAMP(3);
  STAMP(4);
#endif
}

template <typename T>
int launch_t(const pmi_igemm_args& a, hipStream_t s) {
  const dim3 grid((a.M / (a.H * a.W)) * (a.Hin / 8) * (a.Win / 32) * 4 * (a.N / 256));
  if (!a.pro_a) hipLaunchKernelGGL((conv3x3_up_wd_kernel<T, 0>), grid, dim3(512), 0, s, a);
  else if (a.pro_act == PMI_ACT_SILU) hipLaunchKernelGGL((conv3x3_up_wd_kernel<T, 1 + PMI_ACT_SILU>), grid, dim3(512), 0, s, a);
  else if (a.pro_act == PMI_ACT_RELU) hipLaunchKernelGGL((conv3x3_up_wd_kernel<T, 1 + PMI_ACT_RELU>), grid, dim3(512), 0, s, a);
  else if (a.pro_act == PMI_ACT_NONE) hipLaunchKernelGGL((conv3x3_up_wd_kernel<T, 1 + PMI_ACT_NONE>), grid, dim3(512), 0, s, a);
  else return PMI_ERR_ARG;
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

}  // namespace

// Tile config 9 (pmi_conv3x3_halo_config): Bf = [N/32][phase 2a + b][Cin/64][dx][2][dy][2][64 lanes][8], the phase weights of PackedLinear.frag16_up
int pmi_conv3x3_up_wd_launch(const pmi_igemm_args* a, void* stream) {
  if (!a->Bf || a->up != 1 || a->taps != 9 || a->stride != 1 || a->A1 || a->C1 || a->R || a->split_in || a->split_out || a->out_f32 || a->splitk > 1 ||
      a->act != PMI_ACT_NONE || (a->N % 256) || (a->C0 % 64) || (a->Win % 32) || (a->Hin % 8) || a->H != 2 * a->Hin || a->W != 2 * a->Win ||
      (a->pro_a && a->C0 > 2048))
    return PMI_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  return a->dtype == PMI_DT_BF16 ? launch_t<BF16>(*a, s) : launch_t<F16>(*a, s);
}
