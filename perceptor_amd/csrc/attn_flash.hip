// Flash-style attention for head dims 8..160 (multiples of 8) with a separate key / value sequence, on gfx950 MFMA (32x32x16).
// The StableDiffusion transformer blocks: self-attention over 4096 / 1024 / 256 / 64 latent pixels with 40 / 80 / 160-channel heads and
// cross-attention onto the 77 prompt tokens (perceptor/models/stable_diffusion/attention.py:268-298; the xformers call at :285).
//
// Same scheme as attn.hip's 64-channel kernel, generalised:
//   S^T[s][t] = sum_c K[s][c] Q[t][c]   (A = K rows, B = Q rows; KQ = ceil(d / 16) k-steps, channels zero-padded)
//   online softmax over s lane-local (+ one exchange with lane^32), in the exp2 domain (scale * log2 e folded into one multiply)
//   O^T[c][t] += V^T[c][s] P^T[s][t]    (A = V^T rows in DB = ceil(d / 32) blocks, B = the P accumulator re-used in place)
// One wave owns QT x 32 queries (QT = 1 by default; with QT = 2 every K / V^T fragment streamed from L2 feeds two MFMAs, but the
// 204 VGPRs leave one wave per SIMD and it measured slower: kept as an A/B option, pmi_set_option(9, 2)).
// No score matrix in HBM (the batched-GEMM path wrote T x T fp32 scores and 16-bit probabilities: 0.8 GB per sample at T = 4096).
#include "common.h"
#include "../../include/perceptor_hip.h"

namespace {

// Q / K fragments: element (t, c) of a 32-token block at [block][kk = c / 16][lhi = (c / 8) & 1][t & 31][c & 7]
__device__ __forceinline__ int64_t rfrag_g(int64_t blk, int KQ, int kk, int lhi, int l31) {
  return (((blk * KQ + kk) * 2 + lhi) * 32 + l31) * 8;
}
// V^T fragments: [block][ks (2)][db (DB)][lhi][c & 31][8 tokens {16 ks + 4 lhi + 0..3, 16 ks + 8 + 4 lhi + 0..3}]
__device__ __forceinline__ int64_t tfrag_g(int64_t blk, int DB, int ks, int db, int lhi, int l31) {
  return ((((blk * 2 + ks) * DB + db) * 2 + lhi) * 32 + l31) * 8;
}

// rows of src ([N][T][ld], head h at channel offset h*d) -> fragment order; zero fill for t >= T and c >= d
template <bool TRANSPOSED>
__device__ __forceinline__ void split_block(const u16* __restrict__ src, int ld, u16* __restrict__ dst, int n, int h, int bh, int tb,
                                            int T, int ntb, int d, int KQ, int DB, u16 (*sv)[168]) {
  const int tid = threadIdx.x, row = tid >> 3, ch = tid & 7, t = tb * 32 + row;
  const int64_t blk = (int64_t)bh * ntb + tb;
  const u16* r = src + ((int64_t)n * T + t) * ld + h * d;
  if constexpr (!TRANSPOSED) {
    for (int c8 = ch; c8 < 2 * KQ; c8 += 8) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (t < T && c8 * 8 < d) v = *(const uint4*)(r + c8 * 8);
      *(uint4*)(dst + rfrag_g(blk, KQ, c8 >> 1, c8 & 1, row)) = v;
    }
  } else {
    for (int c8 = ch; c8 < 4 * DB; c8 += 8) {
      uint4 v = make_uint4(0, 0, 0, 0);
      if (t < T && c8 * 8 < d) v = *(const uint4*)(r + c8 * 8);
      *(uint4*)(&sv[row][c8 * 8]) = v;
    }
    __syncthreads();
    for (int i = tid; i < DB * 128; i += 256) {
      const int c = i >> 2, fks = (i >> 1) & 1, flhi = i & 1;
      u16 e[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) e[j] = sv[16 * fks + 4 * flhi + (j & 3) + 8 * (j >> 2)][c];
      *(uint4*)(dst + tfrag_g(blk, DB, fks, c >> 5, flhi, c & 31)) =
          make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void flash_split_kernel(const u16* __restrict__ q, int ldq, const u16* __restrict__ k, const u16* __restrict__ v,
                                                          int ldkv, u16* __restrict__ qf, u16* __restrict__ kf, u16* __restrict__ vtf,
                                                          int T, int Tk, int heads, int d, int KQ, int DB) {
  __shared__ u16 sv[32][168];
  const int tb = blockIdx.x, bh = blockIdx.y, n = bh / heads, h = bh - n * heads;
  const int ntq = (T + 31) >> 5, ntk = (Tk + 31) >> 5;
  if (tb < ntq) split_block<false>(q, ldq, qf, n, h, bh, tb, T, ntq, d, KQ, DB, sv);
  if (tb < ntk) {
    split_block<false>(k, ldkv, kf, n, h, bh, tb, Tk, ntk, d, KQ, DB, sv);
    split_block<true>(v, ldkv, vtf, n, h, bh, tb, Tk, ntk, d, KQ, DB, sv);
  }
}

template <typename T_, int KQ, int DB, int QT>
__global__ __launch_bounds__(64) void attn_flash_kernel(const u16* __restrict__ qf, const u16* __restrict__ kf, const u16* __restrict__ vtf,
                                                        u16* __restrict__ out, float* __restrict__ lse, int T, int Tk, int heads, int d,
                                                        float scale_log2e) {
  const int lane = threadIdx.x, l31 = lane & 31, lhi = lane >> 5;
  const int nx = gridDim.x;
  const int lin = xcd_remap(blockIdx.x + nx * blockIdx.y, nx * gridDim.y);     // all query tiles of a head on one XCD (its K/V stay in that L2)
  const int bh = lin / nx, bx = lin - bh * nx;
  const int ntq = (T + 31) >> 5, ntk = (Tk + 31) >> 5;
  uint4 qr[QT][KQ];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int tb = min(bx * QT + qt, ntq - 1);                                   // a tile past the end repeats the last one (never stored)
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) qr[qt][kk] = *(const uint4*)(qf + rfrag_g((int64_t)bh * ntq + tb, KQ, kk, lhi, l31));
  }
  f32x16 o[QT][DB];
  float m_run[QT], l_run[QT];
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    m_run[qt] = -1e30f; l_run[qt] = 0.f;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) o[qt][db][r] = 0.f;
  }
  for (int sb = 0; sb < ntk; ++sb) {
    const int64_t blk = (int64_t)bh * ntk + sb;
    f32x16 sacc[QT];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt)
#pragma unroll
      for (int r = 0; r < 16; ++r) sacc[qt][r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) {
      const uint4 kfr = *(const uint4*)(kf + rfrag_g(blk, KQ, kk, lhi, l31));
#pragma unroll
      for (int qt = 0; qt < QT; ++qt) sacc[qt] = T_::mfma32(kfr, qr[qt][kk], sacc[qt]);
    }
    const bool tail = (sb + 1) * 32 > Tk;
    uint4 pfrag[QT][2];
#pragma unroll
    for (int qt = 0; qt < QT; ++qt) {
      float mx = -1e30f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if (tail && sb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi >= Tk) sacc[qt][r] = -1e30f;
        mx = fmaxf(mx, sacc[qt][r]);
      }
      mx = fmaxf(mx, __shfl_xor(mx, 32)) * scale_log2e;              // the scale is positive: max commutes with it
      // Lazy rescaling: the running maximum only follows when a block exceeds it by more than 2^8 (the probabilities then stay below
      // 256: exact in fp32 sums, well inside the 16-bit operand range), so after the first blocks the accumulator rescale (one multiply per
      // accumulator register) and its exp2 almost never run.  The branch is wave-uniform.
      if (__any(mx > m_run[qt] + 8.f)) {
        const float m_new = fmaxf(m_run[qt], mx);
        const float alpha = exp2f(m_run[qt] - m_new);
        l_run[qt] *= alpha;
        m_run[qt] = m_new;
#pragma unroll
        for (int db = 0; db < DB; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) o[qt][db][r] *= alpha;
      }
      const float mneg = -m_run[qt];
      float rs = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float p = exp2f(fmaf(sacc[qt][r], scale_log2e, mneg));   // one fused multiply-add + one v_exp per score
        sacc[qt][r] = p;
        rs += p;
      }
      rs += __shfl_xor(rs, 32);
      l_run[qt] += rs;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        float pf[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) pf[j] = sacc[qt][8 * ks + j];
        pfrag[qt][ks] = pack8<T_>(pf);
      }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        const uint4 vf = *(const uint4*)(vtf + tfrag_g(blk, DB, ks, db, lhi, l31));
#pragma unroll
        for (int qt = 0; qt < QT; ++qt) o[qt][db] = T_::mfma32(vf, pfrag[qt][ks], o[qt][db]);
      }
  }
  const int n = bh / heads, h = bh - n * heads;
#pragma unroll
  for (int qt = 0; qt < QT; ++qt) {
    const int t = (bx * QT + qt) * 32 + l31;
    if (lse && lhi == 0 && bx * QT + qt < ntq) lse[(int64_t)bh * ntq * 32 + t] = t < T ? m_run[qt] + log2f(l_run[qt]) : 0.f;   // training forward only
    if (t >= T) continue;
    const float inv = 1.f / l_run[qt];
    u16* ob = out + ((int64_t)n * T + t) * (heads * d) + h * d;
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int c = 32 * db + 8 * g + 4 * lhi;
        if (c < d)
          *(uint2*)(ob + c) = pack4<T_>(o[qt][db][4 * g] * inv, o[qt][db][4 * g + 1] * inv, o[qt][db][4 * g + 2] * inv, o[qt][db][4 * g + 3] * inv);
      }
  }
}

// The same computation with FOUR waves (128 queries) per workgroup sharing every K / V^T fragment through LDS: one wave per 32 queries
// streams 7 KB (d = 40) per key block from L2, at T = 4096 that is 7 GB per call and 12 TB/s of L2 -> register traffic -- the bound
// of the one-wave kernel.  Here the workgroup loads a key block's fragments once (register-staged, one block ahead, double-buffered in
// LDS: one barrier per key block) and the four waves read them from LDS (fragment order: 64 lanes x 16 B contiguous, conflict-free).
template <typename T_, int KQ, int DB>
__global__ __launch_bounds__(256) void attn_flash_lds_kernel(const u16* __restrict__ qf, const u16* __restrict__ kf, const u16* __restrict__ vtf,
                                                            u16* __restrict__ out, float* __restrict__ lse, int T, int Tk, int heads, int d,
                                                            float scale_log2e) {
  constexpr int NP = KQ + 2 * DB;                      // 1 KB fragment pieces per key block
  constexpr int NPI = (NP + 3) / 4;                    // pieces staged per thread
  __shared__ uint4 kv[2][NP * 64];
  const int tid = threadIdx.x, lane = tid & 63, l31 = lane & 31, lhi = lane >> 5;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nx = gridDim.x;
  const int lin = xcd_remap(blockIdx.x + nx * blockIdx.y, nx * gridDim.y);
  const int bh = lin / nx, bx = lin - bh * nx;
  const int ntq = (T + 31) >> 5, ntk = (Tk + 31) >> 5;
  const int tq = bx * 4 + wid;                         // this wave's query tile (past the end: repeats the last one, never stored)
  uint4 qr[KQ];
#pragma unroll
  for (int kk = 0; kk < KQ; ++kk) qr[kk] = *(const uint4*)(qf + rfrag_g((int64_t)bh * ntq + min(tq, ntq - 1), KQ, kk, lhi, l31));
  f32x16 o[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) o[db][r] = 0.f;
  float m_run = -1e30f, l_run = 0.f;

  const u16* const kbase = kf + (int64_t)bh * ntk * KQ * 512;
  const u16* const vbase = vtf + (int64_t)bh * ntk * 2 * DB * 512;
  // piece p of key block sb: K fragment p (p < KQ) or V^T fragment p - KQ; thread (wave w, lane) stages pieces w, w + 4, ...
  // (plain macros: as lambdas capturing the staging array the compiler demoted it to scratch)
  uint4 st[NPI];
#define FLASH_LOAD_BLOCK(SB)                                                                                              \
  _Pragma("unroll") for (int i = 0; i < NPI; ++i) {                                                                       \
    const int p = wid + 4 * i;                                                                                            \
    const u16* src = p < KQ ? kbase + ((int64_t)(SB) * KQ + p) * 512 : vbase + ((int64_t)(SB) * 2 * DB + (p - KQ)) * 512; \
    st[i] = p < NP ? *(const uint4*)(src + lane * 8) : make_uint4(0, 0, 0, 0);                                            \
  }
#define FLASH_STORE_BLOCK(BUF)                                                                                            \
  _Pragma("unroll") for (int i = 0; i < NPI; ++i) {                                                                       \
    const int p = wid + 4 * i;                                                                                            \
    if (p < NP) kv[BUF][p * 64 + lane] = st[i];                                                                           \
  }
  FLASH_LOAD_BLOCK(0)
  FLASH_STORE_BLOCK(0)
  if (ntk > 1) { FLASH_LOAD_BLOCK(1) }
  __syncthreads();
  for (int sb = 0; sb < ntk; ++sb) {
    const uint4* const cur = kv[sb & 1];
    f32x16 sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) sacc = T_::mfma32(cur[kk * 64 + lane], qr[kk], sacc);
    const bool tail = (sb + 1) * 32 > Tk;
    float mx = -1e30f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (tail && sb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi >= Tk) sacc[r] = -1e30f;
      mx = fmaxf(mx, sacc[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32)) * scale_log2e;
    if (__any(mx > m_run + 8.f)) {                     // lazy rescaling, as in attn_flash_kernel
      const float m_new = fmaxf(m_run, mx);
      const float alpha = exp2f(m_run - m_new);
      l_run *= alpha;
      m_run = m_new;
#pragma unroll
      for (int db = 0; db < DB; ++db)
#pragma unroll
        for (int r = 0; r < 16; ++r) o[db][r] *= alpha;
    }
    const float mneg = -m_run;
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = exp2f(fmaf(sacc[r], scale_log2e, mneg));
      sacc[r] = p;
      rs += p;
    }
    rs += __shfl_xor(rs, 32);
    l_run += rs;
    // the next block's fragments (in flight since the previous iteration) go to the other buffer: every wave finished reading it before
    // the barrier that ended the previous iteration
    if (sb + 1 < ntk) { FLASH_STORE_BLOCK((sb + 1) & 1) }
    if (sb + 2 < ntk) { FLASH_LOAD_BLOCK(sb + 2) }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      float pf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = sacc[8 * ks + j];
      const uint4 pfrag = pack8<T_>(pf);
#pragma unroll
      for (int db = 0; db < DB; ++db) o[db] = T_::mfma32(cur[(KQ + ks * DB + db) * 64 + lane], pfrag, o[db]);
    }
    __syncthreads();
  }
  const int t = tq * 32 + l31;
  if (lse && lhi == 0 && tq < ntq) lse[(int64_t)bh * ntq * 32 + t] = t < T ? m_run + log2f(l_run) : 0.f;       // training forward only
  if (tq >= ntq || t >= T) return;
  const int n = bh / heads, h = bh - n * heads;
  const float inv = 1.f / l_run;
  u16* ob = out + ((int64_t)n * T + t) * (heads * d) + h * d;
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = 32 * db + 8 * g + 4 * lhi;
      if (c < d) *(uint2*)(ob + c) = pack4<T_>(o[db][4 * g] * inv, o[db][4 * g + 1] * inv, o[db][4 * g + 2] * inv, o[db][4 * g + 3] * inv);
    }
#undef FLASH_LOAD_BLOCK
#undef FLASH_STORE_BLOCK
}

static int g_flash_qt = 0;       // A/B switch (pmi_set_option 9): 0 = automatic (LDS-shared kernel for long sequences), 1 / 2 = one-wave kernel with 1 / 2 query tiles per wave

template <typename T_, int KQ, int DB>
void launch_flash(const u16* qf, const u16* kf, const u16* vtf, u16* out, float* lse, int N, int T, int Tk, int heads, int d, float sl2, hipStream_t st) {
  const int ntq = (T + 31) / 32;
  // two query tiles per wave where the sequence is long enough to still fill the chip (and the accumulators fit: DB <= 3)
  if (g_flash_qt != 1 && g_flash_qt != 2 && ntq >= 64) {     // long query sequences (T >= 2048): four waves per workgroup share K / V^T through LDS (0.61 vs 0.65 ms at T = 4096)
    hipLaunchKernelGGL((attn_flash_lds_kernel<T_, KQ, DB>), dim3((ntq + 3) / 4, N * heads), dim3(256), 0, st, qf, kf, vtf, out, lse, T, Tk, heads, d, sl2);
    return;
  }
  if constexpr (DB <= 2) {
    if (g_flash_qt == 2) {      // measured at T = 4096, d = 40: 0.85 ms against 0.65 ms with one tile per wave (204 VGPRs: one wave per SIMD)
      hipLaunchKernelGGL((attn_flash_kernel<T_, KQ, DB, 2>), dim3((ntq + 1) / 2, N * heads), dim3(64), 0, st, qf, kf, vtf, out, lse, T, Tk, heads, d, sl2);
      return;
    }
  }
  hipLaunchKernelGGL((attn_flash_kernel<T_, KQ, DB, 1>), dim3(ntq, N * heads), dim3(64), 0, st, qf, kf, vtf, out, lse, T, Tk, heads, d, sl2);
}

template <typename T_>
int dispatch_flash(const u16* qf, const u16* kf, const u16* vtf, u16* out, float* lse, int N, int T, int Tk, int heads, int d, float sl2, hipStream_t st) {
  const int KQ = (d + 15) / 16, DB = (d + 31) / 32;
#define CASE(kq, db) if (KQ == kq && DB == db) { launch_flash<T_, kq, db>(qf, kf, vtf, out, lse, N, T, Tk, heads, d, sl2, st); return PMI_OK; }
  CASE(1, 1) CASE(2, 1) CASE(3, 2) CASE(4, 2) CASE(5, 3) CASE(6, 3) CASE(7, 4) CASE(8, 4) CASE(9, 5) CASE(10, 5)
#undef CASE
  return PMI_ERR_ARG;
}


// ---- backward: P recomputed per 32 x 32 tile from the forward's log-sum-exp, no T x Tk matrix in HBM, no atomics ---------------------------
// The scheme of attn.hip's 64-channel vit_attn_bwd_kernel, generalised to KQ k-steps / DB channel blocks and a separate key length:
//   dQ role   : one wave per 32-query tile, loops over key tiles.   S^T = K Q^T and dP^T = V dO^T put the query on the lane (lse, delta are
//               lane-local); dS^T, still in the accumulator, is the B operand of dQ^T += K^T dS^T.
//   dK/dV role: one wave per 32-key tile, loops over query tiles.   S = Q K^T and dP = dO V^T put the key on the lane; P and dS are the B
//               operands of dV^T += dO^T P and dK^T += Q^T dS.
// Both roles of a layer are one launch (workgroups [0, ntk) own key tiles, the rest query tiles); cross-attention with a frozen
// prompt compiles the dQ role alone, with a differentiable prompt the split key role further down.  Every output element is written once by one wave in a fixed order: run-to-run bit-identical.
// Extra fragments (flash_bwd_split_kernel): dO and V in Q / K order, K^T (and, with dK / dV, dO^T and Q^T) in V^T order;
// delta[bh][t] = sum_c dO[t][c] O[t][c] fp32.  P = exp2(S scale log2e - lse): lse is in the exp2 domain, as the forward's running maximum.
template <typename T_>
__global__ __launch_bounds__(256) void flash_bwd_split_kernel(const u16* __restrict__ q, int ldq, const u16* __restrict__ k, const u16* __restrict__ v,
                                                              int ldkv, const u16* __restrict__ o, const u16* __restrict__ dout,
                                                              u16* __restrict__ dof, u16* __restrict__ vf, u16* __restrict__ ktf,
                                                              u16* __restrict__ dotf, u16* __restrict__ qtf, float* __restrict__ delta, int T, int Tk,
                                                              int heads, int d, int KQ, int DB, int dq_only) {
  __shared__ u16 sv[32][168];
  const int tb = blockIdx.x, bh = blockIdx.y, n = bh / heads, h = bh - n * heads;
  const int ntq = (T + 31) >> 5, ntk = (Tk + 31) >> 5, C = heads * d;
  if (tb < ntq) {
    split_block<false>(dout, C, dof, n, h, bh, tb, T, ntq, d, KQ, DB, sv);
    const int tid = threadIdx.x, row = tid >> 3, ch = tid & 7, t = tb * 32 + row;
    float p = 0.f;
    if (t < T) {
      const int64_t off = ((int64_t)n * T + t) * C + h * d;
      for (int c8 = ch; c8 * 8 < d; c8 += 8) {
        float a[8], b[8];
        unpack8<T_>(*(const uint4*)(dout + off + c8 * 8), a);
        unpack8<T_>(*(const uint4*)(o + off + c8 * 8), b);
#pragma unroll
        for (int e = 0; e < 8; ++e) p += a[e] * b[e];
      }
    }
    p += __shfl_xor(p, 1); p += __shfl_xor(p, 2); p += __shfl_xor(p, 4);
    if (ch == 0) delta[(int64_t)bh * ntq * 32 + t] = p;
    if (!dq_only) {
      split_block<true>(dout, C, dotf, n, h, bh, tb, T, ntq, d, KQ, DB, sv);
      split_block<true>(q, ldq, qtf, n, h, bh, tb, T, ntq, d, KQ, DB, sv);
    }
  }
  if (tb < ntk) {
    split_block<false>(v, ldkv, vf, n, h, bh, tb, Tk, ntk, d, KQ, DB, sv);
    split_block<true>(k, ldkv, ktf, n, h, bh, tb, Tk, ntk, d, KQ, DB, sv);
  }
}

// channel rows of an accumulator block set (the forward's output order) -> rows of dst [..][ld], head channels [0, d)
template <typename T_, int DB>
__device__ __forceinline__ void store_rows(const f32x16* acc, u16* dst, int d, int lhi) {
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = 32 * db + 8 * g + 4 * lhi;
      if (c < d) *(uint2*)(dst + c) = pack4<T_>(acc[db][4 * g], acc[db][4 * g + 1], acc[db][4 * g + 2], acc[db][4 * g + 3]);
    }
}

template <typename T_, int KQ, int DB>
__device__ __forceinline__ void flash_dq_body(const u16* __restrict__ qf, const u16* __restrict__ dof, const u16* __restrict__ kf,
                                              const u16* __restrict__ vf, const u16* __restrict__ ktf, const float* __restrict__ lse,
                                              const float* __restrict__ delta, u16* __restrict__ dq, int lddq, int T, int Tk, int heads, int d,
                                              float sl2, float scale, int bx, int bh) {
  const int lane = threadIdx.x, l31 = lane & 31, lhi = lane >> 5;
  const int ntq = (T + 31) >> 5, ntk = (Tk + 31) >> 5;
  uint4 qr[KQ], dor[KQ];
#pragma unroll
  for (int kk = 0; kk < KQ; ++kk) {
    qr[kk] = *(const uint4*)(qf + rfrag_g((int64_t)bh * ntq + bx, KQ, kk, lhi, l31));
    dor[kk] = *(const uint4*)(dof + rfrag_g((int64_t)bh * ntq + bx, KQ, kk, lhi, l31));
  }
  const float nlse = -lse[((int64_t)bh * ntq + bx) * 32 + l31], my_delta = delta[((int64_t)bh * ntq + bx) * 32 + l31];
  f32x16 g[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) g[db][r] = 0.f;
  for (int sb = 0; sb < ntk; ++sb) {
    const int64_t blk = (int64_t)bh * ntk + sb;
    f32x16 sacc, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) {
      sacc = T_::mfma32(*(const uint4*)(kf + rfrag_g(blk, KQ, kk, lhi, l31)), qr[kk], sacc);
      dp = T_::mfma32(*(const uint4*)(vf + rfrag_g(blk, KQ, kk, lhi, l31)), dor[kk], dp);
    }
    const bool tail = (sb + 1) * 32 > Tk;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float p = exp2f(fmaf(sacc[r], sl2, nlse));
      if (tail && sb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi >= Tk) p = 0.f;       // a padded key has no weight
      sacc[r] = p * (dp[r] - my_delta) * scale;                                    // dS^T[s][t]
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = sacc[8 * ks + j];
      const uint4 dsf = pack8<T_>(f);
#pragma unroll
      for (int db = 0; db < DB; ++db) g[db] = T_::mfma32(*(const uint4*)(ktf + tfrag_g(blk, DB, ks, db, lhi, l31)), dsf, g[db]);
    }
  }
  const int t = bx * 32 + l31;
  if (t >= T) return;
  const int n = bh / heads, h = bh - n * heads;
  store_rows<T_, DB>(g, dq + ((int64_t)n * T + t) * lddq + h * d, d, lhi);
}

template <typename T_, int KQ, int DB>
__device__ __forceinline__ void flash_dkdv_body(const u16* __restrict__ qf, const u16* __restrict__ dof, const u16* __restrict__ kf,
                                                const u16* __restrict__ vf, const u16* __restrict__ qtf, const u16* __restrict__ dotf,
                                                const float* __restrict__ lse, const float* __restrict__ delta, u16* __restrict__ dk,
                                                u16* __restrict__ dv, int lddkv, int T, int Tk, int heads, int d, float sl2, float scale, int bx,
                                                int bh) {
  const int lane = threadIdx.x, l31 = lane & 31, lhi = lane >> 5;
  const int ntq = (T + 31) >> 5, ntk = (Tk + 31) >> 5;
  uint4 kr[KQ], vr[KQ];
#pragma unroll
  for (int kk = 0; kk < KQ; ++kk) {
    kr[kk] = *(const uint4*)(kf + rfrag_g((int64_t)bh * ntk + bx, KQ, kk, lhi, l31));
    vr[kk] = *(const uint4*)(vf + rfrag_g((int64_t)bh * ntk + bx, KQ, kk, lhi, l31));
  }
  const bool key_ok = bx * 32 + l31 < Tk;
  f32x16 gk[DB], gv[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) { gk[db][r] = 0.f; gv[db][r] = 0.f; }
  for (int tb = 0; tb < ntq; ++tb) {
    const int64_t blk = (int64_t)bh * ntq + tb;
    // the 16 query rows of this lane's accumulator registers: 4 runs of 4 consecutive rows
    float4 ls[4], dl[4];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      ls[g4] = *(const float4*)(lse + blk * 32 + 8 * g4 + 4 * lhi);
      dl[g4] = *(const float4*)(delta + blk * 32 + 8 * g4 + 4 * lhi);
    }
    f32x16 sacc, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) {
      sacc = T_::mfma32(*(const uint4*)(qf + rfrag_g(blk, KQ, kk, lhi, l31)), kr[kk], sacc);        // rows = queries, lane = key
      dp = T_::mfma32(*(const uint4*)(dof + rfrag_g(blk, KQ, kk, lhi, l31)), vr[kk], dp);
    }
    const bool tail = (tb + 1) * 32 > T;
    float pf[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* l4 = (const float*)&ls[r >> 2];
      const float* d4 = (const float*)&dl[r >> 2];
      float p = key_ok ? exp2f(fmaf(sacc[r], sl2, -l4[r & 3])) : 0.f;
      if (tail && tb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi >= T) p = 0.f;
      pf[r] = p;
      sacc[r] = p * (dp[r] - d4[r & 3]) * scale;                                                     // dS[t][s]
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const uint4 pfrag = pack8<T_>(pf + 8 * ks);
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = sacc[8 * ks + j];
      const uint4 dsf = pack8<T_>(f);
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        gv[db] = T_::mfma32(*(const uint4*)(dotf + tfrag_g(blk, DB, ks, db, lhi, l31)), pfrag, gv[db]);
        gk[db] = T_::mfma32(*(const uint4*)(qtf + tfrag_g(blk, DB, ks, db, lhi, l31)), dsf, gk[db]);
      }
    }
  }
  const int s = bx * 32 + l31;
  if (s >= Tk) return;
  const int n = bh / heads, h = bh - n * heads;
  const int64_t off = ((int64_t)n * Tk + s) * lddkv + h * d;
  store_rows<T_, DB>(gk, dk + off, d, lhi);
  store_rows<T_, DB>(gv, dv + off, d, lhi);
}

struct FlashBwdArgs {
  const u16 *qf, *kf, *dof, *vf, *ktf, *dotf, *qtf;
  const float *lse, *delta;
  u16 *dq, *dk, *dv;
  int lddq, lddkv, T, Tk, heads, d;
  float sl2, scale;
};

// ---- dK / dV for a short key sequence (cross-attention onto the prompt: Tk = 77 is three key tiles) ----------------------------------------
// One wave per key tile walking every query tile leaves 3 N heads one-wave workgroups, each serial in T.  Here the query tiles are cut
// into S chunks of L tiles: workgroup (key tile, chunk, sample x head) runs the key role over its chunk and leaves its fp32 accumulators
// as a partial tile; flash_kv_reduce_kernel, a launch of its own (the kernel boundary makes the partials visible across the per-XCD L2s),
// adds the S partials of every element in chunk order and writes fp32 dK | dV once.  No atomics; S depends on the shape alone
// (flash_kv_chunks), so two runs are bit-identical.  S = 1: the accumulators go straight to dK | dV, the unsplit role's arithmetic.
// dK / dV stay fp32: they sum up to T terms whose size no 16-bit range argument covers (dK = dS^T Q has no bound in terms of dO), and the
// fp32 GEMM onto the prompt encodings takes them as they are.
// Partial tile of (bh, key tile, chunk): [dK | dV][db][4 row groups][64 lanes] float4 = the accumulator registers, lane-contiguous.
// flash_dkdv_body's loop over the query tiles [tb0, tb1) only, the accumulators handed back: dV^T += dO^T P and dK^T += Q^T dS into gv / gk
// (zeroed here).  A function of its own so that the self-attention kernels above compile to exactly what they were.
template <typename T_, int KQ, int DB>
__device__ __forceinline__ void flash_dkdv_accumulate(const u16* __restrict__ qf, const u16* __restrict__ dof, const u16* __restrict__ kf,
                                                      const u16* __restrict__ vf, const u16* __restrict__ qtf, const u16* __restrict__ dotf,
                                                      const float* __restrict__ lse, const float* __restrict__ delta, int T, int Tk, float sl2,
                                                      float scale, int bx, int bh, int tb0, int tb1, f32x16* gk, f32x16* gv) {
  const int lane = threadIdx.x, l31 = lane & 31, lhi = lane >> 5;
  const int ntq = (T + 31) >> 5, ntk = (Tk + 31) >> 5;
  uint4 kr[KQ], vr[KQ];
#pragma unroll
  for (int kk = 0; kk < KQ; ++kk) {
    kr[kk] = *(const uint4*)(kf + rfrag_g((int64_t)bh * ntk + bx, KQ, kk, lhi, l31));
    vr[kk] = *(const uint4*)(vf + rfrag_g((int64_t)bh * ntk + bx, KQ, kk, lhi, l31));
  }
  const bool key_ok = bx * 32 + l31 < Tk;
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) { gk[db][r] = 0.f; gv[db][r] = 0.f; }
  for (int tb = tb0; tb < tb1; ++tb) {
    const int64_t blk = (int64_t)bh * ntq + tb;
    // the 16 query rows of this lane's accumulator registers: 4 runs of 4 consecutive rows
    float4 ls[4], dl[4];
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      ls[g4] = *(const float4*)(lse + blk * 32 + 8 * g4 + 4 * lhi);
      dl[g4] = *(const float4*)(delta + blk * 32 + 8 * g4 + 4 * lhi);
    }
    f32x16 sacc, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < KQ; ++kk) {
      sacc = T_::mfma32(*(const uint4*)(qf + rfrag_g(blk, KQ, kk, lhi, l31)), kr[kk], sacc);        // rows = queries, lane = key
      dp = T_::mfma32(*(const uint4*)(dof + rfrag_g(blk, KQ, kk, lhi, l31)), vr[kk], dp);
    }
    const bool tail = (tb + 1) * 32 > T;
    float pf[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float* l4 = (const float*)&ls[r >> 2];
      const float* d4 = (const float*)&dl[r >> 2];
      float p = key_ok ? exp2f(fmaf(sacc[r], sl2, -l4[r & 3])) : 0.f;
      if (tail && tb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi >= T) p = 0.f;
      pf[r] = p;
      sacc[r] = p * (dp[r] - d4[r & 3]) * scale;                                                     // dS[t][s]
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const uint4 pfrag = pack8<T_>(pf + 8 * ks);
      float f[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = sacc[8 * ks + j];
      const uint4 dsf = pack8<T_>(f);
#pragma unroll
      for (int db = 0; db < DB; ++db) {
        gv[db] = T_::mfma32(*(const uint4*)(dotf + tfrag_g(blk, DB, ks, db, lhi, l31)), pfrag, gv[db]);
        gk[db] = T_::mfma32(*(const uint4*)(qtf + tfrag_g(blk, DB, ks, db, lhi, l31)), dsf, gk[db]);
      }
    }
  }
}

template <int DB>
__device__ __forceinline__ void store_rows_f32(const f32x16* acc, float* dst, int d, int lhi) {
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int c = 32 * db + 8 * g + 4 * lhi;
      if (c < d) *(float4*)(dst + c) = make_float4(acc[db][4 * g], acc[db][4 * g + 1], acc[db][4 * g + 2], acc[db][4 * g + 3]);
    }
}

struct FlashBwdKvArgs {
  FlashBwdArgs b;
  float *part, *dk32, *dv32;     // dk32 / dv32 [N][Tk][lddkv] fp32, head h at channel offset h*d
  int S, L;                      // chunks per key tile, query tiles per chunk (S = ceil(ntq / L): no chunk is empty)
};

template <typename T_, int KQ, int DB>
__global__ __launch_bounds__(64) void attn_flash_bwd_kv_kernel(const FlashBwdKvArgs ka) {
  const FlashBwdArgs& a = ka.b;
  const int nx = gridDim.x;
  const int lin = xcd_remap(blockIdx.x + nx * blockIdx.y, nx * gridDim.y);     // a head's tiles on one XCD, as the forward
  const int bh = lin / nx, bx = lin - bh * nx;
  const int ntq = (a.T + 31) >> 5, ntk = (a.Tk + 31) >> 5, nkey = ntk * ka.S;
  if (bx >= nkey) {
    flash_dq_body<T_, KQ, DB>(a.qf, a.dof, a.kf, a.vf, a.ktf, a.lse, a.delta, a.dq, a.lddq, a.T, a.Tk, a.heads, a.d, a.sl2, a.scale, bx - nkey, bh);
    return;
  }
  const int kt = bx / ka.S, ch = bx - kt * ka.S;
  const int lane = threadIdx.x, l31 = lane & 31, lhi = lane >> 5;
  f32x16 gk[DB], gv[DB];
  flash_dkdv_accumulate<T_, KQ, DB>(a.qf, a.dof, a.kf, a.vf, a.qtf, a.dotf, a.lse, a.delta, a.T, a.Tk, a.sl2, a.scale, kt, bh, ch * ka.L,
                                    min(ntq, (ch + 1) * ka.L), gk, gv);
  if (ka.S == 1) {
    const int s = kt * 32 + l31;
    if (s >= a.Tk) return;
    const int n = bh / a.heads, h = bh - n * a.heads;
    const int64_t off = ((int64_t)n * a.Tk + s) * a.lddkv + h * a.d;
    store_rows_f32<DB>(gk, ka.dk32 + off, a.d, lhi);
    store_rows_f32<DB>(gv, ka.dv32 + off, a.d, lhi);
    return;
  }
  float4* p = (float4*)ka.part + (((int64_t)bh * ntk + kt) * ka.S + ch) * (2 * DB * 4 * 64) + lane;
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      p[(db * 4 + g) * 64] = make_float4(gk[db][4 * g], gk[db][4 * g + 1], gk[db][4 * g + 2], gk[db][4 * g + 3]);
      p[((DB + db) * 4 + g) * 64] = make_float4(gv[db][4 * g], gv[db][4 * g + 1], gv[db][4 * g + 2], gv[db][4 * g + 3]);
    }
}

// one thread per float4 of a (bh, key tile) output tile: the S partials added in chunk order, then written once
__global__ __launch_bounds__(256) void flash_kv_reduce_kernel(const float4* __restrict__ part, float* __restrict__ dk32, float* __restrict__ dv32,
                                                              int lddkv, int64_t total, int Tk, int heads, int d, int DB, int S) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int per = 2 * DB * 4 * 64, ntk = (Tk + 31) >> 5;
  const int64_t tile = i / per;                    // bh * ntk + kt
  const int in = (int)(i - tile * per), lane = in & 63, g = (in >> 6) & 3, wdb = in >> 8, which = wdb / DB, db = wdb - which * DB;
  const int bh = (int)(tile / ntk), kt = (int)(tile - (int64_t)bh * ntk);
  const int s = kt * 32 + (lane & 31), c = 32 * db + 8 * g + 4 * (lane >> 5);
  if (s >= Tk || c >= d) return;
  const float4* p = part + tile * S * per + in;
  float4 acc = p[0];
  for (int ch = 1; ch < S; ++ch) {
    const float4 v = p[(int64_t)ch * per];
    acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
  }
  const int n = bh / heads, h = bh - n * heads;
  *(float4*)((which ? dv32 : dk32) + ((int64_t)n * Tk + s) * lddkv + h * d + c) = acc;
}

static int g_kv_chunks = 0;      // A/B switch (pmi_set_option 14): 0 = automatic, n > 0 = at most n chunks (1 = the unsplit key role)

// Chunks per key tile, from the shape alone.  The unsplit role has ntk N heads waves; the chip has 1024 SIMDs and the key role's two
// accumulator sets leave room for about two waves on each, so the target is 2048 key-role workgroups.  A chunk keeps at least 4 query
// tiles: a partial tile is as many bytes as the fragments of one query tile, so the workspace traffic stays below a quarter of the reads
// (T = 64, two query tiles, stays unsplit).
void flash_kv_chunks(int N, int T, int Tk, int heads, int* S, int* L) {
  const int64_t ntq = (T + 31) / 32, ntk = (Tk + 31) / 32, waves = ntk * N * heads;
  int64_t want = (2048 + waves - 1) / waves;
  if (want > ntq / 4) want = ntq / 4;
  if (g_kv_chunks > 0 && want > g_kv_chunks) want = g_kv_chunks;
  if (want < 1) want = 1;
  *L = (int)((ntq + want - 1) / want);
  *S = (int)((ntq + *L - 1) / *L);
}

template <typename T_>
int dispatch_flash_bwd_kv(const FlashBwdKvArgs& ka, int N, hipStream_t st) {
  const FlashBwdArgs& a = ka.b;
  const int KQ = (a.d + 15) / 16, DB = (a.d + 31) / 32, ntq = (a.T + 31) / 32, ntk = (a.Tk + 31) / 32;
  const dim3 grid(ntq + ntk * ka.S, N * a.heads);
#define CASE(kq, db)                                                                                 \
  if (KQ == kq && DB == db) {                                                                        \
    hipLaunchKernelGGL((attn_flash_bwd_kv_kernel<T_, kq, db>), grid, dim3(64), 0, st, ka);           \
    return PMI_OK;                                                                                   \
  }
  CASE(1, 1) CASE(2, 1) CASE(3, 2) CASE(4, 2) CASE(5, 3) CASE(6, 3) CASE(7, 4) CASE(8, 4) CASE(9, 5) CASE(10, 5)
#undef CASE
  return PMI_ERR_ARG;
}

template <typename T_, int KQ, int DB, bool DQ_ONLY>
__global__ __launch_bounds__(64) void attn_flash_bwd_kernel(const FlashBwdArgs a) {
  const int nx = gridDim.x;
  const int lin = xcd_remap(blockIdx.x + nx * blockIdx.y, nx * gridDim.y);     // a head's tiles on one XCD, as the forward
  const int bh = lin / nx, bx = lin - bh * nx;
  const int ntk = (a.Tk + 31) >> 5;
  if constexpr (DQ_ONLY) {
    flash_dq_body<T_, KQ, DB>(a.qf, a.dof, a.kf, a.vf, a.ktf, a.lse, a.delta, a.dq, a.lddq, a.T, a.Tk, a.heads, a.d, a.sl2, a.scale, bx, bh);
  } else {
    if (bx < ntk)      // the key-tile role first: it carries two accumulator sets and the longer loop body
      flash_dkdv_body<T_, KQ, DB>(a.qf, a.dof, a.kf, a.vf, a.qtf, a.dotf, a.lse, a.delta, a.dk, a.dv, a.lddkv, a.T, a.Tk, a.heads, a.d, a.sl2,
                                  a.scale, bx, bh);
    else
      flash_dq_body<T_, KQ, DB>(a.qf, a.dof, a.kf, a.vf, a.ktf, a.lse, a.delta, a.dq, a.lddq, a.T, a.Tk, a.heads, a.d, a.sl2, a.scale, bx - ntk,
                                bh);
  }
}

template <typename T_>
int dispatch_flash_bwd(const FlashBwdArgs& a, int N, bool dq_only, hipStream_t st) {
  const int KQ = (a.d + 15) / 16, DB = (a.d + 31) / 32, ntq = (a.T + 31) / 32, ntk = (a.Tk + 31) / 32;
  const dim3 grid(dq_only ? ntq : ntq + ntk, N * a.heads);
#define CASE(kq, db)                                                                                          \
  if (KQ == kq && DB == db) {                                                                                 \
    if (dq_only) hipLaunchKernelGGL((attn_flash_bwd_kernel<T_, kq, db, true>), grid, dim3(64), 0, st, a);     \
    else hipLaunchKernelGGL((attn_flash_bwd_kernel<T_, kq, db, false>), grid, dim3(64), 0, st, a);            \
    return PMI_OK;                                                                                            \
  }
  CASE(1, 1) CASE(2, 1) CASE(3, 2) CASE(4, 2) CASE(5, 3) CASE(6, 3) CASE(7, 4) CASE(8, 4) CASE(9, 5) CASE(10, 5)
#undef CASE
  return PMI_ERR_ARG;
}

bool flash_args_ok(const void* q, int ldq, const void* k, const void* v, int ldkv, int N, int T, int Tk, int heads, int d, int dtype) {
  return q && k && v && N > 0 && T > 0 && Tk > 0 && heads > 0 && d > 0 && d <= 160 && !(d & 7) && ldq >= heads * d && ldkv >= heads * d &&
         !(ldq & 7) && !(ldkv & 7) && (dtype == PMI_DT_BF16 || dtype == PMI_DT_F16);
}

int flash_forward(const void* q, int ldq, const void* k, const void* v, int ldkv, void* out, void* ws, float* lse, int N, int T, int Tk, int heads,
                  int d, float scale, int dtype, hipStream_t st) {
  const int64_t KQ = (d + 15) / 16, DB = (d + 31) / 32, ntq = (T + 31) / 32, ntk = (Tk + 31) / 32;
  u16* qf = (u16*)ws;
  u16* kf = qf + (int64_t)N * heads * ntq * KQ * 512;
  u16* vtf = kf + (int64_t)N * heads * ntk * KQ * 512;
  hipLaunchKernelGGL(flash_split_kernel, dim3((unsigned)(ntq > ntk ? ntq : ntk), N * heads), dim3(256), 0, st, (const u16*)q, ldq, (const u16*)k,
                     (const u16*)v, ldkv, qf, kf, vtf, T, Tk, heads, d, (int)KQ, (int)DB);
  PMI_CHECK_LAUNCH();
  const float sl2 = scale * 1.4426950408889634f;
  const int rc = dtype == PMI_DT_BF16 ? dispatch_flash<BF16>(qf, kf, vtf, (u16*)out, lse, N, T, Tk, heads, d, sl2, st)
                                      : dispatch_flash<F16>(qf, kf, vtf, (u16*)out, lse, N, T, Tk, heads, d, sl2, st);
  if (rc != PMI_OK) return rc;
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

}  // namespace

void pmi_attn_flash_qt(int v) { g_flash_qt = v; }
void pmi_attn_flash_kv_chunks(int v) { g_kv_chunks = v; }

extern "C" int pmi_attn_flash_workspace(int N, int T, int Tk, int heads, int d) {       // in KiB (every term is a multiple of 1 KiB)
  if (N <= 0 || T <= 0 || Tk <= 0 || heads <= 0 || d <= 0 || d > 160 || (d & 7)) return -1;
  const int64_t KQ = (d + 15) / 16, DB = (d + 31) / 32, ntq = (T + 31) / 32, ntk = (Tk + 31) / 32;
  const int64_t kib = (int64_t)N * heads * (ntq * KQ + ntk * KQ + ntk * DB * 2);
  return kib > 0x7fffffff ? -1 : (int)kib;
}

extern "C" int pmi_attn_flash(const void* q, int ldq, const void* k, const void* v, int ldkv, void* out, void* ws, int N, int T, int Tk,
                              int heads, int d, float scale, int dtype, pmi_stream_t s) {
  if (!flash_args_ok(q, ldq, k, v, ldkv, N, T, Tk, heads, d, dtype) || !out || !ws) return PMI_ERR_ARG;
  return flash_forward(q, ldq, k, v, ldkv, out, ws, nullptr, N, T, Tk, heads, d, scale, dtype, (hipStream_t)s);
}

extern "C" int pmi_attn_flash_train(const void* q, int ldq, const void* k, const void* v, int ldkv, void* out, void* ws, float* lse, int N, int T,
                                    int Tk, int heads, int d, float scale, int dtype, pmi_stream_t s) {
  if (!flash_args_ok(q, ldq, k, v, ldkv, N, T, Tk, heads, d, dtype) || !out || !ws || !lse) return PMI_ERR_ARG;
  return flash_forward(q, ldq, k, v, ldkv, out, ws, lse, N, T, Tk, heads, d, scale, dtype, (hipStream_t)s);
}

extern "C" int pmi_attn_flash_bwd_workspace(int N, int T, int Tk, int heads, int d, int dq_only) {       // in KiB
  if (N <= 0 || T <= 0 || Tk <= 0 || heads <= 0 || d <= 0 || d > 160 || (d & 7)) return -1;
  const int64_t KQ = (d + 15) / 16, DB = (d + 31) / 32, ntq = (T + 31) / 32, ntk = (Tk + 31) / 32;
  const int64_t kib = (int64_t)N * heads * (ntq * KQ + ntk * KQ + ntk * DB * 2 + (dq_only ? 0 : ntq * DB * 4));
  return kib > 0x7fffffff ? -1 : (int)kib;
}

extern "C" int pmi_attn_flash_bwd(const void* q, int ldq, const void* k, const void* v, int ldkv, const void* out, const void* dout,
                                  const void* ws, const float* lse, void* ws_bwd, float* delta, void* dq, int lddq, void* dk, void* dv, int lddkv,
                                  int N, int T, int Tk, int heads, int d, float scale, int dq_only, int dtype, pmi_stream_t s) {
  if (!flash_args_ok(q, ldq, k, v, ldkv, N, T, Tk, heads, d, dtype) || !out || !dout || !ws || !lse || !ws_bwd || !delta || !dq ||
      lddq < heads * d || (lddq & 3))
    return PMI_ERR_ARG;
  if (!dq_only && (!dk || !dv || lddkv < heads * d || (lddkv & 3))) return PMI_ERR_ARG;
  const int64_t KQ = (d + 15) / 16, DB = (d + 31) / 32, ntq = (T + 31) / 32, ntk = (Tk + 31) / 32, NH = (int64_t)N * heads;
  FlashBwdArgs a;
  a.qf = (const u16*)ws;
  a.kf = a.qf + NH * ntq * KQ * 512;
  u16* dof = (u16*)ws_bwd;
  u16* vf = dof + NH * ntq * KQ * 512;
  u16* ktf = vf + NH * ntk * KQ * 512;
  u16* dotf = ktf + NH * ntk * DB * 1024;
  u16* qtf = dotf + NH * ntq * DB * 1024;
  if (dq_only) dotf = qtf = nullptr;
  hipStream_t st = (hipStream_t)s;
  const dim3 sg((unsigned)(ntq > ntk ? ntq : ntk), (unsigned)NH);
  if (dtype == PMI_DT_BF16)
    hipLaunchKernelGGL(flash_bwd_split_kernel<BF16>, sg, dim3(256), 0, st, (const u16*)q, ldq, (const u16*)k, (const u16*)v, ldkv, (const u16*)out,
                       (const u16*)dout, dof, vf, ktf, dotf, qtf, delta, T, Tk, heads, d, (int)KQ, (int)DB, dq_only);
  else
    hipLaunchKernelGGL(flash_bwd_split_kernel<F16>, sg, dim3(256), 0, st, (const u16*)q, ldq, (const u16*)k, (const u16*)v, ldkv, (const u16*)out,
                       (const u16*)dout, dof, vf, ktf, dotf, qtf, delta, T, Tk, heads, d, (int)KQ, (int)DB, dq_only);
  PMI_CHECK_LAUNCH();
  a.dof = dof; a.vf = vf; a.ktf = ktf; a.dotf = dotf; a.qtf = qtf;
  a.lse = lse; a.delta = delta;
  a.dq = (u16*)dq; a.dk = (u16*)dk; a.dv = (u16*)dv;
  a.lddq = lddq; a.lddkv = lddkv; a.T = T; a.Tk = Tk; a.heads = heads; a.d = d;
  a.scale = scale; a.sl2 = scale * 1.4426950408889634f;
  const int rc = dtype == PMI_DT_BF16 ? dispatch_flash_bwd<BF16>(a, N, dq_only != 0, st) : dispatch_flash_bwd<F16>(a, N, dq_only != 0, st);
  if (rc != PMI_OK) return rc;
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_attn_flash_bwd_kv_chunks(int N, int T, int Tk, int heads, int d) {
  if (N <= 0 || T <= 0 || Tk <= 0 || heads <= 0 || d <= 0 || d > 160 || (d & 7)) return -1;
  int S, L;
  flash_kv_chunks(N, T, Tk, heads, &S, &L);
  return S;
}

extern "C" int pmi_attn_flash_bwd_kv_workspace(int N, int T, int Tk, int heads, int d) {       // in KiB: the fragments, then the fp32 partial tiles
  const int base = pmi_attn_flash_bwd_workspace(N, T, Tk, heads, d, 0);
  if (base < 0) return -1;
  int S, L;
  flash_kv_chunks(N, T, Tk, heads, &S, &L);
  const int64_t DB = (d + 31) / 32, ntk = (Tk + 31) / 32;
  const int64_t kib = base + (S > 1 ? (int64_t)N * heads * ntk * S * DB * 8 : 0);
  return kib > 0x7fffffff ? -1 : (int)kib;
}

extern "C" int pmi_attn_flash_bwd_kv(const void* q, int ldq, const void* k, const void* v, int ldkv, const void* out, const void* dout,
                                     const void* ws, const float* lse, void* ws_bwd, float* delta, void* dq, int lddq, float* dk, float* dv,
                                     int lddkv, int N, int T, int Tk, int heads, int d, float scale, int dtype, pmi_stream_t s) {
  if (!flash_args_ok(q, ldq, k, v, ldkv, N, T, Tk, heads, d, dtype) || !out || !dout || !ws || !lse || !ws_bwd || !delta || !dq ||
      lddq < heads * d || (lddq & 3) || !dk || !dv || lddkv < heads * d || (lddkv & 3) || ((uintptr_t)dk & 15) || ((uintptr_t)dv & 15))
    return PMI_ERR_ARG;
  const int64_t KQ = (d + 15) / 16, DB = (d + 31) / 32, ntq = (T + 31) / 32, ntk = (Tk + 31) / 32, NH = (int64_t)N * heads;
  FlashBwdKvArgs ka;
  FlashBwdArgs& a = ka.b;
  flash_kv_chunks(N, T, Tk, heads, &ka.S, &ka.L);
  a.qf = (const u16*)ws;
  a.kf = a.qf + NH * ntq * KQ * 512;
  u16* dof = (u16*)ws_bwd;
  u16* vf = dof + NH * ntq * KQ * 512;
  u16* ktf = vf + NH * ntk * KQ * 512;
  u16* dotf = ktf + NH * ntk * DB * 1024;
  u16* qtf = dotf + NH * ntq * DB * 1024;
  ka.part = (float*)(qtf + NH * ntq * DB * 1024);       // every term above is a multiple of 1 KiB
  ka.dk32 = dk; ka.dv32 = dv;
  hipStream_t st = (hipStream_t)s;
  const dim3 sg((unsigned)(ntq > ntk ? ntq : ntk), (unsigned)NH);
  if (dtype == PMI_DT_BF16)
    hipLaunchKernelGGL(flash_bwd_split_kernel<BF16>, sg, dim3(256), 0, st, (const u16*)q, ldq, (const u16*)k, (const u16*)v, ldkv, (const u16*)out,
                       (const u16*)dout, dof, vf, ktf, dotf, qtf, delta, T, Tk, heads, d, (int)KQ, (int)DB, 0);
  else
    hipLaunchKernelGGL(flash_bwd_split_kernel<F16>, sg, dim3(256), 0, st, (const u16*)q, ldq, (const u16*)k, (const u16*)v, ldkv, (const u16*)out,
                       (const u16*)dout, dof, vf, ktf, dotf, qtf, delta, T, Tk, heads, d, (int)KQ, (int)DB, 0);
  PMI_CHECK_LAUNCH();
  a.dof = dof; a.vf = vf; a.ktf = ktf; a.dotf = dotf; a.qtf = qtf;
  a.lse = lse; a.delta = delta;
  a.dq = (u16*)dq; a.dk = nullptr; a.dv = nullptr;
  a.lddq = lddq; a.lddkv = lddkv; a.T = T; a.Tk = Tk; a.heads = heads; a.d = d;
  a.scale = scale; a.sl2 = scale * 1.4426950408889634f;
  const int rc = dtype == PMI_DT_BF16 ? dispatch_flash_bwd_kv<BF16>(ka, N, st) : dispatch_flash_bwd_kv<F16>(ka, N, st);
  if (rc != PMI_OK) return rc;
  PMI_CHECK_LAUNCH();
  if (ka.S > 1) {
    const int64_t total = NH * ntk * 2 * DB * 4 * 64;
    hipLaunchKernelGGL(flash_kv_reduce_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const float4*)ka.part, dk, dv, lddkv, total,
                       Tk, heads, d, (int)DB, ka.S);
    PMI_CHECK_LAUNCH();
  }
  return PMI_OK;
}
