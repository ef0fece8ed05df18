// Flash-style self-attention for head dim 64 on gfx950 MFMA (32x32x16), one wave per 32 queries.
//
//   S^T[s][t] = sum_d K[s][d] Q[t][d]   (MFMA A = K rows, B = Q rows) -> lane = query t, regs = keys s
//   online softmax over s is lane-local (+ one exchange with lane^32)
//   O^T[d][t] += V^T[d][s] P^T[s][t]    (MFMA A = V^T rows, B = the P accumulator re-used in place)
//
// The P^T accumulator feeds the second product without any lane movement or LDS: registers
// 8ks..8ks+7 of a 32x32 accumulator are, in order, k-elements 16ks + 8(j>>2) + 4(lane>>5) + (j&3),
// so the V^T fragment is read in that same k order (two 8-byte loads per k-step).
// K, Q and V^T fragments come straight from global memory (L2-resident: T <= 1024 keys x 64 x 2 B).
#include "common.h"
#include "../../include/perceptor_hip.h"

namespace {

// Transposed operands (head dim on the MFMA rows, tokens on k) are stored in FRAGMENT order: the 8 tokens a lane needs for one
// MFMA A operand, {16 ks + 4 lhi + 0..3} and {16 ks + 8 + 4 lhi + 0..3} of a 32-token block (the k order of an accumulator tile
// re-used as B operand), are 16 contiguous bytes and the 64 lanes of a wave are contiguous: one coalesced 1 KB load per fragment.
// With plain [bh][64][Tp] rows every fragment load touched 64 separate 8-byte pieces 2*Tp bytes apart.
__device__ __forceinline__ int64_t tfrag(int bh, int ntb, int tb, int ks, int db, int lhi, int l31) {
  return ((((((int64_t)bh * ntb + tb) * 2 + ks) * 2 + db) * 2 + lhi) * 32 + l31) * 8;
}

// The row operands (tokens on the MFMA rows, head dim on k: Q, K, V, dO) use the same idea: element (t, c) of a 32-token block
// lives at [block][kk = c / 16][lhi = (c / 8) & 1][t & 31][c & 7], so the fragment of step kk is one contiguous 1 KB run.
__device__ __forceinline__ int64_t rfrag(int bh, int ntb, int tb, int kk, int lhi, int l31) {
  return ((((((int64_t)bh * ntb + tb) * 4 + kk) * 2 + lhi) * 32 + l31) * 8);
}

// qkv [N][T][3C] -> Q,K [N*heads][Tp/32][fragment order, rfrag], Vt [N*heads][Tp/32][fragment order, tfrag]; zero fill for t >= T.
template <typename T_>
__global__ __launch_bounds__(256) void qkv_split_kernel(const u16* __restrict__ qkv, u16* __restrict__ q,
                                                        u16* __restrict__ k, u16* __restrict__ vt, int T, int Tp,
                                                        int heads, int order) {
  __shared__ u16 sv[32][72];
  const int tid = threadIdx.x, t0 = blockIdx.x * 32, bh = blockIdx.y;
  const int n = bh / heads, h = bh - n * heads;
  const int C = heads * 64;
  const int qoff = order == 0 ? h * 192 : h * 64;
  const int koff = order == 0 ? h * 192 + 64 : C + h * 64;
  const int voff = order == 0 ? h * 192 + 128 : 2 * C + h * 64;
  const int row = tid >> 3, ch = tid & 7;
  const int t = t0 + row;
  uint4 vq = make_uint4(0, 0, 0, 0), vk = vq, vv = vq;
  if (t < T) {
    const u16* src = qkv + ((int64_t)n * T + t) * 3 * C + ch * 8;
    vq = *(const uint4*)(src + qoff); vk = *(const uint4*)(src + koff); vv = *(const uint4*)(src + voff);
  }
  const int64_t o = rfrag(bh, Tp >> 5, blockIdx.x, ch >> 1, ch & 1, row);
  *(uint4*)(q + o) = vq;
  *(uint4*)(k + o) = vk;
  *(uint4*)(&sv[row][ch * 8]) = vv;
  __syncthreads();
  const int d = tid >> 2, tc = tid & 3, fks = tc >> 1, flhi = tc & 1;
  u16 e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = sv[16 * fks + 4 * flhi + (j & 3) + 8 * (j >> 2)][d];
  uint4 out = make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
  *(uint4*)(vt + tfrag(bh, Tp >> 5, blockIdx.x, fks, d >> 5, flhi, d & 31)) = out;
}

// Workgroup -> (row block, head) with all row blocks of a head on ONE XCD (round-robin dispatch puts consecutive linear ids on different
// XCDs; each XCD has its own L2, so without this every XCD fetches every head's K/V: FETCH_SIZE of vit_attn_bwd was 8x its operands).
__device__ __forceinline__ void head_xcd_remap(int& bx, int& bh) {
  const int nx = gridDim.x;
  const int lin = xcd_remap(blockIdx.x + nx * blockIdx.y, nx * gridDim.y);
  bh = lin / nx;
  bx = lin - bh * nx;
}

template <typename T_>
__global__ __launch_bounds__(64) void attn_d64_kernel(const u16* __restrict__ q, const u16* __restrict__ k,
                                                      const u16* __restrict__ vt, u16* __restrict__ out, int T, int Tp,
                                                      int heads, float scale) {
  const int lane = threadIdx.x, l31 = lane & 31, lhi = lane >> 5;
  int bx, bh;
  head_xcd_remap(bx, bh);
  const int t0 = bx * 32;
  const int ntb = Tp >> 5;
  uint4 qf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf[kk] = *(const uint4*)(q + rfrag(bh, ntb, bx, kk, lhi, l31));

  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m_run = -1e30f, l_run = 0.f;

  for (int s0 = 0; s0 < Tp; s0 += 32) {
    f32x16 sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const uint4 kf = *(const uint4*)(k + rfrag(bh, ntb, s0 >> 5, kk, lhi, l31));
      sacc = T_::mfma32(kf, qf[kk], sacc);
    }
    float mx = -1e30f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int s = s0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      float v = sacc[r] * scale;
      v = s < T ? v : -1e30f;
      sacc[r] = v;
      mx = fmaxf(mx, v);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx);
    const float alpha = __expf(m_run - m_new);
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = __expf(sacc[r] - m_new);
      sacc[r] = p;
      rs += p;
    }
    rs += __shfl_xor(rs, 32);
    l_run = l_run * alpha + rs;
    m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      float pf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = sacc[8 * ks + j];
      const uint4 pfrag = pack8<T_>(pf);
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        const uint4 vf = *(const uint4*)(vt + tfrag(bh, Tp >> 5, s0 >> 5, ks, db, lhi, l31));
        if (db == 0) o0 = T_::mfma32(vf, pfrag, o0);
        else o1 = T_::mfma32(vf, pfrag, o1);
      }
    }
  }
  const int t = t0 + l31;
  if (t < T) {
    const float inv = 1.f / l_run;
    const int n = bh / heads, h = bh - n * heads;
    u16* ob = out + ((int64_t)n * T + t) * (heads * 64) + h * 64 + 4 * lhi;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      *(uint2*)(ob + 8 * g) = pack4<T_>(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
      *(uint2*)(ob + 32 + 8 * g) = pack4<T_>(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
    }
  }
}

}  // namespace

extern "C" int pmi_qkv_split(const void* qkv, void* q, void* k, void* vt, int N, int T, int heads, int order, int dtype,
                             pmi_stream_t s) {
  if (!qkv || !q || !k || !vt || N <= 0 || T <= 0 || heads <= 0 || (order != 0 && order != 1)) return PMI_ERR_ARG;
  const int Tp = (T + 31) / 32 * 32;
  dim3 grid(Tp / 32, N * heads), block(256);
  if (dtype == PMI_DT_BF16) hipLaunchKernelGGL(qkv_split_kernel<BF16>, grid, block, 0, (hipStream_t)s, (const u16*)qkv, (u16*)q, (u16*)k, (u16*)vt, T, Tp, heads, order);
  else hipLaunchKernelGGL(qkv_split_kernel<F16>, grid, block, 0, (hipStream_t)s, (const u16*)qkv, (u16*)q, (u16*)k, (u16*)vt, T, Tp, heads, order);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_attn_d64(const void* q, const void* k, const void* vt, void* out, int N, int T, int heads, float scale,
                            int dtype, pmi_stream_t s) {
  if (!q || !k || !vt || !out || N <= 0 || T <= 0 || heads <= 0) return PMI_ERR_ARG;
  const int Tp = (T + 31) / 32 * 32;
  dim3 grid(Tp / 32, N * heads), block(64);
  if (dtype == PMI_DT_BF16) hipLaunchKernelGGL(attn_d64_kernel<BF16>, grid, block, 0, (hipStream_t)s, (const u16*)q, (const u16*)k, (const u16*)vt, (u16*)out, T, Tp, heads, scale);
  else hipLaunchKernelGGL(attn_d64_kernel<F16>, grid, block, 0, (hipStream_t)s, (const u16*)q, (const u16*)k, (const u16*)vt, (u16*)out, T, Tp, heads, scale);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

// =====================================================================================================================
// ViT attention with backward (head dim 64, any T): forward saves O and the log-sum-exp; backward is two kernels that
// each recompute the 32x32 probability blocks on MFMA (no T x T matrix in HBM, no transposes, no atomics):
//   dq kernel   : one wave per 32-query tile, loops over key tiles    -> dQ
//   dkdv kernel : one wave per 32-key tile,   loops over query tiles  -> dK, dV
// Layouts (all 16-bit, Tp = T rounded up to 32, zero filled): Q,K,V,dO [B*H][Tp/32][fragment order, see rfrag]; Qt,Kt,Vt,dOt [B*H][Tp/32][fragment order, see tfrag];
// lse, delta fp32 [B*H][Tp]  (delta[t] = sum_d dO[t][d] * O[t][d]).
// Replaces nn.MultiheadAttention forward + autograd in the CLIP tower (ruclip/model.py:40-52).
// =====================================================================================================================
namespace {

// qkv [N][T][3C] with channels (which, head, d) -> Q,K,V [bh][Tp][64] and Qt,Kt,Vt in fragment order (tfrag)
template <typename T_>
__global__ __launch_bounds__(256) void vit_qkv_split_kernel(const u16* __restrict__ qkv, u16* __restrict__ q, u16* __restrict__ k,
                                                            u16* __restrict__ v, u16* __restrict__ qt, u16* __restrict__ kt,
                                                            u16* __restrict__ vt, int T, int Tp, int heads) {
  __shared__ u16 s[3][32][72];
  const int tid = threadIdx.x, t0 = blockIdx.x * 32, bh = blockIdx.y;
  const int n = bh / heads, h = bh - n * heads, C = heads * 64;
  const int row = tid >> 3, ch = tid & 7, t = t0 + row;
  u16* dst[3] = {q, k, v};
  u16* dstt[3] = {qt, kt, vt};
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    uint4 val = make_uint4(0, 0, 0, 0);
    if (t < T) val = *(const uint4*)(qkv + ((int64_t)n * T + t) * 3 * C + w * C + h * 64 + ch * 8);
    *(uint4*)(dst[w] + rfrag(bh, Tp >> 5, blockIdx.x, ch >> 1, ch & 1, row)) = val;
    *(uint4*)(&s[w][row][ch * 8]) = val;
  }
  __syncthreads();
  const int d = tid >> 2, tc = tid & 3, fks = tc >> 1, flhi = tc & 1;
#pragma unroll
  for (int w = 0; w < 3; ++w) {
    u16 e[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) e[j] = s[w][16 * fks + 4 * flhi + (j & 3) + 8 * (j >> 2)][d];
    *(uint4*)(dstt[w] + tfrag(bh, Tp >> 5, blockIdx.x, fks, d >> 5, flhi, d & 31)) =
        make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
  }
}

// dO [N][T][C] (head, d) -> dO [bh][Tp][64], dOt [bh][64][Tp], delta[bh][Tp] = sum_d dO*O   (O in [N][T][C])
template <typename T_>
__global__ __launch_bounds__(256) void vit_do_prep_kernel(const u16* __restrict__ dout, const u16* __restrict__ o,
                                                          u16* __restrict__ d_o, u16* __restrict__ d_ot, float* __restrict__ delta,
                                                          int T, int Tp, int heads) {
  __shared__ u16 s[32][72];
  const int tid = threadIdx.x, t0 = blockIdx.x * 32, bh = blockIdx.y;
  const int n = bh / heads, h = bh - n * heads, C = heads * 64;
  const int row = tid >> 3, ch = tid & 7, t = t0 + row;
  uint4 val = make_uint4(0, 0, 0, 0), ov = val;
  if (t < T) {
    val = *(const uint4*)(dout + ((int64_t)n * T + t) * C + h * 64 + ch * 8);
    ov = *(const uint4*)(o + ((int64_t)n * T + t) * C + h * 64 + ch * 8);
  }
  *(uint4*)(d_o + rfrag(bh, Tp >> 5, blockIdx.x, ch >> 1, ch & 1, row)) = val;
  *(uint4*)(&s[row][ch * 8]) = val;
  float a[8], b[8], p = 0.f;
  unpack8<T_>(val, a); unpack8<T_>(ov, b);
#pragma unroll
  for (int e = 0; e < 8; ++e) p += a[e] * b[e];
  p += __shfl_xor(p, 1); p += __shfl_xor(p, 2); p += __shfl_xor(p, 4);
  if (ch == 0) delta[(int64_t)bh * Tp + t] = p;
  __syncthreads();
  const int d = tid >> 2, tc = tid & 3, fks = tc >> 1, flhi = tc & 1;
  u16 e[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) e[j] = s[16 * fks + 4 * flhi + (j & 3) + 8 * (j >> 2)][d];
  *(uint4*)(d_ot + tfrag(bh, Tp >> 5, blockIdx.x, fks, d >> 5, flhi, d & 31)) =
      make_uint4(e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16));
}

// forward: as attn_d64_kernel, plus lse[bh][t] = m + log(l)
template <typename T_>
__global__ __launch_bounds__(64) void vit_attn_fwd_kernel(const u16* __restrict__ q, const u16* __restrict__ k, const u16* __restrict__ vt,
                                                          u16* __restrict__ out, float* __restrict__ lse, int T, int Tp, int heads, float scale) {
  const int lane = threadIdx.x, l31 = lane & 31, lhi = lane >> 5;
  int bx, bh;
  head_xcd_remap(bx, bh);
  const int t0 = bx * 32;
  const int ntb = Tp >> 5;
  uint4 qf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) qf[kk] = *(const uint4*)(q + rfrag(bh, ntb, bx, kk, lhi, l31));
  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m_run = -1e30f, l_run = 0.f;
  struct Tile { uint4 k[4], vt[2][2]; };                 // a key tile's fragments, fetched one tile ahead (see vit_attn_dkdv_body)
  auto load_tile = [&](int sb, Tile& f) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) f.k[kk] = *(const uint4*)(k + rfrag(bh, ntb, sb, kk, lhi, l31));
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int db = 0; db < 2; ++db) f.vt[ks][db] = *(const uint4*)(vt + tfrag(bh, ntb, sb, ks, db, lhi, l31));
  };
  auto compute = [&](const Tile& f, int s0) {
    f32x16 sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) sacc = T_::mfma32(f.k[kk], qf[kk], sacc);
    float mx = -1e30f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int s = s0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      const float v = s < T ? sacc[r] * scale : -1e30f;
      sacc[r] = v; mx = fmaxf(mx, v);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx), alpha = __expf(m_run - m_new);
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { const float p = __expf(sacc[r] - m_new); sacc[r] = p; rs += p; }
    rs += __shfl_xor(rs, 32);
    l_run = l_run * alpha + rs; m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      float pf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = sacc[8 * ks + j];
      const uint4 pfrag = pack8<T_>(pf);
      o0 = T_::mfma32(f.vt[ks][0], pfrag, o0);
      o1 = T_::mfma32(f.vt[ks][1], pfrag, o1);
    }
  };
  Tile ta, tb_;
  load_tile(0, ta);
  for (int sb = 0; sb < ntb; sb += 2) {
    load_tile(sb + 1 < ntb ? sb + 1 : sb, tb_);
    __builtin_amdgcn_sched_barrier(0);
    compute(ta, sb * 32);
    __builtin_amdgcn_sched_barrier(0);
    if (sb + 1 < ntb) {
      load_tile(sb + 2 < ntb ? sb + 2 : sb + 1, ta);
      __builtin_amdgcn_sched_barrier(0);
      compute(tb_, (sb + 1) * 32);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const int t = t0 + l31;
  if (lhi == 0) lse[(int64_t)bh * Tp + t] = t < T ? m_run + __logf(l_run) : 0.f;
  if (t < T) {
    const float inv = 1.f / l_run;
    const int n = bh / heads, h = bh - n * heads;
    u16* ob = out + ((int64_t)n * T + t) * (heads * 64) + h * 64 + 4 * lhi;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      *(uint2*)(ob + 8 * g) = pack4<T_>(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
      *(uint2*)(ob + 32 + 8 * g) = pack4<T_>(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
    }
  }
}

// dQ: wave per 32-query tile.  S^T = K.Q^T and dP^T = V.dO^T put the query on the lane, so lse/delta are lane-local;
// dS^T (accumulator) is the B operand of dQ^T += K^T . dS^T without any movement.
template <typename T_>
__device__ __forceinline__ void vit_attn_dq_body(const u16* __restrict__ q, const u16* __restrict__ k, const u16* __restrict__ v,
                                                 const u16* __restrict__ kt, const u16* __restrict__ d_o,
                                                 const float* __restrict__ lse, const float* __restrict__ delta,
                                                 u16* __restrict__ dqkv, int T, int Tp, int heads, float scale, int bx, int bh) {
  const int lane = threadIdx.x, l31 = lane & 31, lhi = lane >> 5;
  const int t0 = bx * 32;
  const int64_t rb = (int64_t)bh * Tp;
  uint4 qf[4], dof[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    qf[kk] = *(const uint4*)(q + rfrag(bh, Tp >> 5, bx, kk, lhi, l31));
    dof[kk] = *(const uint4*)(d_o + rfrag(bh, Tp >> 5, bx, kk, lhi, l31));
  }
  const float my_lse = lse[rb + t0 + l31], my_delta = delta[rb + t0 + l31];
  f32x16 g0, g1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { g0[r] = 0.f; g1[r] = 0.f; }
  struct Tile { uint4 k[4], v[4], kt[2][2]; };           // a key tile's fragments, fetched one tile ahead (see the dK/dV body)
  const int ntb = Tp >> 5;
  auto load_tile = [&](int sb, Tile& f) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      f.k[kk] = *(const uint4*)(k + rfrag(bh, ntb, sb, kk, lhi, l31));
      f.v[kk] = *(const uint4*)(v + rfrag(bh, ntb, sb, kk, lhi, l31));
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int db = 0; db < 2; ++db) f.kt[ks][db] = *(const uint4*)(kt + tfrag(bh, ntb, sb, ks, db, lhi, l31));
  };
  auto compute = [&](const Tile& f, int s0) {
    f32x16 sacc, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      sacc = T_::mfma32(f.k[kk], qf[kk], sacc);
      dp = T_::mfma32(f.v[kk], dof[kk], dp);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int s = s0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      const float p = s < T ? __expf(sacc[r] * scale - my_lse) : 0.f;
      sacc[r] = p * (dp[r] - my_delta) * scale;                 // dS^T[s][t]
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      float g[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = sacc[8 * ks + j];
      const uint4 dsf = pack8<T_>(g);
      g0 = T_::mfma32(f.kt[ks][0], dsf, g0);
      g1 = T_::mfma32(f.kt[ks][1], dsf, g1);
    }
  };
  Tile ta, tb_;
  load_tile(0, ta);
  for (int sb = 0; sb < ntb; sb += 2) {
    load_tile(sb + 1 < ntb ? sb + 1 : sb, tb_);
    __builtin_amdgcn_sched_barrier(0);
    compute(ta, sb * 32);
    __builtin_amdgcn_sched_barrier(0);
    if (sb + 1 < ntb) {
      load_tile(sb + 2 < ntb ? sb + 2 : sb + 1, ta);
      __builtin_amdgcn_sched_barrier(0);
      compute(tb_, (sb + 1) * 32);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const int t = t0 + l31;
  if (t < T) {
    const int n = bh / heads, h = bh - n * heads, C = heads * 64;
    u16* ob = dqkv + ((int64_t)n * T + t) * 3 * C + h * 64 + 4 * lhi;        // dQ slot
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      *(uint2*)(ob + 8 * g) = pack4<T_>(g0[4 * g], g0[4 * g + 1], g0[4 * g + 2], g0[4 * g + 3]);
      *(uint2*)(ob + 32 + 8 * g) = pack4<T_>(g1[4 * g], g1[4 * g + 1], g1[4 * g + 2], g1[4 * g + 3]);
    }
  }
}

// dK, dV: wave per 32-key tile.  S = Q.K^T and dP = dO.V^T put the key on the lane and the query on the accumulator rows,
// so P and dS are the B operands of dV^T += dO^T . P and dK^T += Q^T . dS.
template <typename T_>
__device__ __forceinline__ void vit_attn_dkdv_body(const u16* __restrict__ q, const u16* __restrict__ k, const u16* __restrict__ v,
                                                   const u16* __restrict__ qt, const u16* __restrict__ d_o, const u16* __restrict__ d_ot,
                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                   u16* __restrict__ dqkv, int T, int Tp, int heads, float scale, int bx, int bh) {
  const int lane = threadIdx.x, l31 = lane & 31, lhi = lane >> 5;
  const int s0 = bx * 32;
  const int64_t rb = (int64_t)bh * Tp;
  uint4 kf[4], vf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    kf[kk] = *(const uint4*)(k + rfrag(bh, Tp >> 5, bx, kk, lhi, l31));
    vf[kk] = *(const uint4*)(v + rfrag(bh, Tp >> 5, bx, kk, lhi, l31));
  }
  const bool key_ok = s0 + l31 < T;
  f32x16 dk0, dk1, dv0, dv1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { dk0[r] = 0.f; dk1[r] = 0.f; dv0[r] = 0.f; dv1[r] = 0.f; }
  // One wave, no LDS: every operand of a query tile comes straight from global memory in fragment order.  The tile's 16 fragment loads and
  // its 32 lse / delta values are fetched ONE TILE AHEAD into a second register set (a 64-thread workgroup has the registers): the loop
  // used to wait a full memory latency per tile with two or three waves per SIMD to cover it.
  struct Tile { uint4 q[4], dO[4], dot[2][2], qt[2][2]; float ls[16], dl[16]; };
  const int ntb = Tp >> 5;
  auto load_tile = [&](int tb, Tile& f) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      f.q[kk] = *(const uint4*)(q + rfrag(bh, ntb, tb, kk, lhi, l31));
      f.dO[kk] = *(const uint4*)(d_o + rfrag(bh, ntb, tb, kk, lhi, l31));
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int db = 0; db < 2; ++db) {
        const int64_t fo = tfrag(bh, ntb, tb, ks, db, lhi, l31);
        f.dot[ks][db] = *(const uint4*)(d_ot + fo); f.qt[ks][db] = *(const uint4*)(qt + fo);
      }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = tb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      f.ls[r] = lse[rb + t]; f.dl[r] = delta[rb + t];
    }
  };
  auto compute = [&](const Tile& f, int t0) {
    f32x16 sacc, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      sacc = T_::mfma32(f.q[kk], kf[kk], sacc);     // rows = queries, lane = key
      dp = T_::mfma32(f.dO[kk], vf[kk], dp);
    }
    float pf[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int t = t0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      const float p = (key_ok && t < T) ? __expf(sacc[r] * scale - f.ls[r]) : 0.f;
      pf[r] = p;
      sacc[r] = p * (dp[r] - f.dl[r]) * scale;            // dS[t][s]
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const uint4 pfrag = pack8<T_>(pf + 8 * ks);
      float g[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = sacc[8 * ks + j];
      const uint4 dsf = pack8<T_>(g);
      dv0 = T_::mfma32(f.dot[ks][0], pfrag, dv0); dk0 = T_::mfma32(f.qt[ks][0], dsf, dk0);
      dv1 = T_::mfma32(f.dot[ks][1], pfrag, dv1); dk1 = T_::mfma32(f.qt[ks][1], dsf, dk1);
    }
  };
  Tile ta, tb_;
  load_tile(0, ta);
  for (int tb = 0; tb < ntb; tb += 2) {                  // two tiles per trip: the register sets swap roles without copies
    load_tile(tb + 1 < ntb ? tb + 1 : tb, tb_);
    __builtin_amdgcn_sched_barrier(0);
    compute(ta, tb * 32);
    __builtin_amdgcn_sched_barrier(0);
    if (tb + 1 < ntb) {
      load_tile(tb + 2 < ntb ? tb + 2 : tb + 1, ta);
      __builtin_amdgcn_sched_barrier(0);
      compute(tb_, (tb + 1) * 32);
      __builtin_amdgcn_sched_barrier(0);
    }
  }
  const int s = s0 + l31;
  if (s < T) {
    const int n = bh / heads, h = bh - n * heads, C = heads * 64;
    u16* okp = dqkv + ((int64_t)n * T + s) * 3 * C + C + h * 64 + 4 * lhi;       // dK slot
    u16* ovp = okp + C;                                                           // dV slot
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      *(uint2*)(okp + 8 * g) = pack4<T_>(dk0[4 * g], dk0[4 * g + 1], dk0[4 * g + 2], dk0[4 * g + 3]);
      *(uint2*)(okp + 32 + 8 * g) = pack4<T_>(dk1[4 * g], dk1[4 * g + 1], dk1[4 * g + 2], dk1[4 * g + 3]);
      *(uint2*)(ovp + 8 * g) = pack4<T_>(dv0[4 * g], dv0[4 * g + 1], dv0[4 * g + 2], dv0[4 * g + 3]);
      *(uint2*)(ovp + 32 + 8 * g) = pack4<T_>(dv1[4 * g], dv1[4 * g + 1], dv1[4 * g + 2], dv1[4 * g + 3]);
    }
  }
}

// dQ and dK/dV of one attention layer in ONE launch (grid.z selects the role): each role alone is 9 x 128 single-wave workgroups
// -- about one wave per SIMD -- and runs latency-bound; issued together the two roles fill each other's stalls.
template <typename T_>
__global__ __launch_bounds__(64) void vit_attn_bwd_kernel(const u16* __restrict__ q, const u16* __restrict__ k, const u16* __restrict__ v,
                                                          const u16* __restrict__ qt, const u16* __restrict__ kt,
                                                          const u16* __restrict__ d_o, const u16* __restrict__ d_ot,
                                                          const float* __restrict__ lse, const float* __restrict__ delta,
                                                          u16* __restrict__ dqkv, int T, int Tp, int heads, float scale) {
  int bx, bh;
  head_xcd_remap(bx, bh);
  if (blockIdx.z == 0) vit_attn_dkdv_body<T_>(q, k, v, qt, d_o, d_ot, lse, delta, dqkv, T, Tp, heads, scale, bx, bh);
  else vit_attn_dq_body<T_>(q, k, v, kt, d_o, lse, delta, dqkv, T, Tp, heads, scale, bx, bh);
}

}  // namespace

// =====================================================================================================================
// LDS-resident route (head dim 64, Tp <= 288: the CLIP ViT towers): one head's whole problem fits a CU's LDS, so a multi-wave workgroup
// per (image, head) loads its operands ONCE with coalesced 16-byte loads and serves every wave's fragments from LDS.  No layout pass:
// the forward's load is also the rfrag-ordered write of Q, K, V, and the transposed operands (V^T, dO^T, Q^T, K^T) are the same row
// images read with ds_read_b64_tr_b16.  Tile order and per-element arithmetic are those of the kernels above, so out, lse and dqkv are
// bit-identical to theirs.
//
// LDS image of a [Tp][64] operand: 32-token tile -> 8 chunk planes of 512 B (chunk = 8 channels = 16 B) -> 32 rows of 16 B, as rfrag, with
// the row XOR-ed by 4 * (chunk & 3).  Row reads (ds_read_b128: one chunk plane, 32 rows) stay conflict-free under the XOR (a permutation
// of 4-row blocks inside the plane); a transposed read's 32-lane half takes 4 rows x 4 chunks (chunk & 3 = 0..3), which the XOR spreads
// over the four 64-byte quarters of the 256-byte bank row instead of stacking them on one (4-way).
// =====================================================================================================================
namespace {

constexpr int VL_MAX_TP = 288;      // 4 images of 288 x 128 B + lse + delta = 149,760 B of the 160 KB
constexpr int VL_FWD_QT = 5;        // query tiles per forward workgroup: a head with more is split over two workgroups (256 CUs, 128 heads)
constexpr int VL_BWD_WAVES = 9;     // VL_MAX_TP / 32: one key tile (dK, dV role) or one query tile (dQ role) per wave

typedef short vl_s4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int vl_off(int t, int ch) {      // byte offset of chunk ch (0..7) of token row t in an image
  return (t >> 5) * 4096 + ch * 512 + (((t & 31) ^ ((ch & 3) << 2)) << 4);
}

// per-lane parts of the fragment addresses
struct VlLane {
  int row0, row1;   // row read, k-step kk even / odd: chunk 2 kk + lhi, row l31
  int tr;           // transposed read: lane 4q + p of a 16-lane group supplies row q, channels 4p .. 4p + 3 of the group's 4 x 16 block
  __device__ __forceinline__ VlLane(int lane) {
    const int l31 = lane & 31, lhi = lane >> 5;
    row0 = lhi * 512 + ((l31 ^ (lhi << 2)) << 4);
    row1 = lhi * 512 + ((l31 ^ ((2 + lhi) << 2)) << 4);
    const int q = (lane >> 2) & 3, p = lane & 3, k = 2 * ((lane >> 4) & 1) + (p >> 1);      // k = chunk & 3
    tr = k * 512 + ((((4 * lhi) ^ (4 * k)) + q) << 4) + 8 * (p & 1);
  }
};

// fragment of k-step kk (channels 16 kk + 8 lhi .. + 7 of row l31) of token tile tb: what rfrag addresses in global memory
__device__ __forceinline__ uint4 vl_row_frag(const unsigned char* img, const VlLane& L, int tb, int kk) {
  return *(const uint4*)(img + tb * 4096 + kk * 1024 + ((kk & 1) ? L.row1 : L.row0));
}
// transposed fragment (channel 32 db + l31; tokens 16 ks + 4 lhi + {0..3, 8..11} of tile tb): what tfrag addresses in global memory
__device__ __forceinline__ uint4 vl_tr_frag(const unsigned char* img, const VlLane& L, int tb, int ks, int db) {
  typedef __attribute__((address_space(3))) vl_s4* lds_s4;
  const unsigned char* p = img + tb * 4096 + db * 2048 + ks * 256;
  const vl_s4 a = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(p + L.tr));
  const vl_s4 b = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4)(p + (L.tr ^ 128)));       // rows + 8: bit 3 of the row, under the XOR too
  const uint2 ua = __builtin_bit_cast(uint2, a), ub = __builtin_bit_cast(uint2, b);
  return make_uint4(ua.x, ua.y, ub.x, ub.y);
}

// forward: grid (ceil(Tp / 32 / 5), N * heads), 5 waves.  Every workgroup stages the head's K and V (zero rows for t >= T); wave w takes
// query tile 5 * blockIdx.x + w with its Q fragments straight from qkv.  Q, K, V go to ws16 parts 0..2 in rfrag order on the way.
template <typename T_>
__global__ __launch_bounds__(VL_FWD_QT * 64) void vit_attn_fwd_lds_kernel(const u16* __restrict__ qkv, u16* __restrict__ wq, u16* __restrict__ wk,
                                                                            u16* __restrict__ wv, u16* __restrict__ out, float* __restrict__ lse,
                                                                            int T, int Tp, int heads, float scale) {
  extern __shared__ __align__(16) unsigned char vl_smem[];
  unsigned char* ki = vl_smem;
  unsigned char* vi = vl_smem + Tp * 128;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  int part, bh;
  head_xcd_remap(part, bh);
  const int n = bh / heads, h = bh - n * heads, C = heads * 64, ntb = Tp >> 5;
  const u16* src = qkv + (int64_t)n * T * 3 * C + h * 64;
  constexpr int NT = VL_FWD_QT * 64, IT = (VL_MAX_TP * 8 + NT - 1) / NT;
  // 64 consecutive items = 8 rows x 8 chunks with the ROW on the low lane bits: 8 neighbouring lanes write 128 contiguous bytes of one chunk
  // plane, in LDS (no bank conflict) and in ws16
  uint4 kr[IT], vr[IT];
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int e = i * NT + tid, t = (e >> 6) * 8 + (e & 7), ch = (e >> 3) & 7;
    const u16* p = src + (int64_t)(t < T ? t : T - 1) * 3 * C + ch * 8;      // always a valid row: the loads need no branch, all are in flight together
    kr[i] = *(const uint4*)(p + C); vr[i] = *(const uint4*)(p + 2 * C);
    if (t >= T) { kr[i] = make_uint4(0, 0, 0, 0); vr[i] = kr[i]; }
  }
  const int bx = part * VL_FWD_QT + wave;
  const bool active = bx < ntb;                            // wave-uniform
  const int t0 = bx * 32;
  uint4 qf[4];
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int t = t0 + l31;
    qf[kk] = *(const uint4*)(src + (int64_t)(t < T ? t : T - 1) * 3 * C + kk * 16 + lhi * 8);
    if (t >= T) qf[kk] = make_uint4(0, 0, 0, 0);
  }
#pragma unroll
  for (int i = 0; i < IT; ++i) {
    const int e = i * NT + tid, t = (e >> 6) * 8 + (e & 7), ch = (e >> 3) & 7;
    if (e < Tp * 8) {
      const int o = vl_off(t, ch);
      *(uint4*)(ki + o) = kr[i]; *(uint4*)(vi + o) = vr[i];
      const int64_t g = rfrag(bh, ntb, t >> 5, ch >> 1, ch & 1, t & 31);
      if (part == 0) *(uint4*)(wk + g) = kr[i];
      if (part == (int)gridDim.x - 1) *(uint4*)(wv + g) = vr[i];
    }
  }
  if (active) {
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) *(uint4*)(wq + rfrag(bh, ntb, bx, kk, lhi, l31)) = qf[kk];
  }
  __syncthreads();
  if (!active) return;
  const VlLane L(lane);
  f32x16 o0, o1;
#pragma unroll
  for (int r = 0; r < 16; ++r) { o0[r] = 0.f; o1[r] = 0.f; }
  float m_run = -1e30f, l_run = 0.f;
  for (int sb = 0; sb < ntb; ++sb) {
    const int s0 = sb * 32;
    f32x16 sacc;
#pragma unroll
    for (int r = 0; r < 16; ++r) sacc[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) sacc = T_::mfma32(vl_row_frag(ki, L, sb, kk), qf[kk], sacc);
    uint4 vt[2][2];
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2)
#pragma unroll
      for (int db = 0; db < 2; ++db) vt[k2][db] = vl_tr_frag(vi, L, sb, k2, db);
    float mx = -1e30f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int s = s0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
      const float v = s < T ? sacc[r] * scale : -1e30f;
      sacc[r] = v; mx = fmaxf(mx, v);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float m_new = fmaxf(m_run, mx), alpha = __expf(m_run - m_new);
    float rs = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) { const float p = __expf(sacc[r] - m_new); sacc[r] = p; rs += p; }
    rs += __shfl_xor(rs, 32);
    l_run = l_run * alpha + rs; m_run = m_new;
#pragma unroll
    for (int r = 0; r < 16; ++r) { o0[r] *= alpha; o1[r] *= alpha; }
#pragma unroll
    for (int k2 = 0; k2 < 2; ++k2) {
      float pf[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) pf[j] = sacc[8 * k2 + j];
      const uint4 pfrag = pack8<T_>(pf);
      o0 = T_::mfma32(vt[k2][0], pfrag, o0);
      o1 = T_::mfma32(vt[k2][1], pfrag, o1);
    }
  }
  const int t = t0 + l31;
  if (lhi == 0) lse[(int64_t)bh * Tp + t] = t < T ? m_run + __logf(l_run) : 0.f;
  if (t < T) {
    const float inv = 1.f / l_run;
    u16* ob = out + ((int64_t)n * T + t) * C + h * 64 + 4 * lhi;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      *(uint2*)(ob + 8 * g) = pack4<T_>(o0[4 * g] * inv, o0[4 * g + 1] * inv, o0[4 * g + 2] * inv, o0[4 * g + 3] * inv);
      *(uint2*)(ob + 32 + 8 * g) = pack4<T_>(o1[4 * g] * inv, o1[4 * g + 1] * inv, o1[4 * g + 2] * inv, o1[4 * g + 3] * inv);
    }
  }
}

// backward: grid (2, N * heads), 9 waves: two workgroups per head, one per role, so 128 heads fill 256 CUs (one workgroup doing both roles
// in turn measured 32.2 us against 24.0).  Both stage Q, K, V from ws16 parts 0..2 (one contiguous block per head), dO from the row-major
// dout, lse from the forward and delta = sum_d dO * O formed while loading (O is not kept); then wave w owns key tile w (role 0: dK, dV over
// all query tiles, the arithmetic of vit_attn_dkdv_body) or query tile w (role 1: dQ over all key tiles, vit_attn_dq_body), every operand
// from LDS.  No atomics: each output element has one owner and a fixed accumulation order.
template <typename T_>
__global__ __launch_bounds__(VL_BWD_WAVES * 64) void vit_attn_bwd_lds_kernel(const u16* __restrict__ wq, const u16* __restrict__ wk,
                                                                            const u16* __restrict__ wv, const u16* __restrict__ dout,
                                                                            const u16* __restrict__ o, const float* __restrict__ lse,
                                                                            u16* __restrict__ dqkv, int T, int Tp, int heads, float scale) {
  extern __shared__ __align__(16) unsigned char vl_smem[];
  unsigned char* qi = vl_smem;
  unsigned char* ki = qi + Tp * 128;
  unsigned char* vi = ki + Tp * 128;
  unsigned char* di = vi + Tp * 128;
  float* ls = (float*)(di + Tp * 128);
  float* dl = ls + Tp;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, lhi = lane >> 5;
  int role, bh;                                           // role 0 = dK, dV, role 1 = dQ; a head's two workgroups run on one XCD
  head_xcd_remap(role, bh);
  const int n = bh / heads, h = bh - n * heads, C = heads * 64, ntb = Tp >> 5;
  constexpr int NT = VL_BWD_WAVES * 64, IT = VL_MAX_TP * 8 / NT;
  static_assert(IT * NT == VL_MAX_TP * 8, "items per thread");
  {
    const uint4* gq = (const uint4*)(wq + (int64_t)bh * Tp * 64);
    const uint4* gk = (const uint4*)(wk + (int64_t)bh * Tp * 64);
    const uint4* gv = (const uint4*)(wv + (int64_t)bh * Tp * 64);
    uint4 a[IT], b[IT], c[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = i * NT + tid, ec = e < Tp * 8 ? e : Tp * 8 - 1;      // clamped, not branched: every load is in flight at once
      a[i] = gq[ec]; b[i] = gk[ec]; c[i] = gv[ec];
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = i * NT + tid;                          // rfrag order: [tile][chunk][row]
      if (e < Tp * 8) {
        const int off = vl_off((e >> 8) * 32 + (e & 31), (e >> 5) & 7);
        *(uint4*)(qi + off) = a[i]; *(uint4*)(ki + off) = b[i]; *(uint4*)(vi + off) = c[i];
      }
    }
  }
  {
    const int64_t base = (int64_t)n * T * C + h * 64;
    uint4 a[IT], b[IT];
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = i * NT + tid, t = (e >> 6) * 8 + (e & 7), ch = (e >> 3) & 7;
      const int64_t g = base + (int64_t)(t < T ? t : T - 1) * C + ch * 8;
      a[i] = *(const uint4*)(dout + g); b[i] = *(const uint4*)(o + g);
      if (t >= T) { a[i] = make_uint4(0, 0, 0, 0); b[i] = a[i]; }
    }
#pragma unroll
    for (int i = 0; i < IT; ++i) {
      const int e = i * NT + tid, t = (e >> 6) * 8 + (e & 7), ch = (e >> 3) & 7;
      if (e < Tp * 8) {                                    // wave-uniform: Tp * 8 is a multiple of 64 and so is NT
        *(uint4*)(di + vl_off(t, ch)) = a[i];
        float x[8], y[8], p = 0.f;
        unpack8<T_>(a[i], x); unpack8<T_>(b[i], y);
#pragma unroll
        for (int j = 0; j < 8; ++j) p += x[j] * y[j];
        p += __shfl_xor(p, 8); p += __shfl_xor(p, 16); p += __shfl_xor(p, 32);      // the row's 8 chunks sit 8 lanes apart
        if (ch == 0) dl[t] = p;
      }
    }
    for (int t = tid; t < Tp; t += NT) ls[t] = lse[(int64_t)bh * Tp + t];
  }
  __syncthreads();
  if (wave >= ntb) return;                                 // wave-uniform, after the only barrier
  const VlLane L(lane);
  const int bx = wave;
  if (role == 0) {  // ---- dK, dV of key tile bx
    // the tile's own K and V fragments are re-read from LDS per query tile (bxo: opaque, so the reads are not hoisted): held in registers
    // (32 more) the loop spills at 3 waves per SIMD
    const bool key_ok = bx * 32 + l31 < T;
    f32x16 dk0, dk1, dv0, dv1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { dk0[r] = 0.f; dk1[r] = 0.f; dv0[r] = 0.f; dv1[r] = 0.f; }
    for (int tb = 0; tb < ntb; ++tb) {
      const int t0 = tb * 32;
      int bxo = bx;
      asm volatile("" : "+v"(bxo));
      f32x16 sacc, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        sacc = T_::mfma32(vl_row_frag(qi, L, tb, kk), vl_row_frag(ki, L, bxo, kk), sacc);     // rows = queries, lane = key
        dp = T_::mfma32(vl_row_frag(di, L, tb, kk), vl_row_frag(vi, L, bxo, kk), dp);
      }
      float pf[16];
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 l4 = *(const float4*)(ls + t0 + 8 * g + 4 * lhi), d4 = *(const float4*)(dl + t0 + 8 * g + 4 * lhi);
        const float lv[4] = {l4.x, l4.y, l4.z, l4.w}, dv[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int r = 4 * g + j, t = t0 + 8 * g + 4 * lhi + j;
          const float p = (key_ok && t < T) ? __expf(sacc[r] * scale - lv[j]) : 0.f;
          pf[r] = p;
          sacc[r] = p * (dp[r] - dv[j]) * scale;            // dS[t][s]
        }
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const uint4 pfrag = pack8<T_>(pf + 8 * ks);
        float g[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = sacc[8 * ks + j];
        const uint4 dsf = pack8<T_>(g);
        dv0 = T_::mfma32(vl_tr_frag(di, L, tb, ks, 0), pfrag, dv0); dk0 = T_::mfma32(vl_tr_frag(qi, L, tb, ks, 0), dsf, dk0);
        dv1 = T_::mfma32(vl_tr_frag(di, L, tb, ks, 1), pfrag, dv1); dk1 = T_::mfma32(vl_tr_frag(qi, L, tb, ks, 1), dsf, dk1);
      }
    }
    const int s = bx * 32 + l31;
    if (s < T) {
      u16* okp = dqkv + ((int64_t)n * T + s) * 3 * C + C + h * 64 + 4 * lhi;       // dK slot
      u16* ovp = okp + C;                                                           // dV slot
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        *(uint2*)(okp + 8 * g) = pack4<T_>(dk0[4 * g], dk0[4 * g + 1], dk0[4 * g + 2], dk0[4 * g + 3]);
        *(uint2*)(okp + 32 + 8 * g) = pack4<T_>(dk1[4 * g], dk1[4 * g + 1], dk1[4 * g + 2], dk1[4 * g + 3]);
        *(uint2*)(ovp + 8 * g) = pack4<T_>(dv0[4 * g], dv0[4 * g + 1], dv0[4 * g + 2], dv0[4 * g + 3]);
        *(uint2*)(ovp + 32 + 8 * g) = pack4<T_>(dv1[4 * g], dv1[4 * g + 1], dv1[4 * g + 2], dv1[4 * g + 3]);
      }
    }
  } else {  // ---- dQ of query tile bx
    uint4 qf[4], dof[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) { qf[kk] = vl_row_frag(qi, L, bx, kk); dof[kk] = vl_row_frag(di, L, bx, kk); }
    const float my_lse = ls[bx * 32 + l31], my_delta = dl[bx * 32 + l31];
    f32x16 g0, g1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { g0[r] = 0.f; g1[r] = 0.f; }
    for (int sb = 0; sb < ntb; ++sb) {
      const int s0 = sb * 32;
      f32x16 sacc, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { sacc[r] = 0.f; dp[r] = 0.f; }
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        sacc = T_::mfma32(vl_row_frag(ki, L, sb, kk), qf[kk], sacc);
        dp = T_::mfma32(vl_row_frag(vi, L, sb, kk), dof[kk], dp);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int s = s0 + (r & 3) + 8 * (r >> 2) + 4 * lhi;
        const float p = s < T ? __expf(sacc[r] * scale - my_lse) : 0.f;
        sacc[r] = p * (dp[r] - my_delta) * scale;                 // dS^T[s][t]
      }
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        float g[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = sacc[8 * ks + j];
        const uint4 dsf = pack8<T_>(g);
        g0 = T_::mfma32(vl_tr_frag(ki, L, sb, ks, 0), dsf, g0);
        g1 = T_::mfma32(vl_tr_frag(ki, L, sb, ks, 1), dsf, g1);
      }
    }
    const int t = bx * 32 + l31;
    if (t < T) {
      u16* ob = dqkv + ((int64_t)n * T + t) * 3 * C + h * 64 + 4 * lhi;        // dQ slot
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        *(uint2*)(ob + 8 * g) = pack4<T_>(g0[4 * g], g0[4 * g + 1], g0[4 * g + 2], g0[4 * g + 3]);
        *(uint2*)(ob + 32 + 8 * g) = pack4<T_>(g1[4 * g], g1[4 * g + 1], g1[4 * g + 2], g1[4 * g + 3]);
      }
    }
  }
}

}  // namespace

static int g_vit_lds = 1;        // A/B switch (pmi_set_option 17): 0 = the fragment-order kernels everywhere, 1 = the LDS-resident kernels where eligible
void pmi_vit_attn_lds(int v) { g_vit_lds = v; }

// THE route rule of pmi_vit_attn_fwd / pmi_vit_attn_bwd (head dim 64): a function of the sequence and the type only, never of N, so a
// shard and its slice of a larger batch take the same kernels.  Forward and backward of one call must see the same option value: the
// LDS forward does not write the transposed workspace parts the fragment-order backward reads.
static bool vit_lds_route(int T, int dtype) {
  return g_vit_lds && (T + 31) / 32 * 32 <= VL_MAX_TP && (dtype == PMI_DT_BF16 || dtype == PMI_DT_F16);
}

// more than 64 KB of dynamic LDS needs the limit raised per kernel and device
template <typename K>
static bool vl_allow_lds(K kern, int bytes) {
  static bool done[64] = {};                               // one flag per kernel instantiation and device
  int dev = 0;
  if (bytes <= 64 * 1024) return true;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
  if (!done[dev]) done[dev] = hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
  return done[dev];
}

#define VIT_BY_DTYPE(KERN, G, B, ...)                                                             \
  do {                                                                                            \
    if (dtype == PMI_DT_BF16) hipLaunchKernelGGL(KERN<BF16>, G, B, 0, (hipStream_t)s, __VA_ARGS__); \
    else hipLaunchKernelGGL(KERN<F16>, G, B, 0, (hipStream_t)s, __VA_ARGS__);                     \
  } while (0)

// launch of an LDS-route kernel with `bytes` of dynamic LDS; false when the LDS limit could not be raised
template <typename K, typename... A>
static bool vl_launch(K kern, dim3 g, int threads, int bytes, pmi_stream_t s, A... args) {
  if (!vl_allow_lds(kern, bytes)) return false;
  hipLaunchKernelGGL(kern, g, dim3(threads), bytes, (hipStream_t)s, args...);
  return true;
}
#define VIT_LDS_LAUNCH(KERN, G, B, BYTES, ...) \
  (dtype == PMI_DT_BF16 ? vl_launch(KERN<BF16>, G, B, BYTES, s, __VA_ARGS__) : vl_launch(KERN<F16>, G, B, BYTES, s, __VA_ARGS__))

extern "C" int pmi_vit_attn_fwd(const void* qkv, void* ws16, float* lse, void* out, int N, int T, int heads, float scale, int dtype,
                                pmi_stream_t s) {
  if (!qkv || !ws16 || !lse || !out || N <= 0 || T <= 0 || heads <= 0) return PMI_ERR_ARG;
  const int Tp = (T + 31) / 32 * 32;
  const int64_t blk = (int64_t)N * heads * Tp * 64;
  u16* w = (u16*)ws16;   // Q, K, V, Qt, Kt, Vt
  if (vit_lds_route(T, dtype)) {   // Q, K, V only: nothing reads the transposed parts on this route
    const bool ok = VIT_LDS_LAUNCH(vit_attn_fwd_lds_kernel, dim3((Tp / 32 + VL_FWD_QT - 1) / VL_FWD_QT, N * heads), VL_FWD_QT * 64, 2 * Tp * 128, (const u16*)qkv,
                                   w, w + blk, w + 2 * blk, (u16*)out, lse, T, Tp, heads, scale);
    if (!ok) return PMI_ERR_LAUNCH;
    PMI_CHECK_LAUNCH();
    return PMI_OK;
  }
  dim3 g(Tp / 32, N * heads);
  VIT_BY_DTYPE(vit_qkv_split_kernel, g, dim3(256), (const u16*)qkv, w, w + blk, w + 2 * blk, w + 3 * blk, w + 4 * blk, w + 5 * blk, T, Tp, heads);
  PMI_CHECK_LAUNCH();
  VIT_BY_DTYPE(vit_attn_fwd_kernel, g, dim3(64), w, w + blk, w + 5 * blk, (u16*)out, lse, T, Tp, heads, scale);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}

extern "C" int pmi_vit_attn_bwd(const void* ws16, const float* lse, const void* o, const void* dout, void* ws16b, float* delta,
                                void* dqkv, int N, int T, int heads, float scale, int dtype, pmi_stream_t s) {
  if (!ws16 || !lse || !o || !dout || !ws16b || !delta || !dqkv || N <= 0 || T <= 0 || heads <= 0) return PMI_ERR_ARG;
  const int Tp = (T + 31) / 32 * 32;
  const int64_t blk = (int64_t)N * heads * Tp * 64;
  const u16* w = (const u16*)ws16;
  u16* wb = (u16*)ws16b;   // dO, dOt
  if (vit_lds_route(T, dtype)) {   // ws16b and delta stay unwritten: dO and delta live in LDS
    const int bytes = 4 * Tp * 128 + 2 * Tp * 4;
    const bool ok = VIT_LDS_LAUNCH(vit_attn_bwd_lds_kernel, dim3(2, N * heads), VL_BWD_WAVES * 64, bytes, w, w + blk, w + 2 * blk, (const u16*)dout, (const u16*)o,
                                   lse, (u16*)dqkv, T, Tp, heads, scale);
    if (!ok) return PMI_ERR_LAUNCH;
    PMI_CHECK_LAUNCH();
    return PMI_OK;
  }
  dim3 g(Tp / 32, N * heads);
  VIT_BY_DTYPE(vit_do_prep_kernel, g, dim3(256), (const u16*)dout, (const u16*)o, wb, wb + blk, delta, T, Tp, heads);
  PMI_CHECK_LAUNCH();
  dim3 g2(Tp / 32, N * heads, 2);
  VIT_BY_DTYPE(vit_attn_bwd_kernel, g2, dim3(64), w, w + blk, w + 2 * blk, w + 3 * blk, w + 4 * blk, wb, wb + blk, lse, delta, (u16*)dqkv, T, Tp,
               heads, scale);
  PMI_CHECK_LAUNCH();
  return PMI_OK;
}
