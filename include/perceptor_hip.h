/* perceptor_hip.h — C ABI of libperceptor_hip.so (gfx950 / MI355X).
 *
 * perceptor itself has no FFI: its hot path is stock PyTorch ops dispatched from
 * Python.  Each entry point below replaces the PyTorch op
 * sequence of the cited reference lines; the Python classes in perceptor_amd/
 * (same names and signatures as the reference's) bind them through ctypes with
 * tensor.data_ptr() and the current HIP stream.
 *
 * Conventions: plain pointers + sizes, caller owns every buffer (including
 * workspaces), no global state, no C++ exceptions; return 0 on success,
 * negative on error (PMI_ERR_ARG = -1 bad argument, PMI_ERR_LAUNCH = -2).
 * All launches are asynchronous on `stream`.  Activations are NHWC
 * ("pixel-major": [N][H*W][C]) 16-bit (dtype 0 = f16, 1 = bf16) unless noted;
 * matrices are row-major with the contraction index contiguous.
 */
#ifndef PERCEPTOR_HIP_H
#define PERCEPTOR_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* pmi_stream_t; /* hipStream_t */

int pmi_abi_version(void);

/* ---- implicit-GEMM convolution / GEMM on MFMA ----------------------------------
 * D[m][n] = act(alpha * sum_k A(m,k) * B[n][k] + bias[n] + nbias[m / hw][n]) + R[m][n]
 * conv mode (taps 9 or 16, stride 2, or up): m = (img, y, x) over the OUTPUT grid H x W,
 * k = tap * Cin + c; A(m,k) gathers pixel (y*stride + dy, x*stride + dx) of the
 * (optionally nearest-2x upsampled) input with zero padding.  taps 9: dy, dx in -1..1
 * (3x3); taps 16 (stride 2 only, Hin = 2H, Win = 2W): dy = tap/4 - 1, dx = tap%4 - 1 in
 * -1..2, the 4x4 window of the input gradient of nearest-x2 + conv3x3 (Upsample2D) with
 * phase-folded weights.  taps 9 with stride 2 and up 2: the input gradient of Downsample2D
 * (pad right / bottom by one, 3x3 stride-2 convolution; stable_diffusion.py:175-192 through
 * vae.encode) by output phase: the input is the low-resolution gradient Hin x Win, H = 2 Hin,
 * W = 2 Win, M = images * H * W; output pixel (2p+a, 2q+b) sums the taps ky = a, kx = b (mod 2)
 * at input pixels (p - ty, q - tx), ty < 2 - a, tx < 2 - b, and B holds the transposed taps
 * phase-major (k offsets 0, 4, 6, 8 taps for the phases 2a + b = 0..3).  One source, no
 * residual / per-sample bias / statistics / split-K / batch in that form.  Channels [0,C0) come
 * from A0, [C0,C0+C1) from A1 (skip-concat without materialising torch.cat).
 * Replaces: nn.Conv2d 3x3 / 1x1 / Conv1d k=1 / nn.Linear / einsum-bmm in
 *   guided_diffusion/unet.py:232-252 (ResBlock), :294-300 (AttentionBlock qkv/proj),
 *   :81-138 (Upsample/Downsample), :462-467 (time_embed), :650-652 (th.cat + conv),
 *   velocity_diffusion/yfcc_2.py:17-28,52-70, cc12m_1.py:19-61, and the CLIP ViT
 *   linears (ruclip/model.py:27-58,72-131) incl. their input-gradient GEMMs.        */
typedef struct {
  const void* A0; const void* A1; const void* B;
  const float* bias;   /* [N] or NULL */
  const float* nbias;  /* [M/hw][N] per-sample bias or NULL */
  const void* R;       /* residual or NULL */
  void* D;
  const float* pro_a;  /* optional fused input prologue x <- pro_act(x * pro_a[img][c] + pro_b[img][c]) (GroupNorm-apply+FiLM+SiLU */
  const float* pro_b;  /* of the consumer's input, zero padding stays zero); only where pmi_conv3x3_halo_config() >= 0 */
  void* ws;            /* split-K workspace: splitk * M * N floats (caller-owned), NULL when splitk <= 1 */
  float* stats;        /* optional: per-channel (sum, sumsq) partials of the OUTPUT, [img][stats_p][N][2] fp32, for the next GroupNorm */
  int32_t M, N, K;     /* K % 8 == 0; N % 4 == 0 unless bias/nbias/R are NULL and ldd >= roundup(N,4) */
  int32_t C0, C1;      /* channel split of the K index (C0 + C1 = Cin) */
  int32_t lda0, lda1;  /* elements between consecutive pixels/rows of A0 / A1 */
  int32_t ldb, ldd, ldr;
  int32_t H, W, Hin, Win; /* conv mode only */
  int32_t taps;        /* 1, 9 or 16 */
  int32_t stride;      /* 1 or 2 */
  int32_t up;          /* 1: nearest x2 upsample of the input (Hin = H/2); 2 (taps 9, stride 2): the phased Downsample2D adjoint */
  int32_t res_up;      /* residual is an [H/2 x W/2] grid read at (y>>1, x>>1): nearest x2 upsample of the skip path */
  int32_t act;         /* PMI_ACT_* */
  int32_t out_f32, res_f32;
  int32_t hw;          /* pixels per sample for nbias (0 if unused) */
  float alpha;
  int32_t batch, batch_inner; /* grid.z batches: z -> (z / batch_inner, z % batch_inner) */
  int64_t sA_o, sA_i, sB_o, sB_i, sD_o, sD_i, sR_o, sR_i; /* element strides */
  int32_t dtype;       /* 0 f16, 1 bf16, 2 precise (f16 MFMA on hi + lo pairs, see split_out) */
  int32_t ldnb;        /* row pitch of nbias (0 = N) */
  int32_t pro_act;     /* activation of the fused prologue */
  int32_t stats_p;     /* partial rows per image = pmi_igemm_stats_rows(); 0 = no statistics */
  int32_t splitk;      /* <= 1: none; else K is split over grid.z and reduced by a second kernel (see pmi_igemm_splitk) */
  int32_t reserved;
  const void* Bf;      /* optional: the same weights in MFMA fragment order for the weights-direct kernels; NULL = not packed.  conv3x3
                        * (csrc/conv_wd.hip): config 4 [N/32][Cin/64][3 dx][4][3 dy][64 lanes][8], configs 6 / 7 (16x16x32 MFMA, ck = 64 / 32)
                        * [N/32][Cin/ck][3 dx][ck/32][3 dy][2][64 lanes][8], config 8 [N/32][ceil(9 Cin / 32)][2][64 lanes][8]; the GEMM
                        * (csrc/gemm_wd.hip): see pmi_gemm_wd_eligible */
  int32_t split_out;   /* "precise" mode (dtype 2): D (and a 16-bit R) hold hi + lo f16 pairs in groups of split_out (32, or 8 / 16 / 24 = N) logical channels,
                        * ldd / ldr count 16-bit elements of the 2N-wide rows; 0 = plain.  A split INPUT needs no flag: it is a tensor with 2 Cin
                        * channels whose weights are duplicated along K by the caller.  Generic kernel only (no LDS-halo config). */
  int32_t split_in;    /* 1: the inputs are precise (hi + lo) tensors whose 2 Cin physical channels are the K dimension (C0 / C1 / K count them; weights
                        *    duplicated along K).  A fused prologue is taken by the weights-direct conv3x3 configs 6 / 7 only: they stage (hi, lo) PAIRS,
                        *    apply it to the value hi + lo and split the result again (chunk K order [yh of ck/2 channels | their yl]: Bf packed so).
                        * 2: mixed mode, single operand: the inputs are hi + lo tensors but C0 / C1 / K count LOGICAL channels; the fused prologue
                        *    (required) rounds act((hi + lo) * a + b) once to f16: plain weights, plain K loop.  Configs 6 / 7 only. */
  /* fused epilogue extras of the weights-direct GEMM (pmi_gemm_wd_eligible() == 1, 16-bit output, no split-K), the MLP of the CLIP tower
   * (ruclip/model.py:27-58) and its input gradient: */
  void* D2;            /* optional second output [M][ldd] 16-bit: the PRE-activation value (c_fc output kept for the backward pass) */
  const void* aux;     /* optional [M][ldd] 16-bit: the output is multiplied by act'(aux) with act = aux_act (dh * gelu'(h_pre) of the c_proj input gradient) */
  int32_t aux_act;
  int32_t reserved3;   /* 1: split-K weights-direct GEMM, the caller consumes the raw slabs; 2: Bf holds no phase weights -- an up-sampling conv3x3 stays off tile config 9 */
} pmi_igemm_args;
int pmi_igemm(const pmi_igemm_args* a, pmi_stream_t stream);
/* >= 0 when an LDS-halo conv3x3 kernel takes this shape.  csrc/conv3x3.hip: tile config 0: 8x32 px x 256 ch, 1: 16x32 x 128, 2: 8x32 x 128 with two
 * workgroups per CU, 3: 8x32 px x <= 32 output channels (also a split input with fp32 output, N <= 32: a plain K over the 2 Cin physical
 * channels); csrc/conv_wd.hip (weights-direct, needs Bf != NULL): 4: 8x32 px x 256 ch (32x32x16 MFMA), 6: 8x32 px x 256 ch (16x16x32 MFMA,
 * 64-channel chunks), 7: 8x32 px x 128 ch (16x16x32, 32-channel chunks, also a masked Cout tail), 8: at most 32 input channels, one source,
 * the whole K in registers; csrc/conv_up_wd.hip: 9: up = 1 by output phase -- four 2x2 convolutions on the low-resolution grid, 8x32 low-resolution
 * positions x one phase x 256 ch, Bf = [N/32][phase 2a + b][Cin/64][2 dx][2][2 dy][2][64 lanes][8] with the tap sums a = 0: w0 | w1 + w2, a = 1: w0 + w1 | w2
 * per axis (one source, no residual / output activation, N % 256 == 0, Win % 32 == 0, Hin % 8 == 0; the MFMA work issued is 4/9 of the algorithmic
 * 9-tap FLOP).  Split (precise / mixed) outputs take configs 6 / 7 / 8 only.  -1 when pmi_igemm uses the generic implicit-GEMM
 * kernel (which has no fused prologue). */
int pmi_conv3x3_halo_config(const pmi_igemm_args* a);
/* 1 when the weights-direct GEMM (csrc/gemm_wd.hip) takes this call: plain GEMM (taps 1, one source, no per-sample bias / statistics / prologue),
 * K % 128 == 0, N % 256 == 0 and Bf = the weights in its fragment order [N/32][K/128][4][2][64 lanes][8] */
int pmi_gemm_wd_eligible(const pmi_igemm_args* a);
/* tile of the weights-direct GEMM launch for these arguments (splitk as it will be passed): rows * 1000 + columns (128 / 144 rows, 128 / 256 columns) */
int pmi_gemm_wd_tile(const pmi_igemm_args* a);
/* split-K factor recommended for this shape (1 = none); with splitk = S the caller passes ws = S*M*N floats */
int pmi_igemm_splitk(const pmi_igemm_args* a);
/* number of per-image partial rows the fused output statistics of this call would produce (0: not available for this shape) */
int pmi_igemm_stats_rows(const pmi_igemm_args* a);
/* debugging / A-B switches: key 0 = allow the LDS-halo conv3x3 kernel (default 1, returns the previous value);
 * key 1 = force a conv3x3 tile config where eligible (-1 = automatic; 6 / 7 keep up-sampling convolutions on the gather route, 9 puts them on the phased one);
 * key 2 = prefer the 8-wave 256-channel halo config over two 4-wave workgroups per CU where the grid allows (default 1);
 * key 6 = allow the weights-direct conv3x3 kernel (default 1); key 7 = its 16x16x32-MFMA form, tile config 6, instead of config 4 (default 1);
 * key 8 = allow its 128-channel form, tile config 7 (4 waves, two workgroups per CU), for Cout % 256 != 0 (default 1);
 * key 13 = allow its first-convolution form, tile config 8 (at most 32 input channels, the whole K in registers) (default 1);
 * key 9 = query-tile rows per wave of pmi_attn_flash (0 = automatic); key 10 = allow split-K in the weights-direct conv3x3 (default 1);
 * key 11 = largest split-K factor of the weights-direct GEMM (default 8); key 12 = workgroup count below which that GEMM uses its
 * 128-column tiles (default 128); key 14 = most query chunks per key tile of pmi_attn_flash_bwd_kv (0 = automatic, 1 = the unsplit key role);
 * key 15 = allow tile config 9, up-sampling conv3x3 by output phase (default 1; 0: the gather route of configs 6 / 7 takes them).
 * key 16 = allow the fused conv2 + skip launch, pmi_conv3x3_skip (default 1; 0: pmi_conv3x3_skip_eligible answers 0 and callers keep the skip GEMM).
 * key 17 = allow the LDS-resident kernels of pmi_vit_attn_fwd / pmi_vit_attn_bwd (head dim 64, T <= 288: one workgroup per image and head,
 * no layout passes) (default 1; 0: the fragment-order kernels take every shape).  The route is a function of (T, dtype) only; a call's forward
 * and backward must run under the same value, as the LDS forward writes only the Q, K, V parts of its workspace.
 * `python bench.py --opt "k=v,..."` sets them for a same-box A/B.
 * The library links no vendor GEMM / BLAS: every kernel it launches is in csrc/. */
int pmi_set_option(int key, int value);

/* ---- ResBlock conv2 with the two-source 1x1 skip convolution folded into its K loop ----------------------------------------------
 * D = conv3x3(silu(pro_a * h + pro_b)) + Wf * (X0 | X1) + bias: `a` describes the 3x3 convolution over h exactly as for pmi_igemm
 * (fragment-ordered Bf, fused SiLU prologue, R = NULL, bias = conv2's bias + the skip convolution's, summed in fp32 by the caller); the
 * skip product is accumulated in the same fp32 accumulators before the epilogue, so its own output tensor, its read-back as the residual
 * and one rounding to 16 bits disappear; output statistics see conv + skip.  X0 [M][ld0], X1 [M][ld1] (or NULL, C1 = 0): the block's raw
 * input on the OUTPUT grid H x W, C0 / C1 multiples of 64; Wf: the [N][C0 + C1] skip weights in fragment order
 * [N/32][(C0 + C1)/32][16-channel block (2)][lane = 16*(k quarter) + channel][8 k].
 * Replaces: guided_diffusion/unet.py:232-252 ResBlock `self.skip_connection(x) + h` with x = th.cat([h, hs.pop()], dim=1) of :650-652.
 * pmi_conv3x3_skip_eligible: the tile config (6 or 7, non-zero) pmi_conv3x3_skip runs the call in -- the caller packs Bf for it (any non-NULL
 * Bf for the query) -- or 0: f16 / bf16, SiLU prologue, alpha = 1, no output activation, no residual / res_up / up / split-K / split (mixed,
 * precise) tensors / fp32 output, 16-byte aligned pointers; N % 256 == 0 takes the 256-channel tiles (config 6), any other N % 128 == 0 the
 * 128-channel tiles (config 7), bf16 only.  Answer and config are functions of the layer and the map, never of the number of images: a fused
 * launch is never split along K.  pmi_conv3x3_skip returns PMI_ERR_ARG where the query answers 0, without a launch. */
typedef struct {
  const void* X0; const void* X1; const void* Wf;
  int32_t C0, C1;      /* channels of X0 / X1 */
  int32_t ld0, ld1;    /* elements between consecutive pixels of X0 / X1 */
} pmi_skip_args;
int pmi_conv3x3_skip_eligible(const pmi_igemm_args* a, const pmi_skip_args* k);
int pmi_conv3x3_skip(const pmi_igemm_args* a, const pmi_skip_args* k, pmi_stream_t stream);

/* ---- "precise" mode helpers (dtype 2: hi + lo f16 pairs, eps max-abs error < 1e-3 vs the fp32 reference path) ----------------
 * exact-fp32 batched GEMM on the f32-input MFMA: D[b][m][n] = act(alpha * sum_k A[b][m][k] * B[b][n][k] + bias[n]); transB: B is [k][n]; transA: A is
 * [k][m] (the attention backward's P^T dO and dS^T Q).
 * Replaces the attention einsums of unet.py:332-348 / yfcc_2.py:62-70 and the time MLPs (unet.py:462-467) in that mode. */
typedef struct {
  const float* A; const float* B; const float* bias; float* D;
  int32_t M, N, K, lda, ldb, ldd;
  int32_t transB, act;
  float alpha;
  int32_t batch, batch_inner;          /* grid.z batches: z -> (z / batch_inner, z % batch_inner) */
  int64_t sA_o, sA_i, sB_o, sB_i, sD_o, sD_i;
  const float* R;                      /* optional residual added after the activation, laid out like D */
  int32_t transA;                      /* appended last: a caller must zero-initialise the struct (lda >= M when set, >= K otherwise) */
} pmi_gemm_f32_args;
int pmi_gemm_f32(const pmi_gemm_f32_args* a, pmi_stream_t stream);
int pmi_softmax_f32(float* S, int rows, int T, int ld, float scale, pmi_stream_t s);   /* in place, fp32 (unet.py:346) */
/* in place on dP: dS = scale * P o (dP - rowsum(dP o P)), fp32 rows -- what autograd forms for the softmax of unet.py:346 / yfcc_2.py:67 */
int pmi_softmax_bwd_f32(float* dP, const float* P, int rows, int T, int ld, float scale, pmi_stream_t s);
/* fp32 [rows][C] (row pitch ld_in) <-> precise [rows][2C] */
int pmi_split_from_f32(const float* in, int ld_in, void* out, int64_t rows, int C, pmi_stream_t s);
int pmi_split_to_f32(const void* in, float* out, int64_t rows, int C, pmi_stream_t s);
/* plain f16 [rows][C] <-> precise [rows][2C] (to_split 1: low parts zero; 0: hi + lo rounded once): the level boundaries of the mixed mode,
 * where unet.py:626-654's tensors change between the two storage forms */
int pmi_split_convert(const void* in, void* out, int64_t rows, int C, int to_split, pmi_stream_t s);

/* ---- GroupNorm (+FiLM, +activation, +2x2 average pool) ---------------------------
 * unet.py:232-252 / nn.py:17-19 (GroupNorm32 -> SiLU, FiLM h*(1+scale)+shift),
 * yfcc_2.py:56 (GroupNorm(1,C)), cc12m_1.py:33-61 (GroupNorm(1,C,affine=False) + Modulation2d + ReLU).
 * stats: partial sums per (sample, pixel-chunk, channel) -> ws[N][nchunk][C][2] (fp32)
 * finalize: coefficients a[n][c], b[n][c] so that y = act(x * a + b)
 * apply: y (optionally 2x2 average-pooled after the activation)                      */
/* x1/C0: optional second source: channels [0,C0) from x, [C0,C) from x1 (normalising a skip-concat, unet.py:650-652,
 * without materialising it); pass x1 = NULL, C0 = C otherwise. */
int pmi_gn_stats(const void* x, const void* x1, int C0, float* ws, int N, int HW, int C, int G, int nchunk, int dtype, pmi_stream_t s);
/* finalize from per-CHANNEL partials s0[N][P0][C0][2] (and optionally s1[N][P1][C1][2] for the second half of a concat):
 * the layout pmi_gn_stats and the fused statistics epilogue of pmi_igemm both write. */
int pmi_gn_finalize(const float* s0, int P0, int C0, const float* s1, int P1, int C1, const float* gamma, const float* beta,
                    const float* film, int film_ld, float* coef_a, float* coef_b, int N, int HW, int G, float eps, pmi_stream_t s);
/* res: optional 16-bit NHWC tensor added after the activation (cc12m_1.py:46-61: relu(mod(norm(conv))) + skip) */
int pmi_gn_apply(const void* x, const void* x1, int C0, const float* coef_a, const float* coef_b, const void* res, void* y, int N, int H, int W, int C,
                 int act, int pool, int dtype, pmi_stream_t s);
/* the down ResBlock's two pooled tensors from ONE pass over x (unet.py:232-243: h = AvgPool(SiLU(GN(x))), skip = AvgPool(x)) */
int pmi_gn_apply_pool_skip(const void* x, const float* coef_a, const float* coef_b, void* y, void* y_raw, int N, int H, int W, int C, int act,
                           int dtype, pmi_stream_t s);

/* ---- attention, head dim 64 (flash-style, MFMA) -----------------------------------
 * unet.py:332-348 (QKVAttentionLegacy), :364-382 (QKVAttention), yfcc_2.py:62-70.
 * qkv_split re-tiles the qkv 1x1-conv output [N][T][3C] into Q,K [N*heads][Tp][64]
 * and V^T [N*heads][64][Tp] (Tp = T rounded up to 32, zero filled).
 * order: 0 = heads then q,k,v (legacy), 1 = q,k,v then heads (new order and v-diffusion). */
/* Flash-style attention for head dims 8..160 (multiples of 8) with a separate key / value sequence: the StableDiffusion transformer
 * blocks' self- and cross-attention (stable_diffusion/attention.py:268-298, replaces the xformers call at :285).
 * q [N][T][ldq], k and v [N][Tk][ldkv] 16-bit with head h at channel offset h*d of each pointer; out [N][T][heads*d];
 * ws: caller-owned scratch of pmi_attn_flash_workspace(...) KiB (operands re-tiled into MFMA fragment order; < 0: unsupported). */
int pmi_attn_flash_workspace(int N, int T, int Tk, int heads, int d);
int pmi_attn_flash(const void* q, int ldq, const void* k, const void* v, int ldkv, void* out, void* ws, int N, int T, int Tk, int heads,
                   int d, float scale, int dtype, pmi_stream_t s);
/* The same with an input gradient: what autograd forms upstream when a loss on the predicted noise reaches the latents through the
 * transformer blocks' attention (stable_diffusion/attention.py:268-298 under stable_diffusion.py:259-271).
 * pmi_attn_flash_train = pmi_attn_flash (same kernels, same output bits) that also writes lse[N*heads][Tp] fp32, Tp = T rounded up to 32,
 * in the EXP2 domain: lse = log2 sum_s exp2(S[t][s] scale log2 e) (0 for the rows t >= T), and leaves the Q / K fragments in ws.
 * pmi_attn_flash_bwd recomputes P = exp2(S scale log2 e - lse) per 32 x 32 tile: dP = dO V^T, dS = P o (dP - delta) scale, dQ = dS K,
 * dK = dS^T Q, dV = P^T dO, delta[t] = sum_c dO[t][c] O[t][c] (written to delta[N*heads][Tp] by its first pass).  out / dout [N][T][heads*d];
 * ws: the forward's; ws_bwd: pmi_attn_flash_bwd_workspace(...) KiB; dq [N][T][lddq], dk / dv [N][Tk][lddkv], head h at channel offset h*d
 * (self-attention: three slices of d qkv [N][T][3C]).  dq_only = 1 (cross-attention: k, v come from the frozen prompt encodings,
 * conditioning.py:16): only dq is written, dk / dv may be NULL.  No atomics: results are run-to-run bit-identical. */
int pmi_attn_flash_train(const void* q, int ldq, const void* k, const void* v, int ldkv, void* out, void* ws, float* lse, int N, int T, int Tk,
                         int heads, int d, float scale, int dtype, pmi_stream_t s);
int pmi_attn_flash_bwd_workspace(int N, int T, int Tk, int heads, int d, int dq_only);
int pmi_attn_flash_bwd(const void* q, int ldq, const void* k, const void* v, int ldkv, const void* out, const void* dout, const void* ws,
                       const float* lse, void* ws_bwd, float* delta, void* dq, int lddq, void* dk, void* dv, int lddkv, int N, int T, int Tk,
                       int heads, int d, float scale, int dq_only, int dtype, pmi_stream_t s);
/* Cross-attention with a differentiable prompt (conditioning.encodings.requires_grad_(), stable_diffusion.py:259-271): dq as
 * pmi_attn_flash_bwd(dq_only = 1) writes it, bit for bit, and dk / dv [N][Tk][lddkv] in FP32 (16-byte aligned, lddkv % 4 == 0), head h at
 * channel offset h*d.  For Tk << T one wave per key tile would walk all of T alone: the query tiles are cut into
 * S = pmi_attn_flash_bwd_kv_chunks(...) chunks, a function of the shape only; every (key tile, chunk) leaves an fp32 partial tile in ws_bwd
 * and a second launch adds the S partials of each element in chunk order.  No atomics: run-to-run bit-identical.
 * ws_bwd: pmi_attn_flash_bwd_kv_workspace(...) KiB.  S follows pmi_set_option key 14: the option must not change between the
 * workspace query and the launch it sizes (a larger S would write partial tiles past the workspace). */
int pmi_attn_flash_bwd_kv_chunks(int N, int T, int Tk, int heads, int d);
int pmi_attn_flash_bwd_kv_workspace(int N, int T, int Tk, int heads, int d);
int pmi_attn_flash_bwd_kv(const void* q, int ldq, const void* k, const void* v, int ldkv, const void* out, const void* dout, const void* ws,
                          const float* lse, void* ws_bwd, float* delta, void* dq, int lddq, float* dk, float* dv, int lddkv, int N, int T,
                          int Tk, int heads, int d, float scale, int dtype, pmi_stream_t s);
int pmi_qkv_split(const void* qkv, void* q, void* k, void* vt, int N, int T, int heads, int order, int dtype, pmi_stream_t s);
int pmi_attn_d64(const void* q, const void* k, const void* vt, void* out, int N, int T, int heads, float scale,
                 int dtype, pmi_stream_t s);

/* ViT attention with input-gradient (head dim 64, any T; nn.MultiheadAttention in ruclip/model.py:40-52), flash style:
 * fwd: qkv [N][T][3C] with channels (q|k|v, head, d) -> out [N][T][C]; saves ws16 = 6 x [N*heads][Tp][64] 16-bit
 *      (Q,K,V and their transposes, Tp = T rounded up to 32) and lse [N*heads][Tp] fp32 for the backward.
 * bwd: dout [N][T][C] -> dqkv [N][T][3C]; needs o (= fwd out), ws16b = 2 x [N*heads][Tp][64] 16-bit and delta [N*heads][Tp] fp32 scratch. */
int pmi_vit_attn_fwd(const void* qkv, void* ws16, float* lse, void* out, int N, int T, int heads, float scale, int dtype, pmi_stream_t s);
int pmi_vit_attn_bwd(const void* ws16, const float* lse, const void* o, const void* dout, void* ws16b, float* delta, void* dqkv,
                     int N, int T, int heads, float scale, int dtype, pmi_stream_t s);

/* ---- layout / elementwise on the UNet path -----------------------------------------
 * prep: images NCHW fp32 in [0,1] -> x = 2*img-1 (diffusion_space.py:1-2) as NHWC 16-bit with
 *       Cpad channels; channels [3, 3+nplanes) are per-sample constants planes[n][j]
 *       (yfcc_2.py:73-74,247-249 expand_to_planes of the Fourier timestep features).
 * finish: NHWC (fp32, ld channels) -> NCHW fp32 first `cout` channels (guided_diffusion.py:125-133 [:, :3].float()) */
int pmi_prep_input(const float* img, const float* planes, int nplanes, void* x, int N, int H, int W, int Cpad, int dtype, pmi_stream_t s);
int pmi_finish_output(const float* y, int ld, float* out, int N, int H, int W, int cout, pmi_stream_t s);
/* StableDiffusion latents / VAE (models/stable_diffusion/stable_diffusion.py:194-198,259-271): generic NCHW fp32 <-> NHWC layout
 * conversion with an affine map (x*mul + add: the 1/0.18215 latent scale, diffusion_space.decode's (x+1)/2), and the GEGLU
 * gate of the transformer blocks' feed-forward (stable_diffusion/attention.py:346-348): h[M][2F] = (value | gate) -> value*gelu(gate);
 * interleaved = 1: h holds 16 value then 16 gate columns per 32 (the column order of weights packed for pmi_igemm's act = 5 = GEGLU
 * epilogue, which writes value*gelu(gate) directly -- N / 2 output columns, weights-direct GEMM only -- and makes this pass unnecessary). */
int pmi_nchw_to_nhwc(const float* in, void* x, int N, int C, int H, int W, int Cpad, float mul, float add, int dtype, pmi_stream_t s);
int pmi_nhwc_to_nchw(const float* y, int ld, float* out, int N, int H, int W, int cout, float mul, float add, pmi_stream_t s);
int pmi_geglu(const void* h, void* out, int64_t M, int F, int interleaved, int dtype, pmi_stream_t s);
/* GEGLU backward (autograd through stable_diffusion/attention.py:346-348): from the kept h[M][2F] and dg[M][F] = d loss / d output,
 * dh[M][2F] in h's column order: d value = dg gelu(gate), d gate = dg value gelu'(gate) (erf GELU). */
int pmi_geglu_bwd(const void* h, const void* dg, void* dh, int64_t M, int F, int interleaved, int dtype, pmi_stream_t s);
int pmi_avgpool2(const void* x, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s);            /* nn.AvgPool2d(2) */
int pmi_upsample_bilinear2(const void* x, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s);  /* align_corners=False */
int pmi_upsample_nearest2(const void* x, void* y, int N, int H, int W, int C, pmi_stream_t s);              /* nn.Upsample(2, 'nearest'), 16-bit NHWC */
/* nn.py:101-118 sinusoidal embedding [cos|sin] -> 16-bit [N][dim] */
int pmi_timestep_embedding(const float* t, void* out, int N, int dim, float max_period, int dtype, pmi_stream_t s);
/* yfcc_2.py:41-49 Fourier features: out[n] = [cos(2 pi t w_j) | sin(2 pi t w_j)] fp32 */
int pmi_fourier_features(const float* t, const float* w, float* out, int N, int half, pmi_stream_t s);
int pmi_cast_f32_to_16(const float* in, void* out, int64_t n, int act, int dtype, pmi_stream_t s);

/* ---- sampler updates (fp32, NCHW, per-sample scalars) -------------------------------
 * guided_diffusion/predictions.py:51-59,61-98 ; velocity_diffusion/predictions.py:50-62,68-105 ;
 * guided: predictions.py:147-154 (both forms): p += scale * sigma_from * clamp(g,+-c)/c          */
int pmi_ddim_eps_step(const float* img, const float* eps, const float* a_from, const float* s_from,
                      const float* a_to, const float* s_to, float* next_img, float* denoised_img,
                      int N, int64_t chw, pmi_stream_t s);
int pmi_ddim_v_step(const float* img, const float* v, const float* a_from, const float* s_from,
                    const float* a_to, const float* s_to, float* next_img, float* denoised_img,
                    int N, int64_t chw, pmi_stream_t s);
int pmi_guided_update(const float* pred, const float* grad, const float* s_from, float scale, float clamp_value,
                      float* out, int N, int64_t chw, pmi_stream_t s);

/* remaining Predictions algebra (predictions.py:101-145,174-179 ; velocity_diffusion/predictions.py:107-200):
 * out = ca[n]*a + cb[n]*b + cc[n] with per-sample coefficients (b, cb, cc optional); clamp with per-sample bounds, Tensor.clamp's
 * values: a NaN input stays NaN */
int pmi_lincomb2(const float* a, const float* b, const float* ca, const float* cb, const float* cc, float* out, int N,
                 int64_t chw, pmi_stream_t s);
int pmi_clamp(const float* a, const float* lo, const float* hi, float* out, int N, int64_t chw, pmi_stream_t s);

/* ---- Predictions variants and clamp_with_grad (csrc/sampling.hip), fp32, one row per sample ------------------
 * pmi_quantile_abs: out[n] = torch.quantile(|x[n, :]|, q) (linear interpolation; equal order statistics are returned as they are, so q = 1 is
 *   the row's max |x| also when that is inf), radix select -- replaces the quantile in
 *   Predictions.dynamic_threshold (guided_diffusion/predictions.py:156-172 ; velocity_diffusion/predictions.py:148-164).
 * pmi_randn: standard-normal noise for step(eta>0) / resample_noise / noisy_reverse_step (predictions.py:61-98,126-145), replacing
 *   torch.randn_like.  Philox4x32-10 + Box-Muller; element e of the draw (seed, stream) is a function of (seed, stream,
 *   first_element + e) only, so a rank that holds samples [r0, r1) of a batch passes first_element = r0 * chw and gets the same values
 *   as a single process.  pmi_philox4x32_10 exposes the raw generator for known-answer tests.
 * pmi_sort_rows / pmi_wasserstein: Predictions.wasserstein_distance / wasserstein_square_distance (predictions.py:184-198):
 *   rows sorted ascending into work[rows][pmi_sort_rows_padded(n)] (bitonic network, +inf padding), then
 *   out[0] = mean |sorted - Normal(0,1).icdf(linspace(0.5/n, 1-0.5/n, n))|^power (power 1 or 2); partial = 1024 floats of workspace.
 * pmi_clamp_grad: backward of clamp_with_grad (transforms/clamp_with_grad.py:8-23) with per-sample bounds:
 *   out = grad * (grad * (x - clamp(x, lo, hi)) >= 0), the mask multiplied as there: a NaN gradient stays NaN, a blocked infinite one is NaN. */
int pmi_quantile_abs(const float* x, float* out, int N, int64_t n, float q, pmi_stream_t s);
int pmi_randn(float* out, int64_t n, int64_t first_element, int64_t seed_bits, int64_t stream_bits, pmi_stream_t s);
int pmi_philox4x32_10(uint32_t* out4, int64_t counter_lo, int64_t counter_hi, int64_t key, pmi_stream_t s);
int pmi_sort_rows_padded(int64_t n);
int pmi_sort_rows(const float* x, float* work, int rows, int64_t n, pmi_stream_t s);
int pmi_wasserstein(const float* sorted, int rows, int64_t n, int power, float* partial, float* out, pmi_stream_t s);
int pmi_clamp_grad(const float* x, const float* grad, const float* lo, const float* hi, float* out, int N, int64_t chw, pmi_stream_t s);

/* ---- input-gradient of the v-diffusion UNets (csrc/backward.hip) --------------------------------------------
 * What autograd computes upstream when losses/velocity_diffusion.py:33-61 (guided_resample_) backpropagates a loss on the denoised
 * image to the noise.  dX of every convolution is pmi_igemm on flipped / transposed packed weights and the attention backward is
 * pmi_vit_attn_bwd; these are the memory-bound adjoints between them (16-bit NHWC, dtype 0 / 1):
 * pmi_add16: out = a + b (ResConvBlock main + skip, yfcc_2.py:17-28, when the ReLU output must survive for its mask);
 * pmi_avgpool2_bwd: dy [N][H/2][W/2][C] -> dx [N][H][W][C] (nn.AvgPool2d(2)); pmi_upsample_bilinear2_bwd: dy [N][2H][2W][C] -> dx
 * [N][H][W][C] (exact adjoint of pmi_upsample_bilinear2); pmi_gn1_bwd: GroupNorm(1, C) with affine, dx = r (g - mean g - xhat mean(g xhat))
 * (+ res), g = (gamma[n * gamma_ld + c] + gamma_add) dy: gamma_ld = 0 for a shared affine weight (SelfAttention2d.norm, yfcc_2.py:41-52),
 * > 0 with gamma_add = 1 for Modulation2d's per-sample scale after GroupNorm(1, C, affine=False) (cc12m_1.py:33-61); two launches
 * (slice sums into `partial`, then every workgroup adds the slices in index order and streams its part): deterministic.                       */
int pmi_add16(const void* a, const void* b, void* out, int64_t n, int dtype, pmi_stream_t s);
int pmi_avgpool2_bwd(const void* dy, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_upsample_bilinear2_bwd(const void* dy, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_upsample_nearest2_bwd(const void* dy, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s);   /* wikiart_256.py:117 */
/* GroupNorm32 (+FiLM) + activation backward of the ADM UNet (unet.py:232-252 out_layers / in_layers, nn.py:17-19; the gradient autograd forms
 * when GuidedDiffusion.predicted_noise is differentiated, guided_diffusion.py:125-133).  The forward is y = act(a x + b) with pmi_gn_finalize's
 * coefficients; stats: per-channel partials of dt = dy act'(a x + b) and dt x, ws [N][nchunk][C][2]; finalize: from the FORWARD partials s0 / s1
 * (as given to pmi_gn_finalize) and those, P / Q per channel; apply: dx = a dt + P x + Q (+ gadd), one output per concat source. */
int pmi_gn_bwd_stats(const void* x, const void* x1, int C0, const void* dy, const float* coef_a, const float* coef_b, int act, float* ws,
                     int N, int HW, int C, int nchunk, int dtype, pmi_stream_t s);
int pmi_gn_bwd_finalize(const float* s0, int P0, int C0, const float* s1, int P1, int C1, const float* ws_bwd, int PB, const float* gamma,
                        const float* film, int film_ld, float* coef_p, float* coef_q, int N, int HW, int G, float eps, pmi_stream_t s);
int pmi_gn_bwd_apply(const void* x, const void* x1, int C0, const void* dy, const float* coef_a, const float* coef_b, const float* coef_p,
                     const float* coef_q, int act, const void* gadd0, const void* gadd1, void* dx0, void* dx1, int N, int HW, int C,
                     int dtype, pmi_stream_t s);
/* The same adjoints over precise tensors (PMI_DT_F16X2: [rows][C/G][hi G | lo G]; C = logical channels, a multiple of 32 or of 8 up to 32).
 * Both halves are added on load, the arithmetic is fp32, the result is split again on store.  They give the precise mode the input gradient
 * autograd provides upstream (guided_diffusion.py:125-133, losses/velocity_diffusion.py:33-61).
 * Names: pmi_split_<twin>, like the split conversions above, and not <twin>_split: tests/test_norm_resample_bounds_cpu.py requires every
 * pmi_gn* / pmi_avgpool* / pmi_upsample* prototype to be exercised by tests/test_gpu_norm_resample.py, which covers the 16-bit entry points
 * only (those keep rejecting dtype 2); the split ones are covered by tests/test_gpu_precise_backward.py.
 * pmi_split_add: (a_hi + a_lo) + (b_hi + b_lo); pmi_split_relu_bwd: out = g [y > 0] with the sign of y_hi + y_lo (F.relu's backward,
 * yfcc_2.py:17-28); out may alias an input in both.  The rest as their 16-bit twins (pmi_gn_bwd_finalize is fp32 only and shared). */
int pmi_split_add(const void* a, const void* b, void* out, int64_t rows, int C, pmi_stream_t s);
int pmi_split_relu_bwd(const void* g, const void* y, void* out, int64_t rows, int C, pmi_stream_t s);
int pmi_split_avgpool2_bwd(const void* dy, void* dx, int N, int H, int W, int C, pmi_stream_t s);
int pmi_split_upsample_bilinear2_bwd(const void* dy, void* dx, int N, int H, int W, int C, pmi_stream_t s);
int pmi_split_upsample_nearest2_bwd(const void* dy, void* dx, int N, int H, int W, int C, pmi_stream_t s);
int pmi_split_gn1_bwd(const void* x, const void* dy, const float* gamma, int gamma_ld, float gamma_add, const void* res, void* dx,
                      double* partial, int N, int64_t hw, int C, float eps, pmi_stream_t s);
int pmi_split_gn_bwd_stats(const void* x, const void* x1, int C0, const void* dy, const float* coef_a, const float* coef_b, int act, float* ws,
                           int N, int HW, int C, int nchunk, pmi_stream_t s);
int pmi_split_gn_bwd_apply(const void* x, const void* x1, int C0, const void* dy, const float* coef_a, const float* coef_b, const float* coef_p,
                           const float* coef_q, int act, const void* gadd0, const void* gadd1, void* dx0, void* dx1, int N, int HW, int C,
                           pmi_stream_t s);
int pmi_gn1_bwd_partials(int64_t hw, int C);   /* slices per sample: the caller passes partial = N * this * 4 doubles of workspace */
int pmi_gn1_bwd(const void* x, const void* dy, const float* gamma, int gamma_ld, float gamma_add, const void* res, void* dx,
                double* partial, int N, int64_t hw, int C, float eps, int dtype, pmi_stream_t s);

/* ---- CLIP guidance path (forward + input-gradient) ---------------------------------------
 * ViT arithmetic: open-clip-torch 2.0.2 visual tower == OpenAI-CLIP VisionTransformer, in-tree copy
 * ruclip/model.py:11-131; wrapper models/open_clip.py:109-123; loss losses/clip/clip.py:89-99.
 * The linear layers (and their dX = dY * W input gradients) run on pmi_igemm; these are the
 * memory-bound pieces between them.                                                           */
/* LayerNorm (ruclip/model.py:11-17): fp32 rows -> 16-bit and/or fp32; mean_rstd = [mean[M] | rstd[M]] saved for bwd */
int pmi_layernorm_fwd(const float* x, int ld_x, const float* gamma, const float* beta, void* y16, float* y32, float* mean_rstd,
                      int M, int D, float eps, int dtype, pmi_stream_t s);
/* input gradient; dy row r (stride dy_ld) belongs to row r*row_stride of x/gres/outputs; out = dx + gres */
int pmi_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean_rstd, const float* gres,
                      float* g32, void* g16, int M, int D, int dy_ld, int row_stride, int dtype, pmi_stream_t s);
/* LayerNorm fused with the split-K reduction of the GEMM in front of it: the caller runs pmi_igemm with splitk > 1 and reserved3 = 1 (the
 * slabs ws[splitk][M][D] are left unreduced) and passes them here.  forward: x = sum_s ws[s] + bias + residual -> x_out (fp32) and
 * LayerNorm(x) as 16-bit operand (+ mean_rstd[2][M]); backward: dy = sum_s ws[s], then as pmi_layernorm_bwd.  D % 256 == 0, D <= 2048. */
int pmi_layernorm_fwd_slabs(const float* ws, int nslab, int64_t slab_stride, const float* bias, const float* residual, float* x_out,
                            const float* gamma, const float* beta, void* y16, float* mean_rstd, int M, int D, float eps, int dtype, pmi_stream_t s);
int pmi_layernorm_bwd_slabs(const float* ws, int nslab, int64_t slab_stride, const float* x, const float* gamma, const float* mean_rstd,
                            const float* gres, float* g32, void* g16, int M, int D, int dtype, pmi_stream_t s);
/* softmax over the first T columns of fp32 scores * scale -> 16-bit probabilities (zero padded to ld_out) */
int pmi_softmax_fwd(const float* S, void* P, int rows, int T, int ld_in, int ld_out, float scale, int dtype, pmi_stream_t s);
/* CLIP text tower (open_clip text transformer reached through models/open_clip.py:99-107; transformers CLIPTextModel through
 * models/stable_diffusion/stable_diffusion.py:295-323): causal variant of pmi_softmax_fwd -- rows = batch*heads*T, query row r
 * sees keys 0..(r mod T) -- plus x[n][t][:] = tok[ids[n][t]][:] + pos[t][:] (pos may be NULL) and a row gather (the EOT token's row). */
int pmi_softmax_causal_fwd(const float* S, void* P, int rows, int T, int ld_in, int ld_out, float scale, int dtype, pmi_stream_t s);
int pmi_embed_tokens(const int64_t* ids, const float* tok, const float* pos, float* x, int N, int T, int D, int vocab, pmi_stream_t s);
int pmi_gather_rows(const float* src, const int64_t* idx, float* dst, int R, int D, int ld, int64_t src_rows, pmi_stream_t s);
int pmi_softmax_bwd(const float* dP, const void* P, void* dS, int rows, int T, int ld_dp, int ld_p, float scale, int dtype, pmi_stream_t s);
/* in[b][R][Cc] (row stride ld_in, batch offset (b/batch_inner)*sI_o + (b%batch_inner)*sI_i) -> out[b][Cc][Rp], Rp = R rounded up to 8 */
int pmi_transpose_16(const void* in, void* out, int R, int Cc, int ld_in, int64_t sI_o, int64_t sI_i, int batch_inner, int batch, pmi_stream_t s);
int pmi_act_bwd(const void* dh, const void* hpre, void* out, int64_t n, int act, int dtype, pmi_stream_t s); /* out = dh * act'(hpre) */
/* transforms/resize/resize_right.py:34-189 as a banded operator along the middle axis of [outer][in_sz][inner]:
 * out[o][j][i] = sum_t w[j][t] * in[o][idx[j][t]][i] (idx < 0 skipped).  The adjoint (image gradient) is the same call
 * with the transposed band.  r0/r1 reserved (0). */
int pmi_resize_apply(const float* in, float* out, const int* idx, const float* w, int outer, int in_sz, int inner, int out_sz,
                     int taps, int r0, int r1, pmi_stream_t s);
/* Normalize (models/open_clip.py:78-81) + patch conv as im2col (ruclip/model.py:84-90,105): col[N*g*g][Kp] 16-bit */
int pmi_patchify(const float* img, const float* mean, const float* stdv, void* col, int N, int R, int P, int Kp, int r0, int dtype, pmi_stream_t s);
int pmi_unpatchify(const float* dcol, const float* stdv, float* dimg, int N, int R, int P, int Kp, float mul, pmi_stream_t s);
int pmi_act_fwd(const void* in, void* out, int64_t n, int act, int dtype, pmi_stream_t s);   /* QuickGELU / GELU (ruclip/model.py:20-23) */
int pmi_l2norm_rows(const float* x, float* y, int M, int D, float scale, pmi_stream_t s);    /* scale * F.normalize(x): models/open_clip.py:120-121, cc12m_1.py:294 */
int pmi_vit_assemble(const float* emb, const float* cls, const float* pos, float* x, int N, int T, int D, int r0, pmi_stream_t s);
/* GLIDE CLIP image stem (perceptor/models/glide_clip/encoders.py), one launch per direction, fp32 on the vector ALU (glide.hip).
 * fwd: a = (255 img - mean_c) / std_c; x0[n][1+p] = w a_p + pos[1+p], x0[n][0] = w_t[clamp(ts[n], 0, n_timestep-1)] + pos[0];
 *      x = LayerNorm(x0) * gamma + beta; mean_rstd[2][N*T] as pmi_layernorm_bwd reads it.  w is [W][3 P P], k = c P^2 + py P + px.
 * bwd: dimg = mul * 255 / std_c * sum_j w[j][k] * LN'(g)[j] over the patch rows (token 0's row is dropped); every pixel is stored once.
 * P must be 4, W a multiple of 64 up to 2048, R a multiple of P; anything else returns PMI_ERR_ARG before a launch. */
int pmi_glide_embed_fwd(const float* img, const float* mean, const float* stdv, const float* w, const int64_t* ts, const float* w_t,
                        const float* pos, const float* gamma, const float* beta, float* x0, float* x, float* mean_rstd,
                        int N, int R, int P, int W, int n_timestep, float eps, pmi_stream_t s);
int pmi_glide_embed_bwd(const float* g, const float* x0, const float* gamma, const float* mean_rstd, const float* w, const float* stdv,
                        float* dimg, int N, int R, int P, int W, float mul, pmi_stream_t s);
/* losses/clip/clip.py:89-99 (+ F.normalize of models/open_clip.py:120-121): loss = mult * sum_{n,k} w_k 2 asin(|e_n-t_k|/2)^2 / (n_total*K);
 * demb = gscale * dloss/demb (emb un-normalised).  n_total = global batch (>= N) so a sharded batch keeps the global mean. */
int pmi_spherical_loss(const float* emb, const float* tgt, const float* wts, float* loss, float* demb, int N, int K, int D,
                       int n_total, float mult, float gscale, pmi_stream_t s);

/* ---- CLIP ModifiedResNet image tower (open_clip / OpenAI-CLIP RN50 .. RN50x64; csrc/resnet.hip) ------------------------------------------
 * The reference runs open_clip's model.encode_image + autograd (models/open_clip.py:109-123, RN towers of models/open_clip.py:24-44 and
 * models/clip.py:6-27).  Convolutions (BatchNorm folded into weight + bias), their input gradients, pools and ReLU masks are pmi_igemm /
 * pmi_avgpool2(_bwd) / pmi_act_fwd / pmi_act_bwd; these replace the rest, 16-bit dtype 0 / 1:
 * Normalize(mean, std) of the resized NCHW fp32 image (models/open_clip.py:78-81) -> the stem convolution's input [N][H][W][8] (channels 3..7 zero);
 * the adjoint: dimg[n][c][y][x] = mul * dx[n][y][x][c] / std[c], dx fp32 with channel pitch ldc */
int pmi_rn_stage_input(const float* img, const float* mean, const float* stdv, void* out, int N, int H, int W, int dtype, pmi_stream_t s);
int pmi_rn_stage_input_bwd(const float* dx, int ldc, const float* stdv, float* dimg, int N, int H, int W, float mul, pmi_stream_t s);
/* AttentionPool2d's tokens (flatten + torch.cat([mean, x]) + positional_embedding): x [N][HW][C] -> tok [N*(HW+1)][C], the mean in fp32;
 * the adjoint dx[n][p] = dtok[n][1+p] + (dtok[n][0] + dq0[n]) / HW (dq0 [N][C] fp32: the query path's gradient of row 0, or NULL) */
int pmi_rn_tokens(const void* x, const float* pos, void* tok, int N, int HW, int C, int dtype, pmi_stream_t s);
int pmi_rn_tokens_bwd(const void* dtok, const float* dq0, void* dx, int N, int HW, int C, int dtype, pmi_stream_t s);
/* AttentionPool2d's F.multi_head_attention_forward with the mean token as the only query, head dim 64, T <= 1024 keys:
 * q [N][C], kv [N*T][2C] (K | V, projections applied) -> o [N][C], P [N*heads][T] fp32 softmax(scale q.k) (kept for the backward);
 * backward: dO [N][C] -> dq [N][C] (before the scale is applied to q), dkv [N*T][2C] (dK | dV), one workgroup per (image, head) */
int pmi_rn_attn_fwd(const void* q, const void* kv, void* o, float* P, int N, int T, int C, int heads, float scale, int dtype, pmi_stream_t s);
int pmi_rn_attn_bwd(const void* q, const void* kv, const float* P, const void* dout, void* dq, void* dkv, int N, int T, int C, int heads,
                    float scale, int dtype, pmi_stream_t s);

/* ---- guidance losses beside the spherical CLIP loss (csrc/losses.hip), fp32, each with its gradient; no atomics: every scalar is a
 * two-stage sum in a fixed order through the caller's `partial` workspace, so results are bit-identical from run to run.
 * pmi_head_loss: a linear probe on the tower's un-normalised embedding emb [N][D], W [K][D], b [K] (K <= 16, D <= 4096); with
 *   e = emb / max(|emb|, 1e-12), l = W e + b, p = softmax(l):
 *   mode 0 (K = 1; losses/simulacra_aesthetic.py:36-41 over models/simulacra_aesthetic/simulacra_aesthetic.py:58-60, whose second
 *     F.normalize is the identity): r = W (sqrt(D) e) + b, loss = mult * sum_n (r_n - target)^2 / n_total;
 *   mode 1 "logit" (losses/aesthetic_visual_assessment.py:41-42): loss = -0.01 mult sum_n l[n][target - 1] / n_total;
 *   mode 2 "expected" (:43-47): loss = 0.01 mult sum_n sum_k (p[n][k] (k + 1) - target)^2 / (n_total K) -- each of the K products is
 *     squared on its own, as the reference does; they are NOT summed into an expectation first;
 *   mode 3 "probability" (:48-49): loss = -mult sum_n p[n][target - 1] / n_total (modes 1 and 3: target an integer in 1 .. K).
 *   out [N][K] = r (mode 0) or l; demb [N][D] = gscale * dloss/demb; n_total = global batch (>= N) as in pmi_spherical_loss;
 *   partial = N floats.
 * pmi_smoothness (losses/smoothness.py:5-10), x [N][C][H][W]: loss = sum (x[h+1] - x[h])^2 / (n_total C (H-1) W) +
 *   sum (x[w+1] - x[w])^2 / (n_total C H (W-1)), grad = gscale * dloss/dx written in one pass; H < 2 or W < 2 is an argument error (the
 *   reference yields NaN); partial = 2048 floats.
 * pmi_sqdiff_loss (the tail of losses/resize.py:14-18): loss = sum (a - b)^2 / n_total_count, g = dloss/da = 2 (a - b) / n_total_count
 *   (dloss/db = -g); n_total_count >= count is the global element count of a sharded batch; partial = 1024 floats. */
int pmi_head_loss(const float* emb, const float* W, const float* b, float* loss, float* demb, float* out, float* partial, int N, int K,
                  int D, int mode, float target, int n_total, float mult, float gscale, pmi_stream_t s);
int pmi_smoothness(const float* x, float* loss, float* grad, float* partial, int N, int C, int H, int W, int n_total, float gscale,
                   pmi_stream_t s);
int pmi_sqdiff_loss(const float* a, const float* b, float* loss, float* g, float* partial, int64_t count, int64_t n_total_count,
                    pmi_stream_t s);

/* ---- VGG-19 feature tower and the style-transfer loss (csrc/vgg.hip; perceptor/losses/style_transfer.py), 16-bit NHWC, dtype 0 / 1,
 * fp32 accumulation, no atomics (results are bit-identical from run to run).  Convolutions + bias + ReLU and their input gradients
 * are pmi_igemm, the ReLU masks pmi_act_bwd.
 * pmi_maxpool2: nn.MaxPool2d(2, 2), x [N][H][W][C] -> y [N][H/2][W/2][C]; H, W even, C % 8 == 0.
 * pmi_maxpool2_bwd: dx = route(dy) * (x > 0): each window's dy goes to its FIRST maximum in the order (0,0), (0,1), (1,0), (1,1)
 *   (PyTorch's rule), recomputed from x (no index tensor); x is a post-ReLU activation, whose mask is applied in the same pass.
 * pmi_gram: G[(n,c)][(m,d)] = scale * sum_p f[n][p][c] f[m][p][d], fp32 [N C][N C], exactly symmetric; C % 16 == 0, N C <= 8192, any
 *   HW >= 1; ws = pmi_gram_workspace(N, HW, C) floats (split-K slabs, added in slab order).
 * pmi_style_level: loss2[0] = mean |fa - fb| over N HW C values, loss2[1] = mean |Ga - Gb| over (N C)^2, S [N C][N C] 16-bit =
 *   sign(Ga - Gb) in {-1, 0, +1}; partial = 2048 floats.
 * pmi_gram_bwd: dF[n][p][c] = (fa > 0) * ( gscale * ( c_feat * sign(fa - fb)[n][p][c] + c_gram * sum_{m,d} (S + S^T)[(n,c)][(m,d)]
 *   fa[m][p][d] ) + g_in[n][p][c] ), g_in nullable (the gradient arriving from deeper layers, already scaled by gscale); T = workspace of
 *   (N C)^2 16-bit values that receives S + S^T. */
int pmi_maxpool2(const void* x, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_maxpool2_bwd(const void* dy, const void* x, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_gram_workspace(int N, int HW, int C);
int pmi_gram(const void* f, float* G, float* ws, int N, int HW, int C, float scale, int dtype, pmi_stream_t s);
int pmi_style_level(const void* fa, const void* fb, const float* Ga, const float* Gb, void* S, float* loss2, float* partial, int N, int HW,
                    int C, int dtype, pmi_stream_t s);
int pmi_gram_bwd(const void* fa, const void* fb, const void* S, void* T, const void* g_in, void* dF, int N, int HW, int C, float c_feat,
                 float c_gram, float gscale, int dtype, pmi_stream_t s);

/* ---- LPIPS level (csrc/lpips.hip; perceptor/losses/lpips.py -> lpips 0.1 NetLinLayer over unit-normalised features), 16-bit NHWC features
 * fa, fb [N][HW][C], dtype 0 / 1, fp32 arithmetic, no atomics (bit-identical from run to run).  C % 16 == 0, C <= 512, any HW >= 1; anything
 * else is PMI_ERR_ARG without a launch.  eps = 1e-10.
 * pmi_lpips_level: na = |fa|, nb = |fb| per pixel, s[n][p] = sum_c w[c] (fa_c / (na + eps) - fb_c / (nb + eps))^2, all fp32 [N][HW];
 *   mean[n] = sum_p s[n][p] / HW.  w fp32 [C], NULL = all ones.  mean NULL: not computed and partial unused; else partial = 512 N floats.
 * pmi_lpips_level_bwd: r [N][HW] fp32 = dL/ds; q_c = 2 r w_c (fa_c / (na + eps) - fb_c / (nb + eps));
 *   dFa = (fa > 0) * ( gscale * ( q / (na + eps) - fa (fa . q) / (na (na + eps)^2) ) + g_in_a ), dFb the same with a and b swapped (q -> -q).
 *   g_in_a / g_in_b nullable: the gradient arriving from deeper layers, already masked and scaled by gscale.  dFa / dFb nullable (not both):
 *   one launch writes either side or both from one read of fa and fb.  At an all-zero pixel the gradient is 0 (autograd gives NaN there). */
int pmi_lpips_level(const void* fa, const void* fb, const float* w, float* s_out, float* na, float* nb, float* mean, float* partial, int N,
                    int HW, int C, int dtype, pmi_stream_t s);
int pmi_lpips_level_bwd(const void* fa, const void* fb, const float* w, const float* na, const float* nb, const float* r, const void* g_in_a,
                        const void* g_in_b, void* dFa, void* dFb, int N, int HW, int C, float gscale, int dtype, pmi_stream_t s);

/* ---- Real-ESRGAN RRDBNet dense-block convolution (csrc/rrdb.hip), 16-bit NHWC, dtype 0 / 1, fp32 accumulation, forward only.
 * pmi_rdb_conv3x3: one 3x3 / pad 1 / stride 1 convolution over the channel prefix [0, Cin) of X (pixel pitch ldx elements) into the N-channel
 *   slice D (pixel pitch ldd), with everything the networks of perceptor/models/super_resolution/custom_rrdbnet_arch.py put around it:
 *     z = conv(X)[pix][n] + bias[n];  a = z >= 0 ? z : slope z;  D[pix][n] = beta (alpha a + R1[pix][n]) + R2[pix][n]
 *   in fp32 with one rounding at the store.  It replaces ResidualDenseBlock.forward (:32-39: conv1-4 + LeakyReLU write the slices
 *   [64 + 32 (k - 1), + 32) of the dense buffer their own prefix lives in -- no torch.cat; conv5 with alpha = 0.2, R1 = x), RRDB.forward
 *   (:56-61: the last conv5 also gets beta = 0.2, R2 = the RRDB's input), and of CustomRRDBNet.forward (:105-127) conv_body + skip
 *   (R1 = feat), F.interpolate(scale_factor=2, mode="nearest") + conv_up* + LeakyReLU (up = 1: X is the half-size grid, read at
 *   (y >> 1, x >> 1); H and W even) and conv_hr + LeakyReLU.  slope = 1: no activation.  R1 / R2 NULL: absent.
 *   Cin a multiple of 32 in 32 .. 192, N 32 or 64; images, H, W >= 1 (any size: tiles are masked); pitches multiples of 8 and pointers
 *   16-byte aligned; one image of X at most 2^31 - 16 bytes.  Wp: 16-bit weights in fragment order
 *   [Cin / 32][tap = 3 ky + kx][N / 16][lane = 16 q + r][8] = W[16 nb + r][32 chunk + 8 q + j][ky][kx]; bias fp32 [N].
 *   D may be channels of the buffer X points into as long as they lie outside [0, Cin); R1 may be X.  Only D's slice is written.
 * pmi_rdb_conv3x3_eligible: host only, 1 when pmi_rdb_conv3x3 takes the shape (ldr = 0: that residual absent), else 0; pmi_rdb_conv3x3 then
 *   (and for a misaligned or NULL pointer, or a non-finite scalar) returns PMI_ERR_ARG without a launch. */
int pmi_rdb_conv3x3_eligible(int Cin, int N, int ldx, int ldd, int ldr1, int ldr2, int up, int images, int H, int W, int dtype);
int pmi_rdb_conv3x3(const void* X, int ldx, int Cin, const void* Wp, const float* bias, int N, void* D, int ldd, const void* R1, int ldr1,
                    const void* R2, int ldr2, float alpha, float beta, float slope, int up, int images, int H, int W, int dtype,
                    pmi_stream_t s);

/* ---- MonsterDiffusion: the k-diffusion UNet's FIR resamplers (fir.hip) and the EDM sampler algebra (sampling.hip) ----
 * pmi_fir_down2 / pmi_fir_up2: Downsample2d / Upsample2d with the "linear" kernel (base/layers.py:208-241) on 16-bit NHWC (f16, bf16), C a
 *   multiple of 8, pointers 16-byte aligned.  down: reflect-pad 1, depthwise 4x4 k k^T with k = [1, 3, 3, 1] / 8, stride 2, H and W even and
 *   >= 2 -> [N, H/2, W/2, C].  up: reflect-pad 1, conv_transpose2d with (2k)(2k)^T, stride 2, padding 3, H and W >= 2 -> [N, 2H, 2W, C]; per
 *   axis out[2y] = x[refl(y-1)]/4 + 3x[y]/4, out[2y+1] = 3x[y]/4 + x[refl(y+1)]/4 (refl: x[-1] = x[1], x[H] = x[H-2]).  fp32 sums, one
 *   rounding at the store.  Any other shape or dtype: PMI_ERR_ARG, nothing written.
 * pmi_fir_down2_bwd / pmi_fir_up2_bwd: their exact transposes, reflection included (the input gradient).  H, W are the FORWARD input's size:
 *   both write dx [N, H, W, C]; dy is [N, H/2, W/2, C] (down_bwd, H and W even) resp. [N, 2H, 2W, C] (up_bwd).  Gather form, no atomics: per
 *   axis at most 3 resp. 6 terms (the folds of the padded samples land on rows 1 and H-2), fp32 sums of exact products, one rounding at the
 *   store, two runs bit-equal.  Same contract as the forward pair.
 * pmi_edm_*: fp32 NCHW images in [0, 1] (x = 2 img - 1), sigma one value per sample (count N) or one for the batch (count 1); D = sigma_data.
 *   stage_in:  x16 [N, H, W, Cpad] = c_in(sigma) x (channels 3.. zero), c_in = 1 / sqrt(D^2 + sigma^2); c_noise [sigma_n] = ln(sigma) / 4.
 *   stage_out: denoised_xs = c_skip x + c_out F, c_skip = D^2 / (D^2 + sigma^2), c_out = sigma D / sqrt(D^2 + sigma^2); F = net_out fp32 NHWC,
 *              ld values per pixel.
 *   stage_out_bwd: g16 [N, H, W, Cpad] = (scale c_out) d_denoised (channels 3.. zero) from d_denoised fp32 NCHW [N, 3, H, W]; scale > 0 is the
 *              caller's power of two that keeps an f16 gradient in range (1 for bf16).
 *   stage_in_bwd: d_images = 2 (c_skip d_denoised + (c_in inv_scale) gx) fp32 NCHW; gx = the fp32 NHWC gradient wrt the network input, ld
 *              values per pixel, still scaled; the 2 is x = 2 img - 1.  The gradient wrt sigma is not computed.
 *   predict:  eps = (x - denoised_xs) / sigma; step = decode(denoised_xs + eps sigma_to); corr = decode(x_prev + (sigma - sigma_prev)
 *              (eps + eps_prev) / 2); decode(x) = (x + 1) / 2.  Each output may be NULL (at least one is not); an output's inputs must be given.
 *   inject_noise: decode(x + sqrt(sigma_rev^2 - sigma^2) noise s_noise).
 *   lms:       decode(x + sum_{k < order} coeff_k eps_k), order 1..4, over `total` elements. */
int pmi_fir_down2(const void* x, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_fir_up2(const void* x, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_fir_down2_bwd(const void* dy, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_fir_up2_bwd(const void* dy, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_edm_stage_out_bwd(const float* d_denoised, const float* sigma, int sigma_n, float sigma_data, float scale, void* g, int N, int H,
                          int W, int Cpad, int dtype, pmi_stream_t s);
int pmi_edm_stage_in_bwd(const float* d_denoised, const float* gx, int ld, const float* sigma, int sigma_n, float sigma_data,
                         float inv_scale, float* d_images, int N, int H, int W, pmi_stream_t s);
int pmi_edm_stage_in(const float* img, const float* sigma, int sigma_n, float sigma_data, void* x, float* c_noise, int N, int H, int W,
                     int Cpad, int dtype, pmi_stream_t s);
int pmi_edm_stage_out(const float* img, const float* net_out, int ld, const float* sigma, int sigma_n, float sigma_data, float* denoised_xs,
                      int N, int H, int W, pmi_stream_t s);
int pmi_edm_predict(const float* img, const float* denoised_xs, const float* sigma, int sigma_n, const float* sigma_to, int sigma_to_n,
                    const float* prev_img, const float* prev_sigma, int prev_sigma_n, const float* prev_eps, float* eps_out,
                    float* step_out, float* corr_out, int N, int64_t chw, pmi_stream_t s);
int pmi_edm_inject_noise(const float* img, const float* sigma, int sigma_n, const float* sigma_rev, int sigma_rev_n, const float* noise,
                         float s_noise, float* out, int N, int64_t chw, pmi_stream_t s);
int pmi_edm_lms(const float* img, const float* eps0, const float* eps1, const float* eps2, const float* eps3, float coeff0, float coeff1,
                float coeff2, float coeff3, int order, float* out, int64_t total, pmi_stream_t s);

/* ---- Real-ESRGAN U-Net discriminator: the image gradient's own kernels (disc.hip) ----
 * Replaces: the autograd backward of Conv2d(Cin, Cout, 4, 2, 1, bias=False) -- torch.nn.grad.conv2d_input / F.conv_transpose2d(g, W,
 *   stride=2, padding=1) -- fused with the skip-gradient addition and the LeakyReLU mask of the layer before it, and F.leaky_relu /
 *   its backward and Tensor.mean of unet_discriminator_sn.py:34-63 and discriminator.py:28-29.
 * pmi_convt4x4s2: G [images, h, w, ldg] 16-bit NHWC gradient (Cout channels used) -> D [images, 2h, 2w, ldd] (Cin channels written):
 *   acc[2p+a, 2q+b, ci] = sum_{u,v in {0,1}} sum_co W[co, ci, ky(a,u), kx(b,v)] G[p+a-1+u, q+b-1+v, co], ky(0,u) = 3 - 2u, ky(1,u) = 2 - 2u
 *   (kx alike), G zero outside the image; D = (acc + R) * (Y >= 0 ? 1 : slope) with R, Y optional 16-bit NHWC on D's grid with their own
 *   pitches.  fp32 accumulation, one rounding at the store; out_f32 = 1: D is fp32 (ldd counts floats).  Wp: the weights packed per phase
 *   in fragment order [Cin / 16][phase = 2a + b][Cout / 32][2u + v][q = 4][r = 16][j = 8] = W[32 chunk + 8 q + j][16 block + r][ky][kx]
 *   (engine/disc.py: pack_convt_weights).  Cout % 32 == 0, 32 .. 512; Cin % 32 == 0; pitches % 8 == 0 and >= their channel count; every
 *   pointer 16-byte aligned; any h, w >= 1.  Only the Cin channels of D's pixels are written.
 * pmi_convt4x4s2_eligible: host only, 1 when pmi_convt4x4s2 takes the shape (ldr / ldy = 0: that operand absent), else 0; pmi_convt4x4s2
 *   then (and for a misaligned or NULL pointer, out_f32 outside {0, 1} or a non-finite slope) returns PMI_ERR_ARG without a launch.
 * pmi_lrelu_bwd: dz = (g + g2) * (y >= 0 ? 1 : slope) over n 16-bit values, g2 optional; pmi_lrelu_add: y = lrelu_slope(z) + r, r optional.
 *   fp32 arithmetic, one rounding at the store; any n >= 1, pointers 16-byte aligned.
 * pmi_mean_f32: out[0] = scale * sum_{i < n} x[i] in a fixed order (256 contiguous ranges summed by one workgroup each into partial[256],
 *   then one tree over the partials): two runs are bit-equal. */
int pmi_convt4x4s2_eligible(int Cout, int Cin, int ldg, int ldd, int ldr, int ldy, int images, int h, int w, int dtype);
int pmi_convt4x4s2(const void* G, int ldg, int Cout, const void* Wp, int Cin, void* D, int ldd, const void* R, int ldr, const void* Y, int ldy,
                   float slope, int out_f32, int images, int h, int w, int dtype, pmi_stream_t s);
int pmi_lrelu_bwd(const void* g, const void* g2, const void* y, void* dz, int64_t n, float slope, int dtype, pmi_stream_t s);
int pmi_lrelu_add(const void* z, const void* r, void* y, int64_t n, float slope, int dtype, pmi_stream_t s);
int pmi_mean_f32(const float* x, float* partial, float* out, int64_t n, float scale, pmi_stream_t s);

/* ---- drawers.JPEG: the differentiable JPEG codec (jpeg.hip), fp32, one launch per call ----
 * Coefficients are the reference's own layout (the drawer's state_dict): y [N][(H/8)(W/8)][8][8], cb and cr [N][(H/16)(W/16)][8][8] (4:2:0),
 *   blocks row-major over the block grid, the first index inside a block is the row (vertical frequency).  images / out / d_out are NCHW
 *   [N][3][H][W].  H and W multiples of 16, factor finite and > 0, pointers 16-byte aligned; anything else: PMI_ERR_ARG, nothing written.
 *   Quantisation tables: Annex K luma TRANSPOSED and chroma with its 4 x 4 corner transposed, as jpeg/utils.py:7-31 builds them.
 * pmi_jpeg_decode: decompress_jpeg.forward (jpeg/decompression.py:171-189): c * (table * factor) * alpha(u) alpha(v), separable 8 x 8 inverse
 *   DCT (0.25 sum + 128), block merge, chroma replicated 2 x 2, YCbCr -> RGB with the -128 chroma shift (cancelled against the +128
 *   algebraically), clamp to [0, 255], / 255.
 * pmi_jpeg_decode_bwd: its exact adjoint: d_y, d_cb, d_cr (each may be NULL: not computed; all NULL: no launch) from d_out.  The pre-clamp
 *   value is recomputed with the forward's arithmetic; the gradient passes where 0 < v < 255 and is zero elsewhere (a value exactly at 0 or
 *   255 passes nothing; torch splits such ties).  2 x 2 sums of the chroma pixel gradient, forward DCT basis, alpha, 0.25, table * factor.
 *   Gather form, no atomics: a macroblock's six blocks depend on its own 16 x 16 pixels only; two runs are bit-equal, and a sample's result
 *   does not depend on the batch it is in.
 * pmi_jpeg_encode: compress_jpeg.forward (jpeg/compression.py:176-188): x 255, RGB -> YCbCr, 2 x 2 mean of the chroma, block split, forward
 *   DCT with 0.25 alpha(u) alpha(v), / (table * factor), then round_mode 1: diff_round(x) = round(x) + (x - round(x))^3 with round half to
 *   even (utils.py:34-41), 0: no rounding (the reference's rounding= argument given the identity).  Forward only. */
int pmi_jpeg_decode(const float* y, const float* cb, const float* cr, float factor, float* out, int N, int H, int W, pmi_stream_t s);
int pmi_jpeg_decode_bwd(const float* y, const float* cb, const float* cr, float factor, const float* d_out, float* d_y, float* d_cb,
                        float* d_cr, int N, int H, int W, pmi_stream_t s);
int pmi_jpeg_encode(const float* images, float factor, int round_mode, float* y, float* cb, float* cr, int N, int H, int W, pmi_stream_t s);

/* ---- OWL-ViT detection heads on the ViT tower's last hidden state (owlvit.hip); fp32 unless stated, no float atomics: two runs are bit-equal ----
 * pmi_owl_merge_ln_fwd: x [N][T][W] (the last hidden state).  y = LayerNorm(x; g1, b1) on all T rows (post_layernorm), m[p] = y[p + 1] * y[0]
 *   (the class-token merge), feats = LayerNorm(m; g2, b2) for the P = T - 1 patch rows, written as fp32 feats32 [N P][W] and as the 16-bit
 *   GEMM operand feats16 (dtype f16 / bf16).  mean_rstd1 [2][N T] and mean_rstd2 [2][N P] receive (mean | rstd) of the two norms.  One launch.
 *   W % 4 == 0, W <= 2048, T >= 2, pointers 16-byte aligned.
 * pmi_owl_merge_ln_bwd: the exact adjoint: dfeats [N P][W] -> dx [N][T][W], every row written.  The class row's gradient is the sum over an
 *   image's patch rows: pmi_owl_merge_bwd_blocks(T) partial rows per image (partials: [N][blocks][W] floats of workspace) summed in a fixed
 *   order by a second launch.  Two launches.
 * pmi_owl_class_logits_fwd: g [M][ldg] = the packed class-head GEMM's fp32 output (columns 0..D-1 dense0, D logit_shift, D + 1 logit_scale, bias
 *   included; the rest padding), q [Q][D] the prepared queries.  class_embeds [M][D] = e / (|e| + 1e-6); logits [M][Q] =
 *   (class_embeds . q + shift) * (elu(scale) + 1).  D <= 1024, Q D <= 12288 (the query block is staged in LDS once per workgroup).
 * pmi_owl_class_logits_bwd: dlogits [M][Q] -> dg [M][ldg] 16-bit (dtype), the gradient at g and the operand of the transposed-weight GEMM:
 *   D columns through the normalisation, the shift column, the scale column through ELU', zeros in the padding.
 * pmi_owl_topk_loss: logits [N][P][Q], weights [Q].  Per (n, q): log-softmax over the P tokens, S = the k_eff = min(k, P) largest (ties: the
 *   lower index); partials [N Q] receives -0.01 w_q / (N k_eff) sum_{p in S} logsoftmax_p (the loss is their sum) and
 *   dlogits[n][p][q] = mul * -0.01 w_q / (N k_eff) ([p in S] - k_eff softmax_p).  One workgroup per (n, q); P <= 16256 (64 KB of LDS), k <= 64.
 * pmi_owl_box_out: h [M][ldh] 16-bit (the box head after dense1 + GELU), w2 [4][W], b2 [4], box_bias [P][4] ->
 *   boxes [M][4] = sigmoid(h w2^T + b2 + box_bias[row % P]).  W % 8 == 0. */
int pmi_owl_merge_ln_fwd(const float* x, const float* g1, const float* b1, const float* g2, const float* b2, float* feats32, void* feats16,
                         float* mean_rstd1, float* mean_rstd2, int N, int T, int W, float eps, int dtype, pmi_stream_t s);
int pmi_owl_merge_bwd_blocks(int T);
int pmi_owl_merge_ln_bwd(const float* dfeats, const float* x, const float* g1, const float* b1, const float* g2, const float* mean_rstd1,
                         const float* mean_rstd2, float* dx, float* partials, int N, int T, int W, pmi_stream_t s);
int pmi_owl_class_logits_fwd(const float* g, int ldg, const float* q, float* logits, float* class_embeds, int64_t M, int D, int Q, pmi_stream_t s);
int pmi_owl_class_logits_bwd(const float* dlogits, const float* g, int ldg, const float* q, void* dg, int64_t M, int D, int Q, int dtype,
                             pmi_stream_t s);
int pmi_owl_topk_loss(const float* logits, const float* weights, float* dlogits, float* partials, int N, int P, int Q, int k, float mul,
                      pmi_stream_t s);
int pmi_owl_box_out(const void* h, int ldh, const float* w2, const float* b2, const float* box_bias, float* boxes, int64_t M, int P, int W,
                    int dtype, pmi_stream_t s);

/* ---- DeepImagePrior: a skip network trained through its WEIGHTS (dip.hip, the 8-tap resamplers in fir.hip) ----
 * Tensors are NHWC 16-bit (dtype = f16 / bf16), C a multiple of 4, pointers 8-byte aligned.  "ring r" (0 or 1): the tensor is
 * [N, H + 2r, W + 2r, ld] and its interior is the H x W map.  Parameters, statistics and parameter gradients are fp32.  No float atomics.
 * pmi_dip_pack_w: w [Cout][Cin][taps] fp32 -> fwd [n_p][taps][cin_p] (pmi_igemm's B, zero padded) and, unless NULL, dxp [rows_p][taps][cout_p] =
 *   w transposed with the taps reversed (the input-gradient convolution's B).  Runs every forward: no packing outlives a weight update.
 * pmi_dip_wgrad: dW [Cout][Cin][taps] (PyTorch's layout) = alpha sum_{n,y,x} dY[n,y,x,co] X[n,y+ky,x+kx,ci], db [Cout] = alpha sum dY (NULL: skipped).
 *   taps 9: X has ring 1 (the padded input the forward convolved); taps 1: X's interior pixel.  Cout > 4: MFMA 32x32x16 on pixel-major LDS tiles
 *   read with ds_read_b64_tr_b16 (rows 16-byte aligned, ld % 8 == 0, ld >= the channel count rounded up to 8); Cout <= 4: a plain reduction.
 *   slabs: splits * (Cout Cin taps + Cout) floats, splits = pmi_dip_wgrad_splits(N H W, Cout, Cin, taps); a fixed-order reduce sums them.
 * pmi_dip_bn_stats: mean [C], rstd [C] = 1 / sqrt(biased var + eps) over N H W (partial sums, then a centred second pass); running_mean /
 *   running_var (NULL: untouched) move by `momentum` toward the mean and the UNBIASED variance.  part: pmi_dip_bn_blocks(N H W) * C floats.
 * pmi_dip_bn_apply: y = act(a x + b), a = gamma rstd, b = beta - mean a; act 0 none, 1 LeakyReLU(0.2).  y has pitch ldy (a channel slice of a wider
 *   tensor through the pointer) and ring y_ring, which is filled by reflection.
 * pmi_dip_bn_bwd: sums [2][C] = (sum dy', sum dy' xhat), dy' = dy act'(a x + b); dbeta = alpha sums[0], dgamma = alpha sums[1] (NULL: skipped);
 *   dx = a (dy' - sums[0] / P - xhat sums[1] / P) into the interior of a tensor with ring dx_ring (the ring is the caller's).  dy has no ring.
 *   part: 2 * pmi_dip_bn_blocks(N H W) * C floats.
 * pmi_dip_reflect_pad: [N, H, W, C] -> [N, H + 2, W + 2, C];  pmi_dip_pad_fold: its adjoint (+ add, NULL or [N, H, W, C]).
 * pmi_dip_head_fwd: out NCHW fp32 = sigmoid?(cm^T (w x + b)): w [Cout][Cin], Cout <= 4, Cin % 8 == 0 and <= 512; cm: NULL or the row-major 3 x 3
 *   matrix of einsum("nchw,cd->ndhw").  pmi_dip_head_bwd: dz [N HW][8] 16-bit = scale cm (dout sigmoid'(out)), channels Cout .. 7 zero.
 * pmi_fir8_*: the 8-tap cubic resamplers (reflect pad 3 resp. 2) and their exact adjoints in gather form; H, W are the FORWARD input's size.
 *   down2: x ring x_ring -> [N, H/2, W/2, C], H, W even and >= 4; up2: -> [N, 2H, 2W, C], H, W >= 3; down2_bwd writes a ring-dx_ring tensor. */
int pmi_dip_pack_w(const float* w, void* fwd, void* dxp, int Cout, int Cin, int taps, int n_p, int cin_p, int rows_p, int cout_p, int dtype,
                   pmi_stream_t s);
int pmi_dip_wgrad_splits(int64_t P, int Cout, int Cin, int taps);
int pmi_dip_wgrad(const void* dy, int ldy, int dy_ring, const void* x, int ldx, int x_ring, float* slabs, float* dW, float* db, int N, int H,
                  int W, int Cout, int Cin, int taps, int splits, float alpha, int dtype, pmi_stream_t s);
int pmi_dip_bn_blocks(int64_t P);
int pmi_dip_bn_stats(const void* x, int ldx, int x_ring, float* part, float* mean, float* rstd, float* running_mean, float* running_var, int N,
                     int H, int W, int C, float momentum, float eps, int dtype, pmi_stream_t s);
int pmi_dip_bn_apply(const void* x, int ldx, int x_ring, const float* mean, const float* rstd, const float* gamma, const float* beta, void* y,
                     int ldy, int y_ring, int N, int H, int W, int C, int act, int dtype, pmi_stream_t s);
int pmi_dip_bn_bwd(const void* x, int ldx, int x_ring, const void* dy, int lddy, const float* mean, const float* rstd, const float* gamma,
                   const float* beta, float* part, float* sums, float* dgamma, float* dbeta, void* dx, int lddx, int dx_ring, int N, int H, int W,
                   int C, int act, float alpha, int dtype, pmi_stream_t s);
int pmi_dip_reflect_pad(const void* x, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_dip_pad_fold(const void* gp, const void* add, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_dip_head_fwd(const void* x, const float* w, const float* bias, const float* cm, float* out, int N, int HW, int Cin, int Cout, int sigmoid,
                     int dtype, pmi_stream_t s);
int pmi_dip_head_bwd(const float* dout, const float* out, const float* cm, void* dz, int N, int HW, int Cout, int sigmoid, float scale, int dtype,
                     pmi_stream_t s);
int pmi_fir8_down2(const void* x, int x_ring, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_fir8_up2(const void* x, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_fir8_down2_bwd(const void* dy, void* dx, int dx_ring, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_fir8_up2_bwd(const void* dy, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s);

/* ---- DPT depth decoder (dpt.hip): the memory-bound steps between the convolutions of models.MidasDepth ----
 * Tensors are NHWC 16-bit (dtype = f16 / bf16) unless stated, C a multiple of 8, pointers 16-byte aligned; fp32 arithmetic, one rounding at
 * the store.  No atomics: two runs are bit-equal.  Bad arguments return PMI_ERR_ARG without a launch.
 * pmi_bilinear2_ac_fwd: y [N, 2H, 2W, C] = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=True) (+ r, NULL or a tensor on the
 *   OUTPUT grid: the other summand of the next fusion block).  Output index o reads source o (L - 1) / (2L - 1); L = 1 copies.  H, W <= 16384.
 *   (pmi_upsample_bilinear2 is align_corners=False: another operator.)
 * pmi_bilinear2_ac_bwd: the exact adjoint in gather form, g [N, 2H, 2W, C] -> dx [N, H, W, C]; H, W are the FORWARD input's size.
 * pmi_depth_to_space: x [N, H, W, k k C] with columns ordered (ky, kx, c) -> y [N, kH, kW, C], y[n, k y + ky, k x + kx, c] = x[n, y, x, (ky, kx, c)]
 *   + bias[c] (fp32, NULL: none); k in {2, 4}.  With the GEMM to k k C columns before it this is ConvTranspose2d(C', C, k, stride=k).
 * pmi_space_to_depth: the inverse permutation (the adjoint's first step), y -> x; after pmi_depth_to_space without bias it returns x bit for bit.
 * pmi_dpt_tap_split: x fp32 [N][T][W] -> tok 16-bit [N (T - 1)][W] (rows 1 .. T - 1) and cls 16-bit [N][W] (row 0).  W % 4 == 0, T >= 2.
 * pmi_dpt_tap_join: d_tok fp32 [N (T - 1)][W], d_cls fp32 [N][W] -> out fp32 [N][T][W].
 * pmi_dpt_tap_add: out32 = a + b (fp32, n values, n % 4 == 0) and out16 = the same sum rounded once.
 * pmi_dpt_colsum: x 16-bit [N][P][W] -> out fp32 [N][W] = sum over p, rows p = j (mod 4) summed in order into s_j, then (s0 + s1) + (s2 + s3).
 *   W even, x 4-byte aligned, N <= 65535.
 * pmi_dpt_relu_bwd: dz = g (y > 0 ? 1 : 0) (+ r, NULL or like g); y is the ReLU's output OR its input (the masks agree), n % 8 == 0.
 * pmi_dpt_head_fwd: h 16-bit [P][32] (post-ReLU), w fp32 [32], b fp32 [1] -> out fp32 [P] = -relu(w . h + b) (NCHW with one channel); the fp32
 *   pointers of both head kernels 4-byte aligned.
 * pmi_dpt_head_bwd: dh 16-bit [P][32], dh[p][c] = -scale dout[p] (out[p] < 0) w[c] (h[p][c] > 0): out < 0 exactly where the pre-ReLU value was
 *   positive, and the mask of the ReLU that produced h is folded in. */
int pmi_bilinear2_ac_fwd(const void* x, const void* r, void* y, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_bilinear2_ac_bwd(const void* g, void* dx, int N, int H, int W, int C, int dtype, pmi_stream_t s);
int pmi_depth_to_space(const void* x, const float* bias, void* y, int N, int H, int W, int C, int k, int dtype, pmi_stream_t s);
int pmi_space_to_depth(const void* y, void* x, int N, int H, int W, int C, int k, int dtype, pmi_stream_t s);
int pmi_dpt_tap_split(const float* x, void* tok, void* cls, int N, int T, int W, int dtype, pmi_stream_t s);
int pmi_dpt_tap_join(const float* d_tok, const float* d_cls, float* out, int N, int T, int W, pmi_stream_t s);
int pmi_dpt_tap_add(const float* a, const float* b, float* out32, void* out16, int64_t n, int dtype, pmi_stream_t s);
int pmi_dpt_colsum(const void* x, float* out, int N, int P, int W, int dtype, pmi_stream_t s);
int pmi_dpt_relu_bwd(const void* g, const void* y, const void* r, void* dz, int64_t n, int dtype, pmi_stream_t s);
int pmi_dpt_head_fwd(const void* h, const float* w, const float* b, float* out, int64_t P, int dtype, pmi_stream_t s);
int pmi_dpt_head_bwd(const float* dout, const float* out, const void* h, const float* w, void* dh, int64_t P, float scale, int dtype,
                     pmi_stream_t s);

#ifdef __cplusplus
}
#endif
#endif
