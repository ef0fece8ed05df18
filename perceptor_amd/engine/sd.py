"""HIP execution engines for the StableDiffusion path: the latent UNet (eps-prediction with text cross-attention) and the VAE decoder.

Replaces ``diffusers.UNet2DConditionModel`` / ``AutoencoderKL.decode`` as called at
perceptor/models/stable_diffusion/stable_diffusion.py:195-198,259-271 (diffusers 0.6.0, poetry.lock:365-366), with the transformer
blocks of perceptor/models/stable_diffusion/attention.py:120-348 (SpatialTransformer, BasicTransformerBlock, CrossAttention incl. the
fused-attention call at :285, FeedForward/GEGLU) and the VAE's AttentionBlock (:23-117).  NHWC 16-bit activations through
libperceptor_hip.so:

  * ResnetBlock2D = conv -> conv with GroupNorm-apply+SiLU fused into each conv's patch staging, statistics out of the producer's
    epilogue, the additive time projection as a per-sample bias, shortcut / residual add in the second conv's epilogue; skip
    concatenations are two source pointers; nearest-x2 up-sampling is fused into the following conv's gather;
  * all ``time_emb_proj`` linears run as ONE GEMM per step;
  * transformer blocks keep an fp32 residual stream ([tokens][C]); q|k|v (self) and k|v (cross) projections are one GEMM each;
    GEGLU is one pass over the 8C-wide projection;
  * the context's k|v projections of all cross-attention layers depend only on the prompt: computed once per conditioning and cached.

State-dict keys are diffusers' (time_embedding.linear_1, down_blocks.{i}.resnets.{j}.conv1, ...attentions.{j}.transformer_blocks.0.attn2.to_k, ...),
so a real checkpoint's tensors load as they are.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import torch

from .. import _hip
from .._hip import ACT_NONE, ACT_SILU, call, ptr
from . import ops
from .ops import PackedLinear


@dataclass(frozen=True)
class SdConfig:
    in_channels: int = 4
    out_channels: int = 4
    block_out: Tuple[int, ...] = (320, 640, 1280, 1280)
    cross_attn: Tuple[bool, ...] = (True, True, True, False)      # CrossAttnDownBlock2D x3, DownBlock2D (mirrored on the way up)
    layers_per_block: int = 2
    heads: int = 8                                                  # `attention_head_dim` of the v1 configs is the head COUNT
    context_dim: int = 768
    groups: int = 32


@dataclass(frozen=True)
class VaeConfig:
    latent_channels: int = 4
    out_channels: int = 3
    block_out: Tuple[int, ...] = (128, 256, 512, 512)
    layers_per_block: int = 2
    groups: int = 32


SD_V1 = SdConfig()
SD_INPAINTING = SdConfig(in_channels=9)          # runwayml/stable-diffusion-inpainting: latents | mask | masked-image latents
VAE_V1 = VaeConfig()


class _Shapes:
    def __init__(self):
        self.S: Dict[str, Tuple[int, ...]] = {}

    def lin(self, k, o, i, bias=True):
        self.S[k + ".weight"] = (o, i)
        if bias:
            self.S[k + ".bias"] = (o,)

    def conv(self, k, o, i, ks):
        self.S[k + ".weight"] = (o, i, ks, ks); self.S[k + ".bias"] = (o,)

    def norm(self, k, c):
        self.S[k + ".weight"] = (c,); self.S[k + ".bias"] = (c,)

    def resnet(self, k, i, o, ted=None):
        self.norm(k + ".norm1", i); self.conv(k + ".conv1", o, i, 3)
        if ted:
            self.lin(k + ".time_emb_proj", o, ted)
        self.norm(k + ".norm2", o); self.conv(k + ".conv2", o, o, 3)
        if i != o:
            self.conv(k + ".conv_shortcut", o, i, 1)


def unet_plan(cfg: SdConfig):
    """Blocks in execution order: ("res", key, cin, cout, srcs) / ("attn", key, c) / ("down"|"up", key, c)."""
    bo = cfg.block_out
    down: List[list] = []
    ch = bo[0]
    skip_ch = [ch]
    for i, o in enumerate(bo):
        for j in range(cfg.layers_per_block):
            blk = [("res", f"down_blocks.{i}.resnets.{j}", ch, o, None)]
            ch = o
            if cfg.cross_attn[i]:
                blk.append(("attn", f"down_blocks.{i}.attentions.{j}", o))
            down.append(blk)
            skip_ch.append(ch)
        if i != len(bo) - 1:
            down.append([("down", f"down_blocks.{i}.downsamplers.0.conv", o)])
            skip_ch.append(ch)
    mid = [("res", "mid_block.resnets.0", ch, ch, None), ("attn", "mid_block.attentions.0", ch), ("res", "mid_block.resnets.1", ch, ch, None)]
    up: List[list] = []
    ca = list(reversed(cfg.cross_attn))
    for i, o in enumerate(reversed(bo)):
        for j in range(cfg.layers_per_block + 1):
            s = skip_ch.pop()
            blk = [("res", f"up_blocks.{i}.resnets.{j}", ch + s, o, (ch, s))]
            ch = o
            if ca[i]:
                blk.append(("attn", f"up_blocks.{i}.attentions.{j}", o))
            if j == cfg.layers_per_block and i != len(bo) - 1:
                blk.append(("up", f"up_blocks.{i}.upsamplers.0.conv", o))
            up.append(blk)
    return down, mid, up


def unet_gflop(cfg: SdConfig, h: int, w: int, tc: int = 77) -> float:
    """Algorithmic GFLOP of ONE UNet evaluation of ONE sample at h x w latents (2 per multiply-add; the prompt's k|v projections are
    per-conditioning work and not counted): convolutions, linears and the attention products."""
    fl = 0.0
    down, mid, up = unet_plan(cfg)
    hh, ww = h, w
    fl += 2.0 * hh * ww * cfg.in_channels * cfg.block_out[0] * 9 + 2.0 * hh * ww * cfg.block_out[0] * cfg.out_channels * 9
    ted = 4 * cfg.block_out[0]
    fl += 2.0 * (cfg.block_out[0] * ted + ted * ted)
    for blk in down + [mid] + up:
        for l in blk:
            if l[0] == "res":
                _, _, ci, co, _ = l
                fl += 2.0 * hh * ww * (ci * co * 9 + co * co * 9 + (ci * co if ci != co else 0)) + 2.0 * ted * co
            elif l[0] == "attn":
                c, t = l[2], hh * ww
                fl += 2.0 * t * c * c * (2 + 3 + 1 + 1 + 1 + 8 + 4) + 4.0 * t * t * c + 4.0 * t * tc * c
            elif l[0] == "down":
                hh, ww = hh // 2, ww // 2
                fl += 2.0 * hh * ww * l[2] * l[2] * 9
            else:
                hh, ww = hh * 2, ww * 2
                fl += 2.0 * hh * ww * l[2] * l[2] * 9
    return fl / 1e9


def vae_decoder_gflop(cfg: "VaeConfig", h: int, w: int, fused_up: bool = True) -> Tuple[float, float]:
    """Algorithmic GFLOP (2 per multiply-add) of ONE VAE decode of ONE sample at h x w latents: (forward, input-gradient backward).
    Forward: convolutions, linears and the mid attention's two products.  Backward: every convolution's dX (the same MFMA work as its
    forward), the attention's four products (dP, dV, dQ, dK) and both projections; the up-samplers' adjoints cost 16 taps at the low
    resolution when fused (16 / 36 of their forward) or their forward count when composed.  GroupNorm / SiLU / softmax are not counted."""
    lc, top, bo = cfg.latent_channels, cfg.block_out[-1], cfg.block_out
    hh, ww = h, w
    res = lambda hw, ci, co: 2.0 * hw * (ci * co * 9 + co * co * 9 + (ci * co if ci != co else 0))
    fwd = 2.0 * hh * ww * lc * lc + 2.0 * hh * ww * lc * top * 9
    fwd += 2 * res(hh * ww, top, top)
    t = hh * ww
    proj = 2.0 * t * top * top * 4                                     # q | k | v and proj_attn
    fwd += proj + 4.0 * t * t * top
    bwd = fwd + 4.0 * t * t * top                                      # four t x t x C products instead of two
    ch = top
    up_b = 0.0
    for i, o in enumerate(reversed(bo)):
        for _ in range(cfg.layers_per_block + 1):
            f = res(hh * ww, ch, o)
            fwd += f; bwd += f
            ch = o
        if i != len(bo) - 1:
            f = 2.0 * (4 * hh * ww) * o * o * 9
            fwd += f
            up_b += (2.0 * hh * ww * o * o * 16) if fused_up else f
            hh, ww = 2 * hh, 2 * ww
    f = 2.0 * hh * ww * ch * cfg.out_channels * 9
    fwd += f; bwd += f + up_b
    return fwd / 1e9, bwd / 1e9


def fold_upsample_weights(weight: torch.Tensor) -> torch.Tensor:
    """Weights of the one-pass adjoint of Upsample2D (nearest x2, then a 3x3 convolution with padding 1).

    With y = conv3x3(up2(x)), dx[p] gathers the rows 2p-1 .. 2p+2 of dy; the kernel rows that reach pixel p from them are
    {2}, {1, 2}, {0, 1}, {0} (the same per column).  So dx = conv2d(dy, W', stride=2, padding=1) with
    W'[ci, co, i, j] = sum over ky in S_i, kx in S_j of W[co, ci, ky, kx]: 16 taps per low-resolution pixel instead of 4 x 9.
    weight [Cout, Cin, 3, 3] -> [Cin, Cout, 4, 4] float64."""
    w = weight.detach().double()
    s = ((2,), (1, 2), (0, 1), (0,))
    rows = torch.stack([w[:, :, list(si), :].sum(2) for si in s], 2)                 # [Cout, Cin, 4, 3]
    folded = torch.stack([rows[..., list(sj)].sum(-1) for sj in s], 3)                # [Cout, Cin, 4, 4]
    return folded.permute(1, 0, 2, 3).contiguous()


# phase-major tap order of the Downsample2D adjoint: output phase (a, b) = (row, column) parity meets the kernel taps ky = a, kx = b (mod 2)
DOWN_ADJOINT_TAPS = ((0, 0), (0, 2), (2, 0), (2, 2),      # phase (0, 0): gradient pixels (p, q), (p, q-1), (p-1, q), (p-1, q-1)
                     (0, 1), (2, 1),                      # phase (0, 1): (p, q), (p-1, q)
                     (1, 0), (1, 2),                      # phase (1, 0): (p, q), (p, q-1)
                     (1, 1))                              # phase (1, 1): (p, q)


def pack_downsample_adjoint_weights(weight: torch.Tensor) -> torch.Tensor:
    """Weights of the one-pass adjoint of Downsample2D (pad right / bottom by one, then a 3x3 stride-2 convolution without padding).

    With y[oy, ox] = sum over ky, kx of W[ky, kx] x[2 oy + ky, 2 ox + kx], input pixel (2p + a, 2q + b) is read by tap (ky, kx) of output
    (p + (a - ky) / 2, q + (b - kx) / 2) only where ky = a and kx = b (mod 2):
        dx[2p + a, 2q + b] = sum over ty < 2 - a, tx < 2 - b of W[a + 2 ty, b + 2 tx]^T dy[p - ty, q - tx]
    (dy outside its grid dropped): 4, 2, 2 and 1 taps for the four phases, 9 per 2x2 block of dx instead of the 36 of a 3x3 pass over a
    zero-inserted dy.  No flip and no sum: the taps are only transposed and reordered phase-major (DOWN_ADJOINT_TAPS), which is the K
    order pmi_igemm's phased geometry reads.  weight [Cout, Cin, 3, 3] -> [Cin, Cout, 3, 3] float64 whose flattened last two axes are
    that order."""
    w = weight.detach().double()
    ky = [t[0] for t in DOWN_ADJOINT_TAPS]
    kx = [t[1] for t in DOWN_ADJOINT_TAPS]
    return w[:, :, ky, kx].permute(1, 0, 2).reshape(w.shape[1], w.shape[0], 3, 3).contiguous()


def unet_state_dict_shapes(cfg: SdConfig) -> Dict[str, Tuple[int, ...]]:
    sh, ted = _Shapes(), 4 * cfg.block_out[0]
    sh.lin("time_embedding.linear_1", ted, cfg.block_out[0]); sh.lin("time_embedding.linear_2", ted, ted)
    sh.conv("conv_in", cfg.block_out[0], cfg.in_channels, 3)
    down, mid, up = unet_plan(cfg)
    for blk in down + [mid] + up:
        for l in blk:
            if l[0] == "res":
                sh.resnet(l[1], l[2], l[3], ted)
            elif l[0] == "attn":
                k, c = l[1], l[2]
                sh.norm(k + ".norm", c); sh.conv(k + ".proj_in", c, c, 1); sh.conv(k + ".proj_out", c, c, 1)
                b = k + ".transformer_blocks.0"
                for a, ctx in ((".attn1", c), (".attn2", cfg.context_dim)):
                    sh.lin(b + a + ".to_q", c, c, False); sh.lin(b + a + ".to_k", c, ctx, False); sh.lin(b + a + ".to_v", c, ctx, False)
                    sh.lin(b + a + ".to_out.0", c, c)
                for nm in (".norm1", ".norm2", ".norm3"):
                    sh.norm(b + nm, c)
                sh.lin(b + ".ff.net.0.proj", 8 * c, c); sh.lin(b + ".ff.net.2", c, 4 * c)
            else:
                sh.conv(l[1], l[2], l[2], 3)
    sh.norm("conv_norm_out", cfg.block_out[0]); sh.conv("conv_out", cfg.out_channels, cfg.block_out[0], 3)
    return sh.S


def vae_decoder_state_dict_shapes(cfg: VaeConfig) -> Dict[str, Tuple[int, ...]]:
    sh, top = _Shapes(), cfg.block_out[-1]
    sh.conv("post_quant_conv", cfg.latent_channels, cfg.latent_channels, 1)
    sh.conv("decoder.conv_in", top, cfg.latent_channels, 3)
    sh.resnet("decoder.mid_block.resnets.0", top, top); sh.resnet("decoder.mid_block.resnets.1", top, top)
    a = "decoder.mid_block.attentions.0"
    sh.norm(a + ".group_norm", top)
    for nm in ("query", "key", "value", "proj_attn"):
        sh.lin(f"{a}.{nm}", top, top)
    ch = top
    for i, o in enumerate(reversed(cfg.block_out)):
        for j in range(cfg.layers_per_block + 1):
            sh.resnet(f"decoder.up_blocks.{i}.resnets.{j}", ch, o)
            ch = o
        if i != len(cfg.block_out) - 1:
            sh.conv(f"decoder.up_blocks.{i}.upsamplers.0.conv", o, o, 3)
    sh.norm("decoder.conv_norm_out", ch); sh.conv("decoder.conv_out", cfg.out_channels, ch, 3)
    return sh.S


def vae_encoder_state_dict_shapes(cfg: VaeConfig) -> Dict[str, Tuple[int, ...]]:
    sh = _Shapes()
    sh.conv("encoder.conv_in", cfg.block_out[0], cfg.out_channels, 3)
    ch = cfg.block_out[0]
    for i, o in enumerate(cfg.block_out):
        for j in range(cfg.layers_per_block):
            sh.resnet(f"encoder.down_blocks.{i}.resnets.{j}", ch, o)
            ch = o
        if i != len(cfg.block_out) - 1:
            sh.conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", o, o, 3)
    sh.resnet("encoder.mid_block.resnets.0", ch, ch); sh.resnet("encoder.mid_block.resnets.1", ch, ch)
    a = "encoder.mid_block.attentions.0"
    sh.norm(a + ".group_norm", ch)
    for nm in ("query", "key", "value", "proj_attn"):
        sh.lin(f"{a}.{nm}", ch, ch)
    sh.norm("encoder.conv_norm_out", ch); sh.conv("encoder.conv_out", 2 * cfg.latent_channels, ch, 3)
    sh.conv("quant_conv", 2 * cfg.latent_channels, 2 * cfg.latent_channels, 1)
    return sh.S


class _Blocks:
    """What the UNet and the VAE decoder share: packed weights by key and the ResnetBlock2D launch sequence."""

    def _init_common(self, state_dict, device, dtype):
        self.device = torch.device(device)
        self.dt = _hip.dtype_code(dtype)
        if self.dt not in (_hip.DT_BF16, _hip.DT_F16):
            raise ValueError("the StableDiffusion engines run in 'bf16' or 'f16'")
        _hip.lib()
        self.sd = state_dict
        self.w: Dict[str, object] = {}

    def _f32(self, k):
        return self.sd[k].detach().float().to(self.device).contiguous()

    def _lin(self, k, **kw):
        return PackedLinear(self.sd[k + ".weight"], self.sd.get(k + ".bias"), self.dt, self.device, **kw)

    def _pack_resnet(self, k, srcs=None):
        w = self.w
        w[k + ".gn1"] = (self._f32(k + ".norm1.weight"), self._f32(k + ".norm1.bias"))
        w[k + ".conv1"] = self._lin(k + ".conv1", sources=srcs)
        w[k + ".gn2"] = (self._f32(k + ".norm2.weight"), self._f32(k + ".norm2.bias"))
        w[k + ".conv2"] = self._lin(k + ".conv2")
        if k + ".conv_shortcut.weight" in self.sd:
            w[k + ".skip"] = self._lin(k + ".conv_shortcut", sources=srcs)

    def _resnet(self, k, x, x1, nbias, groups, eps, tape=None):
        """ResnetBlock2D on x (and the skip tensor x1 it concatenates).  Inference and training mode issue the same launches: with a tape,
        the block's record for _res_back (its inputs, both norms' coefficients and partials, conv1's output) is appended to it."""
        dt, w = self.dt, self.w
        gn1 = ops.group_norm_coeffs_train(x, *w[k + ".gn1"], groups, dt, x1=x1, eps=eps)
        h = ops.igemm(x, w[k + ".conv1"], a1=x1, nbias=nbias, prologue=(gn1[0], gn1[1], ACT_SILU), want_stats=True)
        gn2 = ops.group_norm_coeffs_train(h, *w[k + ".gn2"], groups, dt, eps=eps)
        skip = ops.igemm(x, w[k + ".skip"], a1=x1) if (k + ".skip") in w else x
        assert (k + ".skip") in w or x1 is None
        if tape is not None:
            tape.append(("res", k, x, x1, gn1, h, gn2))
        return ops.igemm(h, w[k + ".conv2"], residual=skip, prologue=(gn2[0], gn2[1], ACT_SILU), want_stats=True)

    def _res_back(self, rec, g, sd, groups, eps):
        """(gradient wrt x, wrt x1 or None) of the ResnetBlock2D recorded in `rec` from g = gradient wrt its output."""
        _, k, x, x1, gn1, h, gn2 = rec
        dt, w, dev = self.dt, self.w, self.device
        d_a2 = ops.igemm(g, ops.packed_dx(w, k + ".conv2T", sd[k + ".conv2.weight"], dt, dev))                  # wrt SiLU(GN2(h))
        dh, _ = ops.group_norm_backward(h, d_a2, *gn2, w[k + ".gn2"][0], groups, dt, act=ACT_SILU, eps=eps)
        d_a1 = ops.igemm(dh, ops.packed_dx(w, k + ".conv1T", sd[k + ".conv1.weight"], dt, dev))                 # wrt SiLU(GN1(cat(x, x1)))
        gs0, gs1 = g, None
        if (k + ".skip") in w:
            skw = sd[k + ".conv_shortcut.weight"]
            if x1 is None:
                gs0 = ops.igemm(g, ops.packed_dx(w, k + ".skipT", skw, dt, dev))
            else:
                c0 = x.shape[-1]
                gs0 = ops.igemm(g, ops.packed_dx(w, k + ".skipT0", skw[:, :c0], dt, dev))
                gs1 = ops.igemm(g, ops.packed_dx(w, k + ".skipT1", skw[:, c0:], dt, dev))
        return ops.group_norm_backward(x, d_a1, *gn1, w[k + ".gn1"][0], groups, dt, x1=x1, act=ACT_SILU, gadd0=gs0, gadd1=gs1, eps=eps)

    def _up_back(self, k, g, sd):
        """Gradient wrt the input of nearest-x2 + conv3x3 from g = gradient wrt its output [N, 2h, 2w, C]: one stride-2 pass on the
        phase-folded weights, faster at all three SD-v1 shapes than dX at the high resolution + the 2x2 sum."""
        if k + ".fold" not in self.w:
            self.w[k + ".fold"] = PackedLinear(fold_upsample_weights(sd[k + ".weight"].cpu()).float(), None, self.dt, self.device)
        return ops.igemm(g, self.w[k + ".fold"], stride=2)

    def _pack_vae_attention(self, a):
        sd = self.sd
        self.w[a + ".gn"] = (self._f32(a + ".group_norm.weight"), self._f32(a + ".group_norm.bias"))
        self.w[a + ".qkv"] = PackedLinear(torch.cat([sd[f"{a}.{nm}.weight"].float() for nm in ("query", "key", "value")], 0),
                                          torch.cat([sd[f"{a}.{nm}.bias"].float() for nm in ("query", "key", "value")], 0), self.dt, self.device)
        self.w[a + ".proj"] = self._lin(a + ".proj_attn")

    def _vae_attention(self, a, h, groups):
        """AttentionBlock (stable_diffusion/attention.py:71-117): GroupNorm -> q|k|v -> one head over all pixels -> proj + residual."""
        dt, w = self.dt, self.w
        n, h2, w2, cc = h.shape
        m = n * h2 * w2
        hn = ops.group_norm(h, *w[a + ".gn"], groups, dt, eps=1e-6)
        qkv = ops.igemm(hn.view(m, cc), w[a + ".qkv"])
        at = ops.attention(qkv.view(n, h2 * w2, 3 * cc), 1, 1, dt)
        o = ops.igemm(at.view(m, cc), w[a + ".proj"], residual=h.view(m, cc), want_stats=True, hw=h2 * w2)
        return ops.view_nhwc(o, n, h2, w2)


    # ---- what the VAE decoder's and encoder's input gradients share: the tape-keeping form of the mid attention (other kernels than
    # _vae_attention: the softmax P is kept) and the backward steps (see VaeDecoderEngine) -------------------------------------------------
    def _vae_attention_train(self, a, x, tape, groups):
        dt, w = self.dt, self.w
        n, h2, w2, cc = x.shape
        m = n * h2 * w2
        ca, cb, parts = ops.group_norm_coeffs_train(x, *w[a + ".gn"], groups, dt, eps=1e-6)
        hn = torch.empty_like(x)
        call("pmi_gn_apply", ptr(x), None, cc, ptr(ca), ptr(cb), None, ptr(hn), n, h2, w2, cc, ACT_NONE, 0, dt)
        qkv = ops.igemm(hn.view(m, cc), w[a + ".qkv"])
        at, pm = ops.attention_train(qkv.view(n, h2 * w2, 3 * cc), 1, dt)       # = ops.attention's batched-GEMM path (head dim > 160)
        o = ops.igemm(at.view(m, cc), w[a + ".proj"], residual=x.view(m, cc), want_stats=True, hw=h2 * w2)
        tape.append(("attn", a, x, (ca, cb, parts), qkv, pm))
        return ops.view_nhwc(o, n, h2, w2)

    def _vae_attn_back(self, rec, g, sd, groups):
        _, a, x, gn, qkv, pm = rec
        dt, w, dev = self.dt, self.w, self.device
        n, h2, w2, cc = x.shape
        t, m = h2 * w2, n * h2 * w2
        da = ops.igemm(g.view(m, cc), ops.packed_dx(w, a + ".projT", sd[a + ".proj_attn.weight"], dt, dev))
        dqkv = ops.attention_backward(qkv.view(n, t, 3 * cc), pm, da.view(n, t, cc), 1, dt)
        if a + ".qkvT" not in w:
            ops.packed_dx(w, a + ".qkvT", torch.cat([sd[f"{a}.{nm}.weight"].cpu() for nm in ("query", "key", "value")], 0), dt, dev)
        dhn = ops.igemm(dqkv.view(m, 3 * cc), w[a + ".qkvT"]).view(n, h2, w2, cc)
        gx, _ = ops.group_norm_backward(x, dhn, *gn, w[a + ".gn"][0], groups, dt, act=ACT_NONE, gadd0=g, eps=1e-6)
        return gx

    def _down_back(self, k, g, sd):
        """Gradient wrt the input of Downsample2D from g = gradient wrt its output [N, h, w, C]: one phased pmi_igemm launch writes the
        [N, 2h, 2w, C] result (ops.downsample_adjoint)."""
        if k + ".phase" not in self.w:
            self.w[k + ".phase"] = PackedLinear(pack_downsample_adjoint_weights(sd[k + ".weight"].cpu()).float(), None, self.dt, self.device)
        return ops.downsample_adjoint(g, self.w[k + ".phase"])

class SdUnetEngine(_Blocks):
    def __init__(self, cfg: SdConfig, state_dict: Dict[str, torch.Tensor], device, dtype="f16"):
        self._init_common(state_dict, device, dtype)
        self.cfg = cfg
        sd = state_dict
        self.down, self.mid, self.up = unet_plan(cfg)
        self.te1, self.te2 = self._lin("time_embedding.linear_1"), self._lin("time_embedding.linear_2")
        self.conv_in = self._lin("conv_in", cin_pad=(cfg.in_channels + 7) // 8 * 8)
        emb_w, emb_b, off = [], [], 0
        self.emb_off: Dict[str, Tuple[int, int]] = {}
        cat = lambda keys: torch.cat([sd[k].detach().float() for k in keys], dim=0)
        for blk in self.down + [self.mid] + self.up:
            for l in blk:
                if l[0] == "res":
                    k = l[1]
                    self._pack_resnet(k, l[4])
                    emb_w.append(sd[k + ".time_emb_proj.weight"].float()); emb_b.append(sd[k + ".time_emb_proj.bias"].float())
                    self.emb_off[k] = (off, l[3])
                    off += l[3]
                elif l[0] == "attn":
                    k, b, w = l[1], l[1] + ".transformer_blocks.0", self.w
                    w[k + ".gn"] = (self._f32(k + ".norm.weight"), self._f32(k + ".norm.bias"))
                    w[k + ".proj_in"], w[k + ".proj_out"] = self._lin(k + ".proj_in"), self._lin(k + ".proj_out")
                    for nm in ("norm1", "norm2", "norm3"):
                        w[f"{b}.{nm}"] = (self._f32(f"{b}.{nm}.weight"), self._f32(f"{b}.{nm}.bias"))
                    w[b + ".qkv1"] = PackedLinear(cat([b + ".attn1.to_q.weight", b + ".attn1.to_k.weight", b + ".attn1.to_v.weight"]), None, self.dt, self.device)
                    w[b + ".out1"] = self._lin(b + ".attn1.to_out.0")
                    w[b + ".q2"] = self._lin(b + ".attn2.to_q")
                    w[b + ".kv2"] = PackedLinear(cat([b + ".attn2.to_k.weight", b + ".attn2.to_v.weight"]), None, self.dt, self.device)
                    w[b + ".out2"] = self._lin(b + ".attn2.to_out.0")
                    wf, bf = ops.interleave_geglu(sd[b + ".ff.net.0.proj.weight"].detach().float(), sd[b + ".ff.net.0.proj.bias"].detach().float())
                    w[b + ".ff1"] = PackedLinear(wf, bf, self.dt, self.device)      # (16 value | 16 gate) column groups: GEGLU in the GEMM's epilogue
                    w[b + ".ff2"] = self._lin(b + ".ff.net.2")
                else:
                    self.w[l[1]] = self._lin(l[1])
        self.emb_all = PackedLinear(torch.cat(emb_w, 0), torch.cat(emb_b, 0), self.dt, self.device)
        self.gn_out = (self._f32("conv_norm_out.weight"), self._f32("conv_norm_out.bias"))
        self.conv_out = self._lin("conv_out")
        self.sd = None                                      # packed: drop the reference to the caller's tensors
        self._kv_cache: Tuple[Optional[tuple], Dict[str, torch.Tensor]] = (None, {})

    # ---- transformer block (attention.py:173-188, 236-247) -------------------------------------------
    def _ln(self, x32, gb, m, c):
        y = torch.empty((m, c), dtype=_hip.TORCH_DTYPE[self.dt], device=x32.device)
        call("pmi_layernorm_fwd", ptr(x32), c, ptr(gb[0]), ptr(gb[1]), ptr(y), None, None, m, c, 1e-5, self.dt)
        return y

    def _context_kv(self, context: torch.Tensor) -> Dict[str, torch.Tensor]:
        """k|v projections of the prompt encodings for every cross-attention layer; they depend on the conditioning only, so they
        are computed when a new context tensor is seen and reused over the sampling steps."""
        key = (context.data_ptr(), context._version, tuple(context.shape))
        if self._kv_cache[0] != key:
            n, tc, cd = context.shape
            c16 = torch.empty((n * tc, cd), dtype=_hip.TORCH_DTYPE[self.dt], device=self.device)
            ctx = context.float().contiguous()
            call("pmi_cast_f32_to_16", ptr(ctx), ptr(c16), ctx.numel(), ACT_NONE, self.dt)
            kv = {k: ops.igemm(c16, w) for k, w in self.w.items() if k.endswith(".kv2")}
            self._kv_cache = (key, kv, context)             # holding the tensor keeps its data_ptr from being recycled
        return self._kv_cache[1]

    def _attn(self, k, x, kv_all, tc):
        dt, w, heads = self.dt, self.w, self.cfg.heads
        n, hh, ww, c = x.shape
        t, m = hh * ww, n * hh * ww
        b = k + ".transformer_blocks.0"
        hn = ops.group_norm(x, *w[k + ".gn"], self.cfg.groups, dt, eps=1e-6)
        h = ops.igemm(hn.view(m, c), w[k + ".proj_in"], out_f32=True)                             # fp32 token stream [m, c]
        qkv = ops.igemm(self._ln(h, w[b + ".norm1"], m, c), w[b + ".qkv1"])
        a = ops.attention(qkv.view(n, t, 3 * c), heads, 1, dt)
        h = ops.igemm(a.view(m, c), w[b + ".out1"], residual=h, out_f32=True)
        q = ops.igemm(self._ln(h, w[b + ".norm2"], m, c), w[b + ".q2"])
        a = ops.cross_attention(q.view(n, t, c), kv_all[b + ".kv2"].view(n, tc, 2 * c), heads, dt)
        h = ops.igemm(a.view(m, c), w[b + ".out2"], residual=h, out_f32=True)
        gg = ops.geglu_linear(self._ln(h, w[b + ".norm3"], m, c), w[b + ".ff1"])                  # value * gelu(gate), [m, 4c]
        h16 = ops.igemm(gg, w[b + ".ff2"], residual=h)                                            # fp32 residual in, 16-bit tokens out
        out = ops.igemm(h16, w[k + ".proj_out"], residual=x.view(m, c), want_stats=True, hw=t)
        return ops.view_nhwc(out, n, hh, ww)

    def _run(self, blk, h, h1, emb, kv_all, tc, tape=None):
        """One block of the plan on h (and the skip tensor h1 its first ResnetBlock2D concatenates).  With a tape (training mode) every layer
        appends its record for _back."""
        for l in blk:
            if l[0] == "res":
                off, co = self.emb_off[l[1]]
                h = self._resnet(l[1], h, h1, emb[:, off:off + co], self.cfg.groups, 1e-5, tape)
            elif l[0] == "attn":
                h = self._attn(l[1], h, kv_all, tc) if tape is None else self._attn_train(l[1], h, kv_all, tc, tape)
            else:
                if tape is not None:
                    tape.append((l[0], l[1]))
                h = ops.igemm(h, self.w[l[1]], stride=2, want_stats=True) if l[0] == "down" else ops.igemm(h, self.w[l[1]], up=True, want_stats=True)
            h1 = None
        return h

    def _unet(self, emb, kv_all, tc, h, tape=None):
        """The U over down / mid / up from conv_in's output -> the input of the output norm.  tape: {"down": [], "mid": [], "up": []}, filled
        with one list of records per block (mid: the records themselves)."""
        def sub(key):
            if tape is None:
                return None
            tape[key].append([])
            return tape[key][-1]
        hs = [h]
        for blk in self.down:
            h = self._run(blk, h, None, emb, kv_all, tc, sub("down"))
            hs.append(h)
        h = self._run(self.mid, h, None, emb, kv_all, tc, None if tape is None else tape["mid"])
        for blk in self.up:
            h = self._run(blk, h, hs.pop(), emb, kv_all, tc, sub("up"))
        return h

    def _inputs(self, latents, timesteps, context):
        """Checked inputs -> (all time_emb_proj outputs [N, sum Cout] fp32, the context's k|v per layer, context length, conv_in's output)."""
        cfg, dt, dev = self.cfg, self.dt, self.device
        if not latents.is_cuda or not context.is_cuda:
            raise RuntimeError("SdUnetEngine runs on a HIP device only (no CPU fallback)")
        latents = latents.float().contiguous()
        n, cin, hh, ww = latents.shape
        levels = len(cfg.block_out) - 1
        if cin != cfg.in_channels or hh % (1 << levels) or ww % (1 << levels):
            raise ValueError(f"latents must be [N, {cfg.in_channels}, h, w] with h, w divisible by {1 << levels}")
        if context.ndim != 3 or context.shape[0] != n or context.shape[2] != cfg.context_dim:
            raise ValueError(f"context must be [N, T, {cfg.context_dim}] with N = {n}")
        tdt = _hip.TORCH_DTYPE[dt]
        t = timesteps.to(device=dev, dtype=torch.float32).contiguous()
        temb = torch.empty((n, cfg.block_out[0]), dtype=tdt, device=dev)
        call("pmi_timestep_embedding", ptr(t), ptr(temb), n, cfg.block_out[0], 10000.0, dt)
        e = ops.igemm(temb, self.te1, act=ACT_SILU)
        e = ops.igemm(e, self.te2, act=ACT_SILU)              # SiLU(emb): the only form the ResnetBlocks consume
        emb = ops.igemm(e, self.emb_all, out_f32=True)        # all time_emb_proj outputs, [N, sum Cout]
        kv_all, tc = self._context_kv(context), context.shape[1]
        cp = self.conv_in.cin_p
        x = torch.empty((n, hh, ww, cp), dtype=tdt, device=dev)
        call("pmi_nchw_to_nhwc", ptr(latents), ptr(x), n, cin, hh, ww, cp, 1.0, 0.0, dt)
        return emb, kv_all, tc, ops.igemm(x, self.conv_in, want_stats=True)

    def _output(self, h, ca, cb):
        cfg = self.cfg
        n, hh, ww, _ = h.shape
        y = ops.igemm(h, self.conv_out, out_f32=True, prologue=(ca, cb, ACT_SILU))
        out = torch.empty((n, cfg.out_channels, hh, ww), dtype=torch.float32, device=self.device)
        call("pmi_nhwc_to_nchw", ptr(y), y.shape[-1], ptr(out), n, hh, ww, cfg.out_channels, 1.0, 0.0)
        return out

    @torch.no_grad()
    def forward(self, latents: torch.Tensor, timesteps: torch.Tensor, context: torch.Tensor) -> torch.Tensor:
        """latents NCHW fp32 [N, in, h, w], timesteps [N], context [N, T, context_dim] fp32 -> predicted noise NCHW fp32."""
        emb, kv_all, tc, h = self._inputs(latents, timesteps, context)
        h = self._unet(emb, kv_all, tc, h)
        ca, cb = ops.group_norm_coeffs(h, *self.gn_out, self.cfg.groups, self.dt)
        return self._output(h, ca, cb)

    # ---- input gradient (d loss / d latents through the frozen UNet: what autograd gives upstream when the latents require grad) ------------
    # forward_train() issues forward()'s launch sequence and keeps what the nonlinear steps need.  Per ResnetBlock2D: its input(s), the GN1
    # coefficients and partials, conv1's output, the GN2 ones.  Per transformer block: its input and GroupNorm, the fp32 token stream in front
    # of each LayerNorm with mean_rstd, q|k|v / q with the attention output and log-sum-exp (flash route) or the softmax (kept-P route), and
    # ff1's pre-GEGLU output.  Samplers keep nothing; the time embedding and the context's k|v are constants of the backward.
    # The one launch that differs from forward(): ff1 runs without the fused GEGLU epilogue and pmi_geglu follows (the gate's input must
    # exist in memory).  Where forward() fuses it (weights-direct GEMM), eps differs at rounding level: the fused form gates the fp32
    # accumulator, the unfused one its 16-bit rounding; elsewhere forward_train() == forward() bit for bit.
    flash_backward = True       # False: attention through the kept-P route (ops.attention_train / attention_backward), for the A/B

    def _use_flash(self, c):
        d = c // self.cfg.heads
        return self.flash_backward and ops.FLASH_ENABLED and d <= 160 and d % 8 == 0

    def _ln_train(self, x32, gb, m, c):
        y = torch.empty((m, c), dtype=_hip.TORCH_DTYPE[self.dt], device=x32.device)
        mr = torch.empty((2, m), dtype=torch.float32, device=x32.device)
        call("pmi_layernorm_fwd", ptr(x32), c, ptr(gb[0]), ptr(gb[1]), ptr(y), None, ptr(mr), m, c, 1e-5, self.dt)
        return y, mr

    def _attn_train(self, k, x, kv_all, tc, tape):
        dt, w, heads = self.dt, self.w, self.cfg.heads
        n, hh, ww, c = x.shape
        t, m, d = hh * ww, n * hh * ww, c // heads
        b = k + ".transformer_blocks.0"
        flash = self._use_flash(c)
        ca, cb, parts = ops.group_norm_coeffs_train(x, *w[k + ".gn"], self.cfg.groups, dt, eps=1e-6)
        hn = torch.empty_like(x)
        call("pmi_gn_apply", ptr(x), None, c, ptr(ca), ptr(cb), None, ptr(hn), n, hh, ww, c, ACT_NONE, 0, dt)
        h0 = ops.igemm(hn.view(m, c), w[k + ".proj_in"], out_f32=True)
        z, mr1 = self._ln_train(h0, w[b + ".norm1"], m, c)
        qkv = ops.igemm(z, w[b + ".qkv1"]).view(n, t, 3 * c)
        if flash:
            a, s1 = ops.flash_attention_train(qkv, qkv[..., c:], qkv[..., 2 * c:], heads, d, dt)
        else:
            a, pm = ops.attention_train(qkv, heads, dt)
            s1 = (qkv, pm)
        h1 = ops.igemm(a.view(m, c), w[b + ".out1"], residual=h0, out_f32=True)
        z, mr2 = self._ln_train(h1, w[b + ".norm2"], m, c)
        q = ops.igemm(z, w[b + ".q2"]).view(n, t, c)
        kv = kv_all[b + ".kv2"].view(n, tc, 2 * c)
        if flash:
            a, s2 = ops.flash_attention_train(q, kv, kv[..., c:], heads, d, dt)
        else:
            a, pm = ops.cross_attention_train(q, kv, heads, dt)
            s2 = (kv, pm)
        h2 = ops.igemm(a.view(m, c), w[b + ".out2"], residual=h1, out_f32=True)
        z, mr3 = self._ln_train(h2, w[b + ".norm3"], m, c)
        f = ops.igemm(z, w[b + ".ff1"])                                             # pre-GEGLU, (16 value | 16 gate) column groups: kept
        gg = torch.empty((m, 4 * c), dtype=f.dtype, device=f.device)
        call("pmi_geglu", ptr(f), ptr(gg), m, 4 * c, 1, dt)
        h16 = ops.igemm(gg, w[b + ".ff2"], residual=h2)
        out = ops.igemm(h16, w[k + ".proj_out"], residual=x.view(m, c), want_stats=True, hw=t)
        tape.append(("attn", k, x, (ca, cb, parts), (h0, mr1, s1), (h1, mr2, s2), (h2, mr3, f), flash))
        return ops.view_nhwc(out, n, hh, ww)

    @torch.no_grad()
    def forward_train(self, latents: torch.Tensor, timesteps: torch.Tensor, context: torch.Tensor):
        """As forward(), keeping what backward() needs: (predicted noise NCHW fp32, tape)."""
        emb, kv_all, tc, h = self._inputs(latents, timesteps, context)
        tape = {"down": [], "mid": [], "up": [], "in_shape": tuple(latents.shape), "ctx_shape": tuple(context.shape)}
        h = self._unet(emb, kv_all, tc, h, tape)
        gn = ops.group_norm_coeffs_train(h, *self.gn_out, self.cfg.groups, self.dt)
        tape["last"] = (h, gn)
        out = self._output(h, gn[0], gn[1])
        tape["out_shape"] = tuple(out.shape)
        return out, tape

    def _ln_back(self, dy32, x32, gb, mr, gres, m, c):
        """(fp32, 16-bit) gradient wrt the token stream in front of a LayerNorm: LayerNorm backward of dy32 plus gres, the gradient that
        reaches the same stream through the residual connection."""
        g32 = torch.empty((m, c), dtype=torch.float32, device=x32.device)
        g16 = torch.empty((m, c), dtype=_hip.TORCH_DTYPE[self.dt], device=x32.device)
        call("pmi_layernorm_bwd", ptr(dy32), ptr(x32), ptr(gb[0]), ptr(mr), ptr(gres), ptr(g32), ptr(g16), m, c, c, 1, self.dt)
        return g32, g16

    def _ctx_back(self, b, dkv, sd, cg):
        """One cross-attention layer's share of d loss / d context: dkv [N, Tc, 2C] fp32 times (to_k | to_v) [2C, context_dim], added to the
        running sum cg["acc"] in the GEMM's epilogue (layers in the backward's order: a fixed order).  All fp32 (csrc/f32gemm.hip): dK / dV sum
        up to T = 4096 terms and dK = dS^T Q has no bound in terms of the cotangent, so no 16-bit hand-over can be argued free of overflow in
        f16; an fp32 operand needs no argument.  The weights are the forward's 16-bit operands widened (the gradient of the function the
        forward computes), kept on the engine like every transposed weight.  alpha divides the f16 cotangent scale out."""
        key = b + ".kv2T"
        if key not in self.w:
            wkv = torch.cat([sd[b + ".attn2.to_k.weight"].to(self.device), sd[b + ".attn2.to_v.weight"].to(self.device)], 0)
            self.w[key] = wkv.float().to(_hip.TORCH_DTYPE[self.dt]).float().contiguous()        # rounded on the device, once
        wkv = self.w[key]
        n, tc, c2 = dkv.shape
        out = torch.empty((n * tc, wkv.shape[1]), dtype=torch.float32, device=self.device)
        ops.gemm_f32(dkv, wkv, out, M=n * tc, N=wkv.shape[1], K=c2, lda=c2, ldb=wkv.shape[1], ldd=wkv.shape[1], trans_b=True,
                     alpha=cg["mul"], residual=cg["acc"])
        cg["acc"] = out

    def _attn_back(self, rec, g, sd, cg=None):
        _, k, x, gn, (h0, mr1, s1), (h1, mr2, s2), (h2, mr3, f), flash = rec
        dt, w, dev, heads = self.dt, self.w, self.device, self.cfg.heads
        n, hh, ww, c = x.shape
        t, m, d = hh * ww, n * hh * ww, c // heads
        b = k + ".transformer_blocks.0"
        T = lambda key, wt: ops.packed_dx(w, key, wt, dt, dev)
        g = g.contiguous()
        gh32 = ops.igemm(g.view(m, c), T(k + ".proj_outT", sd[k + ".proj_out.weight"]), out_f32=True)          # wrt ff2's output = wrt h2 (residual)
        gh16 = torch.empty((m, c), dtype=g.dtype, device=dev)
        call("pmi_cast_f32_to_16", ptr(gh32), ptr(gh16), gh32.numel(), ACT_NONE, dt)
        d_gg = ops.igemm(gh16, T(b + ".ff2T", sd[b + ".ff.net.2.weight"]))
        d_f = ops.geglu_backward(f, d_gg, dt)
        if b + ".ff1T" not in w:
            T(b + ".ff1T", ops.interleave_geglu(sd[b + ".ff.net.0.proj.weight"].detach().cpu().float(), None)[0])
        d_z = ops.igemm(d_f, w[b + ".ff1T"], out_f32=True)
        gh32, gh16 = self._ln_back(d_z, h2, w[b + ".norm3"], mr3, gh32, m, c)                                    # wrt h2
        d_a = ops.igemm(gh16, T(b + ".out2T", sd[b + ".attn2.to_out.0.weight"])).view(n, t, c)
        if cg is None:
            dq = ops.flash_attention_backward(s2, d_a, heads, d, dt, dq_only=True) if flash else ops.cross_attention_backward(s2[0], s2[1], d_a, heads, dt)
        else:
            if flash:
                dq, dkv = ops.flash_attention_backward(s2, d_a, heads, d, dt)
            else:       # the kept-P tape holds no q (it stays what the latent-only backward keeps): the forward's two launches again, same bits
                q = ops.igemm(self._ln(h1, w[b + ".norm2"], m, c), w[b + ".q2"]).view(n, t, c)
                dq, dkv = ops.cross_attention_backward(s2[0], s2[1], d_a, heads, dt, q=q)
            self._ctx_back(b, dkv, sd, cg)
        d_z = ops.igemm(dq.view(m, c), T(b + ".q2T", sd[b + ".attn2.to_q.weight"]), out_f32=True)
        gh32, gh16 = self._ln_back(d_z, h1, w[b + ".norm2"], mr2, gh32, m, c)                                    # wrt h1
        d_a = ops.igemm(gh16, T(b + ".out1T", sd[b + ".attn1.to_out.0.weight"])).view(n, t, c)
        dqkv = ops.flash_attention_backward(s1, d_a, heads, d, dt) if flash else ops.attention_backward(s1[0], s1[1], d_a, heads, dt)
        if b + ".qkv1T" not in w:
            T(b + ".qkv1T", torch.cat([sd[f"{b}.attn1.{nm}.weight"].detach().cpu().float() for nm in ("to_q", "to_k", "to_v")], 0))
        d_z = ops.igemm(dqkv.view(m, 3 * c), w[b + ".qkv1T"], out_f32=True)
        gh32, gh16 = self._ln_back(d_z, h0, w[b + ".norm1"], mr1, gh32, m, c)                                    # wrt h0
        d_hn = ops.igemm(gh16, T(k + ".proj_inT", sd[k + ".proj_in.weight"])).view(n, hh, ww, c)
        gx, _ = ops.group_norm_backward(x, d_hn, *gn, w[k + ".gn"][0], self.cfg.groups, dt, act=ACT_NONE, gadd0=g, eps=1e-6)
        return gx

    def _back(self, tp, g, sd, cg=None):
        """Gradient wrt the input(s) of the layers recorded in `tp` from g = gradient wrt their output: (g_in, g_skip or None).
        cg: the context gradient's running state (backward(cond_grad=True)), None when the prompt is a constant."""
        g1 = None
        for rec in reversed(tp):
            assert g1 is None
            if rec[0] == "res":
                g, g1 = self._res_back(rec, g, sd, self.cfg.groups, 1e-5)
            elif rec[0] == "attn":
                g = self._attn_back(rec, g, sd, cg)
            elif rec[0] == "up":
                g = self._up_back(rec[1], g, sd)
            else:      # stride-2 convolution: dX = stride-1 convolution of the zero-inserted gradient with the flipped weights
                n, h_, w_, c = g.shape
                z = torch.zeros((n, 2 * h_, 2 * w_, c), dtype=g.dtype, device=g.device)
                z[:, ::2, ::2] = g
                g = ops.igemm(z, ops.packed_dx(self.w, rec[1] + "T", sd[rec[1] + ".weight"], self.dt, self.device))
        return g, g1

    @torch.no_grad()
    def backward(self, tape, d_eps: torch.Tensor, state_dict, cond_grad: bool = False):
        """d loss / d latents (NCHW fp32 [N, in, h, w]) from d loss / d eps (NCHW fp32, forward_train()'s output shape) and its tape.
        `state_dict`: the UNet's tensors by name (StableDiffusion.unet.state_dict()); transposed / folded weights are packed from it on first
        use and kept on the engine.  cond_grad=True: (d_latents, d_context), d_context fp32 [N, Tc, context_dim] = d loss / d context, the sum
        over the cross-attention layers of (dK | dV) (to_k | to_v); d_latents has the bits of the cond_grad=False call.  Timesteps get no
        gradient.  f16 engines scale the gradient by a power of two on the way in and back on the way out (ops.grad_to_nhwc), for both results;
        bf16 needs no scaling."""
        cfg, dt, dev, w = self.cfg, self.dt, self.device, self.w
        if not d_eps.is_cuda:
            raise RuntimeError("SdUnetEngine runs on a HIP device only (no CPU fallback)")
        if tuple(d_eps.shape) != tape["out_shape"]:
            raise ValueError(f"d_eps must have the output's shape {tape['out_shape']}, got {tuple(d_eps.shape)}")
        sd = {k: v.detach() for k, v in state_dict.items()}
        g, gscale = ops.grad_to_nhwc(d_eps, dt, dev)
        cg = {"acc": None, "mul": 1.0 / gscale} if cond_grad else None
        h, gn = tape["last"]
        d_act = ops.igemm(g, ops.packed_dx(w, "conv_outT", sd["conv_out.weight"], dt, dev, cin_pad=8))
        g, _ = ops.group_norm_backward(h, d_act, *gn, self.gn_out[0], cfg.groups, dt, act=ACT_SILU)
        g_hs = []                                               # gradients of the skip tensors: the last up block read hs[0], ...
        for tp in reversed(tape["up"]):
            g, gk = self._back(tp, g, sd, cg)
            g_hs.append(gk)
        g, _ = self._back(tape["mid"], g, sd, cg)
        for i in range(len(tape["down"]) - 1, -1, -1):          # hs[i + 1], the output of down block i, feeds the next block AND an up block
            g, _ = self._back(tape["down"][i], ops.add2(g, g_hs[i + 1], dt), sd, cg)
        g = ops.add2(g, g_hs[0], dt)
        gx = ops.igemm(g, ops.packed_dx(w, "conv_inT", sd["conv_in.weight"], dt, dev, rows=self.conv_in.cin_p), out_f32=True)
        gx = ops.grad_to_nchw(gx, cfg.in_channels, 1.0 / gscale)
        if not cond_grad:
            return gx
        if cg["acc"] is None:
            raise RuntimeError("cond_grad: this UNet configuration has no cross-attention layer")
        return gx, cg["acc"].view(tape["ctx_shape"])


class VaeDecoderEngine(_Blocks):
    """AutoencoderKL.decode (stable_diffusion.py:195-198): latents / 0.18215 -> post_quant_conv -> decoder -> (x + 1) / 2."""

    def __init__(self, cfg: VaeConfig, state_dict: Dict[str, torch.Tensor], device, dtype="bf16"):
        self._init_common(state_dict, device, dtype)
        self.cfg = cfg
        sd = state_dict
        # post_quant_conv (1x1, 4 -> 4) with its output channels zero-padded to the 8 the next convolution reads
        lc, lp = cfg.latent_channels, (cfg.latent_channels + 7) // 8 * 8
        wq = torch.zeros((lp, lc, 1, 1)); wq[:lc] = sd["post_quant_conv.weight"].detach().float()
        bq = torch.zeros(lp); bq[:lc] = sd["post_quant_conv.bias"].detach().float()
        self.pq = PackedLinear(wq, bq, self.dt, self.device, cin_pad=lp)
        self.conv_in = self._lin("decoder.conv_in", cin_pad=lp)
        self._pack_resnet("decoder.mid_block.resnets.0"); self._pack_resnet("decoder.mid_block.resnets.1")
        self._pack_vae_attention("decoder.mid_block.attentions.0")
        self.plan = []
        for i, o in enumerate(reversed(cfg.block_out)):
            for j in range(cfg.layers_per_block + 1):
                k = f"decoder.up_blocks.{i}.resnets.{j}"
                self._pack_resnet(k)
                self.plan.append(("res", k))
            if i != len(cfg.block_out) - 1:
                k = f"decoder.up_blocks.{i}.upsamplers.0.conv"
                self.w[k] = self._lin(k)
                self.plan.append(("up", k))
        self.gn_out = (self._f32("decoder.conv_norm_out.weight"), self._f32("decoder.conv_norm_out.bias"))
        self.conv_out = self._lin("decoder.conv_out")
        self.sd = None

    def _conv_in(self, latents, scale):
        """latents NCHW fp32 -> latents * scale as NHWC 16-bit -> post_quant_conv -> conv_in (with its GroupNorm statistics)."""
        cfg, dt = self.cfg, self.dt
        if not latents.is_cuda:
            raise RuntimeError("VaeDecoderEngine runs on a HIP device only (no CPU fallback)")
        latents = latents.float().contiguous()
        n, c, hh, ww = latents.shape
        if c != cfg.latent_channels:
            raise ValueError(f"latents must have {cfg.latent_channels} channels")
        x = torch.empty((n, hh, ww, self.pq.cin_p), dtype=_hip.TORCH_DTYPE[dt], device=self.device)
        call("pmi_nchw_to_nhwc", ptr(latents), ptr(x), n, c, hh, ww, self.pq.cin_p, float(scale), 0.0, dt)
        return ops.igemm(ops.igemm(x, self.pq), self.conv_in, want_stats=True)

    def _output(self, h, ca, cb, to_images):
        """conv_out on SiLU(GroupNorm(h)) given the norm's coefficients -> NCHW fp32 images in [0, 1] (to_images) or x in [-1, 1]."""
        y = ops.igemm(h, self.conv_out, out_f32=True, prologue=(ca, cb, ACT_SILU))
        n, ho, wo, _ = y.shape
        out = torch.empty((n, self.cfg.out_channels, ho, wo), dtype=torch.float32, device=self.device)
        mul, add = (0.5, 0.5) if to_images else (1.0, 0.0)          # diffusion_space.decode: (x + 1) / 2
        call("pmi_nhwc_to_nchw", ptr(y), y.shape[-1], ptr(out), n, ho, wo, self.cfg.out_channels, mul, add)
        return out

    def _blocks(self, h, rec=None):
        """The mid block and the up blocks from conv_in's output -> the input of the output norm.  With rec (training mode) every layer appends
        its record for backward()."""
        g, eps, a = self.cfg.groups, 1e-6, "decoder.mid_block.attentions.0"
        h = self._resnet("decoder.mid_block.resnets.0", h, None, None, g, eps, rec)
        h = self._vae_attention(a, h, g) if rec is None else self._vae_attention_train(a, h, rec, g)
        h = self._resnet("decoder.mid_block.resnets.1", h, None, None, g, eps, rec)
        for kind, k in self.plan:
            if kind == "res":
                h = self._resnet(k, h, None, None, g, eps, rec)
            else:
                if rec is not None:
                    rec.append(("up", k))
                h = ops.igemm(h, self.w[k], up=True, want_stats=True)
        return h

    @torch.no_grad()
    def forward(self, latents: torch.Tensor, scale: float = 1.0 / 0.18215, to_images: bool = True) -> torch.Tensor:
        """latents NCHW fp32 (the UNet's space) -> images NCHW fp32 in [0, 1] (to_images) or the decoder's x in [-1, 1]."""
        h = self._blocks(self._conv_in(latents, scale))
        ca, cb = ops.group_norm_coeffs(h, *self.gn_out, self.cfg.groups, self.dt, eps=1e-6)
        return self._output(h, ca, cb, to_images)

    # ---- input gradient (d loss / d latents through the frozen decoder: loss-guided sampling) -----------------------------------------
    # forward_train() issues forward()'s launch sequence and keeps the operands of every nonlinear step: per ResnetBlock2D its input x,
    # the GN1 coefficients and statistics partials, conv1's output h and the GN2 ones; for the mid attention its input, GN, q|k|v and the
    # softmax P; the last h with its GN.  The up-samplers and every convolution are linear in their input: nothing is kept for them.
    # backward() walks the tape once.  A convolution's dX is pmi_igemm on transposed, flipped weights; GroupNorm + SiLU backward is
    # pmi_gn_bwd_*; the attention's is ops.attention_backward on the kept P; an up-sampler's adjoint is one stride-2 4x4-tap pmi_igemm on
    # phase-folded weights (fold_upsample_weights) instead of dX at the high resolution + pmi_upsample_nearest2_bwd.
    @torch.no_grad()
    def forward_train(self, latents: torch.Tensor, scale: float = 1.0 / 0.18215, to_images: bool = True):
        """As forward(), keeping what backward() needs: (images NCHW fp32, tape).  For head dims above 160 (SD-v1: 512) the value equals
        forward()'s bit for bit; a 64-channel head runs forward()'s d64 kernel there and the batched GEMMs here (rounding-level)."""
        rec: List[tuple] = []
        h = self._blocks(self._conv_in(latents, scale), rec)
        gn = ops.group_norm_coeffs_train(h, *self.gn_out, self.cfg.groups, self.dt, eps=1e-6)
        out = self._output(h, gn[0], gn[1], to_images)
        tape = {"rec": rec, "last": (h, gn), "scale": float(scale), "to_images": bool(to_images),
                "in_shape": tuple(latents.shape), "out_shape": tuple(out.shape)}
        return out, tape

    @torch.no_grad()
    def backward(self, tape, d_out: torch.Tensor, state_dict) -> torch.Tensor:
        """d loss / d latents (NCHW fp32) from d loss / d output (NCHW fp32, the shape forward_train() returned) and its tape.
        `state_dict`: the decoder's tensors by name (StableDiffusion.vae.state_dict()); the transposed / folded weights are packed from it on
        the first call and kept on the engine.  f16 engines scale the gradient by a power of two on the way in and back on the way out
        (ops.grad_to_nhwc); bf16 needs no scaling."""
        cfg, dt, dev, w = self.cfg, self.dt, self.device, self.w
        if not d_out.is_cuda:
            raise RuntimeError("VaeDecoderEngine runs on a HIP device only (no CPU fallback)")
        if tuple(d_out.shape) != tape["out_shape"]:
            raise ValueError(f"d_out must have the output's shape {tape['out_shape']}, got {tuple(d_out.shape)}")
        sd = state_dict
        g_, eps = cfg.groups, 1e-6
        g, gscale = ops.grad_to_nhwc(d_out, dt, dev, mul=0.5 if tape["to_images"] else 1.0)
        h, gn = tape["last"]
        d_act = ops.igemm(g, ops.packed_dx(w, "decoder.conv_outT", sd["decoder.conv_out.weight"], dt, dev, cin_pad=8))
        g, _ = ops.group_norm_backward(h, d_act, *gn, self.gn_out[0], g_, dt, act=ACT_SILU, eps=eps)
        for rec in reversed(tape["rec"]):
            if rec[0] == "res":
                g, _ = self._res_back(rec, g, sd, g_, eps)
            elif rec[0] == "attn":
                g = self._vae_attn_back(rec, g, sd, g_)
            else:
                g = self._up_back(rec[1], g, sd)
        lp = self.pq.cin_p
        gz = ops.igemm(g, ops.packed_dx(w, "decoder.conv_inT", sd["decoder.conv_in.weight"], dt, dev, rows=lp))   # [.., lp]: rows past 4 are 0
        pqt = ops.packed_dx(w, "post_quant_convT", sd["post_quant_conv.weight"], dt, dev, rows=lp)                  # 1x1, 4 -> 4 padded to lp
        gx = ops.igemm(gz, pqt, out_f32=True)                                                                      # [n, h, w, lp] fp32
        return ops.grad_to_nchw(gx, cfg.latent_channels, tape["scale"] / gscale)


class VaeEncoderEngine(_Blocks):
    """AutoencoderKL.encode (stable_diffusion.py:176-192): images -> 2*img-1 -> encoder -> quant_conv -> (mean, logvar)."""

    def __init__(self, cfg: VaeConfig, state_dict: Dict[str, torch.Tensor], device, dtype="bf16"):
        self._init_common(state_dict, device, dtype)
        self.cfg = cfg
        self.conv_in = self._lin("encoder.conv_in", cin_pad=8)
        self.plan = []
        for i, o in enumerate(cfg.block_out):
            for j in range(cfg.layers_per_block):
                k = f"encoder.down_blocks.{i}.resnets.{j}"
                self._pack_resnet(k)
                self.plan.append(("res", k))
            if i != len(cfg.block_out) - 1:
                k = f"encoder.down_blocks.{i}.downsamplers.0.conv"
                self.w[k] = self._lin(k)
                self.plan.append(("down", k))
        self._pack_resnet("encoder.mid_block.resnets.0"); self._pack_resnet("encoder.mid_block.resnets.1")
        self._pack_vae_attention("encoder.mid_block.attentions.0")
        self.gn_out = (self._f32("encoder.conv_norm_out.weight"), self._f32("encoder.conv_norm_out.bias"))
        self.conv_out = self._lin("encoder.conv_out")
        self.quant = (self._f32("quant_conv.weight").flatten(1), self._f32("quant_conv.bias"))
        self.sd = None

    def _down(self, h, lin):
        """Downsample2D(padding=0): pad right/bottom by one, 3x3 stride-2 conv without padding.  Run as the symmetric pad-1 stride-2
        convolution on a copy with a one-pixel zero frame: its output (oy+1, ox+1) reads exactly x[2oy..2oy+2, 2ox..2ox+2]."""
        n, hh, ww, c = h.shape
        xp = torch.zeros((n, hh + 2, ww + 2, c), dtype=h.dtype, device=h.device)
        xp[:, 1:hh + 1, 1:ww + 1] = h
        return ops.igemm(xp, lin, stride=2)[:, 1:, 1:].contiguous()

    def _conv_in(self, images):
        """images NCHW fp32 in [0, 1] -> 2*img - 1 as NHWC 16-bit (3 channels padded to 8) -> conv_in (with its GroupNorm statistics)."""
        cfg, dt, dev = self.cfg, self.dt, self.device
        if not images.is_cuda:
            raise RuntimeError("VaeEncoderEngine runs on a HIP device only (no CPU fallback)")
        images = images.float().contiguous()
        n, c, hh, ww = images.shape
        down = 1 << (len(cfg.block_out) - 1)
        if c != cfg.out_channels or hh % down or ww % down:
            raise ValueError(f"images must be [N, {cfg.out_channels}, H, W] with H, W divisible by {down}")
        x = torch.empty((n, hh, ww, 8), dtype=_hip.TORCH_DTYPE[dt], device=dev)
        call("pmi_nchw_to_nhwc", ptr(images), ptr(x), n, c, hh, ww, 8, 2.0, -1.0, dt)      # diffusion_space.encode: 2*img - 1
        return ops.igemm(x, self.conv_in, want_stats=True)

    def _output(self, h, ca, cb):
        """conv_out on SiLU(GroupNorm(h)) given the norm's coefficients -> quant_conv -> (mean, logvar) NCHW fp32."""
        dev = self.device
        y = ops.igemm(h, self.conv_out, out_f32=True, prologue=(ca, cb, ACT_SILU))        # [n, h/8, w/8, 8] fp32
        n, ho, wo, c2 = y.shape
        m = n * ho * wo
        mom = ops.linear_f32(y.view(m, c2), self.quant[0], self.quant[1])                  # quant_conv (1x1, 8 -> 8) in exact fp32
        out = torch.empty((n, c2, ho, wo), dtype=torch.float32, device=dev)
        call("pmi_nhwc_to_nchw", ptr(mom), c2, ptr(out), n, ho, wo, c2, 1.0, 0.0)
        lc = self.cfg.latent_channels
        return out[:, :lc].contiguous(), out[:, lc:2 * lc].contiguous()

    def _blocks(self, h, rec=None):
        """The down blocks and the mid block from conv_in's output -> the input of the output norm.  With rec (training mode) every layer
        appends its record for backward()."""
        g, eps, a = self.cfg.groups, 1e-6, "encoder.mid_block.attentions.0"
        for kind, k in self.plan:
            if kind == "res":
                h = self._resnet(k, h, None, None, g, eps, rec)
            else:
                if rec is not None:
                    rec.append(("down", k))
                h = self._down(h, self.w[k])
        h = self._resnet("encoder.mid_block.resnets.0", h, None, None, g, eps, rec)
        h = self._vae_attention(a, h, g) if rec is None else self._vae_attention_train(a, h, rec, g)
        return self._resnet("encoder.mid_block.resnets.1", h, None, None, g, eps, rec)

    @torch.no_grad()
    def forward(self, images: torch.Tensor):
        """images NCHW fp32 in [0, 1] -> (mean, logvar) NCHW fp32 [N, latent, H/8, W/8] of the latent distribution."""
        h = self._blocks(self._conv_in(images))
        ca, cb = ops.group_norm_coeffs(h, *self.gn_out, self.cfg.groups, self.dt, eps=1e-6)
        return self._output(h, ca, cb)

    # ---- input gradient (d loss / d images through the frozen encoder: pixel-space optimisation against SD) ---------------------------
    # The decoder's scheme (VaeDecoderEngine) in the other direction.  forward_train() issues forward()'s launch sequence and keeps, per
    # ResnetBlock2D, x, the GN1 coefficients and partials, h and the GN2 ones; for the mid attention its input, GN, q|k|v and P; the last h
    # with its GN.  Down-samplers and convolutions are linear: nothing is kept.  backward() walks the tape once: quant_conv^T, conv_out^T,
    # GroupNorm + SiLU backward, the mid block, the plan in reverse (_res_back; a down-sampler's adjoint is ONE phased pmi_igemm launch,
    # _down_back), conv_in^T with fp32 output, NCHW.
    @torch.no_grad()
    def forward_train(self, images: torch.Tensor):
        """As forward(), keeping what backward() needs: ((mean, logvar), tape).  For head dims above 160 (SD-v1: 512) the values equal
        forward()'s bit for bit; a 64-channel mid attention runs forward()'s d64 kernel there and the batched GEMMs here (rounding-level)."""
        rec: List[tuple] = []
        h = self._blocks(self._conv_in(images), rec)
        gn = ops.group_norm_coeffs_train(h, *self.gn_out, self.cfg.groups, self.dt, eps=1e-6)
        mean, logvar = self._output(h, gn[0], gn[1])
        tape = {"rec": rec, "last": (h, gn), "in_shape": tuple(images.shape), "out_shape": tuple(mean.shape)}
        return (mean, logvar), tape

    def _quant_back(self, sd, both: bool) -> PackedLinear:
        """quant_conv^T (1x1, 8 -> 8) over the cotangent as it arrives: d_mean and d_logvar are separate 4-channel tensors, each laid out as
        an 8-channel NHWC tensor (channels 4..7 zero), read through the two source pointers of one pmi_igemm launch -- K = 16 with the
        rows of quant_conv's weight for (mean | 0 | logvar | 0); `both` False: d_logvar = 0, K = 8."""
        key = "quant_convT2" if both else "quant_convT1"
        if key not in self.w:
            lc = self.cfg.latent_channels
            wq = sd["quant_conv.weight"].detach().cpu().double().flatten(1)                  # [2 lc (moments), 2 lc (conv_out channels)]
            wt = torch.zeros((2 * lc, 16 if both else 8), dtype=torch.float64)
            wt[:, :lc] = wq[:lc].t()
            if both:
                wt[:, 8:8 + lc] = wq[lc:].t()
            self.w[key] = PackedLinear(wt.float(), None, self.dt, self.device)
        return self.w[key]

    @torch.no_grad()
    def backward(self, tape, d_mean: torch.Tensor, d_logvar: Optional[torch.Tensor], state_dict) -> torch.Tensor:
        """d loss / d images (NCHW fp32, the images' shape, including the factor 2 of 2*img - 1) from d loss / d mean and d loss / d logvar
        (NCHW fp32, the shape of forward_train()'s moments; d_logvar None = zero) and its tape.  `state_dict`: the VAE's tensors by name
        (StableDiffusion.vae.state_dict()); the transposed and phase-packed weights are packed from it on the first call and kept on the
        engine.  f16 engines scale the cotangent by ONE power of two over both tensors on the way in and back on the way out (the rule of
        ops.grad_to_nhwc); bf16 needs no scaling."""
        cfg, dt, dev, w = self.cfg, self.dt, self.device, self.w
        parts = [d_mean] if d_logvar is None else [d_mean, d_logvar]
        for d in parts:
            if not d.is_cuda:
                raise RuntimeError("VaeEncoderEngine runs on a HIP device only (no CPU fallback)")
            if tuple(d.shape) != tape["out_shape"]:
                raise ValueError(f"d_mean / d_logvar must have the moments' shape {tape['out_shape']}, got {tuple(d.shape)}")
        sd = state_dict
        g_, eps = cfg.groups, 1e-6
        parts = [d.float().contiguous() for d in parts]
        n, lc, ho, wo = parts[0].shape
        gscale = 1.0
        if dt == _hip.DT_F16:
            amax = torch.empty((len(parts), n), dtype=torch.float32, device=dev)
            for i, d in enumerate(parts):
                call("pmi_quantile_abs", ptr(d), ptr(amax[i]), n, lc * ho * wo, 1.0)
            gscale = ops.f16_grad_scale(amax.flatten().tolist())
        gs = []
        for d in parts:
            gq = torch.empty((n, ho, wo, 8), dtype=_hip.TORCH_DTYPE[dt], device=dev)
            call("pmi_nchw_to_nhwc", ptr(d), ptr(gq), n, lc, ho, wo, 8, gscale, 0.0, dt)
            gs.append(gq)
        g = ops.igemm(gs[0].view(-1, 8), self._quant_back(sd, len(gs) == 2), a1=gs[1].view(-1, 8) if len(gs) == 2 else None).view(n, ho, wo, 8)
        h, gn = tape["last"]
        d_act = ops.igemm(g, ops.packed_dx(w, "encoder.conv_outT", sd["encoder.conv_out.weight"], dt, dev))
        g, _ = ops.group_norm_backward(h, d_act, *gn, self.gn_out[0], g_, dt, act=ACT_SILU, eps=eps)
        for rec in reversed(tape["rec"]):
            if rec[0] == "res":
                g, _ = self._res_back(rec, g, sd, g_, eps)
            elif rec[0] == "attn":
                g = self._vae_attn_back(rec, g, sd, g_)
            else:
                g = self._down_back(rec[1], g, sd)
        gx = ops.igemm(g, ops.packed_dx(w, "encoder.conv_inT", sd["encoder.conv_in.weight"], dt, dev), out_f32=True)      # [n, H, W, 4] fp32
        return ops.grad_to_nchw(gx, cfg.out_channels, 2.0 / gscale)
