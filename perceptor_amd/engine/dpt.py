"""HIP engine for the DPT depth network (MiDaS ``dpt_large``): forward and the gradient of the depth map w.r.t. the input image.

Replaces perceptor/models/midas_depth (DPTDepthModel over timm's ViT-L/16 at 384 x 384, dpt_depth.py:64-105, vit.py:56-97, blocks.py:260-391)
+ autograd on the guidance path.  The weights are frozen, so the backward is one dX GEMM per convolution, the ReLU masks and the adjoints of
the layout steps.

  tower        engine/vit.py with timm's flavour (exact GELU, LayerNorm eps 1e-6, no ln_pre, no pooled head), the residual stream tapped at four
               blocks (the reference's forward hooks); the four gradients re-enter the tower's backward walk at their blocks
  readout      ProjectReadout: GELU(Linear([tok | cls])) = GELU(tok Wa^T + (cls Wb^T + b)): no concatenation, the class part is a per-image
               row bias of the patch GEMM
  reassemble   1 x 1 convolution, then ConvTranspose 4 x 4 / 4 (tap 1), 2 x 2 / 2 (tap 2) = one GEMM to k k C columns + pmi_depth_to_space,
               nothing (tap 3), Conv 3 x 3 stride 2 (tap 4)
  fusion       layer{k}_rn (3 x 3, no bias), then per block: (+ resConfUnit1(skip)), resConfUnit2, bilinear x 2 (align_corners), out_conv.
               out_conv is 1 x 1 and the interpolation weights sum to one, so out_conv(up(x)) = up(out_conv(x)) exactly: it runs on the
               LOW-resolution grid, a quarter of the work; the up-sampling kernel adds the next block's resConfUnit1(skip) in the same pass
  head         3 x 3 F -> F/2, bilinear x 2, 3 x 3 F/2 -> 32 + ReLU, then pmi_dpt_head_fwd: -relu(1 x 1 to one channel)

Activations are 16-bit NHWC (bf16 by default), the residual stream and its gradient fp32.  State-dict keys are the reference's:
``pretrained.model.*`` (timm), ``pretrained.act_postprocess{k}.*``, ``scratch.*``.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .. import _hip
from .._hip import ACT_GELU, ACT_NONE, ACT_RELU, call, ptr
from . import ops
from .ops import PackedLinear
from .vit import VitEngine, from_timm_vit_state_dict, timm_vit_state_dict_shapes

# name: (res, patch, width, layers, heads, hooks, reassemble channels, features)
DPT_CONFIGS = {"dpt_large": (384, 16, 1024, 24, 16, (5, 11, 17, 23), (256, 512, 1024, 1024), 256)}
HEAD_CHANNELS = 32          # dpt_depth.py:92
IGNORED_PREFIXES = ("pretrained.model.head.", "pretrained.model.norm.")     # timm's classifier and its final norm: computed by the reference, never used


def check_config(cfg) -> None:
    res, patch, width, layers, heads, hooks, channels, features = cfg
    if patch != 16 or res % 32:
        raise ValueError("DPT reassembles a 16 x 16 patch grid (vit.py:208, 285) and halves it once: patch must be 16 and res a multiple of 32")
    if len(hooks) != 4 or list(hooks) != sorted(set(hooks)) or hooks[0] < 0 or hooks[3] >= layers:
        raise ValueError(f"hooks must be four ascending block indices below {layers}, got {hooks}")
    if len(channels) != 4 or any(c % 8 for c in channels) or features % 16 or width % 8:
        raise ValueError("reassemble channels and the width must be multiples of 8, features a multiple of 16 (16-byte NHWC vectors)")


def dpt_state_dict_shapes(cfg) -> Dict[str, Tuple[int, ...]]:
    """Every key the engine reads, with its shape (IGNORED_PREFIXES are extra keys of the reference's checkpoint)."""
    res, patch, width, layers, heads, hooks, channels, features = cfg
    S = {"pretrained.model." + k: v for k, v in timm_vit_state_dict_shapes((res, patch, width, layers, heads, 0)).items()}
    for k, c in enumerate(channels, start=1):
        p = f"pretrained.act_postprocess{k}."
        S[p + "0.project.0.weight"] = (width, 2 * width); S[p + "0.project.0.bias"] = (width,)
        S[p + "3.weight"] = (c, width, 1, 1); S[p + "3.bias"] = (c,)
        if k in (1, 2):
            S[p + "4.weight"] = (c, c, 6 - 2 * k, 6 - 2 * k); S[p + "4.bias"] = (c,)
        elif k == 4:
            S[p + "4.weight"] = (c, c, 3, 3); S[p + "4.bias"] = (c,)
        S[f"scratch.layer{k}_rn.weight"] = (features, c, 3, 3)
        r = f"scratch.refinenet{k}."
        S[r + "out_conv.weight"] = (features, features, 1, 1); S[r + "out_conv.bias"] = (features,)
        for u in (1, 2):
            for cv in (1, 2):
                S[r + f"resConfUnit{u}.conv{cv}.weight"] = (features, features, 3, 3); S[r + f"resConfUnit{u}.conv{cv}.bias"] = (features,)
    S["scratch.output_conv.0.weight"] = (features // 2, features, 3, 3); S["scratch.output_conv.0.bias"] = (features // 2,)
    S["scratch.output_conv.2.weight"] = (HEAD_CHANNELS, features // 2, 3, 3); S["scratch.output_conv.2.bias"] = (HEAD_CHANNELS,)
    S["scratch.output_conv.4.weight"] = (1, HEAD_CHANNELS, 1, 1); S["scratch.output_conv.4.bias"] = (1,)
    return S


def reference_state_dict_shapes(cfg) -> Dict[str, Tuple[int, ...]]:
    """What the reference's ``DPTDepthModel.state_dict()`` holds: dpt_state_dict_shapes plus timm's final norm and classifier."""
    S = dpt_state_dict_shapes(cfg)
    width = cfg[2]
    S.update({"pretrained.model.norm.weight": (width,), "pretrained.model.norm.bias": (width,),
              "pretrained.model.head.weight": (1000, width), "pretrained.model.head.bias": (1000,)})
    return S


def check_state_dict(sd, cfg) -> Dict[str, torch.Tensor]:
    """-> the keys the engine reads.  Missing, unexpected or mis-shaped keys are ValueErrors; IGNORED_PREFIXES are accepted and dropped."""
    want = dpt_state_dict_shapes(cfg)
    have = {k: v for k, v in sd.items() if not k.startswith(IGNORED_PREFIXES)}
    missing, extra = sorted(set(want) - set(have)), sorted(set(have) - set(want))
    if missing or extra:
        raise ValueError(f"DPT state dict: missing keys {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                         f"unexpected keys {extra[:4]}{'...' if len(extra) > 4 else ''}")
    bad = [k for k in want if tuple(have[k].shape) != tuple(want[k])]
    if bad:
        raise ValueError(f"DPT state dict: {bad[0]} has shape {tuple(have[bad[0]].shape)}, expected {tuple(want[bad[0]])}")
    return have


class _Conv:
    """A convolution's forward packing and the packing of its input-gradient convolution (transposed, taps flipped)."""

    def __init__(self, w, b, dt, dev):
        self.fwd = PackedLinear(w, b, dt, dev)
        self.bwd = ops.packed_dx({}, "dx", w, dt, dev)


class DptEngine:
    def __init__(self, cfg, state_dict, device, dtype="bf16"):
        self.cfg, self.device = tuple(cfg), torch.device(device)
        check_config(self.cfg)
        res, patch, width, layers, heads, hooks, channels, features = self.cfg
        if dtype not in ("f16", "fp16", "bf16"):
            raise ValueError("the DPT engine runs in 'f16' or 'bf16'")
        sd = {k: v.detach().float().cpu() for k, v in check_state_dict(state_dict, self.cfg).items()}
        self.hooks = tuple(int(h) for h in hooks)
        self.vit = VitEngine((res, patch, width, layers, heads, 0), from_timm_vit_state_dict(sd, "pretrained.model."), device, dtype,
                             quick_gelu=False, ln_eps=1e-6, pre_ln=False, pooled_head=False, norm=((0.5,) * 3, (0.5,) * 3))     # midas_depth.py:57
        self.dt, self.gscale = self.vit.dt, self.vit.gscale
        dt, dev = self.dt, self.device
        tdt = _hip.TORCH_DTYPE[dt]
        self.taps = []
        for k, c in enumerate(channels, start=1):
            p = f"pretrained.act_postprocess{k}."
            wp, bp = sd[p + "0.project.0.weight"], sd[p + "0.project.0.bias"]
            wa, wb = wp[:, :width].contiguous(), wp[:, width:].contiguous()   # cat((tokens, readout), -1): the token half first (vit.py:40)
            T = dict(c=c,
                     ra=PackedLinear(wa, None, dt, dev), ra_t=PackedLinear(wa.t().contiguous(), None, dt, dev),
                     rb=PackedLinear(wb, bp, dt, dev),
                     rb_t=wb.to(tdt).float().t().contiguous().to(dev),         # fp32 [in, out] of the 16-bit weights the forward multiplied
                     proj=_Conv(sd[p + "3.weight"], sd[p + "3.bias"], dt, dev),
                     rn=_Conv(sd[f"scratch.layer{k}_rn.weight"], None, dt, dev))
            if k in (1, 2):
                kk = 6 - 2 * k
                w2 = sd[p + "4.weight"].permute(2, 3, 1, 0).reshape(kk * kk * c, c).contiguous()       # rows (ky, kx, co), columns ci
                T.update(k=kk, up=PackedLinear(w2, None, dt, dev), up_t=PackedLinear(w2.t().contiguous(), None, dt, dev),
                         up_b=sd[p + "4.bias"].to(dev).contiguous())
            elif k == 4:
                T.update(down=_Conv(sd[p + "4.weight"], sd[p + "4.bias"], dt, dev))
            self.taps.append(T)
        self.fusion = []
        for k in range(1, 5):
            r = f"scratch.refinenet{k}."
            unit = lambda u: (_Conv(sd[r + f"resConfUnit{u}.conv1.weight"], sd[r + f"resConfUnit{u}.conv1.bias"], dt, dev),
                              _Conv(sd[r + f"resConfUnit{u}.conv2.weight"], sd[r + f"resConfUnit{u}.conv2.bias"], dt, dev))
            # refinenet4 has one input: its resConfUnit1 is in the checkpoint and never runs (blocks.py:378)
            self.fusion.append(dict(u1=unit(1) if k < 4 else None, u2=unit(2),
                                    out=_Conv(sd[r + "out_conv.weight"], sd[r + "out_conv.bias"], dt, dev)))
        self.head0 = _Conv(sd["scratch.output_conv.0.weight"], sd["scratch.output_conv.0.bias"], dt, dev)
        self.head2 = _Conv(sd["scratch.output_conv.2.weight"], sd["scratch.output_conv.2.bias"], dt, dev)
        self.head4 = (sd["scratch.output_conv.4.weight"].reshape(HEAD_CHANNELS).to(dev).contiguous(),
                      sd["scratch.output_conv.4.bias"].reshape(1).to(dev).contiguous())
        self.saved = None

    # ---- kernels by name, each on its own so that tests can drive one ----------------------------------------------------------------
    def _like(self, shape):
        return torch.empty(shape, dtype=_hip.TORCH_DTYPE[self.dt], device=self.device)

    def up2(self, x, r=None):
        n, h, w, c = x.shape
        y = self._like((n, 2 * h, 2 * w, c))
        call("pmi_bilinear2_ac_fwd", ptr(x), ptr(r), ptr(y), n, h, w, c, self.dt)
        return y

    def up2_bwd(self, g):
        n, h2, w2, c = g.shape
        dx = self._like((n, h2 // 2, w2 // 2, c))
        call("pmi_bilinear2_ac_bwd", ptr(g), ptr(dx), n, h2 // 2, w2 // 2, c, self.dt)
        return dx

    def relu(self, x):
        y = torch.empty_like(x)
        call("pmi_act_fwd", ptr(x), ptr(y), x.numel(), ACT_RELU, self.dt)
        return y

    def relu_bwd(self, g, y, r=None):
        dz = torch.empty_like(g)
        call("pmi_dpt_relu_bwd", ptr(g), ptr(y), ptr(r), ptr(dz), g.numel(), self.dt)
        return dz

    # ---- blocks ------------------------------------------------------------------------------------------------------------------------
    def _unit(self, x, unit, tape):
        """ResidualConvUnit_custom: conv2(relu(conv1(relu(x)))) + x -- the skip adds the UN-activated input (nn.ReLU(False), dpt_depth.py:16)."""
        t = ops.igemm(self.relu(x), unit[0].fwd, act=ACT_RELU)
        if tape is not None:
            tape.append((x, t))
        return ops.igemm(t, unit[1].fwd, residual=x)

    def _unit_bwd(self, g, unit, saved):
        x, t = saved
        dz = self.relu_bwd(ops.igemm(g, unit[1].bwd), t)
        return self.relu_bwd(ops.igemm(dz, unit[0].bwd), x, g)                # + g: the skip

    def _readout(self, T, tap, n, p, width, tape):
        """tap fp32 [N, T, W] -> GELU(tok Wa^T + cls Wb^T + b), 16-bit [N P, W]"""
        tok, cls = self._like((n * p, width)), self._like((n, width))
        call("pmi_dpt_tap_split", ptr(tap), ptr(tok), ptr(cls), n, p + 1, width, self.dt)
        row_bias = ops.igemm(cls, T["rb"], out_f32=True)                      # [N, W] fp32: the class part, once per image
        pre = ops.igemm(tok, T["ra"], nbias=row_bias, hw=p)
        act = torch.empty_like(pre)
        call("pmi_act_fwd", ptr(pre), ptr(act), pre.numel(), ACT_GELU, self.dt)
        if tape is not None:
            tape["pre"].append(pre)
        return act

    def _readout_bwd(self, T, dact, pre, n, p, width):
        """dact 16-bit [N P, W] -> the tap's gradient fp32 [N, T, W]"""
        dpre = torch.empty_like(dact)
        call("pmi_act_bwd", ptr(dact), ptr(pre), ptr(dpre), dact.numel(), ACT_GELU, self.dt)
        d_tok = ops.igemm(dpre, T["ra_t"], out_f32=True)
        colsum = torch.empty((n, width), dtype=torch.float32, device=self.device)
        call("pmi_dpt_colsum", ptr(dpre), ptr(colsum), n, p, width, self.dt)
        d_cls = torch.empty((n, width), dtype=torch.float32, device=self.device)
        ops.gemm_f32(colsum, T["rb_t"], d_cls, M=n, N=width, K=width, lda=width, ldb=width, ldd=width)
        d_tap = torch.empty((n, p + 1, width), dtype=torch.float32, device=self.device)
        call("pmi_dpt_tap_join", ptr(d_tok), ptr(d_cls), ptr(d_tap), n, p + 1, width)
        return d_tap, dpre

    # ---- forward -------------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, images: torch.Tensor, save: bool = False, record: Optional[dict] = None) -> torch.Tensor:
        """images NCHW fp32 in [0, 1], any size (resized to res x res) -> -relu(depth), fp32 [N, 1, res, res] (midas_depth.py:128).
        record (tests): receives references to tensors this pass makes anyway: taps (fp32), maps (the four reassembled maps), rn, sums (the
        input of every block's resConfUnit2: path + resConfUnit1(skip)), path1, h (the head's post-ReLU 32-channel map)."""
        if not images.is_cuda:
            raise RuntimeError("DptEngine runs on a HIP device only (no CPU fallback)")
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"DptEngine expects NCHW images with 3 channels, got {tuple(images.shape)}")
        res, patch, width, layers, heads, hooks, channels, features = self.cfg
        n, g = images.shape[0], res // patch
        p = g * g
        _, taps = self.vit.forward(images.float(), save=save, taps=self.hooks)
        tape = dict(n=n, vit=self.vit.saved, pre=[], u1=[None] * 4, u2=[None] * 4) if save else None
        self.vit.saved = None
        maps, rn = [], []
        for k, (T, tap) in enumerate(zip(self.taps, taps)):
            act = self._readout(T, tap.contiguous(), n, p, width, tape)
            y = ops.igemm(act, T["proj"].fwd)                                  # [N P, C_k]
            c = T["c"]
            if k < 2:                                                          # ConvTranspose2d(c, c, kk, stride=kk): GEMM + depth-to-space
                kk = T["k"]
                cols = ops.igemm(y, T["up"]).view(n, g, g, kk * kk * c)
                m = self._like((n, kk * g, kk * g, c))
                call("pmi_depth_to_space", ptr(cols), ptr(T["up_b"]), ptr(m), n, g, g, c, kk, self.dt)
            elif k == 2:
                m = y.view(n, g, g, c)
            else:
                m = ops.igemm(y.view(n, g, g, c), T["down"].fwd, stride=2)
            maps.append(m)
            rn.append(ops.igemm(m, T["rn"].fwd))
        sums, x = [None] * 4, rn[3]
        for k in (3, 2, 1, 0):                                                 # refinenet4 .. refinenet1
            F = self.fusion[k]
            sums[k] = x
            l2 = [] if save else None
            r = self._unit(x, F["u2"], l2)
            q = ops.igemm(r, F["out"].fwd)                                     # out_conv on the low-resolution grid (module doc)
            addend = None
            if k > 0:
                l1 = [] if save else None
                addend = self._unit(rn[k - 1], self.fusion[k - 1]["u1"], l1)
                if save:
                    tape["u1"][k - 1] = l1[0]
            x = self.up2(q, addend)                                            # k > 0: path_{k+1} + resConfUnit1(layer_k_rn), the next block's sum
            if save:
                tape["u2"][k] = l2[0]
        path1 = x
        hd = self.up2(ops.igemm(path1, self.head0.fwd))
        h = ops.igemm(hd, self.head2.fwd, act=ACT_RELU)                        # [N, res, res, 32]
        out = torch.empty((n, 1, res, res), dtype=torch.float32, device=self.device)
        call("pmi_dpt_head_fwd", ptr(h), ptr(self.head4[0]), ptr(self.head4[1]), ptr(out), n * res * res, self.dt)
        if save:
            tape.update(h=h, out=out)
            self.saved = tape
        if record is not None:
            record.update(taps=taps, maps=maps, rn=rn, sums=sums, path1=path1, h=h)
        return out

    # ---- input gradient ------------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def backward(self, d_depth: torch.Tensor, record: Optional[dict] = None) -> torch.Tensor:
        """d_depth: dL/d(output) * self.gscale, fp32 [N, 1, res, res] -> dL/d(images), fp32 NCHW at the size forward() was given.
        f16: the gradient is scaled once more by a power of two from its largest value (ops.f16_grad_scale) and the image gradient back.
        record (tests): references to what this pass makes anyway: masks = the tensors whose sign the ReLU gradients read (out, h, and per
        unit (input, middle)), g_path1, g_sums, g_maps, d_taps (all times gscale and the f16 scale ``scale``), and the tower's own."""
        tape = self.saved
        if tape is None:
            raise RuntimeError("call forward(images, save=True) before backward()")
        res, patch, width, layers, heads, hooks, channels, features = self.cfg
        n, g = tape["n"], res // patch
        p = g * g
        if not d_depth.is_cuda:
            raise RuntimeError("DptEngine runs on a HIP device only (no CPU fallback)")
        if d_depth.dtype != torch.float32 or tuple(d_depth.shape) != (n, 1, res, res):
            raise ValueError(f"d_depth must be fp32 [{n}, 1, {res}, {res}]")
        d = d_depth.contiguous()
        scale = 1.0
        if self.dt == _hip.DT_F16:
            amax = torch.empty((n,), dtype=torch.float32, device=self.device)
            call("pmi_quantile_abs", ptr(d), ptr(amax), n, res * res, 1.0)
            scale = ops.f16_grad_scale(amax.tolist())
        h, out = tape["h"], tape["out"]
        dh = torch.empty_like(h)
        call("pmi_dpt_head_bwd", ptr(d), ptr(out), ptr(h), ptr(self.head4[0]), ptr(dh), n * res * res, scale, self.dt)
        gx = ops.igemm(self.up2_bwd(ops.igemm(dh, self.head2.bwd)), self.head0.bwd)          # gradient at path_1
        g_path1, g_sums, g_rn = gx, [None] * 4, [None] * 4
        for k in (0, 1, 2, 3):                                                 # refinenet1 .. refinenet4
            F = self.fusion[k]
            gq = self.up2_bwd(gx)
            gs = self._unit_bwd(ops.igemm(gq, F["out"].bwd), F["u2"], tape["u2"][k])
            g_sums[k] = gs                                                     # the sum's gradient goes to both summands as it is
            if k < 3:
                g_rn[k] = self._unit_bwd(gs, F["u1"], tape["u1"][k])
            else:
                g_rn[k] = gs
            gx = gs
        d_taps, g_maps = [], []
        for k, T in enumerate(self.taps):
            gm = ops.igemm(g_rn[k], T["rn"].bwd)
            g_maps.append(gm)
            c = T["c"]
            if k < 2:
                kk = T["k"]
                cols = self._like((n, g, g, kk * kk * c))
                call("pmi_space_to_depth", ptr(gm), ptr(cols), n, g, g, c, kk, self.dt)
                gy = ops.igemm(cols.view(n * p, kk * kk * c), T["up_t"])
            elif k == 2:
                gy = gm.view(n * p, c)
            else:                                                              # stride-2 conv: dX = stride-1 conv of the zero-inserted gradient with
                z = torch.zeros((n, g, g, c), dtype=gm.dtype, device=gm.device)     # the flipped weights (as engine/adm.py's down-sampler)
                z[:, ::2, ::2] = gm
                gy = ops.igemm(z, T["down"].bwd).view(n * p, c)
            dact = ops.igemm(gy, T["proj"].bwd)
            d_tap, _ = self._readout_bwd(T, dact, tape["pre"][k], n, p, width)
            d_taps.append(d_tap)
        if record is not None:
            record.update(scale=scale, masks=dict(out=out, h=h, u1=tape["u1"], u2=tape["u2"]), g_path1=g_path1, g_sums=g_sums, g_maps=g_maps,
                          d_taps=d_taps)
        self.vit.saved = tape["vit"]
        self.saved = None
        return self.vit.backward_taps(d_taps, record, scale=scale)             # the stem divides the image gradient by gscale * scale
