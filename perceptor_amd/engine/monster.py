"""HIP engine for MonsterDiffusion's k-diffusion UNet under Karras et al.'s EDM parameterisation.

Replaces base.Model.forward (perceptor/models/monster_diffusion/base/model.py:143-229, layers in base/layers.py) together with
MonsterDiffusion.denoised_ (monster_diffusion.py:103-125): images + sigma -> denoised_xs.

Kernel mapping: AdaGN (layers.py:92-107: F.group_norm without affine, then x * (1 + weight) + bias from a per-layer Linear on the mapping
network's output) is pmi_gn_stats + pmi_gn_finalize(gamma = NULL, film = ...) + pmi_gn_apply with exact GELU, G = C / 32 groups; the mappers
of ALL layers are one fp32 GEMM whose output row holds every layer's (weight | bias), each layer reading at its column offset.  The 3x3 and
1x1 convolutions are pmi_igemm launches with the residual add in their epilogue; a UBlock's torch.cat([input, skip]) is never materialised
(pmi_gn_stats and the 1x1 skip convolution take two source pointers).  SelfAttention2d (layers.py:113-132) = AdaGN -> 1x1 qkv -> fused
head-dim-64 attention in the (q, k, v)-then-heads channel order (one narrower head through the flash kernel where a block's last layer has
fewer than 64 channels) -> 1x1 out + residual.  Downsample2d / Upsample2d are the FIR kernels of
csrc/fir.hip.  c_in * x, c_noise and c_skip * x + c_out * F are the pmi_edm_stage_* kernels; the conditioning (Fourier features, mapping
network, AdaGN mappers) stays fp32.  Nothing inside an evaluation synchronises with the host.

Input gradient (what autograd gives the reference for a loss on the predictions): forward_train() is forward() with a tape, backward() walks
it in reverse through the transposed convolutions, pmi_gn_bwd_*, the attention backward, the FIR adjoints pmi_fir_*_bwd and the EDM staging
adjoints pmi_edm_stage_*_bwd.  Weights, sigma and the augmentations are not differentiated.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from .. import _hip
from .._hip import ACT_GELU, ACT_NONE, call, ptr
from . import ops
from .ops import PackedLinear

SIGMA_DATA = 0.5                     # diffusion.py
GROUP_SIZE, HEAD_SIZE = 32, 64       # base/model.py: ResConvBlock / DBlock defaults


def product_config():
    """base.Model(mapping_cond_dim=9): (feats_in, depths, channels, self_attn_depths, mapping_cond_dim)."""
    return (256, [2, 4, 4], [128, 256, 512], [False, True, True], 9)


def check_config(config) -> None:
    feats, depths, channels, attn, mcd = config
    if not (len(depths) == len(channels) == len(attn)) or len(depths) < 1:
        raise ValueError("monster config: depths, channels and self_attn_depths must have one entry per level")
    if feats <= 0 or feats % 2 or mcd < 0 or any(d < 1 for d in depths):
        raise ValueError("monster config: feats_in must be even and positive, depths at least 1")
    for i, c in enumerate(channels):
        if c <= 0 or c % GROUP_SIZE or (attn[i] and c % HEAD_SIZE):
            raise ValueError(f"monster config: level {i} has {c} channels (multiples of 32, of 64 on an attention level)")
    for prog in sum(_blocks(config), []):
        for l in prog:
            if isinstance(l, Attn) and l.c % max(1, l.c // HEAD_SIZE):
                raise ValueError(f"monster config: an attention over {l.c} channels does not split into heads of 64")
    for i in range(len(channels) - 1):       # a UBlock whose two-source first block would keep its width has an identity skip over a concat
        cout = channels[i] if depths[i] > 1 else channels[max(i - 1, 0)]
        if 2 * channels[i] == cout:
            raise ValueError(f"monster config: level {i} would need an identity skip over a concatenated input")


def check_size(config, h: int, w: int) -> None:
    """H and W divisible by 2^(levels - 1), the deepest map at least 2 x 2 (the reflect padding needs two samples per axis)."""
    f = 2 ** (len(config[1]) - 1)
    if h % f or w % f or h // f < 2 or w // f < 2:
        raise ValueError(f"images of {h}x{w}: height and width must be multiples of {f} and at least {2 * f}")


class Res:
    def __init__(self, key, cin, cmid, cout, srcs=None):
        self.key, self.cin, self.cmid, self.cout, self.srcs = key, cin, cmid, cout, srcs
        self.mod1 = self.mod2 = 0


class Attn:
    def __init__(self, key, c):
        self.key, self.c, self.mod = key, c, 0


class Down:
    def __init__(self, key):
        self.key = key


class Up:
    def __init__(self, key):
        self.key = key


def _blocks(config) -> Tuple[List[list], List[list]]:
    """(d_blocks, u_blocks) as lists of layers, u_blocks in running order (deepest first), keys as nn.Sequential numbers them."""
    feats, depths, channels, attn, _ = config
    L = len(depths)

    def block(prefix, n_layers, c_in, c_mid, c_out, self_attn, down=False, up=False, two=False):
        prog, j = [], 0
        if down:
            prog.append(Down(f"{prefix}.{j}")); j += 1
        for i in range(n_layers):
            a = c_in if i == 0 else c_mid
            b = c_mid if i < n_layers - 1 else c_out
            prog.append(Res(f"{prefix}.{j}", a, c_mid, b, srcs=(a // 2, a // 2) if (two and i == 0) else None)); j += 1
            if self_attn:
                prog.append(Attn(f"{prefix}.{j}", b)); j += 1
        if up:
            prog.append(Up(f"{prefix}.{j}"))
        return prog

    d = [block(f"u_net.d_blocks.{i}", depths[i], channels[i] if i == 0 else channels[i - 1], channels[i], channels[i], attn[i], down=i > 0)
         for i in range(L)]
    u = []
    for pos, i in enumerate(reversed(range(L))):
        c_in = channels[i] * 2 if i < L - 1 else channels[i]
        u.append(block(f"u_net.u_blocks.{pos}", depths[i], c_in, channels[i], channels[i] if i == 0 else channels[i - 1], attn[i], up=i > 0,
                       two=i < L - 1))
    return d, u


def monster_state_dict_shapes(config) -> Dict[str, Tuple[int, ...]]:
    """Names and shapes of base.Model(...).state_dict() in its own order (buffers included: the Fourier weight and the resamplers' kernels)."""
    check_config(config)
    feats, depths, channels, attn, mcd = config
    S: Dict[str, Tuple[int, ...]] = {"timestep_embed.weight": (feats // 2, 1)}
    if mcd > 0:
        S["mapping_cond.weight"] = (feats, mcd)
    for i in (0, 2):
        S[f"mapping.{i}.weight"] = (feats, feats); S[f"mapping.{i}.bias"] = (feats,)
    S["proj_in.weight"] = (channels[0], 3, 1, 1); S["proj_in.bias"] = (channels[0],)
    S["proj_out.weight"] = (3, channels[0], 1, 1); S["proj_out.bias"] = (3,)
    d, u = _blocks(config)
    for prog in d + u:
        for l in prog:
            p = l.key
            if isinstance(l, (Down, Up)):
                S[p + ".kernel"] = (4, 4)
            elif isinstance(l, Res):
                S[p + ".main.0.mapper.weight"] = (2 * l.cin, feats); S[p + ".main.0.mapper.bias"] = (2 * l.cin,)
                S[p + ".main.2.weight"] = (l.cmid, l.cin, 3, 3); S[p + ".main.2.bias"] = (l.cmid,)
                S[p + ".main.4.mapper.weight"] = (2 * l.cmid, feats); S[p + ".main.4.mapper.bias"] = (2 * l.cmid,)
                S[p + ".main.6.weight"] = (l.cout, l.cmid, 3, 3); S[p + ".main.6.bias"] = (l.cout,)
                if l.cin != l.cout:
                    S[p + ".skip.weight"] = (l.cout, l.cin, 1, 1)
            else:
                S[p + ".norm_in.mapper.weight"] = (2 * l.c, feats); S[p + ".norm_in.mapper.bias"] = (2 * l.c,)
                S[p + ".qkv_proj.weight"] = (3 * l.c, l.c, 1, 1); S[p + ".qkv_proj.bias"] = (3 * l.c,)
                S[p + ".out_proj.weight"] = (l.c, l.c, 1, 1); S[p + ".out_proj.bias"] = (l.c,)
    return S


def fir_kernel_buffers() -> Tuple[torch.Tensor, torch.Tensor]:
    """The `kernel` buffers of Downsample2d("linear") and Upsample2d("linear") (layers.py:208-232): k k^T and (2k)(2k)^T, k = [1, 3, 3, 1] / 8."""
    k = torch.tensor([[1 / 8, 3 / 8, 3 / 8, 1 / 8]])
    return k.T @ k, (2 * k).T @ (2 * k)


def synthetic_state_dict(config, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Name-keyed synthetic weights (utils.synth) for every entry -- proj_out too, which the reference zero-initialises: a zero output would pin
    nothing -- with the resamplers' `kernel` buffers at their true values."""
    from ..utils.synth import synth_state_dict
    shapes = monster_state_dict_shapes(config)
    sd = synth_state_dict(shapes, seed)
    kd, ku = fir_kernel_buffers()
    for k in shapes:
        if k.endswith(".kernel"):
            sd[k] = (kd if ".d_blocks." in k else ku).clone()
    return sd


def bare_state_dict(state_dict) -> Dict[str, torch.Tensor]:
    """The network's keys without the wrapper's `network.` prefix (the published checkpoints are MonsterDiffusion.state_dict())."""
    if state_dict and all(k.startswith("network.") for k in state_dict):
        return {k[len("network."):]: v for k, v in state_dict.items()}
    return dict(state_dict)


def check_state_dict(config, sd) -> None:
    shapes = monster_state_dict_shapes(config)
    missing, extra = sorted(set(shapes) - set(sd)), sorted(set(sd) - set(shapes))
    if missing or extra:
        raise ValueError(f"monster state dict: missing keys {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                         f"unexpected keys {extra[:4]}{'...' if len(extra) > 4 else ''}")
    for k, s in shapes.items():
        if tuple(sd[k].shape) != tuple(s):
            raise ValueError(f"monster state dict: {k} has shape {tuple(sd[k].shape)}, expected {tuple(s)}")
    kd, ku = fir_kernel_buffers()
    for k in shapes:
        if k.endswith(".kernel"):
            want = kd if ".d_blocks." in k else ku
            if not torch.equal(sd[k].detach().float().cpu(), want):
                raise ValueError(f"monster state dict: {k} is not the linear resampling kernel [1, 3, 3, 1] (the only one the HIP kernels implement)")


class MonsterEngine:
    def __init__(self, config, state_dict, device, dtype="bf16"):
        check_config(config)
        self.config, self.device = config, torch.device(device)
        self.dt = _hip.dtype_code(dtype)
        if self.dt not in (_hip.DT_F16, _hip.DT_BF16):
            raise ValueError("MonsterEngine: dtype must be 'bf16' or 'f16'")
        _hip.lib()
        sd = bare_state_dict(state_dict)
        check_state_dict(config, sd)
        dev, dt = self.device, self.dt
        self.feats, self.mcd = config[0], config[4]
        f32 = lambda k: sd[k].detach().float().to(dev).contiguous()
        self.tw = f32("timestep_embed.weight").reshape(-1)
        self.map_cond = f32("mapping_cond.weight") if self.mcd > 0 else None
        self.map = [(f32(f"mapping.{i}.weight"), f32(f"mapping.{i}.bias")) for i in (0, 2)]
        self.d_blocks, self.u_blocks = _blocks(config)
        self.w: Dict[str, PackedLinear] = {"proj_in": PackedLinear(sd["proj_in.weight"], sd["proj_in.bias"], dt, dev, cin_pad=8),
                                           "proj_out": PackedLinear(sd["proj_out.weight"], sd["proj_out.bias"], dt, dev)}
        mw, mb, off = [], [], 0

        def mapper(key, c):
            nonlocal off
            mw.append(sd[key + ".mapper.weight"].detach().float()); mb.append(sd[key + ".mapper.bias"].detach().float())
            at, off = off, off + 2 * c
            return at

        for prog in self.d_blocks + self.u_blocks:
            for l in prog:
                p = l.key
                if isinstance(l, Res):
                    l.mod1 = mapper(p + ".main.0", l.cin)
                    l.mod2 = mapper(p + ".main.4", l.cmid)
                    self.w[p + ".c1"] = PackedLinear(sd[p + ".main.2.weight"], sd[p + ".main.2.bias"], dt, dev)
                    self.w[p + ".c2"] = PackedLinear(sd[p + ".main.6.weight"], sd[p + ".main.6.bias"], dt, dev)
                    if l.cin != l.cout:
                        self.w[p + ".skip"] = PackedLinear(sd[p + ".skip.weight"], None, dt, dev, sources=l.srcs)
                elif isinstance(l, Attn):
                    l.mod = mapper(p + ".norm_in", l.c)
                    self.w[p + ".qkv"] = PackedLinear(sd[p + ".qkv_proj.weight"], sd[p + ".qkv_proj.bias"], dt, dev)
                    self.w[p + ".out"] = PackedLinear(sd[p + ".out_proj.weight"], sd[p + ".out_proj.bias"], dt, dev)
        # every AdaGN mapper of the network as ONE linear layer [sum 2C, feats]
        self.mod_w, self.mod_b = torch.cat(mw, 0).to(dev).contiguous(), torch.cat(mb, 0).to(dev).contiguous()

    # ---- conditioning ------------------------------------------------------------------------------------------------------------
    def cond(self, c_noise: torch.Tensor, augmentations: Optional[torch.Tensor] = None) -> torch.Tensor:
        """mapping(timestep_embed(c_noise) + mapping_cond(augmentations)) (model.py:213-219), fp32 [rows, feats]; rows = c_noise's count, or
        the batch when augmentations are given.  augmentations = None stands for the zeros the samplers pass: a bias-free Linear of zeros."""
        ff = torch.empty((c_noise.numel(), self.feats), dtype=torch.float32, device=self.device)
        call("pmi_fourier_features", ptr(c_noise), ptr(self.tw), ptr(ff), c_noise.numel(), self.feats // 2)
        if augmentations is not None:
            if self.map_cond is None:
                raise ValueError("this network takes no mapping_cond")
            aug = augmentations.to(device=self.device, dtype=torch.float32).contiguous()
            if ff.shape[0] != aug.shape[0]:
                ff = ff.expand(aug.shape[0], -1).contiguous()                       # (layout only: one row of features for every sample)
            ff = ops.linear_f32(aug, self.map_cond, None, residual=ff)
        h = ops.linear_f32(ff, *self.map[0], act=ACT_GELU)
        return ops.linear_f32(h, *self.map[1], act=ACT_GELU)

    # ---- blocks ------------------------------------------------------------------------------------------------------------------
    def _adagn(self, x, x1, c, off, mod, act, keep=None):
        # mod has one row when sigma is one value for the batch: film_ld = 0 then reads that row for every sample
        groups, film, ld = max(1, c // GROUP_SIZE), mod[:, off:], (mod.stride(0) if mod.shape[0] > 1 else 0)
        if keep is None:
            return ops.group_norm(x, None, None, groups, self.dt, x1=x1, film=film, film_ld=ld, act=act)
        # training mode: the launches of ops.group_norm, with the (ca, cb, parts) of the coefficients kept for group_norm_backward
        gn = ops.group_norm_coeffs_train(x, None, None, groups, self.dt, x1=x1, film=film, film_ld=ld)
        n, hh, ww, c0 = x.shape
        y = torch.empty((n, hh, ww, c), dtype=x.dtype, device=x.device)
        call("pmi_gn_apply", ptr(x), ptr(x1), c0, ptr(gn[0]), ptr(gn[1]), None, ptr(y), n, hh, ww, c, act, 0, self.dt)
        keep.append(gn)
        return y

    def _res(self, l: Res, x, x1, mod, tape=None):
        w, p = self.w, l.key
        gns = None if tape is None else []
        skip = ops.igemm(x, w[p + ".skip"], a1=x1) if l.cin != l.cout else x
        h = self._adagn(x, x1, l.cin, l.mod1, mod, ACT_GELU, gns)
        h1 = ops.igemm(h, w[p + ".c1"])
        h = self._adagn(h1, None, l.cmid, l.mod2, mod, ACT_GELU, gns)
        if tape is not None:         # no GELU output is kept: pmi_gn_bwd_* recompute act'(a x + b) from the norm's input
            tape.append(("res", l, x, x1, h1, gns[0], gns[1]))
        return ops.igemm(h, w[p + ".c2"], residual=skip)

    def _attn(self, l: Attn, x, mod, tape=None):
        w, p = self.w, l.key
        n, hh, ww, c = x.shape
        gns = None if tape is None else []
        hn = self._adagn(x, None, c, l.mod, mod, ACT_NONE, gns)
        qkv = ops.igemm(hn.view(n * hh * ww, c), w[p + ".qkv"])
        # heads = max(1, C // 64) as DBlock / UBlock build it: 64-wide heads, or ONE narrower head where a block's last layer leaves the level
        # with fewer than 64 channels; order 1: (q, k, v) first, heads inside
        heads = max(1, c // HEAD_SIZE)
        a = ops.attention(qkv.view(n, hh * ww, 3 * c), heads, 1, self.dt)
        if tape is not None:
            # the output above stays the inference kernels' (forward_train returns forward's bits); what the backward kernels need -- the
            # log-sum-exp and head-major copies at d = 64, the kept probabilities otherwise -- comes from the training-form kernels
            tape.append(("attn", l, x, gns[0], ops.self_attention_train(qkv, n, hh * ww, heads, self.dt)[1]))
        return ops.igemm(a.view(n * hh * ww, c), w[p + ".out"], residual=x.view(n * hh * ww, c)).view(n, hh, ww, c)

    def _run(self, prog, x, x1, mod, tape=None):
        """The block `prog` on x (and the stored skip x1).  With a tape every layer appends the record _back needs."""
        for l in prog:
            if isinstance(l, Res):
                x, x1 = self._res(l, x, x1, mod, tape), None
            elif isinstance(l, Attn):
                x = self._attn(l, x, mod, tape)
            elif isinstance(l, Down):
                x = ops.fir_down2(x, self.dt)
                if tape is not None:
                    tape.append(("down",))
            else:
                x = ops.fir_up2(x, self.dt)
                if tape is not None:
                    tape.append(("up",))
        assert x1 is None
        return x

    def network(self, x: torch.Tensor, cond: torch.Tensor, taps: Optional[dict] = None, tape: Optional[dict] = None) -> torch.Tensor:
        """base.Model.forward after its mapping network: x NHWC 16-bit [N, H, W, 8] (3 channels + zeros), cond fp32 [N or 1, feats] ->
        the fp32 NHWC output [N, H, W, 4] (3 channels + padding).  taps: filled with every block's output (tests).  tape: filled with
        `mod` and one record list per d- and u-block (training mode)."""
        mod = ops.linear_f32(cond, self.mod_w, self.mod_b)                          # every AdaGN's (weight | bias) at once
        tap = (lambda k, v: taps.__setitem__(k, v)) if taps is not None else (lambda k, v: None)

        def recs(name):
            if tape is None:
                return None
            return tape.setdefault(name, [])

        if tape is not None:
            tape["mod"] = mod
        h = ops.igemm(x, self.w["proj_in"])
        tap("proj_in", h)
        skips = []
        for i, prog in enumerate(self.d_blocks):
            h = self._run(prog, h, None, mod, recs(f"d{i}"))
            skips.append(h)
            tap(f"d{i}", h)
        for i, prog in enumerate(self.u_blocks):
            h = self._run(prog, h, skips[len(skips) - 1 - i] if i > 0 else None, mod, recs(f"u{i}"))
            tap(f"u{i}", h)
        y = ops.igemm(h, self.w["proj_out"], out_f32=True)
        tap("proj_out", y)
        return y

    def _evaluate(self, images, sigma, augmentations, taps, tape):
        if not images.is_cuda:
            raise RuntimeError("MonsterEngine runs on a HIP device only (no CPU fallback)")
        if images.ndim != 4 or images.shape[1] != 3:
            raise ValueError("images must be [N, 3, H, W]")
        dev, dt = self.device, self.dt
        images = images.float().contiguous()
        n, _, hh, ww = images.shape
        check_size(self.config, hh, ww)
        sigma = sigma.to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if sigma.numel() not in (1, n):
            raise ValueError(f"sigma has {sigma.numel()} values for a batch of {n}")
        x = torch.empty((n, hh, ww, 8), dtype=_hip.TORCH_DTYPE[dt], device=dev)
        c_noise = torch.empty((sigma.numel(),), dtype=torch.float32, device=dev)
        call("pmi_edm_stage_in", ptr(images), ptr(sigma), sigma.numel(), SIGMA_DATA, ptr(x), ptr(c_noise), n, hh, ww, 8, dt)
        cond = self.cond(c_noise, augmentations)
        if taps is not None:
            taps["x_in"], taps["c_noise"], taps["cond"] = x, c_noise, cond
        if tape is not None:
            tape["sigma"] = sigma
        y = self.network(x, cond, taps, tape)
        out = torch.empty_like(images)
        call("pmi_edm_stage_out", ptr(images), ptr(y), y.shape[-1], ptr(sigma), sigma.numel(), SIGMA_DATA, ptr(out), n, hh, ww)
        return out

    @torch.no_grad()
    def forward(self, images: torch.Tensor, sigma: torch.Tensor, augmentations: Optional[torch.Tensor] = None, taps: Optional[dict] = None) -> torch.Tensor:
        """images NCHW fp32 in [0, 1]; sigma: fp32 device tensor with one value or one per sample -> denoised_xs NCHW fp32 (denoised_)."""
        return self._evaluate(images, sigma, augmentations, taps, None)

    # ---- input gradient ----------------------------------------------------------------------------------------------------------
    # What autograd gives the reference when a loss on predictions.denoised_images back-propagates to diffused_images: d loss / d images
    # through c_skip x + c_out F(c_in x), weights frozen.  forward_train() is forward() with a tape; backward() walks it in reverse.  dX of
    # a convolution is the forward kernel on flipped, transposed weights (ops.packed_dx, built lazily, once, into self.w); AdaGN + GELU goes
    # back through pmi_gn_bwd_* (gamma = NULL, the FiLM row, erf-GELU's derivative recomputed from the norm's input); the resamplers through
    # their exact transposes pmi_fir_*_bwd.  Out of scope: the gradient to sigma / ts, the gradient to the augmentations, weight gradients,
    # and the precise and mixed types (MonsterEngine has neither).

    @torch.no_grad()
    def forward_train(self, images: torch.Tensor, sigma: torch.Tensor, augmentations: Optional[torch.Tensor] = None):
        """As forward() -- the same kernels and output bits -- keeping what backward() needs.  Returns (denoised_xs NCHW fp32, tape).
        The tape holds sigma, `mod` (every AdaGN row) and per layer: a Res its input(s) x, x1, conv1's output and both norms'
        (ca, cb, parts); an Attn its input, the norm's coefficients and self_attention_train's `saved`.  Not differentiated: sigma / ts, the
        augmentations, the weights; there is no precise or mixed type."""
        tape: dict = {}
        return self._evaluate(images, sigma, augmentations, None, tape), tape

    def _film(self, mod, off):
        return dict(film=mod[:, off:], film_ld=mod.stride(0) if mod.shape[0] > 1 else 0)

    def _res_back(self, rec, g, sd, mod):
        _, l, x, x1, h1, gn1, gn2 = rec
        w, p, dt, dev = self.w, l.key, self.dt, self.device
        d3 = ops.igemm(g, ops.packed_dx(w, p + ".c2T", sd[p + ".main.6.weight"], dt, dev))
        d1 = ops.group_norm_backward(h1, d3, *gn2, None, max(1, l.cmid // GROUP_SIZE), dt, act=ACT_GELU, **self._film(mod, l.mod2))[0]
        d2 = ops.igemm(d1, ops.packed_dx(w, p + ".c1T", sd[p + ".main.2.weight"], dt, dev))
        if l.cin == l.cout:                                                       # identity skip (never over a concat: check_config)
            gs = (g, None)
        elif x1 is None:
            gs = (ops.igemm(g, ops.packed_dx(w, p + ".skipT", sd[p + ".skip.weight"], dt, dev)), None)
        else:                                                                     # bias-free 1x1 over cat([x, x1]): one dX per source
            skw, c0 = sd[p + ".skip.weight"], x.shape[-1]
            gs = (ops.igemm(g, ops.packed_dx(w, p + ".skipT0", skw[:, :c0], dt, dev)),
                  ops.igemm(g, ops.packed_dx(w, p + ".skipT1", skw[:, c0:], dt, dev)))
        return ops.group_norm_backward(x, d2, *gn1, None, max(1, l.cin // GROUP_SIZE), dt, x1=x1, act=ACT_GELU, gadd0=gs[0], gadd1=gs[1],
                                       **self._film(mod, l.mod1))

    def _attn_back(self, rec, g, sd, mod):
        _, l, x, gn, saved = rec
        w, p, dt, dev = self.w, l.key, self.dt, self.device
        n, hh, ww, c = x.shape
        t, heads = hh * ww, max(1, c // HEAD_SIZE)
        g2 = g.reshape(n * t, c)
        da = ops.igemm(g2, ops.packed_dx(w, p + ".outT", sd[p + ".out_proj.weight"], dt, dev))
        dqkv = ops.self_attention_backward(saved, da, n, t, heads, dt)
        dhn = ops.igemm(dqkv, ops.packed_dx(w, p + ".qkvT", sd[p + ".qkv_proj.weight"], dt, dev))
        return ops.group_norm_backward(x, dhn.view(n, hh, ww, c), *gn, None, max(1, c // GROUP_SIZE), dt, act=ACT_NONE, gadd0=g,
                                       **self._film(mod, l.mod))[0]

    def _back(self, recs, g, sd, mod):
        """(gradient wrt the block's input, gradient wrt its stored skip or None) from g = gradient wrt its output."""
        g1 = None
        for rec in reversed(recs):
            assert g1 is None
            if rec[0] == "res":
                g, g1 = self._res_back(rec, g, sd, mod)
            elif rec[0] == "attn":
                g = self._attn_back(rec, g, sd, mod)
            elif rec[0] == "down":
                g = ops.fir_down2_bwd(g, self.dt)
            else:
                g = ops.fir_up2_bwd(g, self.dt)
        return g, g1

    @torch.no_grad()
    def backward(self, tape, d_denoised: torch.Tensor, state_dict, taps: Optional[dict] = None) -> torch.Tensor:
        """d loss / d images (NCHW fp32, images in [0, 1]) from d loss / d denoised_xs (NCHW fp32 [N, 3, H, W]) and forward_train()'s tape:
        pmi_edm_stage_out_bwd -> proj_out^T -> the u-blocks in reverse -> the d-blocks in reverse -> proj_in^T -> pmi_edm_stage_in_bwd.
        `state_dict`: the network's parameters (reference key names); the transposed packings are built from it on first use.
        f16 scales the gradient by a power of two from the per-sample maxima of c_out * d_denoised (ops.f16_grad_scale: one host read)
        and divides it out at the end; bf16 is unscaled and never synchronises with the host.
        taps: receives `gx` (the fp32 NHWC network-input gradient, scale divided out) and, as d<i> / u<i>, the gradient arriving at every
        block's input (fp32 NHWC, scale divided out; a two-source u-block's is the concat of both sources' gradients).
        Not computed: the gradient to sigma / ts, to the augmentations and to the weights; no precise or mixed type."""
        dev, dt = self.device, self.dt
        sigma, mod = tape["sigma"], tape["mod"]
        d = d_denoised.to(device=dev, dtype=torch.float32).contiguous()
        n = d.shape[0]
        scale = 1.0
        if dt == _hip.DT_F16:
            amax = torch.empty((n,), dtype=torch.float32, device=dev)
            call("pmi_quantile_abs", ptr(d), ptr(amax), n, d[0].numel(), 1.0)
            s64 = sigma.double().expand(n) if sigma.numel() == 1 else sigma.double()
            c_out = s64 * SIGMA_DATA / torch.sqrt(SIGMA_DATA ** 2 + s64 ** 2)
            scale = ops.f16_grad_scale((amax.double() * c_out).tolist())
        sd = bare_state_dict(state_dict)
        w = self.w
        tap = (lambda k, *v: taps.__setitem__(k, torch.cat([t.float() for t in v if t is not None], dim=-1) / scale)) if taps is not None \
            else (lambda k, *v: None)
        g = ops.edm_stage_out_bwd(d, sigma, SIGMA_DATA, scale, dt)
        g = ops.igemm(g, ops.packed_dx(w, "proj_outT", sd["proj_out.weight"], dt, dev, cin_pad=8))
        L, pending = len(self.d_blocks), {}
        for i in reversed(range(L)):
            g, g1 = self._back(tape[f"u{i}"], g, sd, mod)
            tap(f"u{i}", g, g1)
            if g1 is not None:
                pending[L - 1 - i] = g1                                           # the gradient of the stored skip: d-block L-1-i's output
        for i in reversed(range(L)):
            if i in pending:
                g = ops.add2(g, pending.pop(i), dt)
            g, g1 = self._back(tape[f"d{i}"], g, sd, mod)
            assert g1 is None
            tap(f"d{i}", g)
        gx = ops.igemm(g, ops.packed_dx(w, "proj_inT", sd["proj_in.weight"], dt, dev), out_f32=True)
        if taps is not None:
            taps["gx"] = gx[..., :3] / scale
        return ops.edm_stage_in_bwd(d, gx, sigma, SIGMA_DATA, 1.0 / scale)
