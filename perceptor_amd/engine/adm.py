"""HIP execution engine for the ADM UNet (ε-prediction) — replaces UNetModel.forward.

Mirrors perceptor/models/guided_diffusion/unet.py:626-654 (forward), :232-252
(ResBlock), :294-300 (AttentionBlock) and the constructor loops :471-601, but runs
NHWC 16-bit activations through libperceptor_hip.so:

  * every conv3x3 / conv1x1 / linear is one pmi_igemm launch (MFMA implicit GEMM) with
    bias, per-sample bias, residual add, nearest-up gather and skip-concat (two source
    pointers) fused, so th.cat / F.interpolate / "+ skip" never touch HBM on their own;
  * GroupNorm32+SiLU(+FiLM)(+AvgPool) is stats -> finalize -> apply, fp32 statistics;
  * all 49 emb_layers linears run as ONE GEMM per step (their weights are concatenated);
  * attention with 64-channel heads runs the fused flash kernel.

State-dict keys are the reference's, so a real checkpoint loads as is.
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
class AdmConfig:
    """Resolved hyper-parameters (script_util.py:130-184)."""
    image_size: int
    model_channels: int
    num_res_blocks: int
    channel_mult: Tuple[float, ...]
    attention_ds: Tuple[int, ...]
    num_heads: int = 1
    num_head_channels: int = -1
    num_heads_upsample: int = -1
    use_scale_shift_norm: bool = False
    resblock_updown: bool = False
    use_new_attention_order: bool = False
    in_channels: int = 3
    out_channels: int = 6
    conv_resample: bool = True


_DEFAULT_MULT = {512: (0.5, 1, 1, 2, 2, 4, 4), 256: (1, 1, 2, 2, 4, 4), 128: (1, 1, 2, 3, 4), 64: (1, 2, 3, 4)}


def openimages_config() -> AdmConfig:   # create_models.py:8-33
    return AdmConfig(512, 256, 2, _DEFAULT_MULT[512], (16, 32, 64), num_head_channels=64,
                     use_scale_shift_norm=True, resblock_updown=True)


def pixelart_config() -> AdmConfig:     # create_models.py:36-62
    return AdmConfig(256, 128, 2, _DEFAULT_MULT[256], (16,), num_heads=1)


class _Res:
    def __init__(self, prefix, cin, cout, up=False, down=False, srcs=None):
        self.p, self.cin, self.cout, self.up, self.down = prefix, cin, cout, up, down
        self.srcs = srcs          # channel counts of a concat input (h, skip), None for a single source
        self.emb_off = 0


class _Attn:
    def __init__(self, prefix, c, heads):
        self.p, self.c, self.heads = prefix, c, heads


class _Resample:
    def __init__(self, prefix, c, up):
        self.p, self.c, self.up = prefix, c, up


def build_plan(cfg: AdmConfig):
    """Layer descriptors in execution order + parameter shapes (names as in the reference)."""
    mc = cfg.model_channels

    def heads(c, upsample=False):
        if cfg.num_head_channels != -1:
            return c // cfg.num_head_channels
        if upsample and cfg.num_heads_upsample != -1:
            return cfg.num_heads_upsample
        return cfg.num_heads

    ch = int(cfg.channel_mult[0] * mc)
    inp: List[list] = [[("conv0", "input_blocks.0.0", cfg.in_channels, ch)]]
    skip_ch = [ch]
    ds = 1
    for level, mult in enumerate(cfg.channel_mult):
        for _ in range(cfg.num_res_blocks):
            i = len(inp)
            cout = int(mult * mc)
            layers = [_Res(f"input_blocks.{i}.0", ch, cout)]
            ch = cout
            if ds in cfg.attention_ds:
                layers.append(_Attn(f"input_blocks.{i}.1", ch, heads(ch)))
            inp.append(layers)
            skip_ch.append(ch)
        if level != len(cfg.channel_mult) - 1:
            i = len(inp)
            if cfg.resblock_updown:
                inp.append([_Res(f"input_blocks.{i}.0", ch, ch, down=True)])
            else:
                inp.append([_Resample(f"input_blocks.{i}.0", ch, up=False)])
            skip_ch.append(ch)
            ds *= 2
    mid = [_Res("middle_block.0", ch, ch), _Attn("middle_block.1", ch, heads(ch)), _Res("middle_block.2", ch, ch)]
    out: List[list] = []
    for level, mult in list(enumerate(cfg.channel_mult))[::-1]:
        for i in range(cfg.num_res_blocks + 1):
            j = len(out)
            ich = skip_ch.pop()
            cout = int(mc * mult)
            layers = [_Res(f"output_blocks.{j}.0", ch + ich, cout, srcs=(ch, ich))]
            ch = cout
            k = 1
            if ds in cfg.attention_ds:
                layers.append(_Attn(f"output_blocks.{j}.{k}", ch, heads(ch, True)))
                k += 1
            if level and i == cfg.num_res_blocks:
                if cfg.resblock_updown:
                    layers.append(_Res(f"output_blocks.{j}.{k}", ch, ch, up=True))
                else:
                    layers.append(_Resample(f"output_blocks.{j}.{k}", ch, up=True))
                ds //= 2
            out.append(layers)
    return inp, mid, out, ch


def state_dict_shapes(cfg: AdmConfig) -> Dict[str, Tuple[int, ...]]:
    mc, ted = cfg.model_channels, 4 * cfg.model_channels
    inp, mid, out, ch_last = build_plan(cfg)
    S: Dict[str, Tuple[int, ...]] = {
        "time_embed.0.weight": (ted, mc), "time_embed.0.bias": (ted,),
        "time_embed.2.weight": (ted, ted), "time_embed.2.bias": (ted,)}
    for layers in inp + [mid] + out:
        for l in layers:
            if isinstance(l, tuple):
                S[l[1] + ".weight"] = (l[3], l[2], 3, 3); S[l[1] + ".bias"] = (l[3],)
            elif isinstance(l, _Res):
                p = l.p
                S[p + ".in_layers.0.weight"] = (l.cin,); S[p + ".in_layers.0.bias"] = (l.cin,)
                S[p + ".in_layers.2.weight"] = (l.cout, l.cin, 3, 3); S[p + ".in_layers.2.bias"] = (l.cout,)
                e = 2 * l.cout if cfg.use_scale_shift_norm else l.cout
                S[p + ".emb_layers.1.weight"] = (e, ted); S[p + ".emb_layers.1.bias"] = (e,)
                S[p + ".out_layers.0.weight"] = (l.cout,); S[p + ".out_layers.0.bias"] = (l.cout,)
                S[p + ".out_layers.3.weight"] = (l.cout, l.cout, 3, 3); S[p + ".out_layers.3.bias"] = (l.cout,)
                if l.cin != l.cout:
                    S[p + ".skip_connection.weight"] = (l.cout, l.cin, 1, 1); S[p + ".skip_connection.bias"] = (l.cout,)
            elif isinstance(l, _Attn):
                p = l.p
                S[p + ".norm.weight"] = (l.c,); S[p + ".norm.bias"] = (l.c,)
                S[p + ".qkv.weight"] = (3 * l.c, l.c, 1); S[p + ".qkv.bias"] = (3 * l.c,)
                S[p + ".proj_out.weight"] = (l.c, l.c, 1); S[p + ".proj_out.bias"] = (l.c,)
            elif isinstance(l, _Resample) and cfg.conv_resample:
                n = l.p + (".conv" if l.up else ".op")
                S[n + ".weight"] = (l.c, l.c, 3, 3); S[n + ".bias"] = (l.c,)
    S["out.0.weight"] = (ch_last,); S["out.0.bias"] = (ch_last,)
    S["out.2.weight"] = (cfg.out_channels, int(cfg.channel_mult[0] * mc), 3, 3); S["out.2.bias"] = (cfg.out_channels,)
    return S


class AdmEngine:
    def __init__(self, cfg: AdmConfig, state_dict: Dict[str, torch.Tensor], device, dtype="bf16"):
        self.cfg, self.device = cfg, torch.device(device)
        self.dt = _hip.dtype_code(dtype)
        _hip.lib()
        sd, dev, dt = state_dict, self.device, self.dt
        self.inp, self.mid, self.out, self.ch_last = build_plan(cfg)
        f32 = lambda k: sd[k].detach().float().to(dev).contiguous()
        lin = lambda k, **kw: PackedLinear(sd[k + ".weight"], sd.get(k + ".bias"), dt, dev, **kw)
        self.w: Dict[str, object] = {}
        self.precise = dt == _hip.DT_F16X2
        if self.precise:      # fp32 time MLPs (exact-fp32 MFMA GEMM): their weights stay fp32 in the reference too (unet.py:610-616)
            self.te0, self.te2 = (f32("time_embed.0.weight"), f32("time_embed.0.bias")), (f32("time_embed.2.weight"), f32("time_embed.2.bias"))
        else:
            self.te0, self.te2 = lin("time_embed.0"), lin("time_embed.2")
        emb_w, emb_b, off = [], [], 0
        for layers in self.inp + [self.mid] + self.out:
            for l in layers:
                if isinstance(l, tuple):
                    self.w[l[1]] = lin(l[1], cin_pad=8)
                elif isinstance(l, _Res):
                    p = l.p
                    self.w[p + ".gn1"] = (f32(p + ".in_layers.0.weight"), f32(p + ".in_layers.0.bias"))
                    self.w[p + ".conv1"] = lin(p + ".in_layers.2", sources=l.srcs, up_phase=l.up)       # (an up block's conv1 reads nearest-x2(x): phase weights)
                    self.w[p + ".gn2"] = (f32(p + ".out_layers.0.weight"), f32(p + ".out_layers.0.bias"))
                    self.w[p + ".conv2"] = lin(p + ".out_layers.3")
                    if l.cin != l.cout:
                        self.w[p + ".skip"] = lin(p + ".skip_connection", sources=l.srcs)
                        if self._skip_fusable(l):
                            self.w[p + ".skip.b"] = ops.fused_skip_bias(self.w[p + ".conv2"], self.w[p + ".skip"])
                    l.emb_off = off
                    emb_w.append(sd[p + ".emb_layers.1.weight"].float()); emb_b.append(sd[p + ".emb_layers.1.bias"].float())
                    off += emb_w[-1].shape[0]
                elif isinstance(l, _Attn):
                    p = l.p
                    self.w[p + ".gn"] = (f32(p + ".norm.weight"), f32(p + ".norm.bias"))
                    self.w[p + ".qkv"] = lin(p + ".qkv")
                    self.w[p + ".proj"] = lin(p + ".proj_out")
                elif isinstance(l, _Resample) and cfg.conv_resample:
                    self.w[l.p] = lin(l.p + (".conv" if l.up else ".op"), up_phase=l.up)
        if self.precise:
            self.emb_all = (torch.cat(emb_w, 0).to(dev).contiguous(), torch.cat(emb_b, 0).to(dev).contiguous())
        else:
            self.emb_all = PackedLinear(torch.cat(emb_w, 0), torch.cat(emb_b, 0), dt, dev)
        self.gn_out = (f32("out.0.weight"), f32("out.0.bias"))
        self.conv_out = lin("out.2")

    # ---- blocks ----------------------------------------------------------------------------------
    def _skip_fusable(self, l: _Res) -> bool:
        """Structure of a ResBlock whose two-source skip convolution can ride in its conv2 launch (ops.igemm(skip=...)): 16-bit modes, a
        concatenated input, no resampling, channel counts the 128-channel tiles divide.  The map size joins in _conv2 (SKIP_FUSE_MIN_HW)."""
        return not self.precise and l.srcs is not None and l.cin != l.cout and not l.up and not l.down \
            and l.cout % 128 == 0 and all(c % 64 == 0 for c in l.srcs)

    def _conv2(self, l: _Res, h, x, x1, prologue):
        """out_layers' convolution + the skip path (unet.py:232-252): one fused launch where the block and the map allow, else the skip
        GEMM and conv2 with its output as the residual.  The choice depends on the layer, the dtype and the map size only, never on the batch
        (pmi_conv3x3_skip_eligible counts no workgroups; f16 layers with cout % 256 != 0 keep the two launches)."""
        w = self.w
        if l.cin != l.cout:
            sb = w.get(l.p + ".skip.b")
            if sb is not None and h.shape[1] * h.shape[2] >= ops.SKIP_FUSE_MIN_HW and h.shape[1] % 8 == 0 and h.shape[2] % 32 == 0:
                return ops.igemm(h, w[l.p + ".conv2"], prologue=prologue, want_stats=True, skip=(w[l.p + ".skip"], x, x1, sb))
            x = ops.igemm(x, w[l.p + ".skip"], a1=x1)
        elif x1 is not None:
            raise NotImplementedError("identity skip over a concatenated input does not occur in the shipped configs")
        return ops.igemm(h, w[l.p + ".conv2"], residual=x, res_up=l.up, prologue=prologue, want_stats=True)

    def _res(self, l: _Res, x, x1, emb, tape=None):
        """ResBlock (unet.py:232-252).  Inference and training mode issue the same launches: with a tape, the block's record for _res_back
        (its inputs, both norms' coefficients and partials, conv1's output) is appended to it."""
        cfg, dt, w = self.cfg, self.dt, self.w
        g1, b1 = w[l.p + ".gn1"]
        ecols = 2 * l.cout if cfg.use_scale_shift_norm else l.cout
        e = emb[:, l.emb_off:l.emb_off + ecols]
        film = e if cfg.use_scale_shift_norm else None
        nb = None if cfg.use_scale_shift_norm else e
        skip, skip1 = x, x1
        if l.down:
            # SiLU(GN(x)) must be pooled AFTER the activation: streaming apply+pool kernel, then the conv
            if x1 is None:      # both pooled tensors from one pass over x
                h, skip, gn1 = ops.group_norm_pool_skip_train(x, g1, b1, 32, dt, act=ACT_SILU)
            elif tape is not None:
                raise NotImplementedError("down-sampling ResBlock over a concatenated input does not occur in the shipped configs: it has no backward")
            else:
                h = ops.group_norm(x, g1, b1, 32, dt, x1=x1, act=ACT_SILU, pool=True)
                skip = ops.avgpool2(x, dt)
            h = ops.igemm(h, w[l.p + ".conv1"], nbias=nb, want_stats=True)
        else:
            # GroupNorm-apply + SiLU fused into the conv's patch staging (no activated copy in HBM)
            gn1 = ops.group_norm_coeffs_train(x, g1, b1, 32, dt, x1=x1)
            h = ops.igemm(x, w[l.p + ".conv1"], a1=x1, up=l.up, nbias=nb, prologue=(gn1[0], gn1[1], ACT_SILU), want_stats=True)
        g2, b2 = w[l.p + ".gn2"]
        gn2 = ops.group_norm_coeffs_train(h, g2, b2, 32, dt, film=film, film_ld=emb.stride(0) if film is not None else 0)
        out = self._conv2(l, h, skip, skip1, (gn2[0], gn2[1], ACT_SILU))
        if tape is not None:
            tape.append(("res", l, x, x1, gn1, h, gn2, film))
        return out

    def _attn(self, l: _Attn, x):
        dt, w = self.dt, self.w
        n, hh, ww, c = x.shape
        g, b = w[l.p + ".gn"]
        hn = ops.group_norm(x, g, b, 32, dt)
        qkv = ops.igemm(hn.view(n * hh * ww, c), w[l.p + ".qkv"])
        a = ops.attention(qkv.view(n, hh * ww, 3 * c), l.heads, 1 if self.cfg.use_new_attention_order else 0, dt)
        out = ops.igemm(a.view(n * hh * ww, c), w[l.p + ".proj"], residual=x.view(n * hh * ww, c), want_stats=True, hw=hh * ww)
        return ops.view_nhwc(out, n, hh, ww)

    def _embed_input(self, images, timesteps):
        """Time embedding (all emb_layers outputs at once) and the padded NHWC input x = 2 * images - 1: (emb, x)."""
        cfg, dt, dev = self.cfg, self.dt, self.device
        if not images.is_cuda:
            raise RuntimeError(f"{type(self).__name__} runs on a HIP device only (no CPU fallback)")
        images = images.float().contiguous()
        n, _, hh, ww = images.shape
        t = timesteps.to(device=dev, dtype=torch.float32).contiguous()
        tdt = _hip.TORCH_DTYPE[dt]
        temb = torch.empty((n, cfg.model_channels), dtype=torch.float32 if self.precise else tdt, device=dev)
        call("pmi_timestep_embedding", ptr(t), ptr(temb), n, cfg.model_channels, 10000.0, dt)
        if self.precise:
            e = ops.linear_f32(temb, *self.te0, act=ACT_SILU)
            e = ops.linear_f32(e, *self.te2, act=ACT_SILU)
            emb = ops.linear_f32(e, *self.emb_all)
        else:
            e = ops.igemm(temb, self.te0, act=ACT_SILU)
            e = ops.igemm(e, self.te2, act=ACT_SILU)            # = SiLU(emb): the only form the ResBlocks consume
            emb = ops.igemm(e, self.emb_all, out_f32=True)       # [N, sum of all emb_layers outputs]
        x = torch.empty((n, hh, ww, 16 if self.precise else 8), dtype=tdt, device=dev)
        call("pmi_prep_input", ptr(images), None, 0, ptr(x), n, hh, ww, 8, dt)
        return emb, x

    def _output(self, h, ca, cb, out_channels):
        """conv_out on SiLU(GroupNorm(h)) given the norm's coefficients -> NCHW fp32 model output."""
        n, hh, ww, _ = h.shape
        y = ops.igemm(h, self.conv_out, out_f32=True, prologue=(ca, cb, ACT_SILU))
        co = out_channels or self.cfg.out_channels
        out = torch.empty((n, co, hh, ww), dtype=torch.float32, device=self.device)
        call("pmi_finish_output", ptr(y), y.shape[-1], ptr(out), n, hh, ww, co)
        return out

    def _run(self, layers, h, h1, emb, tape=None, sd=None):
        """One layer list of the plan on h (and the skip tensor h1 its first block concatenates).  With a tape (training mode; sd: the state
        dict, for the attention's repacked qkv) every layer appends its record for _back."""
        for l in layers:
            if isinstance(l, tuple):
                if tape is not None:
                    tape.append(("conv", l, h))
                h = ops.igemm(h, self.w[l[1]], want_stats=True)
            elif isinstance(l, _Res):
                h = self._res(l, h, h1, emb, tape)
            elif isinstance(l, _Attn):
                h = self._attn(l, h) if tape is None else self._attn_train(l, h, tape, sd)
            elif isinstance(l, _Resample):                # unet.py:81-138: nearest x2 + conv / stride-2 conv
                if not self.cfg.conv_resample:
                    raise NotImplementedError("conv_resample=False is not used by the shipped configs")
                h = ops.igemm(h, self.w[l.p], up=l.up, stride=1 if l.up else 2, want_stats=True)
                if tape is not None:
                    tape.append(("resample", l))
            h1 = None
        return h

    def _unet(self, emb, h, tape=None, sd=None):
        """The U over inp / mid / out -> the input of the output norm.  tape: {"inp": [], "mid": [], "out": []}, filled with one list of
        records per layer list (mid: the records themselves)."""
        def sub(key):
            if tape is None:
                return None
            tape[key].append([])
            return tape[key][-1]
        hs = []
        for layers in self.inp:
            h = self._run(layers, h, None, emb, sub("inp"), sd)
            hs.append(h)
        h = self._run(self.mid, h, None, emb, None if tape is None else tape["mid"], sd)
        for layers in self.out:
            h = self._run(layers, h, hs.pop(), emb, sub("out"), sd)
        return h

    @torch.no_grad()
    def forward(self, images: torch.Tensor, timesteps: torch.Tensor, out_channels: Optional[int] = None) -> torch.Tensor:
        """images: NCHW fp32 in [0,1] (encoded to x = 2*img-1 on the fly); returns NCHW fp32 model output."""
        emb, h = self._embed_input(images, timesteps)
        h = self._unet(emb, h)
        ca, cb = ops.group_norm_coeffs(h, *self.gn_out, 32, self.dt)
        return self._output(h, ca, cb, out_channels)

    # ---- input gradient -----------------------------------------------------------------------------------
    # Upstream GuidedDiffusion.predicted_noise is differentiable (guided_diffusion.py:125-133) and runs its blocks through CheckpointFunction
    # (nn.py:138-189, unet.py:228-229, 292): activations are dropped and recomputed in the backward to fit 16-40 GB cards.  Here the
    # training-mode forward keeps them instead -- every tensor it keeps is one the inference forward writes to HBM anyway (block inputs,
    # conv1 outputs, attention operands), 14.2 GB for GD "standard" at 512x512 x 8 of 288 GB -- and backward() walks the tape
    # once: no recomputation.  dX of a convolution is the forward kernel on transposed + flipped weights (ops.packed_dx); GroupNorm32 (+FiLM)
    # + SiLU backward is pmi_gn_bwd_*; attention backward is ops.self_attention_backward.
    # precise mode walks the same tape over hi + lo tensors: the convolutions' dX on split-operand packings of the transposed weights, the
    # memory-bound adjoints in their pmi_split_* forms, attention backward in exact fp32 (ops.attention_precise_backward).

    def _qkv_order1(self, l: _Attn, sd):
        """qkv projection producing channels (q|k|v, head, d) -- the layout of pmi_vit_attn_fwd / ops.attention_train -- whatever the
        checkpoint's order (unet.py:332-348 legacy: (head, q|k|v, d))."""
        key = l.p + ".qkv_o1"
        if key not in self.w:
            wq, bq = sd[l.p + ".qkv.weight"].detach().float(), sd[l.p + ".qkv.bias"].detach().float()
            if not self.cfg.use_new_attention_order:
                d = l.c // l.heads
                idx = torch.arange(3 * l.c).view(l.heads, 3, d).permute(1, 0, 2).reshape(-1)
                wq, bq = wq[idx], bq[idx]
            self.w[key] = PackedLinear(wq, bq, self.dt, self.device)
            self.w[key + ".w"] = wq
        return self.w[key], self.w[key + ".w"]

    def _attn_train(self, l: _Attn, x, tape, sd):
        dt, w = self.dt, self.w
        n, hh, ww, c = x.shape
        t = hh * ww
        g, b = w[l.p + ".gn"]
        ca, cb, parts = ops.group_norm_coeffs_train(x, g, b, 32, dt)
        hn = torch.empty_like(x)
        cl = ops.logical_c(x, dt)
        call("pmi_gn_apply", ptr(x), None, cl, ptr(ca), ptr(cb), None, ptr(hn), n, hh, ww, cl, ACT_NONE, 0, dt)
        lin, _ = self._qkv_order1(l, sd)
        a, saved = ops.self_attention_train(ops.igemm(hn.view(n * t, c), lin), n, t, l.heads, dt)
        out = ops.igemm(a, w[l.p + ".proj"], residual=x.view(n * t, c), want_stats=True, hw=t)
        tape.append(("attn", l, x, (ca, cb, parts), saved))
        return ops.view_nhwc(out, n, hh, ww)

    @torch.no_grad()
    def forward_train(self, images: torch.Tensor, timesteps: torch.Tensor, state_dict, out_channels: Optional[int] = None):
        """As forward(), keeping what backward() needs.  Returns (model output NCHW fp32, tape)."""
        emb, h = self._embed_input(images, timesteps)
        tape = {"inp": [], "mid": [], "out": [], "emb_ld": emb.stride(0)}
        h = self._unet(emb, h, tape, state_dict)
        gn = ops.group_norm_coeffs_train(h, *self.gn_out, 32, self.dt)
        tape["last"] = (h, gn)
        return self._output(h, gn[0], gn[1], out_channels), tape

    def _resample_bwd(self, l: _Res, g):
        """Gradient through the block's resampling of a path (nearest x2 up / 2x2 average down)."""
        if l.up:
            return ops.upsample_nearest2_bwd(g, self.dt)
        return ops.avgpool2_bwd(g, self.dt) if l.down else g

    def _res_back(self, rec, g, sd, ld):
        _, l, x, x1, gn1, h, gn2, film = rec
        dt, w, dev = self.dt, self.w, self.device
        p = l.p
        d_a2 = ops.igemm(g, ops.packed_dx(w, p + ".conv2T", sd[p + ".out_layers.3.weight"], dt, dev))                # wrt SiLU(GN2(h))
        dh, _ = ops.group_norm_backward(h, d_a2, gn2[0], gn2[1], gn2[2], w[p + ".gn2"][0], 32, dt, film=film, film_ld=ld if film is not None else 0,
                                        act=ACT_SILU)
        d_a1 = self._resample_bwd(l, ops.igemm(dh, ops.packed_dx(w, p + ".conv1T", sd[p + ".in_layers.2.weight"], dt, dev)))   # wrt SiLU(GN1(cat(x, x1)))
        if l.cin != l.cout:
            skw = sd[p + ".skip_connection.weight"]
            if x1 is None:
                gs0, gs1 = ops.igemm(g, ops.packed_dx(w, p + ".skipT", skw, dt, dev)), None
            else:
                c0 = ops.logical_c(x, dt)
                gs0 = ops.igemm(g, ops.packed_dx(w, p + ".skipT0", skw[:, :c0], dt, dev))
                gs1 = ops.igemm(g, ops.packed_dx(w, p + ".skipT1", skw[:, c0:], dt, dev))
        else:
            gs0, gs1 = self._resample_bwd(l, g), None
        return ops.group_norm_backward(x, d_a1, gn1[0], gn1[1], gn1[2], w[p + ".gn1"][0], 32, dt, x1=x1, act=ACT_SILU, gadd0=gs0, gadd1=gs1)

    def _attn_back(self, rec, g, sd):
        _, l, x, gn, saved = rec
        dt, w, dev = self.dt, self.w, self.device
        n, hh, ww, c = x.shape
        t = hh * ww
        da = ops.igemm(g.reshape(n * t, c), ops.packed_dx(w, l.p + ".projT", sd[l.p + ".proj_out.weight"], dt, dev))
        dqkv = ops.self_attention_backward(saved, da, n, t, l.heads, dt)
        _, wq = self._qkv_order1(l, sd)
        dhn = ops.igemm(dqkv, ops.packed_dx(w, l.p + ".qkvT", wq, dt, dev)).view(n, hh, ww, c)
        gx, _ = ops.group_norm_backward(x, dhn, gn[0], gn[1], gn[2], w[l.p + ".gn"][0], 32, dt, act=ACT_NONE, gadd0=g.contiguous())
        return gx

    def _back(self, tp, g, sd, ld):
        """Gradient wrt the input(s) of the layer list recorded in `tp` given g = gradient wrt its output: (g_in, g_skip or None)."""
        g1 = None
        for rec in reversed(tp):
            assert g1 is None
            if rec[0] == "res":
                g, g1 = self._res_back(rec, g, sd, ld)
            elif rec[0] == "attn":
                g = self._attn_back(rec, g, sd)
            elif rec[0] == "resample":
                l = rec[1]
                wt = ops.packed_dx(self.w, l.p + "T", sd[l.p + (".conv" if l.up else ".op") + ".weight"], self.dt, self.device)
                if l.up:                             # conv over nearest-up(x): dX at the high resolution, then the sum of each 2x2 block
                    g = ops.upsample_nearest2_bwd(ops.igemm(g, wt), self.dt)
                else:                                # stride-2 conv: dX = stride-1 conv of the zero-inserted gradient with the flipped weights
                    n, h_, w_, c = g.shape           # (two torch ops for the layout step: only the conv_resample configs -- pixelart -- come here)
                    z = torch.zeros((n, 2 * h_, 2 * w_, c), dtype=g.dtype, device=g.device)
                    z[:, ::2, ::2] = g
                    g = ops.igemm(z, wt)
            else:                                    # the first convolution: fp32 gradient wrt the padded input
                g = ops.igemm(g, ops.packed_dx(self.w, rec[1][1] + "T", sd[rec[1][1] + ".weight"], self.dt, self.device), out_f32=True)
        return g, g1

    @torch.no_grad()
    def backward(self, tape, d_out: torch.Tensor, state_dict) -> torch.Tensor:
        """d loss / d images (NCHW fp32, images in [0, 1]) from d loss / d output (NCHW fp32, the first d_out.shape[1] output channels) and the
        tape of forward_train().  f16 and precise engines scale the gradient by a power of two on the way in and back on the way out
        (ops.grad_to_nhwc); bf16 needs no scaling."""
        dt = self.dt
        sd = {k: v.detach() for k, v in state_dict.items()}
        g, scale = ops.grad_to_nhwc(d_out, dt, self.device)                                     # output channels + padding
        ld = tape["emb_ld"]
        h, gn = tape["last"]
        d_act = ops.igemm(g, ops.packed_dx(self.w, "out.2T", sd["out.2.weight"], self.dt, self.device, cin_pad=8))
        g, _ = ops.group_norm_backward(h, d_act, gn[0], gn[1], gn[2], self.gn_out[0], 32, dt, act=ACT_SILU)
        g_hs = []                                                                               # gradients of the skip tensors, in pop order
        for tp in reversed(tape["out"]):
            g, gk = self._back(tp, g, sd, ld)
            g_hs.append(gk)
        g, _ = self._back(tape["mid"], g, sd, ld)
        # the out blocks popped hs from the end: the LAST out list read hs[0]; walking them reversed gives g_hs = [for hs[0], hs[1], ...]
        for i in range(len(tape["inp"]) - 1, -1, -1):
            gk = g_hs[i]
            tot = ops.add2(g, gk, dt)                                                      # hs[i] feeds the next block AND an out block
            g, _ = self._back(tape["inp"][i], tot, sd, ld)
        return ops.grad_to_nchw(g, 3, 2.0 / scale)                                              # x = 2 * images - 1
