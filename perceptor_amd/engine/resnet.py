"""HIP engine for the CLIP ResNet image towers (RN50, RN101, RN50x4, RN50x16, RN50x64): forward and gradient w.r.t. the input image.

Replaces open_clip's ``model.encode_image`` + autograd on the guidance path (perceptor/models/open_clip.py:109-123) for the
``ModifiedResNet`` towers of the reference's model lists (models/open_clip.py:24-44, models/clip.py:6-27).  In eval mode:
  stem      three 3x3 pad-1 convolutions without bias (3 -> w/2 at stride 2, w/2 -> w/2, w/2 -> w), each + BatchNorm + ReLU, then AvgPool2d(2)
  layer1-4  Bottleneck blocks: 1x1 conv-BN-ReLU, 3x3 conv-BN-ReLU, AvgPool2d(stride), 1x1 conv-BN to 4 planes, + skip, ReLU;
            skip = AvgPool2d(stride) -> 1x1 conv -> BN where stride > 1 or the channel count changes, else the identity;
            the first block of layer2-4 has stride 2
  attnpool  tokens = [mean of the HW pixels | the pixels] + positional_embedding; multi-head attention with the mean token as the only
            query (head dim 64, separate q / k / v projections), then c_proj: the embedding

BatchNorm (eps 1e-5, running statistics) follows every convolution, so it is folded on the host into the convolution's weight and bias
(exact: the zero padding is applied before the convolution).  The CLIP mean / std cannot be folded into the stem convolution -- its zero
padding lives in the normalised space -- so pmi_rn_stage_input applies them while staging the 8-channel NHWC input.

Only the input gradient is needed (frozen weights): dX of a convolution is the forward convolution on transposed, flipped weights; the
stride-2 stem convolution's dX is a stride-1 convolution of the zero-inserted gradient (engine/adm.py does the same); the post-ReLU
outputs double as the ReLU masks of pmi_act_bwd.  Activations and gradients are 16-bit NHWC (bf16 by default; f16 scales the gradient by
a power of two: gscale = 65536 on the caller's side, as engine/vit.py does, times one chosen in backward() from the largest |d_emb| -- the
gradient shrinks by three to four orders of magnitude on its way to the stem and a fixed scale leaves it among f16's subnormals).

State-dict keys follow open_clip's ``visual.*``: conv{1,2,3}.weight, bn{1,2,3}.*, layer{1..4}.{i}.conv{1,2,3}.weight / .bn{1,2,3}.* /
.downsample.0.weight / .downsample.1.*, attnpool.positional_embedding, attnpool.{q,k,v,c}_proj.{weight,bias}.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .. import _hip
from .._hip import ACT_NONE, ACT_RELU, call, ptr
from ..transforms.resize import resize as _resize, resize_backward as _resize_backward
from . import ops
from .ops import PackedLinear
from .vit import CLIP_MEAN, CLIP_STD

RN_CONFIGS = {
    # name: (image, layers, width, heads, out_dim)   heads = width * 32 / 64 (attention-pool width 32 * width, head dim 64)
    "RN50": (224, (3, 4, 6, 3), 64, 32, 1024),
    "RN101": (224, (3, 4, 23, 3), 64, 32, 512),
    "RN50x4": (288, (4, 6, 10, 6), 80, 40, 640),
    "RN50x16": (384, (6, 8, 18, 8), 96, 48, 768),
    "RN50x64": (448, (3, 15, 36, 10), 128, 64, 1024),
}
BN_EPS = 1e-5
# f16 backward: where the largest |d_emb| is put (ops.f16_grad_scale's (0.5, 1] times this).  What the fixed gscale = 65536 gives at a loss
# gradient of ~1e-2: a factor 64 below f16's largest value, and the stem's gradients (~1e-4 of d_emb's) stay normal numbers.
F16_DEMB_TOP = 1024.0


def blocks(cfg):
    """(prefix, inplanes, planes, stride, has_downsample) of every Bottleneck, in forward order."""
    res, layers, width, heads, out = cfg
    inplanes, out_ = width, []
    for li, nb in enumerate(layers):
        planes = width * 2 ** li
        for b in range(nb):
            stride = 2 if (li > 0 and b == 0) else 1
            out_.append((f"layer{li + 1}.{b}.", inplanes, planes, stride, stride > 1 or inplanes != 4 * planes))
            inplanes = 4 * planes
    return out_


def rn_state_dict_shapes(cfg) -> Dict[str, Tuple[int, ...]]:
    res, layers, width, heads, out = cfg
    S: Dict[str, Tuple[int, ...]] = {}

    def conv_bn(conv, bn, cout, cin, k):
        S[conv + ".weight"] = (cout, cin, k, k)
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            S[f"{bn}.{leaf}"] = (cout,)

    h = width // 2
    conv_bn("conv1", "bn1", h, 3, 3)
    conv_bn("conv2", "bn2", h, h, 3)
    conv_bn("conv3", "bn3", width, h, 3)
    for p, inplanes, planes, stride, ds in blocks(cfg):
        conv_bn(p + "conv1", p + "bn1", planes, inplanes, 1)
        conv_bn(p + "conv2", p + "bn2", planes, planes, 3)
        conv_bn(p + "conv3", p + "bn3", 4 * planes, planes, 1)
        if ds:
            conv_bn(p + "downsample.0", p + "downsample.1", 4 * planes, inplanes, 1)
    c = width * 32
    S["attnpool.positional_embedding"] = ((res // 32) ** 2 + 1, c)
    for n in "qkv":
        S[f"attnpool.{n}_proj.weight"] = (c, c)
        S[f"attnpool.{n}_proj.bias"] = (c,)
    S["attnpool.c_proj.weight"] = (out, c)
    S["attnpool.c_proj.bias"] = (out,)
    return S


_BN_LEAVES = ("weight", "bias", "running_mean", "running_var")


def fold_bn(weight: torch.Tensor, bn):
    """conv (no bias) followed by eval-mode BatchNorm -> (weight, bias) of one convolution, in the weight's float type.
    bn: {"weight", "bias", "running_mean", "running_var"} -> [Cout] tensors."""
    w = weight.detach()
    g, b, mu, var = (bn[k].to(w.dtype) for k in _BN_LEAVES)
    s = g / torch.sqrt(var + BN_EPS)
    return w * s.view(-1, 1, 1, 1), b - mu * s


class _Conv:
    """A BatchNorm-folded convolution: forward weights + bias, and the transposed (3x3: flipped) weights of its input gradient."""

    def __init__(self, sd, conv, bn, dt, dev):
        w, b = fold_bn(sd[conv + ".weight"].detach().cpu().double(), {k: sd[f"{bn}.{k}"].detach().cpu().double() for k in _BN_LEAVES})
        self.fwd = PackedLinear(w, b, dt, dev)
        wt = w.permute(1, 0, 2, 3)
        if wt.shape[-1] == 3:
            wt = wt.flip(2, 3)
        self.bwd = PackedLinear(wt.contiguous(), None, dt, dev)


class ResNetEngine:
    def __init__(self, cfg, state_dict, device, dtype="bf16"):
        self.cfg, self.device = cfg, torch.device(device)
        self.dt = _hip.dtype_code(dtype)
        if self.dt not in (_hip.DT_BF16, _hip.DT_F16):
            raise ValueError("the ResNet tower runs in 'bf16' or 'f16'")
        # fp16 cannot hold ~1e-6 gradients: scale the loss gradient up and the image gradient back down
        self.gscale = 1.0 if self.dt == _hip.DT_BF16 else 65536.0
        res, layers, width, heads, out = cfg
        if width * 32 != heads * 64 or width % 16 or out % 8 or res % 32:
            raise ValueError(f"unsupported ResNet config {cfg}: heads = width / 2 (head dim 64), width % 16 == 0, out_dim % 8 == 0 and "
                             "image % 32 == 0 are required (every 2x2 pool and its adjoint need even maps)")
        _hip.lib()
        sd, dev, dt = state_dict, self.device, self.dt
        self.stem = [_Conv(sd, f"conv{i}", f"bn{i}", dt, dev) for i in (1, 2, 3)]
        self.blocks = []
        for p, inplanes, planes, stride, ds in blocks(cfg):
            self.blocks.append(dict(stride=stride, c1=_Conv(sd, p + "conv1", p + "bn1", dt, dev), c2=_Conv(sd, p + "conv2", p + "bn2", dt, dev),
                                    c3=_Conv(sd, p + "conv3", p + "bn3", dt, dev),
                                    ds=_Conv(sd, p + "downsample.0", p + "downsample.1", dt, dev) if ds else None))
        a = "attnpool."
        f = lambda k: sd[a + k].detach().float().cpu()
        self.pos = f("positional_embedding").to(dev).contiguous()
        self.q = PackedLinear(f("q_proj.weight"), f("q_proj.bias"), dt, dev)
        self.kv = PackedLinear(torch.cat([f("k_proj.weight"), f("v_proj.weight")]), torch.cat([f("k_proj.bias"), f("v_proj.bias")]), dt, dev)
        self.cp = PackedLinear(f("c_proj.weight"), f("c_proj.bias"), dt, dev)
        self.q_t = PackedLinear(f("q_proj.weight").t().contiguous(), None, dt, dev)
        self.kv_t = PackedLinear(torch.cat([f("k_proj.weight"), f("v_proj.weight")]).t().contiguous(), None, dt, dev)
        self.cp_t = PackedLinear(f("c_proj.weight").t().contiguous(), None, dt, dev)
        self.mean = torch.tensor(CLIP_MEAN, device=dev)
        self.std = torch.tensor(CLIP_STD, device=dev)
        self.output_dim = out
        self.saved = None

    def _relu(self, x):
        y = torch.empty_like(x)
        call("pmi_act_fwd", ptr(x), ptr(y), x.numel(), ACT_RELU, self.dt)
        return y

    def _relu_bwd(self, g, y):
        """g * (y > 0): the ReLU mask from its saved output."""
        out = torch.empty_like(g)
        call("pmi_act_bwd", ptr(g), ptr(y), ptr(out), g.numel(), ACT_RELU, self.dt)
        return out

    # ---- forward --------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, images: torch.Tensor, save: bool = False, record: Optional[dict] = None):
        """images NCHW fp32 in [0,1] (any size) -> un-normalised embeddings [N, out_dim] fp32.
        record (tests): a dict that receives references to tensors this pass makes anyway and `saved` does not keep (no launch, no copy):
        resized (the image at the tower's resolution), x0 (the staged stem input), pooled (the stem's output), x_in (every block's input, in
        forward order), tok, o."""
        if not images.is_cuda:
            raise RuntimeError("ResNetEngine runs on a HIP device only (no CPU fallback)")
        res, layers, width, heads, out = self.cfg
        dt, dev = self.dt, self.device
        tdt = _hip.TORCH_DTYPE[dt]
        n = images.shape[0]
        resized = _resize(images, (res, res)).contiguous()
        x0 = torch.empty((n, res, res, 8), dtype=tdt, device=dev)
        call("pmi_rn_stage_input", ptr(resized), ptr(self.mean), ptr(self.std), ptr(x0), n, res, res, dt)
        s1 = ops.igemm(x0, self.stem[0].fwd, stride=2, act=ACT_RELU)
        s2 = ops.igemm(s1, self.stem[1].fwd, act=ACT_RELU)
        s3 = ops.igemm(s2, self.stem[2].fwd, act=ACT_RELU)
        x = ops.avgpool2(s3, dt)
        if record is not None:
            record.update(resized=resized, x0=x0, pooled=x, x_in=[])
        tape = []
        for blk in self.blocks:
            if record is not None:
                record["x_in"].append(x)
            h1 = ops.igemm(x, blk["c1"].fwd, act=ACT_RELU)
            h2 = ops.igemm(h1, blk["c2"].fwd, act=ACT_RELU)
            h2p = ops.avgpool2(h2, dt) if blk["stride"] > 1 else h2
            if blk["ds"] is not None:
                skip = ops.igemm(ops.avgpool2(x, dt) if blk["stride"] > 1 else x, blk["ds"].fwd)
            else:
                skip = x
            y = self._relu(ops.igemm(h2p, blk["c3"].fwd, residual=skip))      # ReLU after the add: conv3's residual epilogue, then the ReLU pass
            if save:
                tape.append((h1, h2, y))
            x = y
        # ---- attention pool
        _, hh, ww, c = x.shape
        hw = hh * ww
        t = hw + 1
        tok = torch.empty((n * t, c), dtype=tdt, device=dev)
        call("pmi_rn_tokens", ptr(x), ptr(self.pos), ptr(tok), n, hw, c, dt)
        kv = ops.igemm(tok, self.kv)                                             # [n*t, 2c]: K | V
        q = ops.igemm(tok.view(n, t, c)[:, 0], self.q)                           # the mean token's row of every image
        o = torch.empty((n, c), dtype=tdt, device=dev)
        P = torch.empty((n * heads, t), dtype=torch.float32, device=dev)
        call("pmi_rn_attn_fwd", ptr(q), ptr(kv), ptr(o), ptr(P), n, t, c, heads, 64.0 ** -0.5, dt)
        emb = ops.igemm(o, self.cp, out_f32=True)
        if record is not None:
            record.update(tok=tok, o=o)
        if save:
            self.saved = dict(in_hw=tuple(images.shape[2:]), n=n, stem=(s1, s2, s3), tape=tape, feat_hw=(hh, ww), q=q, kv=kv, P=P)
        return emb[:, :out] if emb.shape[1] != out else emb

    # ---- input gradient -----------------------------------------------------------------------------------
    @torch.no_grad()
    def backward(self, d_emb: torch.Tensor, record: Optional[dict] = None) -> torch.Tensor:
        """d_emb: dL/d(embedding) * self.gscale, fp32 [N, out_dim]  ->  dL/d(images), fp32 NCHW.  (f16 multiplies d_emb by a further power of
        two chosen from its largest value, ops.f16_grad_scale: one host read of n floats.)
        record (tests): a dict that receives references to gradient tensors this pass makes anyway (no launch, no copy; all but dres are times
        `scale`, the whole power of two, which it receives as well): d_o, dq, dkv, dtok, dq0, g (the gradient at every block boundary: at the
        last block's output first, at the first block's input last), stem (the gradients at s3, s2 and s1, after their ReLU masks), dx (the
        stem convolution's fp32 dX), dres (the gradient of the resized image)."""
        sv = self.saved
        if sv is None:
            raise RuntimeError("call forward(images, save=True) before backward()")
        res, layers, width, heads, out = self.cfg
        dt, dev = self.dt, self.device
        tdt = _hip.TORCH_DTYPE[dt]
        n = sv["n"]
        c = width * 32
        hh, ww = sv["feat_hw"]
        hw = hh * ww
        t = hw + 1
        d16 = torch.empty((n, out), dtype=tdt, device=dev)
        d_emb = d_emb.contiguous()          # named: a temporary would be released before the launch is queued
        scale = self.gscale
        if dt == _hip.DT_F16:
            # the gradient shrinks by three to four orders of magnitude from the embedding to the stem: whatever size the caller's loss
            # gradient has, a further power of two (exact) puts its largest value into (F16_DEMB_TOP / 2, F16_DEMB_TOP]
            amax = torch.empty((n,), dtype=torch.float32, device=dev)
            call("pmi_quantile_abs", ptr(d_emb), ptr(amax), n, out, 1.0)
            extra = ops.f16_grad_scale(amax.tolist()) * F16_DEMB_TOP
            if extra != 1.0:
                d_emb, scale = d_emb * extra, scale * extra
        call("pmi_cast_f32_to_16", ptr(d_emb), ptr(d16), n * out, ACT_NONE, dt)
        d_o = ops.igemm(d16, self.cp_t)                                          # [n, c]
        dq = torch.empty((n, c), dtype=tdt, device=dev)
        dkv = torch.empty((n * t, 2 * c), dtype=tdt, device=dev)
        call("pmi_rn_attn_bwd", ptr(sv["q"]), ptr(sv["kv"]), ptr(sv["P"]), ptr(d_o), ptr(dq), ptr(dkv), n, t, c, heads, 64.0 ** -0.5, dt)
        dtok = ops.igemm(dkv, self.kv_t)                                         # [n*t, c]
        dq0 = ops.igemm(dq, self.q_t, out_f32=True)                              # [n, c]: the query path's share of row 0
        g = torch.empty((n, hh, ww, c), dtype=tdt, device=dev)
        call("pmi_rn_tokens_bwd", ptr(dtok), ptr(dq0), ptr(g), n, hw, c, dt)
        if record is not None:
            record.update(d_o=d_o, dq=dq, dkv=dkv, dtok=dtok, dq0=dq0, g=[g])
        for blk, (h1, h2, y) in zip(reversed(self.blocks), reversed(sv["tape"])):
            gy = self._relu_bwd(g, y)
            gh = ops.igemm(gy, blk["c3"].bwd)
            if blk["stride"] > 1:
                gh = ops.avgpool2_bwd(gh, self.dt)
            gh = self._relu_bwd(gh, h2)
            gh = self._relu_bwd(ops.igemm(gh, blk["c2"].bwd), h1)
            if blk["ds"] is not None:
                gs = ops.igemm(gy, blk["ds"].bwd)
                if blk["stride"] > 1:
                    gs = ops.avgpool2_bwd(gs, self.dt)
            else:
                gs = gy
            g = ops.igemm(gh, blk["c1"].bwd, residual=gs)                        # conv1's dX + the skip path's gradient in one epilogue
            if record is not None:
                record["g"].append(g)
        s1, s2, s3 = sv["stem"]
        note = record.setdefault("stem", []).append if record is not None else (lambda t: None)
        g = self._relu_bwd(ops.avgpool2_bwd(g, self.dt), s3)
        note(g)
        g = self._relu_bwd(ops.igemm(g, self.stem[2].bwd), s2)
        note(g)
        g = self._relu_bwd(ops.igemm(g, self.stem[1].bwd), s1)
        note(g)
        nb, h_, w_, cg = g.shape             # stride-2 convolution: dX = stride-1 convolution of the zero-inserted gradient, flipped weights
        z = torch.zeros((nb, 2 * h_, 2 * w_, cg), dtype=g.dtype, device=dev)
        z[:, ::2, ::2] = g
        dx = ops.igemm(z, self.stem[0].bwd, out_f32=True)                        # [n, res, res, 4]: channels 0..2 are the image's
        dres = torch.empty((n, 3, res, res), dtype=torch.float32, device=dev)
        call("pmi_rn_stage_input_bwd", ptr(dx), dx.shape[-1], ptr(self.std), ptr(dres), n, res, res, 1.0 / scale)
        if record is not None:
            record.update(dx=dx, dres=dres, scale=scale)
        self.saved = None
        return _resize_backward(dres, sv["in_hw"])
