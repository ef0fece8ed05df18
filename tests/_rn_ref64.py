"""float64 torch restatement of the CLIP ``ModifiedResNet`` image tower (open_clip / OpenAI-CLIP RN50 .. RN50x64), written from the
architecture, with open_clip's state-dict key names and UNFOLDED BatchNorm (eval mode, running statistics, eps 1e-5):

  stem      conv1 3x3 s2 (3 -> w/2) bn1 relu, conv2 3x3 (w/2 -> w/2) bn2 relu, conv3 3x3 (w/2 -> w) bn3 relu, avgpool 2
  Bottleneck(inplanes, planes, stride): conv1 1x1 bn1 relu, conv2 3x3 bn2 relu, avgpool(stride), conv3 1x1 (-> 4 planes) bn3,
            + skip (downsample = avgpool(stride), 1x1 conv, bn where stride > 1 or inplanes != 4 planes), relu
  attnpool  tokens (HW, row-major) with their mean prepended, + positional_embedding; multi-head attention, the mean token the only
            query, head dim 64, scale 1/8, separate q / k / v projections, then c_proj

``encode(sd, cfg, images)`` takes NCHW images in [0, 1] at the tower's resolution; gradients come from float64 autograd.
``tower(..., stages=[])`` also collects the stem output and each stage's output (the per-stage error table of a diagnostic run).

``emulate=torch.bfloat16 | torch.float16``: the same tower with the 16-bit storage of the HIP engine restated -- BatchNorm folded into
each convolution, folded weights rounded to the 16-bit type (via fp32), and every stored tensor rounded where the engine stores it (the
normalised input, each convolution's activated output, conv3 + skip before its ReLU, pooled maps, the tokens, q / k / v, the attention
output); the rounding passes gradients straight through.  Arithmetic stays float64.  The input gradient of a ReLU network is piecewise
constant in the forward values: a pre-activation that a rounding moves across zero changes the mask, so the gradient of the exact fp64
tower differs from that of ANY 16-bit forward by far more than the rounding itself -- a diagnostic for that effect (the GPU tests pin
the engine's own masks instead: ``masks=``).
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


class _Round(torch.autograd.Function):
    """x rounded to a 16-bit type (returned as float64); the gradient passes straight through."""

    @staticmethod
    def forward(ctx, x, dt):
        return x.to(dt).double()

    @staticmethod
    def backward(ctx, g):
        return g, None


def _rnd(x, dt):
    return _Round.apply(x, dt) if dt is not None else x


def _conv_bn_folded(x, sd, conv, bn, dt, stride=1):
    """conv + eval BatchNorm as one convolution with folded weights rounded to dt (through fp32, as the engine packs them) + fp32 bias."""
    w = sd[conv + ".weight"].double()
    s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + 1e-5)
    wf = (w * s.view(-1, 1, 1, 1)).float().to(dt).double()
    bf = (sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s).float().double()
    return F.conv2d(x, wf, bf, stride=stride, padding=w.shape[-1] // 2)


def _bn(x, sd, p):
    return F.batch_norm(x, sd[p + ".running_mean"].double(), sd[p + ".running_var"].double(), sd[p + ".weight"].double(),
                        sd[p + ".bias"].double(), training=False, eps=1e-5)


def _conv(x, sd, p, stride=1):
    w = sd[p + ".weight"].double()
    return F.conv2d(x, w, stride=stride, padding=w.shape[-1] // 2)


_MASKS = None        # iterator of float64 NCHW 0/1 masks while tower(masks=...) runs


def _relu(x):
    return F.relu(x) if _MASKS is None else x * next(_MASKS)


def _cbn(x, sd, conv, bn, dt, stride=1):
    if dt is None:
        return _bn(_conv(x, sd, conv, stride), sd, bn)
    return _conv_bn_folded(x, sd, conv, bn, dt, stride)


def _pool(x, k, dt):
    return _rnd(F.avg_pool2d(x, k), dt) if k > 1 else x


def _bottleneck(x, sd, p, inplanes, planes, stride, dt=None):
    out = _rnd(_relu(_cbn(x, sd, p + "conv1", p + "bn1", dt)), dt)
    out = _rnd(_relu(_cbn(out, sd, p + "conv2", p + "bn2", dt)), dt)
    out = _pool(out, stride, dt)
    out = _cbn(out, sd, p + "conv3", p + "bn3", dt)
    if stride > 1 or inplanes != 4 * planes:
        idt = _rnd(_cbn(_pool(x, stride, dt), sd, p + "downsample.0", p + "downsample.1", dt), dt)
    else:
        idt = x
    return _relu(_rnd(out + idt, dt))


def _attnpool(x, sd, heads, dt=None):
    n, c, h, w = x.shape
    t = x.flatten(2).permute(0, 2, 1)                                     # [N, HW, C], row-major (h, w)
    t = torch.cat([t.mean(dim=1, keepdim=True), t], dim=1)               # [N, HW + 1, C]
    t = _rnd(t + sd["attnpool.positional_embedding"].double()[None], dt)
    wt = lambda k: sd[f"attnpool.{k}.weight"].double() if dt is None else sd[f"attnpool.{k}.weight"].float().to(dt).double()
    lin = lambda z, k: z @ wt(k).t() + sd[f"attnpool.{k}.bias"].double()
    q = _rnd(lin(t[:, :1], "q_proj"), dt).view(n, 1, heads, -1).transpose(1, 2)    # [N, heads, 1, 64]
    k = _rnd(lin(t, "k_proj"), dt).view(n, -1, heads, c // heads).transpose(1, 2)
    v = _rnd(lin(t, "v_proj"), dt).view(n, -1, heads, c // heads).transpose(1, 2)
    p = torch.softmax((q * (c // heads) ** -0.5) @ k.transpose(-1, -2), dim=-1)
    o = _rnd((p @ v).transpose(1, 2).reshape(n, c), dt)
    return lin(o, "c_proj")


def normalize(images):
    m = torch.tensor(MEAN, dtype=torch.float64).view(1, 3, 1, 1)
    s = torch.tensor(STD, dtype=torch.float64).view(1, 3, 1, 1)
    return (images.double() - m) / s


def tower(sd, cfg, x, stages=None, emulate=None, masks=None):
    """x: normalised NCHW float64 -> embeddings [N, out_dim]; stages (a list) collects the stem and stage outputs.
    masks: the 0/1 masks of every ReLU in forward order (stem 1-3, then per block conv1, conv2, output): the tower becomes the linear map
    of that ReLU pattern, so its input gradient is the gradient of a forward whose masks they are (the HIP engine's saved activations)."""
    global _MASKS
    _MASKS = iter(masks) if masks is not None else None
    try:
        return _tower(sd, cfg, x, stages, emulate)
    finally:
        _MASKS = None


def _tower(sd, cfg, x, stages, emulate):
    res, layers, width, heads, out = cfg
    dt = emulate
    x = _rnd(x, dt)
    x = _rnd(_relu(_cbn(x, sd, "conv1", "bn1", dt, stride=2)), dt)
    x = _rnd(_relu(_cbn(x, sd, "conv2", "bn2", dt)), dt)
    x = _rnd(_relu(_cbn(x, sd, "conv3", "bn3", dt)), dt)
    x = _pool(x, 2, dt)
    if stages is not None:
        stages.append(x.detach())
    inplanes = width
    for li, nb in enumerate(layers):
        planes = width * 2 ** li
        for b in range(nb):
            stride = 2 if (li > 0 and b == 0) else 1
            x = _bottleneck(x, sd, f"layer{li + 1}.{b}.", inplanes, planes, stride, dt)
            inplanes = 4 * planes
        if stages is not None:
            stages.append(x.detach())
    return _attnpool(x, sd, heads, dt)


def encode(sd, cfg, images, emulate=None, masks=None):
    return tower(sd, cfg, normalize(images), emulate=emulate, masks=masks)


def encode_and_grad(sd, cfg, images, d_emb):
    """(embedding, d <embedding, d_emb> / d images) in float64."""
    x = images.detach().double().clone().requires_grad_(True)
    with torch.enable_grad():
        emb = encode(sd, cfg, x)
        (emb * d_emb.double()).sum().backward()
    return emb.detach(), x.grad
