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

import math

import torch
import torch.nn.functional as F

from _vit_ref64 import rel_l2, row_stat

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


# =====================================================================================================================================
# Teacher-forced pieces: the emulated tower cut where the HIP engine stores a tensor, for tests/test_gpu_rn_tower.py and
# tests/test_rn_tower_bounds_cpu.py.  Nothing below calls the library under test.
#
# ``Emu(sd, cfg, emulate)`` holds the folded, rounded weights once.  Each forward piece maps the stored input of one step of
# engine/resnet.py to its next stored tensor; each backward piece is written out (no autograd), takes the ReLU masks and the upstream
# gradient as arguments and passes every forward rounding straight through.  ``bwd=None`` is the reference the gates are measured against;
# ``bwd=<16-bit type>`` restates the 16-bit tensors of the engine's backward as well, and ``work=torch.float32`` runs the same statements in
# fp32 arithmetic (torch's CPU convolutions: another accumulation order) -- together the stand-in of a device.  ``defect=`` seeds one of
# DEFECTS.  Tensors are NCHW (maps), [N, T, C] (tokens) and [N, C]; gradients are UNSCALED unless a function says otherwise.
# =====================================================================================================================================
U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

# ---- 16-bit roundings inside each piece, counted from engine/resnet.py (the gates are sqrt(k) u) ----------------------------------------
K_RESIZE = 1        # fp32 only (the resize tables and sums): an upper count                 (the resized image from the image)
K_X0 = 1            # the staged input                                                       (x0 from the resized image)
K_STEM = 1          # the convolution's activated output; the pooled map                     (s1, s2, s3, pooled, each from its predecessor)
K_H1 = 1            # conv1's activated output                                               (h1 from x_in)
K_H2 = 1            # conv2's activated output                                               (h2 from h1)
K_Y_IDENT = 1       # conv3 + x_in in one epilogue, rounded once; the ReLU pass is exact     (y from h2 and x_in)
K_Y_DS = 2          # the downsample convolution's output, then the sum                      (y, stride 1 with downsample)
K_Y_S2 = 4          # pooled h2, pooled x_in, the downsample convolution's output, the sum   (y, stride 2)
K_TOK = 1           # the token matrix (mean in fp32, + pos, rounded once)                   (tok from x_final)
K_KV = 1            # K | V                                                                  (kv from tok)
K_Q = 1             # the projected mean token                                               (q from tok)
K_O = 1             # the attention output (scores and P stay fp32)                          (o from q and kv)
K_EMB = 1           # fp32 output of a 16-bit GEMM, nothing stored in 16 bit: an upper count (emb from o)
K_DO = 2            # d_emb cast to 16 bit, the GEMM's output                                (d_o from d_emb)
K_ATTN_BWD = 1      # dq and dkv, each rounded once from fp32 values                         (dq, dkv from d_o, q, kv, P)
K_DTOK = 1          # the GEMM's output                                                      (dtok from dkv)
K_G_FINAL = 2       # dtok, then the token adjoint's output (dq0 stays fp32)                 (g at x_final from dkv and dq)
K_BLOCK_BWD = 3     # conv3^T's output, conv2^T's output, conv1^T + gs in one epilogue; masks and the pool adjoint's 0.25 are exact in 16 bit
K_BLOCK_BWD_DS = 4  # the same + the downsample convolution's transposed output gs
K_STEM_POOL_BWD = 1  # 0.25 x and a mask: exact in 16 bit (but for f16 subnormals): an upper count  (the gradient at s3 from g at the pooled map)
K_STEM_BWD = 1      # the transposed convolution's output                                    (through conv3^T, through conv2^T)
K_DRES = 1          # fp32 only (conv1^T with fp32 output, / std / gscale): an upper count   (dx, dres from the gradient at s1)
K_RESIZE_BWD = 1    # fp32 only: an upper count                                              (the image gradient from dres)

DEFECTS = (
    "identity skip",      # the identity skip dropped from a block's sum
    "stem odd",           # the stride-2 stem convolution sampling the odd pixels
    "relu before add",    # the block's ReLU taken on conv3's output, before the skip is added
    "gs dropped",         # the skip path's gradient dropped from a block's input gradient
    "pool bwd 0.25",      # the 0.25 of the average pool's adjoint missing (a stride-2 block's main path)
    "dq0 dropped",        # the query path's gradient of the mean token dropped
    "mean 1/HW",          # the mean token formed without its 1 / HW
    "pos shift",          # the positional rows shifted by one
    "attn scale",         # the attention scale d^-1/2 missing
    "zero insert odd",    # the stem convolution's gradient zero-inserted on the odd phase
    "std channel",        # the image gradient divided by the std of the neighbouring channel
    "last pixel",         # the last pixel of the last block's output map dropped (left zero)
)
FORWARD_DEFECTS = ("identity skip", "stem odd", "relu before add", "mean 1/HW", "pos shift", "attn scale", "last pixel")
SMALL_PROBE = 2.0 ** -14       # the probe scaled to where an f16 gradient needs its loss scale


def block_table(cfg):
    """(prefix, inplanes, planes, stride, has_downsample) of every Bottleneck in forward order (restated from the architecture)"""
    res, layers, width, heads, out = cfg
    inplanes, rows = width, []
    for li, nb in enumerate(layers):
        planes = width * 2 ** li
        for b in range(nb):
            stride = 2 if (li > 0 and b == 0) else 1
            rows.append((f"layer{li + 1}.{b}.", inplanes, planes, stride, stride > 1 or inplanes != 4 * planes))
            inplanes = 4 * planes
    return rows


def k_y(stride, ds):
    return K_Y_S2 if stride > 1 else (K_Y_DS if ds else K_Y_IDENT)


def depth_fwd(cfg) -> int:
    """the sum of k over the pieces on the path image -> embedding (through kv or q: one of the two)"""
    return K_X0 + 4 * K_STEM + sum(K_H1 + K_H2 + k_y(s, ds) for _, _, _, s, ds in block_table(cfg)) + K_TOK + K_KV + K_O + K_EMB


def depth_grad(cfg) -> int:
    """the sum of k over the pieces on the path image -> embedding -> image gradient"""
    return depth_fwd(cfg) + K_DO + K_ATTN_BWD + K_G_FINAL + sum(K_BLOCK_BWD_DS if ds else K_BLOCK_BWD for *_, ds in block_table(cfg)) \
        + K_STEM_POOL_BWD + 2 * K_STEM_BWD + K_DRES


def px(x):
    """NCHW -> NHWC: rows = pixels for row_stat"""
    return x.permute(0, 2, 3, 1)


def pool_t(g, quarter=0.25):
    """adjoint of the 2x2 average pool"""
    return quarter * g.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def resize64(images, out_hw):
    from oracle import clip_vit
    return clip_vit.resize(images, out_hw)


def resize64_vjp(d_out, in_hw):
    x = torch.zeros(d_out.shape[:2] + tuple(in_hw), dtype=d_out.dtype, requires_grad=True)
    with torch.enable_grad():
        (resize64(x, d_out.shape[-2:]) * d_out).sum().backward()
    return x.grad


class Emu:
    def __init__(self, sd, cfg, emulate, work=torch.float64, defect=None):
        self.cfg, self.dt, self.work, self.defect = tuple(cfg), emulate, work, defect
        res, layers, width, heads, out = self.cfg

        def conv(c, bn):
            w = sd[c + ".weight"].double()
            s = sd[bn + ".weight"].double() / torch.sqrt(sd[bn + ".running_var"].double() + 1e-5)
            return ((w * s.view(-1, 1, 1, 1)).float().to(emulate).to(work), (sd[bn + ".bias"].double() - sd[bn + ".running_mean"].double() * s).float().to(work))

        self.stem = [conv(f"conv{i}", f"bn{i}") for i in (1, 2, 3)]
        self.blocks = [dict(stride=stride, c1=conv(p + "conv1", p + "bn1"), c2=conv(p + "conv2", p + "bn2"), c3=conv(p + "conv3", p + "bn3"),
                            ds=conv(p + "downsample.0", p + "downsample.1") if ds else None) for p, _, _, stride, ds in block_table(cfg)]
        w16 = lambda k: sd[f"attnpool.{k}.weight"].float().to(emulate).to(work)
        b32 = lambda k: sd[f"attnpool.{k}.bias"].float().to(work)
        self.pos = sd["attnpool.positional_embedding"].float().to(work)
        self.wq, self.bq = w16("q_proj"), b32("q_proj")
        self.wkv, self.bkv = torch.cat([w16("k_proj"), w16("v_proj")]), torch.cat([b32("k_proj"), b32("v_proj")])
        self.wc, self.bc = w16("c_proj"), b32("c_proj")
        self.mean = torch.tensor(MEAN, dtype=work).view(1, 3, 1, 1)
        self.std = torch.tensor(STD, dtype=work).view(1, 3, 1, 1)
        self.scale = 64.0 ** -0.5

    def r(self, x, dt="fwd"):
        """x as a stored 16-bit tensor (dt: the type, None or False = not rounded; default the forward's)"""
        dt = self.dt if dt == "fwd" or dt is True else dt
        return x if dt is None or dt is False else x.to(dt).to(self.work)

    @staticmethod
    def _conv(wb, x, stride=1):
        return F.conv2d(x, wb[0], wb[1], stride=stride, padding=wb[0].shape[-1] // 2)

    @staticmethod
    def _conv_t(wb, g):
        """dX of the stride-1 convolution"""
        return F.conv_transpose2d(g, wb[0], stride=1, padding=wb[0].shape[-1] // 2)

    @staticmethod
    def _act(y, mask):
        return torch.relu(y) if mask is None else y * mask

    # ---- forward pieces -----------------------------------------------------------------------------------------------------------------
    def resize(self, images):
        res = self.cfg[0]
        x = images.to(self.work)
        return x if tuple(x.shape[-2:]) == (res, res) else resize64(x, (res, res))

    # store=False leaves a piece's LAST rounding out (the value the engine rounds when it stores the piece's output): the reference of a
    # teacher-forced check, so that what a statistic holds is the piece's k roundings and no rounding of the reference's own
    def stage(self, resized, store=True):
        return self.r((resized.to(self.work) - self.mean) / self.std, store)

    def stem_conv(self, i, x, mask=None, store=True):
        if i == 0 and self.defect == "stem odd":
            y = self._conv(self.stem[0], x)[..., 1::2, 1::2]
        else:
            y = self._conv(self.stem[i], x, stride=2 if i == 0 else 1)
        return self.r(self._act(y, mask), store)

    def pool(self, x, store=True):
        return self.r(F.avg_pool2d(x, 2), store)

    def h1(self, i, x_in, mask=None, store=True):
        return self.r(self._act(self._conv(self.blocks[i]["c1"], x_in), mask), store)

    def h2(self, i, h1, mask=None, store=True):
        return self.r(self._act(self._conv(self.blocks[i]["c2"], h1), mask), store)

    def y(self, i, h2, x_in, mask=None, store=True):
        B = self.blocks[i]
        out = self._conv(B["c3"], self.pool(h2) if B["stride"] > 1 else h2)
        if B["ds"] is not None:
            idt = self.r(self._conv(B["ds"], self.pool(x_in) if B["stride"] > 1 else x_in))
        else:
            idt = torch.zeros_like(x_in) if self.defect == "identity skip" else x_in
        if self.defect == "relu before add":
            return self.r(torch.relu(out) + idt, store)
        y = self._act(self.r(out + idt, store), mask)
        if self.defect == "last pixel" and i == len(self.blocks) - 1:
            y = y.clone()
            y[-1, :, -1, -1] = 0
        return y

    def tokens(self, x, store=True):
        t = x.flatten(2).transpose(1, 2)                                                    # [N, HW, C], row-major
        mean = t.sum(dim=1, keepdim=True) if self.defect == "mean 1/HW" else t.mean(dim=1, keepdim=True)
        pos = torch.roll(self.pos, 1, 0) if self.defect == "pos shift" else self.pos
        return self.r(torch.cat([mean, t], dim=1) + pos, store)

    def kv(self, tok, store=True):
        return self.r(tok @ self.wkv.t() + self.bkv, store)

    def q(self, tok, store=True):
        return self.r(tok[:, 0] @ self.wq.t() + self.bq, store)

    def _heads(self, q, kv):
        n, t, c2 = kv.shape
        c, h = c2 // 2, self.cfg[3]
        return q.view(n, h, 64), kv[..., :c].reshape(n, t, h, 64), kv[..., c:].reshape(n, t, h, 64)

    def attn(self, q, kv, store=True):
        """-> (o [N, C] as stored, P [N, heads, T] unrounded)"""
        qh, k, v = self._heads(q, kv)
        s = torch.einsum("nhd,nthd->nht", qh, k) * (1.0 if self.defect == "attn scale" else self.scale)
        p = torch.softmax(s, dim=-1)
        return self.r(torch.einsum("nht,nthd->nhd", p, v).reshape(q.shape), store), p

    def emb(self, o):
        return o @ self.wc.t() + self.bc

    # ---- backward pieces ----------------------------------------------------------------------------------------------------------------
    def d_o(self, d_emb, bwd=None):
        return self.r(self.r(d_emb.to(self.work), bwd) @ self.wc, bwd)

    def attn_vjp(self, d_o, q, kv, p, bwd=None):
        """-> (dq [N, C], dkv [N, T, 2C]) from the stored q, kv and the kept fp32 P"""
        qh, k, v = self._heads(q, kv)
        n, t = kv.shape[:2]
        dO = d_o.view(qh.shape)
        dP = torch.einsum("nhd,nthd->nht", dO, v)
        dS = p * (dP - (p * dP).sum(-1, keepdim=True)) * self.scale
        dq = torch.einsum("nht,nthd->nhd", dS, k).reshape(q.shape)
        dk = torch.einsum("nht,nhd->nthd", dS, qh).reshape(n, t, -1)
        dv = torch.einsum("nht,nhd->nthd", p, dO).reshape(n, t, -1)
        return self.r(dq, bwd), self.r(torch.cat([dk, dv], dim=-1), bwd)

    def g_final(self, dkv, dq, hw, bwd=None):
        """-> (dtok [N, T, C], dq0 [N, C], g NCHW at the last block's output)"""
        hh, ww = hw
        dtok = self.r(dkv @ self.wkv, bwd)
        dq0 = dq @ self.wq
        if self.defect == "dq0 dropped":
            dq0 = torch.zeros_like(dq0)
        g = self.r(dtok[:, 1:] + (dtok[:, :1] + dq0[:, None]) / (hh * ww), bwd)
        return dtok, dq0, g.transpose(1, 2).reshape(g.shape[0], -1, hh, ww)

    def block_vjp(self, i, g_out, m1, m2, my, bwd=None):
        """the gradient at block i's input from the gradient at its output and the 0/1 masks of h1, h2 and y"""
        B = self.blocks[i]
        gy = g_out * my
        gh = self.r(self._conv_t(B["c3"], gy), bwd)
        if B["stride"] > 1:
            gh = pool_t(gh, 1.0 if self.defect == "pool bwd 0.25" else 0.25)
        gh = self.r(self._conv_t(B["c2"], gh * m2), bwd) * m1
        if B["ds"] is not None:
            gs = self.r(self._conv_t(B["ds"], gy), bwd)
            if B["stride"] > 1:
                gs = pool_t(gs)
        else:
            gs = torch.zeros_like(gy) if self.defect == "gs dropped" else gy
        return self.r(self._conv_t(B["c1"], gh) + gs, bwd)

    def stem_pool_vjp(self, g, m3):
        return pool_t(g) * m3

    def stem_conv_vjp(self, i, g, mask, bwd=None):
        """through stem convolution i (2: conv3, 1: conv2) onto the masked output of the one before"""
        return self.r(self._conv_t(self.stem[i], g), bwd) * mask

    def dres(self, g1, gscale=1.0):
        """-> (dx, dres): the stride-2 convolution's dX as the stride-1 transposed convolution of the zero-inserted gradient, then / std / gscale"""
        n, c, h, w = g1.shape
        z = g1.new_zeros(n, c, 2 * h, 2 * w)
        ph = 1 if self.defect == "zero insert odd" else 0
        z[..., ph::2, ph::2] = g1
        dx = F.conv_transpose2d(z, self.stem[0][0], stride=1, padding=1)
        std = torch.roll(self.std, 1, 1) if self.defect == "std channel" else self.std
        return dx, dx / std / gscale

    def resize_vjp(self, dres, in_hw):
        return dres if tuple(in_hw) == tuple(dres.shape[-2:]) else resize64_vjp(dres, in_hw)

    # ---- one run ------------------------------------------------------------------------------------------------------------------------
    def run(self, images, probe, bwd=None, gscale=1.0, masks=None, auto_scale=False):
        """One forward + backward under the unit probe on the normalised embedding, L = <emb / |emb|, probe>, as the dict tower_checks reads
        (the gradient tensors times gscale, as the engine's; auto_scale: times grad_scale's further power of two, as the engine's f16 pass).  masks: the 0/1 masks of every ReLU in forward order (s1, s2, s3, then h1, h2, y per
        block), pinned in the forward and the backward; default: the run's own."""
        M = iter(masks) if masks is not None else None
        nxt = (lambda: None) if M is None else (lambda: next(M).to(self.work))
        resized = self.resize(images)
        x0 = self.stage(resized)
        s1 = self.stem_conv(0, x0, nxt())
        s2 = self.stem_conv(1, s1, nxt())
        s3 = self.stem_conv(2, s2, nxt())
        x = pooled = self.pool(s3)
        blocks = []
        for i in range(len(self.blocks)):
            h1 = self.h1(i, x, nxt())
            h2 = self.h2(i, h1, nxt())
            y = self.y(i, h2, x, nxt())
            blocks.append(dict(x_in=x, h1=h1, h2=h2, y=y))
            x = y
        tok = self.tokens(x)
        kv, q = self.kv(tok), self.q(tok)
        o, p = self.attn(q, kv)
        emb = self.emb(o)
        nrm = emb.norm(dim=1, keepdim=True)
        e = emb / nrm
        g = probe.to(self.work)
        d_emb = (g - e * (e * g).sum(dim=1, keepdim=True)) / nrm * gscale
        if auto_scale:
            extra = grad_scale(float(d_emb.abs().max()))
            d_emb, gscale = d_emb * extra, gscale * extra
        mk = [m.to(self.work) for m in masks] if masks is not None else masks_of(dict(s1=s1, s2=s2, s3=s3, blocks=blocks), self.work)
        d_o = self.d_o(d_emb, bwd)
        dq, dkv = self.attn_vjp(d_o, q, kv, p, bwd)
        dtok, dq0, g = self.g_final(dkv, dq, x.shape[-2:], bwd)
        gl = [g]
        for i in reversed(range(len(self.blocks))):
            g = self.block_vjp(i, g, *mk[3 + 3 * i:6 + 3 * i], bwd=bwd)
            gl.append(g)
        g3 = self.stem_pool_vjp(g, mk[2])
        g2 = self.stem_conv_vjp(2, g3, mk[1], bwd)
        g1 = self.stem_conv_vjp(1, g2, mk[0], bwd)
        dx, dres = self.dres(g1, gscale)
        return dict(n=images.shape[0], gscale=gscale, in_hw=tuple(images.shape[-2:]), resized=resized, x0=x0, s1=s1, s2=s2, s3=s3, pooled=pooled,
                    blocks=blocks, tok=tok, kv=kv, q=q, P=p, o=o, emb=emb, d_emb=d_emb, d_o=d_o, dq=dq, dkv=dkv, dtok=dtok, dq0=dq0, g=gl,
                    stem=[g3, g2, g1], dx=dx, dres=dres, grad=self.resize_vjp(dres, images.shape[-2:]))


def grad_scale(amax: float) -> float:
    """the power of two that puts the largest |d_emb| into (512, 1024] (2^10 times one with its exponent clamped to +-24): what the engine's
    f16 backward multiplies by"""
    if not math.isfinite(amax) or amax <= 0.0:
        return 1024.0
    return 1024.0 * 2.0 ** max(-24, min(24, -math.ceil(math.log2(amax))))


def masks_of(got, work=torch.float64):
    """the 0/1 masks of every ReLU of a run in forward order, from its stored post-ReLU tensors"""
    ts = [got["s1"], got["s2"], got["s3"]] + [B[z] for B in got["blocks"] for z in ("h1", "h2", "y")]
    return [(t > 0).to(work) for t in ts]


def tower_checks(ref: Emu, images, got, whole=None, whole_pinned=None):
    """Every check of the tower tests on one run `got` (Emu.run's dict, or the same tensors taken from the HIP engine), against the float64
    emulated tower `ref`: -> [(name, statistic, k)], to be held to statistic <= sqrt(k) u -- but the check named "attn P", whose third entry
    is None and whose statistic is max |P - ref| / (1e-5 max ref), held to 1.

    Piece by piece, teacher-forced: each piece of `ref` is fed the run's OWN stored input of that piece (and, backward, its own masks and
    upstream gradient), so a statistic holds the roundings of that piece alone.  Statistics are row_stat's, rows = pixels (tokens in the
    attention pool).  whole = ref.run (its own masks) for the embedding, whole_pinned = ref.run(masks=masks_of(got)) for the gradient."""
    D = lambda z: z.double()
    gs = got["gscale"]
    out_ = []
    add = lambda name, stat, k: out_.append((name, stat, k))
    add("resized", row_stat(px(got["resized"]), px(ref.resize(images))), K_RESIZE)
    add("x0", row_stat(px(got["x0"]), px(ref.stage(D(got["resized"]), store=False))), K_X0)
    add("stem s1", row_stat(px(got["s1"]), px(ref.stem_conv(0, D(got["x0"]), store=False))), K_STEM)
    add("stem s2", row_stat(px(got["s2"]), px(ref.stem_conv(1, D(got["s1"]), store=False))), K_STEM)
    add("stem s3", row_stat(px(got["s3"]), px(ref.stem_conv(2, D(got["s2"]), store=False))), K_STEM)
    add("stem pooled", row_stat(px(got["pooled"]), px(ref.pool(D(got["s3"]), store=False))), K_STEM)
    for i, (B, T) in enumerate(zip(got["blocks"], ref.blocks)):
        kind = "s2" if T["stride"] > 1 else ("ds" if T["ds"] is not None else "id")
        add(f"block{i} h1", row_stat(px(B["h1"]), px(ref.h1(i, D(B["x_in"]), store=False))), K_H1)
        add(f"block{i} h2", row_stat(px(B["h2"]), px(ref.h2(i, D(B["h1"]), store=False))), K_H2)
        add(f"block{i} y ({kind})", row_stat(px(B["y"]), px(ref.y(i, D(B["h2"]), D(B["x_in"]), store=False))), k_y(T["stride"], T["ds"] is not None))
    x_final = D(got["blocks"][-1]["y"])
    add("tok", row_stat(got["tok"], ref.tokens(x_final, store=False)), K_TOK)
    add("kv", row_stat(got["kv"], ref.kv(D(got["tok"]), store=False)), K_KV)
    add("q", row_stat(got["q"], ref.q(D(got["tok"]), store=False)), K_Q)
    o, p = ref.attn(D(got["q"]), D(got["kv"]), store=False)
    add("attn o", row_stat(got["o"], o), K_O)
    add("attn P", float((D(got["P"]) - p).abs().max() / (1e-5 * p.max())), None)
    add("emb", row_stat(got["emb"], ref.emb(D(got["o"]))), K_EMB)
    # ---- backward: everything divided by gscale
    mk = masks_of(got)
    G = lambda z: D(z) / gs
    add("d_o", row_stat(G(got["d_o"]), ref.d_o(G(got["d_emb"]))), K_DO)
    dq, dkv = ref.attn_vjp(G(got["d_o"]), D(got["q"]), D(got["kv"]), D(got["P"]))
    add("attn bwd dq", row_stat(G(got["dq"]), dq), K_ATTN_BWD)
    add("attn bwd dkv", row_stat(G(got["dkv"]), dkv), K_ATTN_BWD)
    dtok, dq0, g = ref.g_final(G(got["dkv"]), G(got["dq"]), x_final.shape[-2:])
    add("dtok", row_stat(G(got["dtok"]), dtok), K_DTOK)
    add("dq0", row_stat(G(got["dq0"]), dq0), K_DTOK)                 # fp32 output of a 16-bit GEMM: an upper count
    add("g at x_final", row_stat(px(G(got["g"][0])), px(g)), K_G_FINAL)
    nb = len(ref.blocks)
    for j, i in enumerate(reversed(range(nb))):
        T = ref.blocks[i]
        kind = "s2" if T["stride"] > 1 else ("ds" if T["ds"] is not None else "id")
        want = ref.block_vjp(i, G(got["g"][j]), *mk[3 + 3 * i:6 + 3 * i])
        add(f"block{i} bwd ({kind})", row_stat(px(G(got["g"][j + 1])), px(want)), K_BLOCK_BWD_DS if T["ds"] is not None else K_BLOCK_BWD)
    g3, g2, g1 = (G(z) for z in got["stem"])
    add("stem bwd g3", row_stat(px(g3), px(ref.stem_pool_vjp(G(got["g"][-1]), mk[2]))), K_STEM_POOL_BWD)
    add("stem bwd g2", row_stat(px(g2), px(ref.stem_conv_vjp(2, g3, mk[1]))), K_STEM_BWD)
    add("stem bwd g1", row_stat(px(g1), px(ref.stem_conv_vjp(1, g2, mk[0]))), K_STEM_BWD)
    dx, dres = ref.dres(g1)
    add("stem bwd dx", row_stat(px(G(got["dx"])), px(dx)), K_DRES)
    add("dres", row_stat(px(got["dres"]), px(dres)), K_DRES)
    add("grad from dres", row_stat(px(got["grad"]), px(ref.resize_vjp(D(got["dres"]), got["in_hw"]))), K_RESIZE_BWD)
    if whole is not None:
        add("tower emb", rel_l2(got["emb"], whole["emb"]), depth_fwd(ref.cfg))
    if whole_pinned is not None:
        add("tower grad", rel_l2(got["grad"], whole_pinned["grad"]), depth_grad(ref.cfg))
    return out_


def small_probe_check(ref: Emu, grad_small, whole_pinned):
    """the gradient under the probe times SMALL_PROBE, scaled back, against the whole-tower reference: (name, statistic, k)"""
    return ("tower grad, small probe", rel_l2(grad_small.double() / SMALL_PROBE, whole_pinned["grad"]), depth_grad(ref.cfg))


def ratios(checks, u):
    """[(statistic / gate, name, statistic, k)]"""
    return [(st if k is None else st / (u * math.sqrt(k)), name, st, k) for name, st, k in checks]
