"""HIP engine for Real-ESRGAN's U-Net discriminator with spectral norm (perceptor/losses/super_resolution/unet_discriminator_sn.py:6-63,
num_in_ch = 3, skip_connection = True) and the guidance loss on it (discriminator.py:28-29): logits, loss = -mean(logits) * 0.001 and the
loss's gradient w.r.t. the images.  lrelu = LeakyReLU(0.2), up = bilinear x2 with align_corners=False, every skip added AFTER the activation:

  x0 = lrelu(conv0(x))            3 -> F,   3x3 p1, bias          ops.igemm + pmi_lrelu_add
  x1 = lrelu(conv1(x0))           F -> 2F,  4x4 s2 p1, SN         ops.igemm (taps 16, stride 2; tap = 4 ky + kx) + pmi_lrelu_add
  x2 = lrelu(conv2(x1))           2F -> 4F, 4x4 s2 p1, SN
  x3 = lrelu(conv3(x2))           4F -> 8F, 4x4 s2 p1, SN
  x4 = lrelu(conv4(up(x3))) + x2  8F -> 4F, 3x3 p1, SN            ops.igemm + pmi_lrelu_add (the skip is its r)
  x5 = lrelu(conv5(up(x4))) + x1  4F -> 2F                        pmi_rdb_conv3x3 (slope 0.2, zero bias) where it takes the shape (Cin <= 192,
  x6 = lrelu(conv6(up(x5))) + x0  2F -> F                         N in {32, 64}: conv6 .. conv8, and conv5 at F = 32), the skip then by
  a7 = lrelu(conv7(x6)), a8 = lrelu(conv8(a7))    F -> F          pmi_lrelu_add with slope 1; else as conv4
  logits = conv9(a8)              F -> 1, 3x3 p1, bias, fp32

Spectral norm in its eval-mode meaning: W = weight_orig / sigma, sigma = u . (reshape(weight_orig, [Cout, -1]) v) with u, v exactly as the
state dict stores them, folded once at load in float64 and rounded for packing.  Upstream never calls .eval() on the discriminator, so it
runs one power iteration per call and mutates u; at a trained checkpoint u, v sit at their fixed point and the values agree.  This engine
is the deterministic function.

Tape.  The network is piecewise linear and has no weight gradient here, so the backward needs only each LeakyReLU's sign.  It is read from
a STORED tensor whose sign is the pre-activation's: x0 .. x3 (no skip was added to them), and for conv4 .. conv8 the tensor "s{k}" the
skip was added to -- conv{k}'s 16-bit output z on the ops.igemm route, lrelu(z) on the pmi_rdb_conv3x3 route -- never x{k} - skip recomputed in
16 bit.  Per pixel of the image the tape holds F (x0) + F/2 (x1) + F/4 (x2) + F/8 (x3) + F/4 (s4) + F/2 (s5) + 3 F (s6, s7, s8) values of
16 bit: 5.625 F values, 720 bytes at F = 64 (755 MB for one 1024 x 1024 image).

Backward.  d logits is the constant -0.001 / (n_total H W).  conv9^T .. conv4^T and conv0^T are 3x3 convolutions with transposed, flipped
weights (pmi_rdb_conv3x3 with slope 1 where it takes the shape, else ops.igemm; conv0^T writes fp32), the masks between them pmi_lrelu_bwd,
the up-samplers pmi_upsample_bilinear2_bwd.  conv3^T, conv2^T, conv1^T are pmi_convt4x4s2 (csrc/disc.hip) with R = d x4, d x5, d x6 (the
gradient through the skip) and Y = x2, x1, x0: one launch gives the gradient at the previous pre-activation.  In f16 the gradients carry a
power-of-two factor (ops.f16_grad_scale of |d logits|, at most 2^24: the raw value is about 1e-9 at 1024 x 1024) that is undone at the
image; in bf16 it is 1.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch

from .. import _hip
from .._hip import call, ptr
from ..utils.synth import synth_tensor
from . import ops
from .ops import PackedLinear
from .rrdb import pack_rdb_weights

SLOPE, LOSS_SCALE = 0.2, 0.001
NUM_FEATS = (32, 64)
SN_LAYERS = tuple(range(1, 9))
POWER_ITERATIONS = 8


def _channels(f: int):
    """(Cin, Cout, k) of conv0 .. conv9"""
    return [(3, f, 3), (f, 2 * f, 4), (2 * f, 4 * f, 4), (4 * f, 8 * f, 4), (8 * f, 4 * f, 3), (4 * f, 2 * f, 3), (2 * f, f, 3), (f, f, 3),
            (f, f, 3), (f, 1, 3)]


def disc_state_dict_shapes(num_feat: int) -> Dict[str, Tuple[int, ...]]:
    """The reference's keys (torch.nn.utils.spectral_norm's weight_orig / weight_u / weight_v for conv1 .. conv8), in its module order."""
    S: Dict[str, Tuple[int, ...]] = {}
    for k, (cin, cout, ks) in enumerate(_channels(num_feat)):
        if k in SN_LAYERS:
            S[f"conv{k}.weight_orig"] = (cout, cin, ks, ks)
            S[f"conv{k}.weight_u"] = (cout,)
            S[f"conv{k}.weight_v"] = (cin * ks * ks,)
        else:
            S[f"conv{k}.weight"] = (cout, cin, ks, ks)
            S[f"conv{k}.bias"] = (cout,)
    return S


def map_state_dict(sd, num_feat: int):
    """The bare dict or the one under "params"; strict keys and shapes."""
    if "params" in sd:
        sd = sd["params"]
    want = disc_state_dict_shapes(num_feat)
    missing = [k for k in want if k not in sd]
    extra = [k for k in sd if k not in want]
    if missing or extra:
        raise ValueError(f"UNetDiscriminatorSN state dict: missing {missing[:4]}, unexpected {extra[:4]}")
    for k, shp in want.items():
        if tuple(sd[k].shape) != shp:
            raise ValueError(f"UNetDiscriminatorSN state dict: {k} has shape {tuple(sd[k].shape)}, expected {shp}")
    return {k: sd[k] for k in want}


def fold_sigma(sd, num_feat: int) -> Dict[str, torch.Tensor]:
    """{"conv{k}.weight" (float64, SN layers divided by sigma), "conv0.bias", "conv9.bias"} from a mapped state dict."""
    out = {}
    for k in range(10):
        if k in SN_LAYERS:
            w = sd[f"conv{k}.weight_orig"].detach().cpu().double()
            u, v = sd[f"conv{k}.weight_u"].detach().cpu().double(), sd[f"conv{k}.weight_v"].detach().cpu().double()
            sigma = torch.dot(u, torch.mv(w.reshape(w.shape[0], -1), v))
            out[f"conv{k}.weight"] = w / sigma
        else:
            out[f"conv{k}.weight"] = sd[f"conv{k}.weight"].detach().cpu().double()
            out[f"conv{k}.bias"] = sd[f"conv{k}.bias"].detach().cpu().double()
    return out


def synth_disc_state_dict(num_feat: int, seed: int = 0) -> Dict[str, torch.Tensor]:
    """Deterministic synthetic weights (utils.synth.synth_tensor on weight_orig, weight and bias).  u and v come from POWER_ITERATIONS power
    iterations in float64 from a synth_tensor start, normalised as torch.nn.utils.spectral_norm does (a raw random u, v would give
    sigma ~ 0 and weights that explode), stored as fp32 like every other entry."""
    sd = {}
    for name, shape in disc_state_dict_shapes(num_feat).items():
        if name.endswith(("weight_u", "weight_v")):
            continue
        sd[name] = synth_tensor(name, shape, seed)
    norm = lambda t: t / t.norm().clamp_min(1e-12)
    for k in SN_LAYERS:
        w = sd[f"conv{k}.weight_orig"].double()
        m = w.reshape(w.shape[0], -1)
        u = norm(synth_tensor(f"conv{k}.weight_u", (m.shape[0],), seed).double())
        v = norm(synth_tensor(f"conv{k}.weight_v", (m.shape[1],), seed).double())
        for _ in range(POWER_ITERATIONS):
            v = norm(torch.mv(m.t(), u))
            u = norm(torch.mv(m, v))
        sd[f"conv{k}.weight_u"], sd[f"conv{k}.weight_v"] = u.float(), v.float()
    return {k: sd[k] for k in disc_state_dict_shapes(num_feat)}


def convt_phase_weights(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 4, 4] -> [a, b, u, v, Cout, Cin] = W[co, ci, ky(a, u), kx(b, v)], ky(0, u) = 3 - 2u, ky(1, u) = 2 - 2u: the 2x2 convolution
    of output parity (a, b) over the low-resolution gradient at (p + a - 1 + u, q + b - 1 + v)."""
    if w.ndim != 4 or tuple(w.shape[2:]) != (4, 4):
        raise ValueError(f"convt_phase_weights: unsupported weight shape {tuple(w.shape)}")
    k = torch.tensor([[3, 1], [2, 0]])                       # k[a][u]
    return w[:, :, k[:, :, None, None], k[None, None, :, :]].permute(2, 4, 3, 5, 0, 1)      # [co, ci, a, u, b, v] -> [a, b, u, v, co, ci]


def pack_convt_weights(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 4, 4] -> pmi_convt4x4s2's fragment order [Cin / 16][phase = 2a + b][Cout / 32][2u + v][q = 4][r = 16][j = 8]
    = W[32 chunk + 8 q + j][16 block + r][ky(a, u)][kx(b, v)]."""
    cout, cin = w.shape[:2]
    if cout % 32 or cin % 16:
        raise ValueError(f"pack_convt_weights: unsupported weight shape {tuple(w.shape)}")
    p = convt_phase_weights(w).reshape(2, 2, 2, 2, cout // 32, 4, 8, cin // 16, 16)       # a b u v chunk q j block r
    return p.permute(7, 0, 1, 4, 2, 3, 5, 8, 6).contiguous().reshape(-1)


def rdb_takes(cin: int, n: int) -> bool:
    """The channel counts pmi_rdb_conv3x3 is built for (its _eligible query adds the grid and the pitches)."""
    return cin % 32 == 0 and 32 <= cin <= 192 and n in (32, 64)


class _Conv3:
    """One 3x3 convolution without bias, forward or transposed: pmi_rdb_conv3x3's packing where its channel counts fit, ops.igemm's on demand."""

    def __init__(self, w, dt, dev):
        self.w, self.dt, self.dev = w.float().contiguous(), dt, dev
        self.n, self.cin = int(w.shape[0]), int(w.shape[1])
        self.rdb_w = self.rdb_b = self._lin = None
        if rdb_takes(self.cin, self.n):
            self.rdb_w = pack_rdb_weights(self.w).to(device=dev, dtype=_hip.TORCH_DTYPE[dt])
            self.rdb_b = torch.zeros(self.n, dtype=torch.float32, device=dev)

    @property
    def lin(self) -> PackedLinear:
        if self._lin is None:
            self._lin = PackedLinear(self.w, None, self.dt, self.dev)
        return self._lin


def _transposed(w):
    return w.permute(1, 0, 2, 3).flip(2, 3).contiguous()


class DiscriminatorEngine:
    def __init__(self, num_feat, state_dict, device, dtype="f16"):
        f = int(num_feat)
        if f not in NUM_FEATS:
            raise ValueError(f"unsupported UNetDiscriminatorSN num_feat {num_feat}: one of {NUM_FEATS} is required (pmi_convt4x4s2 takes "
                             "Cin % 32 == 0 and Cout = 8 num_feat <= 512)")
        if dtype not in ("f16", "bf16"):
            raise ValueError("the discriminator runs in 'f16' or 'bf16'")
        self.num_feat, self.device = f, torch.device(device)
        self.dt = _hip.dtype_code(dtype)
        self.tdt = _hip.TORCH_DTYPE[self.dt]
        _hip.lib()
        W = fold_sigma(map_state_dict(state_dict, f), f)
        w = lambda k: W[f"conv{k}.weight"]
        dt, dev = self.dt, self.device
        self.conv0 = PackedLinear(w(0), W["conv0.bias"], dt, dev, cin_pad=8)
        self.conv0_t = PackedLinear(_transposed(w(0)), None, dt, dev)
        self.down = {k: PackedLinear(w(k), None, dt, dev) for k in (1, 2, 3)}
        self.down_t = {k: pack_convt_weights(w(k).float()).to(device=dev, dtype=self.tdt) for k in (1, 2, 3)}
        self.conv = {k: _Conv3(w(k), dt, dev) for k in (4, 5, 6, 7, 8)}
        self.conv_t = {k: _Conv3(_transposed(w(k)), dt, dev) for k in (4, 5, 6, 7, 8)}
        self.conv9 = PackedLinear(w(9), W["conv9.bias"], dt, dev)
        self.conv9_t = PackedLinear(_transposed(w(9)), None, dt, dev, cin_pad=8)

    # ---- launches -----------------------------------------------------------------------------------------
    def _lrelu_add(self, z, r=None, slope=SLOPE):
        y = torch.empty_like(z)
        call("pmi_lrelu_add", ptr(z), ptr(r), ptr(y), z.numel(), float(slope), self.dt)
        return y

    def _lrelu_bwd(self, g, y, g2=None, slope=SLOPE):
        dz = torch.empty_like(g)
        call("pmi_lrelu_bwd", ptr(g), ptr(g2), ptr(y), ptr(dz), g.numel(), float(slope), self.dt)
        return dz

    def _rdb_ok(self, cv: _Conv3, x) -> bool:
        n, h, w, c = x.shape
        return cv.rdb_w is not None and bool(_hip.lib().pmi_rdb_conv3x3_eligible(cv.cin, cv.n, c, cv.n, 0, 0, 0, n, h, w, self.dt))

    def _conv3(self, cv: _Conv3, x, slope):
        """(lrelu_slope(conv(x)) if pmi_rdb_conv3x3 takes the call, else conv(x); whether the activation is applied)"""
        if self._rdb_ok(cv, x):
            n, h, w, c = x.shape
            out = torch.empty((n, h, w, cv.n), dtype=self.tdt, device=x.device)
            call("pmi_rdb_conv3x3", ptr(x), c, cv.cin, ptr(cv.rdb_w), ptr(cv.rdb_b), cv.n, ptr(out), cv.n, None, 0, None, 0,
                 1.0, 1.0, float(slope), 0, n, h, w, self.dt)
            return out, True
        return ops.igemm(x, cv.lin), False

    def _act_conv(self, k, x, skip=None):
        """x_k = lrelu(conv_k(x)) + skip and the stored tensor that carries the activation's sign"""
        s, done = self._conv3(self.conv[k], x, SLOPE)
        if done:
            return (s if skip is None else self._lrelu_add(s, skip, 1.0)), s
        return self._lrelu_add(s, skip), s

    def _conv3_t(self, k, g):
        return self._conv3(self.conv_t[k], g, 1.0)[0]

    def _convt(self, k, g, r, y, out_f32=False):
        n, h, w, cout = g.shape
        cin = y.shape[-1]
        out = torch.empty((n, 2 * h, 2 * w, cin), dtype=torch.float32 if out_f32 else self.tdt, device=g.device)
        call("pmi_convt4x4s2", ptr(g), cout, cout, ptr(self.down_t[k]), cin, ptr(out), cin, ptr(r), cin if r is not None else 0, ptr(y), cin,
             SLOPE, int(out_f32), n, h, w, self.dt)
        return out

    # ---- forward ------------------------------------------------------------------------------------------
    def _check(self, images):
        if not images.is_cuda:
            raise RuntimeError("DiscriminatorEngine runs on a HIP device only (no CPU fallback)")
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"DiscriminatorEngine expects NCHW images with 3 channels, got {tuple(images.shape)}")
        if images.shape[2] % 8 or images.shape[3] % 8 or images.shape[0] < 1 or images.shape[2] < 8 or images.shape[3] < 8:
            raise ValueError(f"UNetDiscriminatorSN needs height and width that are multiples of 8 (three stride-2 levels whose outputs meet "
                             f"their skips again), got {tuple(images.shape[2:])}")

    def _forward(self, images):
        """-> (logits fp32 [N, 1, H, W], tape)"""
        self._check(images)
        x = images.detach().float().contiguous()
        n, _, h, w = x.shape
        xin = torch.empty((n, h, w, 8), dtype=self.tdt, device=x.device)
        call("pmi_nchw_to_nhwc", ptr(x), ptr(xin), n, 3, h, w, 8, 1.0, 0.0, self.dt)
        t = {}
        t["x0"] = self._lrelu_add(ops.igemm(xin, self.conv0))
        for k in (1, 2, 3):
            t[f"x{k}"] = self._lrelu_add(ops.igemm(t[f"x{k - 1}"], self.down[k], stride=2))
        y = t["x3"]
        for k, skip in ((4, "x2"), (5, "x1"), (6, "x0")):
            y, t[f"s{k}"] = self._act_conv(k, ops.upsample_bilinear2(y, self.dt), t[skip])
            t[f"x{k}"] = y
        for k in (7, 8):
            y, t[f"s{k}"] = self._act_conv(k, y)
        out = ops.igemm(y, self.conv9, out_f32=True)
        return ops.grad_to_nchw(out, 1, 1.0), t

    @torch.no_grad()
    def logits(self, images):
        return self._forward(images)[0]

    def _mean(self, logits, scale):
        out = torch.empty(1, dtype=torch.float32, device=logits.device)
        partial = torch.empty(256, dtype=torch.float32, device=logits.device)
        call("pmi_mean_f32", ptr(logits), ptr(partial), ptr(out), logits.numel(), float(scale))
        return out[0]

    # ---- loss and gradient --------------------------------------------------------------------------------
    @torch.no_grad()
    def loss_and_grad(self, images, n_total=None, record: Optional[dict] = None):
        """(loss fp32 scalar, dloss/dimages fp32 NCHW).  n_total: the global batch when this rank holds a shard (the mean is over
        n_total H W).  record: a dict that receives the tape ("x0" .. "x6", "s4" .. "s8"), "logits" and the 16-bit gradients of the backward
        ("d_*"): the LeakyReLU signs a test pins its float64 network to."""
        logits, t = self._forward(images)
        n, _, h, w = logits.shape
        count = float(int(n_total or n) * h * w)
        c = -LOSS_SCALE / count
        loss = self._mean(logits, c)
        gscale = 1.0 if self.dt == _hip.DT_BF16 else ops.f16_grad_scale([abs(c)])
        d = torch.full((n, 1, h, w), c, dtype=torch.float32, device=logits.device)
        g = torch.empty((n, h, w, 8), dtype=self.tdt, device=logits.device)
        call("pmi_nchw_to_nhwc", ptr(d), ptr(g), n, 1, h, w, 8, gscale, 0.0, self.dt)
        G = {}
        G["d_a8"] = ops.igemm(g, self.conv9_t)
        G["d_a7"] = self._conv3_t(8, self._lrelu_bwd(G["d_a8"], t["s8"]))
        G["d_x6"] = self._conv3_t(7, self._lrelu_bwd(G["d_a7"], t["s7"]))
        G["d_x5"] = ops.upsample_bilinear2_bwd(self._conv3_t(6, self._lrelu_bwd(G["d_x6"], t["s6"])), self.dt)
        G["d_x4"] = ops.upsample_bilinear2_bwd(self._conv3_t(5, self._lrelu_bwd(G["d_x5"], t["s5"])), self.dt)
        G["d_x3"] = ops.upsample_bilinear2_bwd(self._conv3_t(4, self._lrelu_bwd(G["d_x4"], t["s4"])), self.dt)
        G["d_z3"] = self._lrelu_bwd(G["d_x3"], t["x3"])
        G["d_z2"] = self._convt(3, G["d_z3"], G["d_x4"], t["x2"])
        G["d_z1"] = self._convt(2, G["d_z2"], G["d_x5"], t["x1"])
        G["d_z0"] = self._convt(1, G["d_z1"], G["d_x6"], t["x0"])
        dx = ops.igemm(G["d_z0"], self.conv0_t, out_f32=True)
        grad = ops.grad_to_nchw(dx, 3, 1.0 / gscale)
        if record is not None:
            record.update(t)
            record.update(G)
            record.update(logits=logits, gscale=gscale)
        return loss, grad
