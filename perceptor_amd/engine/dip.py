"""HIP engine for the DeepImagePrior skip network, the one network here that is trained: its gradient goes to the WEIGHTS.

Replaces get_hq_skip_net(offset_type="none") of perceptor/models/deep_image_prior (skip.py, common.py, updown.py): per scale a 1x1 skip
branch (conv -> BN -> LeakyReLU 0.2) beside a deeper branch (reflect-padded 3x3 conv -> cubic Downsample2d -> BN -> LeakyReLU -> 3x3 conv ->
BN -> LeakyReLU -> the next scale -> cubic Upsample2d), then BN over their concat (skip | deeper), a 3x3 and a 1x1 conv each with BN and
LeakyReLU; at the top a 1x1 conv to the picture's channels, DecorrelatedColorsToRGB and a sigmoid.

Kernel mapping.  Activations are NHWC 16-bit (bf16 / f16); parameters, statistics and every parameter gradient fp32.
  * Convolutions, forward and input gradient: ops.igemm on weights packed on the DEVICE by pmi_dip_pack_w EVERY forward (forward order and the
    transposed, tap-reversed order of dX; ops.PackedLinear.from_device starts with an empty `_frag`), so an optimiser step can never meet a
    stale packing -- nothing is tracked by `_version`, the 1.9 M values are simply packed again.  A reflect-padded 3x3 runs as the same-padded
    convolution on the tensor with a reflected one-pixel ring ([N, H+2, W+2, C], written by pmi_dip_bn_apply or pmi_dip_reflect_pad); only the
    interior of its output is read (the consumers take a `ring` argument).  Its input gradient is the transposed convolution on the
    zero-ringed dY followed by pmi_dip_pad_fold, the reflect pad's adjoint.
  * Weight and bias gradients: pmi_dip_wgrad (MFMA for the 192-channel layers, a plain reduction for the 4-channel skip and the head).
  * BatchNorm2d in training mode: pmi_dip_bn_stats / _apply / _bwd.  BN over the 196-channel concat runs as two channel slices (4 | 192) that
    write one ringed 200-channel tensor (channels 196..199 zero), so the concat is never materialised on its own.
  * Resamplers: pmi_fir8_* (csrc/fir.hip).  Head: pmi_dip_head_fwd / _bwd.
The tape keeps each convolution's input, each BN's input with (mean, 1/sigma); activation signs are recomputed from a x + b with the forward's
own arithmetic.  f16 scales the gradient by a power of two from max |d out| (one host read) and divides it out of every result; bf16 does not.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from .. import _hip
from .._hip import call, ptr
from . import ops
from .ops import PackedLinear

WIDTH, SKIP = 192, 4                 # get_hq_skip_net: skip_n33d = skip_n33u = 192, skip_n11 = 4
BN_MOMENTUM, BN_EPS = 0.1, 1e-5      # nn.BatchNorm2d defaults
CUBIC = [-0.01171875, -0.03515625, 0.11328125, 0.43359375, 0.43359375, 0.11328125, -0.03515625, -0.01171875]   # updown.py


def colcorr_t(dtype=torch.float32) -> torch.Tensor:
    """DecorrelatedColorsToRGB's `colcorr_t` buffer (common.py), computed in fp32 as upstream does."""
    m = torch.tensor([[0.26, 0.09, 0.02], [0.27, 0.00, -0.05], [0.27, -0.09, 0.03]])
    m = m / torch.tensor([1.6, 1.0, 1.0])
    return (m / m.norm(dim=0).max()).T.contiguous().to(dtype)


def cubic_kernels() -> Tuple[torch.Tensor, torch.Tensor]:
    k = torch.tensor([CUBIC])
    return k.T @ k, (2 * k).T @ (2 * k)


def scale_prefixes(n_scales: int) -> List[str]:
    """Module path of every scale's nn.Sequential: the top one is `network`, each deeper one sits at index 7 of its parent's deeper branch."""
    out = ["network"]
    for _ in range(n_scales - 1):
        out.append(out[-1] + ".1.1.7")
    return out


def check_size(n_scales: int, height: int, width: int) -> None:
    """Every scale halves an even map and the deepest map must keep more than 2 samples per axis: the cubic up-sampler reflect-pads by 2
    (upstream's F.pad raises at 8x8 with 2 scales and at 16x16 with 3)."""
    f = 2 ** n_scales
    if height % f or width % f or height // f <= 2 or width // f <= 2:
        raise ValueError(f"DeepImagePrior: {height}x{width} with {n_scales} scales leaves a deepest map of {height / f:g}x{width / f:g}; "
                         f"it must be whole and larger than 2 (reflect padding)")


def state_dict_shapes(n_scales: int, input_channels: int, output_channels: int = 3, decorrelate_rgb: bool = True) -> Dict[str, Tuple[int, ...]]:
    """Names and shapes of the reference module's state_dict() in its own order."""
    S: Dict[str, Tuple[int, ...]] = {}

    def conv(p, co, ci, k):
        S[p + ".weight"] = (co, ci, k, k); S[p + ".bias"] = (co,)

    def bn(p, c):
        S[p + ".weight"] = (c,); S[p + ".bias"] = (c,); S[p + ".running_mean"] = (c,); S[p + ".running_var"] = (c,)
        S[p + ".num_batches_tracked"] = ()

    def scale(p, i, cin):
        conv(p + ".1.0.1.1", SKIP, cin, 1); bn(p + ".1.0.2", SKIP)
        conv(p + ".1.1.1.1", WIDTH, cin, 3); S[p + ".1.1.1.2.kernel"] = (8, 8); bn(p + ".1.1.2", WIDTH)
        conv(p + ".1.1.4.1", WIDTH, WIDTH, 3); bn(p + ".1.1.5", WIDTH)
        if i < n_scales - 1:
            scale(p + ".1.1.7", i + 1, WIDTH)
            S[p + ".1.1.8.kernel"] = (8, 8)
        else:
            S[p + ".1.1.7.kernel"] = (8, 8)
        bn(p + ".2", SKIP + WIDTH)
        conv(p + ".3.1", WIDTH, SKIP + WIDTH, 3); bn(p + ".4", WIDTH)
        conv(p + ".6.1", WIDTH, WIDTH, 1); bn(p + ".7", WIDTH)

    scale("network", 0, input_channels)
    conv("network.9.1", output_channels, WIDTH, 1)
    if decorrelate_rgb:
        S["network.10.colcorr_t"] = (3, 3)
    return S


def synthetic_state_dict(n_scales: int, input_channels: int, output_channels: int = 3, decorrelate_rgb: bool = True, seed: int = 0):
    """Name-keyed synthetic values (utils.synth): BN gains around 1 and biases around 0 but not AT them, running statistics off their
    initial (0, 1), the resampling and colour buffers at their true values."""
    from ..utils.synth import synth_tensor
    kd, ku = cubic_kernels()
    sd = {}
    for k, s in state_dict_shapes(n_scales, input_channels, output_channels, decorrelate_rgb).items():
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.tensor(3, dtype=torch.int64)
        elif k.endswith(".kernel"):
            sd[k] = (kd if k.endswith(".2.kernel") else ku).clone()
        elif k.endswith("colcorr_t"):
            sd[k] = colcorr_t()
        else:
            sd[k] = synth_tensor(k, s, seed)
    return sd


def _r8(c: int) -> int:
    return (c + 7) // 8 * 8


class DIPEngine:
    def __init__(self, n_scales: int, input_channels: int, output_channels: int = 3, sigmoid: bool = True, decorrelate_rgb: bool = True,
                 dtype="bf16"):
        if n_scales < 1:
            raise ValueError("DeepImagePrior: n_scales must be at least 1")
        if not 1 <= output_channels <= 4:
            raise ValueError("DeepImagePrior: the fused output head writes 1 to 4 channels")
        if decorrelate_rgb and output_channels != 3:
            raise ValueError("DeepImagePrior: decorrelate_rgb needs 3 output channels (its matrix is 3 x 3)")
        if input_channels < 1:
            raise ValueError("DeepImagePrior: input_channels must be positive")
        self.n_scales, self.cin, self.cout = n_scales, input_channels, output_channels
        self.sigmoid, self.decorrelate = bool(sigmoid), bool(decorrelate_rgb)
        self.dt = _hip.dtype_code(dtype)
        if self.dt not in (_hip.DT_F16, _hip.DT_BF16):
            raise ValueError("DIPEngine: dtype must be 'bf16' or 'f16'")
        self.prefixes = scale_prefixes(n_scales)

    # ---- helpers ---------------------------------------------------------------------------------------------------------------------
    def _e16(self, shape, dev, zero=False):
        return (torch.zeros if zero else torch.empty)(shape, dtype=_hip.TORCH_DTYPE[self.dt], device=dev)

    def _pack(self, P, name, cin_p, want_dx=True):
        """(forward PackedLinear, dX PackedLinear or None) of conv `name`, packed now from the live fp32 parameters."""
        w, b = P[name + ".weight"], P[name + ".bias"]
        cout, cin, kh, kw = w.shape
        taps, n_p, cout_p = kh * kw, (cout + 3) // 4 * 4, _r8(cout)
        dev = w.device
        fwd = self._e16((n_p, taps * cin_p), dev)
        dxp = self._e16((cin_p, taps * cout_p), dev) if want_dx else None
        call("pmi_dip_pack_w", ptr(w.detach()), ptr(fwd), ptr(dxp), cout, cin, taps, n_p, cin_p, cin_p, cout_p, self.dt)
        bias = b.detach()
        if n_p != cout:
            bias = torch.zeros(n_p, dtype=torch.float32, device=dev)
            bias[:cout] = b.detach()
        lin = PackedLinear.from_device(fwd, bias, cout, cin, taps, self.dt)
        lin_dx = PackedLinear.from_device(dxp, None, cin, cout, taps, self.dt) if want_dx else None
        return lin, lin_dx

    def _bn(self, x, xr, nhw, P, name, lo, hi, act, train, rec, dst=None, dst_off=0, yr=0):
        """BatchNorm channels lo:hi of module `name` over x (ring xr, channels hi - lo) + activation.  dst: a wider destination (written at
        channel dst_off); otherwise a fresh tensor with ring yr.  rec: the tape list (training) that receives (x, xr, mean, rstd)."""
        n, h, w = nhw
        c, dev = hi - lo, x.device
        gamma, beta = P[name + ".weight"].detach()[lo:hi], P[name + ".bias"].detach()[lo:hi]
        rm, rv = P[name + ".running_mean"][lo:hi], P[name + ".running_var"][lo:hi]
        if train:
            mean = torch.empty(c, dtype=torch.float32, device=dev)
            rstd = torch.empty(c, dtype=torch.float32, device=dev)
            part = torch.empty(_hip.lib().pmi_dip_bn_blocks(n * h * w) * c, dtype=torch.float32, device=dev)
            call("pmi_dip_bn_stats", ptr(x), x.shape[-1], xr, ptr(part), ptr(mean), ptr(rstd), ptr(rm), ptr(rv), n, h, w, c, BN_MOMENTUM, BN_EPS,
                 self.dt)
            if lo == 0:
                P[name + ".num_batches_tracked"].add_(1)
        else:
            mean, rstd = rm.float(), torch.rsqrt(rv.float() + BN_EPS)
        if dst is None:
            dst = self._e16((n, h + 2 * yr, w + 2 * yr, c), dev)
        call("pmi_dip_bn_apply", ptr(x), x.shape[-1], xr, ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), dst.data_ptr() + 2 * dst_off, dst.shape[-1],
             yr, n, h, w, c, act, self.dt)
        if rec is not None:
            rec.append((x, xr, mean, rstd))
        return dst

    # ---- forward -----------------------------------------------------------------------------------------------------------------------
    def _scale(self, i, x, nhw, P, tape, train):
        n, h, w = nhw
        p, dev, last = self.prefixes[i], x.device, i == self.n_scales - 1
        cin_p = x.shape[-1]
        keep = tape is not None
        want_dx = keep and (i > 0 or tape["latent_grad"])
        T = {"nhw": nhw, "x": x, "bn": []} if keep else None
        rec = T["bn"] if keep else None
        half = (n, h // 2, w // 2)
        # skip branch
        lin, dxs = self._pack(P, p + ".1.0.1.1", cin_p, want_dx)
        s = ops.igemm(x, lin)
        sa = self._bn(s, 0, nhw, P, p + ".1.0.2", 0, SKIP, 1, train, rec)
        # deeper branch
        xp = self._e16((n, h + 2, w + 2, cin_p), dev)
        call("pmi_dip_reflect_pad", ptr(x), ptr(xp), n, h, w, cin_p, self.dt)
        lin, dx1 = self._pack(P, p + ".1.1.1.1", cin_p, want_dx)
        c1 = ops.igemm(xp, lin)
        d = self._e16((n, h // 2, w // 2, WIDTH), dev)
        call("pmi_fir8_down2", ptr(c1), 1, ptr(d), n, h, w, WIDTH, self.dt)
        dp = self._bn(d, 0, half, P, p + ".1.1.2", 0, WIDTH, 1, train, rec, yr=1)
        lin, dx2 = self._pack(P, p + ".1.1.4.1", WIDTH, keep)
        c2 = ops.igemm(dp, lin)
        e = self._bn(c2, 1, half, P, p + ".1.1.5", 0, WIDTH, 1, train, rec)
        f = e if last else self._scale(i + 1, e, half, P, tape, train)
        u = self._e16((n, h, w, WIDTH), dev)
        call("pmi_fir8_up2", ptr(f), ptr(u), n, h // 2, w // 2, WIDTH, self.dt)
        # BN over (skip | deeper) as two slices of one ringed tensor; channels 196..199 stay zero
        catp = self._e16((n, h + 2, w + 2, _r8(SKIP + WIDTH)), dev, zero=True)
        self._bn(sa, 0, nhw, P, p + ".2", 0, SKIP, 0, train, rec, dst=catp, dst_off=0, yr=1)
        self._bn(u, 0, nhw, P, p + ".2", SKIP, SKIP + WIDTH, 0, train, rec, dst=catp, dst_off=SKIP, yr=1)
        lin, dx3 = self._pack(P, p + ".3.1", _r8(SKIP + WIDTH), keep)
        c3 = ops.igemm(catp, lin)
        g = self._bn(c3, 1, nhw, P, p + ".4", 0, WIDTH, 1, train, rec)
        lin, dx4 = self._pack(P, p + ".6.1", WIDTH, keep)
        c4 = ops.igemm(g, lin)
        out = self._bn(c4, 0, nhw, P, p + ".7", 0, WIDTH, 1, train, rec)
        if keep:
            T.update(xp=xp, dp=dp, catp=catp, g=g, dx=(dxs, dx1, dx2, dx3, dx4))
            tape[p] = T
        return out

    @torch.no_grad()
    def forward(self, latents: torch.Tensor, P: Dict[str, torch.Tensor], train: bool = True, tape: Optional[dict] = None) -> torch.Tensor:
        """latents NCHW fp32 on a HIP device; P: the module's parameters and buffers by reference key name (live tensors: the running
        statistics are updated in place when `train`).  tape: a dict {"latent_grad": bool} that is filled for backward()."""
        if not latents.is_cuda:
            raise RuntimeError("DeepImagePrior runs on a HIP device only (no CPU fallback)")
        if latents.ndim != 4 or latents.shape[1] != self.cin:
            raise ValueError(f"latents must be [N, {self.cin}, H, W], got {tuple(latents.shape)}")
        if tape is not None and not train:
            raise NotImplementedError("DeepImagePrior: no backward in eval mode (running statistics); call .train() to optimise")
        _hip.lib()
        lat = latents.detach().float().contiguous()
        n, c, h, w = lat.shape
        check_size(self.n_scales, h, w)
        dev, cin_p = lat.device, _r8(c)
        x = self._e16((n, h, w, cin_p), dev)
        call("pmi_nchw_to_nhwc", ptr(lat), ptr(x), n, c, h, w, cin_p, 1.0, 0.0, self.dt)
        feat = self._scale(0, x, (n, h, w), P, tape, train)
        out = torch.empty((n, self.cout, h, w), dtype=torch.float32, device=dev)
        hw_, hb = P["network.9.1.weight"].detach(), P["network.9.1.bias"].detach()
        cm = P["network.10.colcorr_t"].detach().float().contiguous() if self.decorrelate else None
        call("pmi_dip_head_fwd", ptr(feat), ptr(hw_), ptr(hb), ptr(cm), ptr(out), n, h * w, WIDTH, self.cout, int(self.sigmoid), self.dt)
        if tape is not None:
            _, dxh = self._pack(P, "network.9.1", WIDTH, True)
            tape.update(feat=feat, out=out, cm=cm, dxh=dxh, nhw=(n, h, w))
        return out

    # ---- backward ----------------------------------------------------------------------------------------------------------------------
    def _wgrad(self, grads, name, dy, dyr, x, xr, nhw, cout, cin, taps, alpha):
        n, h, w = nhw
        dev = dy.device
        splits = _hip.lib().pmi_dip_wgrad_splits(n * h * w, cout, cin, taps)
        slabs = torch.empty(splits * (cout * cin * taps + cout), dtype=torch.float32, device=dev)
        k = 3 if taps == 9 else 1
        dW = torch.empty((cout, cin, k, k), dtype=torch.float32, device=dev)
        db = torch.empty((cout,), dtype=torch.float32, device=dev)
        call("pmi_dip_wgrad", ptr(dy), dy.shape[-1], dyr, ptr(x), x.shape[-1], xr, ptr(slabs), ptr(dW), ptr(db), n, h, w, cout, cin, taps, splits,
             alpha, self.dt)
        grads[name + ".weight"], grads[name + ".bias"] = dW, db

    def _bn_bwd(self, grads, P, name, lo, hi, act, rec, dy, dy_off, nhw, alpha, dxr=0, dx_c=None):
        """dx of BN channels lo:hi (+ activation) from dy (channels dy_off .. of a compact tensor); fills the slice of the module's gradients."""
        n, h, w = nhw
        x, xr, mean, rstd = rec
        c, dev = hi - lo, dy.device
        full = P[name + ".weight"].shape[0]
        for leaf in (".weight", ".bias"):
            if name + leaf not in grads:
                grads[name + leaf] = torch.empty(full, dtype=torch.float32, device=dev)
        gamma, beta = P[name + ".weight"].detach()[lo:hi], P[name + ".bias"].detach()[lo:hi]
        part = torch.empty(2 * _hip.lib().pmi_dip_bn_blocks(n * h * w) * c, dtype=torch.float32, device=dev)
        sums = torch.empty(2 * c, dtype=torch.float32, device=dev)
        ring_or_pad = dxr or (dx_c is not None and dx_c != c)
        dx = self._e16((n, h + 2 * dxr, w + 2 * dxr, dx_c or c), dev, zero=bool(ring_or_pad))
        call("pmi_dip_bn_bwd", ptr(x), x.shape[-1], xr, dy.data_ptr() + 2 * dy_off, dy.shape[-1], ptr(mean), ptr(rstd), ptr(gamma), ptr(beta),
             ptr(part), ptr(sums), ptr(grads[name + ".weight"][lo:hi]), ptr(grads[name + ".bias"][lo:hi]), ptr(dx), dx.shape[-1], dxr, n, h, w, c,
             act, alpha, self.dt)
        return dx

    def _fold(self, gp, nhw, add=None):
        n, h, w = nhw
        dx = self._e16((n, h, w, gp.shape[-1]), gp.device)
        call("pmi_dip_pad_fold", ptr(gp), ptr(add), ptr(dx), n, h, w, gp.shape[-1], self.dt)
        return dx

    def _scale_back(self, i, g, P, tape, grads, alpha):
        p, last = self.prefixes[i], i == self.n_scales - 1
        T = tape[p]
        nhw = T["nhw"]
        n, h, w = nhw
        half = (n, h // 2, w // 2)
        x, bn = T["x"], T["bn"]                  # bn: skip, bn2, bn5, bn196[0:4], bn196[4:196], bn4, bn7 in forward order
        dxs, dx1, dx2, dx3, dx4 = T["dx"]
        cin = P[p + ".1.0.1.1.weight"].shape[1]
        dev = g.device
        dh = self._bn_bwd(grads, P, p + ".7", 0, WIDTH, 1, bn[6], g, 0, nhw, alpha)
        self._wgrad(grads, p + ".6.1", dh, 0, T["g"], 0, nhw, WIDTH, WIDTH, 1, alpha)
        dg = ops.igemm(dh, dx4)
        dc3 = self._bn_bwd(grads, P, p + ".4", 0, WIDTH, 1, bn[5], dg, 0, nhw, alpha, dxr=1)
        self._wgrad(grads, p + ".3.1", dc3, 1, T["catp"], 1, nhw, WIDTH, SKIP + WIDTH, 9, alpha)
        dcat = self._fold(ops.igemm(dc3, dx3), nhw)                                   # [n, h, w, 200]
        dsa = self._bn_bwd(grads, P, p + ".2", 0, SKIP, 0, bn[3], dcat, 0, nhw, alpha)
        du = self._bn_bwd(grads, P, p + ".2", SKIP, SKIP + WIDTH, 0, bn[4], dcat, SKIP, nhw, alpha)
        ds = self._bn_bwd(grads, P, p + ".1.0.2", 0, SKIP, 1, bn[0], dsa, 0, nhw, alpha, dx_c=8)
        self._wgrad(grads, p + ".1.0.1.1", ds, 0, x, 0, nhw, SKIP, cin, 1, alpha)
        dx_skip = ops.igemm(ds, dxs) if dxs is not None else None
        df = self._e16((n, h // 2, w // 2, WIDTH), dev)
        call("pmi_fir8_up2_bwd", ptr(du), ptr(df), n, h // 2, w // 2, WIDTH, self.dt)
        de = df if last else self._scale_back(i + 1, df, P, tape, grads, alpha)
        dc2 = self._bn_bwd(grads, P, p + ".1.1.5", 0, WIDTH, 1, bn[2], de, 0, half, alpha, dxr=1)
        self._wgrad(grads, p + ".1.1.4.1", dc2, 1, T["dp"], 1, half, WIDTH, WIDTH, 9, alpha)
        ddp = self._fold(ops.igemm(dc2, dx2), half)
        dd = self._bn_bwd(grads, P, p + ".1.1.2", 0, WIDTH, 1, bn[1], ddp, 0, half, alpha)
        dc1 = self._e16((n, h + 2, w + 2, WIDTH), dev, zero=True)
        call("pmi_fir8_down2_bwd", ptr(dd), ptr(dc1), 1, n, h, w, WIDTH, self.dt)
        self._wgrad(grads, p + ".1.1.1.1", dc1, 1, T["xp"], 1, nhw, WIDTH, cin, 9, alpha)
        if dx1 is None:
            return None
        return self._fold(ops.igemm(dc1, dx1), nhw, add=dx_skip)

    @torch.no_grad()
    def backward(self, tape: dict, d_out: torch.Tensor, P: Dict[str, torch.Tensor]):
        """(gradients by parameter name, fp32 in PyTorch's layouts; d loss / d latents NCHW fp32 or None) from d loss / d output."""
        n, h, w = tape["nhw"]
        d = d_out.detach().float().contiguous()
        dev = d.device
        scale = 1.0
        if self.dt == _hip.DT_F16:
            amax = torch.empty((n,), dtype=torch.float32, device=dev)
            call("pmi_quantile_abs", ptr(d), ptr(amax), n, d[0].numel(), 1.0)
            scale = ops.f16_grad_scale(amax.tolist())
        alpha = 1.0 / scale
        grads: Dict[str, torch.Tensor] = {}
        dz = self._e16((n, h, w, 8), dev)
        call("pmi_dip_head_bwd", ptr(d), ptr(tape["out"]), ptr(tape["cm"]), ptr(dz), n, h * w, self.cout, int(self.sigmoid), scale, self.dt)
        self._wgrad(grads, "network.9.1", dz, 0, tape["feat"], 0, (n, h, w), self.cout, WIDTH, 1, alpha)
        g = ops.igemm(dz, tape["dxh"])
        gx = self._scale_back(0, g, P, tape, grads, alpha)
        dlat = None
        if gx is not None:
            dlat = (gx[..., :self.cin].float() * alpha).permute(0, 3, 1, 2).contiguous()     # (layout only)
        return grads, dlat
