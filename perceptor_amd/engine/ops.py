"""Tensor-level wrappers over the C ABI (perceptor_amd/_hip.py).

Activations are NHWC 16-bit torch tensors ([N, H, W, C] or [M, C]); every
function launches hand-written HIP kernels on the current stream.  torch is
used only for device memory.
"""
from __future__ import annotations

import math
import os
import ctypes as C
from typing import Optional

import torch

from .. import _hip
from .._hip import ACT_GEGLU, ACT_NONE, DT_F16X2, IgemmArgs, SkipArgs, call, ptr


HALO_ENABLED = True
SPLITK_ENABLED = True
GEMM_WD_ENABLED = True       # weights-direct GEMM (csrc/gemm_wd.hip) for plain GEMMs
GEMM_WD_CONV = os.environ.get("PMI_GEMM_WD_CONV", "1") != "0"   # A-B switch: small-map 3x3 convolutions on the weights-direct GEMM (csrc/gemm_wd.hip, CONV)
# Smallest map (pixels per image) on which a ResBlock's two-source 1x1 skip convolution is folded into its conv2 launch (pmi_conv3x3_skip);
# smaller maps keep the separate skip GEMM.  Set per level by measurement (profiles/conv_skip_ab.txt); structural, never a function of the batch.
SKIP_FUSE_MIN_HW = 64 * 64
FLASH_ENABLED = True    # general flash attention (csrc/attn_flash.hip) instead of batched GEMMs + softmax where the head dim is not 64


def set_halo(enabled: bool) -> None:
    """A/B switch: route conv3x3 through the LDS-halo kernel (default) or the generic implicit-GEMM kernel."""
    global HALO_ENABLED
    HALO_ENABLED = bool(enabled)
    _hip.lib().pmi_set_option(0, int(enabled))


# bench.py sets this to a list to time every 3x3-convolution launch (conv3x3_wd_kernel, conv3x3_halo_kernel) with HIP events on the launch stream
KERNEL_EVENTS = None
GEMM_TRACE = None    # tools/gemm_trace.py: list collecting (desc, flops, ev0, ev1) of every pmi_igemm launch
DEBUG_WS = None      # tools/conv_probe.py --stamps: int64 buffer the PMI_STAMPS build of conv3x3.hip writes phase timestamps to


def _empty(shape, dtype, device):
    return torch.empty(shape, dtype=dtype, device=device)


def split_group(c: int) -> int:
    """Group size of a precise (hi + lo) tensor with c logical channels (csrc/common.h: F16X2)."""
    if c % 32 == 0:
        return 32
    if c > 32 or c % 8:
        raise ValueError(f"precise tensors need a channel count that is a multiple of 32 (or of 8 below 32), got {c}")
    return c


def logical_c(x: torch.Tensor, dt: int) -> int:
    return x.shape[-1] // 2 if dt == DT_F16X2 else x.shape[-1]


class PackedLinear:
    """Weights packed for pmi_igemm: B[Npad][K] 16-bit with k = tap*Cin + c, fp32 bias.

    dt = precise (DT_F16X2): the inputs are hi + lo tensors with 2*Cin channels per pixel ([hi G | lo G] per group of G channels), so
    the f16 weights are duplicated along K in the same pattern: W*hi + W*lo accumulates in fp32 on the MFMA.  `sources` gives the
    logical channel counts of a two-pointer concat input (each source is its own precise tensor with its own grouping).
    concat_sources = False keeps two-source fp32 weights a two-pointer layer (their low part rounded away, with a warning): the mixed
    mode's fused-prologue configs read the two sources through their own pointers.
    up_phase = True: the layer convolves a nearest-x2 up-sampled input (ops.igemm(..., up=True)); where its shape can take the phased
    kernel (csrc/conv_up_wd.hip) the phase weights are summed HERE, from the unrounded weights (frag16_up)."""

    def __init__(self, weight: torch.Tensor, bias: Optional[torch.Tensor], dt: int, device, cin_pad: Optional[int] = None, sources=None,
                 concat_sources: bool = True, up_phase: bool = False):
        w = weight.detach().float()
        if w.ndim == 3:   # Conv1d k=1
            w = w[..., 0]
        if w.ndim == 2:
            w = w[:, :, None, None]
        cout, cin, kh, kw = w.shape
        self.cout, self.cin, self.taps = cout, cin, kh * kw
        self.cin_p = cin_pad if cin_pad is not None else (cin + 7) // 8 * 8
        self.n_p = (cout + 3) // 4 * 4
        packed = torch.zeros(self.n_p, kh * kw, self.cin_p, dtype=torch.float32)
        packed[:cout, :, :cin] = w.permute(0, 2, 3, 1).reshape(cout, kh * kw, cin)
        self.split = dt == DT_F16X2
        self.cin_l = self.cin_p                      # logical input channels
        self.self_concat = False
        self.concat_inputs = False                   # self_concat over two sources: igemm() joins a0 | a1 into one split tensor
        if self.split:
            def dup(wt, lo_zero=False):              # [N, taps, C] -> [N, taps, 2C] in the [hi G | lo G] pattern of the input
                parts, o = [], 0
                for cs in (sources or [self.cin_l]):
                    g = split_group(cs)
                    blk = wt[:, :, o:o + cs].reshape(self.n_p, kh * kw, cs // g, 1, g).expand(-1, -1, -1, 2, -1).clone()
                    if lo_zero:
                        blk[:, :, :, 1, :] = 0
                    parts.append(blk.reshape(self.n_p, kh * kw, 2 * cs))
                    o += cs
                assert o == self.cin_l
                return torch.cat(parts, dim=2)
            w_hi = packed.to(torch.float16).float()
            w_lo = packed - w_hi                     # what f16 cannot hold of fp32 weights (zero for fp16 checkpoints / the synthetic weights)
            self._w1, self._sources = w_hi, list(sources or [self.cin_l])     # un-duplicated weights: other duplication patterns are built on demand
            packed = dup(w_hi)
            self.cin_p = 2 * self.cin_l              # channels of the (physical) input tensors
            # f16 holds the weights to within the mode's own precision: nothing to add.  Otherwise the low part becomes a second K block.
            # The measure is the low part's share of the weight NORM (what reaches a sum over K), not its largest element: bf16-exact or
            # fp16-checkpoint weights of a long-K layer have a few values under the f16 subnormal grid (< 2^-14: they lose < 3e-8 absolute,
            # ~4e-8 of the norm) -- the max-element test of round 2 doubled K for every such layer (4x the MFMA work, for nothing).
            if float(w_lo.norm()) > 2.0 ** -22 * float(w_hi.norm()):
                # two sources whose groupings are all 32 wide: their split tensors concatenate into one split tensor with the same
                # [hi 32 | lo 32] grouping, so the layer is the single-source one below and igemm() concatenates a0 | a1 before the call
                concat_ok = sources is None or (concat_sources and all(cs % 32 == 0 for cs in sources))
                if not concat_ok:
                    import warnings
                    warnings.warn("precise mode: fp32 weights of a two-source (concat) convolution are rounded to f16")
                else:
                    # second K block over the SAME input tensor (passed again as the second source): W_lo * x_hi
                    packed = torch.cat([packed, dup(w_lo, lo_zero=True)], dim=2)
                    self.self_concat = True
                    self.concat_inputs = sources is not None
                    self.cin_p = 2 * self.cin_p
        self.w = packed.reshape(self.n_p, -1).to(device=device, dtype=_hip.TORCH_DTYPE[dt]).contiguous()
        self.b = None
        if bias is not None:
            b = torch.zeros(self.n_p, dtype=torch.float32)
            b[:cout] = bias.detach().float()
            self.b = b.to(device)
        self.dt = dt
        self._frag = {}
        if up_phase and not self.split and kh == 3 and kw == 3 and self.n_p % 256 == 0 and self.cin_p % 64 == 0:
            self._frag[("up", 64)] = self._pack_up(packed.view(self.n_p, 3, 3, self.cin_p), 64, device, dt)

    @classmethod
    def from_device(cls, w16: torch.Tensor, bias: Optional[torch.Tensor], cout: int, cin: int, taps: int, dt: int) -> "PackedLinear":
        """A layer whose B[n_p][taps * cin_p] was packed on the DEVICE (pmi_dip_pack_w) from weights an optimiser moves: engine/dip.py builds
        one per convolution per forward, so `_frag` starts empty and no derived packing of older weights is ever served.  bias: fp32 [n_p]."""
        lin = cls.__new__(cls)
        lin.cout, lin.cin, lin.taps, lin.n_p = cout, cin, taps, w16.shape[0]
        lin.cin_p = lin.cin_l = w16.shape[1] // taps
        lin.split = lin.self_concat = lin.concat_inputs = False
        lin.w, lin.b, lin.dt, lin._frag = w16, bias, dt, {}
        return lin

    @staticmethod
    def _pack_up(w: torch.Tensor, ck: int, device, dt: int) -> torch.Tensor:
        """w: fp32 [N, dy, dx, Cin], unrounded -> the phase weights in the kernel's fragment order (see frag16_up)."""
        n, _, _, cin = w.shape
        # tap sums per axis: phase 0 reads (low-resolution index - 1 | index) with (w0 | w1 + w2), phase 1 (index | index + 1) with (w0 + w1 | w2)
        rows = torch.stack([torch.stack([w[:, 0], w[:, 1] + w[:, 2]], 1), torch.stack([w[:, 0] + w[:, 1], w[:, 2]], 1)], 1)   # [N, a, u, dx, Cin]
        eff = torch.stack([torch.stack([rows[:, :, :, 0], rows[:, :, :, 1] + rows[:, :, :, 2]], 3),
                           torch.stack([rows[:, :, :, 0] + rows[:, :, :, 1], rows[:, :, :, 2]], 3)], 2)                       # [N, a, b, u, v, Cin]
        eff = eff.to(device=device, dtype=_hip.TORCH_DTYPE[dt])                                                               # rounded once
        e = eff.view(n // 32, 2, 16, 2, 2, 2, 2, cin // ck, ck // 32, 4, 8)      # nb, cb, r16, a, b, u (dy), v (dx), chunk, k32, q4, j
        return e.permute(0, 3, 4, 7, 6, 8, 5, 1, 9, 2, 10).contiguous()

    def frag16_up(self, ck: int) -> Optional[torch.Tensor]:
        """Phase weights of a convolution over a nearest-x2 up-sampled input (csrc/conv_up_wd.hip, tile config 9): output parity (a, b) is a
        2x2 convolution on the low-resolution grid whose taps are sums of the 3x3 ones, summed in fp32 from the weights the layer was
        constructed with and rounded once: [N/32][phase 2a + b][Cin/ck][dx][ck/32][dy][16-channel block][lane = 16*(k quarter) + channel][8 k].
        None unless the layer was constructed with up_phase=True (no fp32 copy of the weights is kept to build it later)."""
        return self._frag.get(("up", ck))

    def up_weights(self) -> torch.Tensor:
        """The phase weights as packed, back in [N, a, b, u, v, Cin] order (tests: the kernel's own arithmetic)."""
        f = self._frag[("up", 64)]                      # nb, a, b, chunk, v, k32, u, cb, q4, r16, j
        return f.permute(0, 7, 9, 1, 2, 6, 4, 3, 5, 8, 10).reshape(self.n_p, 2, 2, 2, 2, self.cin_p)

    @property
    def K(self):
        return self.taps * self.cin_p

    def frag_gemm(self) -> torch.Tensor:
        """Fragment order for the weights-direct GEMM (csrc/gemm_wd.hip), 16x16x32 MFMA:
        [N/32][K/128][32-deep k-step (4)][16-column block (2)][lane = 16*(k quarter) + column][8 k]."""
        if "gemm" not in self._frag:
            assert self.taps in (1, 9) and self.n_p % 32 == 0 and self.K % 32 == 0     # (taps 9: the GEMM kernel's conv mode, k = tap * Cin + c)
            kp = (self.K + 127) // 128 * 128                                    # K tail: zero weights up to a whole 128-deep chunk
            w = self.w
            if kp != self.K:
                w = torch.zeros((self.n_p, kp), dtype=self.w.dtype, device=self.w.device)
                w[:, :self.K] = self.w
            w = w.view(self.n_p // 32, 2, 16, kp // 128, 4, 4, 8)              # nb, cb, r16, chunk, k32, q4, j
            self._frag["gemm"] = w.permute(0, 3, 4, 1, 5, 2, 6).contiguous()
        return self._frag["gemm"]

    def frag16(self, ck: int, dup_g: int = 0) -> torch.Tensor:
        """Fragment order for the 16x16x32 MFMA form of the weights-direct kernel:
        [N/32][Cin/ck][dx][ck/32][dy][16-channel block][lane = 16*(k quarter) + channel][8 k].
        dup_g (split weights only): the K order [W of dup_g logical channels | the same again] per group -- the kernel's fused prologue
        over a split input stages a chunk as [yh of ck/2 channels | their yl] (csrc/conv_wd.hip, SIN = 1), so dup_g = ck / 2; the default
        is the tensors' own memory order, groups of 32."""
        key = ("mf16", ck, dup_g)
        if key not in self._frag:
            assert self.taps == 9 and self.n_p % 32 == 0 and self.cin_p % ck == 0
            src = self.w
            if dup_g and dup_g != 32:
                assert self.split and not self.self_concat and all(cs % dup_g == 0 for cs in self._sources)
                parts, o = [], 0
                for cs in self._sources:
                    blk = self._w1[:, :, o:o + cs].reshape(self.n_p, 9, cs // dup_g, 1, dup_g).expand(-1, -1, -1, 2, -1)
                    parts.append(blk.reshape(self.n_p, 9, 2 * cs))
                    o += cs
                src = torch.cat(parts, dim=2).reshape(self.n_p, -1).to(device=self.w.device, dtype=self.w.dtype).contiguous()
            w = src.view(self.n_p // 32, 2, 16, 3, 3, self.cin_p // ck, ck // 32, 4, 8)   # nb, cb, r16, dy, dx, chunk, k32, q4, j
            self._frag[key] = w.permute(0, 5, 4, 6, 3, 1, 7, 2, 8).contiguous()
        return self._frag[key]

    def frag_skip(self) -> torch.Tensor:
        """A 1x1 (two-source) skip convolution's weights for the skip segment of the weights-direct conv3x3 (csrc/conv_wd.hip, pmi_conv3x3_skip):
        the centre tap only, k = the concatenated channel index, in the 16x16x32 fragment order of frag16 without its tap dimensions:
        [N/32][K/32][16-channel block][lane = 16*(k quarter) + channel][8 k] -- one order for both chunk sizes (ck = 32 / 64)."""
        if "skip" not in self._frag:
            assert self.taps == 1 and not self.split and self.n_p % 32 == 0 and self.K % 64 == 0
            w = self.w.view(self.n_p // 32, 2, 16, self.K // 32, 4, 8)        # nb, cb, r16, k32, q4, j
            self._frag["skip"] = w.permute(0, 3, 1, 4, 2, 5).contiguous()
        return self._frag["skip"]

    def frag_c8(self) -> torch.Tensor:
        """Fragment order for config 8 of the weights-direct kernel (at most 32 input channels): k = tap * Cin + c zero-padded to whole
        32-deep MFMA steps, [N/32][steps][16-channel block (2)][lane = 16*(k quarter) + channel][8 k]."""
        if "c8" not in self._frag:
            assert self.taps == 9 and self.n_p % 32 == 0 and self.cin_p % 8 == 0 and self.cin_p <= 32
            ks = (9 * self.cin_p + 31) // 32
            w = torch.zeros((self.n_p, ks * 32), dtype=self.w.dtype, device=self.w.device)
            w[:, :self.K] = self.w
            w = w.view(self.n_p // 32, 2, 16, ks, 4, 8)                       # nb, cb, r16, step, q4, j
            self._frag["c8"] = w.permute(0, 3, 1, 4, 2, 5).contiguous()
        return self._frag["c8"]

    def frag(self, ck: int) -> torch.Tensor:
        """The 3x3 weights in MFMA fragment order for the weights-direct kernel (csrc/conv_wd.hip):
        [N/32][Cin/ck][dx][ck/16][dy][lane = 32*(k half) + channel][8 k] -- every (n-block, chunk, dx, k-step, dy)
        fragment is one contiguous 1 KB piece and a wave's whole weight stream is contiguous in its loop order."""
        if ck not in self._frag:
            assert self.taps == 9 and self.n_p % 32 == 0 and self.cin_p % ck == 0
            w = self.w.view(self.n_p // 32, 32, 3, 3, self.cin_p // ck, ck // 16, 2, 8)   # nb, l31, dy, dx, chunk, ks, h, j
            self._frag[ck] = w.permute(0, 4, 3, 5, 2, 6, 1, 7).contiguous()
        return self._frag[ck]


class MixedLinear:
    """Both packings of one 3x3 convolution for the mixed mode (engine/adm_mixed.py), built on first use: `single` = plain f16 weights over the
    logical channels (the operand act(GroupNorm(hi + lo)) is rounded once to f16), `dbl` = weights duplicated along K for the hi + lo operand
    (also what the generic fallback path takes)."""

    def __init__(self, weight, bias, device, sources=None, cin_pad=None):
        self._args = (weight, bias, device, sources, cin_pad)
        self._single = self._dbl = None

    @property
    def single(self) -> PackedLinear:
        if self._single is None:
            w, b, dev, _, cp = self._args
            self._single = PackedLinear(w, b, _hip.DT_F16, dev, cin_pad=cp)
        return self._single

    @property
    def dbl(self) -> PackedLinear:
        if self._dbl is None:
            w, b, dev, src, cp = self._args
            self._dbl = PackedLinear(w, b, DT_F16X2, dev, cin_pad=cp, sources=src, concat_sources=False)
        return self._dbl


def fused_skip_bias(conv: PackedLinear, skip: PackedLinear) -> torch.Tensor:
    """Bias table of the fused conv2 + skip launch: the two layers' biases added once, in fp32, when the weights are packed."""
    assert conv.n_p == skip.n_p
    b = torch.zeros(conv.n_p, dtype=torch.float32, device=conv.w.device)
    for lin in (conv, skip):
        if lin.b is not None:
            b += lin.b
    return b


# ---- input gradients: dX of a convolution is the forward kernel on transposed + flipped weights -------------------------------------
def packed_dx(cache: dict, key: str, weight: torch.Tensor, dt: int, device, cin_pad: Optional[int] = None,
              rows: Optional[int] = None) -> PackedLinear:
    """Packed weights of the input-gradient convolution of `weight` ([Cout, Cin] linear, [Cout, Cin, 1] Conv1d or [Cout, Cin, k, k]):
    [Cin, Cout, k, k] with both taps flipped, built once and kept in cache[key].  rows: zero-pad its output channels (the forward's
    zero-padded input channels) to this count."""
    if key not in cache:
        wt = weight.detach().cpu().float()
        if wt.ndim == 3:
            wt = wt[..., None]
        elif wt.ndim == 2:
            wt = wt[:, :, None, None]
        wt = wt.permute(1, 0, 2, 3).flip(2, 3)
        if rows is not None and rows > wt.shape[0]:
            wt = torch.cat([wt, wt.new_zeros((rows - wt.shape[0],) + tuple(wt.shape[1:]))], 0)
        cache[key] = PackedLinear(wt.contiguous(), None, dt, device, cin_pad=cin_pad)
    return cache[key]


def f16_grad_scale(amax) -> float:
    """Power of two that keeps an f16 gradient in range, from the per-sample max |d_out|: 2**clamp(-ceil(log2(max)), -24, 24) in float64
    (the largest value lands in (0.5, 1]; a power of two is exact), 1.0 when every sample is zero or any holds a NaN or an inf."""
    amax = [float(a) for a in amax]
    m = max(amax, default=0.0)
    if not all(math.isfinite(a) for a in amax) or m <= 0.0:
        return 1.0
    return 2.0 ** max(-24, min(24, -math.ceil(math.log2(m))))


def grad_to_nhwc(d_out: torch.Tensor, dt: int, device, cpad: int = 8, mul: float = 1.0):
    """d loss / d output (NCHW fp32, any device) -> (NHWC 16-bit [N, H, W, cpad] = d_out * mul * scale, scale).  f16 scales by
    f16_grad_scale (image gradients of a CLIP loss are ~1e-6 and would flush to zero in f16); bf16 needs no scaling.  precise: a split
    [N, H, W, 2 cpad] tensor with the same scale -- hi + lo has f16's exponent range, and keeps its ~22 bits only while lo is a normal f16."""
    d = d_out.to(device=device, dtype=torch.float32).contiguous()
    n, c, h, w = d.shape
    scale = 1.0
    if dt in (_hip.DT_F16, DT_F16X2):
        amax = _empty((n,), torch.float32, device)
        call("pmi_quantile_abs", ptr(d), ptr(amax), n, c * h * w, 1.0)
        scale = f16_grad_scale(amax.tolist())
    g = _empty((n, h, w, 2 * cpad if dt == DT_F16X2 else cpad), _hip.TORCH_DTYPE[dt], device)
    call("pmi_nchw_to_nhwc", ptr(d), ptr(g), n, c, h, w, cpad, mul * scale, 0.0, dt)
    return g, scale


def grad_to_nchw(g: torch.Tensor, c: int, mul: float) -> torch.Tensor:
    """The first c channels of an fp32 NHWC gradient [N, H, W, >= c] as NCHW fp32, times mul (undoing the input scale)."""
    n, h, w, _ = g.shape
    out = _empty((n, c, h, w), torch.float32, g.device)
    call("pmi_nhwc_to_nchw", ptr(g), g.shape[-1], ptr(out), n, h, w, c, mul, 0.0)
    return out


def add2(a: torch.Tensor, b: torch.Tensor, dt: int) -> torch.Tensor:
    """a + b of two activation-shaped tensors (two gradients of a value consumed twice, main + skip of a block); precise: the sum of the two
    hi + lo values in fp32, split again."""
    out = torch.empty_like(a)
    if dt == DT_F16X2:
        call("pmi_split_add", ptr(a), ptr(b), ptr(out), a.numel() // a.shape[-1], a.shape[-1] // 2)
    else:
        call("pmi_add16", ptr(a), ptr(b), ptr(out), a.numel(), dt)
    return out


def view_nhwc(y: torch.Tensor, n: int, h: int, w: int) -> torch.Tensor:
    """[N*H*W, C] as [N, H, W, C], keeping the GroupNorm statistics its producer left behind (_pmi_stats)."""
    v = y.view(n, h, w, y.shape[-1])
    if hasattr(y, "_pmi_stats"):
        v._pmi_stats = y._pmi_stats
    return v


def split_convert(x: torch.Tensor, to_split: bool) -> torch.Tensor:
    """plain f16 [..., C] <-> split (hi + lo) [..., 2C] (pmi_split_convert): the level boundaries of the mixed mode."""
    c = x.shape[-1] if to_split else x.shape[-1] // 2
    y = _empty(x.shape[:-1] + ((2 * c) if to_split else c,), torch.float16, x.device)
    call("pmi_split_convert", ptr(x), ptr(y), x.numel() // x.shape[-1], c, int(to_split))
    return y


MIXED_TRACE = None      # tools / tests: list collecting (route, operand, shape) of every conv3x3_mixed call
_MARK = 1               # a pointer that is not there yet in a host query (_as_if): the C ABI tests such fields against NULL only


def _igemm_args(lin: PackedLinear, m: int, a0: Optional[torch.Tensor] = None, a1: Optional[torch.Tensor] = None, c0: Optional[int] = None,
                c1: int = 0, *, out=None, residual=None, nbias=None, grid=None, hw: int = 1, stride: int = 1, up: int = 0, res_up: bool = False,
                act: int = ACT_NONE, alpha: float = 1.0, split_out: int = 0) -> IgemmArgs:
    """What the tensors and the geometry give of a pmi_igemm call of m rows through `lin` (shapes, pitches, pointers, types): no library query, no
    routing field.  c0 / c1: channels of a0 / a1 as the kernel counts them; grid = (H, W, Hin, Win).  Without tensors: a plain GEMM on dense rows of lin's
    own K, the probe geglu_linear and fused_mlp_epilogues ask about.  (Fields that stay zero are not written: this runs for every launch.)"""
    a = IgemmArgs()
    a.M, a.N, a.K, a.ldb, a.hw, a.batch, a.batch_inner, a.dtype = m, lin.n_p, lin.K, lin.K, hw, 1, 1, lin.dt
    a.taps, a.stride, a.alpha = lin.taps, stride, alpha
    if up or res_up or act:
        a.up, a.res_up, a.act = int(up), int(res_up), act
    if lin.split or split_out:
        a.split_in, a.split_out = int(lin.split), split_out
    if grid is not None:
        a.H, a.W, a.Hin, a.Win = grid
    if a0 is not None:
        a.A0, a.C0, a.lda0, a.B, a.bias = ptr(a0), c0, a0.stride(-2), ptr(lin.w), ptr(lin.b)
    else:
        a.C0, a.lda0 = lin.K, lin.K
    if a1 is not None:
        a.A1, a.C1, a.lda1 = ptr(a1), c1, a1.stride(-2)
    if out is not None:
        a.D, a.ldd = ptr(out), out.stride(-2)
        if out.dtype is torch.float32:
            a.out_f32 = 1
    else:
        a.ldd = lin.n_p
    if residual is not None:
        a.R, a.ldr = ptr(residual), residual.stride(-2)
        if residual.dtype is torch.float32:
            a.res_f32 = 1
    if nbias is not None:
        a.nbias, a.ldnb = ptr(nbias), nbias.stride(0)
    return a


def _as_if(query, ref, *more, Bf=_MARK, **fields) -> int:
    """query(ref, *more) as if fragment-ordered weights were offered (Bf) and `fields` were set -- the one place that writes markers: the library reads a
    pointer of a query as "this operand will be there" (pro_a: a fused prologue, D2: a second output).  The struct comes back as it was found."""
    a = ref._obj
    old_bf, old = a.Bf, [getattr(a, f) for f in fields] if fields else ()
    a.Bf = Bf
    for f, v in fields.items():
        setattr(a, f, v)
    try:
        return query(ref, *more)
    finally:
        a.Bf = old_bf
        for f, v in zip(fields, old):
            setattr(a, f, v)


def _timed(name: str, args):          # one library call between two events on the launch stream: (e0, e1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    call(name, *args)
    e1.record()
    return e0, e1


def _traced_call(name: str, args, desc: str, flops: float) -> None:
    """One library call between two events, appended to GEMM_TRACE as (desc, flops, ev0, ev1)."""
    GEMM_TRACE.append((desc, flops) + _timed(name, args))


def _launch(name: str, *args, events=None, trace=None) -> None:
    """The one launch seam: events = (flops, bytes, desc): timed into KERNEL_EVENTS as (e0, e1, flops, bytes, desc); trace = (desc, flops): into GEMM_TRACE."""
    if events is None and trace is None:
        call(name, *args)
    elif events is not None:
        KERNEL_EVENTS.append(_timed(name, args) + events)
    else:
        _traced_call(name, args, *trace)


def _stats_buffer(a: IgemmArgs, out: torch.Tensor, n: int, rows: int, cols: int) -> None:
    if rows > 0:       # the launch leaves per-channel (sum, sumsq) partials of its output for the next GroupNorm, kept on the output as _pmi_stats
        st = _empty((n, rows, cols, 2), torch.float32, out.device)
        a.stats, a.stats_p = ptr(st), rows
        out._pmi_stats = (st, rows)


def conv3x3_mixed(x: torch.Tensor, mlin: MixedLinear, *, operand: str, prologue, x1: Optional[torch.Tensor] = None, up: bool = False,
                  residual: Optional[torch.Tensor] = None, res_up: bool = False, nbias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Stride-1 3x3 convolution of the mixed mode: x (and x1: skip-concat) are split tensors [N, H, W, 2C]; prologue = (coef_a, coef_b, act) is
    the fused GroupNorm-apply + SiLU of the input; operand "single": the activated value is rounded once to f16 (K = 9 Cin), "dbl": it is
    kept as hi + lo (K = 18 Cin, fp32-grade product).  Split output [N, H, W, 2 Cout] with fused statistics; split residual.
    Shapes the weights-direct kernel does not take fall back to apply pass + generic split convolution (always the doubled operand)."""
    assert operand in ("single", "dbl")
    n, hin, win, _ = x.shape
    h, w = (hin * 2, win * 2) if up else (hin, win)
    ca, cb, pact = prologue
    lin = mlin.single if operand == "single" else mlin.dbl
    div = 2 if operand == "single" else 1                  # single: C0 / C1 / K count logical channels
    c0, c1 = x.shape[-1] // div, (x1.shape[-1] // div if x1 is not None else 0)
    m = n * h * w
    a = _igemm_args(lin, m, x, x1, c0, c1, residual=residual, nbias=nbias, grid=(h, w, hin, win), hw=h * w, up=up, res_up=res_up, split_out=32)
    a.dtype, a.split_in = DT_F16X2, (2 if operand == "single" else 1)     # split tensors whatever the weights' type (an fp32 residual: the same bytes as a split one)
    a.pro_act = pact
    ref, lib = C.byref(a), _hip.lib()
    cfg = -1
    if lin.n_p % 128 == 0 and lin.K == 9 * (c0 + c1) and HALO_ENABLED:
        cfg = _as_if(lib.pmi_conv3x3_halo_config, ref, pro_a=_MARK, pro_b=_MARK)
    if MIXED_TRACE is not None:
        MIXED_TRACE.append(("wd" if cfg >= 6 else "fallback", operand, (n, h, w, c0 + c1, lin.cout)))
    if cfg < 6:
        if residual is not None and residual.dtype == torch.float32:      # the generic split epilogue reads a split residual
            rs = _empty(residual.shape[:-1] + (2 * residual.shape[-1],), torch.float16, x.device)
            call("pmi_split_from_f32", ptr(residual), residual.stride(-2), ptr(rs), residual.numel() // residual.shape[-1], residual.shape[-1])
            residual = rs
        return igemm(x, mlin.dbl, a1=x1, up=up, residual=residual, res_up=res_up, nbias=nbias, prologue=prologue, want_stats=True)
    ck = 64 if cfg == 6 else 32
    a.Bf = ptr(lin.frag16(ck) if operand == "single" else lin.frag16(ck, dup_g=ck // 2))
    a.pro_a, a.pro_b = ptr(ca), ptr(cb)
    out = _empty((n, h, w, 2 * lin.n_p), torch.float16, x.device)
    a.D, a.ldd = ptr(out), out.stride(-2)
    _stats_buffer(a, out, n, lib.pmi_igemm_stats_rows(ref), lin.n_p)
    if DEBUG_WS is not None:
        a.ws = ptr(DEBUG_WS)
        a.reserved = 77
    events = None
    if KERNEL_EVENTS is not None:
        nbytes = (x.numel() + (x1.numel() if x1 is not None else 0)) * 2 + lin.w.numel() * 2 + out.numel() * 2 + (residual.numel() * 2 if residual is not None else 0)
        events = (2.0 * m * lin.cout * lin.cin * 9, float(nbytes), f"{h}x{w} {c0}+{c1}->{lin.cout} cfg{cfg} mixed-{operand}")
    _launch("pmi_igemm", ref, events=events)
    return out


def _wd_tile_desc(a: IgemmArgs) -> str:
    """GEMM_TRACE: the tile details the weights-direct GEMM's instantiations differ in (rows x columns per workgroup, two-source K, conv mode,
    gated epilogue), as pmi_gemm_wd_tile reports them for the arguments of the launch."""
    t = _hip.lib().pmi_gemm_wd_tile(C.byref(a))
    return f" rows={t // 1000} cols={t % 1000}{' two' if a.A1 else ''}{' convmode' if a.taps == 9 else ''}{' geglu' if a.act == ACT_GEGLU else ''}"


_CONV_PACKING = {4: lambda lin: lin.frag(64), 6: lambda lin: lin.frag16(64), 7: lambda lin: lin.frag16(32), 8: lambda lin: lin.frag_c8(),
                 9: lambda lin: lin.frag16_up(64)}     # the weight order each weights-direct 3x3 tile config reads through Bf (the others: lin.w)


def igemm(a0: torch.Tensor, lin: PackedLinear, *, a1: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
          act: int = ACT_NONE, up: bool = False, stride: int = 1, res_up: bool = False, nbias: Optional[torch.Tensor] = None,
          out_f32: bool = False, out: Optional[torch.Tensor] = None, alpha: float = 1.0, prologue=None,
          want_stats: bool = False, hw: Optional[int] = None, pre_out: Optional[torch.Tensor] = None,
          act_grad_of: Optional[torch.Tensor] = None, act_grad: int = ACT_NONE, defer_reduce: bool = False,
          split_out: bool = False, skip=None) -> torch.Tensor:
    """Convolution (a0 is [N,H,W,C]) or linear (a0 is [M,C]) through pmi_igemm.

    skip = (skip_lin, x0, x1, bias): a ResBlock's conv2 whose residual is the 1x1 convolution skip_lin over x0 | x1 (x1 may be None);
    bias = fused_skip_bias(lin, skip_lin).  Where pmi_conv3x3_skip takes the shape the product is accumulated inside this launch; otherwise
    the skip GEMM runs on its own and its output is the residual, as without the argument.

    prologue = (coef_a [N,Cin], coef_b [N,Cin], act): fused GroupNorm-apply(+FiLM)+activation on the conv input
    (LDS-halo conv3x3 kernel only); when the shape is not eligible the apply kernel runs first.
    pre_out: 16-bit tensor like the output that receives the PRE-activation value (fused act epilogue keeps the backward's input);
    act_grad_of / act_grad: the output is multiplied by act'(act_grad_of) -- both only where fused_mlp_epilogues(lin) is True."""
    # ---- 1. geometry and arguments: no library query ----
    dt, conv = lin.dt, a0.ndim == 4
    if lin.concat_inputs and a1 is not None and prologue is None:
        # (a prologue materialises one applied tensor from both sources below: no copy needed there)
        a0, a1 = torch.cat([a0, a1], dim=-1), None
    c0, c1 = a0.shape[-1], (a1.shape[-1] if a1 is not None else 0)
    assert (c0 + c1) * (2 if lin.self_concat else 1) == lin.cin_p, (c0, c1, lin.cin_p)
    if conv:
        n, hin, win, _ = a0.shape
        hv, wv = (hin * 2, win * 2) if up else (hin, win)
        h, w = hv // stride, wv // stride
        m, grid, hw = n * h * w, (h, w, hin, win), h * w
        oshape = (n, h, w, lin.n_p)
    else:
        assert lin.taps == 1 and not up and stride == 1
        m, grid, hw = a0.shape[0], None, hw or 1
        oshape = (m, lin.n_p // 2 if act == ACT_GEGLU else lin.n_p)
    so = split_group(lin.n_p) if (lin.split and not out_f32) or split_out else 0
    if so:     # precise output: hi + lo pairs, 2*N 16-bit values per row (split_out: from plain f16 operands too -- the mixed mode's attention
        oshape = oshape[:-1] + (2 * lin.n_p,)             # projection back onto a split stream)
    if out is None:
        out = _empty(oshape, torch.float32 if out_f32 else _hip.TORCH_DTYPE[dt], a0.device)
    a = _igemm_args(lin, m, a0, a1, c0, c1, out=out, residual=residual, nbias=nbias, grid=grid, hw=hw, stride=stride, up=up, res_up=res_up, act=act,
                    alpha=alpha, split_out=so)
    if pre_out is not None or act_grad_of is not None:
        a.D2, a.aux, a.aux_act = ptr(pre_out), ptr(act_grad_of), act_grad
    ref, lib, packed, cfg = C.byref(a), _hip.lib(), False, -1          # packed: Bf holds a weight order (steps 2, 3, 4, 7)
    # ---- 2. 3x3 tile config and its packing, asked BEFORE the steps below change the struct: pmi_igemm chooses again from the struct as launched ----
    if conv and lin.taps == 9 and stride == 1 and HALO_ENABLED and lin.n_p % 32 == 0 and ((lin.n_p >= 128 and lin.cin_p % 64 == 0) or (lin.cin_p <= 32 and a1 is None)):
        if up and lin.frag16_up(64) is None:
            a.reserved3 = 2            # no phase weights: the up-sampling convolution stays on the gather route (config 9 needs them); stays set for the launch
        if prologue is not None and not lin.split:         # (the table size limit depends on a fused prologue)
            cfg = _as_if(lib.pmi_conv3x3_halo_config, ref, pro_a=_MARK)
        else:
            cfg = _as_if(lib.pmi_conv3x3_halo_config, ref)
        if cfg in _CONV_PACKING:
            a.Bf, packed = ptr(_CONV_PACKING[cfg](lin)), True
    # ---- 3. weights-direct GEMM (csrc/gemm_wd.hip) for a plain GEMM (split weights: their duplicated K is an ordinary K; its epilogues write plain 16-bit or fp32 rows only) ----
    wd = GEMM_WD_ENABLED and lin.taps == 1 and (not lin.split or out_f32) and not up and stride == 1 and lin.n_p % 32 == 0 and lin.K % 32 == 0 \
        and nbias is None and prologue is None
    if wd and want_stats:
        # the weights-direct GEMM has no statistics epilogue; the generic kernel has none either once it splits K (attention proj_out on
        # 16x16 / 8x8 maps): then the faster GEMM runs and the consumer's GroupNorm takes its statistics pass as before
        wd = SPLITK_ENABLED and lib.pmi_igemm_splitk(ref) > 1          # (asked without Bf: the GENERIC kernel's split rule)
    if wd:                                     # ask whether the kernel takes this shape, and only then pack its weight order
        wd = bool(_as_if(lib.pmi_gemm_wd_eligible, ref))
        if wd:
            a.Bf, packed, want_stats = ptr(lin.frag_gemm()), True, False
    # ---- 4. a ResBlock's skip convolution: inside this launch (pmi_conv3x3_skip), or its own GEMM whose output is the residual ----
    fcfg = 0
    if skip is not None:
        slin, s0, s1, sbias = skip
        assert residual is None and conv and prologue is not None
        if act == ACT_NONE and a1 is None and HALO_ENABLED and not lin.split and not slin.split and slin.taps == 1 and slin.n_p == lin.n_p \
                and lin.n_p % 128 == 0 and lin.cin_p % 64 == 0 and slin.K % 64 == 0:
            k = SkipArgs()
            k.X0, k.X1, k.Wf = ptr(s0), ptr(s1), ptr(slin.frag_skip())
            k.C0, k.C1 = s0.shape[-1], (s1.shape[-1] if s1 is not None else 0)
            k.ld0, k.ld1 = s0.stride(-2), (s1.stride(-2) if s1 is not None else 0)
            fcfg = _as_if(lib.pmi_conv3x3_skip_eligible, ref, C.byref(k), Bf=ptr(lin.w), bias=ptr(sbias), pro_a=ptr(prologue[0]),
                          pro_b=ptr(prologue[1]), pro_act=prologue[2])     # (Bf: any 16-byte aligned pointer; the config names the packing)
        if fcfg in (6, 7):
            a.Bf, a.bias, packed = ptr(lin.frag16(64 if fcfg == 6 else 32)), ptr(sbias), True
        else:
            residual = igemm(s0, slin, a1=s1)
            a.R, a.ldr, a.res_f32 = ptr(residual), residual.stride(-2), 0
    fused_skip = fcfg in (6, 7)
    # ---- 5. prologue: fused where a 3x3 tile config takes the struct as it stands (Bf from step 2, no pro_a marker), else the apply pass ----
    fused_pro = False
    if prologue is not None:
        ca, cb, pact = prologue
        fused_pro = fused_skip or (HALO_ENABLED and not lin.split and lib.pmi_conv3x3_halo_config(ref) >= 0)
        if fused_pro:
            a.pro_a, a.pro_b, a.pro_act = ptr(ca), ptr(cb), pact
        else:   # not eligible: materialise act(x*a+b) with the streaming kernel, then convolve
            if lin.split and a1 is not None and (c0 // 2) % 32 + (c1 // 2) % 32:
                # the applied tensor is ONE precise tensor grouped by split_group(C0 + C1); weights duplicated per source match it only
                # when both sources are grouped by 32 as well
                raise ValueError(f"precise two-source prologue: sources of {c0 // 2} + {c1 // 2} channels are not both multiples of 32")
            n_, h_, w_, _ = a0.shape
            y = _empty((n_, h_, w_, c0 + c1), a0.dtype, a0.device)
            lc0, lc = (c0 // 2, (c0 + c1) // 2) if lin.split else (c0, c0 + c1)       # logical channel counts
            call("pmi_gn_apply", ptr(a0), ptr(a1), lc0, ptr(ca), ptr(cb), None, ptr(y), n_, h_, w_, lc, pact, 0, dt)
            a.A0, a.A1, a.C0, a.C1, a.lda0, a.lda1 = ptr(y), None, c0 + c1, 0, c0 + c1, 0
            a0 = y
    # ---- 6. self_concat (precise mode, fp32 weights): their low part multiplies the SAME input again as a second source ----
    if lin.self_concat:
        assert a.A1 is None
        a.A1, a.C1, a.lda1 = a.A0, a.C0, a.lda0
    # ---- 7. a 3x3 convolution the conv3x3 kernels do not take (16x16 / 8x8 maps): the weights-direct GEMM's conv mode, if it does ----
    conv_gemm = False
    if conv and lin.taps == 9 and stride == 1 and not up and GEMM_WD_ENABLED and GEMM_WD_CONV and not lin.split and not packed \
            and not fused_pro and lin.n_p % 32 == 0 and c0 % 128 == 0 and c1 % 128 == 0:
        conv_gemm = bool(_as_if(lib.pmi_gemm_wd_eligible, ref))
        if conv_gemm:
            a.Bf = ptr(lin.frag_gemm())
    # ---- 8. split-K: few output tiles, long K -- the reduction over grid.z into fp32 slabs (asked with the Bf of steps 2 / 3 / 7) ----
    sk = 0
    if SPLITK_ENABLED and not fused_skip:
        sk = lib.pmi_igemm_splitk(ref)
        if sk > 1:
            ws = _empty((sk, m, lin.n_p), torch.float32, a0.device)
            a.ws, a.splitk = ptr(ws), sk
            if defer_reduce and packed and not conv and lib.pmi_gemm_wd_eligible(ref):
                # the caller fuses the reduction (+ bias / residual) into its next pass (LayerNorm): leave the raw slabs
                a.reserved3 = 1
                _launch("pmi_igemm", ref, trace=None if GEMM_TRACE is None else
                        (f"gemm M={m} N={lin.n_p} K={lin.K} taps=1 splitk={sk} halo=-1 wd=1{_wd_tile_desc(a)} defer", 2.0 * m * lin.n_p * lin.K))
                return ("slabs", ws, sk)
    if conv_gemm and (nbias is not None or res_up) and sk <= 1:
        a.Bf, conv_gemm = None, False      # a per-sample bias / up-sampled residual is the split-K reduce kernel's: unsplit, the generic kernel takes the call (sk: asked with Bf set)
    # ---- 9. statistics: fused per-channel (sum, sumsq) of the output for the next GroupNorm ----
    if want_stats:
        _stats_buffer(a, out, m // hw, (h // 8) * (w // 32) if fused_skip else lib.pmi_igemm_stats_rows(ref), lin.n_p)
    if DEBUG_WS is not None and sk <= 1:      # (a split-K call's ws is its slab workspace: the phase stamps of the probes are for unsplit calls only)
        a.ws = ptr(DEBUG_WS)
        a.reserved = 77
    # ---- 10. launch; instrumented: a 3x3 launch on a tile config goes to KERNEL_EVENTS when that is on, otherwise to GEMM_TRACE ----
    events = trace = None
    if KERNEL_EVENTS is not None or GEMM_TRACE is not None:
        # what pmi_igemm itself computes from the struct as launched is what is printed: its tile config here, its weights-direct GEMM test below
        tile = fcfg if fused_skip else lib.pmi_conv3x3_halo_config(ref) if (HALO_ENABLED and lin.taps == 9) else -1
        if KERNEL_EVENTS is not None and tile >= 0:
            # algorithmic HBM bytes: input read once, packed weights, output written once, residual read once; a fused skip adds its product's FLOP, its two sources and its weights
            nbytes = (a0.numel() + (a1.numel() if a1 is not None else 0)) * 2 + lin.w.numel() * 2 + out.numel() * out.element_size() \
                + (residual.numel() * residual.element_size() if residual is not None else 0)
            if fused_skip:
                nbytes += (s0.numel() + (s1.numel() if s1 is not None else 0)) * 2 + slin.w.numel() * 2
            desc = f"{h}x{w} {c0}+{c1}->{lin.cout} cfg{tile}{' pro' if prologue is not None else ''}{' res' if residual is not None else ''}" \
                   f"{' up' if up else ''}{f' skip {k.C0}+{k.C1}' if fused_skip else ''}{' stats' if want_stats else ''}"
            events = (2.0 * m * lin.cout * (lin.cin * lin.taps + (slin.cin if fused_skip else 0)), float(nbytes), desc)
        elif GEMM_TRACE is not None and fused_skip:
            trace = (f"conv M={m} N={lin.n_p} K={lin.K} taps=9 splitk=0 halo={tile} wd=0{' stats' if a.stats else ''} skip={k.C0}+{k.C1}",
                     2.0 * m * lin.n_p * (lin.K + slin.K))
        elif GEMM_TRACE is not None:
            kind = "conv" if conv and (lin.taps == 9 or up or stride == 2) else "gemm"
            # (not the locals of steps 3 / 7: statistics attached in step 9 make pmi_igemm refuse the weights-direct GEMM and ignore Bf)
            wd = bool(a.Bf) and bool(lib.pmi_gemm_wd_eligible(ref))
            desc = f"{kind} M={m} N={lin.n_p} K={lin.K} taps={lin.taps}{' up' if up else ''}{' s2' if stride == 2 else ''} splitk={a.splitk} halo={tile} wd={int(wd)}" \
                   f"{' res' if residual is not None else ''}{' f32out' if a.out_f32 else ''}{' nbias' if nbias is not None else ''}{' stats' if a.stats else ''}" \
                   f"{' split_in' if a.split_in else ''}{' split_out' if a.split_out else ''}{' self_concat' if lin.self_concat else ''}" \
                   f"{_wd_tile_desc(a) if wd else ''}"
            trace = (desc, 2.0 * m * lin.n_p * lin.K)
    if fused_skip:
        _launch("pmi_conv3x3_skip", ref, C.byref(k), events=events, trace=trace)
    else:
        _launch("pmi_igemm", ref, events=events, trace=trace)
    return out


def downsample_adjoint_args(g: torch.Tensor, lin: PackedLinear, out: torch.Tensor) -> IgemmArgs:
    """pmi_igemm's phased geometry (taps 9, stride 2, up 2) for g [N, h, w, C] -> out [N, 2h, 2w, C']: H x W is the output grid, Hin x Win the
    gradient's, M counts output pixels (a quarter of them per phase)."""
    n, h, w, c = g.shape
    a = _igemm_args(lin, 4 * n * h * w, g, None, c, out=out, grid=(2 * h, 2 * w, h, w), hw=4 * h * w, stride=2, up=2)
    a.bias = None          # (a gradient takes no bias)
    return a


def downsample_adjoint(g: torch.Tensor, lin: PackedLinear, *, out_f32: bool = False, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Input gradient of Downsample2D (pad right / bottom by one, 3x3 stride-2 convolution without padding) in one launch: g [N, h, w, C]
    is the gradient wrt its output, `lin` the phase-packed weights (engine/sd.py: pack_downsample_adjoint_weights), the result
    [N, 2h, 2w, C'] the gradient wrt its input.  Every output phase gathers only the taps that reach it -- no zero-inserted
    [N, 2h, 2w, C] buffer and a quarter of the MFMA work of a 3x3 pass over one."""
    n, h, w, c = g.shape
    assert lin.taps == 9 and not lin.split and c == lin.cin_p, (lin.taps, c, lin.cin_p)
    if out is None:
        out = _empty((n, 2 * h, 2 * w, lin.n_p), torch.float32 if out_f32 else _hip.TORCH_DTYPE[lin.dt], g.device)
    call("pmi_igemm", C.byref(downsample_adjoint_args(g, lin, out)))
    return out


def geglu_linear(x: torch.Tensor, lin: PackedLinear) -> torch.Tensor:
    """x [M, K] @ lin (columns packed as 16 value | 16 gate per 32: interleave_geglu) -> value * gelu(gate) [M, N / 2].
    In the GEMM's epilogue where the weights-direct kernel takes the shape; otherwise the GEMM followed by the gate pass."""
    if GEMM_WD_ENABLED and not lin.split and lin.n_p % 32 == 0 and lin.K % 32 == 0 \
            and _as_if(_hip.lib().pmi_gemm_wd_eligible, C.byref(_igemm_args(lin, x.shape[0], act=ACT_GEGLU))):
        return igemm(x, lin, act=ACT_GEGLU)
    f = igemm(x, lin)
    out = _empty((x.shape[0], lin.n_p // 2), f.dtype, f.device)
    call("pmi_geglu", ptr(f), ptr(out), x.shape[0], lin.n_p // 2, 1, lin.dt)
    return out


def interleave_geglu(weight: torch.Tensor, bias: Optional[torch.Tensor]):
    """Rows of a GEGLU projection [2F, K] = (value F | gate F) reordered to 16 value rows, their 16 gate rows, 16 value rows, ...
    (every 32-column slice a wave of the weights-direct GEMM owns then holds matching value / gate columns)."""
    f = weight.shape[0] // 2
    assert f % 16 == 0
    idx = torch.arange(f).view(-1, 16)
    perm = torch.cat([idx, idx + f], dim=1).flatten()
    return weight[perm].contiguous(), (bias[perm].contiguous() if bias is not None else None)


def fused_mlp_epilogues(lin: PackedLinear, m: int) -> bool:
    """True when a plain 16-bit-output GEMM of m rows with these weights runs in the weights-direct kernel UNSPLIT, whose epilogue can also
    write the pre-activation value (pre_out) and multiply by an activation gradient (act_grad_of).  The library decides (its split-K cost
    model and A/B options included): pmi_igemm rejects D2 / aux on any other route."""
    # the structural part keeps the choice independent of the batch a rank holds (fused and unfused epilogues round differently: a shard must
    # reproduce its slice of the full-batch gradient, tests/test_gpu_clip.py): wide layers only, any m a ViT batch produces.  The m >= 64
    # floor and the split-K query below still follow m: a shard that crosses either (widths 512 / 768, m = 68 -> 34 in
    # tests/test_gpu_vit_tower.py) equals its slice to 16-bit rounding, not bit for bit
    if not (GEMM_WD_ENABLED and lin.taps == 1 and not lin.split and lin.n_p % 256 == 0 and lin.K % 128 == 0 and m >= 64):
        return False
    ref, lib = C.byref(_igemm_args(lin, m)), _hip.lib()
    if SPLITK_ENABLED and _as_if(lib.pmi_igemm_splitk, ref, D2=_MARK) > 1:       # (D2: asked for a call WITH the second output)
        return False
    return bool(_as_if(lib.pmi_gemm_wd_eligible, ref, D2=_MARK))


def bgemm(A: torch.Tensor, B: torch.Tensor, D: torch.Tensor, *, M: int, N: int, K: int, lda: int, ldb: int, ldd: int,
          batch: int, batch_inner: int, sA, sB, sD, dt: int, alpha: float = 1.0, a_off: int = 0, b_off: int = 0, d_off: int = 0):
    """Batched D[z] = alpha * A[z] @ B[z]^T with two-level (outer, inner) element strides."""
    a = IgemmArgs()
    es = A.element_size()
    a.A0 = A.data_ptr() + a_off * es
    a.B = B.data_ptr() + b_off * B.element_size()
    a.D = D.data_ptr() + d_off * D.element_size()
    a.M, a.N, a.K, a.C0 = M, N, K, K
    a.lda0, a.ldb, a.ldd = lda, ldb, ldd
    a.taps, a.stride, a.hw, a.alpha = 1, 1, 1, alpha
    a.out_f32 = int(D.dtype == torch.float32)
    a.batch, a.batch_inner = batch, batch_inner
    a.sA_o, a.sA_i = sA
    a.sB_o, a.sB_i = sB
    a.sD_o, a.sD_i = sD
    a.dtype = dt
    _launch("pmi_igemm", C.byref(a), trace=None if GEMM_TRACE is None else (f"bgemm M={M} N={N} K={K} batch={batch}", 2.0 * M * N * K * batch))
    return D


def group_norm_coeffs_train(x: torch.Tensor, gamma, beta, groups: int, dt: int, *, x1: Optional[torch.Tensor] = None,
                            film: Optional[torch.Tensor] = None, film_ld: int = 0, eps: float = 1e-5):
    """As group_norm_coeffs, also returning the per-channel (sum, sumsq) partials the coefficients came from, as the argument tuple
    (s0, P0, C0, s1, P1, C1) of pmi_gn_finalize / pmi_gn_bwd_finalize: the backward recomputes the forward moments from them."""
    n, h, w, _ = x.shape
    c0 = logical_c(x, dt)
    c1 = logical_c(x1, dt) if x1 is not None else 0
    c, hw, dev = c0 + c1, h * w, x.device
    ca, cb = _empty((n, c), torch.float32, dev), _empty((n, c), torch.float32, dev)
    st0 = getattr(x, "_pmi_stats", None)
    st1 = getattr(x1, "_pmi_stats", None) if x1 is not None else None
    if st0 is not None and (x1 is None or st1 is not None):
        # statistics came out of the producing kernels' epilogues: no pass over the activations at all
        parts = (st0[0], st0[1], c0, st1[0] if st1 else None, st1[1] if st1 else 0, c1)
    else:
        # pixel chunks per sample: ~1024 workgroups per launch, at least 8 pixels each (64 left a 16x16 map at batch 8 with 32 workgroups whose
        # threads walked 64 pixels one dependent load after the other: 27 us per launch)
        nchunk = max(1, min(hw // 8, (1024 + n - 1) // n))
        ws = _empty((n, nchunk, c, 2), torch.float32, dev)
        call("pmi_gn_stats", ptr(x), ptr(x1), c0, ptr(ws), n, hw, c, groups, nchunk, dt)
        parts = (ws, nchunk, c, None, 0, 0)
    call("pmi_gn_finalize", ptr(parts[0]), parts[1], parts[2], ptr(parts[3]), parts[4], parts[5], ptr(gamma), ptr(beta), ptr(film), film_ld,
         ptr(ca), ptr(cb), n, hw, groups, eps)
    return ca, cb, parts


def group_norm_backward(x: torch.Tensor, dy: torch.Tensor, ca, cb, parts, gamma, groups: int, dt: int, *, x1: Optional[torch.Tensor] = None,
                        film: Optional[torch.Tensor] = None, film_ld: int = 0, act: int = ACT_NONE, gadd0: Optional[torch.Tensor] = None,
                        gadd1: Optional[torch.Tensor] = None, eps: float = 1e-5):
    """Gradient wrt x (and x1) of y = act(GroupNorm(cat(x, x1)) * gamma [FiLM] + beta) given dy = d loss / d y [N, H, W, C] (one tensor over the
    concat) -- pmi_gn_bwd_stats / _finalize / _apply; gadd0 / gadd1: gradients arriving over another path, added on the way out.
    Returns (dx, dx1)."""
    n, h, w, _ = x.shape
    c0 = logical_c(x, dt)
    c1 = logical_c(x1, dt) if x1 is not None else 0
    c, hw, dev = c0 + c1, h * w, x.device
    split = dt == DT_F16X2
    assert logical_c(dy, dt) == c and dy.is_contiguous() and x.is_contiguous() and (x1 is None or x1.is_contiguous())
    nchunk = max(1, min(hw // 8, (1024 + n - 1) // n))
    wsb = _empty((n, nchunk, c, 2), torch.float32, dev)
    if split:
        call("pmi_split_gn_bwd_stats", ptr(x), ptr(x1), c0, ptr(dy), ptr(ca), ptr(cb), act, ptr(wsb), n, hw, c, nchunk)
    else:
        call("pmi_gn_bwd_stats", ptr(x), ptr(x1), c0, ptr(dy), ptr(ca), ptr(cb), act, ptr(wsb), n, hw, c, nchunk, dt)
    cp, cq = _empty((n, c), torch.float32, dev), _empty((n, c), torch.float32, dev)
    call("pmi_gn_bwd_finalize", ptr(parts[0]), parts[1], parts[2], ptr(parts[3]), parts[4], parts[5], ptr(wsb), nchunk, ptr(gamma), ptr(film), film_ld,
         ptr(cp), ptr(cq), n, hw, groups, eps)
    dx0 = torch.empty_like(x)
    dx1 = torch.empty_like(x1) if x1 is not None else None
    if split:
        call("pmi_split_gn_bwd_apply", ptr(x), ptr(x1), c0, ptr(dy), ptr(ca), ptr(cb), ptr(cp), ptr(cq), act, ptr(gadd0), ptr(gadd1), ptr(dx0),
             ptr(dx1), n, hw, c)
    else:
        call("pmi_gn_bwd_apply", ptr(x), ptr(x1), c0, ptr(dy), ptr(ca), ptr(cb), ptr(cp), ptr(cq), act, ptr(gadd0), ptr(gadd1), ptr(dx0), ptr(dx1),
             n, hw, c, dt)
    return dx0, dx1


def group_norm_coeffs(x: torch.Tensor, gamma, beta, groups: int, dt: int, *, x1: Optional[torch.Tensor] = None,
                      film: Optional[torch.Tensor] = None, film_ld: int = 0, eps: float = 1e-5):
    """Per-(sample, channel) coefficients (a, b) with norm(x)*gamma+beta[FiLM] = x*a+b (no apply pass)."""
    return group_norm_coeffs_train(x, gamma, beta, groups, dt, x1=x1, film=film, film_ld=film_ld, eps=eps)[:2]


def group_norm(x: torch.Tensor, gamma, beta, groups: int, dt: int, *, x1: Optional[torch.Tensor] = None,
               film: Optional[torch.Tensor] = None, film_ld: int = 0, residual: Optional[torch.Tensor] = None,
               act: int = ACT_NONE, pool: bool = False, eps: float = 1e-5) -> torch.Tensor:
    """GroupNorm over the channel-concat of x (and x1) -> act(norm * gamma + beta [FiLM]) [-> 2x2 avg pool] [+ residual]."""
    n, h, w, _ = x.shape
    c0 = logical_c(x, dt)
    c = c0 + (logical_c(x1, dt) if x1 is not None else 0)
    ca, cb = group_norm_coeffs(x, gamma, beta, groups, dt, x1=x1, film=film, film_ld=film_ld, eps=eps)
    cphys = 2 * c if dt == DT_F16X2 else c
    y = _empty((n, h // 2, w // 2, cphys) if pool else (n, h, w, cphys), x.dtype, x.device)
    call("pmi_gn_apply", ptr(x), ptr(x1), c0, ptr(ca), ptr(cb), ptr(residual), ptr(y), n, h, w, c, act, int(pool), dt)
    return y


def group_norm_pool_skip_train(x: torch.Tensor, gamma, beta, groups: int, dt: int, act: int = ACT_NONE, eps: float = 1e-5):
    """As group_norm_pool_skip, also returning the norm's (ca, cb, parts) of group_norm_coeffs_train."""
    n, h, w, _ = x.shape
    c = logical_c(x, dt)
    gn = group_norm_coeffs_train(x, gamma, beta, groups, dt, eps=eps)
    y = _empty((n, h // 2, w // 2, x.shape[-1]), x.dtype, x.device)
    y_raw = _empty((n, h // 2, w // 2, x.shape[-1]), x.dtype, x.device)
    call("pmi_gn_apply_pool_skip", ptr(x), ptr(gn[0]), ptr(gn[1]), ptr(y), ptr(y_raw), n, h, w, c, act, dt)
    return y, y_raw, gn


def group_norm_pool_skip(x: torch.Tensor, gamma, beta, groups: int, dt: int, act: int = ACT_NONE, eps: float = 1e-5):
    """(AvgPool2d(2)(act(GroupNorm(x))), AvgPool2d(2)(x)) from one pass over x: both inputs of a down ResBlock (unet.py:232-243)."""
    return group_norm_pool_skip_train(x, gamma, beta, groups, dt, act, eps)[:2]


def avgpool2(x: torch.Tensor, dt: int) -> torch.Tensor:
    n, h, w, c = x.shape
    y = _empty((n, h // 2, w // 2, c), x.dtype, x.device)
    call("pmi_avgpool2", ptr(x), ptr(y), n, h, w, logical_c(x, dt), dt)
    return y


def upsample_bilinear2(x: torch.Tensor, dt: int) -> torch.Tensor:
    n, h, w, c = x.shape
    y = _empty((n, h * 2, w * 2, c), x.dtype, x.device)
    call("pmi_upsample_bilinear2", ptr(x), ptr(y), n, h, w, logical_c(x, dt), dt)
    return y


def fir_down2(x: torch.Tensor, dt: int) -> torch.Tensor:
    """k-diffusion's Downsample2d("linear", reflect): [N, H, W, C] -> [N, H/2, W/2, C] (csrc/fir.hip)."""
    n, h, w, c = x.shape
    y = _empty((n, h // 2, w // 2, c), x.dtype, x.device)
    call("pmi_fir_down2", ptr(x), ptr(y), n, h, w, c, dt)
    return y


def fir_up2(x: torch.Tensor, dt: int) -> torch.Tensor:
    """k-diffusion's Upsample2d("linear", reflect): [N, H, W, C] -> [N, 2H, 2W, C] (csrc/fir.hip)."""
    n, h, w, c = x.shape
    y = _empty((n, h * 2, w * 2, c), x.dtype, x.device)
    call("pmi_fir_up2", ptr(x), ptr(y), n, h, w, c, dt)
    return y


def upsample_nearest2(x: torch.Tensor) -> torch.Tensor:
    n, h, w, c = x.shape
    y = _empty((n, h * 2, w * 2, c), x.dtype, x.device)
    call("pmi_upsample_nearest2", ptr(x), ptr(y), n, h, w, c)
    return y


def avgpool2_bwd(g: torch.Tensor, dt: int) -> torch.Tensor:
    """Adjoint of avgpool2: a quarter of each gradient value to each pixel of its 2x2 block, [N, H, W, C] -> [N, 2H, 2W, C]."""
    n, h, w, c = g.shape
    out = _empty((n, 2 * h, 2 * w, c), g.dtype, g.device)
    if dt == DT_F16X2:
        call("pmi_split_avgpool2_bwd", ptr(g), ptr(out), n, 2 * h, 2 * w, c // 2)
    else:
        call("pmi_avgpool2_bwd", ptr(g), ptr(out), n, 2 * h, 2 * w, c, dt)
    return out


def _up2_bwd(fn: str, fn_split: str, g: torch.Tensor, dt: int) -> torch.Tensor:
    n, h, w, c = g.shape
    out = _empty((n, h // 2, w // 2, c), g.dtype, g.device)
    if dt == DT_F16X2:
        call(fn_split, ptr(g), ptr(out), n, h // 2, w // 2, c // 2)
    else:
        call(fn, ptr(g), ptr(out), n, h // 2, w // 2, c, dt)
    return out


def upsample_nearest2_bwd(g: torch.Tensor, dt: int) -> torch.Tensor:
    """Adjoint of upsample_nearest2: the sum of each 2x2 block, [N, 2H, 2W, C] -> [N, H, W, C]."""
    return _up2_bwd("pmi_upsample_nearest2_bwd", "pmi_split_upsample_nearest2_bwd", g, dt)


def upsample_bilinear2_bwd(g: torch.Tensor, dt: int) -> torch.Tensor:
    """Adjoint of upsample_bilinear2, [N, 2H, 2W, C] -> [N, H, W, C]."""
    return _up2_bwd("pmi_upsample_bilinear2_bwd", "pmi_split_upsample_bilinear2_bwd", g, dt)


def fir_down2_bwd(g: torch.Tensor, dt: int) -> torch.Tensor:
    """Adjoint of fir_down2 (reflection folds included): [N, H/2, W/2, C] -> [N, H, W, C] (csrc/fir.hip)."""
    n, h, w, c = g.shape
    out = _empty((n, 2 * h, 2 * w, c), g.dtype, g.device)
    call("pmi_fir_down2_bwd", ptr(g), ptr(out), n, 2 * h, 2 * w, c, dt)
    return out


def fir_up2_bwd(g: torch.Tensor, dt: int) -> torch.Tensor:
    """Adjoint of fir_up2 (reflection folds included): [N, 2H, 2W, C] -> [N, H, W, C] (csrc/fir.hip)."""
    n, h, w, c = g.shape
    out = _empty((n, h // 2, w // 2, c), g.dtype, g.device)
    call("pmi_fir_up2_bwd", ptr(g), ptr(out), n, h // 2, w // 2, c, dt)
    return out


def edm_stage_out_bwd(d_denoised: torch.Tensor, sigma: torch.Tensor, sigma_data: float, scale: float, dt: int, cpad: int = 8) -> torch.Tensor:
    """Adjoint of pmi_edm_stage_out towards the network: d_denoised NCHW fp32 [N, 3, H, W] -> 16-bit NHWC [N, H, W, cpad] = scale * c_out * d."""
    n, _, h, w = d_denoised.shape
    g = _empty((n, h, w, cpad), _hip.TORCH_DTYPE[dt], d_denoised.device)
    call("pmi_edm_stage_out_bwd", ptr(d_denoised), ptr(sigma), sigma.numel(), sigma_data, scale, ptr(g), n, h, w, cpad, dt)
    return g


def edm_stage_in_bwd(d_denoised: torch.Tensor, gx: torch.Tensor, sigma: torch.Tensor, sigma_data: float, inv_scale: float) -> torch.Tensor:
    """d_images NCHW fp32 = 2 * (c_skip * d_denoised + c_in * inv_scale * gx[..., :3]); gx: fp32 NHWC gradient wrt the network input."""
    n, _, h, w = d_denoised.shape
    out = torch.empty_like(d_denoised)
    call("pmi_edm_stage_in_bwd", ptr(d_denoised), ptr(gx), gx.shape[-1], ptr(sigma), sigma.numel(), sigma_data, inv_scale, ptr(out), n, h, w)
    return out


def _transpose16(src: torch.Tensor, rows: int, cols: int, ld: int, s_o: int, s_i: int, inner: int, batch: int) -> torch.Tensor:
    """[batch, cols, rows padded to 8] 16-bit: block z = (o, i) of src, [rows, cols] with row pitch ld at element o * s_o + i * s_i, transposed."""
    rp = (rows + 7) // 8 * 8
    out = _empty((batch, cols, rp), src.dtype, src.device)
    call("pmi_transpose_16", ptr(src), ptr(out), rows, cols, ld, s_o, s_i, inner, batch)
    return out


def _heads_t(x: torch.Tensor, heads: int, d: int, hs: int) -> torch.Tensor:
    """The heads of a token-major operand, each transposed: x [N, R, .] -> [N*heads, d, Rp]."""
    n, r, ld = x.shape[0], x.shape[1], x.stride(1)
    return _transpose16(x, r, d, ld, r * ld, hs, heads, n * heads)


def _scores_t(s: torch.Tensor, cols: int, heads: int) -> torch.Tensor:
    """A score-shaped matrix transposed per head: s [N*heads, R, >= cols] -> [N*heads, cols, Rp]."""
    nh, r, ld = s.shape
    return _transpose16(s, r, cols, ld, heads * r * ld, r * ld, heads, nh)


def _heads_scores(a: torch.Tensor, b: torch.Tensor, heads: int, d: int, hs: int, dt: int) -> torch.Tensor:
    """a_h b_h^T per (sample, head) of two token-major operands a [N, T, .] and b [N, Tk, .] -> fp32 [N*heads, T, Tkp]."""
    n, t, tk = a.shape[0], a.shape[1], b.shape[1]
    tkp = (tk + 7) // 8 * 8
    s = _empty((n * heads, t, tkp), torch.float32, a.device)
    return bgemm(a, b, s, M=t, N=tk, K=d, lda=a.stride(1), ldb=b.stride(1), ldd=tkp, batch=n * heads, batch_inner=heads,
                 sA=(t * a.stride(1), hs), sB=(tk * b.stride(1), hs), sD=(heads * t * tkp, t * tkp), dt=dt)


def _heads_product(a: torch.Tensor, bt: torch.Tensor, dst: torch.Tensor, heads: int, d: int, dt: int) -> None:
    """Head h of the token-major dst [N, M, .] = a_z bt_z^T, z = (sample, head): a [N*heads, M, Kp] is a score-shaped matrix or its _scores_t,
    bt [N*heads, d, Kp] a _heads_t; Kp is the inner length padded to 8."""
    nh, m, kp = a.shape
    ld = dst.stride(1)
    bgemm(a, bt, dst, M=m, N=d, K=kp, lda=kp, ldb=kp, ldd=ld, batch=nh, batch_inner=heads,
          sA=(heads * m * kp, m * kp), sB=(heads * d * kp, d * kp), sD=(m * ld, d), dt=dt)


def _gemm_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, d: int, dt: int, hs: Optional[int] = None,
                    causal: bool = False):
    """softmax(q k^T d^-1/2) v as two batched MFMA GEMMs, an fp32 softmax and a transpose: the route of every head dim the flash kernels do
    not take, and the one that keeps the softmax for _gemm_attention_backward.  q [N, T, .], k and v [N, Tk, .] are (views of) 16-bit tensors
    as flash_attention takes them: stride(1) is the leading dimension, data_ptr() carries the channel offset and head h sits at channels
    [h*hs, h*hs + d) of the view (hs = d by default; 3*d for channels ordered (head, {q,k,v}, d)).
    -> (out [N, T, heads*d], P [N*heads, T, Tkp] 16-bit with zero pad columns, Tkp = Tk rounded up to 8)."""
    hs = hs or d
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1
    n, t, tk = q.shape[0], q.shape[1], k.shape[1]
    s = _heads_scores(q, k, heads, d, hs, dt)
    p = _empty(tuple(s.shape), q.dtype, q.device)
    call("pmi_softmax_causal_fwd" if causal else "pmi_softmax_fwd", ptr(s), ptr(p), n * heads * t, tk, s.shape[2], s.shape[2], float(d) ** -0.5, dt)
    out = _empty((n, t, heads * d), q.dtype, q.device)
    _heads_product(p, _heads_t(v, heads, d, hs), out, heads, d, dt)
    return out, p


def _gemm_attention_backward(q: Optional[torch.Tensor], k: torch.Tensor, v: torch.Tensor, p: torch.Tensor, d_out: torch.Tensor, heads: int,
                             d: int, dt: int, dq: torch.Tensor, dk: Optional[torch.Tensor] = None, dv: Optional[torch.Tensor] = None) -> None:
    """The gradient of _gemm_attention (hs = d) from d loss / d out [N, T, heads*d] and the kept softmax P, written into the token-major
    destination views dq [N, T, .] and dk, dv [N, Tk, .] (16-bit or fp32; the three slices of one dqkv, or dq and the halves of an fp32 dkv).
    The five products autograd forms: dP = dO V^T, dS = softmax'(P, dP) with the scale folded in, dV = P^T dO, dQ = dS K, dK = dS^T Q.
    With dk and dv None dq alone is written and q may be None."""
    assert (dk is None) == (dv is None) and (dk is None or q is not None), "dk and dv come as a pair, and need q"
    assert all(x.stride(2) == 1 for x in (q, k, v, d_out, dq, dk, dv) if x is not None)
    tk = k.shape[1]
    dp = _heads_scores(d_out, v, heads, d, d, dt)
    ds = _empty(tuple(dp.shape), d_out.dtype, d_out.device)
    call("pmi_softmax_bwd", ptr(dp), ptr(p), ptr(ds), dp.shape[0] * dp.shape[1], tk, dp.shape[2], dp.shape[2], float(d) ** -0.5, dt)
    if dv is not None:
        _heads_product(_scores_t(p, tk, heads), _heads_t(d_out, heads, d, d), dv, heads, d, dt)
    _heads_product(ds, _heads_t(k, heads, d, d), dq, heads, d, dt)
    if dk is not None:
        _heads_product(_scores_t(ds, tk, heads), _heads_t(q, heads, d, d), dk, heads, d, dt)


def attention(qkv: torch.Tensor, heads: int, order: int, dt: int, causal: bool = False) -> torch.Tensor:
    """Self-attention over tokens.  qkv: [N, T, 3C] 16-bit -> [N, T, C].
    causal: query i sees keys 0..i (the CLIP text tower's mask, ruclip/model.py:181-185); runs the batched-GEMM path.

    order 0: channels = (head, {q,k,v}, d) (unet.py:332-348); order 1: ({q,k,v}, head, d).
    Head dim 64 runs the fused flash kernel; other head dims flash_attention (order 1, up to d = 160) or _gemm_attention.
    """
    if dt == DT_F16X2:
        if causal:
            raise NotImplementedError("causal attention has no precise-mode path")
        return attention_precise(qkv, heads, order)
    n, t, c3 = qkv.shape
    c = c3 // 3
    d = c // heads
    dev = qkv.device
    if d == 64 and not causal:
        tp = (t + 31) // 32 * 32
        q = _empty((n * heads, tp, 64), qkv.dtype, dev)
        k = _empty((n * heads, tp, 64), qkv.dtype, dev)
        vt = _empty((n * heads, 64, tp), qkv.dtype, dev)
        out = _empty((n, t, c), qkv.dtype, dev)
        call("pmi_qkv_split", ptr(qkv), ptr(q), ptr(k), ptr(vt), n, t, heads, order, dt)
        call("pmi_attn_d64", ptr(q), ptr(k), ptr(vt), ptr(out), n, t, heads, float(d) ** -0.5, dt)
        return out
    assert d % 8 == 0, "head dim must be a multiple of 8"
    if FLASH_ENABLED and order == 1 and not causal and d <= 160:
        return flash_attention(qkv, qkv[..., c:], qkv[..., 2 * c:], heads, d, dt)
    if order == 0:
        return _gemm_attention(qkv, qkv[..., d:], qkv[..., 2 * d:], heads, d, dt, hs=3 * d, causal=causal)[0]
    return _gemm_attention(qkv, qkv[..., c:], qkv[..., 2 * c:], heads, d, dt, causal=causal)[0]


def _flash_forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, d: int, dt: int, lse: Optional[torch.Tensor] = None):
    """pmi_attn_flash, or with lse [N*heads, Tp32] fp32 pmi_attn_flash_train, which also leaves the log-sum-exp there: (out, the fragment
    workspace).  The same kernels and output bits either way."""
    n, t = q.shape[:2]
    tk = k.shape[1]
    assert q.stride(2) == 1 and k.stride(2) == 1 and v.stride(2) == 1 and k.stride(1) == v.stride(1)
    assert q.stride(0) == t * q.stride(1) and k.stride(0) == tk * k.stride(1)
    kib = _hip.lib().pmi_attn_flash_workspace(n, t, tk, heads, d)
    if kib < 0:
        raise ValueError(f"flash attention: unsupported head dim {d}")
    ws = _empty((kib * 512,), q.dtype, q.device)
    out = _empty((n, t, heads * d), q.dtype, q.device)
    if lse is None:
        call("pmi_attn_flash", ptr(q), q.stride(1), ptr(k), ptr(v), k.stride(1), ptr(out), ptr(ws), n, t, tk, heads, d, float(d) ** -0.5, dt)
    else:
        call("pmi_attn_flash_train", ptr(q), q.stride(1), ptr(k), ptr(v), k.stride(1), ptr(out), ptr(ws), ptr(lse), n, t, tk, heads, d,
             float(d) ** -0.5, dt)
    return out, ws


def flash_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, d: int, dt: int) -> torch.Tensor:
    """softmax(q k^T d^-1/2) v through pmi_attn_flash.  q [N, T, >= heads*d] and k, v [N, Tk, >= heads*d] are (views of) 16-bit tensors
    whose last-dim stride is 1 and whose head h sits at channels [h*d, (h+1)*d) of the view; -> [N, T, heads*d]."""
    return _flash_forward(q, k, v, heads, d, dt)[0]


def flash_attention_train(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, d: int, dt: int):
    """flash_attention keeping what flash_attention_backward needs: (out, saved).  Same kernels and output bits as flash_attention
    (_flash_forward); kept are the operand views, the forward's fragment workspace, the output and lse [N*heads, Tp] fp32 (exp2 domain) --
    no probabilities."""
    lse = _empty((q.shape[0] * heads, (q.shape[1] + 31) // 32 * 32), torch.float32, q.device)
    out, ws = _flash_forward(q, k, v, heads, d, dt, lse)
    return out, (q, k, v, ws, lse, out)


def flash_attention_backward(saved, d_out: torch.Tensor, heads: int, d: int, dt: int, dq_only: bool = False):
    """Gradient of flash_attention_train from d loss / d out [N, T, heads*d] (pmi_attn_flash_bwd: P recomputed per tile from lse).
    Self-attention (q, k, v are the three slices of one qkv tensor): d qkv [N, T, 3C], channels (q|k|v, head, d).  dq_only (cross-attention,
    constant k / v): dq [N, T, C] alone.  Cross-attention (k, v the two halves of one [N, Tk, 2C] tensor) without dq_only: (dq [N, T, C] 16-bit, the dq_only
    bits, and dkv [N, Tk, 2C] FP32 in the layout of the forward's kv) through pmi_attn_flash_bwd_kv, the key role split over query chunks.
    dkv stays fp32: it sums up to T terms and feeds an fp32 GEMM, so no 16-bit range argument is needed."""
    q, k, v, ws, lse, out = saved
    n, t = q.shape[:2]
    tk, c = k.shape[1], heads * d
    assert d_out.is_contiguous() and tuple(d_out.shape) == (n, t, c)
    delta = _empty(tuple(lse.shape), lse.dtype, lse.device)
    # cross-attention: k | v are the two halves of one [N, Tk, 2C] tensor (the forward's kv), the layout dkv is returned in
    if not dq_only and k.stride(1) == 2 * c and v.data_ptr() == k.data_ptr() + c * k.element_size():
        kib = _hip.lib().pmi_attn_flash_bwd_kv_workspace(n, t, tk, heads, d)
        if kib < 0:
            raise ValueError(f"flash attention: unsupported head dim {d}")
        wsb = _empty((kib * 512,), q.dtype, q.device)
        g = _empty((n, t, c), q.dtype, q.device)
        dkv = _empty((n, tk, 2 * c), torch.float32, q.device)
        call("pmi_attn_flash_bwd_kv", ptr(q), q.stride(1), ptr(k), ptr(v), k.stride(1), ptr(out), ptr(d_out), ptr(ws), ptr(lse), ptr(wsb),
             ptr(delta), ptr(g), c, ptr(dkv), dkv.data_ptr() + 4 * c, 2 * c, n, t, tk, heads, d, float(d) ** -0.5, dt)
        return g, dkv
    kib = _hip.lib().pmi_attn_flash_bwd_workspace(n, t, tk, heads, d, int(dq_only))
    wsb = _empty((kib * 512,), q.dtype, q.device)
    if dq_only:
        g = _empty((n, t, c), q.dtype, q.device)
        dk = dv = None
        lddkv = 0
    else:
        assert tk == t
        g = _empty((n, t, 3 * c), q.dtype, q.device)
        dk, dv, lddkv = g[..., c:], g[..., 2 * c:], 3 * c
    call("pmi_attn_flash_bwd", ptr(q), q.stride(1), ptr(k), ptr(v), k.stride(1), ptr(out), ptr(d_out), ptr(ws), ptr(lse), ptr(wsb), ptr(delta),
         ptr(g), g.stride(1), ptr(dk), ptr(dv), lddkv, n, t, tk, heads, d, float(d) ** -0.5, int(dq_only), dt)
    return g


def cross_attention_train(q: torch.Tensor, kv: torch.Tensor, heads: int, dt: int):
    """cross_attention's batched-GEMM route keeping the softmax (_gemm_attention): (out [N, T, C], P [N*heads, T, Tcp] 16-bit)."""
    c = q.shape[2]
    return _gemm_attention(q, kv, kv[..., c:], heads, c // heads, dt)


def cross_attention_backward(kv: torch.Tensor, p: torch.Tensor, d_out: torch.Tensor, heads: int, dt: int, q: Optional[torch.Tensor] = None):
    """d loss / d q [N, T, C] of cross_attention_train from the kept softmax (_gemm_attention_backward).  With q (the forward's queries; a
    differentiable prompt) also d loss / d kv: (dq, dkv [N, Tc, 2C] fp32 in the layout of kv), fp32 out as flash_attention_backward's."""
    n, t, c = d_out.shape
    dq = _empty((n, t, c), d_out.dtype, d_out.device)
    if q is None:
        _gemm_attention_backward(None, kv, kv[..., c:], p, d_out, heads, c // heads, dt, dq)
        return dq
    dkv = _empty((n, kv.shape[1], 2 * c), torch.float32, d_out.device)
    _gemm_attention_backward(q, kv, kv[..., c:], p, d_out, heads, c // heads, dt, dq, dkv, dkv[..., c:])
    return dq, dkv


def geglu_backward(h: torch.Tensor, dg: torch.Tensor, dt: int) -> torch.Tensor:
    """d loss / d h [M, 2F] from the kept pre-activation h (16 value | 16 gate column groups) and dg = d loss / d (value * gelu(gate)) [M, F]."""
    dh = torch.empty_like(h)
    call("pmi_geglu_bwd", ptr(h), ptr(dg), ptr(dh), h.shape[0], dg.shape[1], 1, dt)
    return dh


def cross_attention(q: torch.Tensor, kv: torch.Tensor, heads: int, dt: int) -> torch.Tensor:
    """softmax(q k^T d^-1/2) v with keys / values from another sequence (stable_diffusion/attention.py:268-298, the fused call at :285).
    q [N, T, C], kv [N, Tc, 2C] = (k | v) x (head, d), 16-bit -> [N, T, C].  flash_attention up to d = 160, else _gemm_attention."""
    n, t, c = q.shape
    assert kv.shape[0] == n and kv.shape[2] == 2 * c
    d = c // heads
    assert d % 8 == 0, "head dim must be a multiple of 8"
    if FLASH_ENABLED and d <= 160:
        return flash_attention(q, kv, kv[..., c:], heads, d, dt)
    return _gemm_attention(q, kv, kv[..., c:], heads, d, dt)[0]


def attention_train(qkv: torch.Tensor, heads: int, dt: int):
    """Self-attention for any head dim, channels (q|k|v, head, d), keeping the softmax for attention_backward:
    qkv [N, T, 3C] 16-bit -> (out [N, T, C], P [N*heads, T, Tp] 16-bit) by _gemm_attention."""
    c = qkv.shape[2] // 3
    return _gemm_attention(qkv, qkv[..., c:], qkv[..., 2 * c:], heads, c // heads, dt)


def attention_backward(qkv: torch.Tensor, p: torch.Tensor, d_out: torch.Tensor, heads: int, dt: int) -> torch.Tensor:
    """d loss / d qkv [N, T, 3C] from d loss / d out [N, T, C] and attention_train's softmax P (_gemm_attention_backward)."""
    n, t, c3 = qkv.shape
    c = c3 // 3
    dqkv = _empty((n, t, c3), qkv.dtype, qkv.device)
    _gemm_attention_backward(qkv, qkv[..., c:], qkv[..., 2 * c:], p, d_out.reshape(n, t, c), heads, c // heads, dt,
                             dqkv, dqkv[..., c:], dqkv[..., 2 * c:])
    return dqkv


def self_attention_train(qkv: torch.Tensor, n: int, t: int, heads: int, dt: int):
    """Self-attention keeping what self_attention_backward needs: qkv [N*T, 3C] 16-bit, channels (q|k|v, head, d) -> (out [N*T, C], saved).
    64-channel heads run the flash-style forward that keeps the log-sum-exp (csrc/attn.hip), other head dims attention_train."""
    if dt == DT_F16X2:
        return attention_precise_train(qkv, n, t, heads)
    c = qkv.shape[-1] // 3
    if c // heads == 64:
        tp32 = (t + 31) // 32 * 32
        aws = _empty((6, n * heads, tp32, 64), qkv.dtype, qkv.device)
        lse = _empty((n * heads, tp32), torch.float32, qkv.device)
        a = _empty((n * t, c), qkv.dtype, qkv.device)
        call("pmi_vit_attn_fwd", ptr(qkv), ptr(aws), ptr(lse), ptr(a), n, t, heads, 64.0 ** -0.5, dt)
        return a, (aws, lse, a)
    a, pm = attention_train(qkv.view(n, t, 3 * c), heads, dt)
    return a.view(n * t, c), (qkv, pm)


def self_attention_backward(saved, da: torch.Tensor, n: int, t: int, heads: int, dt: int) -> torch.Tensor:
    """d loss / d qkv [N*T, 3C] from d loss / d out [N*T, C] and self_attention_train's `saved`."""
    if dt == DT_F16X2:
        return attention_precise_backward(saved, da, n, t, heads)
    c = da.shape[-1]
    if c // heads == 64:
        aws, lse, a = saved
        tp32 = (t + 31) // 32 * 32
        bws = _empty((2, n * heads, tp32, 64), da.dtype, da.device)
        delta = _empty((n * heads, tp32), torch.float32, da.device)
        dqkv = _empty((n * t, 3 * c), da.dtype, da.device)
        call("pmi_vit_attn_bwd", ptr(aws), ptr(lse), ptr(a), ptr(da), ptr(bws), ptr(delta), ptr(dqkv), n, t, heads, 64.0 ** -0.5, dt)
        return dqkv
    qkv, pm = saved
    return attention_backward(qkv.view(n, t, 3 * c), pm, da.view(n, t, c), heads, dt).view(n * t, 3 * c)


def gemm_f32(A: torch.Tensor, B: torch.Tensor, D: torch.Tensor, *, M: int, N: int, K: int, lda: int, ldb: int, ldd: int, trans_b: bool = False,
             trans_a: bool = False,
             bias: Optional[torch.Tensor] = None, act: int = ACT_NONE, alpha: float = 1.0, batch: int = 1, batch_inner: int = 1,
             sA=(0, 0), sB=(0, 0), sD=(0, 0), a_off: int = 0, b_off: int = 0, d_off: int = 0, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Exact-fp32 batched GEMM on the f32-input MFMA (csrc/f32gemm.hip): D[z] = act(alpha * A[z] @ B[z]^T + bias); trans_b: B[z] is [K, N],
    trans_a: A[z] is [K, M]."""
    a = _hip.GemmF32Args()
    a.A, a.B, a.bias, a.D = A.data_ptr() + 4 * a_off, B.data_ptr() + 4 * b_off, ptr(bias), D.data_ptr() + 4 * d_off
    a.M, a.N, a.K, a.lda, a.ldb, a.ldd = M, N, K, lda, ldb, ldd
    a.transB, a.act, a.alpha, a.batch, a.batch_inner = int(trans_b), act, alpha, batch, batch_inner
    a.transA = int(trans_a)
    a.sA_o, a.sA_i = sA
    a.sB_o, a.sB_i = sB
    a.sD_o, a.sD_i = sD
    a.R = ptr(residual)
    call("pmi_gemm_f32", C.byref(a))
    return D


def linear_f32(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor], act: int = ACT_NONE,
               residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """fp32 linear layer x [M, K] @ weight [N, K]^T + bias (the time MLPs in precise mode)."""
    m, k = x.shape
    n = weight.shape[0]
    out = _empty((m, n), torch.float32, x.device)
    return gemm_f32(x, weight, out, M=m, N=n, K=k, lda=x.stride(0), ldb=weight.stride(0), ldd=n, bias=bias, act=act, residual=residual)


def _attention_precise(qkv: torch.Tensor, n: int, t: int, heads: int, order: int):
    """Self-attention in precise mode: qkv is a precise tensor [N, T, 2*3C] or [N*T, 2*3C], channel order as `attention`; scores, softmax
    and values in exact fp32 (both operands of these products are activations, so the hi + lo weight trick does not apply).
    -> (precise out [.., 2C] with qkv's leading dims, (the fp32 copy of q, k, v [N, T, 3C], the fp32 softmax P [N*heads, T, T]))."""
    c3 = qkv.shape[-1] // 2
    c = c3 // 3
    d = c // heads
    dev = qkv.device
    q32 = _empty((n, t, c3), torch.float32, dev)
    call("pmi_split_to_f32", ptr(qkv), ptr(q32), n * t, c3)
    ko, vo, hs = (d, 2 * d, 3 * d) if order == 0 else (c, 2 * c, d)
    p = _empty((n * heads, t, t), torch.float32, dev)
    gemm_f32(q32, q32, p, M=t, N=t, K=d, lda=c3, ldb=c3, ldd=t, batch=n * heads, batch_inner=heads,
             sA=(t * c3, hs), sB=(t * c3, hs), sD=(heads * t * t, t * t), b_off=ko)
    call("pmi_softmax_f32", ptr(p), n * heads * t, t, t, float(d) ** -0.5)
    o32 = _empty((n, t, c), torch.float32, dev)
    gemm_f32(p, q32, o32, M=t, N=d, K=t, lda=t, ldb=c3, ldd=c, trans_b=True, batch=n * heads, batch_inner=heads,
             sA=(heads * t * t, t * t), sB=(t * c3, hs), sD=(t * c, d), b_off=vo)
    out = _empty(tuple(qkv.shape[:-1]) + (2 * c,), torch.float16, dev)
    call("pmi_split_from_f32", ptr(o32), c, ptr(out), n * t, c)
    return out, (q32, p)


def attention_precise(qkv: torch.Tensor, heads: int, order: int) -> torch.Tensor:
    """`attention` in precise mode (_attention_precise): qkv is a precise tensor [N, T, 2*3C]; returns a precise [N, T, 2C]."""
    return _attention_precise(qkv, qkv.shape[0], qkv.shape[1], heads, order)[0]


def attention_precise_train(qkv: torch.Tensor, n: int, t: int, heads: int):
    """self_attention_train in precise mode (_attention_precise, order 1): qkv is a precise [N*T, 2*3C] tensor, channels (q|k|v, head, d) ->
    (precise out [N*T, 2C], saved); the fp32 copy of q, k, v and the fp32 softmax P stay on the tape."""
    return _attention_precise(qkv, n, t, heads, 1)


def attention_precise_backward(saved, da: torch.Tensor, n: int, t: int, heads: int) -> torch.Tensor:
    """Precise d loss / d qkv [N*T, 2*3C], channels (q|k|v, head, d), from the precise d loss / d out [N*T, 2C]: the five products of
    _gemm_attention_backward in exact fp32 (pmi_gemm_f32), dS = scale P o (dP - rowsum(dP o P)) in place over dP (pmi_softmax_bwd_f32)."""
    q32, p = saved
    c3 = q32.shape[-1]
    c = c3 // 3
    d = c // heads
    dev = da.device
    nh = n * heads
    do32 = _empty((n, t, c), torch.float32, dev)
    call("pmi_split_to_f32", ptr(da), ptr(do32), n * t, c)
    sP, sQ, sO = (heads * t * t, t * t), (t * c3, d), (t * c, d)
    ds = _empty((nh, t, t), torch.float32, dev)
    gemm_f32(do32, q32, ds, M=t, N=t, K=d, lda=c, ldb=c3, ldd=t, batch=nh, batch_inner=heads, sA=sO, sB=sQ, sD=sP, b_off=2 * c)     # dP = dO V^T
    call("pmi_softmax_bwd_f32", ptr(ds), ptr(p), nh * t, t, t, float(d) ** -0.5)
    dq32 = _empty((n, t, c3), torch.float32, dev)
    gemm_f32(p, do32, dq32, M=t, N=d, K=t, lda=t, ldb=c, ldd=c3, trans_a=True, trans_b=True, batch=nh, batch_inner=heads,
             sA=sP, sB=sO, sD=sQ, d_off=2 * c)                                                                                  # dV = P^T dO
    gemm_f32(ds, q32, dq32, M=t, N=d, K=t, lda=t, ldb=c3, ldd=c3, trans_b=True, batch=nh, batch_inner=heads,
             sA=sP, sB=sQ, sD=sQ, b_off=c)                                                                                      # dQ = dS K
    gemm_f32(ds, q32, dq32, M=t, N=d, K=t, lda=t, ldb=c3, ldd=c3, trans_a=True, trans_b=True, batch=nh, batch_inner=heads,
             sA=sP, sB=sQ, sD=sQ, d_off=c)                                                                                      # dK = dS^T Q
    dqkv = _empty((n * t, 2 * c3), torch.float16, dev)
    call("pmi_split_from_f32", ptr(dq32), c3, ptr(dqkv), n * t, c3)
    return dqkv
