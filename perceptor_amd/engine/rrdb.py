"""HIP engine for Real-ESRGAN's RRDBNet (perceptor/models/super_resolution/custom_rrdbnet_arch.py:9-127) with RealESRGANer's pre- and
post-processing for tile = 0, pre_pad = 0 (real_esrganer.py:50-74, 154-173).  Forward only.

  conv_first (3 | 12 -> 64)   ops.igemm; scale 2: reflect mod-pad of odd H / W on the right and bottom, then pixel-unshuffle by 2 with the
                              reference's channel order c * 4 + 2 * dh + dw (arch_util.py:191-205), both on the 3-channel fp32 input
  body.{i}: three RDBs        csrc/rrdb.hip.  An RDB lives in one 192-channel dense buffer [N, H, W, 192]: x in channels 0 .. 63, x1 .. x4 in
                              64 .. 191.  conv k reads the prefix 64 + 32 (k - 1) and writes its own slice (no torch.cat); conv5 writes
                              channels 0 .. 63 of the next RDB's buffer with alpha = 0.2, R1 = x; the third RDB's conv5 also takes
                              beta = 0.2, R2 = the RRDB's input.
  conv_body                   R1 = feat (the trunk skip)
  conv_up1 / 2 (/ 3)          up = 1 (nearest x2 folded into the halo read), slope 0.2;  conv_hr: slope 0.2
  conv_last (64 -> 3)         ops.igemm, fp32 out

Buffers: three dense buffers in rotation.  An RRDB that starts in buffer s runs its RDBs in s, s + 1, s + 2 (mod 3); the last conv5
reads its RRDB input from s (R2), its x from s + 2 (R1 and X) and writes to s + 1, where the next RRDB starts: the RRDB's input
survives its three RDBs without a copy and no launch writes a byte it also reads.

Activations are 16-bit NHWC; every convolution accumulates in fp32 and rounds once at its store.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
import torch.nn.functional as F

from .. import _hip
from .._hip import call, ptr
from . import ops
from .ops import PackedLinear

NUM_FEAT, NUM_GROW = 64, 32
SCALES = (2, 4, 8)


def rrdb_state_dict_shapes(num_block: int, scale: int, num_feat: int = NUM_FEAT, num_grow: int = NUM_GROW) -> Dict[str, Tuple[int, ...]]:
    """The reference's keys, in its module order."""
    S: Dict[str, Tuple[int, ...]] = {}

    def conv(name, cin, cout):
        S[f"{name}.weight"] = (cout, cin, 3, 3)
        S[f"{name}.bias"] = (cout,)

    conv("conv_first", 12 if scale == 2 else 3, num_feat)
    for i in range(num_block):
        for r in (1, 2, 3):
            for k in range(1, 5):
                conv(f"body.{i}.rdb{r}.conv{k}", num_feat + (k - 1) * num_grow, num_grow)
            conv(f"body.{i}.rdb{r}.conv5", num_feat + 4 * num_grow, num_feat)
    conv("conv_body", num_feat, num_feat)
    conv("conv_up1", num_feat, num_feat)
    conv("conv_up2", num_feat, num_feat)
    if scale == 8:
        conv("conv_up3", num_feat, num_feat)
    conv("conv_hr", num_feat, num_feat)
    conv("conv_last", num_feat, 3)
    return S


def map_state_dict(sd, num_block: int, scale: int):
    """RealESRGANer's precedence (real_esrganer.py:36-43): "params_ema", else "params", else the bare dict; then strict keys and shapes."""
    if "params_ema" in sd:
        sd = sd["params_ema"]
    elif "params" in sd:
        sd = sd["params"]
    want = rrdb_state_dict_shapes(num_block, scale)
    missing = [k for k in want if k not in sd]
    extra = [k for k in sd if k not in want]
    if missing or extra:
        raise ValueError(f"RRDBNet state dict: missing {missing[:4]}, unexpected {extra[:4]}")
    for k, shp in want.items():
        if tuple(sd[k].shape) != shp:
            raise ValueError(f"RRDBNet state dict: {k} has shape {tuple(sd[k].shape)}, expected {shp}")
    return {k: sd[k] for k in want}


def pack_rdb_weights(w: torch.Tensor) -> torch.Tensor:
    """[N, Cin, 3, 3] -> pmi_rdb_conv3x3's fragment order [Cin / 32][tap][N / 16][q = 4][r = 16][j = 8] = W[16 nb + r][32 ch + 8 q + j][ky][kx]."""
    n, cin = w.shape[:2]
    if n % 16 or cin % 32 or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"pack_rdb_weights: unsupported weight shape {tuple(w.shape)}")
    return w.reshape(n // 16, 16, cin // 32, 4, 8, 3, 3).permute(2, 5, 6, 0, 3, 1, 4).contiguous().reshape(-1)


def pixel_unshuffle2(x: torch.Tensor) -> torch.Tensor:
    """arch_util.py:191-205 with scale 2: out[b, c * 4 + 2 * dh + dw, h, w] = x[b, c, 2 h + dh, 2 w + dw]."""
    b, c, hh, hw = x.shape
    return x.reshape(b, c, hh // 2, 2, hw // 2, 2).permute(0, 1, 3, 5, 2, 4).reshape(b, c * 4, hh // 2, hw // 2)


def mod_pad(x: torch.Tensor, scale: int):
    """real_esrganer.py:60-74 for pre_pad = 0: (padded images, pad_h, pad_w); only scale 2 pads."""
    ph = pw = 0
    if scale == 2:
        ph, pw = x.shape[2] % 2, x.shape[3] % 2
        if ph or pw:
            x = F.pad(x, (0, pw, 0, ph), "reflect")
    return x, ph, pw


class _RdbConv:
    def __init__(self, w, b, dt, dev):
        self.cin, self.n = int(w.shape[1]), int(w.shape[0])
        self.w = pack_rdb_weights(w.float()).to(device=dev, dtype=_hip.TORCH_DTYPE[dt])
        self.b = b.float().contiguous().to(dev)


class RrdbEngine:
    def __init__(self, cfg, state_dict, device, dtype="f16"):
        num_feat, num_grow, num_block, scale = (int(v) for v in cfg)
        if (num_feat, num_grow) != (NUM_FEAT, NUM_GROW) or num_block < 1 or scale not in SCALES:
            raise ValueError(f"unsupported RRDBNet config {cfg}: num_feat 64, num_grow 32, num_block >= 1 and scale in {SCALES} are required")
        if dtype not in ("f16", "bf16"):
            raise ValueError("the RRDBNet runs in 'f16' or 'bf16'")
        self.cfg, self.num_block, self.scale, self.device = (num_feat, num_grow, num_block, scale), num_block, scale, torch.device(device)
        self.dt = _hip.dtype_code(dtype)
        self.tdt = _hip.TORCH_DTYPE[self.dt]
        _hip.lib()
        sd = {k: v.detach().float().cpu() for k, v in map_state_dict(state_dict, num_block, scale).items()}
        wb = lambda name: (sd[f"{name}.weight"], sd[f"{name}.bias"])
        self.cin_pad = 16 if scale == 2 else 8
        self.conv_first = PackedLinear(*wb("conv_first"), self.dt, self.device, cin_pad=self.cin_pad)
        self.conv_last = PackedLinear(*wb("conv_last"), self.dt, self.device)
        rc = lambda name: _RdbConv(*wb(name), self.dt, self.device)
        self.body = [[[rc(f"body.{i}.rdb{r}.conv{k}") for k in range(1, 6)] for r in (1, 2, 3)] for i in range(num_block)]
        self.conv_body = rc("conv_body")
        self.ups = [rc(f"conv_up{j}") for j in range(1, 4 if scale == 8 else 3)]
        self.conv_hr = rc("conv_hr")

    # ---- one launch -------------------------------------------------------------------------------------
    def conv(self, cv: _RdbConv, x, out, *, r1=None, r2=None, alpha=1.0, beta=1.0, slope=1.0, up=False):
        """x: [N, Hin, Win, >= cv.cin] (a view's pixel pitch is its stride), out: [N, H, W, cv.n] view; r1 / r2 like out."""
        n, h, w, _ = out.shape
        call("pmi_rdb_conv3x3", ptr(x), x.stride(-2), cv.cin, ptr(cv.w), ptr(cv.b), cv.n, ptr(out), out.stride(-2),
             ptr(r1), r1.stride(-2) if r1 is not None else 0, ptr(r2), r2.stride(-2) if r2 is not None else 0,
             float(alpha), float(beta), float(slope), int(up), n, h, w, self.dt)
        return out

    # ---- forward ------------------------------------------------------------------------------------------
    def _check(self, images):
        if not images.is_cuda:
            raise RuntimeError("RrdbEngine runs on a HIP device only (no CPU fallback)")
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"RrdbEngine expects NCHW images with 3 channels, got {tuple(images.shape)}")

    @torch.no_grad()
    def network(self, x_nchw, record: Optional[dict] = None):
        """CustomRRDBNet.forward on an fp32 NCHW input whose H, W the scale's pixel-unshuffle divides -> fp32 NCHW.  record: a dict that
        receives the 16-bit NHWC checkpoints "conv_first", "rrdb{i}", "conv_body", "up{j}", "hr" (clones)."""
        if self.scale == 2:
            x_nchw = pixel_unshuffle2(x_nchw)
        x_nchw = x_nchw.float().contiguous()
        n, c, h, w = x_nchw.shape
        dev = x_nchw.device
        keep = (lambda k, t: record.__setitem__(k, t.clone())) if record is not None else (lambda k, t: None)
        xin = torch.empty((n, h, w, self.cin_pad), dtype=self.tdt, device=dev)
        call("pmi_nchw_to_nhwc", ptr(x_nchw), ptr(xin), n, c, h, w, self.cin_pad, 1.0, 0.0, self.dt)
        feat = ops.igemm(xin, self.conv_first)
        keep("conv_first", feat)
        bufs = [torch.empty((n, h, w, NUM_FEAT + 4 * NUM_GROW), dtype=self.tdt, device=dev) for _ in range(3)]
        s = 0
        bufs[0][..., :NUM_FEAT].copy_(feat)
        for i, rrdb in enumerate(self.body):
            x_rrdb = bufs[s][..., :NUM_FEAT]
            for r, rdb in enumerate(rrdb):
                b = bufs[(s + r) % 3]
                for k in range(4):
                    lo = NUM_FEAT + NUM_GROW * k
                    self.conv(rdb[k], b, b[..., lo:lo + NUM_GROW], slope=0.2)
                nxt = bufs[(s + r + 1) % 3] if r < 2 else bufs[(s + 1) % 3]
                if r < 2:
                    self.conv(rdb[4], b, nxt[..., :NUM_FEAT], r1=b[..., :NUM_FEAT], alpha=0.2)
                else:
                    self.conv(rdb[4], b, nxt[..., :NUM_FEAT], r1=b[..., :NUM_FEAT], alpha=0.2, beta=0.2, r2=x_rrdb)
            s = (s + 1) % 3
            keep(f"rrdb{i}", bufs[s][..., :NUM_FEAT])
        y = self.conv(self.conv_body, bufs[s], torch.empty_like(feat), r1=feat)
        keep("conv_body", y)
        for j, cv in enumerate(self.ups):
            h, w = 2 * h, 2 * w
            y = self.conv(cv, y, torch.empty((n, h, w, NUM_FEAT), dtype=self.tdt, device=dev), slope=0.2, up=True)
            keep(f"up{j + 1}", y)
        y = self.conv(self.conv_hr, y, torch.empty_like(y), slope=0.2)
        keep("hr", y)
        out = ops.igemm(y, self.conv_last, out_f32=True)
        return ops.grad_to_nchw(out, 3, 1.0)

    @torch.no_grad()
    def upsample(self, images, record: Optional[dict] = None):
        """RealESRGANer.enhance(images).float() for tile = 0, pre_pad = 0: [N, 3, H, W] -> [N, 3, scale H, scale W] fp32."""
        self._check(images)
        x, ph, pw = mod_pad(images.float(), self.scale)
        out = self.network(x, record)
        if ph or pw:
            out = out[:, :, :out.shape[2] - ph * self.scale, :out.shape[3] - pw * self.scale].contiguous()
        return out
