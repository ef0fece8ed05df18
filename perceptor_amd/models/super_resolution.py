"""models.SuperResolution — drop-in for perceptor/models/super_resolution/super_resolution.py:41-160: Real-ESRGAN up-sampling of images in
[0, 1], [N, 3, H, W] -> [N, 3, scale H, scale W] fp32, through RealESRGANer's path for tile = 0, pre_pad = 0 (engine/rrdb.py).  Forward
only: the reference's loss takes the up-sampled images under no_grad, so no backward exists here and an input that requires grad while
grad is enabled raises NotImplementedError -- the result is never silently detached.

Names:
  "x2" / "x4" / "x8"                        CustomRRDBNet, 23 blocks (the reference's sberbank checkpoints)
  "RealESRGAN_x4plus", "RealESRNet_x4plus"  basicsr RRDBNet, 23 blocks, scale 4
  "RealESRGAN_x4plus_anime_6B"              basicsr RRDBNet, 6 blocks, scale 4
  "RealESRGAN_x2plus"                       basicsr RRDBNet, 23 blocks, scale 2
  the SRVGGNetCompact names                 NotImplementedError
The basicsr RRDBNet has CustomRRDBNet's architecture and state-dict keys (scale 2 by the same pixel-unshuffle) and runs on the same
engine, but basicsr is not available here: only the CustomRRDBNet path is pinned to the reference's values (tests/golden/
super_resolution_reference.npz); the parity of the four basicsr names is unpinned.

``self.net`` holds the parameters under the reference's names; it is a container only -- the arithmetic runs in the HIP engine, packed
on first use on the module's device.  The checkpoints are not reachable here: pass ``checkpoint=`` (a file in any of RealESRGANer's
three layouts: {"params_ema": ...}, {"params": ...} or the bare state dict) or get deterministic synthetic weights (gain sqrt(2)).
``half`` is accepted for the reference's signature; the engine's precision is ``dtype``.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .._hip import call, ptr
from ..engine import rrdb as rrdb_engine
from ..transforms.resize import bilinear_tables
from ..utils.synth import synth_state_dict

CONFIGS = {                                   # name -> (blocks, scale)
    "x2": (23, 2), "x4": (23, 4), "x8": (23, 8),
    "RealESRGAN_x4plus": (23, 4), "RealESRNet_x4plus": (23, 4), "RealESRGAN_x4plus_anime_6B": (6, 4), "RealESRGAN_x2plus": (23, 2),
}
COMPACT_NAMES = ("RealESRGANv2-anime-xsx2", "RealESRGANv2-animevideo-xsx2-nousm", "RealESRGANv2-animevideo-xsx2",
                 "RealESRGANv2-anime-xsx4", "RealESRGANv2-animevideo-xsx4-nousm", "RealESRGANv2-animevideo-xsx4")


def _conv(cin, cout):
    return nn.Conv2d(cin, cout, 3, 1, 1)


class _RDB(nn.Module):
    def __init__(self, nf, gc):
        super().__init__()
        for k in range(1, 5):
            setattr(self, f"conv{k}", _conv(nf + (k - 1) * gc, gc))
        self.conv5 = _conv(nf + 4 * gc, nf)


class _RRDB(nn.Module):
    def __init__(self, nf, gc):
        super().__init__()
        self.rdb1, self.rdb2, self.rdb3 = _RDB(nf, gc), _RDB(nf, gc), _RDB(nf, gc)


class _Container(nn.Module):
    """Parameters only, under the reference's names (the key table is engine/rrdb.py: rrdb_state_dict_shapes)."""

    def __init__(self, num_block, scale, nf=rrdb_engine.NUM_FEAT, gc=rrdb_engine.NUM_GROW):
        super().__init__()
        self.conv_first = _conv(12 if scale == 2 else 3, nf)
        self.body = nn.Sequential(*[_RRDB(nf, gc) for _ in range(num_block)])
        self.conv_body, self.conv_up1, self.conv_up2 = _conv(nf, nf), _conv(nf, nf), _conv(nf, nf)
        if scale == 8:
            self.conv_up3 = _conv(nf, nf)
        self.conv_hr, self.conv_last = _conv(nf, nf), _conv(nf, 3)


def _bilinear(x, size):
    """F.interpolate(x, size, mode="bilinear", align_corners=False) as two 2-tap bands (pmi_resize_apply)."""
    n, c, h, w = x.shape
    oh, ow = size
    for axis, i, o in ((2, h, oh), (3, w, ow)):
        if i == o:
            continue
        idx, wt = (t.to(x.device) for t in bilinear_tables(i, o))
        n, c, h, w = x.shape
        if axis == 2:
            out = torch.empty((n, c, o, w), dtype=torch.float32, device=x.device)
            call("pmi_resize_apply", ptr(x), ptr(out), ptr(idx), ptr(wt), n * c, h, w, o, 2, 0, 0)
        else:
            out = torch.empty((n, c, h, o), dtype=torch.float32, device=x.device)
            call("pmi_resize_apply", ptr(x), ptr(out), ptr(idx), ptr(wt), n * c * h, w, 1, o, 2, 0, 0)
        x = out
    return x


class SuperResolution(nn.Module):
    def __init__(self, name="x4", half=False, *, weights="synthetic", checkpoint: Optional[str] = None, dtype="f16", seed: int = 0,
                 num_block: Optional[int] = None):
        super().__init__()
        if name in COMPACT_NAMES:
            raise NotImplementedError(f"SuperResolution {name!r}: the SRVGGNetCompact networks are not implemented")
        if name not in CONFIGS:
            raise ValueError(f"SuperResolution: unknown name {name!r}; known: {sorted(CONFIGS)}")
        if dtype not in ("f16", "bf16"):
            raise ValueError("SuperResolution runs in 'f16' or 'bf16'")
        blocks, self.scale = CONFIGS[name]
        self.name, self.half, self.dtype = name, bool(half), dtype
        self.num_block = int(num_block) if num_block is not None else blocks      # num_block: for tests; the product is the name's
        if self.num_block < 1:
            raise ValueError("SuperResolution: num_block >= 1 is required")
        if checkpoint is not None:
            sd = rrdb_engine.map_state_dict(torch.load(checkpoint, map_location="cpu", weights_only=True), self.num_block, self.scale)
        elif weights == "synthetic":
            sd = synth_state_dict(rrdb_engine.rrdb_state_dict_shapes(self.num_block, self.scale), seed, gain=2 ** 0.5)
        else:
            raise ValueError(f"SuperResolution: weights {weights!r} are not reachable here: pass checkpoint= or weights='synthetic'")
        self.net = _Container(self.num_block, self.scale)
        self.net.load_state_dict(sd)
        self.net.eval()
        self.net.requires_grad_(False)
        self._engine = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_engine", None))

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)

    @property
    def device(self):
        return self.net.conv_first.weight.device

    def _need_engine(self) -> rrdb_engine.RrdbEngine:
        if self._engine is None:
            if self.device.type != "cuda":
                raise RuntimeError("SuperResolution needs a HIP device: call .to('cuda') first (perceptor_amd has no CPU fallback)")
            self._engine = rrdb_engine.RrdbEngine((rrdb_engine.NUM_FEAT, rrdb_engine.NUM_GROW, self.num_block, self.scale),
                                                  self.net.state_dict(), self.device, self.dtype)
        return self._engine

    def forward(self, image):
        return self.upsample(image)

    def upsample(self, image):
        if not image.is_cuda:
            raise RuntimeError("SuperResolution runs on a HIP device only (no CPU fallback)")
        if image.requires_grad and torch.is_grad_enabled():
            raise NotImplementedError("SuperResolution is forward only: no gradient to the input images (call it under torch.no_grad() "
                                      "or on a detached tensor)")
        return self._need_engine().upsample(image.detach())

    @torch.no_grad()
    def downsample(self, upsampled_image, size=None):
        if not upsampled_image.is_cuda:
            raise RuntimeError("SuperResolution runs on a HIP device only (no CPU fallback)")
        if size is None:
            size = (upsampled_image.shape[-2] // self.scale, upsampled_image.shape[-1] // self.scale)
        size = (size, size) if isinstance(size, int) else tuple(int(s) for s in size)
        return _bilinear(upsampled_image.detach().float().contiguous(), size)
