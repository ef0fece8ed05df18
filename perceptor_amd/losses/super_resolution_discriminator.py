"""SuperResolutionDiscriminator — drop-in for perceptor/losses/super_resolution/discriminator.py:13-29: Real-ESRGAN's U-Net critic
(UNetDiscriminatorSN, num_in_ch 3, skip connections) as a guidance term,
    -mean(model(images)) * 0.001,
which pushes a sample towards what the critic calls a real photograph.  Images go in as they are (the reference applies no normalisation);
height and width must be multiples of 8, as upstream, whose skip additions fail otherwise.  ``forward`` is a scalar that works with
``.backward()``; ``loss_and_grad`` is the fused path without autograd; ``logits`` is the critic's fp32 map.  The arithmetic is
engine/disc.py (csrc/disc.hip for the stride-2 adjoints).

Import it from this module, ``from perceptor_amd.losses.super_resolution_discriminator import SuperResolutionDiscriminator``: the
``losses`` package does not re-export the name yet (an existing test pins its absence there), so ``losses.SuperResolutionDiscriminator``
is still an AttributeError.

``self.model`` holds the parameters under the reference's names (``convK.weight_orig`` / ``weight_u`` / ``weight_v`` for K = 1 .. 8); it is a
container only, packed on first use on the module's device and again after ``load_state_dict``.

Deviation from upstream: the reference never calls ``.eval()`` on the discriminator, so it runs one power iteration per call and mutates
``weight_u``.  This class is the deterministic eval-mode function, W = weight_orig / (u . W v) with u, v as stored; at a trained checkpoint
u, v sit at their fixed point and the values agree.

Not available here: the RealESRGAN_x4plus_netD checkpoint (the reference downloads it): pass ``checkpoint=`` (the upstream .pth, a dict with
"params") or get deterministic synthetic weights.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from ..engine import disc as disc_engine
from .open_clip import LossInterface

NAMES = ("RealESRGAN_x4plus_netD",)


class _Slot(nn.Module):
    """The parameters and buffers of one convolution under the reference's names"""

    def __init__(self, entries):
        super().__init__()
        for name, shape in entries:
            if name in ("weight_u", "weight_v"):
                self.register_buffer(name, torch.zeros(shape))
            else:
                setattr(self, name, nn.Parameter(torch.zeros(shape), requires_grad=False))


def _container(num_feat):
    m, slots = nn.Module(), {}
    for key, shape in disc_engine.disc_state_dict_shapes(num_feat).items():
        mod, leaf = key.split(".")
        slots.setdefault(mod, []).append((leaf, shape))
    for mod, entries in slots.items():
        m.add_module(mod, _Slot(entries))
    return m


class _DiscriminatorFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, module):
        loss, g = module._need_engine().loss_and_grad(images.detach(), None)
        ctx.save_for_backward(g)
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return g * grad_out, None


class SuperResolutionDiscriminator(LossInterface):
    def __init__(self, name="RealESRGAN_x4plus_netD", *, weights="synthetic", checkpoint: Optional[str] = None, dtype="f16", seed: int = 0,
                 num_feat: int = 64):
        super().__init__()
        if name not in NAMES:
            raise ValueError(f"SuperResolutionDiscriminator: unknown name {name!r} (one of {NAMES})")
        if dtype not in ("f16", "bf16"):
            raise ValueError("SuperResolutionDiscriminator runs in 'f16' or 'bf16'")
        self.name, self.dtype, self.num_feat = name, dtype, int(num_feat)
        if self.num_feat not in disc_engine.NUM_FEATS:
            raise ValueError(f"SuperResolutionDiscriminator: num_feat {num_feat} is not one of {disc_engine.NUM_FEATS}")
        if checkpoint is not None:
            sd = disc_engine.map_state_dict(torch.load(checkpoint, map_location="cpu", weights_only=True), self.num_feat)
        elif weights == "synthetic":
            sd = disc_engine.synth_disc_state_dict(self.num_feat, seed)
        else:
            raise ValueError(f"SuperResolutionDiscriminator: weights {weights!r} are not reachable here: pass checkpoint= or weights='synthetic'")
        self.model = _container(self.num_feat)
        self.model.load_state_dict(sd)
        self.model.eval()
        self.model.requires_grad_(False)
        self._engine = None
        self.model.register_load_state_dict_post_hook(lambda module, incompatible: setattr(self, "_engine", None))
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_engine", None))

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)

    @property
    def device(self):
        return self.model.conv0.weight.device

    def _need_engine(self) -> disc_engine.DiscriminatorEngine:
        if self._engine is None:
            if self.device.type != "cuda":
                raise RuntimeError("SuperResolutionDiscriminator needs a HIP device: call .to('cuda') first (perceptor_amd has no CPU fallback)")
            self._engine = disc_engine.DiscriminatorEngine(self.num_feat, self.model.state_dict(), self.device, self.dtype)
        return self._engine

    def _check(self, images):
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"SuperResolutionDiscriminator expects NCHW images with 3 channels, got {tuple(images.shape)}")
        if images.shape[-2] % 8 or images.shape[-1] % 8:
            raise ValueError(f"SuperResolutionDiscriminator: height and width must be multiples of 8, got {tuple(images.shape[-2:])}")
        if not images.is_cuda:
            raise RuntimeError("SuperResolutionDiscriminator runs on a HIP device only (no CPU fallback)")

    def forward(self, images):
        self._check(images)
        return _DiscriminatorFn.apply(images, self)

    @torch.no_grad()
    def loss_and_grad(self, images, n_total=None, record=None):
        """(loss, dloss/dimages).  ``n_total``: global batch when this rank holds a shard."""
        self._check(images)
        return self._need_engine().loss_and_grad(images, n_total, record)

    @torch.no_grad()
    def logits(self, images):
        """The critic's map, fp32 [N, 1, H, W]."""
        self._check(images)
        return self._need_engine().logits(images)
