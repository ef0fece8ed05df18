"""losses.SuperResolution — drop-in for perceptor/losses/super_resolution/super_resolution.py:8-35: how far images are from their own
super-resolved down-sampling,
    mean (images - resize(upsample(resize(images, H // p x W // p))))^2,    p = pre_downscale (default: the model's scale),
both resizes with ``resample=mode`` and the second only when the up-sampled shape differs from the images'.  As upstream the up-sampled
images are a constant (computed without gradient): the gradient is 2 (images - upsampled) / count, which pmi_sqdiff_loss writes with
the value.  ``forward`` is a scalar that works with ``.backward()``; ``loss_and_grad`` is the fused path without autograd.
SuperResolutionDiscriminator, the other export of the reference's package, is losses/super_resolution_discriminator.py (imported from
that module; `losses` itself does not re-export it).
"""
from __future__ import annotations

import torch

from .. import transforms
from ..transforms.resize import resize as _resize
from .open_clip import LossInterface
from .pixel import _sqdiff


class _SuperResolutionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images, module):
        loss, g = module._loss_and_grad(images.detach(), None)
        ctx.save_for_backward(g)
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        return g * grad_out, None


class SuperResolution(LossInterface):
    def __init__(self, name="x2", pre_downscale=None, half=True, mode="bicubic", **kwargs):
        super().__init__()
        self.transform = transforms.SuperResolution(name, half, **kwargs)
        self.mode = mode
        self.pre_downscale = self.transform.model.scale if pre_downscale is None else pre_downscale

    @torch.no_grad()
    def upsampled(self, images):
        """The constant side of the loss: images down-sized by pre_downscale, super-resolved, resized back to the images' shape."""
        if not images.is_cuda:
            raise RuntimeError("losses.SuperResolution runs on a HIP device only (no CPU fallback)")
        h, w = images.shape[-2:]
        small = (h // self.pre_downscale, w // self.pre_downscale)
        if small[0] < 1 or small[1] < 1:
            raise ValueError(f"SuperResolution: images of {h} x {w} are smaller than pre_downscale {self.pre_downscale}")
        up = self.transform(_resize(images, small, resample=self.mode))
        if tuple(up.shape[-2:]) != (h, w):
            up = _resize(up, (h, w), resample=self.mode)
        return up

    def _loss_and_grad(self, images, n_total):
        x = images.float().contiguous()
        up = self.upsampled(x)
        count = x.numel() // x.shape[0] * int(n_total or x.shape[0])
        return _sqdiff(x, up, count)

    def forward(self, images):
        return _SuperResolutionFn.apply(images, self)

    @torch.no_grad()
    def loss_and_grad(self, images, n_total=None):
        """(loss, dloss/dimages).  ``n_total``: global batch when this rank holds a shard."""
        return self._loss_and_grad(images, n_total)
