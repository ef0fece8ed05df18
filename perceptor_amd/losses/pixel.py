"""losses.Smoothness / losses.Resize — drop-ins for perceptor/losses/smoothness.py:4-10 and perceptor/losses/resize.py:5-18,
the two guidance terms that need no network.

``forward`` keeps the reference contract (a scalar that works with ``.backward()``); value and gradient come from the same
HIP launch (pmi_smoothness / pmi_sqdiff_loss, csrc/losses.hip), the resize and its adjoint from transforms.resize /
transforms.resize_backward.  ``loss_and_grad`` is the fused path without autograd.
"""
from __future__ import annotations

import torch

from .._hip import call, ptr
from ..transforms.resize import resize as _resize, resize_backward as _resize_backward
from .open_clip import LossInterface


def _smoothness(images, n_total=None, gscale=1.0):
    if images.dim() != 4:
        raise ValueError("Smoothness expects NCHW images")
    x = images.detach().float().contiguous()
    n, c, h, w = x.shape
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    grad = torch.empty_like(x)
    partial = torch.empty(2048, dtype=torch.float32, device=x.device)
    call("pmi_smoothness", ptr(x), ptr(loss), ptr(grad), ptr(partial), n, c, h, w, int(n_total or n), float(gscale))
    return loss[0], grad


def _sqdiff(a, b, n_total_count=None):
    """(mean (a - b)^2, its gradient to a); the gradient to b is the negative."""
    a, b = a.detach().float().contiguous(), b.detach().float().contiguous()
    if a.shape != b.shape:
        raise ValueError(f"shapes differ: {tuple(a.shape)} vs {tuple(b.shape)}")
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    g = torch.empty_like(a)
    partial = torch.empty(1024, dtype=torch.float32, device=a.device)
    call("pmi_sqdiff_loss", ptr(a), ptr(b), ptr(loss), ptr(g), ptr(partial), a.numel(), int(n_total_count or a.numel()))
    return loss[0], g


class _SmoothnessFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images):
        loss, grad = _smoothness(images)
        ctx.save_for_backward(grad)
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_out):
        (grad,) = ctx.saved_tensors
        return grad * grad_out


class Smoothness(LossInterface):
    def forward(self, images):
        return _SmoothnessFn.apply(images)

    @torch.no_grad()
    def loss_and_grad(self, images, n_total=None):
        """(loss, dloss/dimages).  ``n_total``: global batch when this rank holds a shard."""
        return _smoothness(images, n_total)


class _ResizeLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images_a, images_b, size):
        loss, g = _sqdiff(_resize(images_a, size), _resize(images_b, size))
        ctx.save_for_backward(g)
        ctx.hw_a, ctx.hw_b = tuple(images_a.shape[2:]), tuple(images_b.shape[2:])
        return loss.clone()

    @staticmethod
    def backward(ctx, grad_out):
        (g,) = ctx.saved_tensors
        ga = _resize_backward(g, ctx.hw_a) * grad_out if ctx.needs_input_grad[0] else None
        gb = _resize_backward(g, ctx.hw_b) * (-grad_out) if ctx.needs_input_grad[1] else None
        return ga, gb, None


class Resize(LossInterface):
    def __init__(self, size=None):
        super().__init__()
        self.size = size

    def _size(self, size):
        size = self.size if size is None else size
        if size is None:
            raise ValueError("Resize needs a size (constructor or call)")
        return (size, size) if isinstance(size, int) else tuple(size)

    def forward(self, images_a, images_b, size=None):
        return _ResizeLossFn.apply(images_a, images_b, self._size(size))

    @torch.no_grad()
    def loss_and_grad(self, images_a, images_b, size=None, n_total=None):
        """(loss, dloss/dimages_a).  ``n_total``: global batch when this rank holds a shard."""
        size = self._size(size)
        ra, rb = _resize(images_a, size), _resize(images_b, size)
        count = ra.numel() // ra.shape[0] * int(n_total or ra.shape[0])
        loss, g = _sqdiff(ra, rb, count)
        return loss, _resize_backward(g, tuple(images_a.shape[2:]))
