"""Launch wrappers for the differentiable JPEG codec kernels (csrc/jpeg.hip), the hot path of drawers.JPEG.

Coefficients keep the reference's layout (perceptor/drawers/jpeg): y [N, (H/8)(W/8), 8, 8], cb and cr [N, (H/16)(W/16), 8, 8], fp32; images
are NCHW [N, 3, H, W] in [0, 1]; H and W multiples of 16.  One launch per call; HIP device only.
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch

from .._hip import call, ptr


def _check_hw(height: int, width: int) -> None:
    if height <= 0 or width <= 0 or height % 16 or width % 16:
        raise ValueError(f"jpeg: height and width must be positive multiples of 16 (4:2:0 macroblocks), got {height} x {width}")


def _prep(t: torch.Tensor, what: str) -> torch.Tensor:
    if not torch.is_tensor(t) or not t.is_cuda:
        raise RuntimeError(f"jpeg: {what} must be on a HIP device (perceptor_amd has no CPU fallback)")
    return t.detach().float().contiguous()


def _coefficients(y, cb, cr, height: int, width: int):
    # shapes first, the device after: a wrong shape is a ValueError wherever the tensors live
    _check_hw(height, width)
    n = y.shape[0]
    want = {"y": (n, (height // 8) * (width // 8), 8, 8), "cb": (n, (height // 16) * (width // 16), 8, 8)}
    want["cr"] = want["cb"]
    for name, t in (("y", y), ("cb", cb), ("cr", cr)):
        if tuple(t.shape) != want[name]:
            raise ValueError(f"jpeg: {name} has shape {tuple(t.shape)}, a {height} x {width} image of batch {n} needs {want[name]}")
    return _prep(y, "y"), _prep(cb, "cb"), _prep(cr, "cr"), n


def _factor(factor) -> float:
    factor = float(factor)
    if not factor > 0.0 or factor == float("inf"):
        raise ValueError(f"jpeg: factor must be a positive finite number, got {factor}")
    return factor


def jpeg_decode(y, cb, cr, height: int, width: int, factor=1.0) -> torch.Tensor:
    """decompress_jpeg(height, width, factor=factor)(y, cb, cr): images [N, 3, height, width] in [0, 1]."""
    factor = _factor(factor)
    y, cb, cr, n = _coefficients(y, cb, cr, height, width)
    out = torch.empty((n, 3, height, width), dtype=torch.float32, device=y.device)
    call("pmi_jpeg_decode", ptr(y), ptr(cb), ptr(cr), factor, ptr(out), n, height, width)
    return out


def jpeg_decode_backward(y, cb, cr, d_images, factor=1.0, need: Sequence[bool] = (True, True, True)) -> Tuple:
    """(d_y, d_cb, d_cr) of sum(jpeg_decode(y, cb, cr) * d_images); entries whose ``need`` is False are None and are not computed.
    The clamp passes the gradient where the decoded value lies strictly inside (0, 1)."""
    if d_images.dim() != 4 or d_images.shape[1] != 3:
        raise ValueError(f"jpeg: d_images must be [N, 3, H, W], got {tuple(d_images.shape)}")
    height, width = int(d_images.shape[2]), int(d_images.shape[3])
    if d_images.shape[0] != y.shape[0]:
        raise ValueError(f"jpeg: d_images has batch {d_images.shape[0]}, the coefficients {y.shape[0]}")
    factor = _factor(factor)
    y, cb, cr, n = _coefficients(y, cb, cr, height, width)
    d = _prep(d_images, "d_images")
    outs = [torch.empty_like(t) if k else None for t, k in zip((y, cb, cr), need)]
    call("pmi_jpeg_decode_bwd", ptr(y), ptr(cb), ptr(cr), factor, ptr(d), ptr(outs[0]), ptr(outs[1]), ptr(outs[2]), n, height, width)
    return tuple(outs)


def jpeg_encode(images, factor=1.0, rounding: bool = True) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """compress_jpeg(factor=factor)(images): (y, cb, cr).  rounding True: the reference's diff_round; False: the quotients unrounded.
    Forward only."""
    if images.dim() != 4 or images.shape[1] != 3:
        raise ValueError(f"jpeg: images must be [N, 3, H, W], got {tuple(images.shape)}")
    n, _, height, width = (int(v) for v in images.shape)
    _check_hw(height, width)
    factor = _factor(factor)
    x = _prep(images, "images")
    y = torch.empty((n, (height // 8) * (width // 8), 8, 8), dtype=torch.float32, device=x.device)
    cb = torch.empty((n, (height // 16) * (width // 16), 8, 8), dtype=torch.float32, device=x.device)
    cr = torch.empty_like(cb)
    call("pmi_jpeg_encode", ptr(x), factor, 1 if rounding else 0, ptr(y), ptr(cb), ptr(cr), n, height, width)
    return y, cb, cr


class _Decode(torch.autograd.Function):
    @staticmethod
    def forward(ctx, y, cb, cr, height, width, factor):
        ctx.save_for_backward(y, cb, cr)
        ctx.factor = factor
        return jpeg_decode(y, cb, cr, height, width, factor)

    @staticmethod
    def backward(ctx, grad):
        y, cb, cr = ctx.saved_tensors
        d_y, d_cb, d_cr = jpeg_decode_backward(y, cb, cr, grad, ctx.factor, need=ctx.needs_input_grad[:3])
        return d_y, d_cb, d_cr, None, None, None


def jpeg_decode_autograd(y, cb, cr, height: int, width: int, factor=1.0) -> torch.Tensor:
    """jpeg_decode as a node of the autograd graph: the backward pass is one pmi_jpeg_decode_bwd launch."""
    return _Decode.apply(y, cb, cr, height, width, factor)
