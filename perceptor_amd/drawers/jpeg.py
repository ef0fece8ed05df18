"""drawers.JPEG (perceptor/drawers/jpeg/jpeg.py): the picture as quantised 8 x 8 DCT coefficients of Y, Cb and Cr (4:2:0).

``synthesize()`` is a differentiable JPEG decoder: one pmi_jpeg_decode launch forward and one pmi_jpeg_decode_bwd launch for the gradient
of the three coefficient tensors, which are the parameters an optimiser moves.
"""
import torch
from torch import nn

from ..engine.jpeg import jpeg_decode_autograd, jpeg_encode
from ..models.super_resolution import _bilinear
from .interface import DrawingInterface


class JPEG(DrawingInterface):
    def __init__(self, init_images, factor=1):
        super().__init__()
        if not torch.is_tensor(init_images) or init_images.dim() != 4 or init_images.shape[1] != 3:
            raise ValueError("drawers.JPEG: init_images must be a [N, 3, H, W] tensor")
        if not init_images.is_cuda:
            raise ValueError("drawers.JPEG: init_images must be on a HIP device (perceptor_amd has no CPU fallback)")
        height, width = init_images.shape[-2:]
        if height % 16 or width % 16:
            raise ValueError(f"drawers.JPEG: height and width must be multiples of 16 (4:2:0 macroblocks), got {height} x {width}")
        self.shape = init_images.shape
        self.factor = float(factor)
        self.ycbcr = nn.ParameterList([nn.Parameter(parameter) for parameter in self.encode(init_images)])

    def synthesize(self, _=None):
        return self.decode(self.ycbcr)

    @torch.no_grad()
    def encode(self, image):
        """(y, cb, cr) of ``image`` brought to the drawer's size with F.interpolate's bilinear rule (skipped at that size already), with
        the reference's cubic rounding.  Runs under no_grad: upstream's compress_jpeg could be differentiated, but nothing does -- it only
        builds initial parameters -- so no encoder gradient exists here."""
        image = image.detach().float().contiguous()
        if tuple(image.shape[-2:]) != tuple(self.shape[-2:]):
            image = _bilinear(image, tuple(self.shape[-2:]))
        return jpeg_encode(image, self.factor)

    def decode(self, ycbcr):
        y, cb, cr = ycbcr
        return jpeg_decode_autograd(y, cb, cr, int(self.shape[-2]), int(self.shape[-1]), self.factor)
