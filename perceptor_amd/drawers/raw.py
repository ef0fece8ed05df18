"""drawers.Raw (perceptor/drawers/raw/raw.py): the pixels themselves are the parameter."""
from torch import nn

from ..transforms.resize import resize
from .init import fractal, gradient
from .interface import DrawingInterface


class Raw(DrawingInterface):
    def __init__(self, init_images):
        """Minimal container for an nn.Parameter with init helpers:  Raw.random_fractal_image((1, 3, 256, 256))"""
        super().__init__()
        self.images = nn.Parameter(init_images)

    def synthesize(self, _=None):
        return self.images

    def encode(self, images, mode="bilinear"):
        """``images`` resized to the parameter's size with the reference's resize (antialiased triangle kernel by default)."""
        return resize(images, out_shape=tuple(self.images.shape[-2:]), resample=mode)

    def replace_(self, images):
        self.images.data.copy_(images.data)
        return self

    @staticmethod
    def random_fractal_image(shape):
        return Raw(fractal(shape))

    @staticmethod
    def random_gradient_image(shape):
        return Raw(gradient(shape))
