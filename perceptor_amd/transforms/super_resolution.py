"""transforms.SuperResolution — drop-in for perceptor/transforms/super_resolution.py:9-26: ``encode`` up-samples with
models.SuperResolution, ``decode`` resizes back with transforms.resize and its default method (lanczos3 when both sides shrink)."""
from __future__ import annotations

from torch import nn

from .resize import resize


class SuperResolution(nn.Module):
    def __init__(self, name="x4", half=False, **kwargs):
        super().__init__()
        from .. import models                      # (models imports transforms.resize: imported here, not at module load)
        self.name = name
        self.model = models.SuperResolution(name, half, **kwargs)

    def forward(self, images):
        return self.encode(images)

    def encode(self, images):
        return self.model.upsample(images)

    def decode(self, upsampled_images, size=None):
        if size is None:
            size = (upsampled_images.shape[-2] // self.model.scale, upsampled_images.shape[-1] // self.model.scale)
        size = (size, size) if isinstance(size, int) else tuple(int(s) for s in size)
        return resize(upsampled_images, out_shape=size)
