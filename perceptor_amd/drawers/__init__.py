"""perceptor.drawers: image parameterisations whose ``synthesize()`` is the picture the losses score.

Raw holds the pixels, JPEG the quantised DCT coefficients behind a differentiable decoder (csrc/jpeg.hip).  The reference's other drawers
(DeepImagePrior, BruteDiffusion, BruteRuDalle, StyleGANXL) need training-mode networks or packages that are absent and are not provided.
"""
from .interface import DrawingInterface
from .raw import Raw
from .jpeg import JPEG
