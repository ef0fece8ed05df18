"""perceptor.drawers: image parameterisations whose ``synthesize()`` is the picture the losses score.

Raw holds the pixels, JPEG the quantised DCT coefficients behind a differentiable decoder (csrc/jpeg.hip), DeepImagePrior the weights of a
skip network trained through HIP weight gradients (csrc/dip.hip).  The reference's other drawers (BruteDiffusion, BruteRuDalle, StyleGANXL)
need sampling loops through a trained network or packages that are absent and are not provided.
"""
from .interface import DrawingInterface
from .raw import Raw
from .jpeg import JPEG
from .deep_image_prior import DeepImagePrior
