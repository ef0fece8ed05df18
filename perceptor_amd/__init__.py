"""perceptor_amd — MI355X-native guided-diffusion sampling hot path behind perceptor's Python surface.

    from perceptor_amd import models, losses, drawers     # instead of: from perceptor import models, losses, drawers
"""
from . import models  # noqa: F401  (first: losses imports models)
from . import losses, transforms, drawers  # noqa: F401

__version__ = "0.1.0"
