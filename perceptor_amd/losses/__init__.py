"""Drop-in for ``perceptor.losses`` on the guided-diffusion hot path."""
from .open_clip import CLIP, LossInterface, OpenCLIP
from .velocity_diffusion import VelocityDiffusion
from .aesthetic import AestheticVisualAssessment, SimulacraAesthetic
from .pixel import Resize, Smoothness
from .spherical_distance import SphericalDistance
from .shared_tower import tower_loss_and_grad
from .lpips import LPIPS
from .style_transfer import StyleTransfer
from .super_resolution import SuperResolution
from .owlvit import OWLViT
