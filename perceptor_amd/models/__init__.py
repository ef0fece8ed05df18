"""Drop-in for ``perceptor.models`` on the guided-diffusion hot path."""
from .guided_diffusion import GuidedDiffusion
from .open_clip import CLIP, OpenCLIP
from .velocity_diffusion import VelocityDiffusion
from .stable_diffusion import StableDiffusion
from .transformers_openai_clip import TransformersOpenAICLIP
from .simulacra_aesthetic import SimulacraAesthetic
from .vgg import VGG19
from .super_resolution import SuperResolution
from .monster_diffusion import MonsterDiffusion
from .glide_clip import GlideCLIP
from .owlvit import OWLViT, OWLViTEncodings, OWLViTPredictions
from .deep_image_prior import DeepImagePrior
from .midas_depth import MidasDepth
