"""Image space [0, 1] <-> model space [-1, 1] (perceptor/models/monster_diffusion/standardize.py).  Device tensors go through the
pmi_lincomb2 kernel; host tensors (the static helpers random_noise / diffuse on CPU inputs) and tensors that carry an autograd graph
(MonsterDiffusion(input_grad=True): the kernel would drop it) are torch arithmetic."""
import torch

from ...engine import sampler


def _kernel(x):
    return x.is_cuda and not (torch.is_grad_enabled() and x.requires_grad)


def encode(x):
    return sampler.lincomb2(x, 2.0, cc=-1.0) if _kernel(x) else x.mul(2).sub(1)


def decode(x):
    return sampler.lincomb2(x, 0.5, cc=0.5) if _kernel(x) else x.add(1).div(2)
