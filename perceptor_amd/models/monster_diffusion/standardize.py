"""Image space [0, 1] <-> model space [-1, 1] (perceptor/models/monster_diffusion/standardize.py).  Device tensors go through the
pmi_lincomb2 kernel; host tensors (the static helpers random_noise / diffuse on CPU inputs) are host arithmetic."""
from ...engine import sampler


def encode(x):
    return sampler.lincomb2(x, 2.0, cc=-1.0) if x.is_cuda else x.mul(2).sub(1)


def decode(x):
    return sampler.lincomb2(x, 0.5, cc=0.5) if x.is_cuda else x.add(1).div(2)
