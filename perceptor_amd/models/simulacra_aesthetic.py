"""models.SimulacraAesthetic — drop-in for perceptor/models/simulacra_aesthetic/simulacra_aesthetic.py:25-60.

A linear regression probe on a CLIP image tower: ``forward(images) -> [N, 1]`` ratings,
``linear(F.normalize(encode_images(images)) * sqrt(D))``.  The tower is this package's HIP engine
(models.CLIP); the head is a [1, D] matrix applied with torch on the tiny [N, D] embeddings, so a rating is
differentiable to the images through the engine's input gradient.

Not available here: the published probes (the reference downloads them).  ``checkpoint=`` reads a head file with the
reference's keys (``linear.weight``, ``linear.bias``); without one the head is deterministic synthetic (``seed=``).
"""
from __future__ import annotations

from typing import Optional

import torch

from ..utils.synth import synth_tensor
from . import open_clip

MODEL_NAMES = ("ViT-B-32", "ViT-B-16", "ViT-L-14", "RN50", "RN101", "RN50x4", "RN50x16", "RN50x64", "ViT-L-14-336")


def load_head(path: str, weight_key: str, bias_key: str, k: int, dim: int):
    """(weight [k, dim], bias [k]) fp32 from a head file (tensors only: weights_only=True)."""
    raw = torch.load(path, map_location="cpu", weights_only=True)
    if weight_key not in raw or bias_key not in raw:
        raise RuntimeError(f"{path}: expected the keys {weight_key!r} and {bias_key!r}, found {sorted(raw)}")
    w, b = raw[weight_key].detach().float(), raw[bias_key].detach().float()
    if tuple(w.shape) != (k, dim) or tuple(b.shape) != (k,):
        raise RuntimeError(f"{path}: head of shape {tuple(w.shape)} / {tuple(b.shape)} does not fit a [{k}, {dim}] probe")
    return w.contiguous(), b.contiguous()


def resolve_tower(model_name: str, model, kw):
    """The tower to put a head on: ``model`` (shared) or a new models.CLIP(model_name, **kw)."""
    if model is not None:
        if kw:
            raise TypeError(f"model= given: the tower arguments {sorted(kw)} have nothing to configure")
        if not isinstance(model, open_clip.OpenCLIP):
            raise TypeError("model= must be a models.CLIP / models.OpenCLIP")
        return model
    return open_clip.CLIP(model_name, **kw)


class SimulacraAesthetic(torch.nn.Module):
    def __init__(self, model_name="ViT-B-32", *, model=None, checkpoint: Optional[str] = None, seed: int = 0, **kw):
        """
        Args:
            model_name (str): name of the CLIP model (one of MODEL_NAMES, or any name registered through ``config=`` / ``rn_config=``)
            model: an existing models.CLIP / models.OpenCLIP to share (then ``model_name`` only labels the head)
            checkpoint: head file with ``linear.weight`` [1, D] and ``linear.bias`` [1]
            seed: seed of the synthetic head used when no checkpoint is given
            **kw: forwarded to models.CLIP (``weights="synthetic"``, ``config=``, ...)
        """
        super().__init__()
        self.model_name = model_name
        clip_model = resolve_tower(model_name, model, kw)
        dim = clip_model.output_dim
        self.linear = torch.nn.Linear(dim, 1)
        if checkpoint is not None:
            w, b = load_head(checkpoint, "linear.weight", "linear.bias", 1, dim)
        else:   # ratings around the middle of the 1-10 scale
            w = synth_tensor(f"simulacra.{model_name}.linear.weight", (1, dim), seed)
            b = 5.0 + synth_tensor(f"simulacra.{model_name}.linear.bias", (1,), seed)
        with torch.no_grad():
            self.linear.weight.copy_(w)
            self.linear.bias.copy_(b)
        self.linear.eval()
        self.linear.requires_grad_(False)
        self.clip_model = clip_model

    def forward(self, images):
        unit = self.clip_model.encode_images(images)      # unit rows already: the reference's second normalisation is the identity
        return self.linear(unit * float(unit.shape[1]) ** 0.5)
