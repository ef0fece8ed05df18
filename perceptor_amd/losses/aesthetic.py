"""losses.SimulacraAesthetic / losses.AestheticVisualAssessment — drop-ins for perceptor/losses/simulacra_aesthetic.py:8-41
and perceptor/losses/aesthetic_visual_assessment.py:10-51: a linear probe on a CLIP image tower's embedding.

``forward(images)`` keeps the reference contract (a scalar you can ``.backward()`` when ``images.requires_grad``): the tower through
``encode_images`` (the HIP engine's autograd function), the head with torch on the tiny [N, D] tensors.  ``loss_and_grad(images)`` is
the fused path: tower forward -> pmi_head_loss (loss + dL/d emb through F.normalize and the head) -> tower input gradient.
``.model`` is the tower (a models.CLIP / models.OpenCLIP), so several embedding losses on one tower can share a single pass
(losses.tower_loss_and_grad); the reference's ``loss.model`` of SimulacraAesthetic, the rating model, is ``.aesthetic_model`` here.

Not available here: the published heads (the reference downloads them): pass ``checkpoint=`` or get a deterministic synthetic head.
"""
from __future__ import annotations

from typing import Optional

import torch

from .. import models
from .._hip import call, ptr
from ..models import simulacra_aesthetic as _sa
from ..utils.synth import synth_tensor
from .open_clip import _TowerLoss

MODES = {"logit": 1, "expected": 2, "probability": 3}


class _HeadBase(_TowerLoss):
    """A [K, D] linear head on ``self.model``'s embedding; ``_head()`` gives (the nn.Linear, pmi_head_loss's mode, the target)."""

    def _head(self):
        raise NotImplementedError

    def _embedding_loss_and_grad(self, emb, n_total):
        lin, mode, target = self._head()
        n, dim = emb.shape
        k = lin.weight.shape[0]
        dev = emb.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        demb = torch.empty_like(emb)
        out = torch.empty((n, k), dtype=torch.float32, device=dev)      # the ratings / logits: written by the kernel, not used here
        partial = torch.empty(n, dtype=torch.float32, device=dev)
        w, b = lin.weight.data.float().contiguous(), lin.bias.data.float().contiguous()
        call("pmi_head_loss", ptr(emb), ptr(w), ptr(b), ptr(loss), ptr(demb), ptr(out), ptr(partial), n, k, dim, mode, float(target),
             int(n_total or n), float(self.multiplier), float(self.model._need_engine().gscale))
        return loss[0], demb


class SimulacraAesthetic(_HeadBase):
    def __init__(self, model_name="ViT-L-14", aesthetic_target=10, *, model=None, checkpoint: Optional[str] = None, seed: int = 0, **kw):
        """Squared distance between a rating probe's output (a [1, D] linear regression on the CLIP embedding, scale 1-10) and a wanted rating.

        Args:
            model_name (str): CLIP tower the probe was fitted on (models.simulacra_aesthetic.MODEL_NAMES)
            aesthetic_target (int): the rating to pull images towards
            model: an existing models.CLIP / models.OpenCLIP to put the probe on and share with other losses
            checkpoint: probe file (``linear.weight``, ``linear.bias``); seed: of the synthetic probe used otherwise
            **kw: forwarded to the tower (models.CLIP)

        Unlike the reference, ``self.model`` is the image TOWER (what losses.tower_loss_and_grad shares between terms), not a callable
        that returns ratings: a script that calls ``loss.model(images)`` must call ``loss.aesthetic_model(images)`` here.
        """
        super().__init__()
        self._target = float(aesthetic_target)      # host copy for the fused path: reading the Parameter back would sync the stream per call
        self.aesthetic_target = torch.nn.Parameter(torch.tensor(self._target), requires_grad=False)
        self.aesthetic_model = models.SimulacraAesthetic(model_name, model=model, checkpoint=checkpoint, seed=seed, **kw)
        self.model = self.aesthetic_model.clip_model
        self.multiplier = 1e-5 if model_name in ("ViT-L-14", "ViT-L-14-336") else 1e-3

    def _head(self):
        return self.aesthetic_model.linear, 0, self._target

    def forward(self, images):
        miss = self.aesthetic_model(images) - self.aesthetic_target             # [N, 1] ratings against the scalar target
        return miss.square().mean() * self.multiplier


class AestheticVisualAssessment(_HeadBase):
    CLASSES = 10        # the head scores the ratings 1 .. 10

    def __init__(self, aesthetic_target=10, mode="expected", *, model=None, checkpoint: Optional[str] = None, seed: int = 0, **kw):
        """A 10-way rating classifier on the CLIP ViT-B-16 embedding, turned into a loss in one of three ways.

        Args:
            aesthetic_target (int): the rating class (1-10) to pull images towards
            mode (str): "logit" (raise the target class's logit), "probability" (raise its softmax probability) or
                "expected" (squared distance of every probability-weighted rating p_k * k to the target)
            model: an existing models.CLIP / models.OpenCLIP to share (otherwise models.CLIP("ViT-B-16", **kw))
            checkpoint: head file (``weight`` [10, D], ``bias`` [10]); seed: of the synthetic head used otherwise
        """
        super().__init__()
        self.aesthetic_target = aesthetic_target
        self.mode = mode
        self.model = _sa.resolve_tower("ViT-B-16", model, kw)
        dim = self.model.output_dim
        self.aesthetic_head = torch.nn.Linear(dim, self.CLASSES)
        if checkpoint is not None:
            w, b = _sa.load_head(checkpoint, "weight", "bias", self.CLASSES, dim)
        else:   # logits of order 1 on a unit-norm embedding
            w = synth_tensor("ava.weight", (self.CLASSES, dim), seed, gain=float(dim) ** 0.5)
            b = synth_tensor("ava.bias", (self.CLASSES,), seed)
        with torch.no_grad():
            self.aesthetic_head.weight.copy_(w)
            self.aesthetic_head.bias.copy_(b)
        self.aesthetic_head.eval()
        self.aesthetic_head.requires_grad_(False)

    def _mode_code(self):
        if self.mode not in MODES:
            raise ValueError(f"AestheticVisualAssessment: mode {self.mode!r} is none of {sorted(MODES)}")
        return MODES[self.mode]

    def _head(self):
        return self.aesthetic_head, self._mode_code(), float(self.aesthetic_target)

    def forward(self, images):
        code = self._mode_code()
        logits = self.aesthetic_head(self.model.encode_images(images))           # [N, 10]
        cls = int(self.aesthetic_target) - 1
        if code == 1:
            return logits[:, cls].mean() * -0.01
        probs = logits.softmax(dim=1)
        if code == 3:
            return -probs[:, cls].mean()
        ratings = torch.arange(1, self.CLASSES + 1, device=probs.device, dtype=probs.dtype)
        return (probs * ratings - self.aesthetic_target).pow(2).mean() * 0.01    # each p_k * k on its own, as pmi_head_loss mode 2
