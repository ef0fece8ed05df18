"""losses.tower_loss_and_grad — any number of embedding losses on ONE image tower for one tower pass.

The reference runs the tower once per loss object.  The tower's input gradient is linear in dL/d(embedding), so the terms'
embedding gradients are added and pushed through a single backward: one ``engine.forward(save=True)``, one ``engine.backward``.
"""
from __future__ import annotations

import torch

from .open_clip import _TowerLoss


@torch.no_grad()
def tower_loss_and_grad(images, terms, n_total=None):
    """(total loss, d total / d images, [per-term losses]) for ``terms``: losses.CLIP / OpenCLIP / SimulacraAesthetic /
    AestheticVisualAssessment objects whose ``.model`` is the same tower object.  Per-term losses are what each term's own
    ``loss_and_grad`` returns (same bits); the embedding gradients are summed in term order.  ``n_total`` as there."""
    terms = list(terms)
    if not terms:
        raise ValueError("tower_loss_and_grad needs at least one term")
    for t in terms:
        if not isinstance(t, _TowerLoss):
            raise TypeError(f"{type(t).__name__} is no embedding loss (CLIP, OpenCLIP, SimulacraAesthetic, AestheticVisualAssessment)")
    model = terms[0].model
    if any(t.model is not model for t in terms[1:]):
        raise ValueError("tower_loss_and_grad: every term must hold the same tower object as .model (build the terms with model=)")
    eng = model._need_engine()
    emb = eng.forward(images.to(model.device), save=True).contiguous()
    losses, total, demb = [], None, None
    for t in terms:
        loss, d = t._embedding_loss_and_grad(emb, n_total)
        losses.append(loss)
        total = loss if total is None else total + loss
        demb = d if demb is None else demb + d
    return total, eng.backward(demb), losses
