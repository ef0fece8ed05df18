"""losses.SphericalDistance — drop-in for perceptor/losses/spherical_distance.py:4-21: the mean squared great-circle distance between
the embeddings of two image batches on one tower, mean_{i,j} 2 asin(|e_a[i] - e_b[j]| / 2)^2.

``forward(images_a, images_b)`` differentiates to both arguments: two passes of the tower's autograd function, whose saved state is
per call.  ``loss_and_grad(images_a, images_b)`` is the fused path for the usual case of a fixed second batch: images_b is encoded
without saved state and serves as pmi_spherical_loss's targets (unit weights), then one tower input gradient for images_a.
"""
from __future__ import annotations

import torch

from .._hip import call, ptr
from .open_clip import LossInterface


class SphericalDistance(LossInterface):
    def __init__(self, model):
        super().__init__()
        self.model = model

    def forward(self, images_a, images_b):
        ea, eb = self.model.encode_images(images_a), self.model.encode_images(images_b)      # unit rows [Na, D], [Nb, D]
        chord = torch.cdist(ea, eb, compute_mode="donot_use_mm_for_euclid_dist")                                                          # |e_a[i] - e_b[j]|
        return (2 * torch.asin(chord / 2) ** 2).mean()

    @torch.no_grad()
    def loss_and_grad(self, images_a, images_b, n_total=None):
        """(loss, dloss/dimages_a).  ``n_total``: global size of the images_a batch when this rank holds a shard."""
        eng = self.model._need_engine()
        dev = self.model.device
        tgt = self.model.encode_images(images_b.to(dev)).contiguous()
        emb = eng.forward(images_a.to(dev), save=True).contiguous()
        n, dim = emb.shape
        k = tgt.shape[0]
        wts = torch.ones(k, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        demb = torch.empty_like(emb)
        call("pmi_spherical_loss", ptr(emb), ptr(tgt), ptr(wts), ptr(loss), ptr(demb), n, k, dim, int(n_total or n), 1.0, float(eng.gscale))
        return loss[0], eng.backward(demb)
