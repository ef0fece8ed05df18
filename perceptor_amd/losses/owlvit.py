"""losses.OWLViT -- drop-in for perceptor/losses/owlvit.py:9-79: steer a sample towards containing ONE instance of each text query somewhere
in the picture.

loss = -0.01 sum_q w_q mean_{n, the top_k tokens p} log_softmax_p(logits[n, :, q]): per query, the log-softmax over the patch tokens says
where the query is found, and the mean of its ``top_k`` largest values rewards a few tokens that stand out.  Where every CLIP loss here
scores the pooled embedding, this one scores every patch token.

``forward(images, top_k=5)`` keeps the reference contract (a scalar you can ``.backward()`` when ``images.requires_grad``);
``loss_and_grad(images, top_k=5)`` is the fused path the other losses offer: engine forward without the box head -> pmi_owl_topk_loss (the
loss and dloss/dlogits in one launch) -> engine backward.
"""
from __future__ import annotations

import torch

from .. import models
from .open_clip import LossInterface


class OWLViT(LossInterface):
    def __init__(self, **kw):
        """
        OWL-ViT zero-shot text-conditioned bounding box model.

        Loss is designed in such a way that only one example of the text prompt
        is expected to be found in the image.  Keyword arguments go to models.OWLViT.
        """
        super().__init__()
        self.model = models.OWLViT(**kw)
        self.encodings = None
        self.weights = None

    @property
    def device(self):
        return self.model.device

    def to(self, device):
        super().to(device)
        if self.encodings is not None:
            self.encodings.to(device)
        return self

    def add_texts_(self, texts, weights=None):
        return self.add_encodings_(self.model.encode_texts([list(texts)]), weights)

    def add_images_(self, images, weights=None):
        raise NotImplementedError()

    def add_encodings_(self, encodings, weights=None):
        if self.encodings is not None:
            raise ValueError("OWLViT can only have one set of encodings")
        n_q = encodings.batch_encoding["input_ids"].shape[0]
        if isinstance(weights, (list, tuple)):
            weights = torch.tensor(weights)
        elif weights is None:
            weights = torch.ones(len(encodings.texts))      # as the reference: one weight per inner list, so only the first query is scored
        weights = weights.detach().float().reshape(-1)
        if weights.shape[0] > n_q:
            raise ValueError(f"{weights.shape[0]} weights for {n_q} queries")
        # the reference's loss walks the WEIGHTS (losses/owlvit.py:69): a query past the last weight is not scored, i.e. weighs 0
        weights = torch.cat([weights, torch.zeros(n_q - weights.shape[0])])
        self.encodings = encodings
        self.weights = torch.nn.Parameter(weights.to(self.device), requires_grad=False)
        return self

    def _need_encodings(self):
        if self.encodings is None:
            raise RuntimeError("add_texts_ or add_encodings_ first")

    def forward(self, images, top_k=5):
        self._need_encodings()
        predictions = self.model(images, self.encodings)
        lsm = predictions.logits.log_softmax(dim=1)                           # over the patch tokens, per (image, query)
        top = lsm.topk(min(int(top_k), lsm.shape[1]), dim=1).values           # the reference's sort()[:, -top_k:]
        return -(top.mean(dim=(0, 1)) * self.weights).sum() * 0.01

    @torch.no_grad()
    def loss_and_grad(self, images, top_k=5):
        """(loss, dloss/dimages)"""
        self._need_encodings()
        eng = self.model.engine
        images = images.to(self.device)
        out = eng.forward(images, self.encodings.queries, save=True, boxes=False)
        loss, dlogits = eng.topk_loss(out["logits"], self.weights.data, int(top_k), eng.gscale)
        return loss, eng.backward(dlogits)
