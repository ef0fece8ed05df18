"""losses.StyleTransfer — drop-in for perceptor/losses/style_transfer.py:10-68: an L1 loss on VGG-19 features (relu2_2, relu3_3,
relu4_2) and on their Gram matrices, against a style / init image.

``encode`` / ``loss`` / ``forward`` keep the reference's meaning (images in [0, 1] go in WITHOUT mean / std normalisation, resized to
256 x 256 when they are not that size); ``forward`` is a scalar that works with ``.backward()``; ``loss_and_grad`` is the fused path
without autograd.  With ``style_images`` the six encodings are kept as a frozen ParameterList, as upstream, and the engine-format
targets (16-bit features + fp32 Grams) are cached beside them, so a guidance step costs one tower pass.  The Gram matrix is taken over
[N C, H W]: it mixes the samples of the batch, so both sides need the same batch size and there is no ``n_total``.

``self.model`` is a models.VGG19 (the parameter container and the engine's owner).  The ImageNet checkpoint is not reachable here:
pass ``checkpoint=`` or get deterministic synthetic weights.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from .. import models
from .open_clip import LossInterface


class _StyleFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images_a, images_b, module):
        eng = module.model._need_engine()
        need_b = images_b is not None and ctx.needs_input_grad[1]
        tb = module._targets() if images_b is None else eng.targets(images_b.detach(), keep_tape=need_b)
        out = eng.loss_and_grad(images_a.detach(), tb, grad_b=need_b)
        ctx.save_for_backward(*out[1:])
        return out[0].clone()

    @staticmethod
    def backward(ctx, grad_out):
        g = ctx.saved_tensors
        ga = g[0] * grad_out if ctx.needs_input_grad[0] else None
        gb = g[1] * grad_out if len(g) > 1 else None
        return ga, gb, None


class StyleTransfer(LossInterface):
    def __init__(self, style_images=None, *, weights="synthetic", checkpoint: Optional[str] = None, dtype="f16", seed: int = 0,
                 size: int = 256, widths=None):
        """Original style transfer loss.

        Args:
            style_images: NCHW images in [0, 1] on a HIP device whose encodings every later call is compared with
            weights / checkpoint / seed: models.VGG19's; dtype: "f16" (default) or "bf16"
            size, widths: the tower's input size and channel widths (for tests; the product is 256 and VGG-19's widths)
        """
        super().__init__()
        self.model = models.VGG19(weights, checkpoint=checkpoint, dtype=dtype, seed=seed, size=size, widths=widths)
        self._cache = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_cache", None))
        if style_images is not None:
            self.model.to(style_images.device)
            self.encodings = nn.ParameterList([nn.Parameter(t, requires_grad=False) for t in self.encode(style_images)])

    def _apply(self, fn, *a, **k):
        self._cache = None
        return super()._apply(fn, *a, **k)

    @property
    def device(self):
        return self.model.device

    def _targets(self):
        """Engine-format targets of the stored encodings (``self.encodings`` missing: the reference's AttributeError)."""
        encodings = self.encodings
        if self._cache is None:
            self._cache = self.model._need_engine().targets_from_encodings(list(encodings))
        return self._cache

    @torch.no_grad()
    def encode(self, images):
        return self.model._need_engine().encode(images)

    @torch.no_grad()
    def loss(self, encodings_a, encodings_b):
        eng = self.model._need_engine()
        return eng.loss_value(eng.targets_from_encodings(list(encodings_a)), eng.targets_from_encodings(list(encodings_b)))

    def forward(self, images_a, images_b=None):
        if images_b is None:
            self.encodings                      # noqa: B018  (raises as upstream when no style images were given)
        return _StyleFn.apply(images_a, images_b, self)

    @torch.no_grad()
    def loss_and_grad(self, images_a, images_b=None):
        """(loss, dloss/dimages_a)."""
        if images_b is None:
            self.encodings                      # noqa: B018  (as forward)
        eng = self.model._need_engine()
        tb = self._targets() if images_b is None else eng.targets(images_b)
        return eng.loss_and_grad(images_a, tb)
