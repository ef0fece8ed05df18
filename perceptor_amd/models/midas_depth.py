"""MiDaS depth -- drop-in for perceptor.models.MidasDepth (perceptor/models/midas_depth/midas_depth.py:30-128): relative inverse depth of
an image from DPT-Large, differentiable to the image.

Call surface of the reference: ``MidasDepth(name="dpt_large", optimize=True)`` and ``forward(images) -> -depth[:, None]``, fp32
[N, 1, 384, 384]: the images are resized to ``image_size`` and normalised with mean 0.5 / std 0.5 inside the engine
(perceptor_amd.engine.dpt.DptEngine).  The output is an autograd.Function over the engine, so ``depths.mean().backward()`` fills
``images.grad`` as in the reference's own test.  ``optimize`` (channels-last + half on CUDA in the reference) is accepted and ignored:
``dtype`` decides the precision here.

Only ``dpt_large`` is available.  The other five names of the reference build their backbones from timm (``vit_base_resnet50_384``) or
torch.hub (``resnext101_32x8d_wsl``, ``tf_efficientnet_lite3``): those are neither in the reference tree nor installed, so they raise
NotImplementedError.

Not available here: the pretrained weights (no network).  ``weights="synthetic"`` gives deterministic offline weights; ``checkpoint=``
takes the reference's file (base_model.py: a state dict, or ``{"model": state dict, "optimizer": ...}``) with the reference's keys.
"""
from __future__ import annotations

from typing import Optional

import torch

from ..engine import dpt as E
from ..utils.param_tree import ParamTree
from ..utils.synth import synth_state_dict

UNAVAILABLE = {
    "dpt_hybrid": "its backbone is timm's vit_base_resnet50_384 (a ResNetV2 stem under the ViT)",
    "dpt_hybrid_nyu": "its backbone is timm's vit_base_resnet50_384 (a ResNetV2 stem under the ViT)",
    "dpt_hybrid_kitti": "its backbone is timm's vit_base_resnet50_384 (a ResNetV2 stem under the ViT)",
    "midas_v21": "its backbone is torch.hub's facebookresearch/WSL-Images resnext101_32x8d_wsl",
    "midas_v21_small": "its backbone is torch.hub's rwightman/gen-efficientnet-pytorch tf_efficientnet_lite3",
}


class _Depth(torch.autograd.Function):
    """forward / backward are the HIP engine's (cf. owlvit._Logits)"""

    @staticmethod
    def forward(ctx, images, model):
        eng = model.engine
        out = eng.forward(images, save=True)
        ctx.model, ctx.saved_state = model, eng.saved
        return out

    @staticmethod
    def backward(ctx, grad_out):
        eng = ctx.model.engine
        eng.saved = ctx.saved_state
        return eng.backward(grad_out.float().contiguous() * eng.gscale), None


class MidasDepth(torch.nn.Module):
    def __init__(self, name="dpt_large", optimize=True, *, weights="synthetic", checkpoint: Optional[str] = None, dtype="bf16", seed: int = 0,
                 config: Optional[tuple] = None):
        """
        Args:
            name (str): "dpt_large" (the other names of the reference raise NotImplementedError: module doc)
            optimize (bool): accepted and ignored (dtype decides the precision)
            weights (str): "synthetic" for deterministic offline weights, or "dpt_large" with checkpoint=
            checkpoint (str): the reference's checkpoint file (a state dict or {"model": state dict, ...})
            dtype (str): "bf16" (default) or "f16", the type the network multiplies in
            config: (res, patch, width, layers, heads, hooks, reassemble channels, features) for toy sizes
        """
        super().__init__()
        if name in UNAVAILABLE:
            raise NotImplementedError(f"MidasDepth('{name}'): {UNAVAILABLE[name]}, which is neither in the reference tree nor installed; "
                                      "only 'dpt_large' is available")
        if name != "dpt_large":
            raise ValueError(f"midas_model_type '{name}' not implemented")
        if dtype not in ("bf16", "f16", "fp16"):
            raise ValueError(f"Invalid dtype: {dtype} (the HIP network multiplies in 'bf16' or 'f16')")
        self.name, self.optimize = name, optimize
        self.cfg = tuple(config) if config is not None else E.DPT_CONFIGS[name]
        E.check_config(self.cfg)
        self.precision = "bf16" if dtype == "bf16" else "f16"
        if checkpoint is not None:
            sd = torch.load(checkpoint, map_location="cpu", weights_only=True)
            if "optimizer" in sd:                                   # base_model.py:12-13
                sd = sd["model"]
            sd = {k: v.float() for k, v in E.check_state_dict(sd, self.cfg).items()}
        elif weights == "synthetic":
            shapes = E.dpt_state_dict_shapes(self.cfg)
            sd = {k: v.reshape(shapes[k]) for k, v in synth_state_dict(shapes, seed).items()}
        else:
            raise RuntimeError(f"pretrained weights MidasDepth/{weights} cannot be downloaded (no network): pass checkpoint= (the reference's "
                               "checkpoint file) or weights='synthetic'")
        self.weights = weights
        self.model = ParamTree(sd)                 # the reference holds DPTDepthModel as self.model (midas_depth.py:50)
        self.net_w = self.net_h = self.cfg[0]
        self.image_size = (self.net_h, self.net_w)
        self._engine: Optional[E.DptEngine] = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_engine", None))

    @property
    def device(self):
        return next(iter(self.parameters())).device

    @property
    def engine(self) -> E.DptEngine:
        if self.device.type != "cuda":
            raise RuntimeError("MidasDepth needs a HIP device: call .to('cuda') first (perceptor_amd has no CPU fallback)")
        if self._engine is None:
            self._engine = E.DptEngine(self.cfg, self.model.state_dict(), self.device, self.precision)
        return self._engine

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)

    def forward(self, images: torch.Tensor) -> torch.Tensor:
        """images NCHW in [0, 1], any size -> -depth[:, None], fp32 [N, 1, image_size]"""
        if not images.is_cuda:
            raise RuntimeError("MidasDepth runs on a HIP device only (no CPU fallback)")
        if images.requires_grad and torch.is_grad_enabled():
            return _Depth.apply(images, self)
        return self.engine.forward(images)
