"""losses.LPIPS — drop-in for perceptor/losses/lpips.py: the learned perceptual image patch similarity of the ``lpips`` package
(0.1.x, version '0.1') between two image batches in [0, 1], ``lpips.LPIPS(net=name, lpips=linear_layers, spatial=spatial)(a, b,
normalize=True)``, differentiable to either image (engine/lpips.py has the definition).

Deviations from the reference, all deliberate:
  * only ``name="vgg"`` runs here, and it is the default (the reference's default is "squeeze").  "alex" needs 11x11 stride-4 and 5x5
    convolutions, "squeeze" an unpadded 3x3 stride-2 stem and a 3x3 stride-2 ceil-mode max pool; pmi_igemm has no route for either (taps
    1 / 9 / 16, symmetric padding only).  Both raise a ValueError that says so.
  * images run at their own size and need height and width divisible by 16.
  * at a pixel whose features are all zero torch's autograd yields NaN; the gradient here is 0.

``self.model`` is a parameter container whose ``state_dict`` has the lpips package's keys ("net.slice{1..5}.{torchvision index}.weight" /
".bias", "lin{0..4}.model.1.weight", the buffers "scaling_layer.shift" / "scaling_layer.scale"), so an upstream state dict loads with
``load_state_dict``; the arithmetic runs in the HIP engine, packed on first use on the module's device.  Neither the ImageNet VGG-16
checkpoint nor the package's v0.1/vgg.pth is reachable here: pass ``checkpoint=`` (a whole lpips state dict), ``features_checkpoint=``
(a torchvision vgg16 state dict) and / or ``linear_checkpoint=`` (v0.1/vgg.pth), or get deterministic synthetic weights (convolutions as
models.VGG19, gain sqrt(2); lin weights non-negative with mean 1 / C).  Whether real VGG-16 activations stay inside the f16 range has
not been measured: ``dtype="bf16"`` is the safe choice for a real checkpoint until it has.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import nn

from ..engine import lpips as lpips_engine
from ..engine.vgg import conv_indices, map_state_dict, vgg_state_dict_shapes
from ..utils.synth import synth_state_dict, synth_tensor
from .open_clip import LossInterface

_UNSUPPORTED = {
    "alex": "it needs 11x11 stride-4 and 5x5 convolutions",
    "squeeze": "it needs an unpadded 3x3 stride-2 stem convolution and a 3x3 stride-2 ceil-mode max pool",
}


class _ScalingLayer(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor(lpips_engine.SHIFT)[None, :, None, None])
        self.register_buffer("scale", torch.tensor(lpips_engine.SCALE)[None, :, None, None])


class _NetLinLayer(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.model = nn.Sequential(nn.Dropout(), nn.Conv2d(c, 1, 1, bias=False))


class _Vgg16(nn.Module):
    """slice1 .. slice5 with torchvision's ``features`` indices as module names, as lpips.pretrained_networks.vgg16."""

    def __init__(self, widths):
        super().__init__()
        table = lpips_engine.lpips_layer_table(widths)
        for k, (lo, hi) in enumerate(lpips_engine.SLICES):
            seq = nn.Sequential()
            for i in range(lo, hi):
                l = table[i]
                seq.add_module(str(i), nn.Conv2d(l[1], l[2], 3, padding=1) if l[0] == "conv" else nn.ReLU() if l[0] == "relu" else nn.MaxPool2d(2, 2))
            setattr(self, f"slice{k + 1}", seq)


class _LpipsNet(nn.Module):
    def __init__(self, widths):
        super().__init__()
        self.scaling_layer = _ScalingLayer()
        self.net = _Vgg16(widths)
        for k, c in enumerate(widths):
            setattr(self, f"lin{k}", _NetLinLayer(c))


def conv_key(i: int) -> str:
    """The lpips key prefix of torchvision's ``features.{i}``."""
    for k, (lo, hi) in enumerate(lpips_engine.SLICES):
        if lo <= i < hi:
            return f"net.slice{k + 1}.{i}"
    raise ValueError(f"module {i} is outside the LPIPS tower")


def features_to_lpips_keys(sd, widths):
    """A torchvision vgg16 state dict (keys "features.{i}.*" or "{i}.*"; the classifier is ignored) under the lpips package's names."""
    flat = map_state_dict(sd, widths, lpips_engine.VGG16_DEPTHS)
    return {f"{conv_key(int(k.split('.')[0]))}.{k.split('.')[1]}": v for k, v in flat.items()}


def synthetic_state_dict(widths, seed=0):
    """Deterministic weights under the lpips package's keys: convolutions as models.VGG19 (gain sqrt(2)), lin weights |z| / mean|z| / C
    (non-negative, mean 1 / C)."""
    sd = features_to_lpips_keys(synth_state_dict(vgg_state_dict_shapes(widths, lpips_engine.VGG16_DEPTHS), seed, gain=2 ** 0.5), widths)
    for k, c in enumerate(widths):
        z = synth_tensor(f"lin{k}.model.1.weight.z", (c,), seed).abs().double()
        sd[f"lin{k}.model.1.weight"] = (z / z.mean() / c).float().view(1, c, 1, 1)
    return sd


class _LpipsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, images_a, images_b, module):
        eng = module._need_engine()
        need_a, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        out, state = eng.forward_levels(images_a.detach(), images_b.detach(), module.spatial, keep_tape_b=need_b)
        ctx.spatial = module.spatial
        if module.spatial:
            ctx.eng, ctx.state = eng, state                       # the tape waits for backward's grad_out
        elif need_a or need_b:
            grads = eng.backward(state, None, need_a, need_b)     # samples do not mix: per-sample gradients now, scaled by grad_out[n] later
            ctx.save_for_backward(*[g for g in grads if g is not None])
        ctx.which = (need_a, need_b)
        return out.clone()

    @staticmethod
    def backward(ctx, grad_out):
        need_a, need_b = ctx.which
        if ctx.spatial:
            state, ctx.state = ctx.state, None
            if state is None:
                raise RuntimeError("LPIPS(spatial=True): backward ran twice (the tape is released after the first)")
            ga, gb = ctx.eng.backward(state, grad_out, need_a, need_b)
            return ga, gb, None
        saved = list(ctx.saved_tensors)
        ga = saved.pop(0) * grad_out if need_a else None
        gb = saved.pop(0) * grad_out if need_b else None
        return ga, gb, None


class LPIPS(LossInterface):
    def __init__(self, name="vgg", linear_layers=True, spatial=False, *, weights="synthetic", checkpoint: Optional[str] = None,
                 features_checkpoint: Optional[str] = None, linear_checkpoint: Optional[str] = None, dtype="f16", seed: int = 0,
                 widths=None):
        """LPIPS perceptual loss.

        Args:
            name: "vgg" (the only backbone with a kernel route here; "alex" and "squeeze" raise)
            linear_layers: use the learned non-negative 1x1 weights (False: plain sum over channels)
            spatial: return a [N, 1, H, W] distance map instead of [N, 1, 1, 1]
            weights / seed: "synthetic" deterministic weights; checkpoint: a whole lpips state dict; features_checkpoint: a torchvision
            vgg16 state dict; linear_checkpoint: the package's v0.1/vgg.pth; dtype: "f16" (default) or "bf16"
            widths: the tower's channel widths (for tests; the product is VGG-16's)
        """
        super().__init__()
        if name in _UNSUPPORTED:
            raise ValueError(f"LPIPS(name={name!r}) is not available: {_UNSUPPORTED[name]}, and pmi_igemm has no route for that (taps 1 / 9 / "
                             "16, symmetric padding only); use name='vgg'")
        if name != "vgg":
            raise ValueError(f"LPIPS: unknown backbone {name!r} (only 'vgg' runs here)")
        if dtype not in ("f16", "bf16"):
            raise ValueError("LPIPS runs in 'f16' or 'bf16'")
        self.name, self.linear_layers, self.spatial, self.dtype = name, bool(linear_layers), bool(spatial), dtype
        self.widths = tuple(int(w) for w in widths) if widths is not None else lpips_engine.VGG16_WIDTHS
        if len(self.widths) != 5 or any(w <= 0 or w % 16 or w > 512 for w in self.widths):
            raise ValueError(f"unsupported LPIPS widths {self.widths}: five widths, each a multiple of 16 and at most 512, are required")
        self.model = _LpipsNet(self.widths)
        if weights == "synthetic":
            sd = synthetic_state_dict(self.widths, seed)
        elif checkpoint is None and (features_checkpoint is None or (self.linear_layers and linear_checkpoint is None)):
            raise ValueError(f"LPIPS: weights {weights!r} are not reachable here: pass checkpoint=, or features_checkpoint= and "
                             "linear_checkpoint=, or weights='synthetic'")
        else:
            sd = {}
        load = lambda path: torch.load(path, map_location="cpu", weights_only=True)
        if checkpoint is not None:
            sd.update(load(checkpoint))
        if features_checkpoint is not None:
            sd.update(features_to_lpips_keys(load(features_checkpoint), self.widths))
        if linear_checkpoint is not None:
            sd.update(load(linear_checkpoint))
        own = self.model.state_dict()
        sd = {k: v for k, v in sd.items() if not k.startswith("lins.")}      # newer lpips releases list the lins a second time
        for k in ("scaling_layer.shift", "scaling_layer.scale"):
            sd.setdefault(k, own[k])
        if not self.linear_layers:
            for k in own:
                if k.startswith("lin"):
                    sd.setdefault(k, torch.ones_like(own[k]))
        self.model.load_state_dict(sd)
        self.model.eval()
        self.model.requires_grad_(False)
        self._engine = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_engine", None))

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)

    @property
    def device(self):
        return self.model.scaling_layer.shift.device

    def _need_engine(self) -> lpips_engine.LpipsEngine:
        if self._engine is None:
            if self.device.type != "cuda":
                raise RuntimeError("LPIPS needs a HIP device: call .to('cuda') first (perceptor_amd has no CPU fallback)")
            sd = self.model.state_dict()
            feats = {}
            for i in conv_indices(self.widths, lpips_engine.VGG16_DEPTHS):
                for leaf in ("weight", "bias"):
                    feats[f"{i}.{leaf}"] = sd[f"{conv_key(i)}.{leaf}"]
            lins = [sd[f"lin{k}.model.1.weight"] for k in range(5)] if self.linear_layers else None
            if lins is not None and any(bool((l < 0).any()) for l in lins):
                raise ValueError("LPIPS: the lin weights must be non-negative")
            self._engine = lpips_engine.LpipsEngine(self.widths, feats, lins, self.device, self.dtype, sd["scaling_layer.shift"],
                                                    sd["scaling_layer.scale"])
        return self._engine

    def _check(self, images_a, images_b):
        for t in (images_a, images_b):
            if not t.is_cuda:
                raise RuntimeError("LPIPS runs on a HIP device only (no CPU fallback)")
        if tuple(images_a.shape) != tuple(images_b.shape):
            raise ValueError(f"LPIPS needs images of equal shape, got {tuple(images_a.shape)} and {tuple(images_b.shape)}")

    @torch.no_grad()
    def targets(self, images_b, keep_tape=False):
        """The five cached 16-bit feature maps of a fixed ``images_b``: a guidance step against them costs one tower pass."""
        if not images_b.is_cuda:
            raise RuntimeError("LPIPS runs on a HIP device only (no CPU fallback)")
        return self._need_engine().targets(images_b, keep_tape=keep_tape)

    def forward(self, images_a, images_b):
        self._check(images_a, images_b)
        return _LpipsFn.apply(images_a, images_b, self)

    @torch.no_grad()
    def loss_and_grad(self, images_a, images_b_or_targets, grad_out=None, grad_b=False):
        """(output, dL/dimages_a[, dL/dimages_b]) with L = sum(grad_out * output) (grad_out: the output's shape, default ones), without
        autograd.  The second argument is an image batch (it runs with ``images_a`` as one 2N tower pass) or what ``targets`` returned
        (``images_a`` runs alone: another batch route, so the same features up to rounding, not necessarily the same bits)."""
        b = images_b_or_targets
        if not isinstance(b, dict):
            self._check(images_a, b)
        elif not images_a.is_cuda:
            raise RuntimeError("LPIPS runs on a HIP device only (no CPU fallback)")
        return self._need_engine().loss_and_grad(images_a, b, grad_out=grad_out, grad_b=grad_b, spatial=self.spatial)
