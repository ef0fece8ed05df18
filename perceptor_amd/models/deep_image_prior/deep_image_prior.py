"""models.DeepImagePrior (perceptor/models/deep_image_prior/deep_image_prior.py): a picture as the output of a small skip network whose
WEIGHTS the optimiser moves.

The module tree below only HOLDS the state: it is laid out as upstream's get_hq_skip_net(offset_type="none") numbers its modules, so
state_dict() carries the reference's key names, shapes and dtypes (a reference state dict loads with strict=True and the reverse), and the
parameters are ordinary fp32 nn.Parameters initialised by torch's own Conv2d / BatchNorm2d rules.  forward() does not run these modules: it
hands the live parameters to engine.dip.DIPEngine (HIP kernels, training-mode BatchNorm) through one autograd.Function whose backward fills
every parameter's .grad in fp32 and in PyTorch's layout -- any torch.optim optimiser works unchanged.

Refused loudly: deformable convolutions (offset_type other than "none" / None: torchvision.ops is absent), the other get_net families
(ResNet, UNet, texture_nets), resampling modes other than cubic, padding other than reflection, a backward in eval mode, double backward.
"""
import numpy as np
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from ...engine import dip

DEFAULT_SIZE = 256
DEFAULT_SHAPE = (128, DEFAULT_SIZE, DEFAULT_SIZE)


class _Holder(nn.Module):
    """A module of the reference tree that owns one buffer (the resamplers' `kernel`, the colour matrix) and is never called."""

    def __init__(self, name, value):
        super().__init__()
        self.register_buffer(name, value)


def _tree(children):
    s = nn.Sequential()
    for key, module in children:
        s.add_module(key, module)
    return s


def _conv(cin, cout, k, down=False):
    layers = [("0", nn.ReflectionPad2d((k - 1) // 2)), ("1", nn.Conv2d(cin, cout, k))]
    if down:
        layers.append(("2", _Holder("kernel", dip.cubic_kernels()[0])))
    return _tree(layers)


def _act():
    return nn.LeakyReLU(0.2, inplace=True)


def _scale(i, n_scales, cin):
    """One scale as upstream's skip() numbers it (its `add` names a child len + 1, so keys start at 1)."""
    w, s = dip.WIDTH, dip.SKIP
    deeper = [("1", _conv(cin, w, 3, down=True)), ("2", nn.BatchNorm2d(w)), ("3", _act()),
              ("4", _conv(w, w, 3)), ("5", nn.BatchNorm2d(w)), ("6", _act())]
    if i < n_scales - 1:
        deeper.append(("7", _tree(_scale(i + 1, n_scales, w))))
    deeper.append((str(len(deeper) + 1), _Holder("kernel", dip.cubic_kernels()[1])))
    skip = [("1", _conv(cin, s, 1)), ("2", nn.BatchNorm2d(s)), ("3", _act())]
    concat = _tree([("0", _tree(skip)), ("1", _tree(deeper))])
    return [("1", concat), ("2", nn.BatchNorm2d(s + w)), ("3", _conv(s + w, w, 3)), ("4", nn.BatchNorm2d(w)), ("5", _act()),
            ("6", _conv(w, w, 1)), ("7", nn.BatchNorm2d(w)), ("8", _act())]


class _Run(torch.autograd.Function):
    @staticmethod
    def forward(ctx, model, latents, *params):
        P = model._live()
        tape = {"latent_grad": latents.requires_grad} if model.training else None
        if tape is None and torch.is_grad_enabled() and (latents.requires_grad or any(p.requires_grad for p in params)):
            ctx.eval_mode = True
            out = model.engine.forward(latents, P, train=False)
        else:
            ctx.eval_mode = False
            out = model.engine.forward(latents, P, train=True, tape=tape) if model.training else model.engine.forward(latents, P, train=False)
        ctx.model, ctx.tape, ctx.names = model, tape, [k for k, _ in model.named_parameters()]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out):
        if ctx.eval_mode or ctx.tape is None:
            raise NotImplementedError("DeepImagePrior: no backward in eval mode (the forward ran on the running statistics); call .train()")
        grads, dlat = ctx.model.engine.backward(ctx.tape, d_out, ctx.model._live())
        ctx.tape = None
        return (None, dlat if ctx.needs_input_grad[1] else None) + tuple(
            grads[k] if ctx.needs_input_grad[2 + i] else None for i, k in enumerate(ctx.names))


class DeepImagePrior(nn.Module):
    def __init__(self, shape=DEFAULT_SHAPE, offset_type="none", n_scales=2, sigmoid=True, decorrelate_rgb=True, output_channels=3,
                 dtype="bf16"):
        """
        Represent image with latent and deep image prior network.

        Args:
            shape: (number of latent input channels, height, width)
            offset_type: "none" (or None); the deformable variants "1x1" and "full" need torchvision.ops and are refused
            n_scales: number of up-downscales
            sigmoid: whether to use sigmoid activation
            decorrelate_rgb: whether to decorrelate the RGB channels
            output_channels: number of output channels
            dtype: the activations' 16-bit type, "bf16" or "f16" (parameters, statistics and gradients are fp32)
        """
        super().__init__()
        input_channels, height, width = shape
        assert height == width
        assert height % 8 == 0
        if offset_type not in ("none", None):
            raise NotImplementedError(f"DeepImagePrior(offset_type={offset_type!r}): deformable convolutions need torchvision.ops, which is "
                                      "absent; only offset_type='none' is implemented")
        if n_scales is None or int(n_scales) < 1:
            raise ValueError("DeepImagePrior: n_scales must be an integer of at least 1")
        dip.check_size(int(n_scales), height, width)
        self.shape = shape
        self.n_scales = int(n_scales)
        self.output_channels = output_channels
        self.engine = dip.DIPEngine(self.n_scales, input_channels, output_channels, sigmoid, decorrelate_rgb, dtype)
        layers = _scale(0, self.n_scales, input_channels) + [("9", _conv(dip.WIDTH, output_channels, 1))]
        if decorrelate_rgb:
            layers.append(("10", _Holder("colcorr_t", dip.colcorr_t())))
        if sigmoid:
            layers.append((str(len(layers) + 1), nn.Sigmoid()))
        self.network = _tree(layers)

    def _live(self):
        P = dict(self.named_parameters())
        P.update(self.named_buffers())
        return P

    @property
    def device(self):
        return next(self.parameters()).device

    @property
    def input_channels(self):
        return self.shape[0]

    @property
    def height(self):
        return self.shape[1]

    @property
    def width(self):
        return self.shape[2]

    def forward(self, latents):
        """latents [N, C, H, W] fp32 on a HIP device -> [N, output_channels, H, W] fp32 with a grad_fn.  Training mode (the default): batch
        statistics, running statistics updated.  .eval(): the running statistics; its backward raises NotImplementedError."""
        if not torch.is_tensor(latents) or latents.dim() != 4:
            raise ValueError("DeepImagePrior: latents must be a [N, C, H, W] tensor")
        if tuple(latents.shape[1:]) != tuple(self.shape):
            raise ValueError(f"DeepImagePrior: latents of shape {tuple(latents.shape)} do not match the model's (N, {', '.join(map(str, self.shape))})")
        return _Run.apply(self, latents, *self.parameters())

    def random_latents(self, size=1, n_channels=None):
        if n_channels is None:
            n_channels = self.input_channels
        return 0.1 * torch.randn((size, n_channels, self.height, self.width), device=self.device)

    def fourier_latents(self, size=1, n_channels=None, min_log2_frequency=0.0, max_log2_frequency=9.0, log2_space=False):
        if n_channels is None:
            n_channels = self.input_channels
        assert n_channels % 4 == 0
        xs = torch.linspace(-1, 1, self.shape[2])
        ys = torch.linspace(-1, 1, self.shape[1])
        meshgrid = torch.stack(torch.meshgrid(xs, ys, indexing="ij"), dim=0)
        if log2_space:
            frequencies = 2.0 ** torch.linspace(min_log2_frequency, max_log2_frequency, steps=n_channels // 4)
        else:
            frequencies = torch.linspace(2.0 ** min_log2_frequency, 2.0 ** max_log2_frequency, steps=n_channels // 4)
        phases = meshgrid[None] * frequencies[:, None, None, None] * 2 * np.pi
        fourier_latents = torch.cat([torch.sin(phases), torch.cos(phases)], dim=0).flatten(end_dim=1)[None]
        return fourier_latents.to(self.device).repeat(size, 1, 1, 1).mul(0.3)

    def noisy_image_latents(self, images, n_channels=None, log_snr=-1.0):
        if n_channels is None:
            n_channels = self.input_channels
        sigma = 1 / (torch.as_tensor(log_snr).exp().sqrt() + 1)
        channels = images.shape[1]
        repeated_images = torch.stack([images[:, index % channels] for index in range(n_channels)], dim=1)
        return 0.1 * (repeated_images.mul(2).sub(1) * (1 - sigma) + torch.randn_like(repeated_images) * sigma)

    def offset_parameters(self):
        return [p for n, p in self.network.named_parameters() if "offset_branch" in n]

    def non_offset_parameters(self):
        return [p for n, p in self.network.named_parameters() if "offset_branch" not in n]

    def parameter_dicts(self, learning_rate):
        return [dict(params=self.offset_parameters(), lr=learning_rate * 0.1), dict(params=self.non_offset_parameters(), lr=learning_rate)]
