"""MonsterDiffusion -- drop-in for perceptor.models.MonsterDiffusion (perceptor/models/monster_diffusion/monster_diffusion.py:20-353):
a k-diffusion UNet under Karras et al.'s EDM parameterisation with the stochastic Heun ("elucidated") sampler and a linear multistep
sampler.  The network and the EDM algebra run in MonsterEngine (HIP); the sampler updates are the pmi_edm_* kernels."""
from __future__ import annotations

from typing import Optional

import torch

from ...engine import monster, sampler
from ..guided_diffusion.guided_diffusion import WeightStore
from . import diffusion, settings, standardize
from .prediction import PredictionBatch

_NAMES = ("all", "tiny-hero")          # the reference's two checkpoints: both the product config at 48 x 48


class _Denoised(torch.autograd.Function):
    """denoised_(diffused_images, ts, augmentations) with an input gradient, as autograd provides upstream (the network is an nn.Module
    there): forward and backward are MonsterEngine.forward_train / backward.  Weights are frozen; ts and the augmentations get no gradient
    (denoised_ refuses them when they ask for one)."""

    @staticmethod
    def forward(ctx, diffused_images, sigma, model, augmentations=None):
        denoised_xs, tape = model.engine.forward_train(diffused_images, sigma, augmentations)
        ctx.model, ctx.tape = model, tape
        return denoised_xs

    @staticmethod
    def backward(ctx, grad):
        m = ctx.model
        return m.engine.backward(ctx.tape, grad.contiguous(), m.network.state_dict()), None, None, None


class MonsterDiffusion(torch.nn.Module):
    def __init__(self, name="all", *, weights="synthetic", checkpoint: Optional[str] = None, dtype="bf16", seed=0, config=None,
                 input_grad: bool = False):
        """input_grad = True: an input that requires grad (under enabled grad) is evaluated with a tape and a loss on the predictions
        back-propagates to diffused_images (HIP backward, frozen weights); the default refuses such an input, as before."""
        super().__init__()
        self.input_grad = bool(input_grad)
        if name not in _NAMES:
            raise ValueError(f"Unknown model name {name}")
        self.name = name
        self.config = tuple(config) if config is not None else monster.product_config()
        monster.check_config(self.config)
        if config is None and self.config[4] != settings.N_AUGMENTATIONS:
            raise ValueError("the product config takes nine augmentation flags")
        self.compute_dtype = dtype
        shapes = monster.monster_state_dict_shapes(self.config)
        if checkpoint is not None:
            sd = monster.bare_state_dict({k: v.float() for k, v in torch.load(checkpoint, map_location="cpu", weights_only=True).items()})
        elif weights == "synthetic":
            sd = monster.synthetic_state_dict(self.config, seed)
        else:
            raise ValueError("weights must be 'synthetic' or a checkpoint path must be given (no network access)")
        monster.check_state_dict(self.config, sd)
        self.network = WeightStore({k: sd[k] for k in shapes})
        self._engine: Optional[monster.MonsterEngine] = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_engine", None))
        self.eval().requires_grad_(False)

    @property
    def engine(self) -> Optional[monster.MonsterEngine]:
        """Built on first use on a HIP device; dropped when the module moves or a state dict is loaded."""
        if self._engine is None and self.device.type == "cuda":
            self._engine = monster.MonsterEngine(self.config, self.network.state_dict(), self.device, self.compute_dtype)
        return self._engine

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)

    @property
    def device(self):
        return next(self.network.parameters()).device

    # ---- schedule ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def training_ts(size):
        return (diffusion.P_mean + torch.randn(size) * diffusion.P_std).exp()

    @staticmethod
    def _ramp(n_steps):
        ramp = torch.linspace(0, 1, n_steps)
        min_inv_rho = diffusion.sigma_min ** (1 / diffusion.rho)
        max_inv_rho = diffusion.sigma_max ** (1 / diffusion.rho)
        return (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** diffusion.rho

    def _schedule_ts(self, n_steps):
        return self._ramp(n_steps).to(self.device)

    def schedule_ts(self, n_steps):
        schedule_ts = self._schedule_ts(n_steps)
        return zip(schedule_ts[:-1], schedule_ts[1:])

    @staticmethod
    def sigmas(ts):
        return PredictionBatch.sigmas(ts)

    @staticmethod
    def alphas(ts):
        return PredictionBatch.alphas(ts)

    @staticmethod
    def random_noise(size):
        return standardize.decode(torch.randn(size, *settings.INPUT_SHAPE) * diffusion.sigma_max)

    @staticmethod
    def diffuse(images, ts, noise=None):
        if isinstance(ts, float) or ts.ndim == 0:
            ts = torch.full((images.shape[0],), float(ts)).to(images.device)
        if noise is None:
            noise = torch.randn_like(images)
        assert images.shape == noise.shape
        if images.is_cuda:          # decode(x0 + noise * sigma) = images + noise * sigma / 2
            return sampler.lincomb2(images, 1.0, noise.to(images.device), ts.to(images.device) / 2)
        return standardize.decode(standardize.encode(images) + noise * MonsterDiffusion.sigmas(ts))

    # ---- EDM parameterisation (arXiv 2206.00364) -----------------------------------------------------------------------------------
    def c_skip(self, ts):
        return diffusion.sigma_data ** 2 / (diffusion.sigma_data ** 2 + self.sigmas(ts) ** 2)

    def c_out(self, ts):
        return self.sigmas(ts) * diffusion.sigma_data / torch.sqrt(diffusion.sigma_data ** 2 + self.sigmas(ts) ** 2)

    def c_in(self, ts):
        return 1 / torch.sqrt(diffusion.sigma_data ** 2 + self.sigmas(ts) ** 2)

    def c_noise(self, ts):
        return 1 / 4 * self.sigmas(ts).log().view(-1)

    def _need_engine(self):
        if self.engine is None:
            raise RuntimeError("MonsterDiffusion needs a HIP device: call .to('cuda') first (perceptor_amd has no CPU fallback)")
        return self.engine

    def denoised_(self, diffused_images, ts, nonleaky_augmentations=None):
        """denoised_xs = c_skip * x + c_out * network(c_in * x, c_noise, augmentations): one engine evaluation (no host synchronisation).
        nonleaky_augmentations = None are the zeros [N, 9] of the reference."""
        if not torch.is_tensor(diffused_images) or not diffused_images.is_cuda:
            raise RuntimeError("MonsterDiffusion runs on a HIP device only: pass device tensors (perceptor_amd has no CPU fallback)")
        want_grad = torch.is_grad_enabled() and diffused_images.requires_grad
        if want_grad and not self.input_grad:
            raise NotImplementedError("MonsterDiffusion has no input gradient yet: construct it with input_grad=True")
        if self.input_grad and torch.is_grad_enabled() and any(torch.is_tensor(v) and v.requires_grad for v in (ts, nonleaky_augmentations)):
            raise NotImplementedError("MonsterDiffusion(input_grad=True) differentiates diffused_images only: ts and the augmentations have no gradient")
        if diffused_images.ndim != 4 or diffused_images.shape[1] != settings.INPUT_CHANNELS:
            raise ValueError("diffused_images must be [N, 3, H, W]")
        monster.check_size(self.config, *diffused_images.shape[2:])
        eng = self._need_engine()
        sigma = sampler.edm_sigma(torch.as_tensor(ts) if not isinstance(ts, float) else ts, diffused_images.shape[0], self.device)
        if want_grad:
            return _Denoised.apply(diffused_images.to(self.device), sigma, self, nonleaky_augmentations)
        return eng.forward(diffused_images.to(self.device), sigma, nonleaky_augmentations)

    def forward(self, diffused_images, ts, nonleaky_augmentations=None):
        denoised_xs = self.denoised_(diffused_images, ts, nonleaky_augmentations)
        return PredictionBatch(denoised_xs=denoised_xs, diffused_images=diffused_images,
                               ts=torch.as_tensor(ts, dtype=torch.float32).flatten().to(self.device))

    def predictions_(self, diffused_images, ts, nonleaky_augmentations=None):
        return self.forward(diffused_images, ts, nonleaky_augmentations)

    def predictions(self, diffused_images, ts, nonleaky_augmentations=None):
        if self.training:
            raise Exception("Cannot run predictions method while in training mode. Use predictions_")
        return self.predictions_(diffused_images, ts, nonleaky_augmentations)

    # ---- samplers ------------------------------------------------------------------------------------------------------------------
    @staticmethod
    def gamma(ts, n_steps):
        return torch.where(
            (ts >= diffusion.S_tmin) & (ts <= diffusion.S_tmax),
            torch.minimum(torch.tensor(diffusion.S_churn / n_steps), torch.tensor(2).sqrt() - 1).to(ts),
            torch.zeros_like(ts),
        )

    @staticmethod
    def reversed_ts(ts, n_steps):
        return ts + MonsterDiffusion.gamma(ts, n_steps) * ts

    def inject_noise(self, diffused_images, ts, reversed_ts, noise=None):
        """decode(x + sqrt(sigma(reversed_ts)^2 - sigma(ts)^2) * noise * S_noise); noise = None draws torch.randn_like on the device."""
        diffused_images = diffused_images.to(self.device)
        if noise is None:
            noise = torch.randn_like(diffused_images)
        return sampler.edm_inject_noise(diffused_images, torch.as_tensor(ts), torch.as_tensor(reversed_ts), noise.to(self.device), diffusion.S_noise)

    def sample(self, size, n_evaluations=100, progress=False, diffused_images=None):
        return self.elucidated_sample(size, n_evaluations, progress, diffused_images)

    @staticmethod
    def _progress(total, enabled):
        if not enabled:
            return None
        from tqdm import tqdm
        return tqdm(total=total, leave=False)

    def elucidated_sample(self, size, n_evaluations=100, progress=False, diffused_images=None):
        """Elucidated stochastic sampling (arXiv 2206.00364, algorithm 2): n_evaluations // 2 Heun steps, one clamped image each."""
        if self.training:
            raise Exception("Cannot run sample method while in training mode.")
        if diffused_images is None:
            diffused_images = self.random_noise(size)
        diffused_images = diffused_images.to(self.device)
        n_steps = n_evaluations // 2
        bar = self._progress(n_steps, progress)
        for from_ts, to_ts in self.schedule_ts(n_steps):
            reversed_ts = self.reversed_ts(from_ts, n_steps).clamp(max=diffusion.sigma_max)
            reversed_diffused_images = self.inject_noise(diffused_images, from_ts, reversed_ts)

            predictions = self.predictions(reversed_diffused_images, reversed_ts)
            reversed_eps = predictions.eps
            diffused_images = predictions.step(to_ts)

            predictions = self.predictions(diffused_images, to_ts)
            diffused_images = predictions.correction(reversed_diffused_images, reversed_ts, reversed_eps)
            if bar is not None:
                bar.update()
            yield sampler.clamp(predictions.denoised_images, 0.0, 1.0)

        reversed_ts = self.reversed_ts(to_ts, n_steps)
        diffused_images = self.inject_noise(diffused_images, to_ts, reversed_ts)
        predictions = self.predictions(diffused_images, reversed_ts)
        if bar is not None:
            bar.close()
        yield sampler.clamp(predictions.denoised_images, 0.0, 1.0)

    @staticmethod
    def linear_multistep_coeff(order, sigmas, from_index, to_index):
        if order - 1 > from_index:
            raise ValueError(f"Order {order} too high for step {from_index}")
        from scipy import integrate
        s = [float(v) for v in sigmas]

        def lagrange(tau):
            prod = 1.0
            for k in range(order):
                if to_index != k:
                    prod *= (tau - s[from_index - k]) / (s[from_index - to_index] - s[from_index - k])
            return prod

        return integrate.quad(lagrange, s[from_index], s[from_index + 1], epsrel=1e-4)[0]

    def linear_multistep_sample(self, size, n_evaluations=100, progress=False, diffused_images=None, order=4):
        """Katherine Crowson's linear multistep sampler (k-diffusion sampling.py, sample_lms): n_evaluations images."""
        if self.training:
            raise Exception("Cannot run sample method while in training mode.")
        if not 1 <= order <= 4:
            raise ValueError("linear multistep order must be between 1 and 4")
        if diffused_images is None:
            diffused_images = self.random_noise(size)
        diffused_images = diffused_images.to(self.device)
        n_steps = n_evaluations
        host_sigmas = self._ramp(n_steps)                 # the coefficients are host integrals: no device read-back per step
        epses = []
        bar = self._progress(n_steps, progress)
        for from_index, (from_ts, to_ts) in enumerate(self.schedule_ts(n_steps)):
            predictions = self.predictions(diffused_images, from_ts)
            epses.append(predictions.eps)
            if len(epses) > order:
                epses.pop(0)
            current_order = len(epses)
            coeffs = [self.linear_multistep_coeff(current_order, host_sigmas, from_index, to_index) for to_index in range(current_order)]
            diffused_images = sampler.edm_lms(diffused_images, coeffs, list(reversed(epses)))
            if bar is not None:
                bar.update()
            yield sampler.clamp(predictions.denoised_images, 0.0, 1.0)

        predictions = self.predictions(diffused_images, to_ts)
        if bar is not None:
            bar.close()
        yield sampler.clamp(predictions.denoised_images, 0.0, 1.0)
