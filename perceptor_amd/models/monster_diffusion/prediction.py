"""PredictionBatch / Prediction -- drop-in for perceptor.models.monster_diffusion.prediction (prediction.py:10-121, without the PIL
helpers); eps / step / correction are one fused HIP kernel (pmi_edm_predict), sigma itself is the time variable and alpha is 1.  Where the prediction carries an autograd graph (MonsterDiffusion(input_grad=True)) the same
formulas run as torch arithmetic, so a loss on eps / step / correction reaches diffused_images."""
from __future__ import annotations

import torch

from ...engine import sampler
from ...utils.record import FrozenRecord
from . import standardize


class Prediction(FrozenRecord):
    _fields = ("denoised_image", "diffused_image", "t")


class PredictionBatch(FrozenRecord):
    _fields = ("denoised_xs", "diffused_images", "ts")

    def __len__(self):
        return len(self.denoised_xs)

    def __getitem__(self, index):
        # ts holds one value when the batch was evaluated at a scalar sigma
        return Prediction(denoised_image=self.denoised_images[index], diffused_image=self.diffused_images[index],
                          t=self.ts[index if self.ts.numel() > 1 else 0])

    def __iter__(self):
        for index in range(len(self)):
            yield self[index]

    @property
    def device(self):
        return self.denoised_xs.device

    @staticmethod
    def sigmas(ts):
        if isinstance(ts, float):
            ts = torch.as_tensor(ts)
        if ts.ndim == 0:
            return ts.reshape(1)
        return ts[:, None, None, None]

    @staticmethod
    def alphas(ts):
        return torch.ones_like(PredictionBatch.sigmas(ts))

    @property
    def from_sigmas(self):
        return self.sigmas(self.ts).to(self.device)

    @property
    def from_alphas(self):
        return self.alphas(self.ts).to(self.device)

    @property
    def from_xs(self):
        return self.diffused_xs

    @property
    def diffused_xs(self):
        return standardize.encode(self.diffused_images.to(self.device))

    @property
    def denoised_images(self):
        return standardize.decode(self.denoised_xs)

    @property
    def _in_graph(self):
        """a loss on eps / step / correction must reach diffused_images: pmi_edm_predict would drop the graph, so the same formulas run as
        torch arithmetic (fp32, element-wise) when either input carries one"""
        return torch.is_grad_enabled() and (self.denoised_xs.requires_grad or (torch.is_tensor(self.diffused_images) and self.diffused_images.requires_grad))

    def _sig(self, ts):
        s = torch.as_tensor(ts, dtype=torch.float32).to(self.device).reshape(-1)
        return s.reshape(-1, 1, 1, 1) if s.numel() > 1 else s

    def _eps_torch(self):
        return (self.diffused_xs - self.denoised_xs) / self._sig(self.ts)

    @property
    def eps(self):
        if self._in_graph:
            return self._eps_torch()
        return sampler.edm_predict(self.diffused_images.to(self.device), self.denoised_xs, self.ts, eps=True)[0]

    def step(self, to_ts):
        """Step the diffused image to `to_ts`: denoised_xs * 1 + eps * sigma(to_ts), decoded."""
        if self._in_graph:
            return standardize.decode(self.denoised_xs + self._eps_torch() * self._sig(to_ts))
        return sampler.edm_predict(self.diffused_images.to(self.device), self.denoised_xs, self.ts, to_sigma=torch.as_tensor(to_ts))[1]

    def correction(self, previous_diffused_images, previous_ts, previous_eps):
        """Heun's second-order correction from the previous point: x_prev + (sigma - sigma_prev) * (eps + eps_prev) / 2, decoded."""
        if self._in_graph:
            prev_xs = standardize.encode(previous_diffused_images.to(self.device))
            return standardize.decode(prev_xs + (self._sig(self.ts) - self._sig(previous_ts)) * (self._eps_torch() + previous_eps.to(self.device)) / 2)
        return sampler.edm_predict(self.diffused_images.to(self.device), self.denoised_xs, self.ts,
                                   previous=(previous_diffused_images.to(self.device), torch.as_tensor(previous_ts), previous_eps))[2]
