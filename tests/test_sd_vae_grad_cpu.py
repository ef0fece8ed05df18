"""CPU side of the VAE decoder's input gradient (engine/sd.py): the phase-folded Upsample2D adjoint, the FLOP count, the reference-run
fixture against the oracle, and how far each plausible defect of the backward lands from the bounds the GPU tests assert
(tests/test_gpu_sd_vae_grad.py: rel-L2 bf16 2.5e-2 / f16 4e-3, cosine bf16 0.9995 / f16 0.99999)."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import sd as osd
from perceptor_amd.engine import sd
from perceptor_amd.utils.synth import seeded_noise, synth_state_dict

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
REL_BF16, COS_BF16 = 2.5e-2, 0.9995


# ---- the fold --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,cin,cout,h,w", [(2, 5, 7, 6, 9), (1, 8, 8, 4, 4), (3, 3, 16, 1, 5), (1, 16, 4, 7, 2)])
def test_folded_upsample_adjoint_equals_autograd_vjp(n, cin, cout, h, w):
    g = torch.Generator().manual_seed(n * 100 + cin)
    wt = torch.randn((cout, cin, 3, 3), generator=g, dtype=torch.float64)
    x = torch.randn((n, cin, h, w), generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), wt, padding=1)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    folded = sd.fold_upsample_weights(wt)
    assert folded.shape == (cin, cout, 4, 4) and folded.dtype == torch.float64
    got = F.conv2d(dy, folded, stride=2, padding=1)
    assert got.shape == x.shape
    assert float((got - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())


def test_fold_sums_each_3x3_tap_exactly_four_times():
    """Every (ky, kx) tap of W reaches 2 x 2 entries of W' (rows {2},{1,2},{0,1},{0} per axis): the total is 4 x the sum of W."""
    wt = torch.arange(9, dtype=torch.float64).view(1, 1, 3, 3)
    f = sd.fold_upsample_weights(wt)[0, 0]
    assert float(f.sum()) == 4 * 36
    assert f[0, 0] == wt[0, 0, 2, 2] and f[3, 3] == wt[0, 0, 0, 0] and f[1, 1] == wt[0, 0, 1:, 1:].sum()


# ---- FLOP count ------------------------------------------------------------------------------------------------------------------------------------
def test_vae_decoder_gflop_hand_count():
    """VAE_TINY (32, 64), one resnet per level, at 8 x 12 latents, counted by hand layer by layer."""
    cfg = sd.VaeConfig(block_out=(32, 64), layers_per_block=1)
    p = 8 * 12
    mac = p * 4 * 4 + p * 4 * 64 * 9                                  # post_quant_conv, conv_in
    mac += 2 * 2 * p * 64 * 64 * 9                                     # mid resnets: two 3x3 each
    mac += 4 * p * 64 * 64 + 2 * p * p * 64                            # q, k, v, proj; QK^T and PV
    mac += 2 * 2 * p * 64 * 64 * 9                                     # up block 0: two resnets 64 -> 64
    mac_up = 4 * p * 64 * 64 * 9                                       # upsampler conv at 16 x 24
    mac += mac_up
    mac += 2 * 4 * p * (64 * 32 * 9 + 32 * 32 * 9 + 64 * 32)           # first resnet 64 -> 32 with shortcut (two resnets in the level)
    mac -= 4 * p * (64 * 32 * 9 + 32 * 32 * 9 + 64 * 32) - 4 * p * 32 * 32 * 18   # ... the second is 32 -> 32, no shortcut
    mac += 4 * p * 32 * 3 * 9                                          # conv_out
    fwd, bwd = sd.vae_decoder_gflop(cfg, 8, 12)
    assert fwd == pytest.approx(2 * mac / 1e9, rel=1e-12)
    bwd_mac = mac + 2 * p * p * 64 - mac_up + p * 64 * 64 * 16          # two more attention products; the folded up adjoint
    assert bwd == pytest.approx(2 * bwd_mac / 1e9, rel=1e-12)
    assert sd.vae_decoder_gflop(cfg, 8, 12, fused_up=False)[1] == pytest.approx(2 * (bwd_mac - p * 64 * 64 * 16 + mac_up) / 1e9, rel=1e-12)
    f512, _ = sd.vae_decoder_gflop(sd.VAE_V1, 64, 64)
    assert 2500 < f512 < 2530                                          # ~2515 GFLOP per 512 x 512 image, 696 of them in the up-samplers


# ---- the reference-run fixture against the oracle -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["tiny", "v1"])
def test_oracle_vjp_matches_reference_decoder_gradient_fixture(tag):
    g = np.load(os.path.join(GOLDEN, f"sd_ldm_vae_{tag}_grad.npz"))
    ocfg = osd.VAE_TINY if tag == "tiny" else osd.VAE_V1
    w = {k: v.double() for k, v in synth_state_dict(osd.vae_decoder_state_dict_shapes(ocfg), 0).items()}
    z = torch.from_numpy(g["z"]).double().requires_grad_()
    y = osd.vae_decode(w, ocfg, z)
    assert float((y.detach() - torch.from_numpy(g["dec"]).double()).abs().max()) < 1e-5 * float(y.detach().abs().max())
    y.backward(torch.from_numpy(g["cotangent"]).double())
    want = torch.from_numpy(g["grad"]).double()
    assert float((z.grad - want).norm() / want.norm()) < 1e-6


# ---- defects of the backward against the bounds ------------------------------------------------------------------------------------------------
class _F:
    """torch.nn.functional with some entries replaced (oracle.sd reads F.interpolate / F.linear through its module global)."""

    def __init__(self, **over):
        self._over = over

    def __getattr__(self, k):
        return self._over[k] if k in self._over else getattr(F, k)


class _UpNoSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        return F.interpolate(x, scale_factor=2.0, mode="nearest")

    @staticmethod
    def backward(ctx, g):
        return g[:, :, ::2, ::2].clone()                                  # one pixel of each 2x2 block instead of their sum


class _ConvUnflipped(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(w)
        return F.conv2d(x, w, b, padding=1)

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return F.conv2d(g, w.transpose(0, 1), padding=1), None, None      # transposed but not flipped


def _gn_no_mean(x, sd_, k, groups, eps):
    n, c = x.shape[:2]
    xg = x.reshape(n, groups, -1)
    mu, var = xg.mean(-1, keepdim=True).detach(), xg.var(-1, unbiased=False, keepdim=True).detach()
    y = ((xg - mu) / (var + eps).sqrt()).reshape(x.shape)
    return y * sd_[k + ".weight"].view(1, c, 1, 1) + sd_[k + ".bias"].view(1, c, 1, 1)


def _grad(ocfg, w, z, cot):
    zz = z.clone().requires_grad_()
    img = (osd.vae_decode(w, ocfg, zz / 0.18215) + 1) / 2
    img.backward(cot)
    return zz.grad


DEFECTS = ["no_2x2_sum", "unflipped", "no_attention_backward", "gn_no_mean_terms", "no_latent_scale", "no_half"]


@pytest.mark.parametrize("cfg_name", ["VAE_TINY", "VAE_V1"])
def test_each_backward_defect_breaks_the_bf16_bound_by_2x(cfg_name, monkeypatch):
    ocfg = getattr(osd, cfg_name)
    w = {k: v.double() for k, v in synth_state_dict(osd.vae_decoder_state_dict_shapes(ocfg), 0).items()}
    hw = 8 if cfg_name == "VAE_TINY" else 4
    z = seeded_noise((2, 4, hw, hw), 73).double()
    up = 1 << (len(ocfg.block_out) - 1)
    cot = seeded_noise((2, 3, up * hw, up * hw), 91).double() * 1e-6
    exact = _grad(ocfg, w, z, cot)
    proj = w["decoder.mid_block.attentions.0.proj_attn.weight"]
    margins = {}
    for d in DEFECTS:
        with monkeypatch.context() as mp:
            if d == "no_2x2_sum":
                mp.setattr(osd, "F", _F(interpolate=lambda x, scale_factor, mode: _UpNoSum.apply(x)))
            elif d == "unflipped":
                mp.setattr(osd, "_conv", lambda x, sd_, k, stride=1, pad=1: _ConvUnflipped.apply(x, sd_[k + ".weight"], sd_[k + ".bias"])
                           if sd_[k + ".weight"].shape[-1] == 3 else F.conv2d(x, sd_[k + ".weight"], sd_[k + ".bias"], stride=stride, padding=pad))
            elif d == "no_attention_backward":
                mp.setattr(osd, "F", _F(linear=lambda x, wt, b=None: F.linear(x.detach() if wt is proj else x, wt, b)))
            elif d == "gn_no_mean_terms":
                mp.setattr(osd, "_gn", _gn_no_mean)
            if d == "no_latent_scale":                                 # the forward keeps its scale; the backward drops its factor
                bad = exact * 0.18215
            elif d == "no_half":
                bad = exact * 2.0
            else:
                bad = _grad(ocfg, w, z, cot)
        rel = float((bad - exact).norm() / exact.norm())
        cos = float(F.cosine_similarity(bad.flatten(), exact.flatten(), dim=0))
        margins[d] = (rel / REL_BF16, (1 - cos) / (1 - COS_BF16))
        assert rel >= 2 * REL_BF16 or (1 - cos) >= 2 * (1 - COS_BF16), (cfg_name, d, rel, cos)
    print(f"\n[defects] {cfg_name}: " + ", ".join(f"{d} rel/bound {a:.1f}x (1-cos)/(1-bound) {b:.1f}x" for d, (a, b) in margins.items()))
