"""CPU side of the VAE encoder's image gradient (engine/sd.py): the phase-packed Downsample2D adjoint, the reference-run fixtures against
the oracle, and how far each plausible defect of the backward lands from the bounds the GPU tests assert
(tests/test_gpu_sd_vae_enc_grad.py: rel-L2 bf16 2.5e-2 / f16 4e-3, cosine bf16 0.9995 / f16 0.99999)."""
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


# ---- the phase packing -------------------------------------------------------------------------------------------------------------------------------
def phased_adjoint(dy: torch.Tensor, packed: torch.Tensor) -> torch.Tensor:
    """The rule pmi_igemm's phased geometry applies (csrc/igemm.hip), in plain torch: phase ph = 2a + b owns the k range that starts
    (0, 4, 6, 8)[ph] taps in, its tap t sits at gradient pixel (p - ty, q - tx) with ty = t >> (ntx - 1), tx = t & (ntx - 1), ntx = 2 - b,
    and row (p, q) of the phase lands at output pixel (2p + a, 2q + b).  dy [N, Co, h, w], packed [Ci, Co, 3, 3] -> [N, Ci, 2h, 2w]."""
    n, co, h, w = dy.shape
    ci = packed.shape[0]
    wk = packed.reshape(ci, co, 9)
    dx = dy.new_zeros((n, ci, 2 * h, 2 * w))
    for ph in range(4):
        a, b = ph >> 1, ph & 1
        ntx = 2 - b
        for t in range((2 - a) * ntx):
            ty, tx = t >> (ntx - 1), t & (ntx - 1)
            shifted = F.pad(dy, (tx, 0, ty, 0))[..., :h, :w]              # shifted[p, q] = dy[p - ty, q - tx], zero outside the grid
            dx[:, :, a::2, b::2] += torch.einsum("io,nopq->nipq", wk[:, :, (0, 4, 6, 8)[ph] + t], shifted)
    return dx


@pytest.mark.parametrize("n,c,co,h,w", [(2, 5, 7, 8, 12), (1, 8, 8, 4, 4), (3, 3, 16, 2, 6), (1, 16, 4, 14, 2)])
def test_phase_packed_downsample_adjoint_equals_autograd_vjp(n, c, co, h, w):
    g = torch.Generator().manual_seed(n * 100 + c)
    wt = torch.randn((co, c, 3, 3), generator=g, dtype=torch.float64)
    x = torch.randn((n, c, h, w), generator=g, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.pad(x, (0, 1, 0, 1)), wt, stride=2)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    packed = sd.pack_downsample_adjoint_weights(wt)
    assert packed.shape == (c, co, 3, 3) and packed.dtype == torch.float64
    got = phased_adjoint(dy, packed)
    assert got.shape == x.shape
    assert float((got - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())


def test_packing_is_a_transposed_reordering_of_the_nine_taps():
    """No sum and no flip: every tap appears once, phase-major, 4 + 2 + 2 + 1."""
    wt = torch.arange(2 * 3 * 9, dtype=torch.float64).view(2, 3, 3, 3)
    p = sd.pack_downsample_adjoint_weights(wt).reshape(3, 2, 9)
    assert len(set(sd.DOWN_ADJOINT_TAPS)) == 9
    for t, (ky, kx) in enumerate(sd.DOWN_ADJOINT_TAPS):
        assert torch.equal(p[:, :, t], wt[:, :, ky, kx].t())
    assert [(ky & 1, kx & 1) for ky, kx in sd.DOWN_ADJOINT_TAPS] == [(0, 0)] * 4 + [(0, 1)] * 2 + [(1, 0)] * 2 + [(1, 1)]


# ---- the reference-run fixtures against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["tiny", "v1"])
def test_oracle_vjp_matches_reference_encoder_gradient_fixture(tag):
    g = np.load(os.path.join(GOLDEN, f"sd_ldm_vae_enc_{tag}_grad.npz"))
    ocfg = osd.VAE_TINY if tag == "tiny" else osd.VAE_V1
    w = {k: v.double() for k, v in synth_state_dict(osd.vae_encoder_state_dict_shapes(ocfg), 0).items()}
    x = torch.from_numpy(g["x"]).double().requires_grad_()
    assert x.shape[-1] == (32 if tag == "tiny" else 64)
    mom = torch.cat(osd.vae_encode_moments(w, ocfg, x), 1)
    want_mom = torch.cat([torch.from_numpy(g["mean"]), torch.from_numpy(g["logvar"])], 1).double()
    assert float((mom.detach() - want_mom).abs().max()) < 1e-5 * float(want_mom.abs().max())
    mom.backward(torch.from_numpy(g["cotangent"]).double())
    want = torch.from_numpy(g["grad"]).double()
    assert float((x.grad - want).norm() / want.norm()) < 1e-6


# ---- defects of the backward against the bounds ------------------------------------------------------------------------------------------------
class _F:
    """torch.nn.functional with some entries replaced (oracle.sd reads F.linear through its module global)."""

    def __init__(self, **over):
        self._over = over

    def __getattr__(self, k):
        return self._over[k] if k in self._over else getattr(F, k)


class _DownSymmetric(torch.autograd.Function):
    """Downsample2D whose backward is the adjoint of the SYMMETRIC pad-1 stride-2 convolution: every phase one pixel off."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(w)
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        return F.conv_transpose2d(g, w, stride=2, padding=1, output_padding=1), None, None


class _DownFlipped(torch.autograd.Function):
    """Downsample2D whose backward flips the taps (what a stride-1 dX needs and this adjoint does not)."""

    @staticmethod
    def forward(ctx, x, w, b):
        ctx.save_for_backward(w)
        return F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)

    @staticmethod
    def backward(ctx, g):
        (w,) = ctx.saved_tensors
        full = F.conv_transpose2d(g, w.flip(2, 3), stride=2)                # [.., 2h + 1, 2w + 1]: the last row / column is the pad's
        return full[..., :-1, :-1], None, None


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


def _conv_with(down=None, same=None):
    def conv(x, sd_, k, stride=1, pad=1):
        wt, b = sd_[k + ".weight"], sd_[k + ".bias"]
        if stride == 2 and down is not None:
            return down.apply(x[..., :-1, :-1], wt, b)                      # (the oracle hands over the padded tensor)
        if stride == 1 and wt.shape[-1] == 3 and same is not None:
            return same.apply(x, wt, b)
        return F.conv2d(x, wt, b, stride=stride, padding=pad)
    return conv


def _grad(ocfg, w, img, noise, cot, logvar_branch=True):
    """d / d images of <cot, encode(images, "sample")> with the noise fixed: z = 0.18215 (mean + noise exp(clamp(logvar) / 2))."""
    x = img.clone().requires_grad_()
    mean, logvar = osd.vae_encode_moments(w, ocfg, 2 * x - 1)
    if not logvar_branch:
        logvar = logvar.detach()
    z = 0.18215 * (mean + noise * torch.exp(0.5 * logvar.clamp(-30.0, 20.0)))
    z.backward(cot)
    return x.grad


DEFECTS = ["down_symmetric_pad", "down_flipped", "unflipped", "no_attention_backward", "gn_no_mean_terms", "no_factor_2", "no_logvar_branch"]


@pytest.mark.parametrize("cfg_name", ["VAE_TINY", "VAE_V1"])
def test_each_backward_defect_breaks_the_bf16_bound_by_2x(cfg_name, monkeypatch):
    """The rule of DESIGN.md §11: the float64 VJP with ONE defect against the VJP without it must be at least twice the bf16 bound away
    (rel-L2 2.5e-2 or 1 - cos 5e-4), so a passing GPU test cannot hide it."""
    ocfg = getattr(osd, cfg_name)
    w = {k: v.double() for k, v in synth_state_dict(osd.vae_encoder_state_dict_shapes(ocfg), 0).items()}
    down = 1 << (len(ocfg.block_out) - 1)
    hw = 8 if cfg_name == "VAE_TINY" else 4
    img = (seeded_noise((2, 3, down * hw, down * hw), 74) * 0.25 + 0.5).double()
    noise = seeded_noise((2, 4, hw, hw), 75).double()
    cot = seeded_noise((2, 4, hw, hw), 93).double() * 1e-6
    exact = _grad(ocfg, w, img, noise, cot)
    proj = w["encoder.mid_block.attentions.0.proj_attn.weight"]
    margins = {}
    for d in DEFECTS:
        with monkeypatch.context() as mp:
            if d == "down_symmetric_pad":
                mp.setattr(osd, "_conv", _conv_with(down=_DownSymmetric))
            elif d == "down_flipped":
                mp.setattr(osd, "_conv", _conv_with(down=_DownFlipped))
            elif d == "unflipped":
                mp.setattr(osd, "_conv", _conv_with(same=_ConvUnflipped))
            elif d == "no_attention_backward":
                mp.setattr(osd, "F", _F(linear=lambda x, wt, b=None: F.linear(x.detach() if wt is proj else x, wt, b)))
            elif d == "gn_no_mean_terms":
                mp.setattr(osd, "_gn", _gn_no_mean)
            if d == "no_factor_2":                                      # the forward keeps 2 * img - 1; the backward drops its factor
                bad = exact * 0.5
            elif d == "no_logvar_branch":
                bad = _grad(ocfg, w, img, noise, cot, logvar_branch=False)
            else:
                bad = _grad(ocfg, w, img, noise, cot)
        rel = float((bad - exact).norm() / exact.norm())
        cos = float(F.cosine_similarity(bad.flatten(), exact.flatten(), dim=0))
        margins[d] = (rel / REL_BF16, (1 - cos) / (1 - COS_BF16))
        assert rel >= 2 * REL_BF16 or (1 - cos) >= 2 * (1 - COS_BF16), (cfg_name, d, rel, cos)
    print(f"\n[defects] {cfg_name}: " + ", ".join(f"{d} rel/bound {a:.1f}x (1-cos)/(1-bound) {b:.1f}x" for d, (a, b) in margins.items()))
