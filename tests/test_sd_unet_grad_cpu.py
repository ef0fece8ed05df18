"""CPU side of the SD UNet's latent gradient (engine/sd.py SdUnetEngine.forward_train / backward, csrc/attn_flash.hip's backward):

  1. tests/_sd_unet_ref64.py, the float64 yardstick of the GPU tests, is the oracle's own network: in fp32 it reproduces
     oracle.sd.unet_forward exactly;
  2. the new C entry points are declared in the header, exported by the library and bound in _hip._PROTOS with matching parameters;
  3. the tiled backward the kernel implements (P recomputed per key tile from the exp2-domain log-sum-exp, delta = rowsum(dO o O), keys
     zero-padded to whole tiles and masked) equals autograd in float64;
  4. how far each plausible defect of the backward lands from the bounds tests/test_gpu_sd_unet_grad.py asserts (rel-L2 4e-2 in bf16).
"""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import _sd_unet_ref64 as R
from oracle import sd as osd
from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
from test_abi import _header_decls, _kind

REL_BF16 = 4e-2
NEW_ENTRY_POINTS = ["pmi_attn_flash_train", "pmi_attn_flash_bwd_workspace", "pmi_attn_flash_bwd", "pmi_geglu_bwd"]


def _inputs(ocfg, n=2, tok=7):
    w = synth_state_dict(osd.unet_state_dict_shapes(ocfg), 0)
    x = seeded_noise((n, ocfg.in_channels, 16, 16), 71)
    return w, x, torch.tensor([981.0, 20.0][:n]), seeded_noise((n, tok, ocfg.context_dim), 72), seeded_noise((n, ocfg.out_channels, 16, 16), 93)


@pytest.mark.parametrize("cfg_name", ["SD_TINY", "SD_MID"])
def test_helper_in_fp32_is_the_oracle(cfg_name):
    ocfg = getattr(osd, cfg_name)
    w, x, ts, ctx, cot = _inputs(ocfg)
    a = x.clone().requires_grad_()
    ea = osd.unet_forward(w, ocfg, a, ts, ctx)
    ea.backward(cot)
    eb, gb = R.latent_grad(w, ocfg, x, ts, ctx, cot, dtype=torch.float32)
    assert torch.equal(ea.detach(), eb) and torch.equal(a.grad, gb)
    _, g64 = R.latent_grad(w, ocfg, x, ts, ctx, cot)
    rel = float((gb.double() - g64).norm() / g64.norm())
    print(f"\n[ref] {cfg_name}: fp32 autograd vs float64 rel-L2 {rel:.2e}, max |g| {float(g64.abs().max()):.2f}")
    assert rel < 1e-5


@pytest.mark.parametrize("tag", ["tiny", "v1"])
def test_oracle_autograd_reproduces_the_reference_unet_gradient_fixture(tag):
    """tests/golden/sd_ldm_unet_{tag}_grad.npz: fp32 autograd of the reference's vendored CompVis UNetModel
    (tools/gen_sd_unet_grad_golden.py).  The oracle's fp32 autograd reproduces it; the float64 helper sits at fp32 rounding from it."""
    import numpy as np
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"sd_ldm_unet_{tag}_grad.npz"))
    ocfg = osd.SD_TINY if tag == "tiny" else osd.SD_V1
    w = synth_state_dict(osd.unet_state_dict_shapes(ocfg), 0)
    x, ts, ctx, cot, want = (torch.from_numpy(g[k]) for k in ("x", "t", "ctx", "cotangent", "grad"))
    a = x.clone().requires_grad_()
    eps = osd.unet_forward(w, ocfg, a, ts, ctx)
    eps.backward(cot)
    rel32 = float((a.grad - want).norm() / want.norm())
    _, g64 = R.latent_grad(w, ocfg, x, ts, ctx, cot)
    rel64 = float((g64 - want.double()).norm() / want.double().norm())
    print(f"\n[fixture] {tag}: oracle fp32 autograd vs fixture rel-L2 {rel32:.2e}; float64 helper vs fixture {rel64:.2e}; max |g| {float(want.abs().max()):.2f}")
    assert float((eps.detach() - torch.from_numpy(g["eps"])).abs().max()) <= 3e-5 * float(eps.detach().abs().max())
    assert rel32 <= 1e-6 and rel64 <= 1e-5


@pytest.mark.parametrize("name", NEW_ENTRY_POINTS)
def test_new_entry_points_in_header_library_and_protos(name):
    from perceptor_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        from perceptor_amd.csrc import build
        build.build()
    decls = _header_decls()
    assert name in decls, f"{name} is not declared in include/perceptor_hip.h"
    assert hasattr(C.CDLL(_hip.LIB_PATH), name), f"{name} is not exported"
    (args,) = _hip._PROTOS[name]
    assert [_kind(p) for p in decls[name]] == list(args)


@pytest.mark.parametrize("t,tk,d", [(100, 77, 24), (64, 64, 40), (33, 7, 160)])
def test_tiled_backward_from_lse_equals_autograd(t, tk, d):
    g = torch.Generator().manual_seed(t + tk)
    q, k, v = (torch.randn((s, d), generator=g, dtype=torch.float64).requires_grad_() for s in (t, tk, tk))
    d_out = torch.randn((t, d), generator=g, dtype=torch.float64)
    scale = d ** -0.5
    out = torch.softmax(q @ k.T * scale, dim=-1) @ v
    out.backward(d_out)
    o2, dq, dk, dv = R.attention_tiled_backward(q.detach(), k.detach(), v.detach(), d_out, scale)
    for got, want in ((o2, out.detach()), (dq, q.grad), (dk, k.grad), (dv, v.grad)):
        assert float((got - want).abs().max()) <= 1e-10 * (1 + float(want.abs().max()))


# ---- defects of the backward against the bound ---------------------------------------------------------------------------------------------
class _F:
    def __init__(self, **over):
        self._over = over

    def __getattr__(self, k):
        return self._over[k] if k in self._over else getattr(F, k)


class _SoftmaxNoDelta(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s):
        p = torch.softmax(s, dim=-1)
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, g):
        (p,) = ctx.saved_tensors
        return p * g                                                         # dS = P o dP, the rowsum(dP o P) term missing


def _ln_frozen_moments(x, shape, wt, b, eps):
    mu, var = x.mean(-1, keepdim=True).detach(), x.var(-1, unbiased=False, keepdim=True).detach()
    return (x - mu) / (var + eps).sqrt() * wt + b


def _attention_no_delta(sd_, k, x, ctx, heads):
    n, t, c = x.shape
    d = c // heads
    q = F.linear(x, sd_[k + ".to_q.weight"]); kk = F.linear(ctx, sd_[k + ".to_k.weight"]); v = F.linear(ctx, sd_[k + ".to_v.weight"])
    sp = lambda z: z.reshape(n, z.shape[1], heads, d).transpose(1, 2)
    a = _SoftmaxNoDelta.apply(sp(q) @ sp(kk).transpose(-1, -2) * d ** -0.5) @ sp(v)
    return F.linear(a.transpose(1, 2).reshape(n, t, c), sd_[k + ".to_out.0.weight"], sd_[k + ".to_out.0.bias"])


DEFECTS = ["cross_dq_dropped", "self_dk_dv_dropped", "softmax_no_delta", "geglu_gate_dropped", "layernorm_frozen_moments", "skip_concat_dropped",
           "padded_keys_weighted"]


@pytest.mark.parametrize("cfg_name", ["SD_TINY", "SD_MID"])
def test_each_backward_defect_breaks_the_bf16_bound_by_2x(cfg_name, monkeypatch):
    """The gradient with one defect against the gradient without, float64.  padded_keys_weighted: the prompt's 7 keys zero-padded to a
    whole 32-key tile and left unmasked (their zero rows get weight exp(-max) in the softmax's normaliser, forward and backward alike)."""
    ocfg = getattr(osd, cfg_name)
    w, x, ts, ctx, cot = _inputs(ocfg)
    _, exact = R.latent_grad(w, ocfg, x, ts, ctx, cot)
    orig = osd._attention
    margins = {}
    for d in DEFECTS:
        kw = {}
        with monkeypatch.context() as mp:
            if d == "cross_dq_dropped":
                mp.setattr(osd, "_attention", lambda s, k, xx, c, h: orig(s, k, xx.detach() if k.endswith("attn2") else xx, c, h))
            elif d == "self_dk_dv_dropped":
                mp.setattr(osd, "_attention", lambda s, k, xx, c, h: orig(s, k, xx, c.detach() if k.endswith("attn1") else c, h))
            elif d == "softmax_no_delta":
                mp.setattr(osd, "_attention", _attention_no_delta)
            elif d == "geglu_gate_dropped":
                mp.setattr(osd, "F", _F(gelu=lambda g: F.gelu(g.detach())))
            elif d == "layernorm_frozen_moments":
                mp.setattr(osd, "F", _F(layer_norm=_ln_frozen_moments))
            elif d == "skip_concat_dropped":
                kw = {"drop_skip_grad": True}
            elif d == "padded_keys_weighted":
                mp.setattr(osd, "_attention", lambda s, k, xx, c, h: orig(s, k, xx, F.pad(c, (0, 0, 0, 32 - c.shape[1])) if k.endswith("attn2") else c, h))
            _, bad = R.latent_grad(w, ocfg, x, ts, ctx, cot, **kw)
        margins[d] = float((bad - exact).norm() / exact.norm())
    print(f"\n[defects] {cfg_name}: " + ", ".join(f"{d} {r:.3f} ({r / REL_BF16:.1f}x)" for d, r in margins.items()))
    for d, r in margins.items():
        assert r >= 2 * REL_BF16, (cfg_name, d, r)
