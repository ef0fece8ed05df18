"""CPU side of the SD UNet's gradient to the prompt encodings (SdUnetEngine.backward(cond_grad=True), csrc/attn_flash.hip's split key role):

  1. tests/_sd_ctx_ref64.py's joint_grad, the float64 yardstick of tests/test_gpu_sd_ctx_grad.py, reproduces in fp32 the context gradient
     of the reference's vendored CompVis UNetModel (tests/golden/sd_ldm_unet_{tiny,v1}_ctx_grad.npz, tools/gen_sd_unet_ctx_grad_golden.py);
  2. the new C entry points are declared, exported and bound; the chunk rule of the library is the documented function of the shape;
  3. the split key role's algebra (32-key tiles, S chunks of query tiles, P from the exp2-domain lse, masked padding, partials added in
     chunk order) equals autograd's dK, dV in float64;
  4. how far each plausible defect of the context gradient lands from the bf16 bound of the GPU tests (rel-L2 4e-2).
"""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as F

import _sd_ctx_ref64 as RC
import _sd_unet_ref64 as R
from oracle import sd as osd
from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
from test_abi import _header_decls, _kind
from test_sd_unet_grad_cpu import _SoftmaxNoDelta, _inputs

REL_BF16 = 4e-2
REL_F16 = 6e-3
NEW_ENTRY_POINTS = ["pmi_attn_flash_bwd_kv", "pmi_attn_flash_bwd_kv_workspace", "pmi_attn_flash_bwd_kv_chunks"]


@pytest.mark.parametrize("tag", ["tiny", "v1"])
def test_joint_autograd_reproduces_the_reference_context_gradient_fixture(tag):
    import numpy as np
    gold = os.path.join(os.path.dirname(__file__), "golden")
    g, gc = np.load(os.path.join(gold, f"sd_ldm_unet_{tag}_grad.npz")), np.load(os.path.join(gold, f"sd_ldm_unet_{tag}_ctx_grad.npz"))
    ocfg = osd.SD_TINY if tag == "tiny" else osd.SD_V1
    w = synth_state_dict(osd.unet_state_dict_shapes(ocfg), 0)
    x, ts, ctx, cot, want_x = (torch.from_numpy(g[k]) for k in ("x", "t", "ctx", "cotangent", "grad"))
    want_c = torch.from_numpy(gc["grad_ctx"])
    assert want_c.shape == ctx.shape
    # the latent gradient of the joint call is the stored latent gradient
    assert float((torch.from_numpy(gc["grad"]) - want_x).norm() / want_x.norm()) <= 1e-6
    _, gx32, gc32 = RC.joint_grad(w, ocfg, x, ts, ctx, cot, dtype=torch.float32)
    _, gx64, gc64 = RC.joint_grad(w, ocfg, x, ts, ctx, cot)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    print(f"\n[fixture] {tag}: context gradient, fp32 autograd vs fixture rel-L2 {rel(gc32, want_c):.2e}; float64 vs fixture {rel(gc64, want_c):.2e}; "
          f"latent gradient float64 vs fixture {rel(gx64, want_x):.2e}; max |grad_ctx| {float(want_c.abs().max()):.3f}")
    assert rel(gc32, want_c) <= 1e-5 and rel(gc64, want_c) <= 1e-5 and rel(gx64, want_x) <= 1e-5
    assert torch.equal(gx64, R.latent_grad(w, ocfg, x, ts, ctx, cot)[1])


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


def test_chunk_rule_is_the_documented_function_of_the_shape():
    """S at the four SD-v1 cross-attention shapes (64 x 64 latents, 8 samples, 8 heads): 11 / 8 / 2 / 1 -- the figures of DESIGN.md §13 -- and
    the workspace grows by S partial tiles of DB x 8 KiB per (sample, head, key tile)."""
    from perceptor_amd import _hip
    lib = _hip.lib()
    got = [lib.pmi_attn_flash_bwd_kv_chunks(8, t, 77, 8, d) for t, d in ((4096, 40), (1024, 80), (256, 160), (64, 160))]
    assert got == [11, 8, 2, 1], got
    for n, t, tk, heads, d in [(8, 4096, 77, 8, 40), (1, 4096, 77, 8, 40), (2, 1000, 33, 4, 64), (1, 100, 77, 2, 24), (2, 4096, 7, 8, 40), (1, 64, 77, 8, 160)]:
        s, _ = RC.kv_chunks(n, t, tk, heads)
        assert lib.pmi_attn_flash_bwd_kv_chunks(n, t, tk, heads, d) == s
        base = lib.pmi_attn_flash_bwd_workspace(n, t, tk, heads, d, 0)
        extra = n * heads * ((tk + 31) // 32) * s * ((d + 31) // 32) * 8 if s > 1 else 0
        assert lib.pmi_attn_flash_bwd_kv_workspace(n, t, tk, heads, d) == base + extra
    assert lib.pmi_attn_flash_bwd_kv_chunks(1, 64, 77, 8, 164) == -1 and lib.pmi_attn_flash_bwd_kv_workspace(1, 64, 77, 8, 168) == -1


@pytest.mark.parametrize("chunks", [1, 2, 5])
@pytest.mark.parametrize("tk", [7, 32, 33, 77])
@pytest.mark.parametrize("t,d", [(100, 24), (333, 40)])
def test_split_key_role_equals_autograd(t, d, tk, chunks):
    """T = 100 (4 query tiles) and 333 (11 tiles) are multiples neither of 32 nor of the chunk length."""
    g = torch.Generator().manual_seed(1000 * t + 10 * tk + chunks)
    q, k, v = (torch.randn((s, d), generator=g, dtype=torch.float64).requires_grad_() for s in (t, tk, tk))
    d_out = torch.randn((t, d), generator=g, dtype=torch.float64)
    scale = d ** -0.5
    (torch.softmax(q @ k.T * scale, dim=-1) @ v).backward(d_out)
    dk, dv, s_used = RC.kv_split_backward(q.detach(), k.detach(), v.detach(), d_out, scale, chunks)
    assert s_used == min(chunks, (t + 31) // 32) or chunks == 5
    for got, want in ((dk, k.grad), (dv, v.grad)):
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-10 * (1 + float(want.abs().max()))


# ---- defects of the context gradient against the bound ------------------------------------------------------------------------------------------
class _SwappedKvProjection(torch.autograd.Function):
    """k = ctx Wk^T, v = ctx Wv^T with the two transposed weights exchanged in the backward."""

    @staticmethod
    def forward(ctx_, c, wk, wv):
        ctx_.save_for_backward(wk, wv)
        return c @ wk.T, c @ wv.T

    @staticmethod
    def backward(ctx_, dk, dv):
        wk, wv = ctx_.saved_tensors
        return dk @ wv + dv @ wk, None, None


def _attention(sd_, k, x, ctx, heads, defect):
    """oracle.sd._attention with one defect of the cross-attention's context gradient."""
    n, t, c = x.shape
    d = c // heads
    cross = k.endswith("attn2")
    ck = ctx.detach() if cross and (defect == "dk_dropped" or defect == "layer_dropped:" + k) else ctx
    cv = ctx.detach() if cross and (defect == "dv_dropped" or defect == "layer_dropped:" + k) else ctx
    if cross and defect == "padded_keys_weighted":
        ck = cv = F.pad(ctx, (0, 0, 0, 32 - ctx.shape[1]))
    q = F.linear(x, sd_[k + ".to_q.weight"])
    if cross and defect == "to_k_to_v_swapped":
        kk, v = _SwappedKvProjection.apply(ctx, sd_[k + ".to_k.weight"], sd_[k + ".to_v.weight"])
    else:
        kk, v = F.linear(ck, sd_[k + ".to_k.weight"]), F.linear(cv, sd_[k + ".to_v.weight"])
    sp = lambda z: z.reshape(n, z.shape[1], heads, d).transpose(1, 2)
    s = sp(q) @ sp(kk).transpose(-1, -2) * d ** -0.5
    p = _SoftmaxNoDelta.apply(s) if cross and defect == "softmax_no_delta" else torch.softmax(s, dim=-1)
    return F.linear((p @ sp(v)).transpose(1, 2).reshape(n, t, c), sd_[k + ".to_out.0.weight"], sd_[k + ".to_out.0.bias"])


DEFECTS = ["dv_dropped", "dk_dropped", "softmax_no_delta", "padded_keys_weighted", "to_k_to_v_swapped"]


@pytest.mark.parametrize("cfg_name", ["SD_TINY", "SD_MID"])
def test_each_context_gradient_defect_breaks_the_bf16_bound_by_2x(cfg_name, monkeypatch):
    """The context gradient with one defect against the one without, float64 (softmax_no_delta and padded_keys_weighted in the
    cross-attention only: the self-attention's are tests/test_sd_unet_grad_cpu.py's).
    One layer's contribution dropped, for EVERY cross-attention layer: the gradient is a sum over the layers, so a global bound sees a
    dropped layer only as far as that layer's share goes.  SD_MID: every layer must clear 2x the bf16 bound.  SD_TINY has 11 layers and its
    mid block (4 x 4 latents, 16 queries) carries 0.055 of the gradient, 1.4x the bf16 bound: there the bound is reconsidered, not the
    defect -- every SD_TINY layer must clear 2x the f16 bound (6e-3; the engine tests run both dtypes on SD_TINY, and f16 is the dtype the
    class ships), and tests/test_gpu_sd_ctx_grad.py::test_engine_single_layer_context_gradient_vs_float64 checks each layer's own
    contribution on its own, in both dtypes, where no other layer can hide it."""
    ocfg = getattr(osd, cfg_name)
    w, x, ts, ctx, cot = _inputs(ocfg)
    _, _, exact = RC.joint_grad(w, ocfg, x, ts, ctx, cot)
    margins = {}
    layers = [k[:-len(".to_k.weight")] for k in osd.unet_state_dict_shapes(ocfg) if k.endswith(".attn2.to_k.weight")]
    shares = {}
    for d in DEFECTS + ["layer_dropped:" + l for l in layers]:
        with monkeypatch.context() as mp:
            mp.setattr(osd, "_attention", lambda s, k, xx, c, h, d=d: _attention(s, k, xx, c, h, d))
            _, _, bad = RC.joint_grad(w, ocfg, x, ts, ctx, cot)
        r = float((bad - exact).norm() / exact.norm())
        if d.startswith("layer_dropped:"):
            shares[d.split(":")[1].replace(".transformer_blocks.0.attn2", "")] = r
        else:
            margins[d] = r
    layer_bound = REL_BF16 if cfg_name == "SD_MID" else REL_F16
    print(f"\n[ctx layers] {cfg_name}: " + ", ".join(f"{l} {r:.3f}" for l, r in shares.items()) +
          f"; smallest {min(shares.values()):.3f} = {min(shares.values()) / layer_bound:.1f}x the bound {layer_bound}")
    for l, r in shares.items():
        assert r >= 2 * layer_bound, (cfg_name, l, r)
    # batch-1 encodings shared by the two samples: the gradient is the SUM over the samples; the defect returns one sample's share
    _, _, shared = RC.joint_grad(w, ocfg, x, ts, ctx[:1], cot)
    _, _, per_sample = RC.joint_grad(w, ocfg, x, ts, ctx[:1].expand(2, -1, -1), cot)
    assert shared.shape == (1,) + tuple(ctx.shape[1:])
    assert float((per_sample.sum(0, keepdim=True) - shared).norm() / shared.norm()) < 1e-12
    margins["expanded_batch_not_summed"] = float((per_sample[:1] - shared).norm() / shared.norm())
    print(f"\n[ctx defects] {cfg_name}: " + ", ".join(f"{d} {r:.3f} ({r / REL_BF16:.1f}x)" for d, r in margins.items()))
    for d, r in margins.items():
        assert r >= 2 * REL_BF16, (cfg_name, d, r)
