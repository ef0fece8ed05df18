"""GPU: the VAE decoder's input gradient (engine/sd.py VaeDecoderEngine.forward_train / backward) and the differentiable
StableDiffusion.decode built on it.

References: float64 autograd of oracle.sd.vae_decode on the same name-keyed weights (the fp32 master copies, so the engine's 16-bit weight
rounding counts against it), and tests/golden/sd_ldm_vae_{tiny,v1}_grad.npz, the z-gradient of the reference's vendored CompVis Decoder
(tools/gen_sd_vae_grad_golden.py).  Cotangents are seeded with a CLIP-like magnitude (~1e-6), so the f16 engine's gradient scaling runs.
Bounds: rel-L2 against float64 within the SD forward budget of tests/test_gpu_sd.py (bf16 2.5e-2, f16 4e-3), cosine of the
ADM gradients (bf16 0.9995, f16 0.99999).
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = {"bf16": (2.5e-2, 0.9995), "f16": (4e-3, 0.99999)}
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def _rel_cos(got, want):
    g, w = got.double().flatten(), want.double().flatten()
    return float((g - w).norm() / w.norm()), float(F.cosine_similarity(g, w, dim=0))


# ---- pmi_igemm taps 16: the folded Upsample2D adjoint ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w,cin,cout", [(2, 8, 12, 64, 32), (1, 10, 18, 40, 24), (3, 16, 16, 128, 256)])
def test_igemm_taps16_vs_float64_conv(dtype, n, h, w, cin, cout):
    """dx = conv2d(dy, W', stride 2, padding 1) over the high-resolution gradient [n, 2h, 2w, cin].  Covers W = 2w not a multiple of 32,
    M = n h w not a multiple of the 128-row tile, a channel count that is not a multiple of the 64-deep k-tile (generic loader)."""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    from perceptor_amd.engine.ops import PackedLinear
    dt = _hip.dtype_code(dtype)
    tdt = _hip.TORCH_DTYPE[dt]
    gen = torch.Generator().manual_seed(5 + cin)
    wf = torch.randn((cout, cin, 4, 4), generator=gen) / (16 * cin) ** 0.5
    lin = PackedLinear(wf, None, dt, "cuda")
    dy = torch.randn((n, 2 * h, 2 * w, cin), generator=gen).to(tdt)
    out = torch.full((n, h, w, lin.n_p), float("nan"), dtype=tdt, device="cuda")
    got = ops.igemm(dy.cuda(), lin, stride=2, out=out).float().cpu()
    w16 = lin.w.view(lin.n_p, 4, 4, lin.cin_p)[:cout, :, :, :cin].permute(0, 3, 1, 2).double().cpu()
    want = F.conv2d(dy.double().permute(0, 3, 1, 2), w16, stride=2, padding=1).permute(0, 2, 3, 1)
    assert bool(torch.isfinite(got).all())
    err = float((got[..., :cout].double() - want).abs().max() / want.abs().max())
    assert err < (8e-3 if dtype == "bf16" else 1e-3), err           # fp32 accumulation, one 16-bit output rounding
    again = ops.igemm(dy.cuda(), lin, stride=2).float().cpu()
    assert torch.equal(again, got)


def test_igemm_taps16_argument_checks():
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    from perceptor_amd.engine.ops import PackedLinear
    lin = PackedLinear(torch.randn(32, 32, 4, 4), None, _hip.DT_BF16, "cuda")
    dy = torch.zeros((1, 8, 8, 32), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(RuntimeError):
        ops.igemm(dy, lin)                     # a 4x4 window is only defined at stride 2
    with pytest.raises(RuntimeError):
        ops.igemm(dy, lin, up=True, stride=2)


# ---- engine VJP against float64 autograd ------------------------------------------------------------------------------------------------------
_REF = {}


def _case(ocfg_name, hw, n):
    """(weights, latents, cotangent, float64 d loss / d latents) -- computed once per case and shared by both dtypes."""
    key = (ocfg_name, hw, n)
    if key not in _REF:
        from oracle import sd as osd
        from perceptor_amd.engine import sd
        from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
        ocfg = getattr(osd, ocfg_name) if isinstance(ocfg_name, str) else ocfg_name
        cfg = sd.VaeConfig(**ocfg.__dict__)
        w = synth_state_dict(sd.vae_decoder_state_dict_shapes(cfg), 0)
        z = seeded_noise((n, cfg.latent_channels, hw, hw), 73)
        up = 1 << (len(cfg.block_out) - 1)
        d_img = seeded_noise((n, cfg.out_channels, up * hw, up * hw), 91) * 1e-6
        w64 = {k: v.double() for k, v in w.items()}
        z64 = z.double().requires_grad_()
        img = (osd.vae_decode(w64, ocfg, z64 / 0.18215) + 1) / 2
        img.backward(d_img.double())
        _REF[key] = (cfg, w, z, d_img, z64.grad.detach())
    return _REF[key]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", ["VAE_TINY-16-2", "C64-8-2", "VAE_V1-32-2"])
def test_engine_vjp_vs_float64_autograd(dtype, case):
    from oracle import sd as osd
    from perceptor_amd.engine import sd
    name, hw, n = case.split("-")
    ocfg = osd.VaeConfig(block_out=(32, 64, 64, 64), layers_per_block=1) if name == "C64" else getattr(osd, name)
    cfg, w, z, d_img, want = _case(ocfg, int(hw), int(n))
    eng = sd.VaeDecoderEngine(cfg, w, "cuda", dtype)
    img, tape = eng.forward_train(z.cuda())
    got = eng.backward(tape, d_img.cuda(), w).cpu()
    assert got.shape == z.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    rel, cos = _rel_cos(got, want)
    print(f"\n[vjp] {case} {dtype}: rel-L2 {rel:.3e} cos {cos:.7f} (bound {BOUND[dtype]})")
    assert rel < BOUND[dtype][0] and cos > BOUND[dtype][1], (case, dtype, rel, cos)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("tag", ["tiny", "v1"])
def test_engine_vjp_vs_reference_ldm_decoder_golden(dtype, tag):
    """The z-gradient of the reference's vendored CompVis Decoder (post_quant_conv as a plain conv2d, no 1/0.18215, no (x+1)/2)."""
    from oracle import sd as osd
    from perceptor_amd.engine import sd
    from perceptor_amd.utils.synth import synth_state_dict
    g = np.load(os.path.join(GOLDEN, f"sd_ldm_vae_{tag}_grad.npz"))
    ocfg = osd.VAE_TINY if tag == "tiny" else osd.VAE_V1
    cfg = sd.VaeConfig(**ocfg.__dict__)
    w = synth_state_dict(sd.vae_decoder_state_dict_shapes(cfg), 0)
    eng = sd.VaeDecoderEngine(cfg, w, "cuda", dtype)
    z, cot, want = torch.from_numpy(g["z"]), torch.from_numpy(g["cotangent"]), torch.from_numpy(g["grad"])
    x, tape = eng.forward_train(z.cuda(), scale=1.0, to_images=False)
    assert float((x.cpu() - torch.from_numpy(g["dec"])).norm() / torch.from_numpy(g["dec"]).norm()) < BOUND[dtype][0]
    got = eng.backward(tape, cot.cuda(), w).cpu()
    rel, cos = _rel_cos(got, want)
    print(f"\n[golden] {tag} {dtype}: rel-L2 {rel:.3e} cos {cos:.7f}")
    assert rel < BOUND[dtype][0] and cos > BOUND[dtype][1], (tag, dtype, rel, cos)


# ---- SD-v1 at 512 x 512 x 4: bits ---------------------------------------------------------------------------------------------------------------
def test_sd_v1_512_bitwise_forward_repeatable_backward_batch_invariance():
    from perceptor_amd.engine import sd
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    w = synth_state_dict(sd.vae_decoder_state_dict_shapes(sd.VAE_V1), 0)
    eng = sd.VaeDecoderEngine(sd.VAE_V1, w, "cuda", "bf16")
    z = seeded_noise((4, 4, 64, 64), 73).cuda()
    ref = eng.forward(z)
    img, tape = eng.forward_train(z)
    assert torch.equal(img, ref)                                      # head dim 512: the same launch sequence, bit for bit
    d = (seeded_noise((4, 3, 512, 512), 91) * 1e-6).cuda()
    g1 = eng.backward(tape, d, w)
    g2 = eng.backward(tape, d, w)
    assert torch.equal(g1, g2) and bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    del tape
    _, tape1 = eng.forward_train(z[:1].contiguous())
    g0 = eng.backward(tape1, d[:1].contiguous(), w)
    rel, cos = _rel_cos(g0, g1[:1])
    print(f"\n[batch] sample 0 of batch 4 vs batch 1: bitwise {torch.equal(g0, g1[:1])} rel-L2 {rel:.3e} cos {cos:.7f}")
    assert rel < BOUND["bf16"][0] and cos > BOUND["bf16"][1]


def test_engine_errors():
    from perceptor_amd.engine import sd
    from perceptor_amd.utils.synth import synth_state_dict
    cfg = sd.VaeConfig(block_out=(32, 64), layers_per_block=1)
    w = synth_state_dict(sd.vae_decoder_state_dict_shapes(cfg), 0)
    eng = sd.VaeDecoderEngine(cfg, w, "cuda", "bf16")
    z = torch.zeros((1, 4, 8, 8))
    with pytest.raises(RuntimeError):
        eng.forward_train(z)
    with pytest.raises(ValueError):
        eng.forward_train(z[:, :3].cuda())
    img, tape = eng.forward_train(z.cuda())
    with pytest.raises(RuntimeError):
        eng.backward(tape, torch.zeros_like(img).cpu(), w)
    with pytest.raises(ValueError):
        eng.backward(tape, torch.zeros_like(img)[..., :8], w)


# ---- the class surface ---------------------------------------------------------------------------------------------------------------------------
TINY_TEXT = (16, 520, 32, 2, 1, 32)


def _tiny_sd():
    from perceptor_amd import models
    from perceptor_amd.engine import sd
    cfg = sd.SdConfig(block_out=(32, 64, 64), cross_attn=(True, True, False), heads=2, context_dim=32)
    vae = sd.VaeConfig(block_out=(32, 64, 64, 64), layers_per_block=1)
    return models.StableDiffusion(fp16=True, config=cfg, vae_config=vae, text_config=TINY_TEXT).to("cuda")


def test_decode_is_differentiable_and_guides_a_step():
    from perceptor_amd import losses
    from perceptor_amd.utils.synth import seeded_noise
    m = _tiny_sd()
    loss = losses.OpenCLIP("sdvae-tiny-vit", "synthetic", quick_gelu=True, config=(32, 8, 64, 2, 1, 32)).to("cuda")
    loss.add_encodings_(F.normalize(seeded_noise((2, 32), 7)))
    ids = torch.tensor([[518, 5, 9, 300, 519] + [519] * 11])
    pos = m.conditioning(token_ids=ids)
    x = seeded_noise((2, 4, 4, 4), 81).cuda()
    pred = m.predictions(x, 600, pos)
    dl = pred.denoised_latents.detach().requires_grad_()
    img = m.decode(dl)
    assert img.grad_fn is not None and img.shape == (2, 3, 32, 32)
    img.retain_grad()
    loss(img).backward()
    assert dl.grad is not None and bool(torch.isfinite(dl.grad).all()) and float(dl.grad.abs().max()) > 0
    # the same bits as the engine applied to that image gradient, and that gradient is loss_and_grad's
    eng = m._engine("decoder")
    _, tape = eng.forward_train(dl.detach())
    assert torch.equal(dl.grad, eng.backward(tape, img.grad, m.vae.state_dict()))
    _, g_img = loss.loss_and_grad(img.detach())
    assert _rel_cos(img.grad, g_img)[0] < 1e-3               # the loss's autograd route and its fused route
    assert torch.equal(eng.backward(tape, g_img, m.vae.state_dict()), eng.backward(tape, g_img.clone(), m.vae.state_dict()))
    nxt = pred.guided(dl.grad).step(560)
    assert nxt.shape == x.shape and bool(torch.isfinite(nxt).all())
    assert m.images(dl).grad_fn is not None


def test_decode_without_grad_is_the_plain_decoder():
    from perceptor_amd.utils.synth import seeded_noise
    m = _tiny_sd()
    z = seeded_noise((1, 4, 4, 4), 81).cuda()
    a = m.decode(z)
    assert a.grad_fn is None
    zr = z.clone().requires_grad_()
    with torch.no_grad():
        b = m.decode(zr)
    assert b.grad_fn is None and torch.equal(a, b)
    assert torch.equal(a, m._engine("decoder").forward(z))
