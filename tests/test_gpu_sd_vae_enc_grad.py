"""GPU: the VAE encoder's image gradient (engine/sd.py VaeEncoderEngine.forward_train / backward), the phased Downsample2D adjoint of
pmi_igemm under it, and the differentiable StableDiffusion.encode / latents built on it.

References: float64 autograd of oracle.sd.vae_encode_moments on the same name-keyed weights (the fp32 master copies, so the engine's 16-bit
weight rounding counts against it), and tests/golden/sd_ldm_vae_enc_{tiny,v1}_grad.npz, the image gradient of the reference's vendored
CompVis Encoder (tools/gen_sd_vae_enc_grad_golden.py).  Cotangents are seeded with a CLIP-like magnitude (~1e-6), so the f16 engine's
gradient scaling runs.  Bounds: those of tests/test_gpu_sd_vae_grad.py: rel-L2 bf16 2.5e-2 / f16 4e-3, cosine bf16 0.9995 /
f16 0.99999.  Measured values: DESIGN.md §14.
"""
import ctypes as C
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


# ---- pmi_igemm's phased geometry: the Downsample2D adjoint ---------------------------------------------------------------------------------------
def _adjoint_case(dtype, n, h, w, c, co, seed=0):
    """(packed weights, dy 16-bit NHWC on the CPU, float64 dx [n, 2h, 2w, co] by autograd through the padded stride-2 convolution on the
    weights and the gradient as the kernel holds them, i.e. rounded to 16 bits)."""
    from perceptor_amd import _hip
    from perceptor_amd.engine import sd
    from perceptor_amd.engine.ops import PackedLinear
    dt = _hip.dtype_code(dtype)
    tdt = _hip.TORCH_DTYPE[dt]
    gen = torch.Generator().manual_seed(11 + c + seed)
    wt = torch.randn((c, co, 3, 3), generator=gen) / (9 * c) ** 0.5           # Downsample2D conv: co input channels -> c output channels
    lin = PackedLinear(sd.pack_downsample_adjoint_weights(wt).float(), None, dt, "cuda")
    dy = torch.randn((n, h, w, c), generator=gen).to(tdt)
    w16 = torch.zeros((c, co, 3, 3), dtype=torch.float64)
    pk = lin.w.view(lin.n_p, 9, lin.cin_p)[:co, :, :c].double().cpu()         # [co, tap, c] in phase order
    for t, (ky, kx) in enumerate(sd.DOWN_ADJOINT_TAPS):
        w16[:, :, ky, kx] = pk[:, t, :].t()
    x = torch.zeros((n, co, 2 * h, 2 * w), dtype=torch.float64, requires_grad=True)
    F.conv2d(F.pad(x, (0, 1, 0, 1)), w16, stride=2).backward(dy.double().permute(0, 3, 1, 2))
    return lin, dy, x.grad.permute(0, 2, 3, 1)


SHAPES = [(2, 5, 9, 64, 32),        # W = 9: rows of a tile wrap image rows; M / 4 = 90 < one 128-row tile
          (1, 10, 18, 40, 20),      # 40 channels: not a multiple of the 64-deep k-tile (generic loader); N = 20: the 8-byte-store epilogue
          (3, 16, 16, 128, 256),    # tiles that straddle images, two column tiles
          (2, 13, 11, 192, 72),     # odd sizes on the buffer-load path, a ragged column tile
          (2, 64, 64, 128, 128)]    # one large shape: the first SD-v1 down-sampler's channels


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n,h,w,c,co", SHAPES)
def test_igemm_phased_downsample_adjoint_vs_float64_autograd(dtype, n, h, w, c, co):
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    lin, dy, want = _adjoint_case(dtype, n, h, w, c, co)
    tdt = _hip.TORCH_DTYPE[_hip.dtype_code(dtype)]
    out = torch.full((n, 2 * h, 2 * w, lin.n_p), float("nan"), dtype=tdt, device="cuda")
    got = ops.downsample_adjoint(dy.cuda(), lin, out=out).float().cpu()
    assert got.shape == (n, 2 * h, 2 * w, lin.n_p)
    assert bool(torch.isfinite(got).all())                                   # every pixel of every phase was written
    err = float((got[..., :co].double() - want).abs().max() / want.abs().max())
    print(f"\n[phased] {(n, h, w, c, co)} {dtype}: max err / max |want| {err:.3e}")
    assert err < (8e-3 if dtype == "bf16" else 1e-3), err                    # fp32 accumulation, one 16-bit output rounding
    again = ops.downsample_adjoint(dy.cuda(), lin).float().cpu()
    assert torch.equal(again, got)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_igemm_phased_downsample_adjoint_fp32_output(dtype):
    from perceptor_amd.engine import ops
    n, h, w, c, co = 2, 6, 10, 64, 12
    lin, dy, want = _adjoint_case(dtype, n, h, w, c, co, seed=3)
    out = torch.full((n, 2 * h, 2 * w, lin.n_p), float("nan"), dtype=torch.float32, device="cuda")
    got = ops.downsample_adjoint(dy.cuda(), lin, out=out).cpu()
    assert bool(torch.isfinite(got).all())
    err = float((got[..., :co].double() - want).abs().max() / want.abs().max())
    assert err < 1e-5, err                                                   # no output rounding: fp32 accumulation order only


def test_igemm_phased_argument_checks():
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops, sd
    from perceptor_amd.engine.ops import PackedLinear
    lin = PackedLinear(sd.pack_downsample_adjoint_weights(torch.randn(32, 32, 3, 3)).float(), None, _hip.DT_BF16, "cuda")
    dy = torch.zeros((1, 8, 8, 32), dtype=torch.bfloat16, device="cuda")
    out = torch.zeros((1, 16, 16, 32), dtype=torch.bfloat16, device="cuda")
    res = torch.zeros_like(out)
    f32 = torch.zeros((64,), dtype=torch.float32, device="cuda")

    def run(**over):
        a = ops.downsample_adjoint_args(dy, lin, out)
        for k, v in over.items():
            setattr(a, k, v)
        _hip.call("pmi_igemm", C.byref(a))

    run()                                                                    # the consistent call goes through
    for bad in (dict(stride=1), dict(taps=16, K=16 * 32), dict(taps=1, K=32), dict(H=8, W=8), dict(Hin=16, Win=16), dict(M=4 * 64 - 2),
                dict(R=res.data_ptr(), ldr=32), dict(res_up=1), dict(nbias=f32.data_ptr(), hw=256), dict(stats=f32.data_ptr(), stats_p=1),
                dict(splitk=2, ws=f32.data_ptr()), dict(batch=2, batch_inner=1), dict(split_out=32), dict(split_in=1),
                dict(A1=dy.data_ptr(), C1=32, lda1=32, K=9 * 64), dict(dtype=_hip.DT_F16X2)):
        with pytest.raises(RuntimeError):
            run(**bad)
    with pytest.raises(RuntimeError):
        ops.igemm(dy, lin, up=True, stride=2)                                # the nearest-upsampled stride-2 form is not the phased one


# ---- engine VJP against float64 autograd ------------------------------------------------------------------------------------------------------
_REF = {}


def _case(ocfg, hw, n):
    """(config, weights, images, (d_mean, d_logvar), float64 d loss / d images) -- computed once per case and shared by both dtypes."""
    key = (ocfg, hw, n)
    if key not in _REF:
        from oracle import sd as osd
        from perceptor_amd.engine import sd
        from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
        cfg = sd.VaeConfig(**ocfg.__dict__)
        w = synth_state_dict(sd.vae_encoder_state_dict_shapes(cfg), 0)
        img = seeded_noise((n, cfg.out_channels, hw, hw), 74) * 0.25 + 0.5
        down = 1 << (len(cfg.block_out) - 1)
        cot = seeded_noise((n, 2 * cfg.latent_channels, hw // down, hw // down), 93) * 1e-6
        w64 = {k: v.double() for k, v in w.items()}
        x64 = img.double().requires_grad_()
        mom = torch.cat(osd.vae_encode_moments(w64, ocfg, 2 * x64 - 1), 1)
        mom.backward(cot.double())
        lc = cfg.latent_channels
        _REF[key] = (cfg, w, img, (cot[:, :lc].contiguous(), cot[:, lc:].contiguous()), x64.grad.detach())
    return _REF[key]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", ["VAE_TINY-32-2", "C64-64-2", "VAE_V1-256-2"])
def test_engine_vjp_vs_float64_autograd(dtype, case):
    from oracle import sd as osd
    from perceptor_amd.engine import sd
    name, hw, n = case.split("-")
    ocfg = osd.VaeConfig(block_out=(32, 64, 64, 64), layers_per_block=1) if name == "C64" else getattr(osd, name)
    cfg, w, img, (dm, dl), want = _case(ocfg, int(hw), int(n))
    eng = sd.VaeEncoderEngine(cfg, w, "cuda", dtype)
    _, tape = eng.forward_train(img.cuda())
    got = eng.backward(tape, dm.cuda(), dl.cuda(), w).cpu()
    assert got.shape == img.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    rel, cos = _rel_cos(got, want)
    print(f"\n[vjp] {case} {dtype}: rel-L2 {rel:.3e} cos {cos:.7f} (bound {BOUND[dtype]})")
    assert rel < BOUND[dtype][0] and cos > BOUND[dtype][1], (case, dtype, rel, cos)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("tag", ["tiny", "v1"])
def test_engine_vjp_vs_reference_ldm_encoder_golden(dtype, tag):
    """The gradient of the reference's vendored CompVis Encoder with respect to its input x = 2 * img - 1 (quant_conv as a plain conv2d):
    the engine's image gradient carries the factor 2 on top."""
    from oracle import sd as osd
    from perceptor_amd.engine import sd
    from perceptor_amd.utils.synth import synth_state_dict
    g = np.load(os.path.join(GOLDEN, f"sd_ldm_vae_enc_{tag}_grad.npz"))
    ocfg = osd.VAE_TINY if tag == "tiny" else osd.VAE_V1
    cfg = sd.VaeConfig(**ocfg.__dict__)
    w = synth_state_dict(sd.vae_encoder_state_dict_shapes(cfg), 0)
    eng = sd.VaeEncoderEngine(cfg, w, "cuda", dtype)
    x, cot, want = torch.from_numpy(g["x"]), torch.from_numpy(g["cotangent"]), torch.from_numpy(g["grad"])
    (mean, logvar), tape = eng.forward_train(((x + 1) / 2).cuda())
    mom, ref = torch.cat([mean, logvar], 1).cpu(), torch.cat([torch.from_numpy(g["mean"]), torch.from_numpy(g["logvar"])], 1)
    assert float((mom - ref).norm() / ref.norm()) < BOUND[dtype][0]
    lc = cfg.latent_channels
    got = eng.backward(tape, cot[:, :lc].contiguous().cuda(), cot[:, lc:].contiguous().cuda(), w).cpu()
    rel, cos = _rel_cos(got, 2.0 * want)
    print(f"\n[golden] {tag} {dtype}: rel-L2 {rel:.3e} cos {cos:.7f}")
    assert rel < BOUND[dtype][0] and cos > BOUND[dtype][1], (tag, dtype, rel, cos)


# ---- SD-v1 at 512 x 512 x 4: bits ---------------------------------------------------------------------------------------------------------------
def test_sd_v1_512_bitwise_forward_repeatable_backward_batch_invariance():
    from perceptor_amd.engine import sd
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    w = synth_state_dict(sd.vae_encoder_state_dict_shapes(sd.VAE_V1), 0)
    eng = sd.VaeEncoderEngine(sd.VAE_V1, w, "cuda", "bf16")
    img = (seeded_noise((4, 3, 512, 512), 74) * 0.25 + 0.5).cuda()
    ref = eng.forward(img)
    (mean, logvar), tape = eng.forward_train(img)
    assert torch.equal(mean, ref[0]) and torch.equal(logvar, ref[1])    # head dim 512: the same launch sequence, bit for bit
    dm, dl = (seeded_noise((4, 4, 64, 64), 93) * 1e-6).cuda(), (seeded_noise((4, 4, 64, 64), 94) * 1e-6).cuda()
    g1 = eng.backward(tape, dm, dl, w)
    g2 = eng.backward(tape, dm, dl, w)
    assert g1.shape == img.shape and g1.dtype == torch.float32
    assert torch.equal(g1, g2) and bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    del tape
    _, tape1 = eng.forward_train(img[:1].contiguous())
    g0 = eng.backward(tape1, dm[:1].contiguous(), dl[:1].contiguous(), w)
    rel, cos = _rel_cos(g0, g1[:1])
    print(f"\n[batch] sample 0 of batch 4 vs batch 1: bitwise {torch.equal(g0, g1[:1])} rel-L2 {rel:.3e} cos {cos:.7f}")
    assert rel < BOUND["bf16"][0] and cos > BOUND["bf16"][1]


def test_engine_errors():
    from perceptor_amd.engine import sd
    from perceptor_amd.utils.synth import synth_state_dict
    cfg = sd.VaeConfig(block_out=(32, 64), layers_per_block=1)
    w = synth_state_dict(sd.vae_encoder_state_dict_shapes(cfg), 0)
    eng = sd.VaeEncoderEngine(cfg, w, "cuda", "bf16")
    img = torch.zeros((1, 3, 16, 16))
    with pytest.raises(RuntimeError):
        eng.forward_train(img)
    with pytest.raises(ValueError):
        eng.forward_train(img[:, :2].cuda())
    (mean, logvar), tape = eng.forward_train(img.cuda())
    assert mean.shape == (1, 4, 8, 8)
    with pytest.raises(RuntimeError):
        eng.backward(tape, torch.zeros_like(mean).cpu(), torch.zeros_like(mean), w)
    with pytest.raises(RuntimeError):
        eng.backward(tape, torch.zeros_like(mean), torch.zeros_like(mean).cpu(), w)
    with pytest.raises(ValueError):
        eng.backward(tape, torch.zeros_like(mean)[..., :4], torch.zeros_like(mean), w)
    with pytest.raises(ValueError):
        eng.backward(tape, torch.zeros_like(mean), torch.zeros_like(mean)[:, :2], w)
    # d_logvar = None is d_logvar = 0
    dm = torch.full_like(mean, 1e-3)
    assert torch.equal(eng.backward(tape, dm, None, w), eng.backward(tape, dm, torch.zeros_like(dm), w))


# ---- the class surface ---------------------------------------------------------------------------------------------------------------------------
TINY_TEXT = (16, 520, 32, 2, 1, 32)


def _tiny_sd():
    from perceptor_amd import models
    from perceptor_amd.engine import sd
    cfg = sd.SdConfig(block_out=(32, 64, 64), cross_attn=(True, True, False), heads=2, context_dim=32)
    vae = sd.VaeConfig(block_out=(32, 64, 64, 64), layers_per_block=1)
    return models.StableDiffusion(fp16=True, config=cfg, vae_config=vae, text_config=TINY_TEXT).to("cuda")


def _images(n=2, hw=32):
    from perceptor_amd.utils.synth import seeded_noise
    return (seeded_noise((n, 3, hw, hw), 74) * 0.25 + 0.5).cuda()


def test_latents_mode_gradient_is_the_engines_backward():
    from perceptor_amd.engine import sampler
    from perceptor_amd.utils.synth import seeded_noise
    m = _tiny_sd()
    x = _images().requires_grad_()
    z = m.latents(x)
    assert z.grad_fn is not None and z.shape == (2, 4, 4, 4)
    assert _rel_cos(z.detach(), m.latents(x.detach()))[0] < BOUND["bf16"][0]      # (64-wide head: forward's d64 kernel vs the batched GEMMs)
    g = (seeded_noise((2, 4, 4, 4), 95) * 1e-6).cuda()
    z.backward(g)
    assert x.grad is not None and x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    eng = m._engine("encoder")
    _, tape = eng.forward_train(x.detach())
    assert torch.equal(x.grad, eng.backward(tape, sampler.lincomb2(g, 0.18215), None, m.vae.state_dict()))


def test_encode_sample_gradient_keeps_the_noise_and_the_clamp():
    from perceptor_amd.engine import sampler
    from perceptor_amd.utils.synth import seeded_noise
    m = _tiny_sd()
    eng = m._engine("encoder")
    x = _images().requires_grad_()
    g = (seeded_noise((2, 4, 4, 4), 95) * 1e-6).cuda()
    try:
        sampler.rng.manual_seed(1234)
        z = m.encode(x, method="sample")
        assert z.grad_fn is not None
        z.backward(g)
        sampler.rng.manual_seed(1234)                                      # the same draw again, by hand
        (mean, logvar), tape = eng.forward_train(x.detach())
        noise = sampler.randn_like(mean)
    finally:
        sampler.rng.generator = None
    std = torch.exp(0.5 * logvar.clamp(-30.0, 20.0))
    assert torch.equal(z.detach(), sampler.lincomb2(mean, 0.18215, noise * std, 0.18215))
    inside = (logvar > -30.0) & (logvar < 20.0)
    d_logvar = sampler.lincomb2(g * (noise * std * inside), 0.18215 * 0.5)
    want = eng.backward(tape, sampler.lincomb2(g, 0.18215), d_logvar, m.vae.state_dict())
    assert torch.equal(x.grad, want)
    assert not torch.equal(want, eng.backward(tape, sampler.lincomb2(g, 0.18215), None, m.vae.state_dict()))    # the logvar branch is there


def test_encode_sample_gradient_is_zero_where_logvar_is_clamped():
    """quant_conv's logvar bias pushed past the clamp on both sides: d_logvar is exactly 0 there, so a cotangent that only reaches logvar
    (zero-weight mean rows) leaves an exactly zero image gradient."""
    from perceptor_amd.utils.synth import seeded_noise
    m = _tiny_sd()
    with torch.no_grad():
        m.vae.state_dict()["quant_conv.bias"][4:6] = 50.0
        m.vae.state_dict()["quant_conv.bias"][6:8] = -50.0
        m.vae.state_dict()["quant_conv.weight"][:4] = 0.0                  # mean does not depend on the image: only logvar carries gradient
    m._drop_caches()
    x = _images().requires_grad_()
    z = m.encode(x, method="sample")
    (_, logvar) = m._engine("encoder").forward(x.detach())
    assert bool(((logvar >= 20.0) | (logvar <= -30.0)).all())
    z.backward((seeded_noise((2, 4, 4, 4), 95) * 1e-3).cuda())
    assert x.grad is not None and float(x.grad.abs().max()) == 0.0


def test_encode_without_grad_is_the_plain_encoder():
    from perceptor_amd.engine import sampler
    m = _tiny_sd()
    x = _images(1)
    a = m.latents(x)
    assert a.grad_fn is None
    xr = x.clone().requires_grad_()
    with torch.no_grad():
        b = m.latents(xr)
    assert b.grad_fn is None and torch.equal(a, b)
    mean, _ = m._engine("encoder").forward(x)
    assert torch.equal(a, sampler.lincomb2(mean, 0.18215))
    assert m.encode(x, method="sample").grad_fn is None
    with pytest.raises(NotImplementedError):
        with m.finetuneable_vae():
            pass


def test_image_to_latents_to_unet_chain_reaches_the_pixels():
    from perceptor_amd.utils.synth import seeded_noise
    m = _tiny_sd()
    ids = torch.tensor([[518, 5, 9, 300, 519] + [519] * 11])
    pos = m.conditioning(token_ids=ids)
    x = _images().requires_grad_()
    z = m.latents(x)
    noise = seeded_noise((2, 4, 4, 4), 96).cuda()
    eps = m.predicted_noise(m.diffuse_latents(z, 600, noise), 600, pos)
    assert eps.grad_fn is not None
    ((eps - noise) ** 2).mean().backward()
    assert x.grad is not None and x.grad.shape == x.shape
    assert bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
