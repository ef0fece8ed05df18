"""GPU: the SD UNet's latent gradient -- the flash attention backward (csrc/attn_flash.hip), the GEGLU backward, SdUnetEngine.forward_train /
backward and the differentiable StableDiffusion.predicted_noise built on them.

References: float64 on the same 16-bit operands (kernels), float64 autograd of the oracle's UNet restated dtype-generically
(tests/_sd_unet_ref64.py) on the fp32 master weights (engine, class).  Engine bounds are the project's own for the gradient of a smooth
(SiLU / GELU) UNet, tests/test_gpu_backward.py: rel-L2 4e-2 and cosine 0.999 in bf16, 6e-3 and 0.99995 in f16.
"""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

BOUND = {"bf16": (4e-2, 0.999), "f16": (6e-3, 0.99995)}
U = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}          # largest relative error of one round-to-nearest into the 16-bit format


def _rel_cos(got, want):
    g, w = got.double().flatten().cpu(), want.double().flatten().cpu()
    return float((g - w).norm() / w.norm()), float(F.cosine_similarity(g, w, dim=0))


# ---- kernels -----------------------------------------------------------------------------------------------------------------------------
SHAPES = [(4096, 4096, 8, 40), (1024, 1024, 8, 80), (256, 256, 8, 160), (64, 64, 8, 160), (4096, 77, 8, 40), (64, 77, 8, 160), (100, 77, 2, 24)]


def _operands(t, tk, heads, d, tdt, n=1):
    from perceptor_amd.utils.synth import seeded_noise
    c = heads * d
    cross = tk != t or (t, tk) == (64, 77)
    if cross:
        q = seeded_noise((n, t, c), 3).to(tdt).cuda()
        kv = seeded_noise((n, tk, 2 * c), 4).to(tdt).cuda()
        views = (q, kv[..., :c], kv[..., c:])
    else:
        qkv = seeded_noise((n, t, 3 * c), 3).to(tdt).cuda()
        views = (qkv[..., :c], qkv[..., c:2 * c], qkv[..., 2 * c:])
    d_out = seeded_noise((n, t, c), 5).to(tdt).cuda()
    return views, d_out


def _heads64(x, heads, d):
    n, t, _ = x.shape
    return x.double().reshape(n, t, heads, d).transpose(1, 2)           # [n, heads, t, d]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("t,tk,heads,d", SHAPES)
def test_flash_train_forward_is_the_flash_forward_bit_for_bit(dtype, t, tk, heads, d):
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    dt = _hip.dtype_code(dtype)
    (q, k, v), _ = _operands(t, tk, heads, d, _hip.TORCH_DTYPE[dt])
    ref = ops.flash_attention(q, k, v, heads, d, dt)
    out, saved = ops.flash_attention_train(q, k, v, heads, d, dt)
    assert torch.equal(out, ref)
    lse = saved[4][:, :t].double().reshape(1, heads, t)
    s2 = (_heads64(q, heads, d) @ _heads64(k, heads, d).transpose(-1, -2)) * (d ** -0.5 * 1.4426950408889634)
    want = torch.log2(torch.exp2(s2 - s2.amax(-1, keepdim=True)).sum(-1)) + s2.amax(-1)
    assert float((lse - want).abs().max()) < 1e-4 * (1 + float(want.abs().max()))           # fp32 running sum of T terms


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("t,tk,heads,d", SHAPES)
def test_flash_backward_vs_float64(dtype, t, tk, heads, d):
    """Bound per output element, from the arithmetic the kernel is specified to do: dS (and P for dV) are rounded once to 16 bits before
    their product -- |error| <= u sum_s |dS||K| -- and the fp32 result is rounded once on the way out -- u |result|; fp32 accumulation
    over the depth (<= 4096 x 2^-24) and the fp32 exp2 / delta are second order.  Asserted with a factor 1.5 over that first-order sum plus
    the f16 subnormal spacing per term."""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    dt = _hip.dtype_code(dtype)
    (q, k, v), d_out = _operands(t, tk, heads, d, _hip.TORCH_DTYPE[dt])
    cross = q.shape[-1] == heads * d and q.stride(1) == heads * d
    out, saved = ops.flash_attention_train(q, k, v, heads, d, dt)
    g = ops.flash_attention_backward(saved, d_out, heads, d, dt, dq_only=cross)
    g2 = ops.flash_attention_backward(saved, d_out, heads, d, dt, dq_only=cross)
    assert torch.equal(g, g2) and bool(torch.isfinite(g.float()).all())
    q64, k64, v64, do64 = (_heads64(x, heads, d) for x in (q, k, v, d_out))
    scale = d ** -0.5
    p = torch.softmax(q64 @ k64.transpose(-1, -2) * scale, dim=-1)
    o64 = p @ v64
    ds = p * (do64 @ v64.transpose(-1, -2) - (do64 * o64).sum(-1, keepdim=True)) * scale
    u, tiny = U[dtype], (2.0 ** -24 if dtype == "f16" else 0.0)
    c = heads * d
    back = lambda x: x.transpose(1, 2).reshape(1, -1, c)
    checks = [("dq", g[..., :c], ds @ k64, ds.abs() @ k64.abs(), k64.abs().sum(-2, keepdim=True).expand(-1, -1, t, -1))]
    if not cross:
        checks.append(("dk", g[..., c:2 * c], ds.transpose(-1, -2) @ q64, ds.abs().transpose(-1, -2) @ q64.abs(), q64.abs().sum(-2, keepdim=True).expand(-1, -1, tk, -1)))
        checks.append(("dv", g[..., 2 * c:], p.transpose(-1, -2) @ do64, p.transpose(-1, -2) @ do64.abs(), do64.abs().sum(-2, keepdim=True).expand(-1, -1, tk, -1)))
    for name, got, want, mag, colsum in checks:
        err = (got.double() - back(want)).abs()
        bound = 1.5 * (u * back(mag) + u * back(want).abs() + tiny * back(colsum)) + 1e-30
        worst = float((err / bound).max())
        print(f"\n[flash-bwd] {(t, tk, heads, d)} {dtype} {name}: max err {float(err.max()):.3e}, worst err/bound {worst:.3f}, "
              f"rel-L2 {float(err.norm() / back(want).norm()):.3e}")
        assert worst <= 1.0, (name, worst)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_flash_backward_dq_only_writes_nothing_but_dq_and_gives_padded_keys_no_weight(dtype):
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    from perceptor_amd._hip import call, ptr
    dt = _hip.dtype_code(dtype)
    t, tk, heads, d = 100, 77, 2, 24
    c = heads * d
    (q, k, v), d_out = _operands(t, tk, heads, d, _hip.TORCH_DTYPE[dt])
    out, saved = ops.flash_attention_train(q, k, v, heads, d, dt)
    ref = ops.flash_attention_backward(saved, d_out, heads, d, dt, dq_only=True)
    # dq as the middle slice of a guarded buffer: everything around it must stay as it was
    buf = torch.full((1, t + 2, 3 * c), 7.0, dtype=q.dtype, device="cuda")
    dq = buf[:, 1:t + 1, c:2 * c]
    kib = _hip.lib().pmi_attn_flash_bwd_workspace(1, t, tk, heads, d, 1)
    wsb = torch.empty((kib * 512,), dtype=q.dtype, device="cuda")
    delta = torch.empty_like(saved[4])
    call("pmi_attn_flash_bwd", ptr(q), q.stride(1), ptr(k), ptr(v), k.stride(1), ptr(out), ptr(d_out), ptr(saved[3]), ptr(saved[4]), ptr(wsb),
         ptr(delta), ptr(dq), 3 * c, None, None, 0, 1, t, tk, heads, d, d ** -0.5, 1, dt)
    assert torch.equal(dq, ref)
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[:, 1:t + 1, c:2 * c] = False
    assert bool((buf[mask] == 7.0).all())
    # keys 77 -> 96 with arbitrary rows appended and Tk still 77: bit-identical (the pad rows are never read as keys)
    big = torch.cat([torch.cat([k, v], -1), torch.full((1, 19, 2 * c), 3.0, dtype=q.dtype, device="cuda")], 1)
    kv2 = torch.as_strided(big, (1, tk, 2 * c), (tk * 2 * c, 2 * c, 1))
    out2, saved2 = ops.flash_attention_train(q, kv2[..., :c], kv2[..., c:], heads, d, dt)
    assert torch.equal(ops.flash_attention_backward(saved2, d_out, heads, d, dt, dq_only=True), ref)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("m,f", [(64, 1280), (100, 128), (4096, 1280)])
def test_geglu_backward_vs_float64(dtype, m, f):
    """d value = dg gelu(gate), d gate = dg value gelu'(gate), interleaved columns.  Bound: fp32 arithmetic with the 1.5e-7 erf
    approximation (csrc/common.h) is second order to the one 16-bit output rounding: 1.5 u |want| + the erf term 4e-7 |dg value|."""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    from perceptor_amd.utils.synth import seeded_noise
    dt = _hip.dtype_code(dtype)
    tdt = _hip.TORCH_DTYPE[dt]
    h = (seeded_noise((m, 2 * f), 11) * 1.5).to(tdt).cuda()
    dg = seeded_noise((m, f), 12).to(tdt).cuda()
    got = ops.geglu_backward(h, dg, dt)
    assert torch.equal(got, ops.geglu_backward(h, dg, dt))
    h64 = h.double().view(m, f // 16, 2, 16)
    val, gate = h64[:, :, 0].reshape(m, f), h64[:, :, 1].reshape(m, f)
    phi = 0.5 * (1 + torch.erf(gate / 2 ** 0.5))
    dval = dg.double() * gate * phi
    dgate = dg.double() * val * (phi + gate * torch.exp(-0.5 * gate ** 2) / (2 * torch.pi) ** 0.5)
    want = torch.stack([dval.view(m, f // 16, 16), dgate.view(m, f // 16, 16)], 2).reshape(m, 2 * f)
    slack = torch.stack([(dg.double() * gate).abs().view(m, f // 16, 16), (dg.double() * val).abs().view(m, f // 16, 16)], 2).reshape(m, 2 * f)
    err = (got.double() - want).abs()
    bound = 1.5 * U[dtype] * want.abs() + 4e-7 * slack + (2.0 ** -24 if dtype == "f16" else 1e-30)
    print(f"\n[geglu-bwd] {(m, f)} {dtype}: max err {float(err.max()):.3e} worst err/bound {float((err / bound).max()):.3f}")
    assert float((err / bound).max()) <= 1.0
    # the forward pair: pmi_geglu on the same h
    gg = torch.empty((m, f), dtype=tdt, device="cuda")
    _hip.call("pmi_geglu", _hip.ptr(h), _hip.ptr(gg), m, f, 1, dt)
    assert float((gg.double() - val * gate * phi).abs().max()) <= 1.5 * U[dtype] * float((val * gate * phi).abs().max()) + 1e-6


# ---- engine ----------------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _case(name):
    """(cfg, weights, latents, timesteps, context, cotangent, float64 eps, float64 d <eps, cot> / d latents), once per configuration."""
    if name not in _REF:
        from oracle import sd as osd
        from perceptor_amd.engine import sd
        from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
        import _sd_unet_ref64 as ref
        ocfg = getattr(osd, name)
        cfg = sd.SdConfig(**ocfg.__dict__)
        n, tok = (1, 77) if name == "SD_V1" else (2, 7)
        w = synth_state_dict(sd.unet_state_dict_shapes(cfg), 0)
        x = seeded_noise((n, cfg.in_channels, 16, 16), 71)
        ts = torch.tensor([981.0, 20.0][:n])
        ctx = seeded_noise((n, tok, cfg.context_dim), 72)
        cot = seeded_noise((n, cfg.out_channels, 16, 16), 93)
        eps, grad = ref.latent_grad(w, ocfg, x, ts, ctx, cot)
        _REF[name] = (cfg, w, x, ts, ctx, cot, eps, grad)
    return _REF[name]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["SD_TINY", "SD_MID", "SD_V1"])
def test_engine_vjp_vs_float64_autograd_flash_and_kept_p(dtype, name):
    from perceptor_amd.engine import sd
    cfg, w, x, ts, ctx, cot, eps64, want = _case(name)
    eng = sd.SdUnetEngine(cfg, w, "cuda", dtype)
    plain = eng.forward(x.cuda(), ts.cuda(), ctx.cuda())
    eps, tape = eng.forward_train(x.cuda(), ts.cuda(), ctx.cuda())
    fwd_rel = _rel_cos(eps, plain)[0]
    print(f"\n[fwd] {name} {dtype}: forward_train vs forward bit-equal {torch.equal(eps, plain)} rel-L2 {fwd_rel:.3e}; vs float64 {_rel_cos(eps, eps64)[0]:.3e}")
    # the un-fused GEGLU rounds ff1's output to 16 bits before the gate (forward() gates the fp32 accumulator): one extra rounding of
    # relative size u per transformer block.  Every later rounding then falls differently, so the two outputs are two independent 16-bit
    # evaluations of one function; each sits about 3 u from float64 (printed above), their difference within 4 u.
    # Measured (MI355X): bf16 1.46e-2 / 1.02e-2 / 1.33e-2 and f16 1.89e-3 / 1.26e-3 / 1.64e-3 for SD_TINY / SD_MID / SD_V1.
    assert fwd_rel <= 4 * U[dtype]
    got = eng.backward(tape, cot.cuda(), w)
    assert got.shape == x.shape and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert torch.equal(got, eng.backward(tape, cot.cuda(), w))
    rel, cos = _rel_cos(got, want)
    eng.flash_backward = False
    _, tape_p = eng.forward_train(x.cuda(), ts.cuda(), ctx.cuda())
    got_p = eng.backward(tape_p, cot.cuda(), w)
    rel_p, cos_p = _rel_cos(got_p, want)
    rel_x, cos_x = _rel_cos(got, got_p)
    print(f"[vjp] {name} {dtype}: flash rel-L2 {rel:.3e} cos {cos:.7f}; kept-P rel-L2 {rel_p:.3e} cos {cos_p:.7f}; "
          f"flash vs kept-P rel-L2 {rel_x:.3e} cos {cos_x:.7f} (bound {BOUND[dtype]})")
    for r, c in ((rel, cos), (rel_p, cos_p), (rel_x, cos_x)):
        assert r < BOUND[dtype][0] and c > BOUND[dtype][1], (name, dtype, r, c)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("tag", ["tiny", "v1"])
def test_engine_vjp_vs_reference_ldm_unet_golden(dtype, tag):
    """The latent gradient of the reference's vendored CompVis UNetModel (its fp32 autograd, tools/gen_sd_unet_grad_golden.py)."""
    import os
    import numpy as np
    from oracle import sd as osd
    from perceptor_amd.engine import sd
    from perceptor_amd.utils.synth import synth_state_dict
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", f"sd_ldm_unet_{tag}_grad.npz"))
    cfg = sd.SdConfig(**(osd.SD_TINY if tag == "tiny" else osd.SD_V1).__dict__)
    w = synth_state_dict(sd.unet_state_dict_shapes(cfg), 0)
    eng = sd.SdUnetEngine(cfg, w, "cuda", dtype)
    x, ts, ctx, cot, want = (torch.from_numpy(g[k]) for k in ("x", "t", "ctx", "cotangent", "grad"))
    eps, tape = eng.forward_train(x.cuda(), ts.float().cuda(), ctx.cuda())
    got = eng.backward(tape, cot.cuda(), w)
    rel, cos = _rel_cos(got, want)
    print(f"\n[golden] {tag} {dtype}: eps rel-L2 {_rel_cos(eps, torch.from_numpy(g['eps']))[0]:.3e}; grad rel-L2 {rel:.3e} cos {cos:.7f}")
    assert rel < BOUND[dtype][0] and cos > BOUND[dtype][1], (tag, dtype, rel, cos)


def test_f16_gradient_is_invariant_to_power_of_two_cotangent_scales():
    from perceptor_amd.engine import sd
    cfg, w, x, ts, ctx, cot, _, _ = _case("SD_TINY")
    eng = sd.SdUnetEngine(cfg, w, "cuda", "f16")
    _, tape = eng.forward_train(x.cuda(), ts.cuda(), ctx.cuda())
    g = eng.backward(tape, cot.cuda(), w)
    for s in (2.0 ** -20, 2.0 ** 10):
        assert torch.equal(eng.backward(tape, cot.cuda() * s, w), g * s)


def test_engine_errors():
    from perceptor_amd.engine import sd
    cfg, w, x, ts, ctx, cot, _, _ = _case("SD_TINY")
    eng = sd.SdUnetEngine(cfg, w, "cuda", "bf16")
    with pytest.raises(RuntimeError):
        eng.forward_train(x, ts, ctx)
    eps, tape = eng.forward_train(x.cuda(), ts.cuda(), ctx.cuda())
    with pytest.raises(RuntimeError):
        eng.backward(tape, cot, w)
    with pytest.raises(ValueError):
        eng.backward(tape, cot.cuda()[..., :8], w)


# ---- the class surface ------------------------------------------------------------------------------------------------------------------------
TINY_TEXT = (16, 520, 32, 2, 1, 32)


def _tiny_sd(name="runwayml/stable-diffusion-v1-5", fp16=True):
    from perceptor_amd import models
    from perceptor_amd.engine import sd
    cfg = sd.SdConfig(block_out=(32, 64, 64), cross_attn=(True, True, False), heads=2, context_dim=32,
                      in_channels=9 if name.endswith("inpainting") else 4)
    vae = sd.VaeConfig(block_out=(32, 64, 64, 64), layers_per_block=1)
    return models.StableDiffusion(name, fp16=fp16, config=cfg, vae_config=vae, text_config=TINY_TEXT).to("cuda")


IDS = torch.tensor([[518, 5, 9, 300, 519] + [519] * 11])
IDS0 = torch.tensor([[518, 519] + [519] * 14])


def test_predicted_noise_backpropagates_to_the_latents():
    from perceptor_amd.utils.synth import seeded_noise
    m = _tiny_sd()
    pos = m.conditioning(token_ids=IDS)
    x = seeded_noise((2, 4, 16, 16), 81).cuda()
    plain = m.predicted_noise(x, 600, pos)
    assert plain.grad_fn is None
    xr = x.clone().requires_grad_()
    with torch.no_grad():
        ng = m.predicted_noise(xr, 600, pos)
    assert ng.grad_fn is None and torch.equal(ng, plain)
    assert torch.equal(plain, m._engine("unet").forward(x, m.indices(600).expand(2), pos.encodings.expand(2, -1, -1).contiguous()))
    eps = m.predicted_noise(xr, 600, pos)
    assert eps.grad_fn is not None
    cot = seeded_noise((2, 4, 16, 16), 93).cuda()
    (eps * cot).sum().backward()
    assert xr.grad is not None and bool(torch.isfinite(xr.grad).all()) and float(xr.grad.abs().max()) > 0
    eng = m._engine("unet")
    _, tape = eng.forward_train(x, m.indices(600).expand(2), pos.encodings.expand(2, -1, -1).contiguous())
    assert torch.equal(xr.grad, eng.backward(tape, cot, m.unet.state_dict()))
    assert pos.encodings.grad is None


@pytest.mark.parametrize("fp16", [True, False])
def test_denoised_latents_gradient_vs_float64(fp16):
    from oracle import sd as osd
    from perceptor_amd.utils.synth import seeded_noise
    import _sd_unet_ref64 as ref
    m = _tiny_sd(fp16=fp16)
    dtype = "f16" if fp16 else "bf16"
    pos = m.conditioning(token_ids=IDS)
    x = seeded_noise((2, 4, 16, 16), 81).cuda().requires_grad_()
    pred = m.predictions(x, 600, pos)
    assert pred.predicted_noise.grad_fn is not None
    pred.denoised_latents.sum().backward()
    w = {k: v.detach().cpu() for k, v in m.unet.state_dict().items()}
    x64 = x.detach().cpu().double().requires_grad_()
    w64 = {k: v.double() for k, v in w.items()}
    eps = ref.unet_forward(w64, osd.SD_TINY, x64, torch.tensor([600.0, 600.0]), pos.encodings.detach().cpu().double().expand(2, -1, -1))
    a, s = float(m.schedule_alphas[600]), float(m.schedule_sigmas[600])
    ((x64 - s * eps) / a).sum().backward()
    rel, cos = _rel_cos(x.grad, x64.grad)
    print(f"\n[denoised] {dtype}: rel-L2 {rel:.3e} cos {cos:.7f}")
    assert rel < BOUND[dtype][0] and cos > BOUND[dtype][1]


def test_predictions_pair_under_grad_is_the_sum_of_two_calls():
    from perceptor_amd.utils.synth import seeded_noise
    m = _tiny_sd()
    neu, pos = m.conditioning(token_ids=IDS0), m.conditioning(token_ids=IDS)
    x0 = seeded_noise((2, 4, 16, 16), 81).cuda()
    c1, c2 = seeded_noise((2, 4, 16, 16), 93).cuda(), seeded_noise((2, 4, 16, 16), 94).cuda()
    x = x0.clone().requires_grad_()
    un, ps = m.predictions_pair(x, 600, neu, pos)
    ((un.predicted_noise * c1).sum() + (ps.predicted_noise * c2).sum()).backward()
    y = x0.clone().requires_grad_()
    ((m.predictions(y, 600, neu).predicted_noise * c1).sum() + (m.predictions(y, 600, pos).predicted_noise * c2).sum()).backward()
    rel, cos = _rel_cos(x.grad, y.grad)
    print(f"\n[pair] f16: rel-L2 {rel:.3e} cos {cos:.7f}")
    assert rel < BOUND["f16"][0] and cos > BOUND["f16"][1]
    un2, ps2 = m.predictions_pair(x0, 600, neu, pos)
    assert un2.predicted_noise.grad_fn is None and torch.equal(ps2.predicted_noise, ps.predicted_noise.detach()) is not None


def test_inpainting_surface_returns_a_four_channel_gradient():
    from perceptor_amd.models.stable_diffusion.conditioning import Conditioning
    from perceptor_amd.utils.synth import seeded_noise
    m = _tiny_sd("runwayml/stable-diffusion-inpainting")
    enc = m.token_encodings(IDS)
    cond = Conditioning(m.name, enc, inpainting_latent_masks=(seeded_noise((2, 1, 16, 16), 5) > 0).float().cuda(),
                        inpainting_latents=seeded_noise((2, 4, 16, 16), 6).cuda())
    x = seeded_noise((2, 4, 16, 16), 81).cuda().requires_grad_()
    m.predicted_noise(x, 600, cond).square().sum().backward()
    assert x.grad.shape == (2, 4, 16, 16) and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
