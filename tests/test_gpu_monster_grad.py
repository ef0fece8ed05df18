"""GPU: MonsterDiffusion's input gradient.  The FIR adjoints pmi_fir_down2_bwd / pmi_fir_up2_bwd (csrc/fir.hip) and the EDM staging adjoints
pmi_edm_stage_out_bwd / pmi_edm_stage_in_bwd (csrc/sampling.hip) against float64 with the per-element bounds of
tests/_monster_grad_ref64.py; MonsterEngine.forward_train / backward on the fixture's two tiny networks against the reference's own autograd
values (tests/golden/monster_diffusion_grad_reference.npz) and against the emulated float64 gradient, per sample and over the batch; the
product configuration against float64 autograd of the restatement; the public class with input_grad=True.

Every comparison prints its worst |got - ref| / bound (or rel-L2 / gate) before it asserts.  Gates: every gradient lies behind a GroupNorm
or a softmax, so each is 2 x the rel-L2 of the EMULATED float64 gradient (emulate=dtype) against the float64 one, measured on the CPU per
sample and over the batch (_monster_grad_ref64.EMU_GRAD*, which tests/test_monster_grad_cpu.py measures again on every run): bf16
3.4e-3 .. 1.0e-2, f16 4.5e-4 .. 1.5e-3.  Per sample matters: in network A sigma = (0.3, 40) puts a factor of about 18 between the two
samples' network gradients, and a batch norm would hide the smaller one; gx is gated on its own because at small sigma the analytic
2 c_skip d term carries most of d_images.  No gate comes from a GPU result.  tests/test_monster_grad_cpu.py runs the seeded defects at these
inputs.
"""
import pytest
import torch

import _monster_grad_ref64 as G
import _monster_ref64 as M
from conftest import golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7B7B                      # a 16-bit pattern (about 6.1e4 in f16, 1.3e36 in bf16) no kernel under test produces
DT_CODE = {"f16": 0, "bf16": 1}


def _lib():
    from perceptor_amd import _hip
    return _hip.lib()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _filled(n, dtype):
    return torch.full((n,), SENTINEL, dtype=torch.int16, device=DEV).view(M.TD[dtype])


def _bits(t):
    return t.contiguous().view(torch.int16)


def _ratio(tag, got, ref, tol):
    r = float(((got.double().cpu() - ref).abs() / tol).max())
    print(f"[monster grad] {tag}: worst |got - ref| / bound {r:.3f}")
    return r


def _gated(tag, dist, gates):
    """dist, gates: per sample, then the batch -> the worst ratio, every figure printed"""
    print(f"[monster grad] {tag}: rel-L2 " + " ".join(f"{d:.3e}" for d in dist) + " | gate " + " ".join(f"{g:.3e}" for g in gates)
          + " | ratio " + " ".join(f"{d / g:.3f}" for d, g in zip(dist, gates)))
    return max(d / g for d, g in zip(dist, gates))


# ---- 1. FIR adjoints ------------------------------------------------------------------------------------------------------------------------
def _fir_bwd(which, dy16, out, dx_shape, dtype):
    n, h, w, c = dx_shape
    fn = _lib().pmi_fir_down2_bwd if which == "down" else _lib().pmi_fir_up2_bwd
    rc = fn(dy16.data_ptr(), out.data_ptr(), n, h, w, c, DT_CODE[dtype], _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("which,shapes", [("down", s) for s in G.fir_bwd_shapes("down")] + [("up", s) for s in G.fir_bwd_shapes("up")])
def test_fir_adjoint_kernel(which, shapes, dtype):
    dx_shape, dy_shape = shapes
    gy = M.fir_input(dy_shape, 23 + dx_shape[1] * dx_shape[2], dtype)
    ref, tol = G.fir_bwd_ref(gy, which, dtype)
    assert tuple(ref.shape) == tuple(dx_shape)
    gy16 = gy.to(M.TD[dtype]).to(DEV)
    guard = 512
    buf = _filled(ref.numel() + guard, dtype)
    assert _fir_bwd(which, gy16, buf, dx_shape, dtype) == 0
    got = buf[:ref.numel()].view(ref.shape)
    assert _ratio(f"pmi_fir_{which}2_bwd {dx_shape} {dtype}", got, ref, tol) <= 1.0
    assert bool((_bits(buf[ref.numel():]) == SENTINEL).all()), "bytes past the output were written"
    again = _filled(ref.numel() + guard, dtype)
    assert _fir_bwd(which, gy16, again, dx_shape, dtype) == 0
    assert torch.equal(_bits(buf), _bits(again)), "two runs differ"
    # the engine's wrapper is the same launch
    from perceptor_amd.engine import ops
    wrapped = (ops.fir_down2_bwd if which == "down" else ops.fir_up2_bwd)(gy16, DT_CODE[dtype])
    assert tuple(wrapped.shape) == tuple(dx_shape) and torch.equal(_bits(wrapped), _bits(got))


@pytest.mark.parametrize("which", ["down", "up"])
def test_fir_adjoints_refuse_out_of_contract_calls(which):
    bad = [(1, 1, 4, 32), (1, 4, 1, 32), (1, 4, 4, 12), (0, 4, 4, 32)] + ([(1, 3, 4, 32), (1, 4, 6 + 1, 32)] if which == "down" else [])
    fn = _lib().pmi_fir_down2_bwd if which == "down" else _lib().pmi_fir_up2_bwd
    x = torch.zeros(8192, dtype=torch.float16, device=DEV)
    out = _filled(8192, "f16")
    for n, h, w, c in bad:
        assert fn(x.data_ptr(), out.data_ptr(), n, h, w, c, 0, _stream()) == -1, (n, h, w, c)
    assert fn(x.data_ptr(), out.data_ptr(), 1, 4, 4, 32, 2, _stream()) == -1          # the precise (hi + lo) type has no FIR kernel
    assert fn(None, out.data_ptr(), 1, 4, 4, 32, 0, _stream()) == -1
    assert fn(x.data_ptr(), None, 1, 4, 4, 32, 0, _stream()) == -1
    assert fn(x.data_ptr() + 2, out.data_ptr(), 1, 4, 4, 32, 0, _stream()) == -1      # 16-byte loads need aligned pointers
    assert fn(x.data_ptr(), out.data_ptr() + 2, 1, 4, 4, 32, 0, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((_bits(out) == SENTINEL).all())


# ---- 2. EDM adjoints ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(4))
def test_edm_adjoint_kernels(case):
    sigma = M.edm_sigma_cases()[case][0]
    I = G.edm_bwd_inputs()
    n, _, h, w = M.EDM_SHAPE
    dev = lambda t: t.float().to(DEV).contiguous()
    d, sg = dev(I["d"]), dev(sigma)
    worst = 0.0
    for dtype, scale in (("f16", 1.0), ("f16", 2.0 ** 9), ("bf16", 1.0)):
        g16 = _filled(n * h * w * 8 + 64, dtype)
        assert _lib().pmi_edm_stage_out_bwd(d.data_ptr(), sg.data_ptr(), sigma.numel(), 0.5, scale, g16.data_ptr(), n, h, w, 8, DT_CODE[dtype],
                                            _stream()) == 0
        torch.cuda.synchronize()
        got = g16[:n * h * w * 8].view(n, h, w, 8)
        ref, tol = G.edm_stage_out_bwd_ref(I["d"], sigma, scale, dtype)
        worst = max(worst, _ratio(f"pmi_edm_stage_out_bwd {case} {dtype} scale {scale:g}", got[..., :3].permute(0, 3, 1, 2), ref, tol))
        assert bool((got[..., 3:] == 0).all()) and bool((_bits(g16[n * h * w * 8:]) == SENTINEL).all())
    for ld, inv_scale in ((4, 1.0), (8, 2.0 ** -9)):
        gx = torch.zeros(n, h, w, ld)
        gx[..., :3] = I["gx"].permute(0, 2, 3, 1).float()
        gx[..., 3:] = 1e30                                                   # the padding is never read
        out = torch.full((n * 3 * h * w + 64,), 7.0, device=DEV)
        assert _lib().pmi_edm_stage_in_bwd(d.data_ptr(), gx.to(DEV).data_ptr(), ld, sg.data_ptr(), sigma.numel(), 0.5, inv_scale, out.data_ptr(),
                                           n, h, w, _stream()) == 0
        torch.cuda.synchronize()
        ref, tol = G.edm_stage_in_bwd_ref(I["d"], I["gx"], sigma, inv_scale)
        worst = max(worst, _ratio(f"pmi_edm_stage_in_bwd {case} ld {ld}", out[:n * 3 * h * w].view(n, 3, h, w), ref, tol))
        assert bool((out[n * 3 * h * w:] == 7.0).all())
    assert worst <= 1.0
    # out of contract: nothing launched
    out = torch.full((64,), 7.0, device=DEV)
    assert _lib().pmi_edm_stage_in_bwd(d.data_ptr(), d.data_ptr(), 2, sg.data_ptr(), sigma.numel(), 0.5, 1.0, out.data_ptr(), n, h, w, _stream()) == -1
    assert _lib().pmi_edm_stage_in_bwd(d.data_ptr(), d.data_ptr(), 4, sg.data_ptr(), 2 if n != 2 else 5, 0.5, 1.0, out.data_ptr(), n, h, w, _stream()) == -1
    assert _lib().pmi_edm_stage_out_bwd(d.data_ptr(), sg.data_ptr(), sigma.numel(), 0.5, 0.0, out.data_ptr(), n, h, w, 8, 1, _stream()) == -1
    assert _lib().pmi_edm_stage_out_bwd(d.data_ptr(), sg.data_ptr(), sigma.numel(), 0.5, 1.0, out.data_ptr(), n, h, w, 8, 2, _stream()) == -1
    assert _lib().pmi_edm_stage_out_bwd(d.data_ptr(), sg.data_ptr(), sigma.numel(), 0.5, 1.0, out.data_ptr(), n, h, w, 4, 1, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_adagn_gelu_backward_layer(dtype):
    """one AdaGN + exact GELU backward as the engine launches it, a per-sample film row and the single row of a scalar sigma (film_ld = 0)"""
    from perceptor_amd._hip import ACT_GELU
    from perceptor_amd.engine import ops
    assert ACT_GELU == G.GELU_CODE
    x, film, dy = G.adagn_bwd_case(dtype)
    x16, dy16 = x.to(M.TD[dtype]).to(DEV), dy.to(M.TD[dtype]).to(DEV)
    groups, dt = x.shape[-1] // 32, DT_CODE[dtype]
    for f in (film, film[:1]):
        fd = f.float().to(DEV).contiguous()
        kw = dict(film=fd, film_ld=fd.stride(0) if fd.shape[0] > 1 else 0)
        ca, cb, parts = ops.group_norm_coeffs_train(x16, None, None, groups, dt, **kw)
        got = ops.group_norm_backward(x16, dy16, ca, cb, parts, None, groups, dt, act=ACT_GELU, **kw)[0]
        assert _ratio(f"adagn + gelu backward {dtype} rows {f.shape[0]}", got, *G.adagn_bwd_ref(x, f, dy, dtype)) <= 1.0


# ---- 3. engine on the fixture's networks ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fwd():
    return golden("monster_diffusion_reference")


@pytest.fixture(scope="module")
def fixture():
    return golden("monster_diffusion_grad_reference")


@pytest.fixture(scope="module")
def emulated(fwd, fixture):
    """the emulated float64 gradients, computed once per (network, dtype)"""
    cache = {}

    def get(net, dtype):
        if (net, dtype) not in cache:
            config, _ = M.NETS[net]
            cache[(net, dtype)] = G.grad64(M.synthetic_state_dict(config), fwd[f"{net}_in"].double(), fwd[f"{net}_sigma"], config,
                                           fixture[f"{net}_cotangent"], emulate=dtype)
        return cache[(net, dtype)]

    return get


def _name(net, k):
    return f"{net}_{k}" if k in ("gx", "d_images") else f"{net}_g_{k}"


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("net", ["A", "B"])
def test_engine_gradients(net, dtype, fwd, fixture, emulated):
    from perceptor_amd.engine.monster import MonsterEngine
    config, shape = M.NETS[net]
    sd = M.synthetic_state_dict(config)
    eng = MonsterEngine(config, sd, DEV, dtype)
    x, sigma = fwd[f"{net}_in"].to(DEV), fwd[f"{net}_sigma"].float().to(DEV)
    plain = eng.forward(x, sigma)
    den, tape = eng.forward_train(x, sigma)
    torch.cuda.synchronize()
    assert torch.equal(den, plain), "forward_train's denoised_xs differs from forward's"
    cot = fixture[f"{net}_cotangent"].to(DEV)
    taps = {}
    d_images = eng.backward(tape, cot, sd, taps=taps)
    again = eng.backward(tape, cot, sd)
    torch.cuda.synchronize()
    assert torch.equal(d_images, again), "two backward runs on one tape differ"
    assert torch.equal(eng.forward(x, sigma), plain)                           # (the lazily packed transposes left the forward alone)
    emu = emulated(net, dtype)
    worst = 0.0
    for k in G.grad_keys(config):
        got = (d_images if k == "d_images" else taps[k].permute(0, 3, 1, 2)).double().cpu().contiguous()
        gates = tuple(2 * v for v in G.EMU_GRAD[(net, dtype)][k])
        worst = max(worst, _gated(f"{net} {dtype} {k} vs emulation", G.per_sample(got, emu[k]), gates))
        worst = max(worst, _gated(f"{net} {dtype} {k} vs fixture", G.per_sample_sampled(got, fixture, _name(net, k)), gates))
    assert worst <= 1.0


# ---- 4. product config -----------------------------------------------------------------------------------------------------------------------
def test_product_config_gradient():
    """batch 2 at 16 x 16, sigma (0.5, 5): d = 64 heads x 2 / 4 / 8 and the 512-channel routes; then a scalar sigma, the one-row film_ld = 0 case"""
    from perceptor_amd.engine.monster import MonsterEngine
    sd = M.synthetic_state_dict(M.PRODUCT)
    img, sigma, cot = G.product_grad_case()
    ref = G.grad64(sd, img.double(), sigma.double(), M.PRODUCT, cot)
    one = torch.tensor([G.PRODUCT_SCALAR_SIGMA])
    ref1 = G.grad64(sd, img.double(), one.double(), M.PRODUCT, cot)
    worst = 0.0
    for dtype in ("bf16", "f16"):
        eng = MonsterEngine(M.PRODUCT, sd, DEV, dtype)
        for tag, sg, r, table in (("per-sample sigma", sigma, ref, G.EMU_GRAD_PRODUCT), ("scalar sigma", one, ref1, G.EMU_GRAD_PRODUCT_SCALAR)):
            den, tape = eng.forward_train(img.to(DEV), sg.to(DEV))
            assert torch.equal(den, eng.forward(img.to(DEV), sg.to(DEV)))
            taps = {}
            d_images = eng.backward(tape, cot.to(DEV), sd, taps=taps)
            for k, got in (("gx", taps["gx"].permute(0, 3, 1, 2)), ("d_images", d_images)):
                gates = tuple(2 * v for v in table[dtype][k])
                worst = max(worst, _gated(f"product {dtype} {tag} {k}", G.per_sample(got.double().cpu(), r[k]), gates))
    assert worst <= 1.0


# ---- 5. public class ---------------------------------------------------------------------------------------------------------------------------
def _model(dtype, input_grad, net="A"):
    from perceptor_amd.models import MonsterDiffusion
    return MonsterDiffusion(config=M.NETS[net][0], dtype=dtype, input_grad=input_grad).to(DEV)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_public_class_input_gradient(dtype, fwd, fixture):
    m, m0 = _model(dtype, True), _model(dtype, False)
    sigma = fwd["A_sigma"].float().to(DEV)
    cot = fixture["A_cotangent"].to(DEV)
    d_ref = fixture["A_d_images"]
    gates = tuple(2 * v for v in G.EMU_GRAD[("A", dtype)]["d_images"])
    today = m0.predictions(fwd["A_in"].to(DEV), sigma)
    x = fwd["A_in"].to(DEV).requires_grad_()
    with torch.enable_grad():
        pred = m.predictions(x, sigma)
        assert pred.denoised_xs.requires_grad and torch.equal(pred.denoised_xs.detach(), today.denoised_xs)
        (pred.denoised_images * (2 * cot)).sum().backward()                    # denoised_images = (denoised_xs + 1) / 2
    worst = _gated(f"public {dtype} x.grad", G.per_sample(x.grad.double().cpu(), d_ref), gates)
    # eps = (x - denoised) / sigma and step(to) = decode(denoised + eps to): d <eps, w> / d img = (2 w - J^T w) / sigma and
    # d <step, w> / d img = ((1 - r) J^T w + 2 r w) / 2 with r = to / sigma, J^T w = the fixture's d_images; their error is J^T w's, scaled
    s4 = fwd["A_sigma"].double().reshape(-1, 1, 1, 1)
    to = fwd["A_to_sigma"].float()
    r4 = to.double().reshape(-1, 1, 1, 1) / s4
    w64 = fixture["A_cotangent"].double()
    for tag, fn, want, err_of in (("eps", lambda p: p.eps, (2 * w64 - d_ref) / s4, d_ref / s4),
                                  ("step", lambda p: p.step(to.to(DEV)), ((1 - r4) * d_ref + 2 * r4 * w64) / 2, (1 - r4) * d_ref / 2)):
        xg = fwd["A_in"].to(DEV).requires_grad_()
        with torch.enable_grad():
            p = m.predictions(xg, sigma)
            out = fn(p)
            assert out.requires_grad
            (out * cot).sum().backward()
        got = xg.grad.double().cpu()
        dist = tuple(float((got[i] - want[i]).norm() / err_of[i].norm()) for i in range(2)) + (float((got - want).norm() / err_of.norm()),)
        worst = max(worst, _gated(f"public {dtype} gradient through {tag}", dist, gates))
        # the values on the graph are the fused kernel's, to fp32 rounding
        ref_val = getattr(today, tag) if tag == "eps" else today.step(to.to(DEV))
        assert M.rel_l2(out.detach().cpu(), ref_val.cpu()) < 1e-6
    assert worst <= 1.0
    # no graph wanted: today's outputs, bit for bit
    def values(images):
        p = m.predictions(images, sigma)
        assert not p.denoised_xs.requires_grad
        return p.denoised_xs, p.eps, p.denoised_images, p.step(to.to(DEV))

    with torch.no_grad():
        quiet = values(fwd["A_in"].to(DEV).requires_grad_())
    for vals in (quiet, values(fwd["A_in"].to(DEV))):
        for got, ref in zip(vals, (today.denoised_xs, today.eps, today.denoised_images, today.step(to.to(DEV)))):
            assert torch.equal(got, ref)
    # what is not differentiated is refused, never silently detached
    with torch.enable_grad():
        with pytest.raises(NotImplementedError):
            m.predictions(fwd["A_in"].to(DEV).requires_grad_(), sigma.clone().requires_grad_())
        with pytest.raises(NotImplementedError):
            m.predictions(fwd["A_in"].to(DEV), sigma, torch.zeros(2, 9, device=DEV).requires_grad_())
        with pytest.raises(NotImplementedError):
            m0.predictions(fwd["A_in"].to(DEV).requires_grad_(), sigma)
