"""GPU: MonsterDiffusion.  The FIR resamplers (csrc/fir.hip) and the EDM kernels (csrc/sampling.hip) against float64 with the per-element
bounds of tests/_monster_ref64.py; engine/monster.py's MonsterEngine on the fixture's two tiny networks, checkpoint by checkpoint, against the
emulated float64 restatement and against the reference's own values (tests/golden/monster_diffusion_reference.npz); the product
configuration against the float64 restatement; the public class's samplers against the recorded trajectories; HIP-graph capture.

Every comparison prints its worst |got - ref| / bound (or rel-L2 / gate) before it asserts.  tests/test_monster_diffusion_cpu.py runs the
seeded defects at these inputs.  Measured figures: DESIGN.md section 22.

Gates of the engine, product and sampler tests.  proj_in comes before any normalisation: the random-walk count holds there, rel-L2 <=
sqrt(R) u with R = 2 (the staged input and proj_in's own output).  Every later checkpoint lies behind a GroupNorm or a softmax, which
rescale the accumulated error, so the gate is 2 x the rel-L2 of the EMULATED float64 restatement (emulate=dtype) against the float64
values, measured on the CPU when this test was written: bf16 3.6e-3 .. 7.9e-3 per checkpoint (9.7e-3 at the product config, up to 1.3e-2 at
the last Heun yield), f16 3.0e-4 .. 9.4e-4 (1.2e-3, 1.4e-3).  The tables are _monster_ref64.EMU*, which tests/test_monster_diffusion_cpu.py
measures again on every run.  No gate comes from a GPU result.
"""
import math

import pytest
import torch

import _monster_ref64 as M
from conftest import golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7B7B                      # a 16-bit pattern (about 6.1e4 in f16, 1.3e36 in bf16) no kernel under test produces
DT_CODE = {"f16": 0, "bf16": 1}
EMU, EMU_PRODUCT, EMU_HEUN, EMU_LMS, gate = M.EMU, M.EMU_PRODUCT, M.EMU_HEUN, M.EMU_LMS, M.gate


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
    print(f"[monster] {tag}: worst |got - ref| / bound {r:.3f}")
    return r


def _rel(tag, got, ref, g):
    r = M.rel_l2(got.double().cpu(), ref)
    print(f"[monster] {tag}: rel-L2 {r:.3e} gate {g:.3e} ratio {r / g:.3f}")
    return r


# ---- 1. FIR resamplers ----------------------------------------------------------------------------------------------------------------------
def _fir(which, x16, out, dtype):
    n, h, w, c = x16.shape
    fn = _lib().pmi_fir_down2 if which == "down" else _lib().pmi_fir_up2
    rc = fn(x16.data_ptr(), out.data_ptr(), n, h, w, c, DT_CODE[dtype], _stream())
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("which,shape", [("down", s) for s in M.FIR_DOWN_SHAPES] + [("up", s) for s in M.FIR_UP_SHAPES])
def test_fir_kernel(which, shape, dtype):
    x = M.fir_input(shape, 11 + shape[1] * shape[2], dtype)
    _, tol = M.fir_ref(x, which, dtype)
    y = M.fir_torch(x, which)                                   # float64 F.pad(reflect) + conv2d / conv_transpose2d
    x16 = x.to(M.TD[dtype]).to(DEV)
    guard = 512
    buf = _filled(y.numel() + guard, dtype)
    assert _fir(which, x16, buf, dtype) == 0
    got = buf[:y.numel()].view(y.shape)
    assert _ratio(f"fir_{which} {shape} {dtype}", got, y, tol) <= 1.0
    assert bool((_bits(buf[y.numel():]) == SENTINEL).all()), "bytes past the output were written"
    again = _filled(y.numel() + guard, dtype)
    assert _fir(which, x16, again, dtype) == 0
    assert torch.equal(_bits(buf), _bits(again)), "two runs differ"


@pytest.mark.parametrize("which", ["down", "up"])
def test_fir_refuses_out_of_contract_shapes(which):
    bad = [(1, 1, 4, 32), (1, 4, 1, 32), (1, 4, 4, 12), (0, 4, 4, 32)] + ([(1, 3, 4, 32), (1, 4, 6 + 1, 32)] if which == "down" else [])
    fn = _lib().pmi_fir_down2 if which == "down" else _lib().pmi_fir_up2
    x = torch.zeros(4096, dtype=torch.float16, device=DEV)
    out = _filled(8192, "f16")
    for n, h, w, c in bad:
        assert fn(x.data_ptr(), out.data_ptr(), n, h, w, c, 0, _stream()) == -1, (n, h, w, c)
    assert fn(x.data_ptr(), out.data_ptr(), 1, 4, 4, 32, 2, _stream()) == -1          # the precise (hi + lo) type has no FIR kernel
    assert fn(None, out.data_ptr(), 1, 4, 4, 32, 0, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((_bits(out) == SENTINEL).all())


# ---- 2. EDM kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(4))
def test_edm_kernels(case):
    from perceptor_amd.engine import sampler
    sigma, to, prev, rev = M.edm_sigma_cases()[case]
    I = M.edm_inputs()
    n, _, h, w = M.EDM_SHAPE
    dev = lambda t: t.float().to(DEV).contiguous()
    img, sg = dev(I["img"]), dev(sigma)
    worst = 0.0
    for dtype in ("f16", "bf16"):
        x16 = _filled(n * h * w * 8 + 64, dtype)
        cn = torch.empty(sigma.numel(), dtype=torch.float32, device=DEV)
        assert _lib().pmi_edm_stage_in(img.data_ptr(), sg.data_ptr(), sigma.numel(), 0.5, x16.data_ptr(), cn.data_ptr(), n, h, w, 8,
                                       DT_CODE[dtype], _stream()) == 0
        torch.cuda.synchronize()
        v, v_tol, c, c_tol = M.edm_stage_in_ref(I["img"], sigma, dtype)
        got = x16[:n * h * w * 8].view(n, h, w, 8)
        worst = max(worst, _ratio(f"stage_in {case} {dtype}", got[..., :3].permute(0, 3, 1, 2), v, v_tol))
        assert bool((got[..., 3:] == 0).all()) and bool((_bits(x16[n * h * w * 8:]) == SENTINEL).all())
        assert float(((cn.double().cpu() - c).abs() - c_tol).max()) <= 0.0, "c_noise"
    net = torch.zeros(n, h, w, 4)
    net[..., :3] = I["net"].permute(0, 2, 3, 1).float()
    net_d, den_out = net.to(DEV), torch.empty(n, 3, h, w, device=DEV)
    assert _lib().pmi_edm_stage_out(img.data_ptr(), net_d.data_ptr(), 4, sg.data_ptr(), sigma.numel(), 0.5, den_out.data_ptr(), n, h, w, _stream()) == 0
    worst = max(worst, _ratio(f"stage_out {case}", den_out, *M.edm_stage_out_ref(I["img"], I["net"], sigma)))
    e, s, c = sampler.edm_predict(img, dev(I["den"]), sg, eps=True, to_sigma=dev(to), previous=(dev(I["prev_img"]), dev(prev), dev(I["prev_eps"])))
    refs = M.edm_predict_ref(I["img"], I["den"], sigma, to, I["prev_img"], prev, I["prev_eps"])
    for tag, got, (ref, tol) in zip(("pmi_edm_predict eps", "pmi_edm_predict step", "pmi_edm_predict correction"), (e, s, c), refs):
        worst = max(worst, _ratio(f"{tag} {case}", got, ref, tol))
    got = sampler.edm_inject_noise(img, sg, dev(rev), dev(I["noise"]), M.S_NOISE)
    worst = max(worst, _ratio(f"pmi_edm_inject_noise {case}", got, *M.edm_inject_ref(I["img"], sigma, rev, I["noise"])))
    coeffs = [-0.19477120421163768, 0.016207442628014334, -0.0007523481336726187, 1.2655031463622994e-05]
    for order in (1, 4):
        got = sampler.edm_lms(img, coeffs[:order], [dev(t) for t in I["eps"][:order]])
        worst = max(worst, _ratio(f"pmi_edm_lms {order} {case}", got, *M.edm_lms_ref(I["img"], coeffs[:order], I["eps"][:order])))
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_adagn_gelu_layer(dtype):
    """one AdaGN + exact GELU as the engine launches it, a per-sample film row and the single row of a scalar sigma (film_ld = 0)"""
    from perceptor_amd._hip import ACT_GELU
    from perceptor_amd.engine import ops
    x, film = M.adagn_case(dtype)
    x16 = x.to(M.TD[dtype]).to(DEV)
    for f in (film, film[:1]):
        fd = f.float().to(DEV).contiguous()
        got = ops.group_norm(x16, None, None, x.shape[-1] // 32, DT_CODE[dtype], film=fd, film_ld=fd.stride(0) if fd.shape[0] > 1 else 0, act=ACT_GELU)
        assert _ratio(f"adagn + gelu {dtype} rows {f.shape[0]}", got, *M.adagn_ref(x, f, dtype)) <= 1.0


# ---- 3. engine on the fixture's networks ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fixture():
    return golden("monster_diffusion_reference")


@pytest.fixture(scope="module")
def emulated(fixture):
    """the emulated restatement's checkpoints, computed once per (network, dtype)"""
    cache = {}

    def get(net, dtype):
        if (net, dtype) not in cache:
            config, _ = M.NETS[net]
            rec = {}
            den = M.denoised64(M.synthetic_state_dict(config), fixture[f"{net}_in"].double(), fixture[f"{net}_sigma"], config, emulate=dtype, record=rec)
            rec["denoised_xs"] = den
            cache[(net, dtype)] = rec
        return cache[(net, dtype)]

    return get


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
@pytest.mark.parametrize("net", ["A", "B"])
def test_engine_checkpoints(net, dtype, fixture, emulated):
    from perceptor_amd.engine.monster import MonsterEngine
    config, shape = M.NETS[net]
    eng = MonsterEngine(config, M.synthetic_state_dict(config), DEV, dtype)
    sigma = fixture[f"{net}_sigma"].float().to(DEV)
    taps = {}
    den = eng.forward(fixture[f"{net}_in"].to(DEV), sigma, taps=taps)
    torch.cuda.synchronize()
    assert taps["cond"].shape[0] == sigma.numel()                    # a scalar sigma gives ONE row of conditioning
    cond, cond_tol = M.cond_ref(M.synthetic_state_dict(config), fixture[f"{net}_sigma"])
    assert _ratio(f"{net} {dtype} cond", taps["cond"], cond, cond_tol) <= 1.0
    assert M.rel_l2(cond.expand(shape[0], -1), fixture[f"{net}_cond"]) < 1e-14      # (the reference's cond has one row per sample, all alike here)
    emu = emulated(net, dtype)
    worst = 0.0
    for k in M.CHECKPOINTS + ("denoised_xs",):
        got = den if k == "denoised_xs" else taps[k][..., :3 if k == "proj_out" else None].permute(0, 3, 1, 2)
        g = gate(net, dtype, k)
        worst = max(worst, _rel(f"{net} {dtype} {k} vs emulation", got, emu[k], g) / g)
        ref = fixture[f"{net}_{k}"]
        worst = max(worst, _rel(f"{net} {dtype} {k} vs fixture", M.sampled(got.double().cpu().contiguous(), fixture, f"{net}_{k}"), ref, g) / g)
    assert worst <= 1.0


# ---- 4. product config -----------------------------------------------------------------------------------------------------------------------
def test_product_config():
    from perceptor_amd.engine.monster import MonsterEngine
    sd = M.synthetic_state_dict(M.PRODUCT)
    img, sigma = M.product_case()
    ref = M.denoised64(sd, img.double(), sigma.double(), M.PRODUCT)
    for dtype in ("bf16", "f16"):
        got = MonsterEngine(M.PRODUCT, sd, DEV, dtype).forward(img.to(DEV), sigma.to(DEV))
        g = 2 * EMU_PRODUCT[dtype]
        assert _rel(f"product {dtype}", got, ref, g) <= g


# ---- 5. public class ---------------------------------------------------------------------------------------------------------------------------
def _model(dtype="bf16", net="A"):
    from perceptor_amd.models import MonsterDiffusion
    return MonsterDiffusion(config=M.NETS[net][0], dtype=dtype).to(DEV)


@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_samplers_follow_recorded_trajectories(dtype, fixture):
    m = _model(dtype)
    x = fixture["A_x0"].to(DEV)
    noises = fixture["A_heun_noise"].float().to(DEV)
    n_steps, ys, k = 3, [], 0
    for a, b in m.schedule_ts(n_steps):
        r = m.reversed_ts(a, n_steps).clamp(max=80.0)
        xr = m.inject_noise(x, a, r, noise=noises[k]); k += 1
        p = m.predictions(xr, r)
        e = p.eps
        x = p.step(b)
        p = m.predictions(x, b)
        x = p.correction(xr, r, e)
        ys.append(p.denoised_images.clamp(0, 1))
    r = m.reversed_ts(b, n_steps)
    ys.append(m.predictions(m.inject_noise(x, b, r, noise=noises[k]), r).denoised_images.clamp(0, 1))
    worst = 0.0
    for i, (got, ref) in enumerate(zip(ys, fixture["A_heun"])):
        g = 2 * EMU_HEUN[dtype][i]
        worst = max(worst, _rel(f"heun yield {i} {dtype}", got, ref, g) / g)
    ys = list(m.linear_multistep_sample(2, n_evaluations=6, diffused_images=fixture["A_x0"].to(DEV)))
    assert len(ys) == 6
    for i, (got, ref) in enumerate(zip(ys, fixture["A_lms"])):
        g = 2 * EMU_LMS[dtype][i]
        worst = max(worst, _rel(f"lms yield {i} {dtype}", got, ref, g) / g)
    assert worst <= 1.0


def test_sample_is_the_manual_loop_bit_for_bit(fixture):
    m = _model()
    x0 = fixture["A_x0"].to(DEV)
    torch.manual_seed(7)
    ys = list(m.sample(2, n_evaluations=6, diffused_images=x0))
    assert len(ys) == 3
    torch.manual_seed(7)
    x, manual = x0, []
    for a, b in m.schedule_ts(3):
        r = m.reversed_ts(a, 3).clamp(max=80.0)
        xr = m.inject_noise(x, a, r, noise=torch.randn_like(x))
        p = m.predictions(xr, r)
        e, x = p.eps, p.step(b)
        p = m.predictions(x, b)
        x = p.correction(xr, r, e)
        manual.append(p.denoised_images.clamp(0, 1))
    r = m.reversed_ts(b, 3)
    manual.append(m.predictions(m.inject_noise(x, b, r, noise=torch.randn_like(x)), r).denoised_images.clamp(0, 1))
    for got, ref in zip(ys, manual):
        assert torch.equal(got, ref)
        assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0


def test_scalar_and_per_sample_ts_agree(fixture):
    m = _model()
    x = fixture["A_in"].to(DEV)
    a = m.predictions(x, torch.tensor(0.7, device=DEV))
    b = m.predictions(x, torch.full((2,), 0.7, device=DEV))
    c = m.predictions(x, 0.7)
    assert a.ts.shape == (1,) and b.ts.shape == (2,)
    assert torch.equal(a.denoised_xs, b.denoised_xs) and torch.equal(a.denoised_xs, c.denoised_xs)
    assert torch.equal(a.eps, b.eps) and torch.equal(a.step(torch.tensor(0.3)), b.step(torch.tensor([0.3, 0.3])))
    assert len(a) == 2 and a[1].t.ndim == 0 and len(list(a)) == 2
    with torch.enable_grad(), pytest.raises(NotImplementedError):
        m.predictions(x.clone().requires_grad_(True), 0.7)
    with pytest.raises(ValueError):
        m.predictions(x[:, :, :6], 0.7)                         # 6 x 12: the deepest map would be 1.5 rows


# ---- 6. capture --------------------------------------------------------------------------------------------------------------------------------
def test_graphed_evaluation_is_bit_equal_to_eager(fixture):
    from perceptor_amd.engine.graph import GraphedStep
    m = _model()
    x, sigma = fixture["A_in"].to(DEV), fixture["A_sigma"].float().to(DEV)
    eager = m.denoised_(x, sigma).clone()
    step = GraphedStep(lambda images, ts: m.denoised_(images, ts), x, sigma)
    got = step(x, sigma)
    torch.cuda.synchronize()
    assert torch.equal(got, eager)
