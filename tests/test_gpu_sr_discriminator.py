"""GPU: csrc/disc.hip's kernels (pmi_convt4x4s2, pmi_lrelu_bwd, pmi_lrelu_add, pmi_mean_f32) against the float64 references and per-element
bounds of tests/_disc_ref64.py, engine/disc.py's DiscriminatorEngine against the emulated float64 restatement tensor by tensor with the
LeakyReLU signs pinned by ``record``, and SuperResolutionDiscriminator (losses/super_resolution_discriminator.py) against the reference's own values
(tests/golden/sr_discriminator_reference.npz).

Every comparison prints its worst |got - ref| / bound (or rel-L2 / gate) before it asserts.  tests/test_sr_discriminator_cpu.py runs the
seeded defects at the engine test's inputs.  Measured figures: DESIGN.md section 23.

Mask operand Y of the kernel tests: the "mixed" regime has |y| >= 2^-7, so no value lies below the rounding unit and the share excluded from
the mask comparison is 0 (checked on the CPU by test_sr_discriminator_cpu.py::test_kernel_mask_operand_has_no_ambiguous_sign).

FIXTURE_TOL: rel-L2 (loss: relative error) of the EMULATED float64 restatement (emulate=dtype, own signs, the engine's gradient scale)
against the fixture, measured on the CPU when this test was written (test_sr_discriminator_cpu.py::test_emulated_restatement_vs_fixture
prints them); the tolerance is 2 x that.  The gradient's figure is dominated by LeakyReLU signs that a 16-bit rounding flips.
"""
import math

import pytest
import torch

import _disc_ref64 as R
from conftest import golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7B7B                      # a 16-bit pattern (about 6.1e4 in f16, 1.3e36 in bf16) no kernel under test produces
DT_CODE = {"f16": 0, "bf16": 1}
GRIDS = ((1, 1, 1), (2, 2, 3), (1, 5, 7), (3, 8, 33))              # one pixel; under a tile, two images; odd sizes; one past a tile, three images
PAIRS = ((64, 32), (128, 64), (256, 128), (512, 256))             # Cout -> Cin; the last only on the two smallest grids
EPILOGUES = (dict(), dict(r=True), dict(y=True), dict(r=True, y=True), dict(r=True, y=True, out_f32=True))
# (logits, loss, gradient) per fixture case and dtype
FIXTURE_TOL = {
    ("f64", "bf16"): (2 * 3.020335e-03, 2 * 7.284474e-04, 2 * 5.026927e-02), ("f64", "f16"): (2 * 4.254059e-04, 2 * 2.183089e-04, 2 * 2.172860e-02),
    ("f32", "bf16"): (2 * 4.055935e-03, 2 * 6.817556e-04, 2 * 5.601038e-02), ("f32", "f16"): (2 * 5.514093e-04, 2 * 3.281919e-04, 2 * 5.767819e-03),
    ("f64_shard", "bf16"): (2 * 3.020335e-03, 2 * 7.284474e-04, 2 * 5.018812e-02), ("f64_shard", "f16"): (2 * 4.254059e-04, 2 * 2.183089e-04, 2 * 2.173875e-02),
}


def _lib():
    from perceptor_amd import _hip
    return _hip.lib()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _filled(n, dtype):
    return torch.full((n,), SENTINEL, dtype=torch.int16, device=DEV).view(R.TD[dtype])


def _bits(t):
    return t.contiguous().view(torch.int16)


def _pack(w, dtype):
    from perceptor_amd.engine.disc import pack_convt_weights
    return pack_convt_weights(w.float()).to(device=DEV, dtype=R.TD[dtype])


def _dev(t, dtype):
    return None if t is None else t.to(R.TD[dtype]).to(DEV).contiguous()


def _convt(G, wp, cin, D, ldd, *, r=None, y=None, slope=0.2, out_f32=False, dtype):
    n, h, w, cout = G.shape
    rc = _lib().pmi_convt4x4s2(_ptr(G), G.stride(-2), cout, _ptr(wp), cin, _ptr(D), ldd, _ptr(r), r.stride(-2) if r is not None else 0,
                               _ptr(y), y.stride(-2) if y is not None else 0, slope, int(out_f32), n, h, w, DT_CODE[dtype], _stream())
    torch.cuda.synchronize()
    return rc


def _convt_case(grid, cout, cin, seed, regime, dtype, *, r=False, y=False, out_f32=False, slope=0.2):
    """One call into a D whose pitch is cin + 8 with a tail past the last pixel, both pre-filled with the sentinel.
    Returns (worst |got - ref| / bound, whether every byte outside D's channels is unchanged)."""
    images, h, w = grid
    g, wt, rr, yy = R.convt_operands(grid, cout, cin, seed, regime, dtype, with_r=r, with_y=y)
    ref, tol = R.convt_ref(g, wt, rr, yy, slope=slope, dtype=dtype, out_f32=out_f32)
    npx, ldd, tail = images * 4 * h * w, cin + 8, 64
    if out_f32:
        buf = torch.full((npx * ldd + tail,), 0x7B7B7B7B, dtype=torch.int32, device=DEV).view(torch.float32)
        raw = lambda: buf.view(torch.int32)
    else:
        buf = _filled(npx * ldd + tail, dtype)
        raw = lambda: buf.view(torch.int16)
    before = raw().clone()
    rc = _convt(_dev(g, dtype), _pack(wt, dtype), cin, buf, ldd, r=_dev(rr, dtype), y=_dev(yy, dtype), slope=slope, out_f32=out_f32, dtype=dtype)
    assert rc == 0, rc
    D = buf[:npx * ldd].view(images, 2 * h, 2 * w, ldd)
    keep = torch.ones(npx * ldd + tail, dtype=torch.bool, device=DEV)
    keep[:npx * ldd].view(images, 2 * h, 2 * w, ldd)[..., :cin] = False
    stray_ok = bool((raw()[keep] == before[keep]).all())
    return R.margin(D[..., :cin].cpu(), ref, tol), stray_ok


# ================================================ pmi_convt4x4s2 ===============================================================================
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("dtype", ("bf16", "f16"))
def test_convt4x4s2_vs_float64(dtype, grid):
    """Every channel pair and epilogue on one grid; regimes alternate.  Nothing outside D's Cin channels changes."""
    worst, ok = 0.0, True
    for i, (cout, cin) in enumerate(PAIRS):
        if cout == 512 and grid not in GRIDS[:2]:
            continue
        for j, epi in enumerate(EPILOGUES):
            regime = ("coherent", "mixed")[(i + j) % 2]
            m, stray_ok = _convt_case(grid, cout, cin, 1000 * i + 10 * j + grid[2], regime, dtype, **epi)
            print(f"[bound] convt4x4s2 {dtype} {regime} {grid} {cout}->{cin} {epi}: worst |got - ref| / bound = {m:.3e}")
            worst, ok = max(worst, m), ok and stray_ok
    assert ok, "bytes outside D's channels changed"
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", ("bf16", "f16"))
def test_convt4x4s2_deterministic_and_batch_independent(dtype):
    g, wt, rr, yy = R.convt_operands((3, 8, 33), 128, 64, 5, "mixed", dtype, with_r=True, with_y=True)
    G, Rr, Y, wp = _dev(g, dtype), _dev(rr, dtype), _dev(yy, dtype), _pack(wt, dtype)

    def run(sl):
        n = sl.stop - sl.start
        D = _filled(n * 16 * 66 * 64, dtype)
        assert _convt(G[sl], wp, 64, D, 64, r=Rr[sl], y=Y[sl], dtype=dtype) == 0
        return _bits(D).view(n, -1)

    both, again = run(slice(0, 3)), run(slice(0, 3))
    assert torch.equal(both, again), "two runs differ"
    for i in range(3):
        assert torch.equal(both[i:i + 1], run(slice(i, i + 1))), "a sample depends on its batch"


def test_convt4x4s2_argument_guards():
    """Shapes the kernel does not take: the host-only query answers 0, the call returns PMI_ERR_ARG, and nothing is written."""
    L = _lib()
    G = torch.zeros((1, 4, 4, 64), dtype=torch.float16, device=DEV)
    wp = torch.zeros(16 * 64 * 32, dtype=torch.float16, device=DEV)
    Y = torch.zeros((1, 8, 8, 32), dtype=torch.float16, device=DEV)
    D = _filled(8 * 8 * 32, "f16")
    ok = dict(cout=64, cin=32, ldg=64, ldd=32, ldr=0, ldy=0, images=1, h=4, w=4, dt=0)
    q = lambda **k: L.pmi_convt4x4s2_eligible(*[{**ok, **k}[f] for f in ("cout", "cin", "ldg", "ldd", "ldr", "ldy", "images", "h", "w", "dt")])

    def run(gp=None, slope=0.2, out_f32=0, yp=None, **k):
        a = {**ok, **k}
        return L.pmi_convt4x4s2(_ptr(G) if gp is None else gp, a["ldg"], a["cout"], _ptr(wp), a["cin"], _ptr(D), a["ldd"], None, a["ldr"], yp,
                                a["ldy"], slope, out_f32, a["images"], a["h"], a["w"], a["dt"], _stream())

    assert q() == 1
    bad = (dict(cout=48), dict(cout=0), dict(cout=544), dict(cin=16), dict(cin=48), dict(cin=0), dict(dt=2), dict(ldg=60), dict(ldg=32),
           dict(ldd=36), dict(ldd=24), dict(h=0), dict(w=0), dict(images=0))
    for k in bad:
        assert q(**k) == 0, k
        assert run(**k) == -1, k
    assert q(ldr=36) == 0 and q(ldy=12) == 0 and q(ldr=16) == 0
    assert run(gp=_ptr(G) + 8) == -1                                   # a misaligned pointer
    assert run(gp=0) == -1                                             # NULL
    assert run(yp=_ptr(Y) + 2, ldy=32) == -1                           # a misaligned optional operand
    assert run(yp=_ptr(Y), ldy=24) == -1                               # Y present with a pitch under Cin
    assert run(slope=float("nan")) == -1 and run(slope=float("inf")) == -1
    assert run(out_f32=2) == -1
    torch.cuda.synchronize()
    assert bool((_bits(D) == SENTINEL).all()), "a refused call wrote"
    assert run() == 0
    torch.cuda.synchronize()
    assert not bool((_bits(D) == SENTINEL).any())


# ================================================ elementwise and mean kernels =================================================================
@pytest.mark.parametrize("n", (1 * 3 * 5 * 40, 1003))
@pytest.mark.parametrize("dtype", ("bf16", "f16"))
def test_lrelu_kernels_vs_float64(dtype, n):
    L, worst = _lib(), 0.0
    g, g2, y, r = (R.operand((n,), 20 + i, "mixed", dtype) for i in range(4))
    G, G2, Y, Rr = (_dev(t, dtype) for t in (g, g2, y, r))
    for has2 in (False, True):
        out = _filled(n + 8, dtype)
        assert L.pmi_lrelu_bwd(_ptr(G), _ptr(G2) if has2 else None, _ptr(Y), _ptr(out), n, 0.2,
                               DT_CODE[dtype], _stream()) == 0
        torch.cuda.synchronize()
        ref, tol = R.lrelu_bwd_ref(g, g2 if has2 else None, y, 0.2, dtype)
        m = float(((out[:n].double().cpu() - ref).abs() / tol).max())
        print(f"[bound] lrelu_bwd {dtype} n={n} g2={has2}: worst |got - ref| / bound = {m:.3e}")
        worst = max(worst, m)
        assert bool((_bits(out[n:]) == SENTINEL).all()), "pmi_lrelu_bwd wrote past n"
        out = _filled(n + 8, dtype)
        assert L.pmi_lrelu_add(_ptr(G), _ptr(Rr) if has2 else None, _ptr(out), n, 0.2, DT_CODE[dtype], _stream()) == 0
        torch.cuda.synchronize()
        ref, tol = R.lrelu_add_ref(g, r if has2 else None, 0.2, dtype)
        m = float(((out[:n].double().cpu() - ref).abs() / tol).max())
        print(f"[bound] lrelu_add {dtype} n={n} r={has2}: worst |got - ref| / bound = {m:.3e}")
        worst = max(worst, m)
        assert bool((_bits(out[n:]) == SENTINEL).all()), "pmi_lrelu_add wrote past n"
    assert worst <= 1.0
    # refusals: NULL, misaligned, n = 0, a non-finite slope
    out = _filled(16, dtype)
    a = G
    assert L.pmi_lrelu_bwd(None, None, _ptr(a), _ptr(out), 8, 0.2, DT_CODE[dtype], _stream()) == -1
    assert L.pmi_lrelu_bwd(_ptr(a) + 2, None, _ptr(a), _ptr(out), 8, 0.2, DT_CODE[dtype], _stream()) == -1
    assert L.pmi_lrelu_add(_ptr(a), None, _ptr(out), 0, 0.2, DT_CODE[dtype], _stream()) == -1
    assert L.pmi_lrelu_add(_ptr(a), None, _ptr(out), 8, float("nan"), DT_CODE[dtype], _stream()) == -1
    assert L.pmi_lrelu_add(_ptr(a), None, _ptr(out), 8, 0.2, 2, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((_bits(out) == SENTINEL).all()), "a refused call wrote"


@pytest.mark.parametrize("n", (1 * 1 * 5 * 40, 1003, 70001))
def test_mean_f32_vs_float64(n):
    L = _lib()
    x = (R.operand((n,), 31, "mixed", "bf16") + 0.25).float()
    xd, partial, out = x.to(DEV), torch.empty(256, device=DEV), torch.full((2,), 7.0, device=DEV)
    scale = -0.001 / n
    assert L.pmi_mean_f32(_ptr(xd), _ptr(partial), _ptr(out), n, scale, _stream()) == 0
    torch.cuda.synchronize()
    ref, tol = R.mean_ref(x, scale)
    m = abs(float(out[0]) - float(ref)) / float(tol + 2.0 ** -24 * abs(ref))        # + the fp32 rounding of the scale itself
    print(f"[bound] mean_f32 n={n}: got {float(out[0]):.9e} ref {float(ref):.9e}, |got - ref| / bound = {m:.3e}")
    assert m <= 1.0 and float(out[1]) == 7.0
    again = torch.empty(1, device=DEV)
    assert L.pmi_mean_f32(_ptr(xd), _ptr(partial), _ptr(again), n, scale, _stream()) == 0
    torch.cuda.synchronize()
    assert float(again[0]) == float(out[0]), "two runs differ"
    assert L.pmi_mean_f32(None, _ptr(partial), _ptr(out), n, scale, _stream()) == -1
    assert L.pmi_mean_f32(_ptr(xd), _ptr(partial), _ptr(out), 0, scale, _stream()) == -1


# ================================================ engine ===================================================================================
def _sd(feat):
    from perceptor_amd.engine.disc import synth_disc_state_dict
    return synth_disc_state_dict(feat, 0)


@pytest.mark.parametrize("dtype", ("bf16", "f16"))
@pytest.mark.parametrize("feat,shape", R.ENGINE_CASES)
def test_engine_vs_emulated_float64(feat, shape, dtype):
    """Every stored activation and backward tensor, the logits, the loss and the image gradient within rel-L2 sqrt(R) u of the emulated
    float64 restatement whose LeakyReLU signs are the engine's own (record); R = the 16-bit roundings on the longest path to the tensor
    (_disc_ref64.TAPE_ROUNDINGS / GRAD_ROUNDINGS / ROUNDINGS)."""
    from perceptor_amd.engine.disc import DiscriminatorEngine
    sd, x = _sd(feat), R.engine_inputs(shape)
    eng = DiscriminatorEngine(feat, sd, DEV, dtype)
    rec = {}
    loss, grad = eng.loss_and_grad(x.to(DEV), record=rec)
    torch.cuda.synchronize()
    assert grad.dtype is torch.float32 and tuple(grad.shape) == tuple(shape) and loss.dtype is torch.float32
    count = shape[0] * shape[2] * shape[3]
    assert rec["gscale"] == R.grad_scale(dtype, count)
    ref_rec = {}
    logits, ref_loss, ref_grad = R.net64(sd, x, emulate=dtype, fused=R.fused_layers(feat), signs={k: v for k, v in rec.items() if k in R.TAPE_ROUNDINGS},
                                         gscale=rec["gscale"], record=ref_rec)
    u, worst = R.U[dtype], 0.0
    checks = [(k, rec[k], ref_rec[k], n) for k, n in {**R.TAPE_ROUNDINGS, **R.GRAD_ROUNDINGS}.items()]
    checks += [("logits", rec["logits"], logits, R.ROUNDINGS["logits"]), ("grad", grad, ref_grad, R.ROUNDINGS["grad"])]
    for k, got, want, n in checks:
        rel, gate = R.rel_l2(got.cpu(), want), math.sqrt(n) * u
        print(f"[bound] disc engine F={feat} {shape} {dtype} {k}: rel-L2 {rel:.3e}, gate sqrt({n}) u = {gate:.3e}, ratio {rel / gate:.3f}")
        worst = max(worst, rel / gate)
    rel, gate = abs(float(loss) - float(ref_loss)) / abs(float(ref_loss)), math.sqrt(R.ROUNDINGS["logits"]) * u
    print(f"[bound] disc engine F={feat} {shape} {dtype} loss: {float(loss):.6e} vs {float(ref_loss):.6e}: rel {rel:.3e}, gate {gate:.3e}, ratio {rel / gate:.3f}")
    assert max(worst, rel / gate) <= 1.0


# ================================================ public class vs the reference ================================================================
@pytest.fixture(scope="module")
def fx():
    return golden("sr_discriminator_reference")


@pytest.mark.parametrize("dtype", ("bf16", "f16"))
@pytest.mark.parametrize("case", ("f64", "f32", "f64_shard"))
def test_losses_discriminator_vs_reference(fx, case, dtype):
    from perceptor_amd.losses.super_resolution_discriminator import SuperResolutionDiscriminator
    feat, n_total = int(fx[f"{case}_num_feat"]), int(fx[f"{case}_n_total"]) or None
    x = fx[f"{case}_in"].to(DEV)
    loss = SuperResolutionDiscriminator(num_feat=feat, dtype=dtype, seed=int(fx[f"{case}_seed"])).to(DEV)
    sd = loss.model.state_dict()
    for k in range(1, 9):                                                # the power iteration reproduces the fixture's u, v
        assert torch.equal(sd[f"conv{k}.weight_u"].cpu(), fx[f"{case}_conv{k}_u"]) and torch.equal(sd[f"conv{k}.weight_v"].cpu(), fx[f"{case}_conv{k}_v"])
    logits = loss.logits(x)
    val, grad = loss.loss_and_grad(x, n_total=n_total)
    assert logits.dtype is torch.float32 and tuple(logits.shape) == (x.shape[0], 1, x.shape[2], x.shape[3])
    tol_l, tol_v, tol_g = FIXTURE_TOL[(case, dtype)]
    ref_v = float(fx[f"{case}_loss"])
    rel_l, rel_v, rel_g = R.rel_l2(logits.cpu(), fx[f"{case}_logits"]), abs(float(val) - ref_v) / abs(ref_v), R.rel_l2(grad.cpu(), fx[f"{case}_grad"])
    print(f"[bound] SuperResolutionDiscriminator {case} {dtype}: logits rel-L2 {rel_l:.3e} / tol {tol_l:.3e} = {rel_l / tol_l:.3f}; loss "
          f"{float(val):.6e} vs {ref_v:.6e}: rel {rel_v:.3e} / tol {tol_v:.3e} = {rel_v / tol_v:.3f}; gradient rel-L2 {rel_g:.3e} / tol {tol_g:.3e} = "
          f"{rel_g / tol_g:.3f}")
    assert rel_l <= tol_l and rel_v <= tol_v and rel_g <= tol_g


def test_losses_discriminator_properties():
    """forward().backward() equals loss_and_grad; n_total scales loss and gradient by N / n_total exactly (a power of two here); the engine is
    rebuilt after load_state_dict; two runs are bit-equal."""
    from perceptor_amd.engine.disc import synth_disc_state_dict
    from perceptor_amd.losses.super_resolution_discriminator import SuperResolutionDiscriminator
    x = R.engine_inputs((2, 3, 16, 24)).to(DEV)
    loss = SuperResolutionDiscriminator(num_feat=32, dtype="bf16").to(DEV)
    val, grad = loss.loss_and_grad(x)
    xg = x.clone().requires_grad_(True)
    out = loss(xg)
    out.backward()
    assert out.dim() == 0 and float(out.detach()) == float(val) and torch.equal(xg.grad, grad)
    val2, grad2 = loss.loss_and_grad(x)
    assert float(val2) == float(val) and torch.equal(grad2, grad), "two runs differ"
    half, ghalf = loss.loss_and_grad(x, n_total=2 * x.shape[0])
    assert float(half) == 0.5 * float(val) and torch.equal(ghalf, 0.5 * grad)
    eng = loss._engine
    assert eng is not None
    loss.model.load_state_dict(synth_disc_state_dict(32, 1))
    assert loss._engine is None
    val3, _ = loss.loss_and_grad(x)
    assert loss._engine is not eng and float(val3) != float(val)
    with pytest.raises(ValueError, match="multiples of 8"):
        loss.loss_and_grad(torch.zeros((1, 3, 12, 20), device=DEV))
    with pytest.raises(RuntimeError):
        loss.loss_and_grad(torch.zeros((1, 3, 16, 16)))
