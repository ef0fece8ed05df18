"""GPU: pmi_rdb_conv3x3 (csrc/rrdb.hip) against the float64 reference and per-element bound of tests/_rrdb_ref64.py, engine/rrdb.py's
RrdbEngine against the emulated float64 restatement checkpoint by checkpoint, models / losses.SuperResolution against the reference's own
values (tests/golden/super_resolution_reference.npz), and the public classes' properties at the product configuration.

Every comparison prints its worst |got - ref| / bound (or rel-L2 / gate) before it asserts.  tests/test_super_resolution_cpu.py runs the
seeded defects at the engine test's inputs.  Measured figures: DESIGN.md section 21.
"""
import math

import pytest
import torch

import _rrdb_ref64 as R
from conftest import golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7B7B                      # a 16-bit pattern (about 6.1e4 in f16, 1.3e36 in bf16) no kernel under test produces
DT_CODE = {"f16": 0, "bf16": 1}
GRIDS = ((1, 8, 32), (2, 9, 33), (1, 5, 7), (3, 16, 40))           # exact tile; one past a tile both ways, two images; under a tile; many tiles
BLOCK_SHAPES = ((64, 32), (96, 32), (128, 32), (160, 32), (192, 64))
EPILOGUES = (dict(), dict(alpha=0.2, residuals=1), dict(alpha=0.2, beta=0.2, residuals=2))
# rel-L2 of the EMULATED float64 restatement (tests/_rrdb_ref64.py, emulate=dtype) against the fixture, measured on the CPU when this test
# was written; the tolerance is 2 x that (accumulation order).  Outputs of the three networks, then (loss value, gradient) of the two loss cases.
FIXTURE_TOL = {("x4", "bf16"): 2 * 6.745052e-3, ("x4", "f16"): 2 * 8.518228e-4, ("x2", "bf16"): 2 * 6.687972e-3, ("x2", "f16"): 2 * 8.715775e-4,
               ("x8", "bf16"): 2 * 5.436390e-3, ("x8", "f16"): 2 * 6.776026e-4}
FIXTURE_LOSS_TOL = {("same", "bf16"): (2 * 6.868309e-4, 2 * 7.816935e-3), ("same", "f16"): (2 * 6.066422e-5, 2 * 9.707886e-4),
                    ("resized", "bf16"): (2 * 9.895531e-4, 2 * 7.354146e-3), ("resized", "f16"): (2 * 2.753022e-5, 2 * 8.667840e-4)}


def _lib():
    from perceptor_amd import _hip
    return _hip.lib()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _filled(shape, dtype):
    return torch.full(shape, SENTINEL, dtype=torch.int16, device=DEV).view(R.TD[dtype])


def _bits(t):
    return t.contiguous().view(torch.int16)


def _launch(X, cin, wp, bias, D, *, r1=None, r2=None, alpha=1.0, beta=1.0, slope=1.0, up=False, dtype):
    """One pmi_rdb_conv3x3 call on views (pitch = stride of the pixel axis); returns the code."""
    n, h, w, nn_ = D.shape
    rc = _lib().pmi_rdb_conv3x3(_ptr(X), X.stride(-2), cin, _ptr(wp), _ptr(bias), nn_, _ptr(D), D.stride(-2), _ptr(r1),
                                r1.stride(-2) if r1 is not None else 0, _ptr(r2), r2.stride(-2) if r2 is not None else 0,
                                alpha, beta, slope, int(up), n, h, w, DT_CODE[dtype], torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc


def _pack(w, dtype):
    from perceptor_amd.engine.rrdb import pack_rdb_weights
    return pack_rdb_weights(w.float()).to(device=DEV, dtype=R.TD[dtype])


def _dense_case(grid, cin, n, seed, regime, dtype, *, alpha=1.0, beta=1.0, slope=1.0, residuals=0):
    """One call laid out as the engine lays it out: X = the prefix of a 192-pitch dense buffer pre-filled with the sentinel (plus a tail past
    the last pixel); cin < 192: D = the slice [cin, cin + n) of the SAME buffer; cin = 192: D = channels [0, n) of a second sentinel buffer,
    R1 = X's first n channels (aliasing X), R2 a tensor of its own.  Returns (got, y, tol, stray_ok)."""
    images, h, w = grid
    x, wt, bias, r1, r2 = R.kernel_operands(grid, cin, n, seed, regime, dtype, residuals=residuals)
    if residuals and cin == 192:
        r1 = x[..., :n]                                              # conv5's R1 is x itself
    y, tol = R.kernel_ref(x, wt, bias, dtype=dtype, slope=slope, alpha=alpha, beta=beta, r1=r1, r2=r2)
    td, tail = R.TD[dtype], 256
    npx = images * h * w
    buf = _filled((npx * 192 + tail,), dtype)
    dense = buf[:npx * 192].view(images, h, w, 192)
    dense[..., :cin] = x.to(td).to(DEV)
    same = cin < 192
    if same:
        obuf, out = buf, dense
        D = dense[..., cin:cin + n]
    else:
        obuf = _filled((npx * 192 + tail,), dtype)
        out = obuf[:npx * 192].view(images, h, w, 192)
        D = out[..., :n]
    before = _bits(obuf).clone()
    R1 = None if r1 is None else (dense[..., :n] if cin == 192 else r1.to(td).to(DEV))
    R2 = None if r2 is None else r2.to(td).to(DEV)
    rc = _launch(dense, cin, _pack(wt, dtype), bias.float().to(DEV), D, r1=R1, r2=R2, alpha=alpha, beta=beta, slope=slope, dtype=dtype)
    assert rc == 0, rc
    after = _bits(obuf)
    mask = torch.ones(npx * 192 + tail, dtype=torch.bool, device=DEV)
    lo = cin if same else 0
    mask[:npx * 192].view(images, h, w, 192)[..., lo:lo + n] = False
    stray_ok = bool((after[mask] == before[mask]).all())
    return D.clone(), y, tol, stray_ok


def _worst(tag, got, ref, bound):
    w = float(((got.double().cpu() - ref).abs() / bound).max())
    print(f"[bound] {tag}: worst |got - ref| / bound = {w:.3e}")
    return w


# ================================================ kernel ===================================================================================
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("regime", ("coherent", "mixed"))
@pytest.mark.parametrize("dtype", ("bf16", "f16"))
def test_rdb_conv_block_shapes(dtype, regime, grid):
    """Every (Cin, N) of the dense block in the dense-buffer layout: conv1-4 with LeakyReLU into their own slice of the buffer they read,
    conv5 with each epilogue (none; alpha, R1 = x aliasing X; alpha, R1, beta, R2).  Nothing outside D's slice changes."""
    worst, ok = 0.0, True
    for i, (cin, n) in enumerate(BLOCK_SHAPES):
        epis = EPILOGUES if cin == 192 else (dict(slope=0.2),)
        for j, epi in enumerate(epis):
            got, y, tol, stray_ok = _dense_case(grid, cin, n, 100 * i + 10 * j + grid[1], regime, dtype, **epi)
            worst = max(worst, _worst(f"rdb_conv {dtype} {regime} {grid} {cin}->{n} {epi}", got, y, tol))
            ok = ok and stray_ok
    assert ok, "bytes outside D's slice changed"
    assert worst <= 1.0


@pytest.mark.parametrize("regime", ("coherent", "mixed"))
@pytest.mark.parametrize("dtype", ("bf16", "f16"))
def test_rdb_conv_tail_shapes(dtype, regime):
    """64 -> 64 on contiguous tensors: the nearest-x2 read (up = 1) on (2, 10, 14) from (2, 5, 7) and on a multi-tile grid, LeakyReLU on
    every grid, and the three epilogues with residuals of their own."""
    td = R.TD[dtype]
    worst = 0.0
    cases = [((2, 10, 14), dict(up=True, slope=0.2)), ((1, 18, 66), dict(up=True, slope=0.2))]
    cases += [(g, dict(slope=0.2)) for g in GRIDS]
    cases += [((2, 9, 33), dict(alpha=e.get("alpha", 1.0), beta=e.get("beta", 1.0), residuals=e.get("residuals", 0))) for e in EPILOGUES]
    for i, (grid, kw) in enumerate(cases):
        up, res = kw.pop("up", False), kw.pop("residuals", 0)
        x, wt, bias, r1, r2 = R.kernel_operands(grid, 64, 64, 1000 + 7 * i, regime, dtype, up=up, residuals=res)
        y, tol = R.kernel_ref(x, wt, bias, dtype=dtype, r1=r1, r2=r2, up=up, **kw)
        D = _filled(tuple(y.shape), dtype)
        dev = lambda t: None if t is None else t.to(td).to(DEV)
        rc = _launch(dev(x), 64, _pack(wt, dtype), bias.float().to(DEV), D, r1=dev(r1), r2=dev(r2), up=up, dtype=dtype, **kw)
        assert rc == 0, rc
        worst = max(worst, _worst(f"rdb_conv {dtype} {regime} {grid} 64->64 up={int(up)} {kw} residuals={res}", D, y, tol))
    assert worst <= 1.0


@pytest.mark.parametrize("dtype", ("bf16", "f16"))
def test_rdb_conv_deterministic_and_batch_independent(dtype):
    td = R.TD[dtype]
    x, wt, bias, r1, r2 = R.kernel_operands((2, 9, 33), 192, 64, 77, "mixed", dtype, residuals=2)
    wp, b = _pack(wt, dtype), bias.float().to(DEV)
    dev = lambda t: t.to(td).to(DEV).contiguous()
    X, R1, R2 = dev(x), dev(r1), dev(r2)

    def run(sl):
        D = _filled((sl.stop - sl.start, 9, 33, 64), dtype)
        assert _launch(X[sl], 192, wp, b, D, r1=R1[sl], r2=R2[sl], alpha=0.2, beta=0.2, dtype=dtype) == 0
        return _bits(D)

    both, again = run(slice(0, 2)), run(slice(0, 2))
    assert torch.equal(both, again), "two runs differ"
    assert torch.equal(both[:1], run(slice(0, 1))) and torch.equal(both[1:], run(slice(1, 2))), "a sample depends on its batch"


def test_rdb_conv_argument_guards():
    """Shapes the kernel does not take: the host-only query answers 0, the call returns PMI_ERR_ARG, and nothing is written."""
    L = _lib()
    X = torch.zeros((1, 8, 8, 200), dtype=torch.float16, device=DEV)
    wp = torch.zeros(9 * 192 * 64, dtype=torch.float16, device=DEV)
    b = torch.zeros(64, device=DEV)
    D = _filled((1, 8, 8, 64), "f16")
    s = torch.cuda.current_stream().cuda_stream
    ok = dict(cin=64, n=64, ldx=200, ldd=64, ldr1=0, ldr2=0, up=0, images=1, h=8, w=8, dt=0)
    q = lambda **k: L.pmi_rdb_conv3x3_eligible(*[{**ok, **k}[f] for f in ("cin", "n", "ldx", "ldd", "ldr1", "ldr2", "up", "images", "h", "w", "dt")])

    def run(xp=None, **k):
        a = {**ok, **k}
        return L.pmi_rdb_conv3x3(_ptr(X) if xp is None else xp, a["ldx"], a["cin"], _ptr(wp), _ptr(b), a["n"], _ptr(D), a["ldd"], None, a["ldr1"],
                                 None, a["ldr2"], 1.0, 1.0, 1.0, a["up"], a["images"], a["h"], a["w"], a["dt"], s)

    assert q() == 1
    bad = (dict(cin=48), dict(cin=224), dict(cin=0), dict(n=48), dict(n=128), dict(dt=2), dict(ldx=196), dict(ldx=56), dict(ldd=60),
           dict(ldd=32), dict(up=1, h=7), dict(up=2), dict(h=0), dict(images=0))
    for k in bad:
        assert q(**k) == 0, k
        assert run(**k) == -1, k
    assert q(ldr1=60) == 0 and q(ldr2=12) == 0
    assert run(xp=_ptr(X) + 8) == -1                                   # a misaligned pointer
    assert L.pmi_rdb_conv3x3(_ptr(X), 200, 64, _ptr(wp), _ptr(b), 64, _ptr(D), 64, None, 0, None, 0, float("nan"), 1.0, 1.0, 0, 1, 8, 8, 0, s) == -1
    assert L.pmi_rdb_conv3x3(None, 200, 64, _ptr(wp), _ptr(b), 64, _ptr(D), 64, None, 0, None, 0, 1.0, 1.0, 1.0, 0, 1, 8, 8, 0, s) == -1
    torch.cuda.synchronize()
    assert bool((_bits(D) == SENTINEL).all()), "a refused call wrote"
    assert run() == 0
    torch.cuda.synchronize()
    assert not bool((_bits(D) == SENTINEL).any())


# ================================================ engine ===================================================================================
def _sd(blocks, scale):
    from perceptor_amd.engine.rrdb import rrdb_state_dict_shapes
    from perceptor_amd.utils.synth import synth_state_dict
    return synth_state_dict(rrdb_state_dict_shapes(blocks, scale), 0, gain=2 ** 0.5)


@pytest.fixture(scope="module")
def fx():
    return golden("super_resolution_reference")


@pytest.mark.parametrize("dtype", ("bf16", "f16"))
@pytest.mark.parametrize("name", ("x4", "x2", "x8"))
def test_engine_checkpoints_vs_emulated_float64(fx, name, dtype):
    """At the fixture's inputs: every checkpoint within rel-L2 sqrt(R) u of the emulated float64 restatement, R = the 16-bit roundings on
    the longest path to it (_rrdb_ref64.roundings)."""
    from perceptor_amd.engine.rrdb import RrdbEngine
    scale, blocks = (int(v) for v in fx[f"{name}_cfg"])
    sd = _sd(blocks, scale)
    x = fx[f"{name}_in"]
    ref_rec, rec = {}, {}
    ref = R.upsample64({k: v.double() for k, v in sd.items()}, x, scale, blocks, emulate=dtype, record=ref_rec)
    eng = RrdbEngine((64, 32, blocks, scale), sd, DEV, dtype)
    out = eng.upsample(x.to(DEV), record=rec)
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(ref.shape) and out.dtype is torch.float32
    assert list(rec) == list(ref_rec)
    rounds, u, worst = R.roundings(scale, blocks), R.U[dtype], 0.0
    for k in list(rec) + ["out"]:
        got, want = (out, ref) if k == "out" else (rec[k], ref_rec[k])
        rel, gate = R.rel_l2(got.cpu(), want), math.sqrt(rounds[k]) * u
        print(f"[bound] rrdb engine {name} {dtype} {k}: rel-L2 {rel:.3e}, gate sqrt({rounds[k]}) u = {gate:.3e}, ratio {rel / gate:.3f}")
        worst = max(worst, rel / gate)
    assert worst <= 1.0


# ================================================ public classes vs the reference ============================================================
@pytest.mark.parametrize("dtype", ("bf16", "f16"))
@pytest.mark.parametrize("name", ("x4", "x2", "x8"))
def test_models_super_resolution_vs_reference(fx, name, dtype):
    from perceptor_amd import models
    scale, blocks = (int(v) for v in fx[f"{name}_cfg"])
    x, ref = fx[f"{name}_in"], fx[f"{name}_out"]
    m = models.SuperResolution(name, num_block=blocks, dtype=dtype).to(DEV)
    y = m(x.to(DEV))
    assert m.scale == scale and y.dtype is torch.float32
    assert tuple(y.shape) == (x.shape[0], 3, x.shape[2] * scale, x.shape[3] * scale)          # odd sizes at scale 2: padded, then cropped
    rel, tol = R.rel_l2(y.cpu(), ref), FIXTURE_TOL[(name, dtype)]
    print(f"[bound] models.SuperResolution {name} {dtype}: rel-L2 vs reference {rel:.3e}, tolerance {tol:.3e}, ratio {rel / tol:.3f}")
    assert rel <= tol
    with pytest.raises(NotImplementedError):
        m(x.to(DEV).requires_grad_(True))
    with torch.no_grad():
        assert torch.equal(m(x.to(DEV).requires_grad_(True)), y)


@pytest.mark.parametrize("dtype", ("bf16", "f16"))
@pytest.mark.parametrize("case", ("same", "resized"))
def test_losses_super_resolution_vs_reference(fx, case, dtype):
    from perceptor_amd import losses
    x = fx[f"loss_{case}_in"].to(DEV)
    ref, ref_grad = float(fx[f"loss_{case}_value"]), fx[f"loss_{case}_grad"]
    loss = losses.SuperResolution("x2", num_block=1, dtype=dtype).to(DEV)
    val, grad = loss.loss_and_grad(x)
    tol_v, tol_g = FIXTURE_LOSS_TOL[(case, dtype)]
    rel_v, rel_g = abs(float(val) - ref) / abs(ref), R.rel_l2(grad.cpu(), ref_grad)
    print(f"[bound] losses.SuperResolution {case} {dtype}: loss {float(val):.6f} vs reference {ref:.6f}: rel {rel_v:.3e} / tol {tol_v:.3e} = "
          f"{rel_v / tol_v:.3f}; gradient rel-L2 {rel_g:.3e} / tol {tol_g:.3e} = {rel_g / tol_g:.3f}")
    assert rel_v <= tol_v and rel_g <= tol_g
    xg = x.clone().requires_grad_(True)
    out = loss(xg)
    out.backward()
    assert float(out.detach()) == float(val) and torch.equal(xg.grad, grad)
    half, _ = loss.loss_and_grad(x, n_total=2 * x.shape[0])
    assert abs(float(half) - 0.5 * float(val)) <= 1e-6 * float(val)


# ================================================ product configuration ========================================================================
def test_product_config_properties():
    """ "x4", 23 blocks, 1 x 3 x 64 x 64 -> 256 x 256 (synthetic gain sqrt(2)): finite, deterministic, batch-independent; the shapes of
    downsample / decode; the autograd path of the default loss ("x2", 23 blocks) equals the fused one."""
    from perceptor_amd import losses, models, transforms
    g = torch.Generator().manual_seed(5)
    x = torch.rand((2, 3, 64, 64), generator=g).to(DEV)
    t = transforms.SuperResolution("x4").to(DEV)
    m = t.model
    assert isinstance(m, models.SuperResolution) and (m.num_block, m.scale) == (23, 4)
    y = m(x)
    assert tuple(y.shape) == (2, 3, 256, 256) and bool(torch.isfinite(y).all())
    assert torch.equal(y, m(x)), "two runs differ"
    assert torch.equal(y[:1], m(x[:1])) and torch.equal(y[1:], m(x[1:])), "a sample depends on its batch"
    assert torch.equal(t.encode(x[:1]), y[:1])
    d = m.downsample(y)
    assert tuple(d.shape) == (2, 3, 64, 64) and bool(torch.isfinite(d).all())
    assert tuple(m.downsample(y, size=(48, 40)).shape) == (2, 3, 48, 40)
    ref = torch.nn.functional.interpolate(y.cpu().double(), size=(64, 64), mode="bilinear", align_corners=False)
    assert float((d.cpu().double() - ref).abs().max()) <= 8 * 2.0 ** -24 * float(y.abs().max())       # fp32 taps and two fp32 passes
    assert tuple(t.decode(y).shape) == (2, 3, 64, 64) and tuple(t.decode(y, size=32).shape) == (2, 3, 32, 32)
    del t, m
    loss = losses.SuperResolution().to(DEV)
    assert (loss.transform.model.num_block, loss.pre_downscale) == (23, 2)
    xg = x[:1].clone().requires_grad_(True)
    out = loss(xg)
    out.backward()
    val, grad = loss.loss_and_grad(x[:1])
    assert bool(torch.isfinite(out)) and float(out.detach()) == float(val) and torch.equal(xg.grad, grad)
