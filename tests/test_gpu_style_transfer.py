"""GPU: the kernels of csrc/vgg.hip (pmi_maxpool2, pmi_maxpool2_bwd, pmi_gram, pmi_style_level, pmi_gram_bwd) against the float64
restatements and bounds of tests/_vgg_ref64.py, engine/vgg.py's VggEngine against the emulated float64 tower (features, loss, and the
image gradient with the engine's own ReLU masks, pool routes and signs pinned), losses.StyleTransfer against the reference's own values
(tests/golden/style_transfer_reference.npz), and the public classes' properties at the product configuration.

Every comparison prints its worst |got - ref| / bound before it asserts.  The inputs are tests/_vgg_ref64.py's seeded generators:
tests/test_style_transfer_cpu.py runs the sign-band condition and the seeded defects at exactly these inputs.

Measured on an MI355X (gradient rel-L2 against the pinned float64 tower, gate sqrt(12) u): see DESIGN.md section 19.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _vgg_ref64 as R
from conftest import golden

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7B7B                      # a 16-bit pattern (about 6.1e4 in f16, 1.3e36 in bf16) no kernel under test produces
DT_CODE = {"f16": 0, "bf16": 1}
# |loss - fixture| of the EMULATED float64 restatement (tests/_vgg_ref64.py, emulate=dtype), measured on the CPU when this test was
# written, times 2 for the accumulation order: same-size case bf16 4.1109e-4, f16 6.8925e-5; resized case bf16 3.4621e-4, f16 4.6339e-5
FIXTURE_LOSS_TOL = {("same", "bf16"): 2 * 4.1109e-4, ("same", "f16"): 2 * 6.8925e-5,
                    ("resized", "bf16"): 2 * 3.4621e-4, ("resized", "f16"): 2 * 4.6339e-5}


def _lib():
    from perceptor_amd import _hip
    return _hip.lib()


def _call(name, *args):
    from perceptor_amd._hip import call
    call(name, *args)
    torch.cuda.synchronize()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _worst(tag, got, ref, bound):
    w = float(((got.double() - ref.double()).abs() / bound).max())
    print(f"[bound] {tag}: worst |got - ref| / bound = {w:.3e}")
    return w


def _padded(shape, dtype, extra):
    """A buffer of prod(shape) + extra elements filled with the sentinel; (the whole buffer, its leading part viewed as shape)."""
    n = math.prod(shape)
    buf = torch.full((n + extra,), SENTINEL, dtype=torch.int16, device=DEV).view(dtype)
    return buf, buf[:n].view(shape)


def _tail_intact(buf, n):
    return bool((buf[n:].view(torch.int16) == SENTINEL).all())


# ================================================ max pool =================================================================================
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", R.POOL_SHAPES)
def test_maxpool2_forward_and_adjoint_bit_exact(shape, dtype):
    dt = R.DTYPES[dtype]
    n, h, w, c = shape
    x, dy = R.pool_inputs(shape, dt)
    xn = x.permute(0, 3, 1, 2).float()
    win = xn.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, -1, 4)
    assert bool((win.amax(-1) == 0).any()), "no all-zero window in the inputs"
    assert bool(((win == win.amax(-1, keepdim=True)).sum(-1) > 1)[win.amax(-1) > 0].any()), "no non-zero tie in the inputs"
    xd, dyd = x.to(DEV), dy.to(DEV)
    ybuf, y = _padded((n, h // 2, w // 2, c), dt, 2 * c)
    _call("pmi_maxpool2", _ptr(xd), _ptr(y), n, h, w, c, DT_CODE[dtype])
    want = F.max_pool2d(xn, 2, 2).permute(0, 2, 3, 1).to(dt)
    assert torch.equal(y.cpu().view(torch.int16), want.contiguous().view(torch.int16)), "pmi_maxpool2 differs from F.max_pool2d"
    assert _tail_intact(ybuf, y.numel())
    dbuf, dx = _padded(shape, dt, 2 * c)
    _call("pmi_maxpool2_bwd", _ptr(dyd), _ptr(xd), _ptr(dx), n, h, w, c, DT_CODE[dtype])
    xg = xn.clone().requires_grad_(True)                           # torch's CPU adjoint: the first maximum of a window takes dy
    F.max_pool2d(xg, 2, 2).backward(dy.permute(0, 3, 1, 2).float())
    adj = torch.where(xn > 0, xg.grad, torch.zeros_like(xn))
    assert torch.equal(adj, R.pool_adjoint(dy.permute(0, 3, 1, 2).float(), xn)), "the restatement's route differs from torch's"
    want = adj.permute(0, 2, 3, 1).to(dt).contiguous()
    assert torch.equal(dx.cpu().view(torch.int16), want.view(torch.int16)), "pmi_maxpool2_bwd differs from torch's adjoint * (x > 0)"
    assert _tail_intact(dbuf, dx.numel())


# ================================================ Gram =====================================================================================
def _gram_run(f, dtype):
    n, hw, c = f.shape
    r = n * c
    nws = _lib().pmi_gram_workspace(n, hw, c)
    assert nws > 0
    ws = torch.full((nws,), float("nan"), device=DEV)
    gbuf = torch.full((r * r + 2 * r,), float("nan"), device=DEV)
    G = gbuf[:r * r].view(r, r)
    _call("pmi_gram", _ptr(f), _ptr(G), _ptr(ws), n, hw, c, 1.0 / (float(r) * hw), DT_CODE[dtype])
    assert bool(torch.isnan(gbuf[r * r:]).all()), "rows past the Gram matrix were written"
    return G


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", R.GRAM_SHAPES)
def test_gram_vs_float64(shape, dtype):
    n, hw, c = shape
    fa, _ = R.gram_inputs(shape, R.DTYPES[dtype])
    fd = fa.to(DEV)
    G = _gram_run(fd, dtype)
    G2 = _gram_run(fd, dtype)
    assert torch.equal(G, G2), "two runs differ"
    assert torch.equal(G, G.t()), "G is not exactly symmetric"
    ref = R.gram(R.nchw(fa, n, hw, c))
    bound = R.gram_bound(fa, 1.0 / (float(n * c) * hw))
    assert _worst(f"pmi_gram {shape} {dtype}", G.cpu(), ref, bound) <= 1.0


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", R.GRAM_SHAPES)
def test_style_level_vs_float64(shape, dtype):
    n, hw, c = shape
    r = n * c
    dt = R.DTYPES[dtype]
    fa, fb = R.gram_inputs(shape, dt)
    fad, fbd = fa.to(DEV), fb.to(DEV)
    Ga, Gb = _gram_run(fad, dtype), _gram_run(fbd, dtype)
    sbuf, S = _padded((r, r), dt, 2 * r)
    loss2 = torch.full((2,), float("nan"), device=DEV)
    partial = torch.full((2048,), float("nan"), device=DEV)
    _call("pmi_style_level", _ptr(fad), _ptr(fbd), _ptr(Ga), _ptr(Gb), _ptr(S), _ptr(loss2), _ptr(partial), n, hw, c, DT_CODE[dtype])
    assert _tail_intact(sbuf, r * r)
    # the means: from the kernel's own fp32 Grams (its inputs) and the 16-bit features, in float64
    d_f, d_g = fa.double() - fb.double(), Ga.cpu().double() - Gb.cpu().double()
    b_f = R.l1_bound(d_f, d_f.numel() // 8, 8)
    b_g = R.l1_bound(d_g, d_g.numel() // 4, 4) + R.EPS32 * float(d_g.abs().mean())       # + the fp32 subtraction Ga - Gb
    w_f = abs(float(loss2[0]) - float(d_f.abs().mean())) / b_f
    w_g = abs(float(loss2[1]) - float(d_g.abs().mean())) / b_g
    print(f"[bound] pmi_style_level {shape} {dtype}: mean|fa - fb| {w_f:.3e}, mean|Ga - Gb| {w_g:.3e} of their bounds")
    assert w_f <= 1.0 and w_g <= 1.0
    # the signs: against float64 Grams wherever the difference is outside what fp32 accumulation can move
    scale = 1.0 / (float(r) * hw)
    g64 = R.gram(R.nchw(fa, n, hw, c)) - R.gram(R.nchw(fb, n, hw, c))
    band = R.gram_bound(fa, scale) + R.gram_bound(fb, scale)
    inside = g64.abs() <= band
    share = float(inside.double().mean())
    print(f"[bound] pmi_style_level {shape} {dtype}: {share:.4%} of Ga - Gb inside the fp32 band (exempt)")
    assert share <= 0.02
    Sc = S.cpu().double()
    assert bool(((Sc == -1) | (Sc == 0) | (Sc == 1)).all())
    assert torch.equal(Sc[~inside], torch.sign(g64)[~inside]), "a sign outside the band differs from float64"
    assert torch.equal(Sc, Sc.t())


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", R.GRAM_SHAPES)
def test_gram_bwd_vs_float64(shape, dtype):
    n, hw, c = shape
    r = n * c
    dt = R.DTYPES[dtype]
    fa, fb = R.gram_inputs(shape, dt)
    g_in = (R.gram_inputs(shape, dt, seed=5)[0] - 0.4).to(dt)
    fad, fbd, gd = fa.to(DEV), fb.to(DEV), g_in.to(DEV)
    Ga, Gb = _gram_run(fad, dtype), _gram_run(fbd, dtype)
    S = torch.empty((r, r), dtype=dt, device=DEV)
    loss2, partial = torch.empty(2, device=DEV), torch.empty(2048, device=DEV)
    _call("pmi_style_level", _ptr(fad), _ptr(fbd), _ptr(Ga), _ptr(Gb), _ptr(S), _ptr(loss2), _ptr(partial), n, hw, c, DT_CODE[dtype])
    c_feat, c_gram = R.level_coefs(n, hw, c, 15.0)
    worst = 0.0
    for gscale in (1.0, 65536.0):
        for gi, gid in ((None, None), (g_in, gd)):
            obuf, out = _padded((n, hw, c), dt, 2 * c)
            tbuf, T = _padded((r, r), dt, 2 * r)
            _call("pmi_gram_bwd", _ptr(fad), _ptr(fbd), _ptr(S), _ptr(T), _ptr(gid), _ptr(out), n, hw, c, c_feat, c_gram, gscale, DT_CODE[dtype])
            assert _tail_intact(obuf, out.numel()) and _tail_intact(tbuf, r * r)
            assert torch.equal(T.float(), S.float() + S.float().t()), "the workspace does not hold S + S^T"
            ref, bound = R.gram_bwd_ref(fa, fb, S.cpu(), gi, c_feat, c_gram, gscale, dt)
            worst = max(worst, _worst(f"pmi_gram_bwd {shape} {dtype} gscale={gscale:g} g_in={gi is not None}", out.cpu(), ref,
                                      bound.clamp_min(1e-300)))
    assert worst <= 1.0
    # fa == fb: S = 0 and sign(fa - fb) = 0, so the level's own gradient is exactly zero
    _call("pmi_style_level", _ptr(fad), _ptr(fad), _ptr(Ga), _ptr(Ga), _ptr(S), _ptr(loss2), _ptr(partial), n, hw, c, DT_CODE[dtype])
    out = torch.full((n, hw, c), 1.0, dtype=dt, device=DEV)
    _call("pmi_gram_bwd", _ptr(fad), _ptr(fad), _ptr(S), _ptr(T), None, _ptr(out), n, hw, c, c_feat, c_gram, 65536.0, DT_CODE[dtype])
    assert float(loss2.abs().max()) == 0.0 and not bool(out.view(torch.int16).bool().any()), "fa == fb does not give exact zeros"


def test_argument_guards():
    """Odd H, C % 16 != 0 and a bad dtype: -1 and nothing written."""
    L = _lib()
    s = torch.cuda.current_stream().cuda_stream
    x = torch.zeros(4096, dtype=torch.float16, device=DEV)
    out = torch.full((4096,), SENTINEL, dtype=torch.int16, device=DEV)
    f32 = torch.full((4096,), float("nan"), device=DEV)
    p = _ptr
    rcs = [L.pmi_maxpool2(p(x), p(out), 1, 3, 4, 16, 0, s), L.pmi_maxpool2(p(x), p(out), 1, 4, 5, 16, 0, s),
           L.pmi_maxpool2(p(x), p(out), 1, 4, 4, 16, 2, s), L.pmi_maxpool2(p(x), p(out), 1, 4, 4, 12, 0, s),
           L.pmi_maxpool2_bwd(p(x), p(x), p(out), 1, 3, 4, 16, 0, s), L.pmi_maxpool2_bwd(p(x), p(x), p(out), 1, 4, 4, 16, 7, s),
           L.pmi_gram_workspace(1, 16, 24), L.pmi_gram(p(x), p(f32), p(f32), 1, 16, 24, 1.0, 0, s),
           L.pmi_gram(p(x), p(f32), p(f32), 1, 16, 16, 1.0, 2, s), L.pmi_gram(p(x), p(f32), p(f32), 1, 0, 16, 1.0, 0, s),
           L.pmi_style_level(p(x), p(x), p(f32), p(f32), p(out), p(f32), p(f32), 1, 16, 24, 0, s),
           L.pmi_style_level(p(x), p(x), p(f32), p(f32), p(out), p(f32), p(f32), 1, 16, 16, 3, s),
           L.pmi_gram_bwd(p(x), p(x), p(x), p(out), None, p(out), 1, 16, 24, 1.0, 1.0, 1.0, 0, s),
           L.pmi_gram_bwd(p(x), p(x), p(x), p(out), None, p(out), 1, 16, 16, 1.0, 1.0, 1.0, -1, s)]
    torch.cuda.synchronize()
    assert rcs == [-1] * len(rcs), rcs
    assert bool((out == SENTINEL).all()) and bool(torch.isnan(f32).all()), "a refused call wrote"


# ================================================ engine ===================================================================================
def _sd(widths):
    from perceptor_amd.engine.vgg import vgg_state_dict_shapes
    from perceptor_amd.utils.synth import synth_state_dict
    return synth_state_dict(vgg_state_dict_shapes(widths), 0, gain=2 ** 0.5)


def _nchw64(t):
    return t.float().cpu().permute(0, 3, 1, 2).double()


def _rel(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["tiny", "mid"])
def test_engine_vs_emulated_float64(name, dtype):
    from perceptor_amd.engine.vgg import VggEngine
    widths, size, n = R.ENGINE_CONFIGS[name]
    dt, u = R.DTYPES[dtype], R.UNIT[R.DTYPES[dtype]]
    sd = _sd(widths)
    eng = VggEngine((widths, size), sd, DEV, dtype)
    a, b = R.engine_inputs(name)
    tb = eng.targets(b.to(DEV))
    rec = {}
    loss, grad = eng.loss_and_grad(a.to(DEV), tb, record=rec)
    torch.cuda.synchronize()
    # ---- features and loss against the emulated tower
    ea, eb = R.level_features(R.tower(sd, widths, a, emulate=dt)), R.level_features(R.tower(sd, widths, b, emulate=dt))
    ok = True
    for l, ((conv, w), depth) in enumerate(zip(R.LEVELS, R.FEATURE_ROUNDINGS)):
        eps = math.sqrt(depth) * u
        ra, rb = _rel(_nchw64(rec["levels"][l][0]), ea[l]), _rel(_nchw64(tb["levels"][l][0]), eb[l])
        print(f"[bound] vgg {name} {dtype} conv {conv}: feature rel-L2 a {ra:.3e} b {rb:.3e}, gate sqrt({depth}) u = {eps:.3e}")
        ok &= ra <= eps and rb <= eps
    fa_eng, fb_eng = [_nchw64(f) for f, _ in rec["levels"]], [_nchw64(f) for f, _ in tb["levels"]]
    kb, fbound = R.loss_kernel_bound(fa_eng, fb_eng), R.loss_feature_bound(ea, eb, u)
    l_own, l64 = float(R.loss(fa_eng, fb_eng)), float(R.loss(ea, eb))
    print(f"[bound] vgg {name} {dtype}: loss {float(loss):.6f} vs float64 of its own features {l_own:.6f}: |diff| / bound = "
          f"{abs(float(loss) - l_own) / kb:.3e}; vs emulated float64 tower {l64:.6f}: |diff| / bound = {abs(float(loss) - l64) / (kb + fbound):.3e}")
    assert ok and abs(float(loss) - l_own) <= kb and abs(float(loss) - l64) <= kb + fbound
    # ---- the image gradient against the emulated tower pinned to the engine's own masks, routes and signs
    layers = R.layer_table(widths)
    acts = {i: _nchw64(t) for i, t in rec["acts"].items()}
    masks = {i: (t > 0).double() for i, t in acts.items()}
    routes = {i: R.first_max_route(acts[i - 2]) for i, l in enumerate(layers[:23]) if l[0] == "pool"}
    signs = [t[1].float().cpu().double() for t in rec["terms"]]
    fsigns = [torch.sign(fa_ - fb_) for fa_, fb_ in zip(fa_eng, fb_eng)]
    x = a.double().clone().requires_grad_(True)
    with torch.enable_grad():
        pinned = R.level_features(R.tower(sd, widths, x, emulate=dt, masks=masks, routes=routes))
        R.loss(pinned, fb_eng, signs=signs, fsigns=fsigns).backward()
    g_rel, gate = _rel(grad.cpu(), x.grad), math.sqrt(R.GRAD_ROUNDINGS) * u
    cos = float(F.cosine_similarity(grad.cpu().double().flatten(), x.grad.flatten(), dim=0))
    print(f"[bound] vgg {name} {dtype}: image gradient vs pinned float64 rel-L2 = {g_rel:.3e} (gate sqrt({R.GRAD_ROUNDINGS}) u = {gate:.3e}), cos = {cos:.6f}")
    assert g_rel <= gate


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("case", ["same", "resized"])
def test_style_transfer_vs_reference_fixture(case, dtype):
    from perceptor_amd import losses
    g = golden("style_transfer_reference")
    widths, size = tuple(int(v) for v in g["widths"]), int(g["size"])
    st = losses.StyleTransfer(widths=widths, size=size, dtype=dtype, seed=int(g["seed"])).to(DEV)
    a, b = g[case + "_a"].float().to(DEV), g[case + "_b"].float().to(DEV)
    loss, grad = st.loss_and_grad(a, b)
    ref = float(g[case + "_loss"])
    cos = float(F.cosine_similarity(grad.cpu().double().flatten(), g[case + "_grad_a"].flatten(), dim=0))
    tol = FIXTURE_LOSS_TOL[(case, dtype)]
    print(f"[bound] StyleTransfer {case} {dtype}: loss {float(loss):.6f} vs reference {ref:.6f}: |diff| / tol = {abs(float(loss) - ref) / tol:.3e}; "
          f"unpinned gradient cosine {cos:.5f} (printed, not asserted: the gradient is piecewise constant in masks, routes and signs)")
    assert grad.shape == a.shape
    assert abs(float(loss) - ref) <= tol
    enc = st.encode(a)
    for i, e in enumerate(enc):
        assert tuple(e.shape) == tuple(int(v) for v in g[f"{case}_enc{i}_shape"])


# ================================================ the public classes at the product configuration ==========================================
@pytest.fixture(scope="module")
def product():
    from perceptor_amd import losses
    from perceptor_amd.utils.synth import seeded_noise
    st = losses.StyleTransfer().to(DEV)
    a = (seeded_noise((2, 3, 256, 256), 11) * 0.25 + 0.5).clamp(0, 1).to(DEV)
    b = (seeded_noise((2, 3, 256, 256), 12) * 0.25 + 0.5).clamp(0, 1).to(DEV)
    return st, a, b


def test_product_identity_and_determinism(product):
    st, a, b = product
    loss, grad = st.loss_and_grad(a, a)
    assert float(loss) == 0.0 and not bool(grad.bool().any()), "loss_and_grad(a, a) is not exactly (0, zeros)"
    l1, g1 = st.loss_and_grad(a, b)
    l2, g2 = st.loss_and_grad(a, b)
    assert torch.equal(l1, l2) and torch.equal(g1, g2), "two runs differ"
    assert float(l1) > 0 and bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
    print(f"[info] StyleTransfer product f16 N=2: loss {float(l1):.6f}, |grad| max {float(g1.abs().max()):.3e}")
    # cached targets of stored encodings against the live images_b
    st.encodings = torch.nn.ParameterList([torch.nn.Parameter(t, requires_grad=False) for t in st.encode(b)])
    st._cache = None
    l3, g3 = st.loss_and_grad(a)
    assert st._cache is not None
    l4, g4 = st.loss_and_grad(a)
    assert torch.equal(l1, l3) and torch.equal(g1, g3) and torch.equal(l3, l4) and torch.equal(g3, g4), "cached targets differ from live images_b"
    st.to(DEV)
    assert st._cache is None, "the cache survived .to()"
    assert float(st.loss(st.encode(a), st.encodings)) == float(l1)
    del st.encodings


def test_product_autograd_paths(product):
    st, a, b = product
    l0, g0 = st.loss_and_grad(a, b)
    x = a.clone().requires_grad_(True)
    y = b.clone()
    val = st(x, y)
    val.backward()
    assert torch.equal(val.detach(), l0) and torch.equal(x.grad, g0)
    assert y.grad is None
    x2, y2 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    st(x2, y2).backward()
    assert torch.equal(x2.grad, g0) and y2.grad is not None and y2.grad.shape == b.shape
    # the gradient to b is the a-gradient of the swapped call: the loss is symmetric in its arguments
    _, gswap = st.loss_and_grad(b, a)
    assert torch.equal(y2.grad, gswap)
    with pytest.raises(AttributeError):
        st(a)
    with pytest.raises(ValueError, match="2 vs 1"):
        st.loss_and_grad(a, b[:1])


def test_product_resized_input_and_vgg19(product):
    from perceptor_amd.utils.synth import seeded_noise
    st, a, b = product
    big = (seeded_noise((2, 3, 320, 288), 13) * 0.25 + 0.5).clamp(0, 1).to(DEV)
    loss, grad = st.loss_and_grad(big, b)
    assert grad.shape == big.shape and bool(torch.isfinite(grad).all()) and float(loss) > 0
    x = a[:, :, :64, :96].clone().requires_grad_(True)
    y = st.model(x)
    assert tuple(y.shape) == (2, 512, 2, 3) and y.dtype == torch.float32
    y.square().sum().backward()
    assert x.grad.shape == x.shape and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
    with pytest.raises(ValueError, match="Width"):
        st.model(a[:, :, :64, :60])
    with pytest.raises(ValueError, match="Height"):
        st.model(a[:, :, :60, :64])
    with pytest.raises(ValueError, match="32"):
        st.model(a[:, :, :64, :72])
    with pytest.raises(RuntimeError):
        st.model(a[:, :, :64, :64].cpu())
