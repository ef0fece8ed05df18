"""GPU: the kernels of csrc/lpips.hip (pmi_lpips_level, pmi_lpips_level_bwd) against the float64 restatements and bounds of
tests/_lpips_ref64.py, engine/lpips.py's LpipsEngine against the emulated float64 tower (tap features, value, and both image gradients with
the engine's own ReLU masks and pool routes pinned), and losses.LPIPS's properties at N = 2, 256 x 256 with VGG-16's widths.

Every comparison prints its worst |got - ref| / bound (or relative L2 and its gate) before it asserts.  The inputs are
tests/_lpips_ref64.py's seeded generators: tests/test_lpips_cpu.py runs the seeded defects at exactly these inputs.

Measured on an MI355X: see DESIGN.md section 29.
"""
import math

import pytest
import torch

import _lpips_ref64 as R

pytestmark = pytest.mark.gpu

DEV = "cuda"
SENTINEL = 0x7B7B                      # a 16-bit pattern (about 6.1e4 in f16, 1.3e36 in bf16) no kernel under test produces
DT_CODE = {"f16": 0, "bf16": 1}


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
    w = float(((got.double().cpu() - ref.double()).abs() / bound.clamp_min(1e-300)).max())
    print(f"[bound] {tag}: worst |got - ref| / bound = {w:.3e}")
    return w


def _padded16(shape, dtype, extra):
    n = math.prod(shape)
    buf = torch.full((n + extra,), SENTINEL, dtype=torch.int16, device=DEV).view(dtype)
    return buf, buf[:n].view(shape)


def _padded32(shape, extra):
    n = math.prod(shape)
    buf = torch.full((n + extra,), float("nan"), dtype=torch.float32, device=DEV)
    return buf, buf[:n].view(shape)


def _tail16(buf, n):
    return bool((buf[n:].view(torch.int16) == SENTINEL).all())


def _tail32(buf, n):
    return bool(torch.isnan(buf[n:]).all())


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ================================================ level kernels ==========================================================================
def _level_fwd(fa, fb, w, n, hw, c, dtype, want_mean=True):
    sb, s = _padded32((n, hw), 64)
    ab, na = _padded32((n, hw), 64)
    bb, nb = _padded32((n, hw), 64)
    mb, mean = _padded32((n,), 8)
    partial = torch.full((512 * n,), float("nan"), device=DEV)
    _call("pmi_lpips_level", _ptr(fa), _ptr(fb), _ptr(w), _ptr(s), _ptr(na), _ptr(nb), _ptr(mean) if want_mean else None,
          _ptr(partial) if want_mean else None, n, hw, c, DT_CODE[dtype])
    assert _tail32(sb, n * hw) and _tail32(ab, n * hw) and _tail32(bb, n * hw) and _tail32(mb, n), "pmi_lpips_level wrote past an output"
    if not want_mean:
        assert bool(torch.isnan(mean).all()) and bool(torch.isnan(partial).all()), "mean = NULL, yet mean or partial was written"
    return s, na, nb, mean


def _level_bwd(fa, fb, w, na, nb, r, gia, gib, sides, n, hw, c, gscale, dtype):
    dt = R.DTYPES[dtype]
    abuf, da = _padded16((n, hw, c), dt, 2 * c)
    bbuf, db = _padded16((n, hw, c), dt, 2 * c)
    _call("pmi_lpips_level_bwd", _ptr(fa), _ptr(fb), _ptr(w), _ptr(na), _ptr(nb), _ptr(r), _ptr(gia), _ptr(gib), _ptr(da) if "a" in sides else None,
          _ptr(db) if "b" in sides else None, n, hw, c, gscale, DT_CODE[dtype])
    assert _tail16(abuf, n * hw * c) and _tail16(bbuf, n * hw * c), "pmi_lpips_level_bwd wrote past an output"
    for side, buf in (("a", abuf), ("b", bbuf)):
        if side not in sides:
            assert bool((buf.view(torch.int16) == SENTINEL).all()), f"side {side} was not asked for, yet written"
    return da, db


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", R.LEVEL_SHAPES)
def test_level_kernels_vs_float64(shape, dtype):
    n, hw, c = shape
    dt = R.DTYPES[dtype]
    cases = R.level_inputs(shape, dt)
    assert R.zero_pixel_patterns(cases) == {"a", "b", "ab"}
    worst = 0.0
    for k, (fa, fb, w, r, gia, gib) in enumerate(cases):
        fad, fbd, wd, rd, giad, gibd = (t.to(DEV) for t in (fa, fb, w, r, gia, gib))
        for wv, wvd in ((w, wd), (None, None)):
            tag = f"{shape} {dtype} case {k} w={'given' if wv is not None else 'NULL'}"
            s, na, nb, mean = _level_fwd(fad, fbd, wvd, n, hw, c, dtype)
            s2, na2, nb2, mean2 = _level_fwd(fad, fbd, wvd, n, hw, c, dtype)
            assert all(torch.equal(_bits(x), _bits(y)) for x, y in ((s, s2), (na, na2), (nb, nb2), (mean, mean2))), "two forward runs differ"
            s3, na3, nb3, _ = _level_fwd(fad, fbd, wvd, n, hw, c, dtype, want_mean=False)
            assert torch.equal(_bits(s), _bits(s3)) and torch.equal(_bits(na), _bits(na3)) and torch.equal(_bits(nb), _bits(nb3))
            refs, bounds = R.level_ref(fa, fb, wv)
            for name, got, ref, bound in zip(("s", "na", "nb", "mean"), (s, na, nb, mean), refs, bounds):
                worst = max(worst, _worst(f"pmi_lpips_level {tag} {name}", got, ref, bound))
            za, zb = fa.float().abs().sum(-1) == 0, fb.float().abs().sum(-1) == 0
            assert not bool(na.cpu()[za].bool().any()) and not bool(nb.cpu()[zb].bool().any()) and not bool(s.cpu()[za & zb].bool().any())
            for gscale in (1.0, 65536.0):
                for gi, gid in (((None, None), (None, None)), ((gia, gib), (giad, gibd))):
                    da, db = _level_bwd(fad, fbd, wvd, na, nb, rd, gid[0], gid[1], "ab", n, hw, c, gscale, dtype)
                    da2, db2 = _level_bwd(fad, fbd, wvd, na, nb, rd, gid[0], gid[1], "ab", n, hw, c, gscale, dtype)
                    assert torch.equal(_bits(da), _bits(da2)) and torch.equal(_bits(db), _bits(db2)), "two backward runs differ"
                    da1, _ = _level_bwd(fad, fbd, wvd, na, nb, rd, gid[0], gid[1], "a", n, hw, c, gscale, dtype)
                    _, db1 = _level_bwd(fad, fbd, wvd, na, nb, rd, gid[0], gid[1], "b", n, hw, c, gscale, dtype)
                    assert torch.equal(_bits(da), _bits(da1)) and torch.equal(_bits(db), _bits(db1)), "a both-sides launch differs from one-sided launches"
                    # the reference takes the kernel's own fp32 norms' inputs: the 16-bit features
                    (ra, rb), (ba, bb) = R.level_bwd_ref(fa, fb, wv, r, gi[0], gi[1], gscale, dt)
                    t2 = f"pmi_lpips_level_bwd {tag} gscale={gscale:g} g_in={gi[0] is not None}"
                    worst = max(worst, _worst(t2 + " dFa", da, ra, ba), _worst(t2 + " dFb", db, rb, bb))
                    assert bool(torch.isfinite(da.float()).all()) and bool(torch.isfinite(db.float()).all())
                    assert not bool(_bits(da).cpu()[za].bool().any()) and not bool(_bits(db).cpu()[zb].bool().any()), "an all-zero pixel has a gradient"
        # the sides swapped: the same bits with the roles exchanged; fa == fb: exact zeros (products are rounded before they are subtracted)
        s, na, nb, mean = _level_fwd(fad, fbd, wd, n, hw, c, dtype)
        sw = _level_fwd(fbd, fad, wd, n, hw, c, dtype)
        assert all(torch.equal(_bits(x), _bits(y)) for x, y in zip((s, na, nb, mean), (sw[0], sw[2], sw[1], sw[3]))), "the level is not bit-symmetric"
        da, db = _level_bwd(fad, fbd, wd, na, nb, rd, giad, gibd, "ab", n, hw, c, 65536.0, dtype)
        da_sw, db_sw = _level_bwd(fbd, fad, wd, nb, na, rd, gibd, giad, "ab", n, hw, c, 65536.0, dtype)
        assert torch.equal(_bits(da), _bits(db_sw)) and torch.equal(_bits(db), _bits(da_sw)), "the adjoint is not bit-symmetric"
        s0, na0, nb0, mean0 = _level_fwd(fad, fad, wd, n, hw, c, dtype)
        d0a, d0b = _level_bwd(fad, fad, wd, na0, nb0, rd, None, None, "ab", n, hw, c, 65536.0, dtype)
        assert not bool(s0.bool().any()) and not bool(mean0.bool().any()) and not bool(d0a.bool().any()) and not bool(d0b.bool().any()), \
            "fa == fb does not give exact zeros"
    assert worst <= 1.0


def test_level_argument_guards():
    """C = 24 (not a multiple of 16), C = 528 (> 512), HW = 0, a bad dtype, no output side: -1 and nothing written."""
    L = _lib()
    st = torch.cuda.current_stream().cuda_stream
    x = torch.zeros(8192, dtype=torch.float16, device=DEV)
    f32 = torch.full((4096,), float("nan"), device=DEV)
    ones = torch.ones(4096, device=DEV)
    out = torch.full((8192,), SENTINEL, dtype=torch.int16, device=DEV)
    p = _ptr
    rcs = [L.pmi_lpips_level(p(x), p(x), None, p(f32), p(f32), p(f32), p(f32), p(f32), 1, 4, 24, 0, st),
           L.pmi_lpips_level(p(x), p(x), None, p(f32), p(f32), p(f32), p(f32), p(f32), 1, 4, 528, 0, st),
           L.pmi_lpips_level(p(x), p(x), None, p(f32), p(f32), p(f32), p(f32), p(f32), 1, 0, 16, 0, st),
           L.pmi_lpips_level(p(x), p(x), None, p(f32), p(f32), p(f32), p(f32), p(f32), 1, 4, 16, 2, st),
           L.pmi_lpips_level(p(x), p(x), None, p(f32), p(f32), p(f32), p(f32), None, 1, 4, 16, 0, st),
           L.pmi_lpips_level_bwd(p(x), p(x), None, p(ones), p(ones), p(ones), None, None, p(out), p(out), 1, 4, 24, 1.0, 0, st),
           L.pmi_lpips_level_bwd(p(x), p(x), None, p(ones), p(ones), p(ones), None, None, p(out), p(out), 1, 4, 528, 1.0, 0, st),
           L.pmi_lpips_level_bwd(p(x), p(x), None, p(ones), p(ones), p(ones), None, None, p(out), p(out), 1, 4, 16, 1.0, 3, st),
           L.pmi_lpips_level_bwd(p(x), p(x), None, p(ones), p(ones), p(ones), None, None, None, None, 1, 4, 16, 1.0, 0, st),
           L.pmi_lpips_level_bwd(p(x), p(x), None, p(ones), p(ones), p(ones), None, None, p(out), p(out), 1, 4, 16, float("nan"), 0, st)]
    torch.cuda.synchronize()
    assert rcs == [-1] * len(rcs), rcs
    assert bool((out == SENTINEL).all()) and bool(torch.isnan(f32).all()), "a refused call wrote"


# ================================================ engine =================================================================================
def _nchw64(t):
    return t.float().cpu().permute(0, 3, 1, 2).double()


def _rel(got, ref):
    return float((got.double().cpu() - ref.double()).norm() / ref.double().norm())


@pytest.fixture(scope="module")
def engine_case():
    widths, n, hw = R.ENGINE_CONFIG
    sd, lins = R.engine_weights(widths)
    a, b = R.engine_inputs()
    emul = {dtype: (R.taps(R.tower(sd, widths, a, dt)), R.taps(R.tower(sd, widths, b, dt))) for dtype, dt in R.DTYPES.items()}
    return widths, sd, lins, a, b, emul


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("mode", ["mean", "spatial", "nolin", "mean-targets"])
def test_engine_vs_emulated_float64(engine_case, mode, dtype):
    """mean / spatial / nolin: a live images_b (one 2N tower pass, both gradients from one 2N backward walk); mean-targets: cached targets
    with their tape (a's tower alone, the two sides walked as two N-sample streams)."""
    from perceptor_amd.engine.lpips import LpipsEngine
    widths, sd, lins, a, b, emul = engine_case
    spatial, lw = mode == "spatial", (None if mode == "nolin" else lins)
    dt, u = R.DTYPES[dtype], R.UNIT[R.DTYPES[dtype]]
    eng = LpipsEngine(widths, sd, lw, DEV, dtype)
    n, hw = a.shape[0], tuple(a.shape[2:])
    go = torch.from_numpy(R._gen(6000).standard_normal((n, 1) + (hw if spatial else (1, 1)))).float()
    second = eng.targets(b.to(DEV), keep_tape=True) if mode == "mean-targets" else b.to(DEV)
    rec = {}
    out, ga, gb = eng.loss_and_grad(a.to(DEV), second, grad_out=go.to(DEV), grad_b=True, spatial=spatial, record=rec)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (n, 1) + (hw if spatial else (1, 1)) and ga.shape == a.shape and gb.shape == b.shape
    # ---- tap features against the emulated tower
    ea, eb = emul[dtype]
    fa_eng, fb_eng = [_nchw64(f) for f in rec["feats_a"]], [_nchw64(f) for f in rec["feats_b"]]
    ok = True
    for l, depth in enumerate(R.FEATURE_ROUNDINGS):
        eps = math.sqrt(depth) * u
        ra, rb = _rel(fa_eng[l], ea[l]), _rel(fb_eng[l], eb[l])
        print(f"[bound] lpips {mode} {dtype} {R.TAP_NAMES[l]}: feature rel-L2 a {ra:.3e} b {rb:.3e}, gate sqrt({depth}) u = {eps:.3e}")
        ok &= ra <= eps and rb <= eps
    assert ok
    # ---- the value against the float64 value of the engine's own features
    own = R.output(fa_eng, fb_eng, lw, hw, spatial)
    vb = R.value_bound(fa_eng, fb_eng, lw, hw, spatial)
    assert _worst(f"lpips {mode} {dtype} value vs float64 of its own features", out, own, vb) <= 1.0
    # ---- both image gradients against the emulated tower pinned to the engine's masks and routes
    gate = math.sqrt(R.GRAD_ROUNDINGS) * u
    acts_a, acts_b = {i: _nchw64(t) for i, t in rec["acts"].items()}, {i: _nchw64(t) for i, t in rec["acts_b"].items()}
    pa = R.pinned_grad(sd, lw, widths, a, acts_a, fb_eng, "a", spatial, go, dt)
    pb = R.pinned_grad(sd, lw, widths, b, acts_b, fa_eng, "b", spatial, go, dt)
    ra, rb = _rel(ga, pa), _rel(gb, pb)
    print(f"[bound] lpips {mode} {dtype}: image gradient vs pinned float64 rel-L2 a {ra:.3e} b {rb:.3e} (gate sqrt({R.GRAD_ROUNDINGS}) u = {gate:.3e})")
    # for the record, not gated: the level adjoint taken at the emulated tower's own features instead of the engine's (adds the forward
    # deviation of the two towers times the level's conditioning; R.pinned_grad has the reasoning)
    qa = R.pinned_grad(sd, lw, widths, a, acts_a, fb_eng, "a", spatial, go, dt, at_engine=False)
    qb = R.pinned_grad(sd, lw, widths, b, acts_b, fa_eng, "b", spatial, go, dt, at_engine=False)
    print(f"[info] lpips {mode} {dtype}: the same with the level adjoint at the emulated features: a {_rel(ga, qa):.3e} b {_rel(gb, qb):.3e}")
    assert bool(torch.isfinite(ga).all()) and bool(torch.isfinite(gb).all()) and ra <= gate and rb <= gate


def test_engine_size_errors():
    from perceptor_amd.engine.lpips import LpipsEngine
    widths, _, _ = R.ENGINE_CONFIG
    sd, lins = R.engine_weights(widths)
    eng = LpipsEngine(widths, sd, lins, DEV, "bf16")
    with pytest.raises(ValueError, match="24 x 32"):
        eng.targets(torch.zeros(1, 3, 24, 32, device=DEV))
    tb = eng.targets(torch.zeros(1, 3, 32, 32, device=DEV))
    with pytest.raises(ValueError, match="equal shape"):
        eng.value(torch.zeros(1, 3, 32, 48, device=DEV), tb)
    with pytest.raises(RuntimeError, match="keep_tape"):
        eng.loss_and_grad(torch.zeros(1, 3, 32, 32, device=DEV), tb, grad_b=True)


# ================================================ the class at N = 2, 256 x 256, VGG-16's widths =========================================
@pytest.fixture(scope="module")
def product():
    from perceptor_amd import losses
    from perceptor_amd.utils.synth import seeded_noise
    lp = losses.LPIPS().to(DEV)
    a = (seeded_noise((2, 3, 256, 256), 21) * 0.25 + 0.5).clamp(0, 1).to(DEV)
    b = (seeded_noise((2, 3, 256, 256), 22) * 0.25 + 0.5).clamp(0, 1).to(DEV)
    return lp, a, b


def test_product_identity_symmetry_determinism(product):
    lp, a, b = product
    v0, g0a, g0b = lp.loss_and_grad(a, a, grad_b=True)
    assert tuple(v0.shape) == (2, 1, 1, 1)
    assert not bool(v0.bool().any()) and not bool(g0a.bool().any()) and not bool(g0b.bool().any()), "lpips(a, a) is not exactly (0, zeros, zeros)"
    v1, ga1, gb1 = lp.loss_and_grad(a, b, grad_b=True)
    v2, ga2, gb2 = lp.loss_and_grad(a, b, grad_b=True)
    assert torch.equal(v1, v2) and torch.equal(ga1, ga2) and torch.equal(gb1, gb2), "two runs differ"
    assert float(v1.min()) > 0 and bool(torch.isfinite(ga1).all()) and bool(torch.isfinite(gb1).all()) and float(ga1.abs().max()) > 0
    print(f"[info] LPIPS product f16 N=2 256x256: value {v1.flatten().tolist()}, |grad a| max {float(ga1.abs().max()):.3e}")
    # both calls run [a; b] resp. [b; a] as one 2N tower pass and one 2N backward walk (the same batch route), so the symmetry is bit for bit
    v3, ga3, gb3 = lp.loss_and_grad(b, a, grad_b=True)
    assert torch.equal(v1, v3), "value(a, b) differs from value(b, a)"
    assert torch.equal(gb1, ga3) and torch.equal(ga1, gb3), "grad_b(a, b) differs from grad_a(b, a)"
    v5, ga5 = lp.loss_and_grad(a, b)
    assert torch.equal(v1, v5), "the value depends on grad_b"
    # cached targets are ANOTHER batch route than a live images_b (each image batch alone, N samples, against one 2N pass): the tap features
    # are held to the feature gate sqrt(d_l) u against each other (and reported when they happen to be bit-equal); two cached calls are bit-equal
    eng = lp._need_engine()
    tb = lp.targets(b)
    la, lb = eng.pair(a, b)
    ta = eng.targets(a)
    u, same = R.UNIT[torch.float16], True
    for l, depth in enumerate(R.FEATURE_ROUNDINGS):
        ra = float((la["feats"][l].double() - ta["feats"][l].double()).norm() / ta["feats"][l].double().norm())
        rb = float((lb["feats"][l].double() - tb["feats"][l].double()).norm() / tb["feats"][l].double().norm())
        same &= ra == 0.0 and rb == 0.0
        print(f"[bound] LPIPS product {R.TAP_NAMES[l]}: 2N pass against N pass, feature rel-L2 a {ra:.3e} b {rb:.3e}, gate {math.sqrt(depth) * u:.3e}")
        assert ra <= math.sqrt(depth) * u and rb <= math.sqrt(depth) * u
    v4, ga4 = lp.loss_and_grad(a, tb)
    v6, ga6 = lp.loss_and_grad(a, tb)
    assert torch.equal(v4, v6) and torch.equal(ga4, ga6), "two runs against cached targets differ"
    print(f"[info] LPIPS product: cached targets against live images_b: features bit-equal: {same}; value {v4.flatten().tolist()} vs {v1.flatten().tolist()}, "
          f"gradient rel-L2 {float((ga4 - ga1).norm() / ga1.norm()):.3e}")


def test_product_autograd_paths(product):
    lp, a, b = product
    """forward(a, b).sum().backward() equals loss_and_grad, like with like: the gradient to a alone walks a's N samples, both gradients walk
    the 2N batch (another batch route of the dX convolutions: equal up to rounding, compared under the gradient gate)."""
    v0, ga0 = lp.loss_and_grad(a, b)
    v1, ga1, gb1 = lp.loss_and_grad(a, b, grad_b=True)
    x, y = a.clone().requires_grad_(True), b.clone()
    val = lp(x, y)
    val.sum().backward()
    assert torch.equal(val.detach(), v0) and torch.equal(x.grad, ga0) and y.grad is None
    x2, y2 = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    val2 = lp(x2, y2)
    val2.sum().backward()
    assert torch.equal(val2.detach(), v1) and torch.equal(v0, v1) and torch.equal(x2.grad, ga1) and torch.equal(y2.grad, gb1)
    rel = float((ga1 - ga0).norm() / ga0.norm())
    print(f"[bound] LPIPS product: gradient to a from the 2N walk against the N walk, rel-L2 {rel:.3e} (gate sqrt(17) u)")
    assert rel <= math.sqrt(R.GRAD_ROUNDINGS) * R.UNIT[torch.float16]
    # per-sample scaling of the eager gradients equals the fused path's grad_out
    wts = torch.tensor([0.5, -2.0], device=DEV).view(2, 1, 1, 1)
    x3 = a.clone().requires_grad_(True)
    (lp(x3, b) * wts).sum().backward()
    assert torch.equal(x3.grad, ga0 * wts)
    _, gw = lp.loss_and_grad(a, b, grad_out=wts)
    assert float((gw - x3.grad).norm() / x3.grad.norm()) <= math.sqrt(R.GRAD_ROUNDINGS) * R.UNIT[torch.float16]
    with pytest.raises(ValueError, match=r"\(2, 3, 256, 256\).*\(1, 3, 256, 256\)"):
        lp(a, b[:1])
    with pytest.raises(RuntimeError):
        lp(a, b.cpu())


def test_product_spatial_autograd(product):
    from perceptor_amd import losses
    lp, a, b = product
    sp = losses.LPIPS(spatial=True).to(DEV)
    go = torch.from_numpy(R._gen(6100).standard_normal((2, 1, 256, 256))).float().to(DEV)
    v0, ga0, gb0 = sp.loss_and_grad(a, b, grad_out=go, grad_b=True)
    assert tuple(v0.shape) == (2, 1, 256, 256) and float(v0.min()) >= 0
    x, y = a.clone().requires_grad_(True), b.clone().requires_grad_(True)
    val = sp(x, y)
    (val * go).sum().backward()
    assert torch.equal(val.detach(), v0) and torch.equal(x.grad, ga0) and torch.equal(y.grad, gb0)
    # the spatial map's mean is the scalar distance up to the bilinear band's edge handling: same order of magnitude, not asserted tightly
    v1, _ = lp.loss_and_grad(a, b)
    print(f"[info] LPIPS spatial map mean {v0.mean(dim=(2, 3)).flatten().tolist()} vs scalar {v1.flatten().tolist()}")
    vz, gz = sp.loss_and_grad(a, a)
    assert not bool(vz.bool().any()) and not bool(gz.bool().any())
