"""GPU: models.MidasDepth -- the kernels of csrc/dpt.hip by name against float64, VitEngine's timm options and taps, DptEngine and the
class against the float64 restatement (tests/_dpt_ref64.py) at two toy configurations, and the product configuration's shapes.

Kernel bounds are n u A: n fp32 operations on terms whose absolute sum is A, u = 2^-24, plus half an ulp of the 16-bit
output type where the output is 16-bit.  Engine gates are 2 x MEASURED: the distance of the bf16 / f16-emulated restatement from the exact
one, measured on the CPU (tests/test_midas_depth_cpu.py recomputes it); the factor 2 covers the GEMMs' accumulation order and the commuted
1 x 1 convolution, which the emulation does not model.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dpt_ref64 as D                      # noqa: E402
from _glue_ref64 import U, ulp16            # noqa: E402

pytestmark = pytest.mark.gpu

DT = {"bf16": (1, torch.bfloat16), "f16": (0, torch.float16)}

# max |emulated - exact| / max |exact| on the CPU (D.measured), rounded up to two digits; z_err: max |z emulated - z exact|, absolute
MEASURED = {
    ("a", "bf16"): dict(depth=0.014, grad_mean=0.0067, grad_rand=0.0088, z_err=0.046),
    ("a", "f16"): dict(depth=0.0014, grad_mean=0.0011, grad_rand=0.0013, z_err=0.0049),
    ("b", "bf16"): dict(depth=0.021, grad_mean=0.012, grad_rand=0.012, z_err=0.099),
    ("b", "f16"): dict(depth=0.0030, grad_mean=0.00084, grad_rand=0.00093, z_err=0.015),
}


def _call(name, *args):
    from perceptor_amd._hip import call
    call(name, *args)


def _guard(shape, dtype, pad=64):
    """a NaN-filled buffer with `pad` NaN elements on either side of the payload: (payload view, whole buffer)"""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((pad + n + pad,), float("nan"), dtype=dtype, device="cuda")
    return buf[pad:pad + n].view(shape), buf


def _intact(buf, pad=64):
    return bool(buf[:pad].isnan().all() and buf[-pad:].isnan().all() and torch.isfinite(buf[pad:-pad]).all())


def _vals(shape, seed, dtype, zeros=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    if zeros:
        x[torch.rand(shape, generator=g) < 0.2] = 0.0
    return x.to(dtype)


def _twice(run):
    """run() -> (outputs, guard buffers); both runs must agree bit for bit and leave the guards alone"""
    a, bufs = run()
    assert all(_intact(b) for b in bufs), "an output was left unwritten, is not finite, or a guard band was written"
    b, _ = run()
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.uint8), y.view(torch.uint8)), "two runs differ"
    return [t.double().cpu() for t in a]


def _hold(name, got, ref, tol):
    w = float(((got - ref).abs() / tol.clamp_min(1e-300)).max())
    print(f"[bound] {name}: worst |got - ref| / bound = {w:.3f}")
    assert w <= 1.0, name


BIL = [(1, 1, 1, 8), (2, 1, 3, 8), (1, 2, 5, 16), (1, 3, 3, 24), (1, 12, 12, 64)]


def _up64(x_nhwc):
    return F.interpolate(x_nhwc.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", BIL)
@pytest.mark.parametrize("addend", [False, True])
def test_bilinear2_ac_fwd(shape, dtype, addend):
    code, td = DT[dtype]
    n, h, w, c = shape
    x = _vals(shape, 1, td).cuda()
    r = _vals((n, 2 * h, 2 * w, c), 2, td).cuda() if addend else None

    def run():
        y, buf = _guard((n, 2 * h, 2 * w, c), td)
        _call("pmi_bilinear2_ac_fwd", x.data_ptr(), r.data_ptr() if addend else None, y.data_ptr(), n, h, w, c, code)
        return [y], [buf]

    (y,) = _twice(run)
    ref = _up64(x.cpu()) + (r.cpu().double() if addend else 0.0)
    A = _up64(x.cpu().abs()) + (r.cpu().double().abs() if addend else 0.0)
    # two weights (a division and a subtraction each), four products, four additions: 10 operations asked
    _hold(f"bilinear2_ac_fwd {shape} {dtype} addend={addend}", y, ref, 10 * U * A + 0.5 * ulp16(ref, dtype) * (1 + 2.0 ** -9))
    if h == 1 and w == 1 and not addend:
        assert torch.equal(y, x.cpu().double().expand(n, 2, 2, c)), "H = W = 1 must copy"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", BIL)
def test_bilinear2_ac_bwd(shape, dtype):
    code, td = DT[dtype]
    n, h, w, c = shape
    g = _vals((n, 2 * h, 2 * w, c), 3, td).cuda()

    def run():
        dx, buf = _guard(shape, td)
        _call("pmi_bilinear2_ac_bwd", g.data_ptr(), dx.data_ptr(), n, h, w, c, code)
        return [dx], [buf]

    (dx,) = _twice(run)

    def adjoint(gg):
        x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
        (d,) = torch.autograd.grad((_up64(x) * gg).sum(), x)
        return d

    ref, A = adjoint(g.cpu().double()), adjoint(g.cpu().double().abs())
    # up to 5 x 5 contributing outputs per input: 25 weighted terms, each weight a product of two 3-operation weights
    _hold(f"bilinear2_ac_bwd {shape} {dtype}", dx, ref, 32 * U * A + 0.5 * ulp16(ref, dtype) * (1 + 2.0 ** -9))
    # <up x, g> = <x, up^T g> with the KERNEL's forward: both sides from 16-bit results, so the roundings of both enter
    x = _vals(shape, 4, td).cuda()
    y = torch.empty((n, 2 * h, 2 * w, c), dtype=td, device="cuda")
    _call("pmi_bilinear2_ac_fwd", x.data_ptr(), None, y.data_ptr(), n, h, w, c, code)
    lhs = float((y.double().cpu() * g.double().cpu()).sum())
    rhs = float((x.double().cpu() * dx).sum())
    eps16 = 2.0 ** (-8 if dtype == "bf16" else -11)
    tol = (eps16 + 40 * U) * (float((_up64(x.cpu().abs()) * g.cpu().double().abs()).sum()) + float((x.cpu().double().abs() * A).sum()))
    print(f"[bound] adjoint identity {shape} {dtype}: |lhs - rhs| / bound = {abs(lhs - rhs) / max(tol, 1e-300):.3f}")
    assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("k", [2, 4])
@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 2, 3, 16), (1, 4, 4, 32)])
def test_depth_space(shape, k, dtype):
    code, td = DT[dtype]
    n, h, w, c = shape
    x = _vals((n, h, w, k * k * c), 5, td).cuda()
    bias = torch.randn(c, generator=torch.Generator().manual_seed(6)).cuda()

    def run(b):
        def go():
            y, buf = _guard((n, k * h, k * w, c), td)
            _call("pmi_depth_to_space", x.data_ptr(), b.data_ptr() if b is not None else None, y.data_ptr(), n, h, w, c, k, code)
            return [y], [buf]
        return go

    (y,) = _twice(run(bias))
    perm = x.cpu().double().view(n, h, w, k, k, c).permute(0, 1, 3, 2, 4, 5).reshape(n, k * h, k * w, c)      # (ky, kx, c) columns
    ref = perm + bias.cpu().double()
    _hold(f"depth_to_space {shape} k={k} {dtype}", y, ref, U * (perm.abs() + bias.cpu().double().abs()) + 0.5 * ulp16(ref, dtype) * (1 + 2.0 ** -9))
    # against ConvTranspose2d: GEMM to (ky, kx, co) columns, then this permutation
    wt = _vals((c, c, k, k), 7, torch.float32).double()
    xin = _vals((n, h, w, c), 8, torch.float32).double()
    cols = xin.reshape(-1, c) @ wt.permute(2, 3, 1, 0).reshape(k * k * c, c).t()
    via = cols.view(n, h, w, k, k, c).permute(0, 1, 3, 2, 4, 5).reshape(n, k * h, k * w, c)
    ct = F.conv_transpose2d(xin.permute(0, 3, 1, 2), wt, None, stride=k).permute(0, 2, 3, 1)
    assert float((via - ct).abs().max()) <= 1e-12 * float(ct.abs().max())
    # the round trip is the identity bit for bit
    y0, _ = run(None)()
    back, buf = _guard((n, h, w, k * k * c), td)
    _call("pmi_space_to_depth", y0[0].data_ptr(), back.data_ptr(), n, h, w, c, k, code)
    assert _intact(buf) and torch.equal(back.view(torch.int16), x.view(torch.int16))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", [(1, 2, 64), (2, 5, 128), (1, 17, 128), (1, 577, 1024)])
def test_tap_split_join_colsum_add(shape, dtype):
    code, td = DT[dtype]
    n, t, w = shape
    p = t - 1
    x = _vals(shape, 9, torch.float32).cuda()

    def split():
        tok, b0 = _guard((n * p, w), td)
        cls, b1 = _guard((n, w), td)
        _call("pmi_dpt_tap_split", x.data_ptr(), tok.data_ptr(), cls.data_ptr(), n, t, w, code)
        return [tok, cls], [b0, b1]

    tok, cls = _twice(split)
    assert torch.equal(tok, x.cpu()[:, 1:].to(td).double().reshape(n * p, w)) and torch.equal(cls, x.cpu()[:, 0].to(td).double())
    d_tok, d_cls = _vals((n * p, w), 10, torch.float32).cuda(), _vals((n, w), 11, torch.float32).cuda()

    def join():
        out, b = _guard(shape, torch.float32)
        _call("pmi_dpt_tap_join", d_tok.data_ptr(), d_cls.data_ptr(), out.data_ptr(), n, t, w)
        return [out], [b]

    (out,) = _twice(join)
    assert torch.equal(out[:, 1:].reshape(n * p, w), d_tok.cpu().double()) and torch.equal(out[:, 0], d_cls.cpu().double())
    t16 = _vals((n, p, w), 12, td).cuda()

    def colsum():
        s, b = _guard((n, w), torch.float32)
        _call("pmi_dpt_colsum", t16.data_ptr(), s.data_ptr(), n, p, w, code)
        return [s], [b]

    (s,) = _twice(colsum)
    _hold(f"colsum {shape} {dtype}", s, t16.cpu().double().sum(1), (p + 3) // 4 * U * t16.cpu().double().abs().sum(1) + 2 * U * t16.cpu().double().abs().sum(1))
    a, b = _vals(shape, 13, torch.float32).cuda(), _vals(shape, 14, torch.float32).cuda()

    def add():
        o32, b0 = _guard(shape, torch.float32)
        o16, b1 = _guard(shape, td)
        _call("pmi_dpt_tap_add", a.data_ptr(), b.data_ptr(), o32.data_ptr(), o16.data_ptr(), n * t * w, code)
        return [o32, o16], [b0, b1]

    o32, o16 = _twice(add)
    assert torch.equal(o32, (a + b).cpu().double()) and torch.equal(o16, (a + b).cpu().to(td).double())


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n", [8, 4096 + 8])
@pytest.mark.parametrize("addend", [False, True])
def test_relu_bwd(n, dtype, addend):
    code, td = DT[dtype]
    g, y = _vals((n,), 15, td).cuda(), _vals((n,), 16, td, zeros=True).relu().cuda()
    r = _vals((n,), 17, td).cuda() if addend else None
    assert bool((y == 0).any()) and bool((y > 0).any())

    def run():
        dz, b = _guard((n,), td)
        _call("pmi_dpt_relu_bwd", g.data_ptr(), y.data_ptr(), r.data_ptr() if addend else None, dz.data_ptr(), n, code)
        return [dz], [b]

    (dz,) = _twice(run)
    ref = g.cpu().double() * (y.cpu() > 0) + (r.cpu().double() if addend else 0.0)
    _hold(f"relu_bwd {n} {dtype} addend={addend}", dz, ref, U * ref.abs() + 0.5 * ulp16(ref, dtype) * (1 + 2.0 ** -9))
    assert bool((dz[(y.cpu() == 0)] == (r.cpu().double()[(y.cpu() == 0)] if addend else 0.0)).all()), "the mask must be strictly > 0"


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("hw", [1, 63, 64, 65, 4096])
@pytest.mark.parametrize("n", [1, 2])
def test_head_fwd_bwd(n, hw, dtype):
    code, td = DT[dtype]
    P = n * hw
    h = _vals((P, 32), 18, td, zeros=True).relu().cuda()
    w = _vals((32,), 19, torch.float32).cuda()
    b = torch.tensor([0.1], device="cuda")

    def fwd():
        out, buf = _guard((P,), torch.float32)
        _call("pmi_dpt_head_fwd", h.data_ptr(), w.data_ptr(), b.data_ptr(), out.data_ptr(), P, code)
        return [out], [buf]

    (out,) = _twice(fwd)
    z = h.cpu().double() @ w.cpu().double() + 0.1
    A = h.cpu().double().abs() @ w.cpu().double().abs() + 0.1
    tol = 34 * U * A
    safe = z.abs() > tol                       # (the sign of z decides the branch: elements inside the bound of zero may take either)
    assert P < 4 or (bool((z[safe] > 0).any()) and bool((z[safe] < 0).any()))
    _hold(f"head_fwd N={n} HW={hw} {dtype}", out, -z.clamp_min(0), tol)
    dout = _vals((P,), 20, torch.float32).cuda()
    out_d = out.float().cuda()

    def bwd():
        dh, buf = _guard((P, 32), td)
        _call("pmi_dpt_head_bwd", dout.data_ptr(), out_d.data_ptr(), h.data_ptr(), w.data_ptr(), dh.data_ptr(), P, 4.0, code)
        return [dh], [buf]

    (dh,) = _twice(bwd)
    ref = (-4.0 * dout.cpu().double() * (out < 0))[:, None] * w.cpu().double()[None, :] * (h.cpu() > 0)
    _hold(f"head_bwd N={n} HW={hw} {dtype}", dh, ref, 3 * U * ref.abs() + 0.5 * ulp16(ref, dtype) * (1 + 2.0 ** -9))


# ---- B. VitEngine with the timm options --------------------------------------------------------------------------------------------------
def _tower(dtype):
    from perceptor_amd.engine.vit import VitEngine, from_timm_vit_state_dict
    cfg, sd, images = D.toy("a")
    eng = VitEngine(cfg[:5] + (0,), from_timm_vit_state_dict(sd, "pretrained.model."), "cuda", dtype, quick_gelu=False, ln_eps=1e-6, pre_ln=False,
                    pooled_head=False, norm=((0.5,) * 3, (0.5,) * 3))
    return cfg, sd, images, eng


# the whole-tower gates of tests/test_gpu_vit_tower.py: rel-L2 <= sqrt(k) u against the emulated tower, k the 16-bit roundings on the longest
# path (the K_* counts of tests/_vit_ref64.py: 1 for the stem, 4 + 3 per block; the gradient adds its own), u = 2^-8 (bf16) / 2^-11 (f16)
UNIT = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_vit_taps_and_backward_taps(dtype):
    cfg, sd, images, eng = _tower(dtype)
    x = images.cuda()
    emb, taps = eng.forward(x, save=True, taps=cfg[5])
    assert emb is None and len(taps) == 4
    import _vit_ref64 as V
    with torch.no_grad():
        ref = D.Dpt64(sd, cfg, emulate=DT[dtype][1]).tower(images.double())
    for k in range(4):
        r, gate = V.rel_l2(taps[k].cpu(), ref[k]), (V.K_STEM_FWD + (cfg[5][k] + 1) * (V.K_ATTN_FWD + V.K_MLP_FWD)) ** 0.5 * UNIT[dtype]
        print(f"[bound] tap {k} {dtype}: rel-L2 {r:.3e} (gate {gate:.2e})")
        assert r <= gate
    g = torch.Generator().manual_seed(3)
    # gradients of the size a guidance run hands in (2^-14, the small probe of tests/test_gpu_vit_tower.py): times gscale they fit f16
    d = [torch.randn(taps[0].shape, generator=g).cuda() * (2.0 ** -14 * eng.gscale) for _ in range(4)]
    saved = eng.saved
    all4 = eng.backward_taps(d)
    # one tap at the last block is backward_tokens, bit for bit
    eng.forward(x, save=True, taps=(cfg[5][3],))
    one = eng.backward_taps([d[3]])
    eng.forward(x, save=True)
    tok = eng.backward_tokens(d[3])
    assert bool(torch.isfinite(tok).all()) and float(tok.abs().max()) > 0 and torch.equal(one, tok)
    # four taps together = the sum of four single-tap runs (the walk is linear in the gradients)
    total = one.double()
    for k in range(3):
        eng.forward(x, save=True, taps=(cfg[5][k],))
        total = total + eng.backward_taps([d[k]]).double()
    r, gate = V.rel_l2(all4.cpu(), total.cpu()), V.depth_grad(cfg[3], True) ** 0.5 * UNIT[dtype]
    print(f"[bound] four taps vs sum of single-tap runs {dtype}: rel-L2 {r:.3e} (gate {gate:.2e})")
    assert r <= gate and saved is not None


# ---- C. DptEngine and the class against the restatement -------------------------------------------------------------------------------------
_runs = {}


def _engine_run(name, dtype):
    if (name, dtype) not in _runs:
        from perceptor_amd.engine.dpt import DptEngine
        cfg, sd, images = D.toy(name)
        eng = DptEngine(cfg, sd, "cuda", dtype)
        out, grads, masks = None, {}, None
        for kind in ("mean", "rand"):
            rec = {}
            out = eng.forward(images.cuda(), save=True)
            grads[kind] = eng.backward((D.upstream(name, kind).float() * eng.gscale).cuda(), record=rec).cpu()
            masks = D.engine_masks(rec["masks"])
        _runs[(name, dtype)] = (out.cpu(), grads, masks)
    return _runs[(name, dtype)]


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_engine_against_restatement(name, dtype):
    cfg, sd, images = D.toy(name)
    out, grads, masks = _engine_run(name, dtype)
    free = D.free_run(name)
    M = MEASURED[(name, dtype)]
    r = D.rel(out, free["depth"])
    print(f"[bound] depth {name} {dtype}: {r:.3e} (gate {2 * M['depth']:.2e})")
    assert r <= 2 * M["depth"]
    # the output mask agrees with float64 outside the band where the emulated run's own error could flip it
    z = free["z"]
    outside = z.abs() > 8 * M["z_err"]
    assert float(outside.double().mean()) >= 0.98                     # (the fixtures keep the band under 2 % of the pixels)
    print(f"[bound] z band {name} {dtype}: {1 - float(outside.double().mean()):.3f} of the pixels lie inside 8 x {M['z_err']:.2e}")
    assert bool(((out < 0) == (z > 0))[outside].all()), "an output ReLU decision differs from float64 outside the z band"
    for kind in ("mean", "rand"):
        gx, _ = D.image_grad(D.Dpt64(sd, cfg), images, D.upstream(name, kind), masks=masks)
        r = D.rel(grads[kind], gx)
        print(f"[bound] d {kind} / d images {name} {dtype}: {r:.3e} (gate {2 * M['grad_' + kind]:.2e})")
        assert r <= 2 * M["grad_" + kind]
        assert tuple(grads[kind].shape) == tuple(images.shape)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("defect", D.DEFECTS)
def test_engine_is_far_from_every_defect(defect, dtype):
    name = D.DEFECT_CONFIG.get(defect, "b")
    cfg, sd, images = D.toy(name)
    out, grads, masks = _engine_run(name, dtype)
    M = MEASURED[(name, dtype)]
    if defect == "tap_grad_not_injected":
        gx, _ = D.image_grad(D.Dpt64(sd, cfg, defect=defect), images, D.upstream(name, "rand"), masks=masks)
        r, gate = D.rel(grads["rand"], gx), 2 * M["grad_rand"]
    else:
        with torch.no_grad():
            bad = D.Dpt64(sd, cfg, defect=defect).forward(images.double())
        r, gate = D.rel(out, bad["depth"]), 2 * M["depth"]
    print(f"[bound] defect {defect} ({name}, {dtype}): engine is {r / gate:.1f} gates away")
    assert r > 2 * gate


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_class_backward_fills_images_grad(dtype):
    from perceptor_amd import models
    cfg, sd, images = D.toy("b")
    m = models.MidasDepth(config=cfg, dtype=dtype)
    m.model.load_state_dict(sd)
    m = m.to("cuda")
    x = images.cuda().requires_grad_(True)
    depths = m(x)
    assert tuple(depths.shape) == (2, 1, cfg[0], cfg[0]) and depths.dtype == torch.float32
    depths.mean().backward()
    out, grads, _ = _engine_run("b", dtype)
    assert torch.equal(depths.detach().cpu(), out)
    assert x.grad is not None and tuple(x.grad.shape) == tuple(images.shape)
    assert D.rel(x.grad, grads["mean"]) <= 1e-6                       # the same engine calls; the upstream value 1 / (N R^2) made by autograd
    with torch.no_grad():
        assert torch.equal(m(images.cuda()).cpu(), out)


# ---- D. product configuration ------------------------------------------------------------------------------------------------------------------
def test_product_configuration():
    from perceptor_amd import models
    m = models.MidasDepth().to("cuda")
    g = torch.Generator().manual_seed(0)
    x = torch.rand((1, 3, 256, 320), generator=g).cuda().requires_grad_(True)
    depths = m(x)
    assert tuple(depths.shape) == (1, 1, 384, 384) and depths.dtype == torch.float32
    assert bool(torch.isfinite(depths).all()) and float(depths.abs().max()) > 0
    depths.mean().backward()
    assert tuple(x.grad.shape) == (1, 3, 256, 320) and bool(torch.isfinite(x.grad).all()) and float(x.grad.abs().max()) > 0
