"""GPU: the JPEG codec kernels (csrc/jpeg.hip) per element against tests/_jpeg_ref64.py with its bound K u sum|terms|, their bit-equality
and adjointness, and the drawers.JPEG / drawers.Raw classes against the reference's own values (tests/golden/drawers_reference.npz).

Shapes (N, H, W): one macroblock; 2 x 1 and 1 x 2 macroblocks (H / W and block order); (3, 32, 48) batch stride and several macroblocks
on both axes; (1, 16, 80): five macroblocks across where a workgroup covers four side by side -- one full workgroup and one with a single
live wave.  (3, 32, 48) has three across, a short workgroup alone.  Factors 1 and 2.5.  No element is left out of a comparison: the seeded
inputs (J.SEEDS) keep the float64 values away from clamp edges and rounding ties by more than the bound, and that is asserted first.
"""
import functools

import pytest
import torch

import _jpeg_ref64 as J
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ("y", "cb", "cr")
CASES = [(s, f) for s in J.SHAPES for f in J.FACTORS]
RESIZE_SEED = 25     # of the 24 x 40 image of the encode-with-resize test: its resized quotients keep clear of rounding ties (asserted there)


def _name(shape, factor):
    return "n%d_%dx%d_f%s" % (*shape, str(factor).replace(".", "p"))


def _E():
    from perceptor_amd.engine import jpeg
    return jpeg


def _dev(ts):
    return [t.to(DEV) for t in ts]


@functools.lru_cache(maxsize=None)
def _gold():
    return golden("drawers_reference")


@functools.lru_cache(maxsize=None)
def _case(shape, factor):
    """float64 reference of one decode case, computed once and shared (never modified)"""
    n, h, w = shape
    coef, wts = J.noisy_coefficients(shape, factor), J.weights(shape)
    dec, decs, pre, prea = J.decode(*coef, h, w, factor)
    adj, adjs = J.decode_adjoint(*coef, wts, factor)
    return dict(coef=coef, w=wts, dec=dec, decs=decs, pre=pre, prea=prea, adj=adj, adjs=adjs)


@functools.lru_cache(maxsize=None)
def _enc_case(shape, factor):
    img = J.image(shape, factor)
    rounded, sums, q = J.encode(img, factor, True)
    return dict(img=img, rounded=rounded, sums=sums, q=q)


@pytest.mark.parametrize("shape,factor", CASES)
def test_decode_and_adjoint_per_element(shape, factor):
    n, h, w = shape
    c = _case(shape, factor)
    # preconditions on the float64 reference alone: the clamp works on both sides, and no fp32 result can take another clamp decision
    margin = J.clamp_margin(c["pre"])
    assert bool((margin > J.tol(c["prea"])).all()), float((margin / J.tol(c["prea"])).min())
    assert float((c["pre"] < 0).double().mean()) > 0.05 and float((c["pre"] > 255).double().mean()) > 0.05
    coef = _dev(c["coef"])
    out = _E().jpeg_decode(*coef, h, w, factor).cpu()
    print(f"decode {shape} f={factor}: worst error / bound {J.worst(out, c['dec'], J.tol(c['decs'])):.3f}")
    assert J.within(out, c["dec"], J.tol(c["decs"]))
    grads = _E().jpeg_decode_backward(*coef, c["w"].to(DEV), factor)
    for k in range(3):
        g = grads[k].cpu()
        print(f"adjoint d_{NAMES[k]} {shape} f={factor}: worst error / bound {J.worst(g, c['adj'][k], J.tol(c['adjs'][k])):.3f}")
        assert J.within(g, c["adj"][k], J.tol(c["adjs"][k])), NAMES[k]


@pytest.mark.parametrize("shape,factor", CASES)
def test_encode_unrounded_per_element(shape, factor):
    e = _enc_case(shape, factor)
    got = _E().jpeg_encode(e["img"].to(DEV), factor, rounding=False)
    for k in range(3):
        g = got[k].cpu()
        print(f"encode {NAMES[k]} {shape} f={factor}: worst error / bound {J.worst(g, e['q'][k], J.tol(e['sums'][k])):.3f}")
        assert J.within(g, e["q"][k], J.tol(e["sums"][k])), NAMES[k]


@pytest.mark.parametrize("shape,factor", CASES)
def test_encode_rounded_per_element(shape, factor):
    e = _enc_case(shape, factor)
    for k in range(3):          # no quotient near a tie, and the fp32 quotient cannot cross one
        m = J.half_margin(e["q"][k])
        assert float(m.min()) >= 1e-4 and bool((J.tol(e["sums"][k]) < m).all())
    got = _E().jpeg_encode(e["img"].to(DEV), factor)
    for k in range(3):
        g = got[k].cpu()
        print(f"encode+round {NAMES[k]} {shape} f={factor}: worst error / bound {J.worst(g, e['rounded'][k], J.tol(e['sums'][k], 1.75)):.3f}")
        assert J.within(g, e["rounded"][k], J.tol(e["sums"][k], 1.75)), NAMES[k]


@pytest.mark.parametrize("shape,factor", [((3, 32, 48), 2.5), ((1, 16, 80), 1.0)])
def test_bit_equality(shape, factor):
    E = _E()
    n, h, w = shape
    c = _case(shape, factor)
    coef, wts, img = _dev(c["coef"]), c["w"].to(DEV), J.image(shape, factor).to(DEV)
    out = E.jpeg_decode(*coef, h, w, factor)
    assert torch.equal(out, E.jpeg_decode(*coef, h, w, factor))
    full = E.jpeg_decode_backward(*coef, wts, factor)
    again = E.jpeg_decode_backward(*coef, wts, factor)
    enc, enc2 = E.jpeg_encode(img, factor), E.jpeg_encode(img, factor)
    for k in range(3):
        assert torch.equal(full[k], again[k]) and torch.equal(enc[k], enc2[k])
    # sample 0 alone against sample 0 of the batch
    one = [t[:1].contiguous() for t in coef]
    assert torch.equal(E.jpeg_decode(*one, h, w, factor), out[:1])
    alone = E.jpeg_decode_backward(*one, wts[:1].contiguous(), factor)
    enc_one = E.jpeg_encode(img[:1].contiguous(), factor)
    for k in range(3):
        assert torch.equal(alone[k], full[k][:1]) and torch.equal(enc_one[k], enc[k][:1])
    # every mask of wanted gradients gives the bits of the full call, and None elsewhere
    for mask in ((True, False, False), (False, True, False), (False, False, True), (True, False, True), (False, True, True)):
        part = E.jpeg_decode_backward(*coef, wts, factor, need=mask)
        for k in range(3):
            assert (part[k] is None) if not mask[k] else torch.equal(part[k], full[k])
    assert E.jpeg_decode_backward(*coef, wts, factor, need=(False, False, False)) == (None, None, None)


@pytest.mark.parametrize("shape,factor", [((2, 32, 16), 1.0), ((3, 32, 48), 2.5)])
def test_adjointness_unclamped(shape, factor):
    """<decode(c) - decode(0), g> = <c, decode_bwd(g)> for the unclamped (affine) map, each side from fp32 results summed in float64"""
    E = _E()
    n, h, w = shape
    gen = torch.Generator().manual_seed(31)
    coef = [(0.05 * torch.randn(t.shape, generator=gen)).float() for t in _case(shape, factor)["coef"]]
    zero = [torch.zeros_like(t) for t in coef]
    g = J.weights(shape)
    _, decs, pre, _ = J.decode(*coef, h, w, factor)
    _, decs0, pre0, _ = J.decode(*zero, h, w, factor)
    assert float(J.clamp_margin(pre).min()) > 1.0 and float(J.clamp_margin(pre0).min()) > 1.0          # nothing clamps
    _, adjs = J.decode_adjoint(*coef, g, factor)
    d1, d0 = E.jpeg_decode(*_dev(coef), h, w, factor).cpu().double(), E.jpeg_decode(*_dev(zero), h, w, factor).cpu().double()
    back = E.jpeg_decode_backward(*_dev(coef), g.to(DEV), factor)
    lhs = float(((d1 - d0) * g.double()).sum())
    rhs = float(sum((c.double() * b.cpu().double()).sum() for c, b in zip(coef, back)))
    bound = float(((J.tol(decs) + J.tol(decs0)) * g.double().abs()).sum()) + float(sum((J.tol(a) * c.double().abs()).sum() for a, c in zip(adjs, coef)))
    print(f"adjointness {shape} f={factor}: lhs {lhs:.9g} rhs {rhs:.9g} |diff| / bound {abs(lhs - rhs) / bound:.4f}")
    assert abs(lhs - rhs) <= bound


def test_entry_points_refuse_bad_arguments_and_match_the_wrappers():
    """pmi_jpeg_decode / pmi_jpeg_decode_bwd / pmi_jpeg_encode called by name: every refusal returns PMI_ERR_ARG (-1) before any launch and
    leaves the output untouched; a direct call gives the wrapper's bits."""
    from perceptor_amd import _hip
    lib, E = _hip.lib(), _E()
    shape, factor = (2, 16, 32), 2.5
    n, h, w = shape
    c = _case(shape, factor)
    y, cb, cr = _dev(c["coef"])
    g = c["w"].to(DEV)
    st = _hip.stream_ptr()
    out = torch.full((n, 3, h, w), -7.0, device=DEV)
    P = lambda t: t.data_ptr()
    bad = [(P(y), P(cb), P(cr), factor, P(out), n, h, w + 8), (P(y), P(cb), P(cr), factor, P(out), n, h + 8, w), (P(y), P(cb), P(cr), factor, P(out), 0, h, w),
           (None, P(cb), P(cr), factor, P(out), n, h, w), (P(y), P(cb), P(cr), factor, None, n, h, w), (P(y) + 4, P(cb), P(cr), factor, P(out), n, h, w),
           (P(y), P(cb), P(cr), 0.0, P(out), n, h, w), (P(y), P(cb), P(cr), -1.0, P(out), n, h, w), (P(y), P(cb), P(cr), float("inf"), P(out), n, h, w),
           (P(y), P(cb), P(cr), float("nan"), P(out), n, h, w)]
    for args in bad:
        assert lib.pmi_jpeg_decode(*args, st) == -1, args[3:]
    d = [torch.full_like(t, -7.0) for t in (y, cb, cr)]
    assert lib.pmi_jpeg_decode_bwd(P(y), P(cb), P(cr), factor, P(g), P(d[0]), P(d[1]), P(d[2]), n, h, w + 8, st) == -1
    assert lib.pmi_jpeg_decode_bwd(P(y), P(cb), P(cr), factor, None, P(d[0]), P(d[1]), P(d[2]), n, h, w, st) == -1
    assert lib.pmi_jpeg_decode_bwd(P(y), P(cb), P(cr), 0.0, P(g), P(d[0]), P(d[1]), P(d[2]), n, h, w, st) == -1
    assert lib.pmi_jpeg_decode_bwd(P(y), P(cb), P(cr), factor, P(g), P(d[0]) + 4, P(d[1]), P(d[2]), n, h, w, st) == -1
    assert lib.pmi_jpeg_decode_bwd(P(y), P(cb), P(cr), factor, P(g), None, None, None, n, h, w, st) == 0          # nothing wanted: no launch
    img = J.image(shape, factor).to(DEV)
    assert lib.pmi_jpeg_encode(P(img), factor, 2, P(d[0]), P(d[1]), P(d[2]), n, h, w, st) == -1
    assert lib.pmi_jpeg_encode(P(img), factor, 1, P(d[0]), P(d[1]), P(d[2]), n, h + 1, w, st) == -1
    assert lib.pmi_jpeg_encode(P(img), factor, 1, P(d[0]), None, P(d[2]), n, h, w, st) == -1
    torch.cuda.synchronize()
    assert float(out.min()) == -7.0 and float(out.max()) == -7.0 and all(float(t.min()) == -7.0 == float(t.max()) for t in d)
    assert lib.pmi_jpeg_decode(P(y), P(cb), P(cr), factor, P(out), n, h, w, st) == 0
    assert torch.equal(out, E.jpeg_decode(y, cb, cr, h, w, factor))
    assert lib.pmi_jpeg_decode_bwd(P(y), P(cb), P(cr), factor, P(g), P(d[0]), P(d[1]), P(d[2]), n, h, w, st) == 0
    back, want_back = [t.clone() for t in d], E.jpeg_decode_backward(y, cb, cr, g, factor)
    assert lib.pmi_jpeg_encode(P(img), factor, 1, P(d[0]), P(d[1]), P(d[2]), n, h, w, st) == 0
    want = E.jpeg_encode(img, factor)
    for k in range(3):
        assert torch.equal(back[k], want_back[k]) and torch.equal(d[k], want[k])


# ---- classes ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,factor", [((2, 16, 32), 2.5), ((3, 32, 48), 1.0)])
def test_jpeg_drawer_reproduces_reference(shape, factor):
    from perceptor_amd import drawers
    gold, name = _gold(), _name(shape, factor)
    n, h, w = shape
    img = gold[name + "_image"]
    e = _enc_case(shape, factor)
    assert torch.equal(img, e["img"])
    drawer = drawers.JPEG(img.to(DEV), factor=factor)
    assert tuple(drawer.shape) == (n, 3, h, w)
    sd = drawer.state_dict()
    assert list(sd) == ["ycbcr.0", "ycbcr.1", "ycbcr.2"]
    assert [tuple(v.shape) for v in sd.values()] == [(n, h * w // 64, 8, 8), (n, h * w // 256, 8, 8), (n, h * w // 256, 8, 8)]
    for k, c in enumerate(NAMES):
        # the reference rounds its DCT to fp32 before dividing (J.encode's dct_to_f32): one more rounding, u |quotient| <= u absum, scaled
        # like every other error of the quotient by the cubic rounding
        bound = J.tol(e["sums"][k], 1.75) + 1.75 * J.U * e["sums"][k]
        assert J.within(sd[f"ycbcr.{k}"].cpu(), gold[f"{name}_enc_{c}"], bound), c
    # the reference's perturbed coefficients through the state dict, its decode and its gradients
    coef = [gold[f"{name}_coef_{c}"] for c in NAMES]
    _, decs, pre, prea = J.decode(*coef, h, w, factor)
    assert bool((J.clamp_margin(pre) > J.tol(prea)).all())
    drawer.load_state_dict({f"ycbcr.{k}": coef[k] for k in range(3)})
    out = drawer()
    assert out.requires_grad and J.within(out.detach().cpu(), gold[name + "_dec"], J.tol(decs))
    assert torch.equal(out.detach(), drawer.synthesize().detach()) and torch.equal(out.detach(), drawer.decode(drawer.ycbcr).detach())
    wts = gold[name + "_w"]
    (out * wts.to(DEV)).sum().backward()
    _, adjs = J.decode_adjoint(*coef, wts, factor)
    for k, c in enumerate(NAMES):
        assert J.within(drawer.ycbcr[k].grad.cpu(), gold[f"{name}_grad_{c}"], J.tol(adjs[k])), c
    # needs_input_grad: a frozen tensor gets no gradient, the others the same bits
    for p in drawer.ycbcr:
        p.grad = None
    drawer.ycbcr[1].requires_grad_(False)
    full = _E().jpeg_decode_backward(*_dev(coef), wts.to(DEV), factor)
    (drawer() * wts.to(DEV)).sum().backward()
    assert drawer.ycbcr[1].grad is None and torch.equal(drawer.ycbcr[0].grad, full[0]) and torch.equal(drawer.ycbcr[2].grad, full[2])
    # an incoming gradient other than the weights alone: twice the loss, twice the gradient
    drawer.ycbcr[0].grad = None
    (2.0 * (drawer() * wts.to(DEV)).sum()).backward()
    assert torch.equal(drawer.ycbcr[0].grad, _E().jpeg_decode_backward(*_dev(coef), 2.0 * wts.to(DEV), factor)[0])


def test_jpeg_drawer_encode_resizes_first():
    from perceptor_amd import drawers
    shape, factor = (2, 16, 32), 2.5
    drawer = drawers.JPEG(J.image(shape, factor).to(DEV), factor=factor)
    other = torch.rand((2, 3, 24, 40), generator=torch.Generator().manual_seed(RESIZE_SEED)).to(DEV)
    got = drawer.encode(other)
    small = torch.nn.functional.interpolate(other, size=(16, 32), mode="bilinear")
    want = _E().jpeg_encode(small, factor)
    # The drawer's two 2-tap band passes and ATen's bilinear kernel round their weights and sums separately: per pixel at most 4 u |pixel|
    # apart (two weights, two sums), which reaches a quotient as at most 4 u absum -- four more roundings of the chain.  So the drawer is
    # held to the float64 encoding of ATen's image with K + 4 in place of K, away from rounding ties by more than that (asserted).
    _, sums, q = J.encode(small.cpu(), factor)
    k4 = (J.K + 4) / J.K
    for k in range(3):
        assert not got[k].requires_grad and got[k].shape == want[k].shape
        assert bool((J.tol(sums[k], k4) < J.half_margin(q[k])).all()), NAMES[k]
        assert J.within(got[k].cpu(), J.diff_round(q[k]), J.tol(sums[k], 1.75 * k4)), NAMES[k]
        assert J.within(want[k].cpu(), J.diff_round(q[k]), J.tol(sums[k], 1.75)), NAMES[k]
    same = drawer.encode(J.image(shape, factor).to(DEV))             # at the drawer's own size: no resize, the parameters' bits
    for k in range(3):
        assert torch.equal(same[k], drawer.ycbcr[k].detach())


def test_raw_drawer_and_bilinear_resize():
    from perceptor_amd import drawers, transforms
    gold = _gold()
    x = gold["resize_down_in"].to(DEV)
    raw = drawers.Raw(torch.zeros(2, 3, 16, 32, device=DEV))
    assert raw() is raw.images and raw.synthesize() is raw.images
    enc = raw.encode(x)
    assert tuple(enc.shape) == (2, 3, 16, 32)
    # two band passes of at most 6 taps with fp32 tables against the reference's float64 run: 1e-6 as on the host, plus fp32 sums
    assert float((enc.cpu().double() - gold["resize_down_out"]).abs().max()) <= 2e-6
    assert raw.replace_(enc) is raw and torch.equal(raw.images.detach(), enc)
    up = drawers.Raw(torch.zeros(2, 3, 32, 48, device=DEV)).encode(gold["resize_up_in"].to(DEV))
    assert float((up.cpu().double() - gold["resize_up_out"]).abs().max()) <= 2e-6
    assert torch.equal(raw.encode(x, mode="linear"), enc)
    # resize / resize_backward with the new method are adjoint
    g = torch.randn((2, 3, 16, 32), generator=torch.Generator().manual_seed(9)).to(DEV)
    back = transforms.resize_backward(g, (24, 40), resample="bilinear")
    assert tuple(back.shape) == (2, 3, 24, 40)
    lhs, rhs = float((enc.double() * g.double()).sum()), float((x.double() * back.double()).sum())
    scale = float((enc.double().abs() * g.double().abs()).sum())
    assert abs(lhs - rhs) <= 32 * J.U * scale, (lhs, rhs)              # two passes of <= 6 taps on each side: (6 + 1) u twice, both sides
    # the default rule is untouched: without resample= the pair plans lanczos3 here, another operator
    assert not torch.allclose(transforms.resize(x, (16, 32)), enc)


@pytest.mark.parametrize("kind", ["jpeg", "raw"])
def test_optimisation_lowers_the_loss(kind):
    from perceptor_amd import drawers, losses
    gen = torch.Generator().manual_seed(17)
    target = (0.25 + 0.5 * torch.rand((2, 3, 32, 48), generator=gen)).to(DEV)
    init = (0.25 + 0.5 * torch.rand((2, 3, 32, 48), generator=gen)).to(DEV)
    drawer = drawers.JPEG(init) if kind == "jpeg" else drawers.Raw(init.clone())
    opt = torch.optim.Adam(drawer.parameters(), lr=0.05 if kind == "jpeg" else 0.01)
    history = []
    for _ in range(20):
        opt.zero_grad()
        loss = torch.nn.functional.mse_loss(drawer(), target)
        loss.backward()
        for p in drawer.parameters():
            assert p.grad is not None and bool(torch.isfinite(p.grad).all())
        history.append(float(loss.detach()))
        opt.step()
    after = float(torch.nn.functional.mse_loss(drawer(), target).detach())
    print(f"{kind}: mse {history[0]:.6f} -> {after:.6f}")
    assert after < history[0]
    # one step of a package loss through the drawer
    for p in drawer.parameters():
        p.grad = None
    losses.Smoothness()(drawer()).backward()
    for p in drawer.parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0
