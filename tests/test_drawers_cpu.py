"""CPU: the float64 restatement of the JPEG codec (tests/_jpeg_ref64.py) against the reference's own float64 values
(tests/golden/drawers_reference.npz, tools/gen_drawers_golden.py), the bounds of tests/test_gpu_drawers.py against planted defects, the
"linear" resize method and the seeded Raw initialisers against the reference's outputs, and the host-side argument checks of the drawers."""
import numpy as np
import pytest
import torch

import _jpeg_ref64 as J
from conftest import golden

NAMES = ("y", "cb", "cr")
GOLDEN_CASES = [(s, f) for s in J.SHAPES[:3] for f in J.FACTORS] + [(J.SHAPES[3], 1.0)]      # what the fixture holds (its generator says why)
ALL_CASES = [(s, f) for s in J.SHAPES for f in J.FACTORS]


def _name(shape, factor):
    return "n%d_%dx%d_f%s" % (*shape, str(factor).replace(".", "p"))


@pytest.fixture(scope="module")
def gold():
    return golden("drawers_reference")


def _close64(a, b):
    """float64 round-off: a few hundred units in the last place of the larger operand"""
    return bool(((a - b).abs() <= 1e-12 * (1.0 + b.abs())).all())


@pytest.mark.parametrize("shape,factor", GOLDEN_CASES)
def test_ref64_matches_reference(gold, shape, factor):
    n, h, w = shape
    name = _name(shape, factor)
    img, wts = gold[name + "_image"], gold[name + "_w"]
    assert torch.equal(img, J.image(shape, factor)) and torch.equal(wts, J.weights(shape))
    enc, _, _ = J.encode(img, factor, rounding=True, dct_to_f32=True)
    encid, _, _ = J.encode(img, factor, rounding=False, dct_to_f32=True)
    coef = [gold[f"{name}_coef_{c}"] for c in NAMES]
    dec, _, _, _ = J.decode(*coef, h, w, factor)
    grads, _ = J.decode_adjoint(*coef, wts, factor)
    for k, c in enumerate(NAMES):
        assert _close64(enc[k], gold[f"{name}_enc_{c}"]), c
        assert _close64(encid[k], gold[f"{name}_encid_{c}"]), c
        assert _close64(grads[k], gold[f"{name}_grad_{c}"]), c
    assert _close64(dec, gold[name + "_dec"])
    # the clamp is live on both sides and the gradient is not trivially dense
    assert float((dec == 0).double().mean()) > 0.05 and float((dec == 1).double().mean()) > 0.05


def _observable(defect, shape, factor):
    return not (defect == "no_factor" and factor == 1.0)


@pytest.mark.parametrize("defect", [d for d in J.DEFECTS if d not in ("mask_ignored", "half_away")])
@pytest.mark.parametrize("shape,factor", ALL_CASES)
def test_bounds_reject_defects(defect, shape, factor):
    if not _observable(defect, shape, factor):
        # at factor 1 a missing factor changes nothing: the defective restatement must then AGREE (the switch does nothing else)
        coef = J.noisy_coefficients(shape, factor)
        assert torch.equal(J.decode(*coef, shape[1], shape[2], factor, defect)[0], J.decode(*coef, shape[1], shape[2], factor)[0])
        return
    n, h, w = shape
    coef, wts, img = J.noisy_coefficients(shape, factor), J.weights(shape), J.image(shape, factor)
    dec, decs, _, _ = J.decode(*coef, h, w, factor)
    assert not J.within(J.decode(*coef, h, w, factor, defect)[0], dec, J.tol(decs)), "decode"
    adj, adjs = J.decode_adjoint(*coef, wts, factor)
    bad, _ = J.decode_adjoint(*coef, wts, factor, defect)
    assert any(not J.within(bad[k], adj[k], J.tol(adjs[k])) for k in range(3)), "adjoint"
    for rounding, k_round in ((False, 1.0), (True, 1.75)):
        enc, encs, _ = J.encode(img, factor, rounding)
        bad, _, _ = J.encode(img, factor, rounding, defect)
        assert any(not J.within(bad[k], enc[k], J.tol(encs[k], k_round)) for k in range(3)), f"encode rounding={rounding}"


@pytest.mark.parametrize("shape,factor", ALL_CASES)
def test_bound_rejects_ignored_clamp_mask(shape, factor):
    coef, wts = J.noisy_coefficients(shape, factor), J.weights(shape)
    adj, adjs = J.decode_adjoint(*coef, wts, factor)
    bad, _ = J.decode_adjoint(*coef, wts, factor, "mask_ignored")
    for k in range(3):
        assert not J.within(bad[k], adj[k], J.tol(adjs[k])), NAMES[k]


def test_bound_rejects_half_away_rounding():
    """Half to even and half away from zero part only AT a tie, which no seeded image produces: the rule is tested on ties themselves,
    against the bound of a quotient of that size (absum >= |x|; here the smallest possible, |x| itself)."""
    ties = torch.tensor([0.5, 2.5, -0.5, -2.5, 4.5, -6.5], dtype=torch.float64)
    good, bad = J.diff_round(ties), J.diff_round(ties, "half_away")
    assert torch.equal(good, torch.tensor([0.125, 2.125, -0.125, -2.125, 4.125, -6.125], dtype=torch.float64))
    assert bool(((good - bad).abs() > J.tol(ties.abs(), 1.75)).all())
    odd = torch.tensor([1.5, -1.5, 3.5], dtype=torch.float64)          # ties whose even neighbour is the one away from zero: both rules agree
    assert torch.equal(J.diff_round(odd), J.diff_round(odd, "half_away"))
    assert torch.equal(J.diff_round(odd), torch.tensor([1.875, -1.875, 3.875], dtype=torch.float64))


def test_decode_is_linear_and_adjoint_in_float64():
    """<decode(c) - decode(0), g> = <c, adjoint(g)> where nothing clamps: the restatement's two halves agree with each other"""
    shape, factor = (2, 16, 32), 2.5
    n, h, w = shape
    g = torch.Generator().manual_seed(5)
    coef = [0.05 * torch.randn(s, generator=g, dtype=torch.float64) for s in ((n, 8, 8, 8), (n, 2, 8, 8), (n, 2, 8, 8))]
    zero = [torch.zeros_like(c) for c in coef]
    wts = J.weights(shape).double()
    dec, _, pre, _ = J.decode(*coef, h, w, factor)
    assert float(J.clamp_margin(pre).min()) > 1.0
    lhs = float(((dec - J.decode(*zero, h, w, factor)[0]) * wts).sum())
    adj, _ = J.decode_adjoint(*coef, wts, factor)
    rhs = float(sum((c * a).sum() for c, a in zip(coef, adj)))
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))


def test_torch_composition_matches_ref64():
    shape, factor = (2, 32, 16), 2.5
    coef = J.noisy_coefficients(shape, factor)
    got = J.TorchDecoder(shape[1], shape[2], factor, dtype=torch.float64)(*(c.double() for c in coef))
    assert _close64(got, J.decode(*coef, shape[1], shape[2], factor)[0])


# ---- transforms.resize: the "linear" / "bilinear" method ---------------------------------------------------------------------------------
def _dense(idx, w, in_sz):
    A = torch.zeros(idx.shape[0], in_sz, dtype=torch.float64)
    for j in range(idx.shape[0]):
        for t in range(idx.shape[1]):
            if int(idx[j, t]) >= 0:
                A[j, int(idx[j, t])] += float(w[j, t])
    return A


@pytest.mark.parametrize("tag,out_shape", [("down", (16, 32)), ("up", (32, 48))])
@pytest.mark.parametrize("resample", ["bilinear", "linear"])
def test_linear_band_tables_reproduce_resize_right(gold, tag, out_shape, resample):
    import importlib
    rz = importlib.import_module("perceptor_amd.transforms.resize")
    x, ref = gold[f"resize_{tag}_in"].double(), gold[f"resize_{tag}_out"]
    method, dims = rz._plan(x.shape[2], x.shape[3], out_shape, resample)
    assert method == "linear"
    for _, axis, i, o in dims:
        idx, w, idx_t, w_t = rz.band_tables(i, o, method)
        A = _dense(idx, w, i)
        assert torch.equal(_dense(idx_t, w_t, o), A.T)                       # the transposed band is the same operator
        x = torch.einsum("ji,nciw->ncjw", A, x) if axis == 2 else torch.einsum("ji,nchi->nchj", A, x)
    assert tuple(x.shape[2:]) == out_shape
    assert float((x - ref).abs().max()) <= 1e-6                              # fp32 tables against the reference's float64 run


def test_resize_defaults_unchanged_and_unknown_method_refused():
    import importlib
    rz = importlib.import_module("perceptor_amd.transforms.resize")
    assert rz._plan(32, 32, (16, 16))[0] == "lanczos3" and rz._plan(16, 16, (32, 32))[0] == "cubic"
    assert rz._plan(16, 16, (32, 32), "bicubic")[0] == "cubic"
    with pytest.raises(ValueError):
        rz._plan(16, 16, (32, 32), "box")


# ---- drawers.Raw initialisers --------------------------------------------------------------------------------------------------------------
def test_seeded_initialisers_reproduce_reference(gold):
    from perceptor_amd.drawers import Raw
    from perceptor_amd.drawers.init import fractal, gradient
    np.random.seed(11)
    f = fractal((1, 3, 24, 40))
    assert f.dtype == torch.float32 and float((f - gold["fractal_seed11_1x3x24x40"]).abs().max()) <= 1e-6
    np.random.seed(12)
    g = gradient((2, 3, 16, 24))
    assert g.dtype == torch.float32 and float((g - gold["gradient_seed12_2x3x16x24"]).abs().max()) <= 1e-6
    np.random.seed(11)
    r = Raw.random_fractal_image((1, 3, 24, 40))
    assert isinstance(r, Raw) and torch.equal(r.images.detach(), f) and r() is r.images
    np.random.seed(12)
    assert torch.equal(Raw.random_gradient_image((2, 3, 16, 24)).synthesize().detach(), g)
    with pytest.raises(ValueError):
        gradient((1, 4, 16, 16))
    with pytest.raises(ValueError):
        Raw.random_gradient_image((1, 1, 16, 16))


# ---- host-side checks ----------------------------------------------------------------------------------------------------------------------
def test_engine_refuses_cpu_tensors_and_bad_shapes():
    from perceptor_amd.engine import jpeg as E
    y, c = torch.zeros(1, 8, 8, 8), torch.zeros(1, 2, 8, 8)
    with pytest.raises(RuntimeError):
        E.jpeg_decode(y, c, c, 16, 32)
    with pytest.raises(RuntimeError):
        E.jpeg_decode_backward(y, c, c, torch.zeros(1, 3, 16, 32))
    with pytest.raises(RuntimeError):
        E.jpeg_encode(torch.zeros(1, 3, 16, 32))
    with pytest.raises(ValueError):
        E.jpeg_decode(y, c, c, 32, 16 + 8)                     # not a multiple of 16
    with pytest.raises(ValueError):
        E.jpeg_decode(y, c, c, 32, 32)                         # block counts of another size
    with pytest.raises(ValueError):
        E.jpeg_decode(y, c, torch.zeros(1, 3, 8, 8), 16, 32)
    with pytest.raises(ValueError):
        E.jpeg_decode_backward(y, c, c, torch.zeros(1, 3, 32, 32))
    with pytest.raises(ValueError):
        E.jpeg_decode_backward(y, c, c, torch.zeros(2, 3, 16, 32))
    with pytest.raises(ValueError):
        E.jpeg_encode(torch.zeros(1, 3, 24, 32))
    with pytest.raises(ValueError):
        E.jpeg_encode(torch.zeros(1, 1, 16, 32))
    with pytest.raises(ValueError):
        E.jpeg_encode(torch.zeros(1, 3, 16, 32), factor=0.0)


def test_drawer_classes_on_the_host():
    import perceptor_amd
    from perceptor_amd import drawers
    assert perceptor_amd.drawers is drawers
    d = drawers.DrawingInterface()
    for call in (d, d.synthesize, d.encode, d.replace_):
        with pytest.raises(NotImplementedError):
            call()
    with pytest.raises(ValueError):
        drawers.JPEG(torch.zeros(1, 3, 32, 32))                # not on the HIP device
    raw = drawers.Raw(torch.zeros(1, 3, 8, 12))
    assert [k for k, _ in raw.named_parameters()] == ["images"]
    assert raw.replace_(torch.ones(1, 3, 8, 12)) is raw and float(raw.images.detach().min()) == 1.0
    with pytest.raises(RuntimeError):
        raw.encode(torch.zeros(1, 3, 16, 24))                  # the resize runs on the device only
    with pytest.raises(NotImplementedError):
        drawers.JPEG.replace_(raw)
