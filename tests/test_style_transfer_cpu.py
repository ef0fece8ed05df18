"""CPU: the float64 restatement of the VGG-19 tower and the style-transfer loss (tests/_vgg_ref64.py) against the reference's own
values (tests/golden/style_transfer_reference.npz, written by tools/gen_style_transfer_golden.py from the reference's code), the layer
and slice table, the state-dict key mapping and the refusals of the public classes, the sign-band condition on the Gram test inputs,
and seeded defects: each must exceed 2x the bound the GPU test (tests/test_gpu_style_transfer.py) holds the product to, at exactly
that test's inputs -- a bound a plausible mistake passes would show nothing.
"""
import pytest
import torch
import torch.nn.functional as F

import _vgg_ref64 as R
from conftest import golden


def _sd(widths, seed=0):
    from perceptor_amd.engine.vgg import vgg_state_dict_shapes
    from perceptor_amd.utils.synth import synth_state_dict
    return synth_state_dict(vgg_state_dict_shapes(widths), seed, gain=2 ** 0.5)


# ---- the restatement equals the reference -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["same", "resized"])
def test_restatement_equals_reference_fixture(case):
    g = golden("style_transfer_reference")
    widths, size = tuple(int(v) for v in g["widths"]), int(g["size"])
    val, ga, gb, enc, grams = R.loss_and_grads(_sd(widths, int(g["seed"])), widths, size, g[case + "_a"], g[case + "_b"])
    ref = float(g[case + "_loss"])
    assert abs(float(val) - ref) <= 2.0 ** -23 * abs(ref)
    for i, G in zip((2, 3, 4), grams):
        want = g[f"{case}_gram{i}"]
        assert G.shape == want.shape and float((G - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max())
    for got, name in ((ga, "_grad_a"), (gb, "_grad_b")):
        want = g[case + name]
        assert got.shape == want.shape
        assert float(F.cosine_similarity(got.flatten(), want.flatten(), dim=0)) >= 1 - 1e-9
        assert float((got - want).norm() / want.norm()) <= 1e-6
    for i, e in enumerate(enc):
        assert tuple(e.shape) == tuple(int(v) for v in g[f"{case}_enc{i}_shape"])
        mom = torch.stack([e.mean(), e.abs().mean(), e.square().mean().sqrt(), e.max()])
        assert torch.allclose(mom, g[f"{case}_enc{i}_moments"], rtol=1e-6, atol=0)
        assert torch.allclose(e.flatten()[::37][:256], g[f"{case}_enc{i}_slice"], rtol=1e-6, atol=1e-9)


# ---- tables -----------------------------------------------------------------------------------------------------------------------------
def test_layer_and_slice_table():
    from perceptor_amd.engine import vgg
    table = vgg.layer_table()
    assert len(table) == 37 and table == R.layer_table(vgg.VGG19_CONFIG[0])
    assert [i for i, l in enumerate(table) if l[0] == "conv"] == [0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34]
    assert [i for i, l in enumerate(table) if l[0] == "pool"] == [4, 9, 18, 27, 36]
    assert all(table[i + 1] == ("relu",) for i, l in enumerate(table) if l[0] == "conv")
    assert vgg.SLICES == R.SLICES == ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))
    # the last module of each slice is a ReLU; name it by (group, position in the group)
    names = []
    for _, end in vgg.SLICES:
        assert table[end - 1] == ("relu",) and table[end - 2][0] == "conv"
        convs = [i for i, l in enumerate(table[:end]) if l[0] == "conv"]
        group = sum(1 for l in table[:end] if l[0] == "pool") + 1
        first = [i for i in convs if sum(1 for l in table[:i] if l[0] == "pool") == group - 1][0]
        names.append(f"relu{group}_{convs.index(end - 2) - convs.index(first) + 1}")
    assert names == ["relu1_2", "relu2_2", "relu3_3", "relu4_2", "relu5_1"]
    assert list(vgg.LEVEL_WEIGHTS.items()) == [(7, 5.0), (14, 15.0), (21, 2.0)] == [tuple(l) for l in R.LEVELS]
    assert [end - 2 for _, end in vgg.SLICES[1:4]] == list(vgg.LEVEL_WEIGHTS) and vgg.LOSS_LAST == 22
    assert [(l[1], l[2]) for l in table if l[0] == "conv"][:5] == [(3, 64), (64, 64), (64, 128), (128, 128), (128, 256)]
    # relu2_2 IS followed directly by a pool (module 9): its adjoint enters the level gradient as g_in
    assert table[9] == ("pool",) and table[16][0] == "conv" and table[23][0] == "conv"


def test_state_dict_key_mapping_and_refusals():
    from perceptor_amd import losses, models
    from perceptor_amd.engine import vgg
    widths = (16, 16, 32, 32, 32)
    sd = _sd(widths)
    assert set(sd) == {f"{i}.{leaf}" for i in vgg.conv_indices(widths) for leaf in ("weight", "bias")}
    pref = {"features." + k: v for k, v in sd.items()}
    pref["classifier.0.weight"] = torch.zeros(4, 4)
    mapped = vgg.map_state_dict(pref, widths)
    assert set(mapped) == set(sd) and all(mapped[k] is sd[k] for k in sd)
    with pytest.raises(ValueError, match="missing"):
        vgg.map_state_dict({k: v for k, v in sd.items() if k != "7.bias"}, widths)
    with pytest.raises(ValueError, match="shape"):
        vgg.map_state_dict({**sd, "0.weight": torch.zeros(16, 3, 1, 1)}, widths)
    for cfg in (((16, 16, 32, 32, 30), 32), ((16, 16, 32, 32), 32), (widths, 48), (widths, 0)):
        with pytest.raises(ValueError):
            vgg.VggEngine(cfg, sd, "cpu")
    with pytest.raises(ValueError):
        vgg.VggEngine((widths, 32), sd, "cpu", dtype="precise")
    m = models.VGG19(widths=widths, size=32)
    assert set(m.state_dict()) == set(pref) - {"classifier.0.weight"}
    assert all(torch.equal(m.state_dict()["features." + k], sd[k]) for k in sd)
    x = torch.rand(2, 3, 32, 32)
    with pytest.raises(RuntimeError):
        m(x)
    st = losses.StyleTransfer(widths=widths, size=32)
    with pytest.raises(AttributeError):
        st(x)
    with pytest.raises(AttributeError):
        st.loss_and_grad(x)
    with pytest.raises(RuntimeError):
        st.loss_and_grad(x, x)
    with pytest.raises(ValueError):
        losses.StyleTransfer(weights="imagenet")


# ---- the sign band: a condition on the inputs -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", R.GRAM_SHAPES)
def test_sign_band_share_of_gram_inputs(shape, dtype):
    n, hw, c = shape
    fa, fb = R.gram_inputs(shape, R.DTYPES[dtype])
    scale = 1.0 / (float(n * c) * hw)
    g64 = R.gram(R.nchw(fa, n, hw, c)) - R.gram(R.nchw(fb, n, hw, c))
    inside = g64.abs() <= R.gram_bound(fa, scale) + R.gram_bound(fb, scale)
    share = float(inside.double().mean())
    print(f"[band] {shape} {dtype}: {share:.4%} of Ga - Gb inside the fp32 band")
    assert share <= 0.02


# ---- seeded defects at the GPU test's inputs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", [s for s in R.GRAM_SHAPES if s[0] > 1])
def test_defects_gram(shape, dtype):
    """Normalising per sample, and dropping the cross-sample blocks (both only exist for N > 1)."""
    n, hw, c = shape
    fa, _ = R.gram_inputs(shape, R.DTYPES[dtype])
    f = R.nchw(fa, n, hw, c)
    ref, bound = R.gram(f), R.gram_bound(fa, 1.0 / (float(n * c) * hw))
    for kw in (dict(per_sample=True), dict(drop_cross=True)):
        worst = float(((R.gram(f, **kw) - ref).abs() / bound).max())
        print(f"[defect] gram {kw} {shape} {dtype}: {worst:.3e} x bound")
        assert worst > 2.0


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", R.GRAM_SHAPES)
def test_defect_gram_bwd_without_transpose(shape, dtype):
    n, hw, c = shape
    dt = R.DTYPES[dtype]
    fa, fb = R.gram_inputs(shape, dt)
    S = torch.sign(R.gram(R.nchw(fa, n, hw, c)) - R.gram(R.nchw(fb, n, hw, c)))
    c_feat, c_gram = R.level_coefs(n, hw, c, 15.0)
    for gscale in (1.0, 65536.0):
        ref, bound = R.gram_bwd_ref(fa, fb, S, None, c_feat, c_gram, gscale, dt)
        bad, _ = R.gram_bwd_ref(fa, fb, S, None, c_feat, c_gram, gscale, dt, transpose=False)
        worst = float(((bad - ref).abs() / bound).max())
        print(f"[defect] gram_bwd S without S^T {shape} {dtype} gscale={gscale:g}: {worst:.3e} x bound")
        assert worst > 2.0


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", R.POOL_SHAPES)
def test_defects_pool_adjoint(shape, dtype):
    """The bound is zero (the GPU test is bit-exact): the last-maximum route and the missing ReLU mask must change some element."""
    x, dy = R.pool_inputs(shape, R.DTYPES[dtype])
    xn, dyn = x.permute(0, 3, 1, 2).double(), dy.permute(0, 3, 1, 2).double()
    ref = R.pool_adjoint(dyn, xn)
    assert not torch.equal(R.pool_adjoint(dyn, xn, route_fn=R.last_max_route), ref)
    assert not torch.equal(R.pool_adjoint(dyn, xn, mask=False), ref)


@pytest.fixture(scope="module")
def engine_features():
    out = {}
    for name, (widths, size, n) in R.ENGINE_CONFIGS.items():
        sd = _sd(widths)
        a, b = R.engine_inputs(name)
        for dtype, dt in R.DTYPES.items():
            out[(name, dtype)] = (R.tower(sd, widths, a, emulate=dt), R.tower(sd, widths, b, emulate=dt))
    return out


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name", list(R.ENGINE_CONFIGS))
def test_defects_loss(engine_features, name, dtype):
    """A missing 0.001, w_l instead of w_l^2 on the Gram term and the two Gram defects against the loss bound; level 4 taken at relu4_1
    against the feature gate of relu4_2 (the loss of wrong-level features is consistent with those features: the feature check is what
    sees it)."""
    ta, tb = engine_features[(name, dtype)]
    u = R.UNIT[R.DTYPES[dtype]]
    ea, eb = R.level_features(ta), R.level_features(tb)
    ref, bound = float(R.loss(ea, eb)), R.loss_kernel_bound(ea, eb) + R.loss_feature_bound(ea, eb, u)
    bad = {"no 0.001": R.loss(ea, eb, scale=1.0), "w instead of w^2": R.loss(ea, eb, gram_pow=1),
           "gram per sample": R.loss(ea, eb, per_sample=True), "no cross-sample blocks": R.loss(ea, eb, drop_cross=True)}
    for tag, val in bad.items():
        ratio = abs(float(val) - ref) / bound
        print(f"[defect] loss {name} {dtype} {tag}: {ratio:.3e} x bound")
        assert ratio > 2.0, tag
    for t in (ta, tb):
        rel = float((t[19] - t[21]).norm() / t[21].norm()) / (R.FEATURE_ROUNDINGS[2] ** 0.5 * u)
        print(f"[defect] features {name} {dtype} relu4_1 for relu4_2: {rel:.3e} x gate")
        assert rel > 2.0
