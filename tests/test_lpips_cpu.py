"""CPU: the LPIPS layer table, the float64 restatement of tests/_lpips_ref64.py against an independent plain torch.nn module built as the
lpips package builds its own, the state-dict layout of losses.LPIPS, its errors, and the bounds of csrc/lpips.hip's kernels: an fp32
evaluation in another summation order stays inside them, and each seeded defect leaves them by more than a factor 2 at the inputs
tests/test_gpu_lpips.py uses."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch import nn

import _lpips_ref64 as R


# ================================================ layer table ============================================================================
def test_layer_table_and_taps():
    from perceptor_amd.engine import lpips as E
    from perceptor_amd.engine import vgg
    table = E.lpips_layer_table()
    assert len(table) == 30 and table == R.layer_table(R.WIDTHS)
    assert [i for i, l in enumerate(table) if l[0] == "conv"] == [0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28]
    assert [i for i, l in enumerate(table) if l[0] == "pool"] == [4, 9, 16, 23]
    assert E.TAPS == (2, 7, 14, 21, 28) and E.LAST == 29
    assert E.tap_names() == {2: "relu1_2", 7: "relu2_2", 14: "relu3_3", 21: "relu4_3", 28: "relu5_3"}
    assert [table[c][2] for c in E.TAPS] == [64, 128, 256, 512, 512]
    assert all(table[c + 1] == ("relu",) for c in E.TAPS)
    # VGG-19's table is what it was
    assert vgg.conv_indices() == [0, 2, 5, 7, 10, 12, 14, 16, 19, 21, 23, 25, 28, 30, 32, 34] and len(vgg.layer_table()) == 37


# ================================================ restatement vs an independent module ===================================================
class _PkgScaling(nn.Module):
    def __init__(self):
        super().__init__()
        self.register_buffer("shift", torch.tensor([-.030, -.088, -.188], dtype=torch.float64)[None, :, None, None])
        self.register_buffer("scale", torch.tensor([.458, .448, .450], dtype=torch.float64)[None, :, None, None])

    def forward(self, x):
        return (x - self.shift) / self.scale


class _PkgLpips(nn.Module):
    """The package's structure: vgg16 ``features`` cut into five Sequential slices, NetLinLayer = Conv2d(C, 1, 1, bias=False), normalize_tensor,
    spatial_average / upsample, written with torch.nn modules and nothing from tests/_lpips_ref64.py."""

    def __init__(self, widths, lpips=True, spatial=False):
        super().__init__()
        cfg = [widths[0]] * 2 + ["M"] + [widths[1]] * 2 + ["M"] + [widths[2]] * 3 + ["M"] + [widths[3]] * 3 + ["M"] + [widths[4]] * 3
        mods, cin = [], 3
        for v in cfg:
            if v == "M":
                mods.append(nn.MaxPool2d(2, 2))
            else:
                mods += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU()]
                cin = v
        feats = nn.Sequential(*mods)
        self.slices = nn.ModuleList([nn.Sequential(*[feats[i] for i in range(lo, hi)]) for lo, hi in ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))])
        self.features = feats
        self.lins = nn.ModuleList([nn.Conv2d(c, 1, 1, bias=False) for c in widths])
        self.scaling = _PkgScaling()
        self.lpips, self.spatial = lpips, spatial

    def forward(self, a, b):
        a, b = 2 * a - 1, 2 * b - 1
        ha, hb = self.scaling(a), self.scaling(b)
        total = 0
        for k, sl in enumerate(self.slices):
            ha, hb = sl(ha), sl(hb)
            ua = ha / (torch.sqrt(torch.sum(ha ** 2, dim=1, keepdim=True)) + 1e-10)
            ub = hb / (torch.sqrt(torch.sum(hb ** 2, dim=1, keepdim=True)) + 1e-10)
            diff = (ua - ub) ** 2
            res = self.lins[k](diff) if self.lpips else diff.sum(dim=1, keepdim=True)
            res = nn.Upsample(size=a.shape[2:], mode="bilinear", align_corners=False)(res) if self.spatial else res.mean([2, 3], keepdim=True)
            total = total + res
        return total


@pytest.fixture(scope="module")
def engine_case():
    widths, n, hw = R.ENGINE_CONFIG
    sd, lins = R.engine_weights(widths)
    a, b = R.engine_inputs()
    return widths, sd, lins, a, b


@pytest.mark.parametrize("spatial", [False, True])
@pytest.mark.parametrize("linear", [True, False])
def test_restatement_vs_plain_module(engine_case, linear, spatial):
    widths, sd, lins, a, b = engine_case
    net = _PkgLpips(widths, lpips=linear, spatial=spatial).double()
    net.features.load_state_dict({k: v.double() for k, v in sd.items()})
    for k in range(5):
        net.lins[k].weight.data = lins[k].double().view(1, -1, 1, 1)
    go = torch.from_numpy(R._gen(77).standard_normal((2, 1) + (tuple(a.shape[2:]) if spatial else (1, 1)))).double()
    x, y = a.double().clone().requires_grad_(True), b.double().clone().requires_grad_(True)
    ref = net(x, y)
    assert bool(torch.isfinite(ref).all())
    (ref * go).sum().backward()
    out, ga, gb = R.value_and_grads(sd, lins if linear else None, widths, a, b, spatial, go)
    for tag, got, want in (("value", out, ref.detach()), ("grad a", ga, x.grad), ("grad b", gb, y.grad)):
        err = float((got - want).abs().max()) / max(1.0, float(want.abs().max()))
        print(f"[info] restatement vs plain module, linear={linear} spatial={spatial}, {tag}: {err:.3e}")
        assert got.shape == want.shape and err <= 1e-12
    assert float(ga.abs().max()) > 0 and float(gb.abs().max()) > 0


def test_level_adjoint_formula_vs_autograd():
    """The closed-form adjoint of the module doc against autograd in float64 (no all-zero pixels: autograd is NaN there)."""
    g = R._gen(91)
    fa = torch.from_numpy(g.standard_normal((2, 48, 5, 7))).clamp_min(0).requires_grad_(True)
    fb = torch.from_numpy(g.standard_normal((2, 48, 5, 7))).clamp_min(0).requires_grad_(True)
    w = torch.from_numpy(g.random(48))
    r = torch.from_numpy(g.standard_normal((2, 1, 5, 7)))
    (R.level(fa, fb, w) * r).sum().backward()
    dfa, dfb = R.level_adjoint(fa.detach(), fb.detach(), w, r)
    ea, eb = float((dfa - fa.grad).abs().max()), float((dfb - fb.grad).abs().max())
    print(f"[info] level adjoint formula vs autograd: {ea:.3e} {eb:.3e}")
    assert ea <= 1e-14 and eb <= 1e-14
    # at an all-zero pixel the gradient is defined as 0 on that side and stays finite on the other
    za = fa.detach().clone()
    za[0, :, 0, 0] = 0
    dza, dzb = R.level_adjoint(za, fb.detach(), w, r)
    assert not bool(dza[0, :, 0, 0].bool().any()) and bool(torch.isfinite(dzb).all()) and float(dzb[0, :, 0, 0].abs().max()) > 0
    x = za.clone().requires_grad_(True)
    (R.level(x, fb.detach(), w) * r).sum().backward()
    assert bool(torch.isfinite(x.grad).all()), "the restatement's own gradient is NaN at an all-zero pixel"


def test_hand_case():
    fa, fb, w = torch.tensor([[3.0, 4.0]]).double(), torch.tensor([[0.0, 5.0]]).double(), torch.tensor([1.0, 2.0])
    assert abs(float(R.level(fa, fb, w)) - 0.44) < 1e-9
    (s, na, nb, mean), _ = R.level_ref(fa.view(1, 1, 2), fb.view(1, 1, 2), w)
    assert abs(float(s) - 0.44) < 1e-9 and abs(float(na) - 5) < 1e-12 and abs(float(nb) - 5) < 1e-12 and abs(float(mean) - 0.44) < 1e-9


# ================================================ the class on the CPU ===================================================================
def test_state_dict_layout_and_loading():
    from perceptor_amd import losses
    widths = (16, 16, 32, 32, 48)
    m = losses.LPIPS(widths=widths)
    keys = set(m.model.state_dict())
    want = {"scaling_layer.shift", "scaling_layer.scale"} | {f"lin{k}.model.1.weight" for k in range(5)}
    for sl, idxs in ((1, (0, 2)), (2, (5, 7)), (3, (10, 12, 14)), (4, (17, 19, 21)), (5, (24, 26, 28))):
        want |= {f"net.slice{sl}.{i}.{leaf}" for i in idxs for leaf in ("weight", "bias")}
    assert keys == want
    assert tuple(m.model.state_dict()["lin2.model.1.weight"].shape) == (1, 32, 1, 1)
    for k, c in enumerate(widths):
        lw = m.model.state_dict()[f"lin{k}.model.1.weight"]
        assert float(lw.min()) >= 0 and abs(float(lw.double().mean()) - 1.0 / c) < 1e-6 / c
    # an upstream-layout state dict loads; a missing key is named
    other = losses.LPIPS(widths=widths, seed=3)
    sd = {k: v.clone() for k, v in other.model.state_dict().items()}
    m.model.load_state_dict(sd)
    assert torch.equal(m.model.state_dict()["net.slice3.12.weight"], sd["net.slice3.12.weight"])
    del sd["net.slice4.19.bias"], sd["lin3.model.1.weight"]
    with pytest.raises(RuntimeError, match=r"net\.slice4\.19\.bias") as ei:
        m.model.load_state_dict(sd)
    assert "lin3.model.1.weight" in str(ei.value)


def test_checkpoints_load(tmp_path):
    from perceptor_amd import losses
    from perceptor_amd.engine.vgg import vgg_state_dict_shapes
    from perceptor_amd.utils.synth import synth_state_dict
    widths = (16, 16, 32, 32, 48)
    feats = {"features." + k: v for k, v in synth_state_dict(vgg_state_dict_shapes(widths, (2, 2, 3, 3, 3)), 5).items()}
    feats["classifier.0.weight"] = torch.zeros(4, 4)
    lin = {f"lin{k}.model.1.weight": torch.full((1, c, 1, 1), 0.5) for k, c in enumerate(widths)}
    torch.save(feats, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lin.pth")
    m = losses.LPIPS(weights=None, features_checkpoint=str(tmp_path / "vgg16.pth"), linear_checkpoint=str(tmp_path / "lin.pth"), widths=widths)
    sd = m.model.state_dict()
    assert torch.equal(sd["net.slice2.7.weight"], feats["features.7.weight"]) and float(sd["lin4.model.1.weight"].mean()) == 0.5
    del feats["features.21.weight"]
    torch.save(feats, tmp_path / "short.pth")
    with pytest.raises(ValueError, match=r"21\.weight"):
        losses.LPIPS(weights=None, features_checkpoint=str(tmp_path / "short.pth"), linear_checkpoint=str(tmp_path / "lin.pth"), widths=widths)
    with pytest.raises(ValueError, match="not reachable"):
        losses.LPIPS(weights="imagenet", widths=widths)


def test_errors():
    from perceptor_amd import losses
    with pytest.raises(ValueError, match="stride-2 stem"):
        losses.LPIPS(name="squeeze")
    with pytest.raises(ValueError, match="11x11"):
        losses.LPIPS(name="alex")
    with pytest.raises(ValueError, match="unknown backbone"):
        losses.LPIPS(name="resnet")
    m = losses.LPIPS(widths=(16, 16, 32, 32, 48))
    a = torch.rand(1, 3, 32, 32)
    with pytest.raises(RuntimeError):
        m(a, a)
    with pytest.raises(RuntimeError):
        m.loss_and_grad(a, a)
    with pytest.raises(RuntimeError):
        m.targets(a)


# ================================================ bounds =================================================================================
def _fp32_level(fa, fb, w, r, gia, gib, gscale, dt):
    """The level and its adjoint in fp32 torch, channels summed in REVERSED order and the norm taken as a product of square roots'
    inverse: another summation order and another operation order than the kernel's."""
    a, b = fa.float().flip(-1), fb.float().flip(-1)
    wv = torch.ones(a.shape[-1]) if w is None else w.float().flip(-1)
    na, nb = a.square().sum(-1, keepdim=True).sqrt(), b.square().sum(-1, keepdim=True).sqrt()
    ia, ib = 1.0 / (na + 1e-10), 1.0 / (nb + 1e-10)
    d = a * ia - b * ib
    s = (wv * d * d).sum(-1)
    q = 2 * r.float().unsqueeze(-1) * wv * d
    outs = []
    for f, n, i, qq, gin in ((a, na, ia, q, gia), (b, nb, ib, -q, gib)):
        p = torch.where(n > 0, (f * qq).sum(-1, keepdim=True) * i * i / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(n))
        v = gscale * (qq * i - f * p) + (gin.float().flip(-1) if gin is not None else 0)
        outs.append(torch.where(f > 0, v, torch.zeros_like(v)).to(dt).flip(-1))
    return s, na[..., 0], nb[..., 0], s.mean(-1), outs


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("shape", R.LEVEL_SHAPES)
def test_fp32_evaluation_inside_bounds(shape, dtype):
    dt = R.DTYPES[dtype]
    cases = R.level_inputs(shape, dt)
    assert R.zero_pixel_patterns(cases) == {"a", "b", "ab"}, "a shape lacks one of the all-zero pixel patterns"
    worst = {}
    assert 0.35 < float((cases[0][0].float() == 0).double().mean()) < 0.75, "the features are not post-ReLU-like"
    for fa, fb, w, r, gia, gib in cases:
        for wv in (w, None):
            for gscale in (1.0, 65536.0):
                for ga, gb in ((None, None), (gia, gib)):
                    s, na, nb, mean, (da, db) = _fp32_level(fa, fb, wv, r, ga, gb, gscale, dt)
                    refs, bounds = R.level_ref(fa, fb, wv)
                    (ra, rb), (ba, bb) = R.level_bwd_ref(fa, fb, wv, r, ga, gb, gscale, dt)
                    for tag, got, ref, bound in (("s", s, refs[0], bounds[0]), ("na", na, refs[1], bounds[1]), ("nb", nb, refs[2], bounds[2]),
                                                 ("mean", mean, refs[3], bounds[3]), ("dFa", da, ra, ba), ("dFb", db, rb, bb)):
                        ok = (got.double() - ref).abs() <= bound
                        ratio = float(((got.double() - ref).abs() / bound.clamp_min(1e-300)).max())
                        worst[tag] = max(worst.get(tag, 0.0), ratio)
                        assert bool(ok.all()), f"{tag} {shape} {dtype}: fp32 evaluation at {ratio:.3e} of the bound"
    print(f"[bound] fp32 evaluation {shape} {dtype}: worst |got - ref| / bound " + ", ".join(f"{k} {v:.3e}" for k, v in worst.items()))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_level_defects_exceed_bounds(dtype):
    """Level defects at the level kernels' inputs: the defective float64 result leaves the bound by more than a factor 2 at every shape
    (sum instead of mean: at every shape with more than one pixel -- with one pixel the sum IS the mean)."""
    dt = R.DTYPES[dtype]
    for shape in R.LEVEL_SHAPES:
        fa, fb, w, r, gia, gib = R.level_inputs(shape, dt)[0]
        (s, _, _, mean), (b_s, _, _, b_mean) = R.level_ref(fa, fb, w)
        (ra, rb), (ba, bb) = R.level_bwd_ref(fa, fb, w, r, gia, gib, 65536.0, dt)
        mult = {}
        for defect in ("no_norm", "w_before_square"):
            bad = R.level(R.cl(fa), R.cl(fb), w, defect)[:, 0]
            mult[defect] = float(((bad - s).abs() / b_s.clamp_min(1e-300)).max())
        if shape[1] > 1:
            mult["sum_pixels"] = float(((s.sum(-1) - mean).abs() / b_mean).max())
        (pa, pb), _ = R.level_bwd_ref(fa, fb, w, r, gia, gib, 65536.0, dt, defect="no_projection")
        mult["no_projection"] = max(float(((pa - ra).abs() / ba.clamp_min(1e-300)).max()), float(((pb - rb).abs() / bb.clamp_min(1e-300)).max()))
        (_, nb_), _ = R.level_bwd_ref(fa, fb, w, r, gia, gib, 65536.0, dt, defect="negate_b")
        mult["negate_b"] = float(((nb_ - rb).abs() / bb.clamp_min(1e-300)).max())
        print(f"[defect] level {shape} {dtype}: multiples of the bound " + ", ".join(f"{k} {v:.3e}" for k, v in mult.items()))
        assert all(v > 2.0 for v in mult.values()), mult


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_tower_defects_exceed_gates(engine_case, dtype):
    """Tower defects at the engine test's inputs: the defective emulated tower's tap features leave the feature gate sqrt(d_l) u (relative
    L2 against the emulated tower) by more than a factor 2 at some tap, and the value leaves the kernel bound by more than a factor 2."""
    widths, sd, lins, a, b = engine_case
    dt, u = R.DTYPES[dtype], R.UNIT[R.DTYPES[dtype]]
    good_a, good_b = R.taps(R.tower(sd, widths, a, dt)), R.taps(R.tower(sd, widths, b, dt))
    val = R.output(good_a, good_b, lins, a.shape[2:])
    vb = R.value_bound(good_a, good_b, lins, a.shape[2:], False)
    for defect in ("relu4_2", "fold_shift", "no_2x_minus_1"):
        bad_a, bad_b = R.taps(R.tower(sd, widths, a, dt, defect=defect), defect), R.taps(R.tower(sd, widths, b, dt, defect=defect), defect)
        rel = [float((x - y).norm() / y.norm()) / (math.sqrt(d) * u) for x, y, d in zip(bad_a, good_a, R.FEATURE_ROUNDINGS)]
        vm = float(((R.output(bad_a, bad_b, lins, a.shape[2:]) - val).abs() / vb).max())
        print(f"[defect] tower {defect} {dtype}: feature rel-L2 / gate per tap " + ", ".join(f"{r:.3e}" for r in rel) + f"; value / bound {vm:.3e}")
        assert max(rel) > 2.0 and vm > 2.0
    # the adjoint defects move the image gradient by far more than its gate sqrt(17) u
    go = torch.ones(2, 1, 1, 1, dtype=torch.float64)
    x = a.double().clone().requires_grad_(True)
    fa = R.taps(R.tower(sd, widths, x, dt))
    feats = [f.detach() for f in fa]
    ref_g = torch.autograd.grad((R.output(fa, good_b, lins, a.shape[2:]) * go).sum(), x, retain_graph=True)[0]
    gate = math.sqrt(R.GRAD_ROUNDINGS) * u

    def image_grad(defect):
        """The tower's autograd seeded with the closed-form level adjoints.  negate_b: the features take the b seat of the level (by
        symmetry their correct gradient is the same), where the defect negates it."""
        seeds = []
        for l, (f, fb) in enumerate(zip(feats, good_b)):
            r = torch.full((f.shape[0], 1) + tuple(f.shape[2:]), 1.0 / (f.shape[2] * f.shape[3]), dtype=torch.float64)
            seeds.append(R.level_adjoint(fb, f, lins[l], r, defect)[1] if defect == "negate_b" else R.level_adjoint(f, fb, lins[l], r, defect)[0])
        return torch.autograd.grad(fa, x, seeds, retain_graph=True)[0]

    assert float((image_grad(None) - ref_g).norm() / ref_g.norm()) <= 1e-12
    for defect in ("no_projection", "negate_b"):
        m = float((image_grad(defect) - ref_g).norm() / ref_g.norm()) / gate
        print(f"[defect] adjoint {defect} {dtype}: image gradient rel-L2 / gate {m:.3e}")
        assert m > 2.0
