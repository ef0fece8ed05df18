"""CPU: MonsterDiffusion.  The float64 restatement (tests/_monster_ref64.py) against the reference's own values
(tests/golden/monster_diffusion_reference.npz, written by tools/gen_monster_diffusion_golden.py), the state-dict names, the host logic
of models.MonsterDiffusion, and seeded defects at the inputs of tests/test_gpu_monster.py.

Measured when this file was written: the restatement reproduces every fixture tensor to a rel-L2 of at most 1.94e-15 (the third Heun
yield; block outputs 3e-16 .. 1.4e-15, cond and proj_in exactly); the gate is 10 x that.
"""
import numpy as np
import pytest
import torch

import _monster_ref64 as M
from conftest import golden

RESTATEMENT_GATE = 10 * 1.94e-15


@pytest.fixture(scope="module")
def g():
    return golden("monster_diffusion_reference")


@pytest.fixture(scope="module")
def clean(g):
    """float64 checkpoints of both networks at the fixture's inputs (shared, never modified)"""
    out = {}
    for net, (config, _) in M.NETS.items():
        rec = {}
        rec["denoised_xs"] = M.denoised64(M.synthetic_state_dict(config), g[f"{net}_in"].double(), g[f"{net}_sigma"], config, record=rec)
        out[net] = rec
    return out


# ---- 1. the restatement reproduces the fixture ------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_fixture(g, clean):
    worst = {}

    def cmp(name, got):
        worst[name] = M.rel_l2(M.sampled(got, g, name), g[name])

    for net, (config, shape) in M.NETS.items():
        sd = M.synthetic_state_dict(config)
        x, sg, rec = g[f"{net}_in"].double(), g[f"{net}_sigma"], clean[net]
        for k in M.CHECKPOINTS + ("denoised_xs",):
            cmp(f"{net}_{k}", rec[k])
            if f"{net}_{k}_norm" in g:                  # a sampled checkpoint: the whole tensor's norm pins the values in between
                assert abs(float(rec[k].norm()) / float(g[f"{net}_{k}_norm"]) - 1) < RESTATEMENT_GATE
        cmp(f"{net}_cond", rec["cond"].expand(shape[0], -1))
        den = rec["denoised_xs"]
        cmp(f"{net}_eps", M.eps64(x, den, sg))
        cmp(f"{net}_step", M.step64(x, den, sg, g[f"{net}_to_sigma"]))
        cmp(f"{net}_correction", M.correction64(x, den, sg, g[f"{net}_prev_in"].double(), g[f"{net}_prev_sigma"], g[f"{net}_prev_eps"].double()))
        cmp(f"{net}_inject", M.inject64(x, sg, sg * 1.3, g[f"{net}_inject_noise"]))
        if net == "A":
            dn = lambda im, s: M.denoised64(sd, im, s, config)
            ys = M.elucidated64(dn, g["A_x0"].double(), 6, list(g["A_heun_noise"]))
            assert len(ys) == len(g["A_heun"]) == 3                      # n_evaluations // 2 yields
            cmp("A_heun", torch.stack(ys))
            coeffs = []
            ys = M.lms_sample64(dn, g["A_x0"].double(), 6, coeffs_out=coeffs)
            assert len(ys) == len(g["A_lms"]) == 6                       # n_evaluations yields
            cmp("A_lms", torch.stack(ys))
            for i, row in enumerate(coeffs):                             # scipy's quad at epsrel 1e-4 against the exact integral
                assert np.allclose(row, g["A_lms_coeffs"][i, :len(row)].numpy(), rtol=1e-4, atol=1e-12)
    print("[monster] restatement vs fixture, worst rel-L2:", max(worst, key=worst.get), max(worst.values()))
    assert max(worst.values()) <= RESTATEMENT_GATE, worst
    assert M.rel_l2(M.schedule64(5), g["schedule_5"]) < 1e-15
    # (the reference's sqrt(2) - 1 is a float32 value whatever the default dtype: torch.tensor(2).sqrt())
    assert torch.allclose(M.gamma64(g["gamma_ts"], 10), g["gamma_10"], rtol=1e-7) and torch.equal(M.gamma64(g["gamma_ts"], 400), g["gamma_400"])
    assert torch.allclose(M.reversed64(g["gamma_ts"], 10), g["reversed_10"], rtol=1e-7)
    for fn in ("c_skip", "c_out", "c_in", "c_noise"):
        assert M.rel_l2(getattr(M, fn + "64")(g["gamma_ts"]), g[fn].reshape(-1)) < 1e-15


def test_resampler_restatement_is_torchs_operator():
    for which, shapes in (("down", M.FIR_DOWN_SHAPES), ("up", M.FIR_UP_SHAPES)):
        for shape in shapes[:3]:
            x = M.fir_input(shape, 3, "bf16")
            assert float((M.fir_ref(x, which, "bf16")[0] - M.fir_torch(x, which)).abs().max()) < 1e-15


def test_gate_tables_are_what_the_emulation_measures(g, clean):
    """the GPU test's gates are 2 x these figures: they must be the emulated restatement's own distances, not something looser"""
    for (net, dtype), table in M.EMU.items():
        config, _ = M.NETS[net]
        rec = {}
        rec["denoised_xs"] = M.denoised64(M.synthetic_state_dict(config), g[f"{net}_in"].double(), g[f"{net}_sigma"], config, emulate=dtype, record=rec)
        for k, v in table.items():
            assert M.rel_l2(M.sampled(rec[k], g, f"{net}_{k}"), g[f"{net}_{k}"]) == pytest.approx(v, rel=0.02), (net, dtype, k)
        assert M.roundings(config)["proj_in"] == 2


# ---- 2. state dict ---------------------------------------------------------------------------------------------------------------------------------
def test_product_state_dict_names_and_shapes(g):
    from perceptor_amd.engine.monster import monster_state_dict_shapes, product_config
    shapes = monster_state_dict_shapes(product_config())
    assert len(shapes) == 276 and list(shapes) == g["product_names"].tolist()
    assert [",".join(str(s) for s in v) for v in shapes.values()] == g["product_shapes"].tolist()
    assert sum(int(np.prod(v)) for v in shapes.values()) == int(g["product_numel"])
    assert sum(k.endswith(".kernel") for k in shapes) == 4


# ---- 3. host logic ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    from perceptor_amd.models import MonsterDiffusion
    return MonsterDiffusion(config=M.NETS["A"][0])


def test_schedule_gamma_and_parameterisation(model, g):
    probe = g["gamma_ts"].float()
    assert torch.allclose(model._schedule_ts(5).double(), g["schedule_5"], rtol=1e-5)
    pairs = list(model.schedule_ts(5))
    assert len(pairs) == 4 and float(pairs[0][0]) == pytest.approx(80.0) and float(pairs[-1][1]) == pytest.approx(0.01)
    assert torch.allclose(model.gamma(probe, 10).double(), g["gamma_10"]) and torch.allclose(model.gamma(probe, 400).double(), g["gamma_400"])
    assert torch.allclose(model.reversed_ts(probe, 10).double(), g["reversed_10"], rtol=1e-6)
    for fn in ("c_skip", "c_out", "c_in", "c_noise"):
        assert torch.allclose(getattr(model, fn)(probe).double().reshape(-1), g[fn].reshape(-1), rtol=1e-5, atol=1e-7), fn
    sig = model.sigmas(model._schedule_ts(6)).flatten()
    for i in range(5):
        for j in range(min(i + 1, 4)):
            assert model.linear_multistep_coeff(min(i + 1, 4), sig, i, j) == pytest.approx(float(g["A_lms_coeffs"][i, j]), rel=1e-4, abs=1e-9)
    with pytest.raises(ValueError):
        model.linear_multistep_coeff(3, sig, 1, 0)                     # order too high for the second step


def test_sigmas_shape_rules(model, g):
    assert tuple(model.sigmas(0.5).shape) == tuple(g["sigmas_float_shape"].tolist()) == (1,)
    assert tuple(model.sigmas(torch.tensor(0.5)).shape) == tuple(g["sigmas_0dim_shape"].tolist()) == (1,)
    assert tuple(model.sigmas(torch.tensor([0.5, 0.7])).shape) == tuple(g["sigmas_1dim_shape"].tolist()) == (2, 1, 1, 1)
    assert torch.equal(model.alphas(torch.tensor([0.5, 0.7])).double(), g["alphas_1dim"])
    assert tuple(model.random_noise(2).shape) == (2, 3, 48, 48) and tuple(model.training_ts(5).shape) == (5,)
    x = torch.rand(2, 3, 8, 12)
    noise = torch.randn(2, 3, 8, 12)
    assert torch.allclose(model.diffuse(x, 0.5, noise), x + noise * 0.25, atol=1e-6)


def test_sampler_yield_counts(model, monkeypatch):
    """both generators' host loops, with the device steps replaced by pass-through stand-ins"""
    from perceptor_amd.engine import sampler
    from perceptor_amd.models.monster_diffusion import MonsterDiffusion

    class Stub:
        def __init__(self, x):
            self.eps = self.denoised_images = x

        def step(self, to_ts):
            return self.eps

        def correction(self, *a):
            return self.eps

    calls = []
    monkeypatch.setattr(sampler, "clamp", lambda a, lo, hi: a.clamp(lo, hi))
    monkeypatch.setattr(sampler, "edm_lms", lambda images, coeffs, epses: images)
    monkeypatch.setattr(MonsterDiffusion, "inject_noise", lambda self, images, ts, rts, noise=None: images)
    monkeypatch.setattr(MonsterDiffusion, "predictions", lambda self, images, ts, aug=None: calls.append(float(ts)) or Stub(images))
    x = torch.rand(1, 3, 8, 12)
    assert len(list(model.sample(1, n_evaluations=6, diffused_images=x))) == 3 and len(calls) == 5
    del calls[:]
    assert len(list(model.linear_multistep_sample(1, n_evaluations=6, diffused_images=x))) == 6 and len(calls) == 6
    assert calls[0] == pytest.approx(80.0) and calls[-1] == pytest.approx(0.01)
    assert len(list(model.elucidated_sample(1, n_evaluations=7, diffused_images=x))) == 3


def test_error_types(model, tmp_path):
    from perceptor_amd import models
    from perceptor_amd.engine import monster
    config = M.NETS["A"][0]
    with pytest.raises(ValueError):
        models.MonsterDiffusion("nope")
    with pytest.raises(ValueError):
        models.MonsterDiffusion(weights="download", config=config)
    x = torch.rand(2, 3, 8, 12)
    with pytest.raises(RuntimeError):
        model.predictions(x, 0.5)                                    # a CPU tensor: no CPU fallback
    model.train()
    try:
        with pytest.raises(Exception, match="training mode"):
            model.predictions(x, 0.5)
        with pytest.raises(Exception, match="training mode"):
            next(model.sample(2, 6, diffused_images=x))
        with pytest.raises(RuntimeError, match="HIP device"):        # predictions_ has no training-mode check: it fails on the CPU tensor
            model.predictions_(x, 0.5)
    finally:
        model.eval()
    sd = M.synthetic_state_dict(config)
    monster.check_state_dict(config, sd)
    monster.check_state_dict(config, monster.bare_state_dict({"network." + k: v for k, v in sd.items()}))
    bad = dict(sd)
    bad["u_net.d_blocks.1.0.kernel"] = torch.full((4, 4), 1 / 16)   # a box filter: the kernels hard-code [1, 3, 3, 1]
    with pytest.raises(ValueError, match="kernel"):
        monster.check_state_dict(config, bad)
    for broken in ({k: v for k, v in sd.items() if k != "proj_out.bias"}, {**sd, "extra.weight": torch.zeros(1)},
                   {**sd, "proj_in.weight": torch.zeros(32, 4, 1, 1)}):
        with pytest.raises(ValueError):
            monster.check_state_dict(config, broken)
    path = tmp_path / "wrapper.pt"
    torch.save(model.state_dict(), path)                               # the wrapper's own state dict: `network.`-prefixed keys
    assert all(k.startswith("network.") for k in model.state_dict())
    models.MonsterDiffusion(checkpoint=str(path), config=config)
    torch.save({k: v for k, v in model.state_dict().items() if "proj_out" not in k}, path)
    with pytest.raises(ValueError):
        models.MonsterDiffusion(checkpoint=str(path), config=config)
    for cfg in ((64, [1, 1], [48, 64], [False, False], 9), (64, [1, 1], [32, 96], [False, True], 9), (64, [1, 1], [32], [False, False], 9)):
        with pytest.raises(ValueError):
            monster.check_config(cfg)
    with pytest.raises(ValueError):
        monster.check_size(config, 4, 4)                                # the deepest map would be 1 x 1: the reflect pad needs 2
    monster.check_size(config, 8, 12)


# ---- 4. seeded defects at the GPU tests' inputs ---------------------------------------------------------------------------------------------------
def test_resampler_defects_exceed_twice_the_bound():
    rows = {}
    for which, shapes, defects in (("down", M.FIR_DOWN_SHAPES, ("down_clamp", "taps_1221")), ("up", M.FIR_UP_SHAPES, ("up_clamp", "taps_1221"))):
        for shape in shapes[:3]:
            for dtype in ("f16", "bf16"):
                x = M.fir_input(shape, 11 + shape[1] * shape[2], dtype)          # the GPU test's input
                y, tol = M.fir_ref(x, which, dtype)
                for d in defects:
                    if which == "down" and shape[1] == 2 and shape[2] == 2:
                        continue        # a 2 x 2 map comes out as its mean under reflect, clamp and any symmetric normalised taps alike
                    rows[(which, d, shape, dtype)] = float(((M.fir_ref(x, which, dtype, d)[0] - y).abs() / tol).max())
    print("[monster] resampler defects, smallest multiple of the bound:", min(rows.values()))
    assert min(rows.values()) > 2.0, {k: v for k, v in rows.items() if v <= 2.0}


def test_edm_defects_exceed_twice_the_bound():
    I = M.edm_inputs()
    for sigma, to, prev, rev in M.edm_sigma_cases():
        v, tol = M.edm_stage_out_ref(I["img"], I["net"], sigma)
        assert float(((M.edm_stage_out_ref(I["img"], I["net"], sigma, "cskip_cout_swapped")[0] - v).abs() / tol).max()) > 2.0
        ref = M.edm_predict_ref(I["img"], I["den"], sigma, to, I["prev_img"], prev, I["prev_eps"])[2]
        bad = M.edm_predict_ref(I["img"], I["den"], sigma, to, I["prev_img"], prev, I["prev_eps"], "heun_no_half")[2]
        assert float(((bad[0] - ref[0]).abs() / ref[1]).max()) > 2.0
        _, _, c, c_tol = M.edm_stage_in_ref(I["img"], sigma, "bf16")
        assert float(((M.edm_stage_in_ref(I["img"], sigma, "bf16", "c_noise_ln")[2] - c).abs() / c_tol).max()) > 2.0


def test_tanh_gelu_exceeds_twice_the_bound_of_the_adagn_layer_test():
    """the tanh form of GELU moves the 16-bit checkpoints by 0.02 - 0.05 of their bf16 gates (0.2 - 0.4 in f16) and the fp32 conditioning by
    about its own bound: the element-wise AdaGN + GELU check of the GPU file is the input at which it shows"""
    for dtype in ("f16", "bf16"):
        x, film = M.adagn_case(dtype)
        for f in (film, film[:1]):
            y, tol = M.adagn_ref(x, f, dtype)
            mult = float(((M.adagn_ref(x, f, dtype, "tanh_gelu")[0] - y).abs() / tol).max())
            print(f"[monster] defect tanh_gelu, AdaGN layer {dtype}: x bound {mult:.1f}")
            assert mult > 2.0


NETWORK_DEFECTS = ("adagn_no_plus1", "adagn_swapped", "groups32", "heads_first", "c_noise_ln", "cskip_cout_swapped")


@pytest.mark.parametrize("net", ["A", "B"])
def test_network_defects_exceed_twice_the_gate(net, g, clean):
    config, _ = M.NETS[net]
    sd = M.synthetic_state_dict(config)
    x, sg = g[f"{net}_in"].double(), g[f"{net}_sigma"]
    rec = {}
    rec["denoised_xs"] = M.denoised64(sd, x, sg, config, defect=M.NOOP_DEFECT, record=rec)
    for k in M.CHECKPOINTS + ("denoised_xs",):                     # one d^-1/2 on q is the same arithmetic: it must NOT move anything
        assert M.rel_l2(rec[k], clean[net][k]) < 1e-14
    _, cond_tol = M.cond_ref(sd, sg)
    for d in NETWORK_DEFECTS:
        rec = {}
        rec["denoised_xs"] = M.denoised64(sd, x, sg, config, defect=d, record=rec)
        cond_mult = float(((rec["cond"] - clean[net]["cond"]).abs() / cond_tol).max())       # the conditioning's per-element bound
        for dtype in ("bf16", "f16"):
            mult = {k: M.rel_l2(rec[k], clean[net][k]) / M.gate(net, dtype, k) for k in M.CHECKPOINTS + ("denoised_xs",)}
            mult["cond"] = cond_mult
            print(f"[monster] defect {d} net {net} {dtype}: x gate, best checkpoint {max(mult, key=mult.get)} {max(mult.values()):.1f}, denoised_xs {mult['denoised_xs']:.1f}")
            assert mult["denoised_xs"] > 2.0 and max(mult.values()) > 2.0, (d, dtype, mult)
