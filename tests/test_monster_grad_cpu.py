"""CPU: MonsterDiffusion's input gradient.  The float64 gradient restatement (tests/_monster_grad_ref64.py) against the reference's own
autograd values (tests/golden/monster_diffusion_grad_reference.npz, written by tools/gen_monster_grad_golden.py), the float64 FIR adjoints,
the gate tables of tests/test_gpu_monster_grad.py, seeded defects at that test's inputs, and the host side of the public surface.

Measured when this file was written: the restatement reproduces every fixture gradient, per sample, to a rel-L2 of at most 5.0e-15 (the
forward agreement is 1.94e-15); the gate is the issue's 1e-12.
"""
import pytest
import torch

import _monster_grad_ref64 as G
import _monster_ref64 as M
from conftest import golden

RESTATEMENT_GATE = 1e-12


@pytest.fixture(scope="module")
def fwd():
    return golden("monster_diffusion_reference")


@pytest.fixture(scope="module")
def g():
    return golden("monster_diffusion_grad_reference")


def _name(net, k):
    return f"{net}_{k}" if k in ("gx", "d_images") else f"{net}_g_{k}"


@pytest.fixture(scope="module")
def clean(fwd, g):
    """float64 gradients of both networks at the fixture's inputs and cotangent (shared, never modified)"""
    return {net: G.grad64(M.synthetic_state_dict(config), fwd[f"{net}_in"].double(), fwd[f"{net}_sigma"], config, g[f"{net}_cotangent"])
            for net, (config, _) in M.NETS.items()}


# ---- 1. the restatement reproduces the fixture ------------------------------------------------------------------------------------------------
def test_gradient_restatement_reproduces_the_fixture(fwd, g, clean):
    worst = {}
    for net, (config, _) in M.NETS.items():
        r = clean[net]
        assert M.rel_l2(r["denoised_xs"], fwd[f"{net}_denoised_xs"]) <= RESTATEMENT_GATE
        for k in G.grad_keys(config):
            name = _name(net, k)
            worst[name] = max(G.per_sample_sampled(r[k], g, name))
            norms = r[k].flatten(1).norm(dim=1)                  # a sampled gradient: the per-sample norms pin the values in between
            assert float((norms / g[name + "_sample_norms"] - 1).abs().max()) <= RESTATEMENT_GATE, name
        # plain autograd over the forward restatement as it stands (no explicit backward piece of this file)
        x = fwd[f"{net}_in"].double().requires_grad_()
        with torch.enable_grad():
            den = M.denoised64(M.synthetic_state_dict(config), x, fwd[f"{net}_sigma"], config)
            (den * g[f"{net}_cotangent"].double()).sum().backward()
        worst[f"{net} autograd of denoised64"] = M.rel_l2(x.grad, g[f"{net}_d_images"])
    print("[monster grad] restatement vs fixture, worst per-sample rel-L2:", max(worst, key=worst.get), max(worst.values()))
    assert max(worst.values()) <= RESTATEMENT_GATE, worst


# ---- 2. FIR adjoints --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 5, 6, 8])
def test_fir_adjoint_matrices(n):
    """per axis: the all-ones closed forms, the term counts, and (up) autograd of the one-axis forward; the 2-D test below covers down"""
    gen = torch.Generator().manual_seed(n)
    B = G.up_bwd_matrix(n)
    x = torch.randn(1, 1, n, 3, generator=gen, dtype=torch.float64, requires_grad=True)
    y = M._up_axis(x, 2, None)
    gy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    (gx,) = torch.autograd.grad((y * gy).sum(), x)
    assert float((gx - torch.einsum("ih,nchw->nciw", B, gy)).abs().max()) <= 1e-15
    assert torch.equal(B.sum(1), G.ones_closed_form("up", n))
    assert int(G.bwd_terms("up", n).max()) == {2: 4, 3: 6}.get(n, 5)
    if n % 2 == 0:
        B = G.down_bwd_matrix(n)
        assert torch.equal(B.sum(1), G.ones_closed_form("down", n))
        assert int(G.bwd_terms("down", n).max()) == (2 if n == 2 else 3)


@pytest.mark.parametrize("which,shape", [("down", s) for s in M.FIR_DOWN_SHAPES[:3]] + [("up", s) for s in M.FIR_UP_SHAPES[:3]])
def test_fir_adjoints_are_the_transposes(which, shape):
    n, h, w, c = shape
    gen = torch.Generator().manual_seed(h * w)
    x = torch.randn(n, c, h, w, generator=gen, dtype=torch.float64, requires_grad=True)
    y = M.fir_down64(x) if which == "down" else M.fir_up64(x)
    gy = torch.randn(y.shape, generator=gen, dtype=torch.float64)
    (auto,) = torch.autograd.grad((y * gy).sum(), x)
    mine = G.fir_bwd64(gy, which)
    assert float((mine - auto).abs().max()) <= 1e-14 * float(auto.abs().max())
    lhs, rhs = float((y.detach() * gy).sum()), float((x.detach() * mine).sum())
    assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), float((y.detach() * gy).abs().sum()))
    ones = G.fir_bwd64(torch.ones_like(gy), which)
    want = G.ones_closed_form(which, h)[:, None] * G.ones_closed_form(which, w)[None, :]
    assert float((ones - want).abs().max()) <= 1e-15


def test_fir_adjoint_defects_exceed_twice_the_bound():
    for which in ("down", "up"):
        for (dxs, dys) in G.fir_bwd_shapes(which)[:3]:
            gy = M.fir_input(dys, 5, "bf16")
            ref, tol = G.fir_bwd_ref(gy, which, "bf16")
            for d in (f"{which}_bwd_clamp", f"{which}_bwd_no_fold", "down_bwd_avgpool" if which == "down" else "up_bwd_bilinear"):
                bad, _ = G.fir_bwd_ref(gy, which, "bf16", defect=d)
                if d in ("down_bwd_clamp", "down_bwd_avgpool") and dxs[1:3] == (2, 2):
                    # two samples per axis: the reflect-padded row (x1, x0, x1, x0) under [1, 3, 3, 1] / 8 is the plain average, and the two
                    # folds carry the same weight 1/8 and only swap places under clamping: the same operator, nothing to see
                    assert torch.equal(bad, ref)
                    continue
                r = float(((bad - ref).abs() / tol).max())
                print(f"[monster grad] {d} at {dxs}: worst |defect - ref| / bound {r:.1f}")
                assert r >= 2.0, (d, dxs)


def test_edm_adjoint_defects_exceed_twice_the_bound():
    I = G.edm_bwd_inputs()
    for sigma, *_ in M.edm_sigma_cases():
        v, tol = G.edm_stage_out_bwd_ref(I["d"], sigma, 1.0, "bf16")
        bad, _ = G.edm_stage_out_bwd_ref(I["d"], sigma, 1.0, "bf16", defect="cout_cin_swapped")
        # (c_out = c_in where sigma D = 1: not at these sigmas)
        assert float(((bad - v).abs() / tol).max()) >= 2.0
        v, tol = G.edm_stage_in_bwd_ref(I["d"], I["gx"], sigma, 1.0)
        for d in ("cout_cin_swapped", "no_cskip_term", "no_factor_2"):
            bad, _ = G.edm_stage_in_bwd_ref(I["d"], I["gx"], sigma, 1.0, defect=d)
            assert float(((bad - v).abs() / tol).max()) >= 2.0, (d, sigma)


# ---- 3. the gate tables are what the emulation measures --------------------------------------------------------------------------------------
def test_gradient_gate_tables_are_what_the_emulation_measures(fwd, g, clean):
    for (net, dtype), table in G.EMU_GRAD.items():
        config, _ = M.NETS[net]
        e = G.grad64(M.synthetic_state_dict(config), fwd[f"{net}_in"].double(), fwd[f"{net}_sigma"], config, g[f"{net}_cotangent"], emulate=dtype)
        assert set(table) == set(G.grad_keys(config))
        for k, v in table.items():
            assert G.per_sample(e[k], clean[net][k]) == pytest.approx(v, rel=0.02), (net, dtype, k)
    sd = M.synthetic_state_dict(M.PRODUCT)
    img, sigma, cot = G.product_grad_case()
    ref = G.grad64(sd, img.double(), sigma.double(), M.PRODUCT, cot)
    one = torch.tensor([G.PRODUCT_SCALAR_SIGMA], dtype=torch.float64)
    ref1 = G.grad64(sd, img.double(), one, M.PRODUCT, cot)
    for tables, sg, r in ((G.EMU_GRAD_PRODUCT, sigma.double(), ref), (G.EMU_GRAD_PRODUCT_SCALAR, one, ref1)):
        for dtype, table in tables.items():
            e = G.grad64(sd, img.double(), sg, M.PRODUCT, cot, emulate=dtype)
            for k, v in table.items():
                assert G.per_sample(e[k], r[k]) == pytest.approx(v, rel=0.02), (dtype, k)


# ---- 4. seeded defects at the GPU test's inputs ----------------------------------------------------------------------------------------------
# A defect counts as seen where some gated quantity (gx, a block-input gradient or d_images; one sample or the batch) moves by at least twice
# its bf16 gate.  Measured when this was written (worst distance / bf16 gate, network A | B): the resampler faults 18 - 31 | 12 - 36, AdaGN
# without the mean terms 64 | 16, without the 1 + 76 | 58, skip dropped 130 | 83, dx1 dropped 76 | 57, attention dropped 53 | 31,
# c_out <-> c_in 826 | 17 (in gx and the block gradients alone: c_out c_in is symmetric, d_images does not move), no c_skip term 111 | 2.6
# (sample 0 of A, sigma 0.3; at sigma 40 c_skip is 1.6e-4 and the term is invisible), no factor 2 55 | 29.  tanh-GELU's derivative moves the
# gradient by 5.7e-4 .. 1.0e-3, 0.06 of a bf16 gate and about half an f16 gate: as in the forward it is below every network-level gate and is reported, not asserted; the
# element-wise AdaGN + GELU backward layer test is where the two derivatives part (test_adagn_backward_defects_... below).
REPORT_ONLY = ("adagn_bwd_tanh_gelu",)


def test_gradient_defects_exceed_twice_the_gate(fwd, g, clean):
    seen = {d: 0.0 for d in G.GRAD_DEFECTS}
    for net, (config, _) in M.NETS.items():
        sd = M.synthetic_state_dict(config)
        for d in G.GRAD_DEFECTS:
            bad = G.grad64(sd, fwd[f"{net}_in"].double(), fwd[f"{net}_sigma"], config, g[f"{net}_cotangent"], defect=d)
            worst = 0.0
            for k in G.grad_keys(config):
                dist = G.per_sample(bad[k], clean[net][k])
                worst = max(worst, max(v / G.grad_gate(net, "bf16", k, i) for i, v in enumerate(dist)))
            print(f"[monster grad] defect {d} on {net}: worst distance / bf16 gate {worst:.2f}")
            seen[d] = max(seen[d], worst)
            if d not in REPORT_ONLY:
                assert worst >= 2.0, (net, d, worst)
    assert seen["adagn_bwd_tanh_gelu"] < 2.0          # (should this ever show at network level, move it out of REPORT_ONLY)


def test_adagn_backward_defects_exceed_twice_the_bound_of_the_layer_test():
    """tanh-GELU's derivative differs from erf-GELU's by at most 8.7e-4 (at |z| = 2.0) and by 29 % where the derivative crosses zero
    (z = -0.75): the element-wise AdaGN + GELU backward check of the GPU file is the input at which it shows (13 - 17 of its bound; the other two AdaGN
    faults 780 - 4500)"""
    for dtype in ("f16", "bf16"):
        x, film, dy = G.adagn_bwd_case(dtype)
        for f in (film, film[:1]):
            ref, tol = G.adagn_bwd_ref(x, f, dy, dtype)
            for d in ("adagn_bwd_tanh_gelu", "adagn_bwd_no_mean", "adagn_bwd_no_plus1"):
                bad, _ = G.adagn_bwd_ref(x, f, dy, dtype, defect=d)
                r = float(((bad - ref).abs() / tol).max())
                print(f"[monster grad] {d} {dtype} rows {f.shape[0]}: worst |defect - ref| / bound of the layer test {r:.1f}")
                assert r >= 2.0, (d, dtype)


# ---- 5. host side of the public surface -----------------------------------------------------------------------------------------------------
def test_public_surface_on_the_cpu(fwd):
    from perceptor_amd import _hip
    from perceptor_amd.models import MonsterDiffusion
    from perceptor_amd.models.monster_diffusion.prediction import PredictionBatch
    m = MonsterDiffusion(config=M.NETS["A"][0], input_grad=True)
    assert m.input_grad and not MonsterDiffusion(config=M.NETS["A"][0]).input_grad
    for name in ("pmi_fir_down2_bwd", "pmi_fir_up2_bwd", "pmi_edm_stage_out_bwd", "pmi_edm_stage_in_bwd"):
        assert name in _hip._PROTOS
    from perceptor_amd.engine.monster import MonsterEngine
    assert hasattr(MonsterEngine, "forward_train") and hasattr(MonsterEngine, "backward")
    # the torch fallbacks of eps / step / correction (taken when the prediction carries a graph) are the float64 formulas
    x, den = fwd["A_in"].clone().requires_grad_(), fwd["A_denoised_xs"].float()
    sg = fwd["A_sigma"].float()
    with torch.enable_grad():
        p = PredictionBatch(denoised_xs=den, diffused_images=x, ts=sg)
        eps, step = p.eps, p.step(fwd["A_to_sigma"].float())
        corr = p.correction(fwd["A_prev_in"], fwd["A_prev_sigma"].float(), fwd["A_prev_eps"])
        assert eps.requires_grad and step.requires_grad and corr.requires_grad
    xd, dd = x.detach().double(), den.double()
    assert M.rel_l2(eps.detach(), M.eps64(xd, dd, sg.double())) < 1e-6
    assert M.rel_l2(step.detach(), M.step64(xd, dd, sg.double(), fwd["A_to_sigma"].float().double())) < 1e-6
    assert M.rel_l2(corr.detach(), M.correction64(xd, dd, sg.double(), fwd["A_prev_in"].double(), fwd["A_prev_sigma"].float().double(),
                                                  fwd["A_prev_eps"].double())) < 1e-6
    # scalar sigma (one value for the batch)
    with torch.enable_grad():
        p1 = PredictionBatch(denoised_xs=den, diffused_images=x, ts=torch.tensor([2.5]))
        assert M.rel_l2(p1.step(torch.tensor(1.0)).detach(), M.step64(xd, dd, torch.tensor([2.5]), torch.tensor([1.0]))) < 1e-6
