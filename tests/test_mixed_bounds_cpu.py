"""CPU: the bounds of tests/_mixed_ref64.py hold for an fp32 emulation of every mixed-mode route and reject the seeded defects; every
case of tests/test_gpu_mixed_routes.py keeps its share of rounding-uncertain operand elements under the cap and claims the route the
library's host queries give it.

Seeded defects (each must land outside the bound, margin > 1, in the regime named):
  (a) the input's low parts dropped before the prologue                       single and doubled, coherent
  (b) yl dropped                                                              doubled, coherent at Cin = 8 (the dropped parts are rounding
      residuals with random signs: their sum grows like sqrt(K), the accumulation term like K -- _mixed_ref64's module doc), and
      coherent_act at Cin = 32, where they all have one sign
  (c) padding pixels given silu(b) instead of zero                            both, mixed and coherent
  (d) sample 0's coefficients used for sample 1                               both, mixed
  (e) the second source's coefficients read at the physical offset 2 C0       both, mixed
  (f) the operand rounding truncating toward zero                             single, coherent
  (g) the residual's low half dropped; the fp32 residual read as a pair       coherent; mixed
  (h) the output's low half zeroed                                            both, mixed
  (i) projection: the residual read as [hi N | lo N] (its inner hi / lo groups swapped), its low half dropped, the output's low half zeroed
"""
import pytest
import torch

import _mixed_ref64 as X
import test_gpu_mixed_routes as T
from test_routes16_bounds_cpu import dry  # noqa: F401  (the fixture: ops entry points on CPU tensors, launches dropped)

OPERANDS = ("single", "dbl")


def _e(**kw):
    cs = dict(n=2, h=6, w=8, srcs=(32,), cout=16, up=False, res=None, res_up=False, nbias=False, regime="mixed", seed=3)
    cs.update(kw)
    return cs


# the emulated shapes: small (the arithmetic does not depend on the tiling), Cin = 32 as the smallest GPU case
EMU = {
    "plain": _e(),
    "two_nbias_split": _e(srcs=(16, 32), nbias=True, res="split"),
    "up_resup": _e(h=4, w=4, up=True, res="split", res_up=True),
    "f32": _e(res="f32"),
    "c8": _e(srcs=(8,)),            # the shortest chain (K = 144 doubled): where a random-sign sum over K stands clear of the K E32 term
}


def _case(variant, regime):
    return dict(EMU[variant], regime=regime)


# ---- claimed routes against the host queries ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,operand", T.PARAMS)
def test_claimed_route_matches_host_queries(dry, name, operand):
    cs = T.CASES[name]
    _, route, _, traced, st = T.run_case(name, operand, "cpu", launches=1)
    fb = operand in cs["fallback"]
    assert route == ("fallback" if fb else "wd"), f"{name} {operand}: the host queries give {route!r}"
    assert (st is not None) == (not fb or cs["cfg"] >= 0), f"{name} {operand}: statistics rows"
    if fb and cs["cfg"] < 0:       # the generic kernel's split-K rule as _precise_ref64 restates it (the bound's chain length comes from the trace)
        ho, wo = (2 * cs["h"], 2 * cs["w"]) if cs["up"] else (cs["h"], cs["w"])
        assert T._splitk_of(traced) == X.generic_splitk(cs["n"] * ho * wo, cs["cout"], 18 * sum(cs["srcs"])), traced


@pytest.mark.parametrize("name", list(T.PROJ_CASES))
def test_projection_route_matches_host_queries(dry, name):
    cs = T.PROJ_CASES[name]
    _, _, route, sk = T.run_proj(name, "cpu", launches=1)
    assert route == cs["route"], (name, route)
    assert sk == X.generic_splitk(cs["m"], cs["n"], cs["k"]) and (sk > 1) == (cs["route"] == T.PROJ_ROUTE_SK)


def test_case_table_covers_what_the_issue_names():
    keys = {T.case_key(cs, op) for cs in T.CASES.values() for op in cs["operands"]}
    for cfg in (6, 7):
        for op in OPERANDS:
            for nsrc, up, res, nb in ((1, False, "none", False), (1, False, "split", False), (1, False, "f32", False), (1, False, "none", True),
                                      (2, False, "f32", False), (2, False, "none", False), (1, True, "split_up", False), (1, True, "none", False),
                                      (1, False, "split_up", False)):
                assert ("wd", cfg, op, nsrc, up, res, nb) in keys, (cfg, op, nsrc, up, res, nb)
            assert any(cs["cfg"] == cfg and cs["regime"] == "wide" and op in cs["operands"] and op not in cs["fallback"] for cs in T.CASES.values())
    assert ("fallback", -1, "any", 1, False, "f32", False) in keys


# ---- the share of rounding-uncertain operand elements ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.CASES))
def test_amb_share_under_cap(name):
    cs = T.CASES[name]
    p, delta = X.activated(T.inputs(name))
    _, _, amb = X.ambiguous(p, delta)
    share = float(amb.double().mean())
    print(f"[mixed-cpu] {name} ({cs['regime']}): amb share {100 * share:.3f} %")
    assert share <= X.AMB_CAP[cs["regime"]], (name, share)


def test_regimes_hold_what_the_defects_need():
    for regime in X.AMB_CAP:
        d = X.build_inputs(_case("plain", regime))
        assert float(d["b"].abs().max()) >= 1.0 and float((d["a"][1] - d["a"][0]).abs().mean()) >= 0.3
    d = X.build_inputs(_case("plain", "wide"))
    u = d["a"].double()[:, None, None, :] * (d["hi"] + d["lo"]) + d["b"].double()[:, None, None, :]
    p, _ = X.activated(d)
    assert float(u.min()) < -12 and float(u.max()) > 12, (float(u.min()), float(u.max()))
    assert bool(((p.abs() < X.SUB_BELOW) & (p != 0)).any()), "the wide regime reaches no f16 subnormal"
    d = X.build_inputs(_case("plain", "coherent_act"))
    p, _ = X.activated(d)
    yl = p - p.half().double()
    assert bool((yl > 0).all()) and float((yl / p).min()) > 0.5 * 2.0 ** -12, "coherent_act: the staged low parts are not coherent"


# ---- emulations inside the bounds ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("operand", OPERANDS)
@pytest.mark.parametrize("regime", list(X.AMB_CAP))
@pytest.mark.parametrize("variant", list(EMU))
def test_emulated_conv_inside_bound(variant, regime, operand):
    cs = _case(variant, regime)
    d = X.build_inputs(cs)
    y, tol, info = X.conv_ref(d, cs, operand)
    m = X.margin(X.emulate_conv(d, cs, operand), y, tol)
    print(f"[mixed-cpu] {variant} {regime} {operand}: emulated err/tol {m:.3f}, amb share {100 * info['amb']:.3f} %")
    assert m <= 1.0, (variant, regime, operand, m)
    assert info["amb"] <= X.AMB_CAP[regime]


@pytest.mark.parametrize("regime", list(X.AMB_CAP))
def test_emulated_operand_flips_only_inside_amb(regime):
    cs = _case("plain", regime)
    d = X.build_inputs(cs)
    p, delta = X.activated(d)
    x, _, amb = X.ambiguous(p, delta)
    u32 = torch.addcmul(d["b"][:, None, None, :], d["hi"].float() + d["lo"].float(), d["a"][:, None, None, :])
    x32 = (u32 / (1 + torch.exp(-u32))).half().double()
    flips = x32 != x
    print(f"[mixed-cpu] {regime}: {100 * float(flips.double().mean()):.4f} % of the fp32 operands round to the other neighbour, amb {100 * float(amb.double().mean()):.3f} %")
    assert not bool((flips & ~amb).any()), "an fp32 operand rounds differently outside the uncertain set"


def test_emulated_fallback_inside_bound():
    cs = _case("f32", "mixed")
    d = X.build_inputs(cs)
    y, tol, _ = X.conv_ref(d, cs, "single", fallback=True, splitk=2)
    rh, rl = X._split32(d["res"])                      # pmi_split_from_f32, then the split residual's two additions
    d2, cs2 = dict(d, res_hi=rh, res_lo=rl, res=X.join_split(rh, rl)), dict(cs, res="split")
    assert X.margin(X.emulate_conv(d2, cs2, "dbl"), y, tol) <= 1.0


# ---- seeded defects ----------------------------------------------------------------------------------------------------------------
DEFECTS = [
    # id, variant, regime, operand, defect
    ("a_single", "plain", "coherent", "single", dict(drop_in_lo=True)),
    ("a_dbl", "plain", "coherent", "dbl", dict(drop_in_lo=True)),
    ("b_dbl", "c8", "coherent", "dbl", dict(drop_yl=True)),
    ("b_dbl_act", "plain", "coherent_act", "dbl", dict(drop_yl=True)),
    ("c_single_mixed", "plain", "mixed", "single", dict(pad_silu=True)),
    ("c_dbl_mixed", "plain", "mixed", "dbl", dict(pad_silu=True)),
    ("c_single_coherent", "plain", "coherent", "single", dict(pad_silu=True)),
    ("c_dbl_coherent", "plain", "coherent", "dbl", dict(pad_silu=True)),
    ("d_single", "plain", "mixed", "single", dict(same_coef=True)),
    ("d_dbl", "plain", "mixed", "dbl", dict(same_coef=True)),
    ("e_single", "two_nbias_split", "mixed", "single", dict(coef_shift=True)),
    ("e_dbl", "two_nbias_split", "mixed", "dbl", dict(coef_shift=True)),
    ("f_single", "plain", "coherent", "single", dict(trunc=True)),
    ("g_lo_single", "two_nbias_split", "coherent", "single", dict(res_drop_lo=True)),
    ("g_lo_dbl", "up_resup", "coherent", "dbl", dict(res_drop_lo=True)),
    ("g_f32_single", "f32", "mixed", "single", dict(res_f32_as_split=True)),
    ("g_f32_dbl", "f32", "mixed", "dbl", dict(res_f32_as_split=True)),
    ("h_single", "plain", "mixed", "single", dict(out_drop_lo=True)),
    ("h_dbl", "two_nbias_split", "mixed", "dbl", dict(out_drop_lo=True)),
]


@pytest.mark.parametrize("tag,variant,regime,operand,defect", DEFECTS, ids=[t[0] for t in DEFECTS])
def test_seeded_conv_defect_outside_bound(tag, variant, regime, operand, defect):
    cs = _case(variant, regime)
    d = X.build_inputs(cs)
    y, tol, _ = X.conv_ref(d, cs, operand)
    good = X.margin(X.emulate_conv(d, cs, operand), y, tol)
    bad = X.margin(X.emulate_conv(d, cs, operand, **defect), y, tol)
    print(f"[mixed-cpu] defect {tag} ({regime}, {operand}): err/tol {bad:.2f} (emulation {good:.3f})")
    assert good <= 1.0 < bad, (tag, good, bad)


# the subtle defects on the GPU cases' own inputs: the device test sees them only where the bound at the case's K is tighter than the defect
ON_GPU_CASES = [("c7_one_tile", "dbl", dict(drop_in_lo=True)), ("c6_one_tile_32", "dbl", dict(drop_in_lo=True)),
                ("c7_one_tile_el", "single", dict(drop_in_lo=True)), ("c6_one_tile", "single", dict(drop_in_lo=True)),
                ("c7_act", "dbl", dict(drop_yl=True)), ("c6_act", "dbl", dict(drop_yl=True)),
                ("c7_one_tile_el", "single", dict(trunc=True)), ("c6_one_tile", "single", dict(trunc=True)),
                ("c7_epi_split", "dbl", dict(res_drop_lo=True)), ("c6_epi_nbias", "single", dict(out_drop_lo=True))]


@pytest.mark.parametrize("name,operand,defect", ON_GPU_CASES, ids=[f"{n}-{o}-{next(iter(k))}" for n, o, k in ON_GPU_CASES])
def test_gpu_case_rejects_its_subtle_defect(name, operand, defect):
    cs, d = T.CASES[name], T.inputs(name)
    y, tol, _ = X.conv_ref(d, cs, operand)
    good = X.margin(X.emulate_conv(d, cs, operand, chunk=16 if operand == "dbl" and cs["cfg"] == 7 else 32), y, tol)
    bad = X.margin(X.emulate_conv(d, cs, operand, **defect), y, tol)
    print(f"[mixed-cpu] {name} {operand} {defect}: err/tol {bad:.2f} (emulation {good:.3f})")
    assert good <= 1.0 < bad, (name, good, bad)


@pytest.mark.parametrize("name", list(T.PROJ_CASES))
def test_emulated_projection_inside_bound_and_defects_outside(name):
    cs = T.PROJ_CASES[name]
    d = X.proj_inputs(cs)
    sk = X.generic_splitk(cs["m"], cs["n"], cs["k"])
    y, tol = X.proj_ref(d, sk)
    good = X.margin(X.emulate_proj(d, splitk=sk), y, tol)
    print(f"[mixed-cpu] {name}: emulated err/tol {good:.3f}")
    assert good <= 1.0, (name, good)
    for defect in ("res_groups_swapped", "res_drop_lo", "out_drop_lo"):
        bad = X.margin(X.emulate_proj(d, splitk=sk, **{defect: True}), y, tol)
        print(f"[mixed-cpu] {name} defect {defect}: err/tol {bad:.2f}")
        assert bad > 1.0, (name, defect, bad)
