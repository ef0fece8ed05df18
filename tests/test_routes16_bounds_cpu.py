"""CPU: the bounds of tests/_routes16_ref64.py hold for an fp32 emulation of every route's arithmetic and reject the seeded defects, and
every case of tests/test_gpu_routes16.py claims the route the library's host queries give it.

The route check runs the GPU harness itself on CPU tensors with the launches stubbed out: ops.igemm then asks pmi_conv3x3_halo_config (under
the case's forced config), pmi_gemm_wd_eligible, pmi_gemm_wd_tile and pmi_igemm_splitk exactly as it does on the device, and the traced
description must give the case's claimed route string -- tile config, split-K factor, weights-direct tile rows / columns and all.  The
search for the smallest shape that still takes a route happens here, without a device."""
import pytest
import torch

import _routes16_ref64 as Q
import test_gpu_routes16 as T

REGIMES = ("coherent", "mixed")


# ---- claimed routes against the host queries -------------------------------------------------------------------------------------
@pytest.fixture
def dry(monkeypatch):
    """ops.igemm on CPU tensors: pointers are host pointers (the queries only test them against NULL), launches are dropped"""
    from perceptor_amd.engine import ops
    monkeypatch.setattr(ops, "ptr", lambda t: None if t is None else t.data_ptr())
    monkeypatch.setattr(ops, "call", lambda *a: None)
    monkeypatch.setattr(ops, "_traced_call", lambda name, args, desc, flops: ops.GEMM_TRACE.append((desc, flops, None, None)))


@pytest.mark.parametrize("name,dtype", T.PARAMS)
def test_claimed_route_matches_host_queries(dry, name, dtype):
    cs = T.CASES[name]
    _, route, st, _ = T.run_case(name, dtype, "cpu", launches=1)
    assert route == cs["route"], f"{name} {dtype}: the host queries give {route!r}, the case claims {cs['route']!r}"
    assert (st is not None) == cs["stats"], f"{name}: statistics rows {'missing' if cs['stats'] else 'unexpected'}"
    # the generic kernel's own rule, restated in _precise_ref64 (the conv-mode fall-back keeps the weights-direct GEMM's answer, 1: ops.igemm
    # asks pmi_igemm_splitk while Bf is still set and only then hands the unsplit call to the generic kernel)
    if " cfg=-1 " in route + " " and " wd=0" in route and not name.startswith("cw_"):
        og = T.out_grid(cs)
        m = cs["n"] * (og[0] * og[1] if og else 1)
        assert Q.generic_splitk(m, cs["cout"], cs["taps"] * sum(cs["srcs"])) == T.splitk_of(cs)


def test_route_table_covers_every_kernel_family():
    routes = {c["route"] for c in T.CASES.values()}
    for cfg in (0, 1, 2, 3, 4, 6, 7, 8):
        assert any(f" cfg={cfg} " in r for r in routes), cfg
    for need in ("cfg=6 sk=1", "cfg=7 sk=1", "wd=1 rows=128 cols=128 convmode", "two convmode", "rows=144 cols=256", "rows=128 cols=256",
                 "rows=128 cols=128 two", "geglu", "wd=1 splitk=", "wd=1 f32out", "conv taps=9 s2 cfg=-1", "conv taps=9 up cfg=-1",
                 "conv taps=9 cfg=-1 sk=1 wd=0 splitk="):
        assert any(need in r for r in routes), need
    assert {T.form_of(c) for c in T.CASES.values()} == set(Q.FORMS), set(Q.FORMS) - {T.form_of(c) for c in T.CASES.values()}
    for key in ("pitch", "stats", "nbias", "res_up", "up"):
        assert any(c[key] for c in T.CASES.values())
    assert any(c["prologue"] is not None and len(c["srcs"]) == 2 for c in T.CASES.values())
    assert {c["regime"] for c in T.CASES.values()} == {"coherent", "mixed", "tiny"}


# ---- the emulated routes are inside their bounds ---------------------------------------------------------------------------------
EMULATED = ["halo2_plain", "wd6_res_pitch", "wd7_two_pro", "wd8_c24_tail", "g_c24", "g_two_16_32", "g_splitk", "cw_12x20_rowtail", "w_res_f32",
            "w_out_f32", "w_128_cols_ntail", "g_tails"]


def _emulate(name, dtype, regime, **defect):
    cs, d = T.CASES[name], T.build_case(name, dtype, regime)
    form = defect.pop("form", T.form_of(cs))
    return Q.emulate(d["x"], d["w"], dtype=dtype, form=form, alpha=cs["alpha"], bias=d["bias"], nbias=d["nbias"], residual=d["res"],
                     res_up=cs["res_up"], act=cs["act"], stride=cs["stride"], up=cs["up"], out_f32=cs["out_f32"], **defect)


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("name", EMULATED)
def test_emulated_route_inside_bound(name, regime, dtype):
    d = T.build_case(name, dtype, regime)
    m = Q.margin(_emulate(name, dtype, regime), d["y"], d["tol"])
    print(f"[routes16-cpu] {name} {regime} {dtype}: form {T.form_of(T.CASES[name])}; emulated err/tol {m:.3f}")
    assert m <= 1.0, (name, regime, dtype, m)


def test_tiny_regime_emulation_inside_bound_and_subnormal():
    d = T.build_case("halo2_tiny", "f16")
    assert float((d["y"].abs() < Q.SUB_BELOW).double().mean()) > 0.5, "the tiny regime's outputs are not in f16's subnormal range"
    assert float((torch.cat(d["srcs"], -1).abs() < Q.SUB_BELOW).double().mean()) > 0.5
    assert Q.margin(_emulate("halo2_tiny", "f16", None), d["y"], d["tol"]) <= 1.0
    # a route that flushed subnormal results to zero is far outside the bound
    flushed = torch.where(d["y"].abs() < Q.SUB_BELOW, 0.0, d["y"])
    assert Q.margin(flushed, d["y"], d["tol"]) > 100


# ---- seeded defects ---------------------------------------------------------------------------------------------------------------
def _ref(name, dtype, regime, **over):
    """the float64 reference of a case with some operands replaced (a defect computed exactly)"""
    cs, d = T.CASES[name], T.build_case(name, dtype, regime)
    kw = dict(x=d["x"], w=d["w"], bias=d["bias"], nbias=d["nbias"], residual=d["res"])
    kw.update(over)
    x, w = kw.pop("x"), kw.pop("w")
    return Q.route_ref(x, w, dtype=dtype, form=T.form_of(cs), K=d["K"], splitk=T.splitk_of(cs), alpha=cs["alpha"], res_up=cs["res_up"],
                       act=cs["act"], stride=cs["stride"], up=cs["up"], out_f32=cs["out_f32"], **kw)[0]


def _rejected(tag, defect, name, dtype, regime="coherent"):
    d = T.build_case(name, dtype, regime)
    m = Q.margin(defect, d["y"], d["tol"])
    print(f"[routes16-defect] {tag} ({name} {regime} {dtype}): {m:.2f} x tol")
    assert m > 1.0, f"{tag}: the bound of {name} {dtype} does not reject this defect ({m:.3f} x tol)"


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", ["halo2_plain", "wd6_res_pitch", "cw_12x20_rowtail"])
def test_defect_tap_dropped_on_border_pixels(name, dtype):
    """the left neighbour's tap (dy 0, dx -1) missing on the first and last image row only"""
    d = T.build_case(name, dtype, "coherent")
    w = d["w"].clone()
    w[:, :, 1, 0] = 0
    bad = _ref(name, dtype, "coherent", w=w)
    y = d["y"].clone()
    y[:, 0], y[:, -1] = bad[:, 0], bad[:, -1]
    _rejected("tap dropped on border pixels", y, name, dtype)


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", ["wd6_res_pitch", "halo2_plain", "w_128_cols_ntail", "g_splitk"])
def test_defect_last_k_slice_dropped(name, dtype):
    """(shapes with K <= 1728 and no prologue: 32 of K = 4608 terms are 0.7 % of the product, under ONE bf16 rounding (0.4 %) of an output that
    also holds bias and residual, and a prologue's own allowance is 2 u of the product -- no bound on a bf16 result can see the slice there)"""
    d = T.build_case(name, dtype, "coherent")
    w = d["w"].clone()
    w[:, -32:, -1, -1] = 0                          # the last 32 channels of the last tap: the end of K
    _rejected("last 32-channel K slice dropped", _ref(name, dtype, "coherent", w=w), name, dtype)


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", ["wd7_two_pro", "halo0_two_tail", "g_two_16_32", "w_two_96", "cw_16x16_splitk_two"])
def test_defect_second_source_read_from_first(name, dtype):
    cs = T.CASES[name]
    c0 = cs["srcs"][0]
    for reg in ("mixed", "coherent"):               # (coherent: the second source lies one binade above the first)
        d = T.build_case(name, dtype, reg)
        if cs["prologue"] is None:
            x = d["x"].clone()
            x[..., c0:c0 + 8] = d["x"][..., 0:8]
        else:                                       # the prologue acts on what was read, with the second source's coefficients
            raw = torch.cat(d["srcs"], -1)
            raw[..., c0:c0 + 8] = raw[..., 0:8]
            x = Q.prologue_ref(raw, *d["pro"], dtype)
        _rejected("second source's first 8 channels read from the first", _ref(name, dtype, reg, x=x), name, dtype, reg)


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", ["wd7_dead_waves", "halo0_two_tail", "w_128_cols_ntail", "wd8_c24_tail", "g_tails"])
def test_defect_bias_missing_on_last_columns(name, dtype):
    d = T.build_case(name, dtype, "coherent")
    b = d["bias"].clone()
    b[-32:] = 0
    _rejected("bias missing on the last 32 columns", _ref(name, dtype, "coherent", bias=b), name, dtype)


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", ["halo1_res", "wd6_splitk", "cw_16x16_splitk_two", "g_two_16_32"])
def test_defect_per_sample_bias_of_the_neighbour(name, dtype):
    cs = T.CASES[name]
    reg = "coherent" if cs["n"] > 1 else "mixed"
    d = T.build_case(name, dtype, reg)
    nb = d["nbias"].roll(1, 0) if cs["n"] > 1 else d["nbias"].roll(1, 1)      # (one sample: the neighbouring column's)
    _rejected("per-sample bias of the neighbouring sample", _ref(name, dtype, reg, nbias=nb), name, dtype, reg)


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", ["halo0_two_tail", "wd6_splitk", "wd8_c24_tail", "g_up"])
def test_defect_upsampled_residual_rounded_up(name, dtype):
    """residual row (y + 1) >> 1 instead of y >> 1"""
    cs, d = T.CASES[name], T.build_case(name, dtype, "mixed")
    assert cs["res_up"]
    full = Q.res_grid(d["res"], True)
    shifted = torch.cat([full[:, 1:], full[:, -1:]], 1)
    bad = d["y"] - full + shifted
    _rejected("up-sampled residual indexed (y + 1) >> 1", bad, name, dtype, "mixed")


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", ["halo2_plain", "wd6_res_pitch", "g_splitk", "w_128_cols_ntail", "g_tails"])
def test_defect_truncated_result(name, dtype):
    _rejected("result truncated toward zero", _emulate(name, dtype, "coherent", trunc=True), name, dtype)


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("name", ["wd6_splitk", "cw_12x20_rowtail", "w_128_cols_ntail"])
def test_defect_rounding_after_every_chunk(name, dtype):
    _rejected("16-bit rounding after every 128-deep chunk", _emulate(name, dtype, "coherent", chunk_round=True), name, dtype)


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("form", ["reduce", "generic_slow", "halo3"])
def test_defect_two_roundings_on_a_one_rounding_route(form, dtype):
    """a one-rounding route running the two-rounding arithmetic: shows where residual and result have opposite signs (|a| >> |y|)"""
    d = T.build_case("g_tails", dtype, "coherent")
    x, w = d["x"], d["w"]
    _, _, p = Q.route_ref(x, w, dtype=dtype, form=form, K=d["K"], bias=d["bias"])
    res = -Q.rnd(p["a"] * 0.97, dtype)
    y, tol, _ = Q.route_ref(x, w, dtype=dtype, form=form, K=d["K"], bias=d["bias"], residual=res)
    good = Q.emulate(x, w, dtype=dtype, form=form, bias=d["bias"], residual=res)
    bad = Q.emulate(x, w, dtype=dtype, form=form, bias=d["bias"], residual=res, force_two=True)
    mg, mb = Q.margin(good, y, tol), Q.margin(bad, y, tol)
    print(f"[routes16-defect] two roundings on the one-rounding form {form} {dtype}: good {mg:.3f}, defect {mb:.2f} x tol")
    assert mg <= 1.0 and mb > 1.0, (mg, mb)
    # ... and the two-rounding form's own bound admits it
    y2, tol2, _ = Q.route_ref(x, w, dtype=dtype, form="gemm_wd", K=d["K"], bias=d["bias"], residual=res)
    assert Q.margin(bad, y2, tol2) <= 1.0


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_defect_k_tail_reads_the_next_row(dtype):
    """K = 136 = 2 x 64 + 8: an unmasked tail's next 8 k are the next row's first channels, in A and in B alike"""
    name = "g_tails"
    cs, d = T.CASES[name], T.build_case(name, dtype, "coherent")
    x, w = d["x"], d["w"]
    xe = torch.cat([x, torch.cat([x[1:, :8], torch.zeros(1, 8, dtype=x.dtype)], 0)], 1)
    we = torch.cat([w, torch.cat([w[1:, :8], torch.zeros(1, 8, 1, 1, dtype=w.dtype)], 0)], 1)
    bad = Q.route_ref(xe, we, dtype=dtype, form=T.form_of(cs), K=d["K"], bias=d["bias"], residual=d["res"], act=cs["act"])[0]
    _rejected("K tail reads the next row's first channels", bad, name, dtype)


def test_bound_not_vacuous_coherent():
    """coherent regime, no residual: the whole bound is one rounding u |y| plus the fp32 terms (|z| <= 2 |act(z)| for z >= 0.5)"""
    for name in ("wd7_up", "w_144_rows"):
        for dtype in T.DTYPES:
            cs, d = T.CASES[name], T.build_case(name, dtype, "coherent")
            rel = float((d["tol"] / d["y"].abs().clamp_min(1e-9)).max())
            lim = Q.U[dtype] + 2 * Q.ACT_HW[cs["act"]] + 2 * Q.ACT_LIP[cs["act"]] * Q.C_B * (d["K"] + Q.N_EPI) * Q.E32
            assert rel <= lim, (name, dtype, rel, lim)
