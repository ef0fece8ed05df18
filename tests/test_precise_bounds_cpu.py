"""CPU: the precise-mode packing restated in float64, the defects the bounds of tests/_precise_ref64.py must reject (each at the
inputs of a GPU case of test_gpu_precise_kernels.py, at least 2x outside its bound), and the coverage of the GPU case tables."""
import os
import re

import pytest
import torch

import _precise_ref64 as P
import test_gpu_precise_kernels as T
from _precise_ref64 import ACT_NONE

REJECT = 2.0


def _lin(w, sources=None, **kw):
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    return ops.PackedLinear(w, None, _hip.DT_F16X2, "cpu", sources=sources, **kw)


def _physical(lin, srcs):
    """the physical K operand of a packed layer: the sources' split tensors side by side, twice for self_concat"""
    a = torch.cat([s.double() for s in srcs], -1)
    return torch.cat([a, a], -1) if lin.self_concat else a


def _packed_w(lin, k):
    return lin.w.double().view(lin.n_p, k * k, lin.cin_p).permute(0, 2, 1).reshape(lin.n_p, lin.cin_p, k, k)


@pytest.mark.parametrize("srcs,wk,k", [((32,), "f16", 3), ((24,), "f32", 3), ((16, 32), "f16", 3), ((32, 64), "f32", 3),
                                       ((8,), "f32", 3), ((64,), "f32", 1), ((32, 32), "f32", 1)])
def test_packing_reproduces_hi_lo_products(srcs, wk, k):
    """PackedLinear(DT_F16X2) weights against the physical split operand == W_hi (x_hi + x_lo) + W_lo x_hi in float64"""
    lead = (2, 6, 6)
    phys, his, los = [], [], []
    for i, c in enumerate(srcs):
        hi, lo = P.mixed_hi_lo(lead + (c,), 40 + i)
        phys.append(P.join_split(hi, lo))
        his.append(hi.double())
        los.append(lo.double())
    w = P.weights((32, sum(srcs), k, k), 41, "mixed", wk)
    lin = _lin(w, list(srcs) if len(srcs) > 1 else None)
    assert lin.self_concat == (wk == "f32")
    assert lin.concat_inputs == (wk == "f32" and len(srcs) > 1)
    got = P.conv64(_physical(lin, phys), _packed_w(lin, k))
    wh, wl = P.weight_parts(w, lin.self_concat)
    x_hi, x_lo = torch.cat(his, -1), torch.cat(los, -1)
    want = P.conv64(x_hi + x_lo, wh) + P.conv64(x_hi, wl)
    scale = P.conv64((x_hi + x_lo).abs(), wh.abs()) + P.conv64(x_hi.abs(), wl.abs())
    assert float(((got[..., :32] - want).abs() / (scale + 1e-300)).max()) <= 2.0 ** -48


def test_two_source_groupings_not_32_keep_warning():
    """sources that do not concatenate into one [hi 32 | lo 32] tensor: the two-pointer layer, its fp32 weights rounded (warned)"""
    w = P.weights((32, 24, 3, 3), 43, "mixed", "f32")
    with pytest.warns(UserWarning):
        lin = _lin(w, [8, 16])
    assert not lin.self_concat
    with pytest.warns(UserWarning):
        lin = _lin(P.weights((32, 64, 3, 3), 44, "mixed", "f32"), [32, 32], concat_sources=False)
    assert not lin.self_concat


@pytest.mark.parametrize("dup_g", [16, 32])
def test_frag16_dup_g_order(dup_g):
    """frag16(ck, dup_g): per source, groups of dup_g logical channels as [W | W] -- undo the fragment permutation and compare"""
    srcs = [64, 32]
    w = P.weights((128, 96, 3, 3), 45, "mixed", "f16")
    lin = _lin(w, srcs)
    fr = lin.frag16(64, dup_g=dup_g)
    inv = [0, 5, 7, 4, 2, 1, 3, 6, 8]          # inverse of frag16's permute(0, 5, 4, 6, 3, 1, 7, 2, 8)
    flat = fr.view(lin.n_p // 32, lin.cin_p // 64, 3, 2, 3, 2, 4, 16, 8).permute(*inv).reshape(lin.n_p, 9, lin.cin_p)
    parts, o = [], 0
    w9 = w.permute(0, 2, 3, 1).reshape(128, 9, 96).half().float()
    for cs in srcs:
        blk = w9[:, :, o:o + cs].reshape(128, 9, cs // dup_g, 1, dup_g).expand(-1, -1, -1, 2, -1)
        parts.append(blk.reshape(128, 9, 2 * cs))
        o += cs
    assert torch.equal(flat.float(), torch.cat(parts, 2))


# ---- defect rejection at the GPU cases' inputs ---------------------------------------------------------------------------------------
def _case(name):
    cs = T.CONV_CASES[name]
    return cs, T.build_case(cs)


def _ref(cs, d, **over):
    kw = dict(self_concat=d["lin"].self_concat, bias=d["bpad"], nbias=d["nbias"], residual=d["res_log"], res_up=cs["res_up"],
              act=cs["act"], stride=cs["stride"], up=cs["up"], split_out=not cs["out_f32"], chain=1)
    x_hi, x_lo = over.pop("x_hi", d["x_hi"]), over.pop("x_lo", d["x_lo"])
    kw.update(over)
    return P.precise_ref(x_hi, x_lo, d["wpad"], **kw)[0]


def _assert_rejected(defect, d, tag):
    m = P.margin(defect, d["y"], d["tol"])
    print(f"[defect] {tag}: {m:.1f} x tol")
    assert m >= REJECT, f"{tag}: the bound does not reject this defect ({m:.2f} x tol)"


def test_defect_activation_lo_dropped():
    cs, d = _case("g3x3_relu_res")
    _assert_rejected(_ref(cs, d, x_lo=torch.zeros_like(d["x_lo"])), d, "activation lo dropped")


@pytest.mark.parametrize("name", ["g3x3_s2_f32w", "g_first_f32w_c8", "g_up_resup_f32w"])
def test_defect_weight_low_block_dropped(name):
    cs, d = _case(name)
    assert cs["regime"] == "coherent"
    _assert_rejected(_ref(cs, d, self_concat=False), d, f"{name}: weight low block dropped")


def test_defect_lo_block_wrong_group_offset():
    """the second K block's weights at the lo offset (+G) of each group: W_lo x_lo instead of W_lo x_hi"""
    cs, d = _case("g3x3_s2_f32w")
    wh, wl = P.weight_parts(d["wpad"], True)
    v = d["x_hi"] + d["x_lo"]
    acc = P.conv64(v, wh, stride=2) + P.conv64(d["x_lo"], wl, stride=2) + d["bpad"].double()
    _assert_rejected(acc, d, "lo block at the wrong group offset")


@pytest.mark.parametrize("name", ["g3x3_relu_res", "wd7_auto", "sk_linear", "g1x1_g8_out"])
def test_defect_output_lo_not_written(name):
    cs, d = _case(name)
    hi = d["y"].float().half().double()
    _assert_rejected(hi, d, f"{name}: output lo not written")


def _slabs(cs, d):
    """the S split-K slabs of a linear case over the physical K (contiguous ranges, as the generic kernel's grid.z splits it)"""
    lin, S = d["lin"], d["splitk"]
    A = _physical(lin, d["srcs"]).reshape(-1, lin.cin_p)
    B = lin.w.double()
    step = -(-lin.K // S)
    return [A[:, s * step:(s + 1) * step] @ B[:, s * step:(s + 1) * step].T for s in range(S)]


def test_defect_splitk_slabs_rounded_to_f16():
    cs, d = _case("sk_linear")
    slabs = _slabs(cs, d)
    assert len(slabs) == 2
    y = sum(s.float().half().double() for s in slabs) + d["bpad"].double() + d["res_log"]
    _assert_rejected(y, d, "split-K slabs rounded to f16")


def test_defect_bias_once_per_slab():
    cs, d = _case("sk_linear")
    _assert_rejected(d["y"] + (d["splitk"] - 1) * d["bpad"].double(), d, "bias added once per slab")


@pytest.mark.parametrize("name", ["g1x1_g24_nbias_silu", "g1x1_g8_out", "g_up_resup_f32w"])
def test_defect_split_off_g32_on_narrow_tensor(name):
    """the kernel stores the output with G = 32 groups ([hi 32 | lo 32]) into a tensor whose consumers read G = C (8 / 16 / 24): the hi
    part of channel c lands at c and its lo at c + 32 -- past the 2C-wide row for c >= C - 32 + C, i.e. into the next pixel's hi parts"""
    cs, d = _case(name)
    y = d["y"].float()
    C = y.shape[-1]
    assert C in (8, 16, 24)
    hi = y.half()
    lo = (y - hi.float()).half()
    flat = torch.zeros(y.numel() * 2 + 64, dtype=torch.float16)
    rows = y.reshape(-1, C)
    for r in range(rows.shape[0]):                 # G = 32 offsets: hi at c, lo at c + 32, row pitch 2C
        base = r * 2 * C
        flat[base:base + C] = hi.reshape(-1, C)[r]
        flat[base + 32:base + 32 + C] = lo.reshape(-1, C)[r]
    phys = flat[:y.numel() * 2].view(y.shape[:-1] + (2 * C,))
    _assert_rejected(P.from_split16(phys), d, f"{name}: split_off with G = 32 on {C} channels")


def test_defect_residual_lo_dropped():
    cs, d = _case("g3x3_relu_res")
    r_hi, _ = P.parts(d["res"])
    _assert_rejected(_ref(cs, d, residual=r_hi), d, "residual lo dropped")


def test_defect_fp32_residual_through_f16():
    cs, d = _case("c3_plain_k")
    _assert_rejected(_ref(cs, d, residual=d["res_log"].float().half().double()), d, "fp32 residual passed through f16")


def test_defect_two_source_f32_weights_rounded():
    """the behaviour before the concatenated self_concat layer: fp32 weights of a two-source convolution rounded to f16"""
    for name in ("g_two_sources_f32w",):        # (coherent, K = 2304: the longer-K two-source cases are too loose to see it)
        cs, d = _case(name)
        assert d["lin"].self_concat and len(cs["srcs"]) == 2
        _assert_rejected(_ref(cs, d, self_concat=False), d, f"{name}: two-source fp32 weights rounded to f16")


def test_defect_gemm_f32_k_tail_dropped():
    M, N, K, transB, alpha, has_bias, act, has_res, _ = T.F32_CASES["k77_relu"]
    A, B = T._f32_operands(M, N, K, transB, 7)
    ref, tol = T._f32_ref(A, B, transB, alpha, None, act, None)
    k = K // 32 * 32
    bad, _ = T._f32_ref(A[:, :k], B[:, :k], transB, alpha, None, act, None)
    m = P.margin(bad, ref, tol)
    assert m >= REJECT, m


def test_defect_gemm_f32_batch_inner_strides_swapped():
    """outer and inner batch strides of A exchanged: z = (zo, zi) reads A at zo * sA_i + zi * sA_o"""
    M, N, K, bo, bi, sA, sB, sD, lda, ldb, ldd = T.BATCH_GEOM
    Ab, Bb = T.batch_operands()
    checked = 0
    for zo in range(bo):
        for zi in range(bi):
            off, off2 = zo * sA[0] + zi * sA[1], zo * sA[1] + zi * sA[0]
            if off2 == off or off2 + M * lda > Ab.numel():
                continue
            a, a2 = (torch.as_strided(Ab, (M, K), (lda, 1), o) for o in (off, off2))
            b = torch.as_strided(Bb, (N, K), (ldb, 1), zo * sB[0] + zi * sB[1])
            ref, tol = T._f32_ref(a, b, False, 1.0, None, ACT_NONE, None)
            bad, _ = T._f32_ref(a2, b, False, 1.0, None, ACT_NONE, None)
            assert P.margin(bad, ref, tol) >= REJECT, (zo, zi)
            checked += 1
    assert checked >= 2


def test_bound_not_vacuous_coherent():
    """the coherent cases' bound stays under the lost-lo effect (~2^-12 relative): below 1e-4 of |y| at their K"""
    for name, cs in T.CONV_CASES.items():
        if cs["regime"] != "coherent" or cs["res"] or cs["prologue"] is not None:
            continue
        d = T.build_case(cs)
        rel = float((d["tol"] / d["y"].abs().clamp_min(1e-6)).max())
        lim = 1.6 * P.C_B * (P.chain_len(d["lin"].K, d["splitk"]) + 4) * P.E32 + 2 * P.U_SPLIT
        assert rel <= lim, (name, rel, lim)


# ---- coverage of the GPU case tables --------------------------------------------------------------------------------------------------
def _any(pred):
    return any(pred(c) for c in T.CONV_CASES.values())


def _route(c, *parts):
    return all(p in c["route"].split() for p in parts)


REQUIRED = {
    "generic 3x3": lambda c: _route(c, "conv", "taps=9", "cfg=-1", "sk=0", "split_out"),
    "generic 1x1": lambda c: _route(c, "gemm", "taps=1", "cfg=-1", "wd=0", "split_out"),
    "generic stride 2 (3x3 and 1x1)": lambda c: c["stride"] == 2 and c["taps"] == 1,
    "generic stride 2 3x3": lambda c: c["stride"] == 2 and c["taps"] == 9,
    "generic up": lambda c: c["up"] and _route(c, "cfg=-1"),
    "generic res_up": lambda c: c["res_up"] and _route(c, "cfg=-1", "sk=0"),
    "generic nbias": lambda c: c["nbias"] and _route(c, "cfg=-1", "sk=0"),
    "generic ReLU": lambda c: c["act"] == 1 and _route(c, "cfg=-1"),
    "generic SiLU": lambda c: c["act"] == 2 and _route(c, "cfg=-1"),
    "generic split residual": lambda c: c["res"] == "split" and _route(c, "cfg=-1", "sk=0"),
    "generic fp32 residual": lambda c: c["res"] == "f32" and _route(c, "cfg=-1"),
    "generic out_f32": lambda c: c["out_f32"] and _route(c, "cfg=-1", "wd=0"),
    "output G=8": lambda c: not c["out_f32"] and c["cout"] == 8,
    "output G=16": lambda c: not c["out_f32"] and c["cout"] == 16,
    "output G=24": lambda c: not c["out_f32"] and c["cout"] == 24,
    "output G=32": lambda c: not c["out_f32"] and c["cout"] % 32 == 0,
    "two sources, own groupings": lambda c: len(c["srcs"]) == 2 and len({P.group_of(s) for s in c["srcs"]}) == 2,
    "M / N / K tails": lambda c: c["linear"] and c["n"] % 128 and c["cout"] % 128 and (2 * sum(c["srcs"])) % 64,
    "split-K + reduce, split output": lambda c: _route(c, "sk=1", "split_out"),
    "config 6 forced": lambda c: _route(c, "cfg=6") and c["force"] == 6,
    "config 6 picked": lambda c: _route(c, "cfg=6") and c["force"] is None,
    "config 7 forced": lambda c: _route(c, "cfg=7") and c["force"] == 7,
    "config 7 picked": lambda c: _route(c, "cfg=7") and c["force"] is None,
    "config 6/7 split residual": lambda c: _route(c, "split_out") and c["res"] == "split" and ("cfg=6" in c["route"] or "cfg=7" in c["route"]),
    "config 6/7 fp32 residual": lambda c: c["res"] == "f32" and ("cfg=6" in c["route"] or "cfg=7" in c["route"]),
    "config 6/7 res_up": lambda c: c["res_up"] and ("cfg=6" in c["route"] or "cfg=7" in c["route"]),
    "config 6/7 nbias": lambda c: c["nbias"] and ("cfg=6" in c["route"] or "cfg=7" in c["route"]),
    "config 6/7 statistics": lambda c: c["stats"] and ("cfg=6" in c["route"] or "cfg=7" in c["route"]),
    "config 8": lambda c: _route(c, "cfg=8", "split_in", "split_out"),
    "config 3 plain_k": lambda c: _route(c, "cfg=3", "f32out", "split_in"),
    "gemm_wd split weights out_f32": lambda c: _route(c, "wd=1", "f32out", "split_in"),
    "self_concat generic": lambda c: _route(c, "cfg=-1", "sk=0", "self_concat"),
    "self_concat split-K": lambda c: _route(c, "sk=1", "self_concat"),
    "self_concat config 6": lambda c: _route(c, "cfg=6", "self_concat"),
    "self_concat config 7": lambda c: _route(c, "cfg=7", "self_concat"),
    "self_concat config 3": lambda c: _route(c, "cfg=3", "self_concat"),
    "self_concat first convolution (C0 <= 32)": lambda c: _route(c, "self_concat") and sum(c["srcs"]) <= 16 and c["cout"] % 128 == 0,
    "self_concat two sources": lambda c: _route(c, "self_concat") and len(c["srcs"]) == 2,
    "prologue, one source": lambda c: c["prologue"] is not None and len(c["srcs"]) == 1,
    "prologue, two sources": lambda c: c["prologue"] is not None and len(c["srcs"]) == 2,
}


@pytest.mark.parametrize("what", list(REQUIRED))
def test_route_covered(what):
    assert _any(REQUIRED[what]), f"no GPU case covers: {what}"


def test_every_engine_route_is_a_case():
    covered = {c["route"] for c in T.CONV_CASES.values()}
    assert T.ENGINE_ROUTES and set(T.ENGINE_ROUTES) <= covered, sorted(set(T.ENGINE_ROUTES) - covered)


def test_every_entry_point_is_exercised():
    src = open(os.path.join(os.path.dirname(__file__), "test_gpu_precise_kernels.py")).read()
    for name in ("pmi_split_from_f32", "pmi_split_to_f32", "ops.split_convert", "ops.gemm_f32", "ops.linear_f32", "ops.igemm",
                 "pmi_conv3x3_halo_config"):
        assert name in src, name
    assert any(c["prologue"] is not None for c in T.CONV_CASES.values())       # pmi_gn_apply through ops.igemm
    for c in T.CONV_CASES.values():                                            # both regimes where it matters
        assert c["regime"] in ("coherent", "mixed")
    assert {c["regime"] for c in T.CONV_CASES.values()} == {"coherent", "mixed"}
    assert re.search(r"def test_gemm_f32_batch_strides", src)


def test_fp16_torso_rule_matches_reference_fixture():
    """the census's fp16_torso rule names exactly the tensors the reference's convert_to_fp16 rounded (fixture adm_tiny_a_fp16w)"""
    from conftest import golden
    from perceptor_amd.engine import adm
    from perceptor_amd.utils.synth import synth_state_dict
    from test_gpu_adm import TINY
    g = golden("adm_tiny_a_fp16w")
    cfg = adm.AdmConfig(**TINY["a"])
    sd = synth_state_dict(adm.state_dict_shapes(cfg), 0, rounding="none")
    assert sorted(T.fp16_torso_keys(sd)) == sorted(g["rounded_keys"].tolist())
