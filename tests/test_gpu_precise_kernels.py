"""GPU: the precise-mode (dtype 2, hi + lo f16 pairs) GEMM / convolution routes, the exact-fp32 GEMM and the split conversions one
at a time against float64 (references and bounds: tests/_precise_ref64.py).

Every call runs on NaN-filled outputs and scratch with a NaN guard past the logical end (ops-level allocations): outputs must come
back finite, guards untouched, and two launches give the same bits.  Each case names the route it claims (the GEMM_TRACE key of
the call: kernel config, split-K, weights-direct GEMM, split / self_concat flags) and the route must match.  The route census
runs the precise engines and requires every route they take to be one a case here covers.
"""
import contextlib
import math
import random
import warnings

import pytest
import torch

import _precise_ref64 as P
from _precise_ref64 import ACT_NONE, ACT_RELU, ACT_SILU

pytestmark = pytest.mark.gpu


def _c(route, **kw):
    cs = dict(n=1, h=8, w=8, srcs=(32,), cout=32, taps=9, stride=1, up=False, wk="f16", regime="coherent", bias=True, nbias=False,
              res=None, res_up=False, res_scale=1.0, act=ACT_NONE, out_f32=False, force=None, linear=False, stats=False, prologue=None, seed=1)
    cs.update(kw)
    if cs["linear"]:
        cs["taps"] = 1
    cs["route"] = route
    return cs


G3, G3SC = "conv taps=9 cfg=-1 sk=0 wd=0 split_in split_out", "conv taps=9 cfg=-1 sk=0 wd=0 split_in split_out self_concat"
GM, GMSC = "gemm taps=1 cfg=-1 sk=0 wd=0 split_in split_out", "gemm taps=1 cfg=-1 sk=0 wd=0 split_in split_out self_concat"
# logical channel counts; a case's route is the GEMM_TRACE key (route_key) the call must produce
CONV_CASES = {
    # generic implicit-GEMM kernel (igemm.hip), split epilogue
    "g3x3_relu_res": _c(G3, n=2, act=ACT_RELU, res="split", res_scale=1024.0),
    "g3x3_mixed": _c(G3, n=2, regime="mixed", act=ACT_SILU, res="split", nbias=True),
    "g3x3_s2_f32w": _c("conv taps=9 s2 cfg=-1 sk=0 wd=0 split_in split_out self_concat", n=2, h=16, w=16, stride=2, srcs=(16,), wk="f32"),
    "g3x3_s2_mixed": _c("conv taps=9 s2 cfg=-1 sk=0 wd=0 split_in split_out", n=2, h=16, w=16, stride=2, srcs=(24,), cout=16,
                        regime="mixed", act=ACT_SILU),
    "g1x1_s2": _c("conv taps=1 s2 cfg=-1 sk=0 wd=0 split_in split_out", n=2, h=16, w=16, stride=2, taps=1, srcs=(64,), cout=32),
    "g1x1_g24_nbias_silu": _c(GM, n=2, taps=1, srcs=(24,), cout=24, nbias=True, act=ACT_SILU, regime="mixed"),
    "g1x1_g8_out": _c(GMSC, n=2, taps=1, srcs=(32,), cout=8, wk="f32", res="split"),
    "g_up_resup_f32w": _c("conv taps=9 up cfg=-1 sk=0 wd=0 split_in split_out self_concat", n=1, h=4, w=4, up=True, srcs=(8,), cout=16,
                          wk="f32", res="split", res_up=True, act=ACT_SILU),
    "g_up_mixed": _c("conv taps=9 up cfg=-1 sk=0 wd=0 split_in split_out", n=2, h=4, w=4, up=True, srcs=(32,), cout=32, regime="mixed",
                     res="split"),
    "g_two_sources": _c(G3, n=2, srcs=(16, 32), cout=32, res="split"),
    "g_two_sources_f32w": _c("conv taps=9 cfg=-1 sk=1 wd=0 split_in split_out self_concat", n=2, srcs=(32, 32), cout=32, wk="f32"),
    "g_two_sources_1x1_f32w": _c(GMSC, n=2, taps=1, srcs=(32, 64), cout=64, wk="f32", regime="mixed"),
    "g_tails_linear": _c(GM, linear=True, n=200, srcs=(24,), cout=24, act=ACT_RELU),
    "g_tails_linear_f32w": _c(GMSC, linear=True, n=77, srcs=(16,), cout=8, wk="f32", regime="mixed"),
    "g_outf32_skip": _c("gemm taps=1 cfg=-1 sk=0 wd=0 f32out split_in self_concat", n=2, taps=1, srcs=(32, 32), cout=3, wk="f32",
                        out_f32=True, bias=False),
    "g_outf32_skip_two": _c("gemm taps=1 cfg=-1 sk=0 wd=0 f32out split_in", n=2, taps=1, srcs=(32, 64), cout=3, out_f32=True,
                            regime="mixed"),
    "g_outf32_3x3_res": _c("conv taps=9 cfg=-1 sk=0 wd=0 f32out split_in", srcs=(32,), cout=3, out_f32=True, res="f32"),
    "g_first_f32w_c8": _c(G3SC, n=1, h=8, w=32, srcs=(8,), cout=128, wk="f32", force=8),
    # split-K: generic slabs + splitk_reduce_kernel writing split output
    "sk_linear": _c("gemm taps=1 cfg=-1 sk=1 wd=0 split_in split_out", linear=True, n=128, srcs=(512,), cout=128, res="split"),
    "sk_conv_f32w": _c("conv taps=9 cfg=-1 sk=1 wd=0 split_in split_out self_concat", srcs=(64,), cout=64, wk="f32", nbias=True,
                       res="split", res_up=True, regime="mixed"),
    "sk_conv": _c("conv taps=9 cfg=-1 sk=1 wd=0 split_in split_out", srcs=(64,), cout=64, res="split", act=ACT_RELU),
    "sk_s2_f32w": _c("conv taps=9 s2 cfg=-1 sk=1 wd=0 split_in split_out self_concat", h=16, w=16, stride=2, srcs=(32,), cout=64,
                     wk="f32"),
    "sk_up": _c("conv taps=9 up cfg=-1 sk=1 wd=0 split_in split_out", h=4, w=4, up=True, srcs=(64,), cout=64, res="split",
                res_up=True, regime="mixed"),
    "sk_up_f32w": _c("conv taps=9 up cfg=-1 sk=1 wd=0 split_in split_out self_concat", h=4, w=4, up=True, srcs=(32,), cout=32,
                     wk="f32", act=ACT_SILU, nbias=True),
    "sk_outf32_f32w": _c("conv taps=9 cfg=-1 sk=1 wd=0 f32out split_in self_concat", srcs=(32,), cout=3, wk="f32", out_f32=True,
                         res="f32"),
    "sk_outf32": _c("conv taps=9 cfg=-1 sk=1 wd=0 f32out split_in", srcs=(64,), cout=3, out_f32=True, res="f32", act=ACT_RELU),
    "sk_linear_f32w": _c("gemm taps=1 cfg=-1 sk=1 wd=0 split_in split_out self_concat", linear=True, n=64, srcs=(256,), cout=96,
                         wk="f32", act=ACT_RELU),
    # weights-direct conv3x3 (conv_wd.hip), SPL epilogue
    "wd7_up_forced_f32w": _c("conv taps=9 up cfg=7 sk=0 wd=0 split_in split_out self_concat", h=4, w=16, up=True, srcs=(32,), cout=128,
                             force=7, wk="f32", res="split", act=ACT_RELU),
    "wd7_up_forced": _c("conv taps=9 up cfg=7 sk=0 wd=0 split_in split_out", h=4, w=16, up=True, srcs=(64,), cout=128, force=7,
                        res="split", regime="mixed"),
    "wd7_auto": _c("conv taps=9 cfg=7 sk=0 wd=0 split_in split_out", n=4, h=32, w=128, srcs=(32,), cout=256, res="split", stats=True),
    "wd7_auto_f32w": _c("conv taps=9 cfg=7 sk=0 wd=0 split_in split_out self_concat", n=4, h=32, w=128, srcs=(32,), cout=256,
                        wk="f32", res="f32", res_up=True, nbias=True, act=ACT_RELU, stats=True),
    "wd7_forced_mixed": _c("conv taps=9 cfg=7 sk=0 wd=0 split_in split_out", n=1, h=8, w=32, srcs=(64,), cout=128, force=7,
                           regime="mixed", res="split", act=ACT_RELU),
    "wd6_forced": _c("conv taps=9 cfg=6 sk=0 wd=0 split_in split_out", n=1, h=8, w=64, srcs=(32,), cout=256, force=6, res="split",
                     act=ACT_RELU, stats=True),
    "wd6_forced_two_f32w": _c("conv taps=9 cfg=6 sk=0 wd=0 split_in split_out self_concat", n=1, h=8, w=32, srcs=(64, 64), cout=256,
                              force=6, wk="f32", res="f32", nbias=True),
    "wd6_auto": _c("conv taps=9 cfg=6 sk=0 wd=0 split_in split_out", n=6, h=32, w=256, srcs=(32,), cout=256, regime="mixed",
                   res="split", res_up=True),
    "wd8_forced": _c("conv taps=9 cfg=8 sk=0 wd=0 split_in split_out", n=1, h=8, w=32, srcs=(8,), cout=128, force=8),
    "wd8_auto_mixed": _c("conv taps=9 cfg=8 sk=0 wd=0 split_in split_out", n=4, h=64, w=256, srcs=(16,), cout=128, regime="mixed",
                         act=ACT_RELU),
    "c3_plain_k": _c("conv taps=9 cfg=3 sk=0 wd=0 f32out split_in", n=4, h=64, w=256, srcs=(32,), cout=3, out_f32=True, res="f32",
                      res_scale=1024.0),
    "c3_plain_k_f32w": _c("conv taps=9 cfg=3 sk=0 wd=0 f32out split_in self_concat", n=4, h=64, w=256, srcs=(32,), cout=8,
                          out_f32=True, wk="f32", regime="mixed"),
    # weights-direct GEMM (gemm_wd.hip) over split weights, fp32 output
    "gemm_wd_f32out": _c("gemm taps=1 cfg=-1 sk=0 wd=1 f32out split_in", linear=True, n=256, srcs=(64,), cout=128, out_f32=True),
    # GroupNorm-apply + activation materialised by pmi_gn_apply before the convolution
    "pro_one_silu": _c(G3, n=2, srcs=(32,), cout=32, prologue=ACT_SILU, regime="mixed"),
    "pro_two_relu_f32w": _c("conv taps=9 cfg=-1 sk=1 wd=0 split_in split_out self_concat", n=2, srcs=(32, 64), cout=32, prologue=ACT_RELU, wk="f32"),
}

GUARD = 64


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


@contextlib.contextmanager
def _guarded(tag, full=True):
    """every ops-level allocation NaN-filled with a NaN guard after its logical end (full: and finite once written)"""
    from perceptor_amd.engine import ops
    from test_gpu_norm_resample import _Guarded
    g = _Guarded()
    old = ops._empty
    ops._empty = g
    try:
        yield g
    finally:
        ops._empty = old
    g.verify(tag, full)


@contextlib.contextmanager
def _forced(cfg):
    from perceptor_amd import _hip
    if cfg is not None:
        _hip.lib().pmi_set_option(1, cfg)
    try:
        yield
    finally:
        if cfg is not None:
            _hip.lib().pmi_set_option(1, -1)


def route_key(desc: str) -> str:
    """the route part of an ops.GEMM_TRACE description"""
    t = desc.split()
    kv = dict(x.split("=", 1) for x in t[1:] if "=" in x)
    fl = {x for x in t[1:] if "=" not in x}
    geo = "".join(f" {f}" for f in ("up", "s2") if f in fl)
    flags = "".join(f" {f}" for f in ("f32out", "split_in", "split_out", "self_concat") if f in fl)
    return f"{t[0]} taps={kv['taps']}{geo} cfg={kv['halo']} sk={int(int(kv['splitk']) > 1)} wd={kv['wd']}{flags}"


def n_pad(cout):
    return (cout + 3) // 4 * 4


def out_grid(cs):
    if cs["linear"]:
        return None
    h, w = (2 * cs["h"], 2 * cs["w"]) if cs["up"] else (cs["h"], cs["w"])
    return h // cs["stride"], w // cs["stride"]


def build_case(cs):
    """operands (CPU) and float64 references of one case: dict with the physical sources, weights, epilogue tensors, the references
    and bounds of _precise_ref64.precise_ref, and the logical parts (x_hi, x_lo) they were computed from."""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    seed, reg = cs["seed"], cs["regime"]
    lead = (cs["n"],) if cs["linear"] else (cs["n"], cs["h"], cs["w"])
    srcs, his, los = [], [], []
    for i, c in enumerate(cs["srcs"]):
        hi, lo = (P.coherent_hi_lo if reg == "coherent" else P.mixed_hi_lo)(lead + (c,), seed * 100 + i)
        srcs.append(P.join_split(hi, lo))
        his.append(hi.double())
        los.append(lo.double())
    x_hi, x_lo = torch.cat(his, -1), torch.cat(los, -1)
    cin, cout, np_ = sum(cs["srcs"]), cs["cout"], n_pad(cs["cout"])
    k = 3 if cs["taps"] == 9 else 1
    w = P.weights((cout, cin, k, k), seed * 100 + 10, reg, cs["wk"])
    wpad = torch.zeros((np_, cin, k, k))
    wpad[:cout] = w
    bias = P.vector(cout, seed * 100 + 11, reg) if cs["bias"] else None
    bpad = None
    if bias is not None:
        bpad = torch.zeros(np_)
        bpad[:cout] = bias
    nbias = P.vector(cs["n"] * np_, seed * 100 + 12, reg).view(cs["n"], np_) if cs["nbias"] else None
    og = out_grid(cs)
    rshape = None
    res_phys = res_log = None
    if cs["res"]:
        rg = og if not cs["res_up"] else (og[0] // 2, og[1] // 2)
        rshape = (cs["n"],) + (tuple(rg) if og else ()) + (np_,)
        if cs["res"] == "split":
            rh, rl = (P.coherent_hi_lo if reg == "coherent" else P.mixed_hi_lo)(rshape, seed * 100 + 13, cs["res_scale"])
            res_phys, res_log = P.join_split(rh, rl), rh.double() + rl.double()
        else:
            res_phys = P.vector(math.prod(rshape), seed * 100 + 13, reg, cs["res_scale"]).view(rshape)
            res_log = res_phys.double()
    pro = None
    tin = None
    if cs["prologue"] is not None:
        g = torch.Generator().manual_seed(seed * 100 + 14)
        ca = torch.rand((cs["n"], cin), generator=g) + 0.5
        cb = torch.rand((cs["n"], cin), generator=g) - 0.5
        pro = (ca, cb, cs["prologue"])
        v = (x_hi + x_lo).float()
        u32 = P.act_ref((v * ca[:, None, None, :] + cb[:, None, None, :]).double(), cs["prologue"]).float()
        uh = u32.half()
        ul = (u32 - uh.float()).half()
        u = P.act_ref((x_hi + x_lo) * ca[:, None, None, :].double() + cb[:, None, None, :].double(), cs["prologue"])
        # the apply pass: fp32 x * a + b, the activation (ACT_HW) and the split store, against float64
        tin = P.C_B * ((4 * P.E32 + P.ACT_HW[ACT_SILU] + P.U_SPLIT) * u.abs() + P.SPLIT_FLOOR)
        x_hi, x_lo = uh.double(), ul.double()
    lin = ops.PackedLinear(w, bias, _hip.DT_F16X2, "cpu", sources=list(cs["srcs"]) if len(cs["srcs"]) > 1 else None)
    K = lin.K
    generic = " cfg=-1 " in cs["route"] and " wd=0" in cs["route"]
    sk = P.generic_splitk(cs["n"] * (og[0] * og[1] if og else 1), np_, K) if generic else 1
    assert (sk > 1) == (" sk=1 " in cs["route"]), "the restated split-K rule disagrees with the claimed route"
    y, yc, tol, tol_c, sabs = P.precise_ref(x_hi, x_lo, wpad, self_concat=lin.self_concat, bias=bpad, nbias=nbias, residual=res_log,
                                            res_up=cs["res_up"], act=cs["act"], stride=cs["stride"], up=cs["up"],
                                            split_out=not cs["out_f32"], chain=P.chain_len(K, sk))
    if tin is not None:
        wh, wl = P.weight_parts(wpad, lin.self_concat)
        u = x_hi + x_lo
        slack = P.conv64(tin, wh.abs() + wl.abs()) + 2.0 ** -21 * P.conv64(u.abs(), wpad.double().abs())
        tol, tol_c = tol + slack, tol_c + slack
    return dict(srcs=srcs, w=w, bias=bias, nbias=nbias, res=res_phys, pro=pro, lin=lin, y=y, yc=yc, tol=tol, tol_c=tol_c,
                sabs=sabs, x_hi=x_hi, x_lo=x_lo, wpad=wpad, bpad=bpad, res_log=res_log, splitk=sk)


def run_case(cs, d, dev):
    """one launch through ops.igemm under GEMM_TRACE: (output, route key, stats or None)"""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    lin = ops.PackedLinear(d["w"], d["bias"], _hip.DT_F16X2, dev, sources=list(cs["srcs"]) if len(cs["srcs"]) > 1 else None)
    a0 = d["srcs"][0].to(dev)
    a1 = d["srcs"][1].to(dev) if len(d["srcs"]) > 1 else None
    kw = dict(act=cs["act"], up=cs["up"], stride=cs["stride"], res_up=cs["res_up"], out_f32=cs["out_f32"], want_stats=cs["stats"])
    if d["nbias"] is not None:
        kw["nbias"] = d["nbias"].to(dev)
    if d["res"] is not None:
        kw["residual"] = d["res"].to(dev)
    if d["pro"] is not None:
        ca, cb, pact = d["pro"]
        kw["prologue"] = (ca.to(dev).contiguous(), cb.to(dev).contiguous(), pact)
    ops.GEMM_TRACE = []
    try:
        with _forced(cs["force"]):
            out = ops.igemm(a0, lin, a1=a1, **kw)
        torch.cuda.synchronize()
        (desc, *_), = ops.GEMM_TRACE
    finally:
        ops.GEMM_TRACE = None
    st = getattr(out, "_pmi_stats", None)
    return out, route_key(desc), st


def logical_out(out, cs):
    if cs["out_f32"]:
        return out.double().cpu()
    return P.from_split16(out.cpu())


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_precise_igemm_route(name):
    cs = CONV_CASES[name]
    dev = _dev()
    d = build_case(cs)
    with _guarded(name):
        out, key, st = run_case(cs, d, dev)
        out2, _, _ = run_case(cs, d, dev)
    assert key == cs["route"], f"{name}: took route {key!r}, the case claims {cs['route']!r}"
    assert torch.equal(out.view(torch.int16 if out.dtype == torch.float16 else torch.int32),
                       out2.view(torch.int16 if out2.dtype == torch.float16 else torch.int32)), f"{name}: two launches differ"
    got = logical_out(out, cs)
    assert got.shape == d["y"].shape, (got.shape, d["y"].shape)
    m, mc = P.margin(got, d["y"], d["tol"]), P.margin(got, d["yc"], d["tol_c"])
    print(f"[precise] {name}: route {key}; err/tol exact {m:.3f}, contract {mc:.3f}")
    assert m <= 1.0, f"{name}: outside the exact-reference bound ({m:.2f} x tol)"
    assert mc <= 1.0, f"{name}: outside the contract bound ({mc:.2f} x tol)"
    if cs["stats"]:
        assert st is not None, f"{name}: no fused statistics"
        s, rows = st
        s = s.double().cpu().sum(1)                                # [n, N, 2]
        y = got.reshape(cs["n"], -1, got.shape[-1])
        hw = y.shape[1]
        for j, yy in enumerate((y, y * y)):
            ref = yy.sum(1)
            tol = P.C_B * (hw * P.E32 + 2 * P.U_SPLIT) * yy.abs().sum(1) + hw * P.SPLIT_FLOOR * (1 + 2 * y.abs().max())
            err = float(((s[..., j] - ref).abs() / tol).max())
            print(f"[precise] {name}: statistics {'sum' if j == 0 else 'sumsq'} err/tol {err:.3f}")
            assert err <= 1.0, (name, j, err)


def test_first_conv_f32_weights_config_query_differs():
    """the first-convolution shape with fp32 weights (C0 <= 32): ops.igemm asks for the config while A1 is unset (8, packing the config-8
    fragments) and pmi_igemm re-derives it once A1 = A0 (self_concat): the generic kernel then takes the call and reads B, not Bf.
    The case g_first_f32w_c8 checks the result against float64; here the two queries are restated."""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    cs = CONV_CASES["g_first_f32w_c8"]
    dev = _dev()
    d = build_case(cs)
    lin = ops.PackedLinear(d["w"], d["bias"], _hip.DT_F16X2, dev)
    assert lin.self_concat and lin.cin_p == 32
    a = _hip.IgemmArgs()
    a.H, a.W, a.Hin, a.Win, a.hw, a.M, a.N, a.K, a.C0, a.C1 = 8, 32, 8, 32, 256, 256, lin.n_p, lin.K, 16, 0
    a.lda0, a.taps, a.stride, a.batch, a.batch_inner, a.dtype, a.split_in, a.split_out, a.Bf, a.A0 = 16, 9, 1, 1, 1, 2, 1, 32, 1, 1
    with _forced(8):
        first = _hip.lib().pmi_conv3x3_halo_config(a)
        a.A1, a.C1, a.lda1 = 1, 16, 16
        second = _hip.lib().pmi_conv3x3_halo_config(a)
    assert (first, second) == (8, -1), (first, second)


def test_ragged_two_source_prologue_refused():
    """two sources whose logical channel counts are not multiples of 32: the applied tensor pmi_gn_apply writes is grouped by
    split_group(C0 + C1), the weights by source -- refused, never silently wrong"""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    dev = _dev()
    cs = _c(G3, n=1, srcs=(8, 16), cout=32, prologue=ACT_SILU)
    d = build_case(dict(cs, prologue=None))
    lin = ops.PackedLinear(d["w"], d["bias"], _hip.DT_F16X2, dev, sources=[8, 16])
    ca, cb = torch.ones((1, 24), device=dev), torch.zeros((1, 24), device=dev)
    with pytest.raises(ValueError):
        ops.igemm(d["srcs"][0].to(dev), lin, a1=d["srcs"][1].to(dev), prologue=(ca, cb, ACT_SILU))


@pytest.mark.parametrize("cout", [40, 56])
def test_precise_output_grouping_refused(cout):
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    dev = _dev()
    x = P.join_split(*P.mixed_hi_lo((1, 8, 8, 32), 3)).to(dev)
    lin = ops.PackedLinear(torch.randn(cout, 32, 3, 3), None, _hip.DT_F16X2, dev)
    with pytest.raises(ValueError):
        ops.igemm(x, lin)


# ---- exact-fp32 GEMM (csrc/f32gemm.hip) ---------------------------------------------------------------------------------------------
F32_CASES = {
    # name: (M, N, K, transB, alpha, bias, act, residual, bitwise)
    "k13_none": (70, 45, 13, False, 1.0, False, ACT_NONE, False, True),
    "k77_relu": (100, 67, 77, False, 1.0, False, ACT_RELU, False, True),
    "k40_transb_relu": (33, 70, 40, True, 1.0, False, ACT_RELU, False, True),
    "k5_tiny": (3, 5, 5, False, 1.0, False, ACT_NONE, False, True),
    "full_epilogue_silu": (65, 33, 40, True, 0.125, True, ACT_SILU, True, False),
    "bias_relu_res": (130, 97, 200, False, 0.5, True, ACT_RELU, True, False),
}


def _f32_operands(M, N, K, transB, seed):
    g = torch.Generator().manual_seed(seed)
    A = torch.randn((M, K), generator=g)
    B = torch.randn((K, N) if transB else (N, K), generator=g)
    return A, B


def _f32_ref(A, B, transB, alpha, bias, act, R):
    Bm = B.double() if transB else B.double().T          # [K, N]
    acc = A.double() @ Bm
    sabs = A.double().abs() @ Bm.abs()
    z = alpha * acc + (bias.double() if bias is not None else 0)
    y = P.act_ref(z, act)
    K = A.shape[1]
    err = P.ACT_LIP[act] * ((K + 2) * P.E32 * (abs(alpha) * sabs + (bias.double().abs() if bias is not None else 0))) + P.ACT_HW[act] * y.abs()
    if R is not None:
        y = y + R.double()
        err = err + P.E32 * (y.abs() + R.double().abs())
    return y, P.C_B * (err + P.E32 * y.abs())


@pytest.mark.parametrize("name", list(F32_CASES))
def test_gemm_f32(name):
    from perceptor_amd.engine import ops
    M, N, K, transB, alpha, has_bias, act, has_res, bitwise = F32_CASES[name]
    dev = _dev()
    A, B = _f32_operands(M, N, K, transB, 7)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(8)) if has_bias else None
    R = torch.randn((M, N), generator=torch.Generator().manual_seed(9)) if has_res else None
    outs = []
    with _guarded(name):
        for _ in range(2):
            D = ops._empty((M, N), torch.float32, dev)
            ops.gemm_f32(A.to(dev), B.to(dev), D, M=M, N=N, K=K, lda=K, ldb=N if transB else K, ldd=N, trans_b=transB, alpha=alpha,
                         bias=bias.to(dev) if bias is not None else None, act=act, residual=R.to(dev) if R is not None else None)
            outs.append(D)
        torch.cuda.synchronize()
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)), f"{name}: two launches differ"
    got = outs[0].cpu()
    ref, tol = _f32_ref(A, B, transB, alpha, bias, act, R)
    m = P.margin(got, ref, tol)
    print(f"[precise] gemm_f32 {name}: err/tol {m:.3f}")
    assert m <= 1.0, (name, m)
    if bitwise:
        # f32gemm.hip: v_mfma_f32_32x32x2_f32 is bit for bit a k-ordered fmaf chain -- exact emulation on a sample of outputs
        rng = random.Random(11)
        Bk = B if transB else B.T                            # [K, N]
        idx = [(rng.randrange(M), rng.randrange(N)) for _ in range(48)] + [(M - 1, N - 1), (0, 0)]
        bad = []
        for i, j in idx:
            e = P.fma_chain_f32(A[i].tolist(), Bk[:, j].tolist())
            e = max(e, 0.0) if act == ACT_RELU else e
            if torch.tensor(e, dtype=torch.float32).view(torch.int32) != got[i, j].view(torch.int32) and not (e == 0 and got[i, j] == 0):
                bad.append((i, j, e, float(got[i, j])))
        assert not bad, f"{name}: {len(bad)} of {len(idx)} outputs differ from the k-ordered fmaf chain, e.g. {bad[:3]}"


BATCH_GEOM = (37, 45, 29, 2, 3, (5000, 1300), (7000, 2100), (9000, 1900), 31, 33, 47)   # M N K batch/inner outer inner sA sB sD lda ldb ldd


def batch_operands():
    M, N, K, bo, bi, sA, sB, sD, *_ = BATCH_GEOM
    g = torch.Generator().manual_seed(21)
    return torch.randn(sA[0] * bo + 10, generator=g), torch.randn(sB[0] * bo + 10, generator=g)


def test_gemm_f32_batch_strides():
    """batch / batch_inner with all six strides distinct: a swapped outer / inner stride or operand shows"""
    from perceptor_amd.engine import ops
    dev = _dev()
    M, N, K, bo, bi, sA, sB, sD, lda, ldb, ldd = BATCH_GEOM
    Ab, Bb = batch_operands()
    with _guarded("gemm_f32 batch") as gd:
        Db = ops._empty((sD[0] * bo,), torch.float32, dev)
        Db.fill_(0.0)
        ops.gemm_f32(Ab.to(dev), Bb.to(dev), Db, M=M, N=N, K=K, lda=lda, ldb=ldb, ldd=ldd, batch=bo * bi, batch_inner=bi, sA=sA, sB=sB,
                     sD=sD)
        torch.cuda.synchronize()
    Dc = Db.cpu()
    for zo in range(bo):
        for zi in range(bi):
            a = torch.as_strided(Ab, (M, K), (lda, 1), zo * sA[0] + zi * sA[1])
            b = torch.as_strided(Bb, (N, K), (ldb, 1), zo * sB[0] + zi * sB[1])
            ref, tol = _f32_ref(a, b, False, 1.0, None, ACT_NONE, None)
            got = torch.as_strided(Dc, (M, N), (ldd, 1), zo * sD[0] + zi * sD[1])
            m = P.margin(got, ref, tol)
            assert m <= 1.0, (zo, zi, m)


def test_linear_f32_mapping_shape():
    """ops.linear_f32 at the v-diffusion mapping network's shape (K = 640, ragged N), bias + ReLU + residual"""
    from perceptor_amd.engine import ops
    dev = _dev()
    M, K, N = 5, 640, 70
    g = torch.Generator().manual_seed(31)
    x, w, b, r = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, generator=g), torch.randn(M, N, generator=g)
    with _guarded("linear_f32"):
        got = ops.linear_f32(x.to(dev), w.to(dev), b.to(dev), act=ACT_RELU, residual=r.to(dev)).cpu()
    ref, tol = _f32_ref(x, w, False, 1.0, b, ACT_RELU, r)
    assert P.margin(got, ref, tol) <= 1.0


# ---- split conversions (csrc/elementwise.hip) ----------------------------------------------------------------------------------------
def split_values(rows, C, seed):
    """normal values, values whose lo lands in the f16 subnormals (|x| near 2^-14 and 2^-24), and |x| > 65504"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((rows, C), generator=g)
    x[1::5] *= 2.0 ** -14
    x[2::5] *= 2.0 ** -24
    x[3::5] *= 2.0 ** 10
    x[4, :4] = torch.tensor([7.0e4, -1.0e5, 65519.0, 65521.0])
    x[4, 4:8] = torch.tensor([65504.0, -65504.0, 3.0e-8, -6.0e-8])
    return x


@pytest.mark.parametrize("C", [8, 16, 24, 32, 96])
def test_split_conversions_bitwise(C):
    from perceptor_amd.engine import ops
    from perceptor_amd._hip import call, ptr
    dev = _dev()
    rows, ld = 37, C + 12
    x = split_values(rows, C, C)
    xin = torch.zeros((rows, ld))
    xin[:, :C] = x
    hi = x.half()
    lo = (x - hi.float()).half()
    want = P.join_split(hi, lo)
    with _guarded(f"split C={C}", full=False):      # (the values past 65504 give non-finite outputs by design)
        s = ops._empty((rows, 2 * C), torch.float16, dev)
        call("pmi_split_from_f32", ptr(xin.to(dev)), ld, ptr(s), rows, C)
        f = ops._empty((rows, C), torch.float32, dev)
        call("pmi_split_to_f32", ptr(s), ptr(f), rows, C)
        plain = x.clamp(-6e4, 6e4).half().to(dev)
        up = ops.split_convert(plain, True)
        down = ops.split_convert(up, False)
        sd = ops.split_convert(s, False)
        torch.cuda.synchronize()
    s, f, up, down, sd = s.cpu(), f.cpu(), up.cpu(), down.cpu(), sd.cpu()
    assert torch.equal(s.view(torch.int16), want.view(torch.int16)), "pmi_split_from_f32 differs from torch's RNE split"
    # overflow stays visible: |x| > 65504 (rounding past 65520) gives a non-finite hi, never a clamped one
    big = x.abs() >= 65520
    assert big.any() and not torch.isfinite(P.parts(s)[0][big]).any()
    fw = hi.float() + lo.float()
    fin = torch.isfinite(fw)
    assert torch.equal(torch.isnan(f), torch.isnan(fw)) and torch.equal(f[fin].view(torch.int32), fw[fin].view(torch.int32))
    assert torch.equal(up.view(torch.int16), P.join_split(plain.cpu(), torch.zeros_like(plain.cpu())).view(torch.int16))
    # (back to plain: f16(hi + lo) with lo = +0 -- IEEE gives -0 + +0 = +0, so a -0 comes back as +0)
    assert torch.equal(down.view(torch.int16), (plain.cpu().float() + 0.0).half().view(torch.int16))
    sdw = (hi.float() + lo.float()).half()
    fin = torch.isfinite(sdw)
    assert torch.equal(sd[fin].view(torch.int16), sdw[fin].view(torch.int16)) and not torch.isfinite(sd[~fin]).any()


# ---- route census ------------------------------------------------------------------------------------------------------------------
# every precise route the engines below take (printed by the census) with fp16-torso, bf16-exact and full-fp32 weights: each is the
# claimed route of a CONV_CASES case.  (gemm_wd never sees self_concat weights: ops.igemm asks pmi_gemm_wd_eligible before it sets
# A1 = A0, with K = 2 C0 and C1 = 0, which the eligibility rule K == C0 + C1 refuses -- the generic kernel takes those calls.)
ENGINE_ROUTES = [
    "conv taps=9 cfg=-1 sk=0 wd=0 f32out split_in",
    "conv taps=9 cfg=-1 sk=0 wd=0 split_in split_out",
    "conv taps=9 cfg=-1 sk=0 wd=0 split_in split_out self_concat",
    "conv taps=9 cfg=-1 sk=1 wd=0 f32out split_in",
    "conv taps=9 cfg=-1 sk=1 wd=0 f32out split_in self_concat",
    "conv taps=9 cfg=-1 sk=1 wd=0 split_in split_out",
    "conv taps=9 cfg=-1 sk=1 wd=0 split_in split_out self_concat",
    "conv taps=9 cfg=7 sk=0 wd=0 split_in split_out",
    "conv taps=9 cfg=7 sk=0 wd=0 split_in split_out self_concat",
    "conv taps=9 s2 cfg=-1 sk=0 wd=0 split_in split_out",
    "conv taps=9 s2 cfg=-1 sk=1 wd=0 split_in split_out self_concat",
    "conv taps=9 up cfg=-1 sk=1 wd=0 split_in split_out",
    "conv taps=9 up cfg=-1 sk=1 wd=0 split_in split_out self_concat",
    "conv taps=9 up cfg=7 sk=0 wd=0 split_in split_out",
    "conv taps=9 up cfg=7 sk=0 wd=0 split_in split_out self_concat",
    "gemm taps=1 cfg=-1 sk=0 wd=0 f32out split_in",
    "gemm taps=1 cfg=-1 sk=0 wd=0 f32out split_in self_concat",
    "gemm taps=1 cfg=-1 sk=0 wd=0 split_in split_out",
    "gemm taps=1 cfg=-1 sk=0 wd=0 split_in split_out self_concat",
    "gemm taps=1 cfg=-1 sk=1 wd=0 split_in split_out",
    "gemm taps=1 cfg=-1 sk=1 wd=0 split_in split_out self_concat",
]


def _census(run):
    from perceptor_amd.engine import ops
    ops.GEMM_TRACE = []
    try:
        run()
        torch.cuda.synchronize()
        return sorted({route_key(d) for d, *_ in ops.GEMM_TRACE if not d.startswith("bgemm")})
    finally:
        ops.GEMM_TRACE = None


TORSO = ("input_blocks.", "middle_block.", "output_blocks.")


def fp16_torso_keys(sd):
    """the tensors the reference's convert_to_fp16 casts (fp16_util.convert_module_to_f16): weight and bias of every convolution of
    input_blocks / middle_block / output_blocks"""
    keys = []
    for k, v in sd.items():
        if k.startswith(TORSO) and k.endswith(".weight") and v.ndim >= 3:
            keys.append(k)
            if k[:-len("weight")] + "bias" in sd:
                keys.append(k[:-len("weight")] + "bias")
    return keys


def fp16_torso(sd):
    """fp32 weights with the fp16_torso_keys rounded to fp16: what a real GuidedDiffusion checkpoint holds"""
    out = dict(sd)
    for k in fp16_torso_keys(sd):
        out[k] = sd[k].half().float()
    return out


def _adm_weights(cfg, kind):
    """"fp16": fp16 torso over fp32 weights (a real checkpoint), "bf16": the synthetic default (golden / benchmark weights), "fp32": all fp32"""
    from perceptor_amd.engine import adm
    from perceptor_amd.utils.synth import synth_state_dict
    if kind == "bf16":
        return synth_state_dict(adm.state_dict_shapes(cfg), 0)
    sd = synth_state_dict(adm.state_dict_shapes(cfg), 0, rounding="none")
    return fp16_torso(sd) if kind == "fp16" else sd


def test_precise_route_census():
    from perceptor_amd.engine import adm, vdiff
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    from test_gpu_adm import TINY
    dev = _dev()
    keys = set()

    def note(tag, run):
        k = _census(run)
        print(f"[precise] census {tag}: {len(k)} routes")
        keys.update(k)

    xt, tt = seeded_noise((2, 3, 64, 64), 31).to(dev) * 0.5 + 0.5, torch.tensor([10, 500]).to(dev)
    for tag in TINY:
        cfg = adm.AdmConfig(**TINY[tag])
        for kind in ("fp16", "bf16", "fp32"):
            eng = adm.AdmEngine(cfg, _adm_weights(cfg, kind), dev, "precise")
            note(f"adm tiny {tag} {kind}", lambda: eng.forward(xt, tt))
    cfg = adm.openimages_config()
    x128 = seeded_noise((1, 3, 128, 128), 3).to(dev) * 0.5 + 0.5
    for kind in ("fp16", "bf16", "fp32"):
        eng = adm.AdmEngine(cfg, _adm_weights(cfg, kind), dev, "precise")
        note(f"adm openimages@128 {kind}", lambda: eng.forward(x128, torch.tensor([500]).to(dev)))
        del eng
    for cond in (False, True):
        spec = vdiff.make_spec("tiny", (3, 32, 32), [64, 128, 128], 2, 2, 4, 1, cond)
        for rounding in ("none", "bf16"):
            with warnings.catch_warnings():
                warnings.filterwarnings("error", message="precise mode")
                veng = vdiff.VDiffEngine(spec, synth_state_dict(vdiff.state_dict_shapes(spec), 0, rounding=rounding), dev, "precise")
            ce = seeded_noise((2, 512), 6).to(dev) if cond else None
            note(f"vdiff tiny cond={cond} {rounding}",
                 lambda: veng.forward(seeded_noise((2, 3, 32, 32), 5).to(dev) * 0.5 + 0.5, torch.tensor([0.7, 0.2]).to(dev), ce))
    keys = sorted(keys)
    print("[precise] census routes:\n  " + "\n  ".join(keys))
    covered = {c["route"] for c in CONV_CASES.values()}
    missing = [k for k in keys if k not in covered]
    assert not missing, f"precise routes no kernel case covers: {missing}"
    assert set(keys) <= set(ENGINE_ROUTES), f"census routes not listed in ENGINE_ROUTES: {sorted(set(keys) - set(ENGINE_ROUTES))}"
