"""GPU: the 16-bit (f16 / bf16) GEMM and convolution routes behind pmi_igemm, one kernel instantiation at a time, against float64
(references, regimes and the per-route bounds: tests/_routes16_ref64.py).

Every case names the route it claims -- the GEMM_TRACE key of the call (kernel config, split-K factor, weights-direct GEMM with its tile rows /
columns, two-source and conv-mode flags) -- and the traced route must equal it; tests/test_routes16_bounds_cpu.py confirms the same strings
on the host queries alone, so the search for the smallest shape that still takes a route needs no device.  Every call runs on NaN-filled
ops-level allocations with a NaN guard past the end; where a case sets `pitch`, inputs, residual and output are column slices of wider
NaN-filled buffers (lda = C + 8, ldr = ldd = N + 8) whose gap columns must stay NaN and must not reach the result, and the input buffers
carry NaN rows past M.  Two launches must give the same bits, and the result must lie inside the per-element bound (err / tol <= 1).

Cases name the smallest shape that still takes their route: forced tile configs on one or two 8 x 32-pixel tiles, the self-selected split-K
instantiations at the smallest K the rules split (pmi_conv3x3_wd_splitk: 512 channels; the weights-direct GEMM's cost model: K = 2560 at
M = 100; conv mode: 512 pixels -- a two-source conv mode call has 18 chunks or more and is always split, so there is no unsplit one), the
144-row tiles at M = 8 x 257 and N = 4096 with K = 128, config 3 at the 256 tiles its rule asks for.  Five cases (cw_16x16_splitk_256,
g_up_splitk, g_tails_f32out, w_two_256_cols, g_gemm_splitk) exist because the full-size census of tests/test_gpu_fullsize.py found their
routes in the benchmark's UNet.

Left out, on purpose: the precise / mixed split forms (tests/test_gpu_precise_kernels.py, tests/test_gpu_mixed.py), and five routes their own
files hold to float64 already: tile config 9 (tests/test_gpu_conv_up_phase.py), the fused skip launch (tests/test_gpu_conv_skip_fused.py), the
taps-16 adjoint and the phased up == 2 adjoint (tests/test_gpu_sd_vae_grad.py, tests/test_gpu_sd_vae_enc_grad.py), and the second-output /
activation-gradient epilogues (tests/test_gpu_transformer_kernels.py).
"""
import pytest
import torch

import _routes16_ref64 as Q
from _routes16_ref64 import ACT_GELU, ACT_NONE, ACT_SILU
from test_gpu_precise_kernels import _dev, _forced, _guarded, route_key

ACT_GEGLU = 5
DTYPES = ("f16", "bf16")
PAD = 8            # gap columns of a pitched tensor
PAD_ROWS = 3       # NaN rows past M of a pitched input


def _c(route, **kw):
    cs = dict(n=1, h=8, w=32, srcs=(64,), cout=128, taps=9, stride=1, up=False, bias=True, nbias=False, res=None, res_up=False,
              act=ACT_NONE, out_f32=False, force=None, pitch=False, stats=False, prologue=None, alpha=1.0, regime="coherent",
              linear=False, dtypes=DTYPES, seed=1)
    cs.update(kw)
    if cs["linear"]:
        cs["taps"] = 1
    cs["route"] = route
    return cs


def _h(cfg, sk=0, geo=""):
    return f"conv taps=9{geo} cfg={cfg} sk={int(sk > 1)} wd=0" + (f" splitk={sk}" if sk > 1 else "")


def _g(kind, taps, geo="", sk=0):
    return f"{kind} taps={taps}{geo} cfg=-1 sk={int(sk > 1)} wd=0" + (f" splitk={sk}" if sk > 1 else "")


def _w(kind, taps, rows, cols, sk=0, extra="", flags=""):
    return f"{kind} taps={taps} cfg=-1 sk={int(sk > 1)} wd=1{flags}" + (f" splitk={sk}" if sk > 1 else "") + f" rows={rows} cols={cols}{extra}"


SMALL, TWO_ROW = dict(n=1, h=8, w=32), dict(n=2, h=16, w=32)
CASES = {
    # ---- conv3x3_halo_kernel, forced tile configs 0 / 1 / 2; config 3 by its own rule (at most 32 output channels, >= 256 tiles) ----
    "halo0_plain": _c(_h(0), **SMALL, srcs=(64,), cout=256, force=0, pitch=True, res="16", regime="mixed"),
    "halo0_two_tail": _c(_h(0), **TWO_ROW, srcs=(128, 64), cout=384, force=0, res="16", res_up=True, act=ACT_SILU, stats=True),
    "halo0_up_pro": _c(_h(0, geo=" up"), n=2, h=8, w=16, srcs=(64,), cout=256, force=0, up=True, prologue=ACT_SILU, nbias=True),
    "halo1_res": _c(_h(1), **TWO_ROW, srcs=(128,), cout=128, force=1, res="16", pitch=True, nbias=True, act=ACT_SILU, stats=True),
    "halo1_two_pro": _c(_h(1), **TWO_ROW, srcs=(128, 64), cout=128, force=1, prologue=ACT_SILU, regime="mixed"),
    "halo2_plain": _c(_h(2), **SMALL, srcs=(64,), cout=128, force=2, res="16", stats=True),
    "halo2_up_resup": _c(_h(2, geo=" up"), n=2, h=8, w=16, srcs=(128,), cout=128, force=2, up=True, res="16", res_up=True, pitch=True),
    "halo2_tiny": _c(_h(2), **SMALL, srcs=(64,), cout=128, force=2, res="16", regime="tiny", dtypes=("f16",)),
    "halo3_f32out": _c(_h(3) + " f32out", n=4, h=64, w=256, srcs=(64,), cout=8, out_f32=True, res="f32"),
    "halo3_res16": _c(_h(3), n=4, h=64, w=256, srcs=(64,), cout=8, res="16", act=ACT_SILU, regime="mixed"),
    # ---- conv3x3_wd_kernel, forced configs 4 / 6 / 7 / 8 ----
    "wd4_res_pitch": _c(_h(4), **SMALL, srcs=(64,), cout=256, force=4, res="16", pitch=True, stats=True),
    "wd4_two_pro": _c(_h(4), **TWO_ROW, srcs=(128, 64), cout=256, force=4, prologue=ACT_SILU, res="16", res_up=True),
    "wd4_up": _c(_h(4, geo=" up"), n=2, h=8, w=16, srcs=(64,), cout=256, force=4, up=True, act=ACT_SILU, regime="mixed"),
    "wd6_res_pitch": _c(_h(6), **SMALL, srcs=(64,), cout=256, force=6, res="16", pitch=True, stats=True, act=ACT_SILU),
    "wd6_two_pro": _c(_h(6), **TWO_ROW, srcs=(128, 64), cout=256, force=6, prologue=ACT_SILU, res="16", res_up=True, nbias=True),
    "wd6_up": _c(_h(6, geo=" up"), n=2, h=8, w=16, srcs=(64,), cout=256, force=6, up=True, res="16", regime="mixed"),
    "wd6_tiny": _c(_h(6), **SMALL, srcs=(64,), cout=256, force=6, res="16", regime="tiny", dtypes=("f16",)),
    "wd6_splitk": _c(_h(6, sk=2), **SMALL, srcs=(512,), cout=256, force=6, act=ACT_SILU, res="16", res_up=True, nbias=True),
    "wd7_res_pitch": _c(_h(7), **SMALL, srcs=(64,), cout=128, force=7, res="16", pitch=True, stats=True),
    "wd7_dead_waves": _c(_h(7), **TWO_ROW, srcs=(64,), cout=320, force=7, res="16", pitch=True, stats=True, regime="mixed"),
    "wd7_two_pro": _c(_h(7), **TWO_ROW, srcs=(128, 64), cout=128, force=7, prologue=ACT_SILU, res="16", res_up=True),
    "wd7_up": _c(_h(7, geo=" up"), n=2, h=8, w=16, srcs=(64,), cout=128, force=7, up=True, act=ACT_SILU),
    "wd7_splitk": _c(_h(7, sk=2), **SMALL, srcs=(256, 256), cout=128, force=7, act=ACT_SILU, res="16", res_up=True, nbias=True,
                     regime="mixed"),
    "wd8_c8": _c(_h(8), **SMALL, srcs=(8,), cout=128, force=8, res="16", pitch=True),
    "wd8_c24_tail": _c(_h(8), **TWO_ROW, srcs=(24,), cout=96, force=8, res="16", res_up=True, act=ACT_SILU, stats=True),
    "wd8_c32": _c(_h(8), **SMALL, srcs=(32,), cout=64, force=8, nbias=True, regime="mixed"),
    # ---- gemm_wd_kernel, conv mode: maps the conv3x3 tiles do not fit, >= 512 pixels, Cin % 128 == 0 ----
    "cw_16x16": _c(_w("conv", 9, 128, 128, extra=" convmode"), n=2, h=16, w=16, srcs=(128,), cout=128, res="16", pitch=True, act=ACT_SILU),
    "cw_16x16_splitk_two": _c(_w("conv", 9, 128, 256, sk=4, extra=" two convmode"), n=2, h=16, w=16, srcs=(128, 128), cout=256, res="16",
                              res_up=True, nbias=True, act=ACT_SILU),
    "cw_16x16_two": _c(_w("conv", 9, 128, 128, sk=4, extra=" two convmode"), n=2, h=16, w=16, srcs=(128, 128), cout=128, res="16", pitch=True),
    "cw_16x16_splitk_256": _c(_w("conv", 9, 128, 256, sk=4, extra=" convmode"), n=2, h=16, w=16, srcs=(256,), cout=256, res="16", act=ACT_SILU,
                              regime="mixed"),
    "cw_4x4_border": _c(_w("conv", 9, 128, 128, extra=" convmode"), n=32, h=4, w=4, srcs=(128,), cout=128, res="16", regime="mixed"),
    "cw_12x20_rowtail": _c(_w("conv", 9, 128, 128, extra=" convmode"), n=3, h=12, w=20, srcs=(128,), cout=128, res="16", pitch=True),
    "cw_nbias_unsplit_generic": _c(_g("conv", 9), n=3, h=12, w=20, srcs=(128,), cout=128, nbias=True, res="16"),
    # ---- igemm_kernel as a convolution ----
    "g_s2": _c(_g("conv", 9, " s2"), n=2, h=16, w=16, srcs=(64,), cout=64, stride=2, res="16", pitch=True),
    "g_c24": _c(_g("conv", 9), n=1, h=12, w=20, srcs=(24,), cout=72, res="f32", act=ACT_SILU, regime="mixed"),
    "g_two_16_32": _c(_g("conv", 9), n=1, h=12, w=20, srcs=(16, 32), cout=72, res="16", pitch=True, nbias=True),
    "g_up": _c(_g("conv", 9, " up"), n=2, h=6, w=10, srcs=(64,), cout=64, up=True, res="16", res_up=True),
    "g_splitk": _c(_g("conv", 9, sk=3), n=1, h=12, w=20, srcs=(192,), cout=72, res="16", res_up=True, nbias=True, act=ACT_SILU),
    "g_up_splitk": _c(_g("conv", 9, " up", sk=3), n=1, h=6, w=10, srcs=(192,), cout=72, up=True, res="16", nbias=True),
    "g_1x1_tiny": _c(_g("gemm", 1), n=1, h=12, w=20, srcs=(64,), cout=72, taps=1, res="16", regime="tiny", dtypes=("f16",)),
    # ---- gemm_wd_kernel as a GEMM ----
    "w_144_rows": _c(_w("gemm", 1, 144, 256), linear=True, n=2056, srcs=(128,), cout=4096, act=ACT_GELU),
    "w_128_rows_res": _c(_w("gemm", 1, 128, 256), linear=True, n=300, srcs=(320,), cout=16384, res="16", alpha=0.5),
    "w_128_cols_ntail": _c(_w("gemm", 1, 128, 128), linear=True, n=200, srcs=(320,), cout=960, res="16", pitch=True, act=ACT_SILU),
    "w_two_96": _c(_w("gemm", 1, 128, 128, extra=" two"), n=1, h=12, w=20, taps=1, srcs=(128, 96), cout=128, res="16", pitch=True),
    "w_two_256_cols": _c(_w("gemm", 1, 128, 256, extra=" two"), n=2, h=64, w=64, taps=1, srcs=(128, 96), cout=512, res="16"),
    "w_splitk": _c(_w("gemm", 1, 128, 256, sk=4), linear=True, n=100, srcs=(2560,), cout=256, res="16", act=ACT_GELU),
    "w_res_f32": _c(_w("gemm", 1, 128, 128), linear=True, n=100, srcs=(128,), cout=256, res="f32", regime="mixed"),
    "w_out_f32": _c(_w("gemm", 1, 128, 128, flags=" f32out"), linear=True, n=100, srcs=(128,), cout=256, out_f32=True, res="f32", act=ACT_SILU),
    "w_tiny": _c(_w("gemm", 1, 128, 128), linear=True, n=100, srcs=(128,), cout=256, res="16", regime="tiny", dtypes=("f16",)),
    "w_geglu": _c(_w("gemm", 1, 128, 256, extra=" geglu"), linear=True, n=100, srcs=(128,), cout=512, act=ACT_GEGLU),
    # ---- igemm_kernel as a GEMM: M, N and K tails (the non-KFAST instantiation) ----
    "g_tails": _c(_g("gemm", 1), linear=True, n=200, srcs=(136,), cout=132, res="16", act=ACT_SILU),
    "g_tails_f32out": _c(_g("gemm", 1) + " f32out", linear=True, n=200, srcs=(136,), cout=132, out_f32=True, res="f32", regime="mixed"),
    "g_gemm_splitk": _c(_g("gemm", 1, sk=2), linear=True, n=200, srcs=(1024,), cout=72, res="16", act=ACT_SILU),
    "g_tails_pitch": _c(_g("gemm", 1), linear=True, n=200, srcs=(136,), cout=136, res="16", pitch=True, regime="mixed"),
}


def route16(desc: str) -> str:
    """route_key plus the split-K factor and the weights-direct GEMM's tile details of a GEMM_TRACE description"""
    t = desc.split()
    sk = [x for x in t if x.startswith("splitk=") and int(x[7:]) > 1]
    tile = [x for x in t if x.startswith(("rows=", "cols=", "skip=")) or x in ("two", "convmode", "geglu", "defer")]
    return " ".join([route_key(desc)] + sk + tile)


def census_key(route: str) -> str:
    """a route16 string as a kernel instantiation: without the split-K factor (sk=1 stays) and the fused skip's channel counts"""
    return " ".join("skip" if t.startswith("skip=") else t for t in route.split() if not t.startswith("splitk="))


# routes of the engines that this file leaves to the files holding them to float64 already (module doc), by the token that names them
COVERED_ELSEWHERE = {"cfg=9": "tests/test_gpu_conv_up_phase.py", "skip": "tests/test_gpu_conv_skip_fused.py"}


def claimed_by(route: str) -> str:
    """the test file that covers a traced route (census_key form), or "" """
    if route in {census_key(c["route"]) for c in CASES.values()}:
        return "tests/test_gpu_routes16.py"
    for token, where in COVERED_ELSEWHERE.items():
        if token in route.split():
            return where
    return ""


def form_of(cs) -> str:
    """the rounding form (Q.FORMS key) of the route a case claims"""
    r = cs["route"].split()
    if cs["act"] == ACT_GEGLU:
        return "geglu"
    if "sk=1" in r:
        return "reduce"
    cfg = int([x for x in r if x.startswith("cfg=")][0][4:])
    if cfg >= 4:
        return f"wd{cfg}"
    if cfg >= 0:
        return f"halo{cfg}"
    if "wd=1" in r:
        return "gemm_wd_f32" if cs["out_f32"] or cs["res"] == "f32" else "gemm_wd"
    pad = PAD if cs["pitch"] else 0
    return Q.generic_form(out_f32=cs["out_f32"], res=cs["res"], res_up=cs["res_up"], n_p=cs["cout"], ldd=cs["cout"] + pad, ldr=cs["cout"] + pad)


def splitk_of(cs) -> int:
    sk = [x for x in cs["route"].split() if x.startswith("splitk=")]
    return int(sk[0][7:]) if sk else 1


def out_grid(cs):
    if cs["linear"]:
        return ()
    h, w = (2 * cs["h"], 2 * cs["w"]) if cs["up"] else (cs["h"], cs["w"])
    return (h // cs["stride"], w // cs["stride"])


_BUILT = {}


def build_case(name, dtype, regime=None):
    """operands (CPU, float64, rounded to the compute type), the float64 reference and the bound of one case; computed once, shared, unchanged
    (regime: the CPU bound tests run a case's shape in the other regime too)"""
    cs = CASES[name]
    regime = regime or cs["regime"]
    if (name, dtype, regime) in _BUILT:
        return _BUILT[(name, dtype, regime)]
    seed, reg = cs["seed"] * 1000 + len(name), regime
    lead = (cs["n"],) if cs["linear"] else (cs["n"], cs["h"], cs["w"])
    # (coherent: the second source one binade above the first, [1, 2): with both in [0.5, 1) a channel read from the wrong source would move
    # the all-positive sum by less than one 16-bit rounding of it)
    srcs = [Q.operand(lead + (c,), seed + i, reg, dtype, scale=2.0 ** i if reg == "coherent" else 1.0) for i, c in enumerate(cs["srcs"])]
    cin, cout = sum(cs["srcs"]), cs["cout"]
    k = 3 if cs["taps"] == 9 else 1
    w = Q.weights((cout, cin, k, k), seed + 10, reg, dtype)
    small = 2.0 ** -15 if reg == "tiny" else 1.0
    side = "mixed" if reg == "tiny" else reg
    bias = Q.operand((cout,), seed + 11, side, "f16", scale=small, spread=2) if cs["bias"] else None       # (fp32 tensors: any 16-bit grid will do)
    nbias = Q.operand((cs["n"], cout), seed + 12, side, "f16", scale=small, spread=2) if cs["nbias"] else None
    og = out_grid(cs)
    res = None
    if cs["res"]:
        rg = tuple(g // 2 for g in og) if cs["res_up"] else og
        res = Q.operand((cs["n"],) + rg + (cout,), seed + 13, side, dtype if cs["res"] == "16" else "f16", scale=small, spread=2)
    x = torch.cat(srcs, -1)
    pro = None
    if cs["prologue"] is not None:
        g = torch.Generator().manual_seed(seed + 14)
        ca = (torch.rand((cs["n"], cin), generator=g) * 0.5 + 0.75).float()
        cb = (torch.rand((cs["n"], cin), generator=g) * 0.25 + 0.25).float()
        if reg != "coherent":
            cb = cb * torch.where(torch.rand((cs["n"], cin), generator=g) < 0.5, -1.0, 1.0)
        pro = (ca, cb, cs["prologue"])
        x = Q.prologue_ref(x, ca, cb, cs["prologue"], dtype)
    K = cs["taps"] * cin
    if cs["act"] == ACT_GEGLU:
        y, tol = Q.geglu_ref(x, w, bias, dtype=dtype, K=K)
    else:
        y, tol, _ = Q.route_ref(x, w, dtype=dtype, form=form_of(cs), K=K, splitk=splitk_of(cs), alpha=cs["alpha"], bias=bias, nbias=nbias,
                                residual=res, res_up=cs["res_up"], act=cs["act"], stride=cs["stride"], up=cs["up"], out_f32=cs["out_f32"],
                                prologue=pro is not None)
    d = dict(srcs=srcs, x=x, w=w, bias=bias, nbias=nbias, res=res, pro=pro, y=y, tol=tol, K=K)
    _BUILT[(name, dtype, regime)] = d
    return d


def _pitched(t, td, dev, pitch, pad_rows):
    """t [..., C] float64 -> (device tensor of the storage type, its whole buffer): with `pitch` a column slice of a NaN-filled buffer with
    PAD more columns and pad_rows more NaN rows"""
    if not pitch:
        return t.to(td).to(dev).contiguous(), None
    C = t.shape[-1]
    rows = t.numel() // C
    buf = torch.full((rows + pad_rows, C + PAD), float("nan"), dtype=td, device=dev)
    buf[:rows, :C] = t.reshape(rows, C).to(td).to(dev)
    return buf[:rows].view(t.shape[:-1] + (C + PAD,))[..., :C], buf


def run_case(name, dtype, dev, launches=2):
    """`launches` calls through ops.igemm under GEMM_TRACE.  Returns (outputs, route, stats, out buffer or None)."""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    cs, d = CASES[name], build_case(name, dtype)
    dt, td = _hip.dtype_code(dtype), Q.TD[dtype]
    lin = ops.PackedLinear(d["w"].float(), d["bias"].float() if d["bias"] is not None else None, dt, dev)
    a = [_pitched(s, td, dev, cs["pitch"], PAD_ROWS)[0] for s in d["srcs"]]
    kw = dict(act=cs["act"], up=cs["up"], stride=cs["stride"], res_up=cs["res_up"], out_f32=cs["out_f32"], want_stats=cs["stats"], alpha=cs["alpha"])
    if d["nbias"] is not None:
        kw["nbias"] = d["nbias"].float().to(dev).contiguous()
    if d["res"] is not None:
        kw["residual"] = _pitched(d["res"], torch.float32 if cs["res"] == "f32" else td, dev, cs["pitch"], 0)[0]
    if d["pro"] is not None:
        ca, cb, pact = d["pro"]
        kw["prologue"] = (ca.to(dev).contiguous(), cb.to(dev).contiguous(), pact)
    outs, route, obuf = [], None, None
    oshape = tuple(d["y"].shape)
    for _ in range(launches):
        if cs["pitch"]:
            obuf = torch.full((d["y"].numel() // oshape[-1], oshape[-1] + PAD), float("nan"), dtype=torch.float32 if cs["out_f32"] else td, device=dev)
            kw["out"] = obuf.view(oshape[:-1] + (oshape[-1] + PAD,))[..., :oshape[-1]]
        ops.GEMM_TRACE = []
        try:
            with _forced(cs["force"]):
                out = ops.igemm(a[0], lin, a1=a[1] if len(a) > 1 else None, **kw)
            (desc, *_), = ops.GEMM_TRACE
        finally:
            ops.GEMM_TRACE = None
        outs.append(out)
        route = route16(desc)
    return outs, route, getattr(outs[0], "_pmi_stats", None), obuf


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


PARAMS = [(name, dtype) for name in CASES for dtype in CASES[name]["dtypes"]]        # (the tiny regime is f16's subnormal range: f16 only)


@pytest.mark.gpu
@pytest.mark.parametrize("name,dtype", PARAMS)
def test_route16(name, dtype):
    cs = CASES[name]
    dev = _dev()
    d = build_case(name, dtype)
    with _guarded(f"{name} {dtype}"):
        (out, out2), route, st, obuf = run_case(name, dtype, dev)
        torch.cuda.synchronize()
    assert route == cs["route"], f"{name}: took route {route!r}, the case claims {cs['route']!r}"
    assert torch.equal(_bits(out), _bits(out2)), f"{name}: two launches differ"
    got = out.double().cpu()
    assert got.shape == d["y"].shape, (got.shape, d["y"].shape)
    assert torch.isfinite(got).all(), f"{name}: non-finite outputs (a NaN gap or padded row reached the result, or rows were left unwritten)"
    if obuf is not None:
        assert torch.isnan(obuf[:, -PAD:].float()).all(), f"{name}: the gap columns of the pitched output were written"
    m = Q.margin(got, d["y"], d["tol"])
    print(f"[routes16] {name} {dtype}: route {route}; form {form_of(cs)}; err/tol {m:.3f}")
    assert m <= 1.0, f"{name} {dtype}: outside the bound ({m:.3f} x tol)"
    if cs["stats"]:
        assert st is not None, f"{name}: no fused statistics"
        s = st[0].double().cpu().sum(1)                               # [n, N, 2]
        y = got.reshape(cs["n"], -1, got.shape[-1])
        for j, (ref, tol) in enumerate(Q.stats_bound(y, dtype, y.shape[1])):
            err = float(((s[..., j] - ref).abs() / tol).max())
            print(f"[routes16] {name} {dtype}: statistics {'sum' if j == 0 else 'sumsq'} err/tol {err:.3f}")
            assert err <= 1.0, (name, j, err)


# ---- igemm_kernel through ops.bgemm: ragged N (the attention-score form) and batch > 1 with batch_inner strides ----------------------
BGEMM = {
    # name: M, N, K, outer, inner, sA (outer, inner), sB, sD, lda, ldb, ldd, out_f32
    "ragged_n_scores": (70, 77, 64, 1, 3, (0, 70 * 64), (0, 80 * 64), (0, 70 * 80), 64, 64, 80, True),
    "batch_inner_16bit": (45, 40, 72, 2, 3, (10000, 72), (10000, 40 * 80), (8000, 40), 216, 80, 120, False),
}


def bgemm_operands(name, dtype):
    M, N, K, bo, bi, sA, sB, sD, lda, ldb, ldd, _ = BGEMM[name]
    na = (bo - 1) * sA[0] + (bi - 1) * sA[1] + (M - 1) * lda + K
    nb = (bo - 1) * sB[0] + (bi - 1) * sB[1] + (N - 1) * ldb + K
    return Q.operand((na,), 51, "mixed", dtype, spread=2), Q.operand((nb,), 52, "mixed", dtype, spread=2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(BGEMM))
def test_route16_bgemm(name, dtype):
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    dev = _dev()
    M, N, K, bo, bi, sA, sB, sD, lda, ldb, ldd, out_f32 = BGEMM[name]
    A, B = bgemm_operands(name, dtype)
    td = Q.TD[dtype]
    nd = (bo - 1) * sD[0] + (bi - 1) * sD[1] + (M - 1) * ldd + (N + 3) // 4 * 4
    outs = []
    with _guarded(f"bgemm {name}", full=False):
        for _ in range(2):
            D = ops._empty((nd,), torch.float32 if out_f32 else td, dev)
            ops.GEMM_TRACE = []
            try:
                ops.bgemm(A.to(td).to(dev), B.to(td).to(dev), D, M=M, N=N, K=K, lda=lda, ldb=ldb, ldd=ldd, batch=bo * bi, batch_inner=bi,
                          sA=sA, sB=sB, sD=sD, dt=_hip.dtype_code(dtype), alpha=0.125)
                (desc, *_), = ops.GEMM_TRACE
            finally:
                ops.GEMM_TRACE = None
            outs.append(D)
        torch.cuda.synchronize()
    assert desc.startswith("bgemm ")
    assert torch.equal(_bits(outs[0]), _bits(outs[1])), f"{name}: two launches differ"
    Dc = outs[0].double().cpu()
    written = torch.zeros(nd, dtype=torch.bool)
    worst = 0.0
    for zo in range(bo):
        for zi in range(bi):
            a = torch.as_strided(A, (M, K), (lda, 1), zo * sA[0] + zi * sA[1])
            b = torch.as_strided(B, (N, K), (ldb, 1), zo * sB[0] + zi * sB[1])
            ref, tol, _ = Q.route_ref(a, b[:, :, None, None], dtype=dtype, form="generic_slow", K=K, alpha=0.125, out_f32=out_f32)
            off = zo * sD[0] + zi * sD[1]
            got = torch.as_strided(Dc, (M, N), (ldd, 1), off)
            torch.as_strided(written, (M, (N + 3) // 4 * 4), (ldd, 1), off).fill_(True)     # (a ragged N: the epilogue's 4-wide vectors, inside the pitch)
            assert torch.isfinite(got).all(), (name, zo, zi)
            worst = max(worst, Q.margin(got, ref, tol))
    # everything outside the M x N blocks is still NaN: no write past a row's (4-padded) N columns or past M rows
    assert torch.isnan(Dc[~written]).all(), f"{name}: the kernel wrote outside the M x N blocks"
    print(f"[routes16] bgemm {name} {dtype}: route generic batch; form generic_slow; err/tol {worst:.3f}")
    assert worst <= 1.0, (name, worst)


def test_gemm_wd_tile_query():
    """pmi_gemm_wd_tile on filled arguments (host logic, no device): the tile GEMM_TRACE reports for a weights-direct GEMM launch"""
    import ctypes as C
    from perceptor_amd import _hip

    def tile(m, n, k, **kw):
        a = _hip.IgemmArgs()
        a.M, a.N, a.K, a.C0, a.taps, a.stride, a.batch, a.batch_inner, a.hw, a.alpha, a.Bf = m, n, k, k, 1, 1, 1, 1, 1, 1.0, 1
        a.lda0, a.ldb, a.ldd = k, k, n
        for key, v in kw.items():
            setattr(a, key, v)
        assert _hip.lib().pmi_gemm_wd_eligible(C.byref(a)) == 1
        return divmod(_hip.lib().pmi_gemm_wd_tile(C.byref(a)), 1000)

    assert tile(2056, 4096, 1024) == (144, 256)          # 15 x 16 = 240 workgroups in one round; 128-row tiles would need 272
    assert tile(2048, 4096, 1024) == (128, 256)
    assert tile(2056, 1024, 1024) == (128, 128)          # fewer than 128 workgroups of 256 columns, unsplit: the 128-column tiles
    assert tile(2056, 1024, 1024, splitk=2, ws=1) == (128, 256)
    assert tile(300, 128, 256) == (128, 128) and tile(300, 320, 256) == (128, 128)      # N = 128; N = 320: a half-filled 256-column tail
    assert tile(100, 512, 128, act=ACT_GEGLU) == (128, 256)      # the gated epilogue exists for the 256-column tiles only
