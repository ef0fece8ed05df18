"""GPU: the kernel paths only dtype='mixed' runs, one launch at a time against float64 with per-element bounds (tests/_mixed_ref64.py):
conv3x3_wd_kernel's split-input staging (single and doubled operand, tile configs 6 and 7) with the split epilogue, its fallback, and the
attention projection from plain f16 operands onto the split stream.

Every call runs on NaN-filled outputs and scratch with NaN guards (test_gpu_precise_kernels._guarded), twice with equal bits, and must
take the route its case names: ops.MIXED_TRACE gives wd / fallback, the ops.KERNEL_EVENTS description the tile config and operand
(`cfgN mixed-<operand>`).  A case's `fallback` lists the operands whose call the weights-direct kernel does not take: the host rule
(conv3x3.hip pmi_conv3x3_halo_config) wants C0 and Cin, as the K index counts them, to be multiples of 64 -- logical channels for the
single operand, physical (twice as many) for the doubled one -- so the single operand of a 32-, 96- or 64 + 32-channel input falls back
while its doubled operand runs the tile kernel.  The 128-channel tiles stage 32-channel chunks two at a time (an even chunk count), so
the odd chunk counts of the seam cases exist for the doubled operand of config 7 (Cin 96: six 16-channel chunks, three loop trips) and
for the single operand of config 6 (Cin 192: three 64-channel chunks); the `_el` cases give config 7's single operand the nearest
eligible shapes.  A fallback under a forced config runs the apply pass and the plain split tile kernel of that config (covered per
route by test_gpu_precise_kernels); unforced it is the generic kernel.

The census runs AdmMixedEngine on the tiny configs and requires every conv3x3_mixed call to match a case here by (route, config,
operand, sources, up, residual kind, nbias) -- a fallback has no config and the same doubled arithmetic whatever operand was asked, so its
key carries neither -- and every other traced call over split tensors to be the projection's route, one of
test_gpu_precise_kernels.ENGINE_ROUTES, or one of MIXED_ENGINE_ROUTES below (what the mixed engine takes and the precise engines do not,
each the claimed route of a precise kernel case).  The shipped config at 128x128, batch 1, is part of the census (2 s): its 1/1 level
already runs config 7's single operand.

Largest err / tol per family on an MI355X (output; fused statistics) -- no margin above 1, the run found no kernel defect:
    config 7 single operand   0.112; 0.006        config 7 doubled operand  0.011; 0.007
    config 6 single operand   0.105; 0.008        config 6 doubled operand  0.011; 0.008
    fallback, forced config 7 0.016; 0.006        fallback, generic kernel  0.013 (no fused statistics)
    projection                0.307
"""
import functools

import pytest
import torch

import _mixed_ref64 as X

pytestmark = pytest.mark.gpu


def _c(cfg, **kw):
    cs = dict(cfg=cfg, n=1, h=8, w=32, srcs=(64,), cout=256 if cfg == 6 else 128, up=False, res=None, res_up=False, nbias=False,
              regime="coherent", seed=1, operands=("single", "dbl"), fallback=())
    cs.update(kw)
    if cfg < 0:
        cs["fallback"] = cs["operands"]
    return cs


CASES = {
    # ---- config 7: 128-channel tiles, 32-channel chunks (16 logical channels with the doubled operand) ----
    "c7_one_tile": _c(7, srcs=(32,), fallback=("single",)),
    "c7_one_tile_el": _c(7, operands=("single",)),
    "c7_seams": _c(7, n=2, h=16, w=64, srcs=(96,), cout=256, regime="mixed", res="split", fallback=("single",), seed=2),
    "c7_seams_el": _c(7, n=2, h=16, w=64, srcs=(128,), cout=256, regime="mixed", res="split", operands=("single",), seed=2),
    "c7_two_src": _c(7, n=2, srcs=(64, 32), fallback=("single",), seed=3),
    "c7_two_src_el": _c(7, n=2, srcs=(128, 64), operands=("single",), seed=3),
    "c7_up_resup": _c(7, h=4, w=16, up=True, res="split", res_up=True, seed=4),
    "c7_up_resup_n2": _c(7, n=2, h=4, w=16, up=True, res="split", res_up=True, regime="mixed", seed=4),
    "c7_up": _c(7, h=4, w=16, up=True, regime="mixed", seed=20),                        # an up ResBlock's conv1 ...
    "c7_resup": _c(7, res="split", res_up=True, seed=21),                                  # ... and its conv2: the residual alone at half the grid
    "c7_epi_none": _c(7, regime="mixed", seed=5),
    "c7_epi_split": _c(7, res="split", seed=6),
    "c7_epi_f32": _c(7, res="f32", seed=7),
    "c7_epi_nbias": _c(7, n=2, nbias=True, regime="mixed", seed=8),
    "c7_epi_f32_two": _c(7, srcs=(64, 64), res="f32", regime="mixed", seed=9),
    "c7_wide": _c(7, n=2, res="split", regime="wide", seed=10),
    "c7_act": _c(7, regime="coherent_act", seed=11),
    # ---- config 6: 256-channel tiles, 64-channel chunks (32 logical channels with the doubled operand) ----
    "c6_one_tile": _c(6),
    "c6_one_tile_32": _c(6, srcs=(32,), operands=("dbl",)),            # one 64-channel chunk of [yh 32 | yl 32]; the shortest chain: a dropped input low part shows
    "c6_seams": _c(6, n=2, h=16, w=64, srcs=(192,), cout=512, regime="mixed", res="split", seed=2),
    "c6_two_src": _c(6, n=2, srcs=(128, 64), seed=3),
    "c6_up_resup": _c(6, h=4, w=16, up=True, res="split", res_up=True, seed=4),
    "c6_up_resup_n2": _c(6, n=2, h=4, w=16, up=True, res="split", res_up=True, regime="mixed", seed=4),
    "c6_up": _c(6, h=4, w=16, up=True, regime="mixed", seed=20),                        # an up ResBlock's conv1 ...
    "c6_resup": _c(6, res="split", res_up=True, seed=21),                                  # ... and its conv2: the residual alone at half the grid
    "c6_epi_none": _c(6, regime="mixed", seed=5),
    "c6_epi_split": _c(6, res="split", seed=6),
    "c6_epi_f32": _c(6, res="f32", seed=7),
    "c6_epi_nbias": _c(6, n=2, nbias=True, regime="mixed", seed=8),
    "c6_epi_f32_two": _c(6, srcs=(64, 64), res="f32", regime="mixed", seed=9),
    "c6_wide": _c(6, n=2, res="split", regime="wide", seed=10),
    "c6_act": _c(6, regime="coherent_act", seed=11),
    # ---- fallback: apply pass + generic split convolution (W % 32 != 0, or Cout % 128 != 0 as in the tiny engines of the census) ----
    "fb_w16_f32": _c(-1, h=16, w=16, res="f32", operands=("single",), seed=12),            # pmi_split_from_f32 + apply pass + generic kernel
    "fb_plain": _c(-1, h=16, w=16, srcs=(32,), cout=32, regime="mixed", operands=("dbl",), seed=13),
    "fb_two": _c(-1, n=2, h=16, w=16, srcs=(64, 32), cout=32, operands=("single",), seed=14),
    "fb_up": _c(-1, h=8, w=8, srcs=(32,), cout=32, up=True, operands=("dbl",), seed=15),
    "fb_nbias": _c(-1, n=2, h=16, w=16, srcs=(32,), cout=64, nbias=True, regime="mixed", operands=("single",), seed=16),
    "fb_two_nbias": _c(-1, n=2, h=16, w=16, srcs=(32, 32), cout=32, nbias=True, operands=("dbl",), seed=17),
    "fb_split": _c(-1, h=16, w=16, srcs=(32,), cout=32, res="split", operands=("single",), seed=18),
    "fb_split_resup": _c(-1, h=16, w=16, srcs=(32,), cout=32, res="split", res_up=True, regime="mixed", operands=("dbl",), seed=19),
}
PARAMS = [(name, op) for name, cs in CASES.items() for op in cs["operands"]]

# the projection: plain f16 rows x plain f16 weights + split residual -> split rows; route = test_gpu_precise_kernels.route_key of the call
PROJ_ROUTE, PROJ_ROUTE_SK = "gemm taps=1 cfg=-1 sk=0 wd=0 split_out", "gemm taps=1 cfg=-1 sk=1 wd=0 split_out"
PROJ_CASES = {
    "proj_ragged": dict(m=72, k=64, n=64, regime="coherent", res_scale=1.0, seed=21, route=PROJ_ROUTE),
    "proj_512": dict(m=128, k=512, n=512, regime="mixed", res_scale=1.0, seed=22, route=PROJ_ROUTE),
    "proj_splitk": dict(m=64, k=1024, n=64, regime="coherent", res_scale=1.0, seed=23, route=PROJ_ROUTE_SK),     # generic_splitk: 2 slabs
    "proj_wide_res": dict(m=72, k=64, n=64, regime="mixed", res_scale=1024.0, seed=24, route=PROJ_ROUTE),
}

# split routes the mixed engine takes beyond test_gpu_precise_kernels.ENGINE_ROUTES (the precise engines' own): the 1x1 skip_connection over a
# split input with fp32 rows out runs the weights-direct GEMM (ops.igemm allows it for out_f32); CONV_CASES["gemm_wd_f32out"] claims the route
# (one source, coherent operands: the kernel and its route, not the mixed engine's two-source operands)
MIXED_ENGINE_ROUTES = ("gemm taps=1 cfg=-1 sk=0 wd=1 f32out split_in",)


def case_key(cs, operand):
    """what the census matches an engine's call by"""
    res = (cs["res"] + ("_up" if cs["res_up"] else "")) if cs["res"] else "none"
    fb = operand in cs["fallback"]
    return ("fallback" if fb else "wd", -1 if fb else cs["cfg"], "any" if fb else operand, len(cs["srcs"]), cs["up"], res, cs["nbias"])


@functools.lru_cache(maxsize=4)
def inputs(name):
    return X.build_inputs(CASES[name])


def run_case(name, operand, dev, launches=2):
    """the case through ops.conv3x3_mixed: ([outputs], route, [KERNEL_EVENTS descriptions], [GEMM_TRACE descriptions], statistics)"""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    from test_gpu_precise_kernels import _forced
    cs, d = CASES[name], inputs(name)
    ml = ops.MixedLinear(d["w"], d["bias"], dev, sources=tuple(cs["srcs"]) if len(cs["srcs"]) > 1 else None)
    x0 = d["srcs"][0].to(dev)
    x1 = d["srcs"][1].to(dev) if len(d["srcs"]) > 1 else None
    kw = dict(operand=operand, prologue=(d["a"].to(dev).contiguous(), d["b"].to(dev).contiguous(), _hip.ACT_SILU), x1=x1, up=cs["up"],
              residual=d["res"].to(dev) if d["res"] is not None else None, res_up=cs["res_up"],
              nbias=d["nbias"].to(dev) if d["nbias"] is not None else None)
    timed = str(dev) != "cpu"                      # (the event descriptions need a device; the CPU route check reads MIXED_TRACE alone)
    ops.MIXED_TRACE, ops.GEMM_TRACE, ops.KERNEL_EVENTS = [], [], ([] if timed else None)
    try:
        with _forced(cs["cfg"] if cs["cfg"] >= 0 else None):
            outs = [ops.conv3x3_mixed(x0, ml, **kw) for _ in range(launches)]
        if timed:
            torch.cuda.synchronize()
        route = ops.MIXED_TRACE[0][0]
        events = [e[-1] for e in ops.KERNEL_EVENTS] if timed else []
        traced = [t[0] for t in ops.GEMM_TRACE]
    finally:
        ops.MIXED_TRACE = ops.GEMM_TRACE = ops.KERNEL_EVENTS = None
    st = getattr(outs[0], "_pmi_stats", None)
    return outs, route, events, traced, st


def _splitk_of(traced):
    for t in traced:
        for tok in t.split():
            if tok.startswith("splitk="):
                return max(1, int(tok[7:]))
    return 1


@pytest.mark.parametrize("name,operand", PARAMS)
def test_mixed_conv_route(name, operand):
    from test_gpu_precise_kernels import _dev, _guarded
    cs, dev = CASES[name], _dev()
    d = inputs(name)
    tag = f"{name} {operand}"
    with _guarded(tag):
        outs, route, events, traced, st = run_case(name, operand, dev)
    fb = operand in cs["fallback"]
    assert route == ("fallback" if fb else "wd"), f"{tag}: took route {route!r}"
    if fb:
        assert not any("mixed-" in e for e in events), (tag, events)
        kernel = f"cfg{cs['cfg']}" if cs["cfg"] >= 0 else "generic"
        if cs["cfg"] >= 0:
            assert len(events) == 2 and all(f" cfg{cs['cfg']} " in e + " " for e in events), (tag, events)
        else:
            assert not events and len(traced) == 2, (tag, events, traced)
    else:
        kernel = f"cfg{cs['cfg']} mixed-{operand}"
        assert len(events) == 2 and all(e.endswith(kernel) for e in events), (tag, events)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{tag}: two launches differ"
    got = X.from_split16(outs[0].cpu())
    y, tol, info = X.conv_ref(d, cs, operand, fallback=fb, splitk=_splitk_of(traced) if fb else 1)
    assert got.shape == y.shape, (got.shape, y.shape)
    assert info["amb"] <= X.AMB_CAP[cs["regime"]], (tag, info["amb"])
    m = X.margin(got, y, tol)
    line = f"[mixed] {tag}: route {route} {kernel}; err/tol {m:.3f}, amb share {100 * info['amb']:.3f} %"
    ms = None
    assert fb or st is not None, f"{tag}: no fused statistics"
    if st is not None:          # every tile-kernel launch, a fallback under a forced config included
        ms = X.stats_check(st[0], got, cs["n"])
        line += f", statistics err/tol {ms:.3f}"
    print(line)
    assert m <= 1.0, f"{tag}: outside the bound ({m:.2f} x tol)"
    assert ms is None or ms <= 1.0, f"{tag}: fused statistics outside the bound ({ms:.2f} x tol)"


def run_proj(name, dev, launches=2):
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    from test_gpu_precise_kernels import route_key
    d = X.proj_inputs(PROJ_CASES[name])
    lin = ops.PackedLinear(d["w"], d["bias"], _hip.DT_F16, dev)
    x, r = d["x"].to(dev), d["res"].to(dev)
    ops.GEMM_TRACE = []
    try:
        outs = [ops.igemm(x, lin, residual=r, split_out=True) for _ in range(launches)]
        if str(dev) != "cpu":
            torch.cuda.synchronize()
        descs = [t[0] for t in ops.GEMM_TRACE]
    finally:
        ops.GEMM_TRACE = None
    return d, outs, route_key(descs[0]), _splitk_of(descs)


@pytest.mark.parametrize("name", list(PROJ_CASES))
def test_plain_to_split_projection(name):
    from test_gpu_precise_kernels import _dev, _guarded
    cs, dev = PROJ_CASES[name], _dev()
    with _guarded(name):
        d, outs, route, sk = run_proj(name, dev)
    assert route == cs["route"], f"{name}: took route {route!r}, the case claims {cs['route']!r}"
    assert sk == X.generic_splitk(cs["m"], cs["n"], cs["k"]), (name, sk)
    assert torch.equal(outs[0].view(torch.int16), outs[1].view(torch.int16)), f"{name}: two launches differ"
    got = X.from_split16(outs[0].cpu())
    y, tol = X.proj_ref(d, sk)
    m = X.margin(got, y, tol)
    print(f"[mixed] {name}: route {route} splitk={sk}; err/tol {m:.3f}")
    assert m <= 1.0, f"{name}: outside the bound ({m:.2f} x tol)"


# ---- census ---------------------------------------------------------------------------------------------------------------------------
def _engine_keys(eng, x, t):
    """one forward under the traces: ({conv3x3_mixed keys}, {route keys of every other traced call over split tensors})"""
    from perceptor_amd.engine import ops
    from test_gpu_precise_kernels import route_key
    real, keys = ops.conv3x3_mixed, set()

    def recording(x_, mlin, *, operand, prologue, x1=None, up=False, residual=None, res_up=False, nbias=None):
        ne = len(ops.KERNEL_EVENTS)
        out = real(x_, mlin, operand=operand, prologue=prologue, x1=x1, up=up, residual=residual, res_up=res_up, nbias=nbias)
        route = ops.MIXED_TRACE[-1][0]
        res = "none" if residual is None else ("f32" if residual.dtype == torch.float32 else "split") + ("_up" if res_up else "")
        cfg = -1
        if route == "wd":
            desc = ops.KERNEL_EVENTS[ne][-1]
            assert desc.endswith(f"mixed-{operand}"), desc
            cfg = int(desc.split()[-2][3:])
        keys.add((route, cfg, operand if route == "wd" else "any", 1 if x1 is None else 2, bool(up), res, nbias is not None))
        return out

    ops.conv3x3_mixed = recording
    ops.MIXED_TRACE, ops.KERNEL_EVENTS, ops.GEMM_TRACE = [], [], None
    try:
        eng.forward(x, t)
        torch.cuda.synchronize()
    finally:
        ops.conv3x3_mixed = real
        ops.MIXED_TRACE = ops.KERNEL_EVENTS = None
    # the other calls: a second forward with GEMM_TRACE alone (a launch on a tile config is traced there only while KERNEL_EVENTS is off)
    ops.GEMM_TRACE = []
    try:
        eng.forward(x, t)
        torch.cuda.synchronize()
        other = {route_key(d) for d, *_ in ops.GEMM_TRACE if not d.startswith("bgemm") and ("split_in" in d or "split_out" in d)}
    finally:
        ops.GEMM_TRACE = None
    return keys, other


def _census_check(found, other):
    from test_gpu_precise_kernels import CONV_CASES, ENGINE_ROUTES
    assert set(MIXED_ENGINE_ROUTES) <= {c["route"] for c in CONV_CASES.values()}, "a route of MIXED_ENGINE_ROUTES has no precise kernel case"
    covered = {case_key(cs, op) for cs in CASES.values() for op in cs["operands"]}
    missing = sorted(k for k in found if k not in covered)
    assert not missing, f"conv3x3_mixed calls no case covers (route, config, operand, sources, up, residual, nbias): {missing}"
    extra = sorted(k for k in other if k not in set(ENGINE_ROUTES) | set(MIXED_ENGINE_ROUTES) | {PROJ_ROUTE, PROJ_ROUTE_SK})
    assert not extra, f"traced calls over split tensors that are neither the projection nor a listed engine route: {extra}"


def test_mixed_route_census_tiny_engines():
    """ADM_TINY "a" and "b": split levels, a split / plain level boundary, up- and down-sampling blocks, two-source convolutions and an
    attention block on a split level.  Their widths (32 and 64 output channels) keep every conv3x3_mixed call on the fallback whatever
    the map size -- the 64x128 input changes the generic kernel's tiling and split-K, not the route; the tile kernels' keys come from the
    shipped config below."""
    from perceptor_amd.engine import adm, adm_mixed
    from perceptor_amd.utils.synth import seeded_noise
    from test_gpu_backward import ADM_TINY
    from test_gpu_precise_kernels import _adm_weights, _dev
    dev = _dev()
    found, other, boundary = set(), set(), False
    for tag, plain_from in (("a", 4), ("b", 4), ("b", 2)):
        cfg = adm.AdmConfig(**ADM_TINY[tag])
        eng = adm_mixed.AdmMixedEngine(cfg, _adm_weights(cfg, "bf16"), dev, plain_from=plain_from)
        for n, hh, ww in ((2, 64, 64), (1, 64, 128)):
            x = seeded_noise((n, 3, hh, ww), 31).to(dev) * 0.5 + 0.5
            boundary |= any(eng._plain(l.ds_in) != eng._plain(l.ds_out) for ls in eng.inp + [eng.mid] + eng.out for l in ls if not isinstance(l, tuple))
            k, o = _engine_keys(eng, x, torch.tensor([10, 500][:n]).to(dev))
            print(f"[mixed] census adm tiny {tag} plain_from={plain_from} {hh}x{ww}: {len(k)} conv3x3_mixed keys, {len(o)} other split routes")
            found |= k
            other |= o
    print("[mixed] census conv3x3_mixed keys:\n  " + "\n  ".join(map(str, sorted(found))))
    print("[mixed] census other split routes:\n  " + "\n  ".join(sorted(other)))
    assert any(k[3] == 2 for k in found) and any(k[4] for k in found), "the census engines run no two-source / no up-sampling convolution"
    assert other & {PROJ_ROUTE, PROJ_ROUTE_SK}, "no attention block ran on a split level"
    assert boundary, "no census engine has a block whose input and output levels differ in form (split / plain)"
    _census_check(found, other)


def test_mixed_route_census_shipped_128():
    """the shipped config at 128x128, batch 1: the full-resolution level runs config 7's single operand (an up block's conv1 and conv2),
    the rest falls back; its skip convolutions add MIXED_ENGINE_ROUTES"""
    from perceptor_amd.engine import adm, adm_mixed
    from perceptor_amd.utils.synth import seeded_noise
    from test_gpu_precise_kernels import _adm_weights, _dev
    dev = _dev()
    cfg = adm.openimages_config()
    eng = adm_mixed.AdmMixedEngine(cfg, _adm_weights(cfg, "bf16"), dev)
    found, other = _engine_keys(eng, seeded_noise((1, 3, 128, 128), 3).to(dev) * 0.5 + 0.5, torch.tensor([500]).to(dev))
    print("[mixed] census shipped@128 conv3x3_mixed keys:\n  " + "\n  ".join(map(str, sorted(found))))
    print("[mixed] census shipped@128 other split routes:\n  " + "\n  ".join(sorted(other)))
    assert any(k[0] == "wd" for k in found), "the shipped config at 128x128 no longer reaches the tile kernels"
    _census_check(found, other)
