"""The rows of the CLIP ResNet tower tests and the pmi_igemm routes engine/resnet.py takes at each of them.

ROWS is shared by tests/test_rn_tower_bounds_cpu.py (which evaluates the routes through the library's own host queries, no device) and
tests/test_gpu_rn_tower.py (which observes them on the device run).  Every row has layers (2, 2, 1, 1): an identity-skip block, a stride-1
block with a downsample and three stride-2 blocks in one tower of six bottlenecks.  Widths 16 and 64 and the product's awkward 80 (channels
80 / 160 / 320 / ... / 2560); resolutions 64, 96 and 160 (final maps 2x2, 3x3 and 5x5: odd maps, as the product's 7x7 and 9x9); n = 1 and
3 (1x1 convolutions of m = 9 .. 75 rows: both sides of the weights-direct GEMM's m >= 64); one row takes its images at another size than the
tower's.  Width 96 is there because the route census needs it: only a 384-channel 3x3 convolution on a 16 x 16 map (m >= 512) takes the
weights-direct GEMM's conv mode with split-K on 128-column tiles at a small shape (the product: RN50x4's 640 channels at 18 x 18).

``igemm_calls(cfg, n)`` restates the ops.igemm calls of ResNetEngine.forward(save=True) + .backward in order; ``host_routes`` makes them on
CPU tensors with the launch seam stubbed and reduces each ops.GEMM_TRACE description to a signature (``signature``):
kind, taps, s2, split-K > 1, halo config, the weights-direct GEMM and its tile, res, f32out.
"""
from __future__ import annotations

import functools

import torch

from _vit_routes import _no_launch

TD = {"bf16": torch.bfloat16, "f16": torch.float16}
GSCALE = {"bf16": 1.0, "f16": 65536.0}          # ResNetEngine.gscale

LAYERS = (2, 2, 1, 1)
ROWS = {
    # name: ((res, layers, width, heads, out), n, input size)
    "w16-r64": dict(cfg=(64, LAYERS, 16, 8, 64), n=3, in_hw=(64, 64)),          # final map 2x2, t = 5, C = 512
    "w64-r96": dict(cfg=(96, LAYERS, 64, 32, 128), n=1, in_hw=(96, 96)),        # final map 3x3, t = 10, C = 2048, m = 9 at the last layer
    "w64-r160": dict(cfg=(160, LAYERS, 64, 32, 128), n=3, in_hw=(160, 160)),    # final map 5x5, t = 26: m >= 64 down to the last layer
    "w80-r160": dict(cfg=(160, LAYERS, 80, 40, 640), n=3, in_hw=(160, 160)),    # C = 2560: RN50x4's channels (80 / 160 / 320 / ... / 2560); m = 75 at the last layer
    "w96-r128": dict(cfg=(128, LAYERS, 96, 48, 96), n=3, in_hw=(128, 128)),     # final map 4x4; 384 channels on a 16x16 map at m = 768
    "w16-r96-in": dict(cfg=(96, LAYERS, 16, 8, 64), n=3, in_hw=(120, 104)),     # images at another size: resize and its adjoint in the path
}

# Signatures of the product towers (RN50 .. RN50x64 at n = 1, 2, 4) that no small row reaches, each with the reason and the full-size test
# that runs it.  tests/test_rn_tower_bounds_cpu.py::test_route_coverage fails on a product signature that is neither covered by ROWS nor
# here, on an entry here that a row does cover, and on an entry the named test's tower does not take.
_X64 = "tests/test_gpu_rn_clip.py::test_rn50x64_properties"       # RN50x64 at n = 1, 2 and 4: it alone runs every signature below
UNREACHED = {
    # signature: (why no small shape reaches it, the full-size test that runs it)
    ("conv", 9, False, False, 2, 0, None, False, False):
        ("conv3x3 tile config 2 wants >= 256 tiles of 8 x 32 pixels: a 224 x 224 map of 64 channels at n = 1", _X64),
    ("conv", 9, False, False, 3, 0, None, False, True):
        ("conv3x3 tile config 3 (<= 32 output channels, the stem's dX) wants >= 256 tiles of 8 x 32 pixels and 64 input channels: width 128 at 448 x 448", _X64),
    ("conv", 9, False, False, 7, 0, None, False, False):
        ("conv3x3 tile config 7 wants >= 128 / 256 tiles of 8 x 32 pixels x 128 channels: 224 x 224 maps at n = 2, 96 x 96 x 192 at n = 4", _X64),
    ("conv", 9, False, False, -1, 1, (128, 256), False, False):
        ("the weights-direct GEMM's conv mode unsplit on 256-column tiles: one round of the chip without split-K needs m = n * 112 * 112 rows", _X64),
    ("gemm", 1, False, False, -1, 1, (128, 256), False, False):
        ("unsplit 256-column tiles need (m / 128) * (N / 256) workgroups to fill the chip: m = n * 112 * 112 or n * 48 * 48 rows", _X64),
    ("gemm", 1, False, False, -1, 1, (128, 256), True, False):
        ("the same with the residual epilogue", _X64),
    ("gemm", 1, False, False, -1, 1, (144, 256), False, False):
        ("144-row tiles are chosen by rounds of 256 workgroups: m = 4 * 112 * 112 rows", _X64),
    ("gemm", 1, False, False, -1, 1, (144, 256), True, False):
        ("the same with the residual epilogue", _X64),
}


def blocks(cfg):
    """(inplanes, planes, stride, has_downsample) of every Bottleneck in forward order"""
    res, layers, width, heads, out = cfg
    inplanes, rows = width, []
    for li, nb in enumerate(layers):
        planes = width * 2 ** li
        for b in range(nb):
            stride = 2 if (li > 0 and b == 0) else 1
            rows.append((inplanes, planes, stride, stride > 1 or inplanes != 4 * planes))
            inplanes = 4 * planes
    return rows


def igemm_calls(cfg, n):
    """The ops.igemm calls of one forward(save=True) + backward on n images, in order:
    (input shape, row pitch or None = dense, (cout, cin, k), bias, dict(stride, relu, residual, out_f32))."""
    res, layers, width, heads, out = cfg
    h = width // 2
    c, t = width * 32, (res // 32) ** 2 + 1
    calls = []
    add = lambda shape, w, bias=True, pitch=None, **kw: calls.append((tuple(shape), pitch, w, bias, kw))
    # ---- forward
    add((n, res, res, 8), (h, 3, 3), stride=2, relu=True)
    add((n, res // 2, res // 2, h), (h, h, 3), relu=True)
    add((n, res // 2, res // 2, h), (width, h, 3), relu=True)
    s = res // 4
    geo = []
    for inpl, pl, stride, ds in blocks(cfg):
        so = s // stride
        add((n, s, s, inpl), (pl, inpl, 1), relu=True)
        add((n, s, s, pl), (pl, pl, 3), relu=True)
        if ds:
            add((n, so, so, inpl), (4 * pl, inpl, 1))
        add((n, so, so, pl), (4 * pl, pl, 1), residual=True)
        geo.append((s, so, inpl, pl, stride, ds))
        s = so
    add((n * t, c), (2 * c, c, 1))
    add((n, c), (c, c, 1), pitch=t * c)
    add((n, c), (out, c, 1), out_f32=True)
    # ---- backward
    add((n, out), (c, out, 1), bias=False)
    add((n * t, 2 * c), (c, 2 * c, 1), bias=False)
    add((n, c), (c, c, 1), bias=False, out_f32=True)
    for s, so, inpl, pl, stride, ds in reversed(geo):
        add((n, so, so, 4 * pl), (pl, 4 * pl, 1), bias=False)
        add((n, s, s, pl), (pl, pl, 3), bias=False)
        if ds:
            add((n, so, so, 4 * pl), (inpl, 4 * pl, 1), bias=False)
        add((n, s, s, pl), (inpl, pl, 1), bias=False, residual=True)
    add((n, res // 2, res // 2, width), (h, width, 3), bias=False)
    add((n, res // 2, res // 2, h), (h, h, 3), bias=False)
    add((n, res, res, h), (3, h, 3), bias=False, out_f32=True)
    return calls


def signature(desc: str):
    """(kind, taps, s2, split-K > 1, halo config, wd, wd tile, res, f32out) of an ops.GEMM_TRACE description"""
    t = desc.split()
    kv = dict(x.split("=", 1) for x in t[1:] if "=" in x)
    fl = {x for x in t[1:] if "=" not in x}
    tile = (int(kv["rows"]), int(kv["cols"])) if kv["wd"] == "1" else None
    return (t[0], int(kv["taps"]), "s2" in fl, int(kv["splitk"]) > 1, int(kv["halo"]), int(kv["wd"]), tile, "res" in fl, "f32out" in fl)


class trace:
    """with trace(ops) as descs: ops.GEMM_TRACE collects, descs() gives the descriptions so far"""

    def __init__(self, ops):
        self.ops = ops

    def __enter__(self):
        assert self.ops.GEMM_TRACE is None
        self.ops.GEMM_TRACE = []
        return lambda: [d[0] for d in self.ops.GEMM_TRACE]

    def __exit__(self, *exc):
        self.ops.GEMM_TRACE = None


@functools.lru_cache(maxsize=None)
def _one_route(call, dtype):
    """the signature of one call of igemm_calls, asked of the library on the host: nothing launched"""
    from perceptor_amd import _hip
    from perceptor_amd._hip import ACT_NONE, ACT_RELU
    from perceptor_amd.engine import ops
    shape, pitch, (cout, cin, k), bias, kw = call
    kw = dict(kw)
    dt = _hip.dtype_code(dtype)
    td = _hip.TORCH_DTYPE[dt]
    lin = ops.PackedLinear(torch.zeros(cout, cin, k, k), torch.zeros(cout) if bias else None, dt, "cpu")
    a0 = torch.zeros(shape, dtype=td) if pitch is None else torch.zeros(shape[0], pitch, dtype=td)[:, :shape[1]]
    oshape = tuple(shape[:-1]) if len(shape) == 2 else (shape[0], shape[1] // kw.get("stride", 1), shape[2] // kw.get("stride", 1))
    residual = torch.zeros(oshape + (lin.n_p,), dtype=td) if kw.get("residual") else None
    traced = ops._traced_call
    ops._traced_call = lambda name, args, desc, flops: ops.GEMM_TRACE.append((desc, flops, None, None))
    try:
        with _no_launch(ops), trace(ops) as descs:
            ops.igemm(a0, lin, stride=kw.get("stride", 1), act=ACT_RELU if kw.get("relu") else ACT_NONE, residual=residual,
                      out_f32=bool(kw.get("out_f32")))
            (desc,) = descs()
    finally:
        ops._traced_call = traced
    return signature(desc)


def _hashable(call):
    shape, pitch, w, bias, kw = call
    return (shape, pitch, w, bias, tuple(sorted(kw.items())))


def host_routes(cfg, n, dtype="bf16"):
    """the signatures of every igemm call of one forward + backward on n images, in order"""
    return [_one_route(_hashable(c), dtype) for c in igemm_calls(cfg, n)]


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(state dict, images [n, 3, h, w] in [0, 1], unit probe [n, out]) of a row: the tests' shared inputs, never modified"""
    from perceptor_amd.engine.resnet import rn_state_dict_shapes
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    row = ROWS[name]
    sd = synth_state_dict(rn_state_dict_shapes(row["cfg"]), 0)
    img = seeded_noise((row["n"], 3) + row["in_hw"], 52) * 0.25 + 0.5
    probe = torch.nn.functional.normalize(seeded_noise((row["n"], row["cfg"][4]), 7))
    return sd, img, probe


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """(float64 emulated tower of a row, its own run: the whole-tower reference of the embedding) -- computed once per session"""
    import _rn_ref64 as RN
    sd, img, probe = inputs(name)
    ref = RN.Emu(sd, ROWS[name]["cfg"], TD[dtype])
    return ref, ref.run(img, probe)
