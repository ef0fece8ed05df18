"""The route table of the ViT tower tests: small 2-layer configs and the kernel routes engine/vit.py takes at each of them.

ROWS is shared by tests/test_vit_tower_bounds_cpu.py (which evaluates the routes through the library's own host queries, no device) and
tests/test_gpu_vit_tower.py (which observes them on the device run).  Flags:

  flash        attention by the head-dim-64 flash kernels (else batched GEMMs + pmi_softmax_fwd / bwd + pmi_transpose_16)
  fused_fc     c_fc forward with the activation in the GEMM epilogue (ops.fused_mlp_epilogues)
  fused_pr     c_proj backward with act' in the GEMM epilogue
  slabs_pr     c_proj forward leaves split-K slabs that _ln_slabs (pmi_layernorm_fwd_slabs) reduces
  slabs_fc     c_fc backward leaves split-K slabs that pmi_layernorm_bwd_slabs reduces
  slabs_qkv    in_proj backward leaves split-K slabs that pmi_layernorm_bwd_slabs reduces
  kp_pad       3 * patch^2 is no multiple of 8: the im2col rows carry pad columns
  t_odd        t % 8 != 0: the batched-GEMM attention path pads its key columns to tp = ceil8(t)
  m_small      m = n * t < 64
"""
from __future__ import annotations

import contextlib
import functools

import torch

FLAGS = ("flash", "fused_fc", "fused_pr", "slabs_pr", "slabs_fc", "slabs_qkv", "kp_pad", "t_odd", "m_small")


def _row(cfg, n, on):
    return dict(cfg=cfg, n=n, routes={f: f in on for f in FLAGS})


ROWS = {
    # name: (res, patch, width, layers, heads, out), n, the flags that are set
    "w512": _row((32, 8, 512, 2, 8, 64), 4, ("flash", "fused_fc", "fused_pr", "slabs_pr", "slabs_fc", "t_odd")),      # m = 68: slabs on the two K = 4 width GEMMs only
    "w768-d96": _row((32, 8, 768, 2, 8, 64), 4, ("fused_fc", "fused_pr", "slabs_pr", "slabs_fc", "slabs_qkv", "t_odd")),   # d = 96, t = 17, tp = 24
    "h14-d80": _row((70, 14, 1280, 2, 16, 64), 3,                                                                      # ViT-H-14's layer: d = 80, t = 26, tp = 32
                    ("fused_fc", "fused_pr", "slabs_pr", "slabs_fc", "slabs_qkv", "kp_pad", "t_odd")),
    "t257": _row((224, 14, 768, 1, 12, 64), 1,                                                                         # one full-length sequence: 9 key tiles, one live row in the last
                 ("flash", "fused_fc", "fused_pr", "slabs_pr", "slabs_fc", "slabs_qkv", "kp_pad", "t_odd")),           # (one layer: slabs_pr is the shape's route, no block takes it)
    "w512-m17": _row((32, 8, 512, 2, 8, 64), 1, ("flash", "t_odd", "m_small")),                                        # m = 17: the unfused MLP at a wide layer
    "tiny-odd": _row((28, 14, 128, 2, 2, 48), 4, ("flash", "kp_pad", "t_odd", "m_small")),                             # nothing fused
}


def geometry(cfg, n):
    res, patch, width, layers, heads, out = cfg
    t = (res // patch) ** 2 + 1
    return dict(t=t, m=n * t, tp=(t + 7) // 8 * 8, d=width // heads, k=3 * patch * patch, kp=(3 * patch * patch + 7) // 8 * 8)


@contextlib.contextmanager
def _no_launch(ops):
    """ops with its launch seam recording nothing and launching nothing: the host queries are the library's own"""
    saved = ops.ptr, ops.call
    ops.ptr = lambda x: None if x is None else x.data_ptr()
    ops.call = lambda name, *args: None
    try:
        yield
    finally:
        ops.ptr, ops.call = saved


def host_routes(cfg, n, dtype="bf16"):
    """The routes of one block of the tower on n images, asked of the library on the host: the igemm calls of engine/vit.py on CPU tensors of
    the engine's shapes, nothing launched."""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    res, patch, width, layers, heads, out = cfg
    G = geometry(cfg, n)
    m, dt = G["m"], _hip.dtype_code(dtype)
    td = _hip.TORCH_DTYPE[dt]
    lin = lambda o, i: ops.PackedLinear(torch.zeros(o, i), None, dt, "cpu")
    z16 = lambda c: torch.zeros(m, c, dtype=td)
    fuse = width % 256 == 0 and width <= 2048
    slabs = lambda ret: isinstance(ret, tuple)
    with _no_launch(ops):
        fc_f, pr_f, pr_b, fc_b, qkv_b = lin(4 * width, width), lin(width, 4 * width), lin(4 * width, width), lin(width, 4 * width), lin(width, 3 * width)
        pr_f.b = torch.zeros(width)
        r = dict(flash=G["d"] == 64,
                 fused_fc=ops.fused_mlp_epilogues(fc_f, m), fused_pr=ops.fused_mlp_epilogues(pr_b, m),
                 slabs_pr=slabs(ops.igemm(z16(4 * width), pr_f, residual=torch.zeros(m, width), out_f32=True, defer_reduce=fuse)),
                 slabs_fc=slabs(ops.igemm(z16(4 * width), fc_b, out_f32=True, defer_reduce=fuse)),
                 slabs_qkv=slabs(ops.igemm(z16(3 * width), qkv_b, out_f32=True, defer_reduce=fuse)),
                 kp_pad=G["kp"] != G["k"], t_odd=G["t"] % 8 != 0, m_small=m < 64)
    return r


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(state dict, images [n, 3, res, res] in [0, 1], unit probe [n, out]) of a table row: the tests' shared inputs, never modified"""
    from perceptor_amd.engine.vit import vit_state_dict_shapes
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    cfg, n = ROWS[name]["cfg"], ROWS[name]["n"]
    sd = synth_state_dict(vit_state_dict_shapes(cfg), 0)
    img = seeded_noise((n, 3, cfg[0], cfg[0]), 52) * 0.25 + 0.5
    probe = torch.nn.functional.normalize(seeded_noise((n, cfg[5]), 7))
    return sd, img, probe


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """(float64 emulated tower of a row with the row's route flags, its own run: the whole-tower reference) -- computed once per session"""
    import _vit_ref64 as V
    R = ROWS[name]["routes"]
    sd, img, probe = inputs(name)
    ref = V.Tower(sd, ROWS[name]["cfg"], emulate=TD[dtype], flash=R["flash"], fused_mlp=R["fused_fc"], fused_mlp_bwd=R["fused_pr"])
    return ref, ref.run(img, probe)


TD = {"bf16": torch.bfloat16, "f16": torch.float16}
GSCALE = {"bf16": 1.0, "f16": 65536.0}          # VitEngine.gscale
