"""CPU: what perceptor_amd/engine/ops.py hands to the library, call by call, against a recorded snapshot (tests/snapshots/igemm_calls.json).

The case tables of the GPU route tests are replayed on CPU tensors with the launches recorded instead of run: ops.ptr, ops.call, ops._empty
and (as ops sees it) torch.cuda.Event / torch.cat are replaced -- with dummy events the launch seam itself (ops._launch, ops._traced_call)
runs as on the device -- and the host queries (pmi_conv3x3_halo_config, pmi_gemm_wd_eligible, pmi_igemm_splitk, ...) are the library's own.  A record holds, per library call, the entry point and every non-zero field of its
IgemmArgs / SkipArgs with each pointer replaced by the role of the tensor it addresses (the name of the ops-level argument, a packing cached
on its PackedLinear, or alloc<i> for a buffer ops allocated), then what the call returned, the GEMM_TRACE description, the KERNEL_EVENTS
(flops, bytes, description) and the MIXED_TRACE entry.  A change of routing, packing choice or argument shows as a diff of the snapshot:

    python tests/test_igemm_calls_cpu.py --record       # regenerate after an INTENDED change, and review the diff
"""
import contextlib
import ctypes as C
import inspect
import json
import os
import re
import sys
import types

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SNAPSHOT = os.path.join(HERE, "snapshots", "igemm_calls.json")
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.dirname(HERE)]

import _precise_ref64 as P
import test_gpu_conv_skip_fused as SK
import test_gpu_conv_up_phase as UP
import test_gpu_mixed as MX
import test_gpu_precise_kernels as PK
import test_gpu_routes16 as T

DTN = {torch.float16: "f16", torch.bfloat16: "bf16", torch.float32: "f32", torch.int64: "i64"}
TD = {"f16": torch.float16, "bf16": torch.bfloat16}


class _Ptr(int):
    """what the replaced ops.ptr returns: an address that can be told from a scalar argument"""


class _Event:
    def __init__(self, enable_timing=False):
        pass

    def record(self):
        pass


class _TorchAsOpsSeesIt:
    """torch with dummy events (no device) and a torch.cat whose result gets a role"""

    def __init__(self, cat):
        self.cuda, self.cat = types.SimpleNamespace(Event=_Event), cat

    def __getattr__(self, name):
        return getattr(torch, name)


def _span(t):
    return (sum((s - 1) * st for s, st in zip(t.shape, t.stride())) + 1) * t.element_size() if t.numel() else 0


def _frag_name(key):
    if key == "gemm":
        return "frag_gemm"
    if key == "skip":
        return "frag_skip"
    if key == "c8":
        return "frag_c8"
    if isinstance(key, int):
        return f"frag({key})"
    if key[0] == "up":
        return f"frag16_up({key[1]})"
    return f"frag16({key[1]})" if not key[2] else f"frag16({key[1]},dup_g={key[2]})"


class Recorder:
    """One case's calls into the library.  Tensors are named when an ops-level entry point receives them (first name wins) and kept alive to
    the end of the case, so an address names one tensor; pointers are resolved once the case is over (packings are cached during it)."""

    def __init__(self, ops):
        self.ops, self.calls, self.named, self.lins, self.allocs, self.ncat = ops, [], [], [], [], 0

    # ---- roles ----
    def name(self, t, role):
        if t is not None and not any(u is t for _, u in self.named):
            self.named.append((role, t))

    def name_lin(self, lin, role):
        if lin is not None and not any(l is lin for _, l in self.lins):
            self.lins.append((role, lin))

    def table(self):
        tab = [(t.data_ptr(), _span(t), role) for role, t in self.named]
        for role, lin in self.lins:
            packs = []
            if isinstance(lin, self.ops.MixedLinear):
                packs = [(f"{role}.{k}", p) for k, p in (("single", lin._single), ("dbl", lin._dbl)) if p is not None]
            else:
                packs = [(role, lin)]
            for r, p in packs:
                tab.append((p.w.data_ptr(), _span(p.w), f"{r}.w"))
                if p.b is not None:
                    tab.append((p.b.data_ptr(), _span(p.b), f"{r}.b"))
                tab += [(f.data_ptr(), _span(f), f"{r}.{_frag_name(k)}") for k, f in p._frag.items()]
        return tab

    def resolve(self, p, tab):
        for base, _, role in tab:
            if p == base:
                return role
        for base, span, role in tab:
            if base < p < base + span:
                return f"{role}+{p - base}"
        return "?"

    # ---- the replaced seams ----
    def empty(self, shape, dtype, device):
        t = torch.empty(tuple(shape), dtype=dtype, device=device)
        self.named.append((f"alloc{len(self.allocs)}", t))
        self.allocs.append(f"{DTN[dtype]}{list(t.shape)}")
        return t

    def cat(self, tensors, dim=0):
        t = torch.cat(tensors, dim=dim)
        self.named.append((f"cat{self.ncat}", t))
        self.ncat += 1
        return t

    def call(self, name, *args):
        rec = []
        for a in args:
            obj = getattr(a, "_obj", None)
            if isinstance(obj, C.Structure):
                rec.append({f: (_Ptr(v) if ty is C.c_void_p else v) for f, ty in obj._fields_ for v in [getattr(obj, f)] if v})
            else:
                rec.append(a)
        self.calls.append((name, rec, self.ops.GEMM_TRACE, self.ops.KERNEL_EVENTS))

    def wrap(self, fn):
        """an ops entry point that names its tensor arguments after its own parameters before it runs"""
        sig = inspect.signature(fn)

        def wrapped(*args, **kw):
            b = sig.bind(*args, **kw).arguments
            for key, v in b.items():
                if isinstance(v, torch.Tensor):
                    self.name(v, key)
                elif isinstance(v, (self.ops.PackedLinear, self.ops.MixedLinear)):
                    self.name_lin(v, key)
                elif key == "prologue" and v is not None:
                    self.name(v[0], "pro_a"), self.name(v[1], "pro_b")
                elif key == "skip" and v is not None:
                    self.name_lin(v[0], "skip"), self.name(v[1], "skip_x0"), self.name(v[2], "skip_x1"), self.name(v[3], "skip_bias")
            return fn(*args, **kw)
        return wrapped

    def finish(self):
        tab = self.table()

        def res(v):
            if isinstance(v, _Ptr):
                return self.resolve(int(v), tab)
            if isinstance(v, dict):
                return {k: res(x) for k, x in v.items()}
            return v
        return [[name] + [res(a) for a in rec] for name, rec, _, _ in self.calls]


ENTRY_POINTS = ("igemm", "conv3x3_mixed", "geglu_linear", "bgemm", "downsample_adjoint")


@contextlib.contextmanager
def recording(mode, debug_ws=False):
    """ops with its seams replaced and the instrumentation globals of `mode`; yields the Recorder"""
    from perceptor_amd.engine import ops
    rec = Recorder(ops)
    saved = {k: getattr(ops, k) for k in ("ptr", "call", "_empty", "torch", "GEMM_TRACE", "KERNEL_EVENTS", "MIXED_TRACE", "DEBUG_WS") + ENTRY_POINTS}
    ops.ptr = lambda t: None if t is None else _Ptr(t.data_ptr())
    ops.call, ops._empty, ops.torch = rec.call, rec.empty, _TorchAsOpsSeesIt(rec.cat)
    for name in ENTRY_POINTS:
        setattr(ops, name, rec.wrap(saved[name]))
    rec.trace = ops.GEMM_TRACE = [] if mode == "trace" else None
    rec.events = ops.KERNEL_EVENTS = [] if mode == "events" else None
    rec.mixed = ops.MIXED_TRACE = []
    if debug_ws:
        ops.DEBUG_WS = torch.zeros(64, dtype=torch.int64)
        rec.name(ops.DEBUG_WS, "debug_ws")
    try:
        yield rec
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def _describe(ret):
    if isinstance(ret, tuple) and ret and isinstance(ret[0], str):
        return {"slabs": list(ret[1].shape), "sk": ret[2]}
    if isinstance(ret, torch.Tensor):
        d = {"shape": list(ret.shape), "dtype": DTN[ret.dtype], "stride": list(ret.stride())}
        if hasattr(ret, "_pmi_stats"):
            d["stats_rows"] = ret._pmi_stats[1]
        return d
    return ret


def replay(case, mode, debug_ws=False):
    """one case under one instrumentation mode -> its record"""
    with recording(mode, debug_ws) as rec:
        ret = case()
        out = {"calls": rec.finish(), "allocs": rec.allocs, "ret": _describe(ret)}
        # (T.run_case installs its own GEMM_TRACE list: the one the calls saw is the one to read)
        traces = [tr for _, _, tr, _ in rec.calls if tr is not None] or [rec.trace]
        if traces[0] is not None:
            out["trace"] = [[d, fl] for d, fl, *_ in traces[0]]
        if rec.events is not None:
            out["events"] = [[fl, by, d] for _, _, fl, by, d in rec.events]
        if rec.mixed:
            out["mixed"] = [[r, o, list(s)] for r, o, s in rec.mixed]
    return out


# ---- the cases: the GPU tests' own tables, on CPU tensors ---------------------------------------------------------------------------
def _ops():
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    return _hip, ops


def _r16_direct(name, dtype):
    """T.run_case's call without its GEMM_TRACE handling (the instrumentation modes are chosen here); test_routes16_direct_is_run_case
    holds it to run_case's own records"""
    _hip, ops = _ops()
    cs, d = T.CASES[name], T.build_case(name, dtype)
    td = T.Q.TD[dtype]
    lin = ops.PackedLinear(d["w"].float(), d["bias"].float() if d["bias"] is not None else None, _hip.dtype_code(dtype), "cpu")
    a = [T._pitched(s, td, "cpu", cs["pitch"], T.PAD_ROWS)[0] for s in d["srcs"]]
    kw = dict(act=cs["act"], up=cs["up"], stride=cs["stride"], res_up=cs["res_up"], out_f32=cs["out_f32"], want_stats=cs["stats"], alpha=cs["alpha"])
    if d["nbias"] is not None:
        kw["nbias"] = d["nbias"].float().contiguous()
    if d["res"] is not None:
        kw["residual"] = T._pitched(d["res"], torch.float32 if cs["res"] == "f32" else td, "cpu", cs["pitch"], 0)[0]
    if d["pro"] is not None:
        kw["prologue"] = (d["pro"][0].contiguous(), d["pro"][1].contiguous(), d["pro"][2])
    if cs["pitch"]:
        osh = tuple(d["y"].shape)
        obuf = torch.full((d["y"].numel() // osh[-1], osh[-1] + T.PAD), float("nan"), dtype=torch.float32 if cs["out_f32"] else td)
        kw["out"] = obuf.view(osh[:-1] + (osh[-1] + T.PAD,))[..., :osh[-1]]
    with T._forced(cs["force"]):
        return ops.igemm(a[0], lin, a1=a[1] if len(a) > 1 else None, **kw)


def _precise(name):
    """a case of test_gpu_precise_kernels with run_case's kwargs; the operands are shapes only (no float64 reference is needed here), the
    weights the case's own (their fp32 low part decides self_concat)"""
    _hip, ops = _ops()
    cs = PK.CONV_CASES[name]
    seed, reg = cs["seed"], cs["regime"]
    lead = (cs["n"],) if cs["linear"] else (cs["n"], cs["h"], cs["w"])
    cin, cout, np_ = sum(cs["srcs"]), cs["cout"], PK.n_pad(cs["cout"])
    k = 3 if cs["taps"] == 9 else 1
    w = P.weights((cout, cin, k, k), seed * 100 + 10, reg, cs["wk"])
    bias = P.vector(cout, seed * 100 + 11, reg) if cs["bias"] else None
    lin = ops.PackedLinear(w, bias, _hip.DT_F16X2, "cpu", sources=list(cs["srcs"]) if len(cs["srcs"]) > 1 else None)
    srcs = [torch.zeros(lead + (2 * c,), dtype=torch.float16) for c in cs["srcs"]]
    kw = dict(act=cs["act"], up=cs["up"], stride=cs["stride"], res_up=cs["res_up"], out_f32=cs["out_f32"], want_stats=cs["stats"])
    if cs["nbias"]:
        kw["nbias"] = torch.zeros(cs["n"], np_)
    if cs["res"]:
        og = PK.out_grid(cs)
        rg = og if not cs["res_up"] else (og[0] // 2, og[1] // 2)
        rshape = (cs["n"],) + (tuple(rg) if og else ())
        kw["residual"] = torch.zeros(rshape + (2 * np_,), dtype=torch.float16) if cs["res"] == "split" else torch.zeros(rshape + (np_,))
    if cs["prologue"] is not None:
        kw["prologue"] = (torch.ones(cs["n"], cin), torch.zeros(cs["n"], cin), cs["prologue"])
    with PK._forced(cs["force"]):
        return ops.igemm(srcs[0], lin, a1=srcs[1] if len(srcs) > 1 else None, **kw)


def _mixed(i, operand):
    _hip, ops = _ops()
    case = MX.CASES[i]
    n, h, w, cin, cout = case["n"], case["h"], case["w"], case["cin"], case["cout"]
    up, sp = case.get("up", False), case.get("split")
    ho, wo = (2 * h, 2 * w) if up else (h, w)
    g = torch.Generator().manual_seed(7)
    wt = (torch.randn(cout, cin, 3, 3, generator=g) / (9 * cin) ** 0.5).half().float()
    ml = ops.MixedLinear(wt, torch.zeros(cout), "cpu", sources=(sp, cin - sp) if sp else None)
    x0 = torch.zeros(n, h, w, 2 * (sp or cin), dtype=torch.float16)
    x1 = torch.zeros(n, h, w, 2 * (cin - sp), dtype=torch.float16) if sp else None
    res = None
    if case.get("res") or case.get("res_up"):
        rshape = (n, ho // 2, wo // 2) if case.get("res_up") else (n, ho, wo)
        res = torch.zeros(rshape + (cout,)) if case.get("res_f32") else torch.zeros(rshape + (2 * cout,), dtype=torch.float16)
    nb = torch.zeros(n, cout) if case.get("nbias") else None
    with PK._forced(case["cfg"] if case["cfg"] >= 0 else None):
        return ops.conv3x3_mixed(x0, ml, x1=x1, operand=operand, prologue=(torch.ones(n, cin), torch.zeros(n, cin), _hip.ACT_SILU), up=up,
                                 residual=res, res_up=bool(case.get("res_up")), nbias=nb)


def _skip_layers(cout, c0, c1, dtype):
    _hip, ops = _ops()
    g = torch.Generator().manual_seed(cout + c0 + 7 * c1)
    dt = _hip.dtype_code(dtype)
    conv = ops.PackedLinear(torch.randn(cout, cout, 3, 3, generator=g) / (3.0 * cout ** 0.5), torch.zeros(cout), dt, "cpu")
    skip = ops.PackedLinear(torch.randn(cout, c0 + c1, 1, 1, generator=g) / (c0 + c1) ** 0.5, torch.zeros(cout), dt, "cpu", sources=[c0, c1])
    return conv, skip, ops.fused_skip_bias(conv, skip)


def _skip(case, dtype, n=SK.N, h=SK.H, w=SK.W, force=True):
    """ops.igemm(skip=...) at a case of test_gpu_conv_skip_fused (its _Dev's padded sources); the f16 cases on the 128-channel tiles are the
    refused ones: the skip GEMM runs on its own"""
    _hip, ops = _ops()
    cfg, cout, c0, c1 = case
    conv, skip, sb = _skip_layers(cout, c0, c1, dtype)
    td = TD[dtype]
    hh = torch.zeros(n, h, w, cout, dtype=td)
    x0, x1 = torch.zeros(n, h, w, c0 + 16, dtype=td)[..., :c0], torch.zeros(n, h, w, c1 + 8, dtype=td)[..., :c1]
    with PK._forced(cfg if force else None):
        return ops.igemm(hh, conv, prologue=(torch.ones(n, cout), torch.zeros(n, cout), _hip.ACT_SILU), want_stats=True, skip=(skip, x0, x1, sb))


def _up(name, dtype, cfg):
    _hip, ops = _ops()
    cs = UP.CASES[name]
    n, h, w, cin, cout = cs["n"], cs["h"], cs["w"], cs["cin"], cs["cout"]
    g = torch.Generator().manual_seed(1000 + h * 3 + cin)
    wide = cs.get("wide", cin)
    x = torch.zeros(n, h, w, wide, dtype=TD[dtype])[..., cs.get("off", 0):cs.get("off", 0) + cin]
    lin = ops.PackedLinear((torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).float(), torch.zeros(cout) if cs.get("bias") else None,
                           _hip.dtype_code(dtype), "cpu", up_phase=True)
    pro = (torch.ones(n, cin), torch.zeros(n, cin), 2) if cs.get("pro") else None
    with PK._forced(cfg):
        return ops.igemm(x, lin, up=True, nbias=torch.zeros(n, cout) if cs.get("nbias") else None, prologue=pro, want_stats=bool(cs.get("stats")))


def _linear(n, k, dtype="bf16"):
    _hip, ops = _ops()
    g = torch.Generator().manual_seed(n + k)
    return ops.PackedLinear(torch.randn(n, k, generator=g) / k ** 0.5, torch.zeros(n), _hip.dtype_code(dtype), "cpu")


def _geglu(m, n, k):
    _hip, ops = _ops()
    return ops.geglu_linear(torch.zeros(m, k, dtype=torch.bfloat16), _linear(n, k))


def _mlp_epilogues(m, n, k, want):
    """fused_mlp_epilogues itself (a host query: its answer is the record), then the call it licenses"""
    _hip, ops = _ops()
    lin = _linear(n, k)
    ok = ops.fused_mlp_epilogues(lin, m)
    assert ok == want, (m, n, k, ok)
    if ok:
        x = torch.zeros(m, k, dtype=torch.bfloat16)
        ops.igemm(x, lin, act=_hip.ACT_GELU, pre_out=torch.zeros(m, n, dtype=torch.bfloat16))
        ops.igemm(x, lin, act_grad_of=torch.zeros(m, n, dtype=torch.bfloat16), act_grad=_hip.ACT_GELU)
    return ok


def _defer(m, n, k):
    """a ViT-B MLP projection (K = 3072 -> 768) at a batch whose few output tiles make the library split K"""
    _hip, ops = _ops()
    return ops.igemm(torch.zeros(m, k, dtype=torch.bfloat16), _linear(n, k), residual=torch.zeros(m, n), out_f32=True, defer_reduce=True)


def _bgemm(name, dtype):
    _hip, ops = _ops()
    M, N, K, bo, bi, sA, sB, sD, lda, ldb, ldd, out_f32 = T.BGEMM[name]
    A, B = T.bgemm_operands(name, dtype)
    nd = (bo - 1) * sD[0] + (bi - 1) * sD[1] + (M - 1) * ldd + (N + 3) // 4 * 4
    D = torch.zeros(nd, dtype=torch.float32 if out_f32 else TD[dtype])
    return ops.bgemm(A.to(TD[dtype]), B.to(TD[dtype]), D, M=M, N=N, K=K, lda=lda, ldb=ldb, ldd=ldd, batch=bo * bi, batch_inner=bi,
                     sA=sA, sB=sB, sD=sD, dt=_hip.dtype_code(dtype), alpha=0.125)


def _bgemm_offsets():
    _hip, ops = _ops()
    A, B, D = (torch.zeros(4096, dtype=torch.bfloat16) for _ in range(3))
    return ops.bgemm(A, B, D, M=16, N=16, K=32, lda=32, ldb=32, ldd=16, batch=2, batch_inner=1, sA=(512, 0), sB=(512, 0), sD=(256, 0),
                     dt=_hip.DT_BF16, a_off=64, b_off=128, d_off=32)


def _down_adjoint():
    _hip, ops = _ops()
    g = torch.Generator().manual_seed(3)
    lin = ops.PackedLinear(torch.randn(64, 64, 3, 3, generator=g) / 24.0, None, _hip.DT_BF16, "cpu")
    return ops.downsample_adjoint(torch.zeros(2, 8, 8, 64, dtype=torch.bfloat16), lin, out_f32=True)


def _conv_stats(n, h, w, cin, cout, pro):
    """a 3x3 convolution on a map the conv3x3 tiles do not fit, WITH statistics (an attention block's neighbours on the 16x16 level): the conv
    mode is chosen and packed before the statistics rows make pmi_igemm refuse it -- the generic kernel runs, Bf set and ignored"""
    _hip, ops = _ops()
    g = torch.Generator().manual_seed(n + cin + cout)
    lin = ops.PackedLinear(torch.randn(cout, cin, 3, 3, generator=g) / (3.0 * cin ** 0.5), torch.zeros(cout), _hip.DT_BF16, "cpu")
    prologue = (torch.ones(n, cin), torch.zeros(n, cin), _hip.ACT_SILU) if pro else None
    return ops.igemm(torch.zeros(n, h, w, cin, dtype=torch.bfloat16), lin, prologue=prologue, want_stats=True)


def _both(thunk, all_modes):
    return thunk, (thunk if all_modes else None)


def _cases():
    """id -> (thunk, the thunk replayed under every instrumentation mode or None).  The routes16 cases go through T.run_case, which sets
    GEMM_TRACE itself: for the modes their call is repeated by _r16_direct (held to run_case's record by test_routes16_direct_is_run_case)"""
    cs = {}
    for name, dtype in T.PARAMS:
        tiled = " cfg=-1 " not in T.CASES[name]["route"] + " "
        cs[f"r16/{name}/{dtype}"] = (lambda n=name, d=dtype: T.run_case(n, d, "cpu", launches=1)[0][0],
                                     (lambda n=name, d=dtype: _r16_direct(n, d)) if tiled else None)
    for name, c in PK.CONV_CASES.items():
        cs[f"precise/{name}"] = _both(lambda n=name: _precise(n), " cfg=-1 " not in c["route"] + " ")
    for i in range(len(MX.CASES)):
        for operand in ("single", "dbl"):
            cs[f"mixed/{i}/{operand}"] = _both(lambda i=i, o=operand: _mixed(i, o), True)
    for case, cid in zip(SK.CASES, SK.IDS):
        for dtype in SK.DTYPES:
            cs[f"skip/{cid}/{dtype}"] = _both(lambda c=case, d=dtype: _skip(c, d), True)
    cs["skip/engine-64x64-512/bf16"] = _both(lambda: _skip((6, 512, 512, 256), "bf16", n=1, h=64, w=64, force=False), True)
    for name in UP.CASES:
        for dtype in UP.DTYPES:
            for cfg in (9, 6):
                cs[f"up/{name}/{dtype}/cfg{cfg}"] = _both(lambda n=name, d=dtype, c=cfg: _up(n, d, c), True)
    cs["geglu/epilogue"] = _both(lambda: _geglu(100, 512, 128), False)
    cs["geglu/gate_pass"] = _both(lambda: _geglu(200, 144, 136), False)
    cs["mlp_epilogues/true"] = _both(lambda: _mlp_epilogues(2056, 3072, 768, True), False)
    cs["mlp_epilogues/false_narrow"] = _both(lambda: _mlp_epilogues(2056, 384, 768, False), False)
    cs["mlp_epilogues/false_splits"] = _both(lambda: _mlp_epilogues(64, 256, 4096, False), False)
    cs["defer_reduce/vit_b_proj"] = _both(lambda: _defer(400, 768, 3072), False)
    for name in T.BGEMM:
        cs[f"bgemm/{name}/bf16"] = _both(lambda n=name: _bgemm(n, "bf16"), False)
    cs["bgemm/offsets"] = _both(_bgemm_offsets, False)
    cs["downsample_adjoint"] = _both(_down_adjoint, False)
    cs["convmode_stats/16x16-128"] = _both(lambda: _conv_stats(2, 16, 16, 128, 128, False), True)
    cs["convmode_stats/16x16-128-256-pro"] = _both(lambda: _conv_stats(4, 16, 16, 128, 256, True), True)
    return cs


CASES = _cases()
_RECORDS = {}


def records():
    """every case's record, computed once: the trace-mode replay, plus the KERNEL_EVENTS entries of the events-mode one"""
    if not _RECORDS:
        for cid, (thunk, modes_thunk) in CASES.items():
            r = replay(thunk, "trace")
            if modes_thunk is not None:
                r["events"] = replay(modes_thunk, "events")["events"]
            _RECORDS[cid] = r
    return _RECORDS


def dump(recs):
    return "{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in recs.items()) + "\n}\n"


# ---- tests ------------------------------------------------------------------------------------------------------------------------
def test_calls_match_the_snapshot():
    with open(SNAPSHOT) as f:
        want = json.load(f)
    got = json.loads(dump(records()))
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    for cid in want:
        assert got[cid] == want[cid], f"{cid}:\n  recorded {json.dumps(want[cid])}\n  now      {json.dumps(got[cid])}"


def test_every_pointer_has_a_role():
    for cid, r in records().items():
        assert '"?"' not in json.dumps(r["calls"]), (cid, r["calls"])


@pytest.mark.parametrize("name,dtype", [p for p in T.PARAMS if " cfg=-1 " not in T.CASES[p[0]]["route"] + " "])
def test_routes16_direct_is_run_case(name, dtype):
    a, b = records()[f"r16/{name}/{dtype}"], replay(CASES[f"r16/{name}/{dtype}"][1], "trace")
    assert {k: a[k] for k in ("calls", "allocs", "ret", "trace")} == {k: b[k] for k in ("calls", "allocs", "ret", "trace")}


@pytest.mark.parametrize("cid", [c for c, (_, m) in CASES.items() if m is not None])
def test_instrumentation_does_not_change_the_calls(cid):
    """GEMM_TRACE on, KERNEL_EVENTS on, both off: the same calls; DEBUG_WS adds ws and reserved = 77 to unsplit launches and nothing else"""
    thunk = CASES[cid][1]
    base = records()[cid]
    for mode in ("events", "off"):
        r = replay(thunk, mode)
        assert (r["calls"], r["allocs"], r["ret"]) == (base["calls"], base["allocs"], base["ret"]), (cid, mode)
        assert r.get("mixed") == base.get("mixed")
    dbg = replay(thunk, "off", debug_ws=True)["calls"]
    assert len(dbg) == len(base["calls"])
    for got, want in zip(dbg, base["calls"]):
        if got[0] in ("pmi_igemm", "pmi_conv3x3_skip") and want[1].get("splitk", 0) <= 1:
            want = [want[0], dict(want[1], ws="debug_ws", reserved=77)] + want[2:]
        assert got == want, cid


def _launches(recs):
    """(case id, index, entry point, its IgemmArgs fields, the case's calls) of every kernel launch that takes an IgemmArgs"""
    for cid, r in recs.items():
        for i, c in enumerate(r["calls"]):
            if c[0] in ("pmi_igemm", "pmi_conv3x3_skip"):
                yield cid, i, c[0], c[1], r["calls"]


def test_the_replay_covers_every_route_step():
    recs = records()
    la = list(_launches(recs))
    descs = [d for r in recs.values() for d, _ in r.get("trace", [])]
    cfgs = {int(m.group(1)) for d in descs for m in [re.search(r" halo=(-?\d+)", d)] if m}
    assert cfgs >= {0, 1, 2, 3, 4, 6, 7, 8, 9, -1}, cfgs
    ptrs = {v.rsplit(".", 1)[-1] for r in recs.values() for c in r["calls"] for x in c[1:] if isinstance(x, dict) for v in x.values() if isinstance(v, str)}
    for need in ("frag16(64)", "frag16(32)", "frag(64)", "frag_c8", "frag16_up(64)", "frag_gemm", "frag_skip"):
        assert need in ptrs, (need, sorted(ptrs))
    assert any(re.fullmatch(r"frag16\(\d+,dup_g=\d+\)", p) for p in ptrs), sorted(ptrs)
    has = lambda pred: any(pred(a) for *_, a, _ in la)
    assert has(lambda a: a.get("reserved3") == 1) and has(lambda a: a.get("reserved3") == 2)
    assert has(lambda a: a.get("splitk", 0) > 1 and "ws" in a)
    assert has(lambda a: "stats" in a and a.get("stats_p", 0) > 0)
    assert has(lambda a: "pro_a" in a and "pro_b" in a)
    assert has(lambda a: "D2" in a) and has(lambda a: "aux" in a)
    assert has(lambda a: a.get("act") == 5)
    assert has(lambda a: a.get("split_in") == 1) and has(lambda a: a.get("split_in") == 2) and has(lambda a: "split_out" in a)
    assert has(lambda a: "A1" in a and a["A1"] == a["A0"]), "self_concat"
    assert has(lambda a: str(a.get("A0", "")).startswith("cat")), "a concat_inputs layer"
    assert has(lambda a: a.get("taps") == 9 and str(a.get("Bf", "")).endswith("frag_gemm")), "conv-mode GEMM"
    # its hand-back: a convolution the conv mode takes, unsplit with a per-sample bias or an up-sampled residual, launched without Bf
    assert has(lambda a: a.get("taps") == 9 and a.get("stride") == 1 and "up" not in a and "Bf" not in a and "split_in" not in a and "pro_a" not in a
               and a["C0"] % 128 == 0 and a.get("C1", 0) % 128 == 0 and a["N"] % 32 == 0 and ("nbias" in a or "res_up" in a) and a.get("splitk", 0) <= 1)
    before = lambda name, entry: any(c[0] == name for _, i, e, _, calls in la if e == entry for c in calls[:i])
    assert before("pmi_gn_apply", "pmi_igemm"), "the apply pass in front of a launch"
    assert before("pmi_split_from_f32", "pmi_igemm"), "the mixed fall-back's residual conversion"
    assert any(c[0] == "pmi_geglu" for r in recs.values() for c in r["calls"])
    assert any(e == "pmi_conv3x3_skip" for _, _, e, _, _ in la)
    # a conv-mode packing that the statistics of step 9 disqualify: launched with Bf = frag_gemm and stats, traced as what runs, wd=0
    assert any(str(a.get("Bf", "")).endswith("frag_gemm") and "stats" in a and a.get("taps") == 9 and " wd=0 " in recs[cid]["trace"][-1][0] + " "
               for cid, _, _, a, _ in la), "conv mode with statistics"
    refused = [cid for cid, r in recs.items() if cid.startswith("skip/") and [c[0] for c in r["calls"]] == ["pmi_igemm", "pmi_igemm"]]
    assert refused, "no refused skip (two pmi_igemm launches)"


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_igemm_calls_cpu.py --record")
    os.makedirs(os.path.dirname(SNAPSHOT), exist_ok=True)
    with open(SNAPSHOT, "w") as f:
        f.write(dump(records()))
    print(f"{len(_RECORDS)} records -> {SNAPSHOT}")
