"""CPU: what the diffusion engines (engine/adm.py, adm_mixed.py, sd.py, vdiff.py) hand to the library over a whole forward() and a whole
forward_train() + backward(), launch by launch, against a recorded snapshot (tests/snapshots/engine_calls.json).

The engines' public entry points run on CPU tensors with the launches recorded instead of run: ptr and call are replaced in ops, adm, sd
and vdiff, ops._empty returns zero-filled buffers (ops.grad_to_nhwc reads the f16 gradient scale back from one), the host queries are the
library's own, and the input tensors answer is_cuda with True.  A record holds, per launch, the entry point, every scalar argument and every
non-zero field of an IgemmArgs / SkipArgs / GemmF32Args (the flattening of test_igemm_calls_cpu.Recorder.call), with each pointer replaced
by b<i>[+offset]: the i-th buffer a launch of the case named, in order of first use, so that moving an allocation does not show.  Per
returned tensor it holds shape, dtype and stride.  The ten cases make 4547 launches, 0.6 MB as text, so the snapshot keeps of them what
summary() says: per case and mode the number of launches, the number per entry point and a digest of every 16 consecutive records.  It holds
still while the code between the entry points and the launches is rearranged:

    python tests/test_engine_calls_cpu.py --record       # regenerate after an INTENDED change ...
    python tests/test_engine_calls_cpu.py --full FILE    # ... and review it: every launch, one per line, to diff between the two commits

test_resblocks_launch_alike_in_both_modes holds the fact the engines' shared ResBlocks rest on: a ResBlock of the ADM UNet, the SD UNet
and the VAE issues the same launches, arguments included, in forward() and in forward_train().
"""
import bisect
import hashlib
import json
import os
import re
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SNAPSHOT = os.path.join(HERE, "snapshots", "engine_calls.json")
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.dirname(HERE)]

import test_gpu_adm as ADM
import test_igemm_calls_cpu as IG

_RESBLOCK = re.compile(r"_(res|resnet|vae_resnet)(_train)?$")     # the ResBlock forms of AdmEngine and sd._Blocks / SdUnetEngine


class _OnDevice(torch.Tensor):
    """an input tensor that passes the engines' is_cuda guards"""
    is_cuda = property(lambda self: True)


def _modules():
    from perceptor_amd.engine import adm, adm_mixed, ops, sd, vdiff
    return adm, adm_mixed, ops, sd, vdiff


class Recording:
    """The seams replaced for one case.  Every tensor that ptr is given, that ops._empty allocates or that ops.gemm_f32 takes the address of is
    kept alive to the end of the case, so an address names one buffer (a storage: a view is an offset into it); pointers are resolved once
    the case is over."""

    def __init__(self):
        adm, _, ops, sd, vdiff = _modules()
        self.rec, self.kept, self.spans, self.saved = IG.Recorder(ops), [], [], []
        for mod in (ops, adm, sd, vdiff):
            self._set(mod, "ptr", self.ptr)
            self._set(mod, "call", self.rec.call)
        self._set(ops, "_empty", lambda shape, dtype, device: self.keep(torch.zeros(tuple(shape), dtype=dtype, device=device)))
        gemm_f32 = ops.gemm_f32          # takes the addresses of its operands itself
        self._set(ops, "gemm_f32", lambda A, B, D, **kw: gemm_f32(self.keep(A), self.keep(B), self.keep(D), **kw))
        for cls in (adm.AdmEngine, sd._Blocks, sd.SdUnetEngine):
            for name, fn in list(vars(cls).items()):
                if _RESBLOCK.match(name):
                    self._set(cls, name, self._marked(fn))

    def _set(self, obj, name, value):
        self.saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)

    def close(self):
        for obj, name, value in reversed(self.saved):
            setattr(obj, name, value)

    def keep(self, t):
        self.kept.append(t)
        return t

    def ptr(self, t):
        return None if t is None else IG._Ptr(self.keep(t).data_ptr())

    def _marked(self, fn):
        """a ResBlock form that notes which launches are its own: (its layer's key, first launch, one past its last)"""
        def marked(eng, l, *args, **kw):
            first = len(self.rec.calls)
            out = fn(eng, l, *args, **kw)
            self.spans.append((getattr(l, "p", l), first, len(self.rec.calls)))
            return out
        return marked

    def launches(self):
        """the calls with every address -- from ptr, or computed by the caller as data_ptr() + offset -- as b<i>[+offset]; "?" if it lies in
        no buffer that ptr has seen"""
        bufs = sorted({(s.data_ptr(), s.nbytes()) for s in (t.untyped_storage() for t in self.kept) if s.nbytes()})
        bases, number = [b for b, _ in bufs], {}

        def res(v):
            if isinstance(v, dict):
                return {k: res(x) for k, x in v.items()}
            if type(v) is not IG._Ptr and not (type(v) is int and v >= 1 << 32):
                return v
            i = bisect.bisect_right(bases, int(v)) - 1
            if i < 0 or int(v) >= bufs[i][0] + bufs[i][1]:
                return "?"
            off = int(v) - bufs[i][0]
            return f"b{number.setdefault(i, len(number))}" + (f"+{off}" if off else "")
        return [[name] + [res(a) for a in args] for name, args, _, _ in self.rec.calls]


def _describe(v):
    if isinstance(v, torch.Tensor):
        return {"shape": list(v.shape), "dtype": IG.DTN[v.dtype], "stride": list(v.stride())}
    return [_describe(x) for x in v]


def replay(case):
    """one case -> its record.  case() -> (engine, forward's arguments, forward_train's, backward's given the tape); the last two None for an
    engine without an input gradient"""
    r = Recording()
    try:
        eng, fwd, train, back = case()
        out = {"forward_ret": _describe(eng.forward(*fwd))}
        marks = [len(r.rec.calls)]
        if train is not None:
            y, tape = eng.forward_train(*train)
            marks.append(len(r.rec.calls))
            out["train_ret"], out["backward_ret"] = _describe(y), _describe(eng.backward(tape, *back(y)))
        calls = r.launches()
        out["forward"], out["train"] = calls[:marks[0]], calls[marks[0]:]
        # the ResBlocks of forward() and of forward_train(), by layer: their launches with the buffers numbered within the block
        out["blocks"] = [{}, {}]
        for key, first, last in r.spans:
            if last <= marks[-1]:
                out["blocks"][first >= marks[0]][key] = _renumbered(calls[first:last])
        return out
    finally:
        r.close()


def _renumbered(calls):
    number = {}
    sub = lambda m: f"b{number.setdefault(m.group(0), len(number))}"
    return json.loads(re.sub(r"(?<=\")b\d+", sub, json.dumps(calls)))


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _in(*shape):
    return torch.zeros(shape).as_subclass(_OnDevice)


def _synth(shapes):
    from perceptor_amd.utils.synth import synth_state_dict
    return synth_state_dict(shapes, 0)


def _adm(tag, dtype):
    adm = _modules()[0]
    cfg = adm.AdmConfig(**ADM.TINY[tag])
    sd = _synth(adm.state_dict_shapes(cfg))
    x, t = _in(2, 3, 32, 32), torch.zeros(2)
    return adm.AdmEngine(cfg, sd, "cpu", dtype), (x, t), (x, t, sd), lambda y: (torch.zeros_like(y), sd)


def _adm_mixed():
    adm, adm_mixed = _modules()[:2]
    cfg = adm.AdmConfig(**ADM.TINY["a"])
    return adm_mixed.AdmMixedEngine(cfg, _synth(adm.state_dict_shapes(cfg)), "cpu", plain_from=4), (_in(2, 3, 32, 32), torch.zeros(2)), None, None


def _sd_unet(dtype, flash_backward, cond_grad):
    sd_ = _modules()[3]
    cfg = sd_.SdConfig(block_out=(32, 64, 64), cross_attn=(True, True, False), heads=2, context_dim=32, layers_per_block=1)
    sd = _synth(sd_.unet_state_dict_shapes(cfg))
    eng = sd_.SdUnetEngine(cfg, sd, "cpu", dtype)
    eng.flash_backward = flash_backward
    args = (_in(2, 4, 16, 16), torch.zeros(2), _in(2, 7, 32))
    return eng, args, args, lambda y: (_in(*y.shape), sd, cond_grad)


def _vae(which):
    sd_ = _modules()[3]
    cfg = sd_.VaeConfig(block_out=(32, 64), layers_per_block=1)
    if which == "decoder":
        sd = _synth(sd_.vae_decoder_state_dict_shapes(cfg))
        return sd_.VaeDecoderEngine(cfg, sd, "cpu", "bf16"), (_in(1, 4, 8, 8),), (_in(1, 4, 8, 8),), lambda y: (_in(*y.shape), sd)
    sd = _synth(sd_.vae_encoder_state_dict_shapes(cfg))
    return sd_.VaeEncoderEngine(cfg, sd, "cpu", "bf16"), (_in(1, 3, 16, 16),), (_in(1, 3, 16, 16),), lambda y: (_in(*y[0].shape), _in(*y[1].shape), sd)


def _vdiff(cond):
    vdiff = _modules()[4]
    spec = vdiff.make_spec("tiny", (3, 32, 32), [64, 128, 128], 2, 2, 4, 1, cond)
    sd = _synth(vdiff.state_dict_shapes(spec))
    args = (_in(2, 3, 32, 48), torch.full((2,), 0.5)) + ((torch.ones(2, 512),) if cond else ())
    return vdiff.VDiffEngine(spec, sd, "cpu", "bf16"), args, args, lambda y: (torch.zeros_like(y), sd)


CASES = {
    "adm/a/bf16": lambda: _adm("a", "bf16"),
    "adm/a/precise": lambda: _adm("a", "precise"),
    "adm/b/f16": lambda: _adm("b", "f16"),
    "sd_unet/f16/flash/cond_grad": lambda: _sd_unet("f16", True, True),
    "sd_unet/bf16/kept_p": lambda: _sd_unet("bf16", False, False),
    "vae_decoder/bf16": lambda: _vae("decoder"),
    "vae_encoder/bf16": lambda: _vae("encoder"),
    "vdiff/uncond/bf16": lambda: _vdiff(False),
    "vdiff/cond/bf16": lambda: _vdiff(True),
    "adm_mixed/a/plain_from4": _adm_mixed,
}
_RECORDS = {}


def records():
    if not _RECORDS:
        for cid, case in CASES.items():
            _RECORDS[cid] = replay(case)
    return _RECORDS


def dump(recs):
    """every launch of every record, one per line (--full: the text to diff between two commits; 0.6 MB, not committed)"""
    lines = lambda calls: "[\n" + ",\n".join(json.dumps(c, separators=(",", ":")) for c in calls) + "\n]"
    return "{\n" + ",\n".join(
        f"{json.dumps(cid)}: {{" + ", ".join(f"{json.dumps(k)}: " + (lines(v) if k in ("forward", "train") else json.dumps(v, separators=(",", ":")))
                                             for k, v in r.items() if k != "blocks") + "}" for cid, r in recs.items()) + "\n}\n"


WINDOW = 16


def summary(r):
    """What the snapshot keeps of a record: the returned tensors as they are and, of forward's and of forward_train + backward's launches, their
    number, the number per entry point and one digest (sha256, 12 hex digits) per WINDOW consecutive launches, arguments included -- any change of
    any launch changes a digest, and the digest that changed says where."""
    out = {k: v for k, v in r.items() if k.endswith("_ret")}
    for k in ("forward", "train"):
        names = {}
        for c in r[k]:
            names[c[0]] = names.get(c[0], 0) + 1
        digests = [hashlib.sha256(json.dumps(r[k][i:i + WINDOW], separators=(",", ":")).encode()).hexdigest()[:12] for i in range(0, len(r[k]), WINDOW)]
        out[k] = {"launches": len(r[k]), "entry_points": dict(sorted(names.items())), "digests": digests}
    return out


def dump_snapshot(recs):
    return "{\n" + ",\n".join(f"{json.dumps(cid)}: {{\n" + ",\n".join(f"  {json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}" for k, v in summary(r).items())
                              + "\n}" for cid, r in recs.items()) + "\n}\n"


# ---- tests ------------------------------------------------------------------------------------------------------------------------
def test_calls_match_the_snapshot():
    with open(SNAPSHOT) as f:
        want = json.load(f)
    recs = records()
    assert sorted(recs) == sorted(want), (sorted(set(recs) ^ set(want)))
    for cid in want:
        got = summary(recs[cid])
        assert sorted(got) == sorted(want[cid]), cid
        for k, w in want[cid].items():
            g = got[k]
            if k in ("forward", "train"):
                assert (g["launches"], g["entry_points"]) == (w["launches"], w["entry_points"]), f"{cid} {k}:\n  recorded {w['launches']} {w['entry_points']}\n  now      {g['launches']} {g['entry_points']}"
                for i, (a, b) in enumerate(zip(g["digests"], w["digests"])):
                    now = "\n".join(f"  [{j}] {json.dumps(c)}" for j, c in enumerate(recs[cid][k][i * WINDOW:(i + 1) * WINDOW], i * WINDOW))
                    assert a == b, f"{cid} {k}: a launch in [{i * WINDOW}, {(i + 1) * WINDOW}) is not the recorded one (--full at both commits shows which); now:\n{now}"
            assert g == w, (cid, k, w, g)


def test_every_pointer_resolved_to_a_buffer():
    for cid, r in records().items():
        text = json.dumps([r["forward"], r["train"]], separators=(",", ":"))
        assert '"?"' not in text, cid
        assert not re.search(r"[\[,:]\d{10,}[\],}]", text), cid      # and no address slipped through as a number


def test_resblocks_launch_alike_in_both_modes():
    """every ResBlock of the ADM UNet, the SD UNet and the VAE: forward()'s launches are forward_train()'s, arguments included"""
    adm, _, _, sd_, _ = _modules()
    for cid, r in records().items():
        fwd, train = r["blocks"]
        if cid.startswith("vdiff") or cid.startswith("adm_mixed"):
            continue
        assert fwd and sorted(fwd) == sorted(train), cid
        for key in fwd:
            assert fwd[key] and fwd[key] == train[key], f"{cid} {key}:\n  forward       {json.dumps(fwd[key])}\n  forward_train {json.dumps(train[key])}"
    plan = adm.build_plan(adm.AdmConfig(**ADM.TINY["a"]))
    want = {l.p for layers in plan[0] + [plan[1]] + plan[2] for l in layers if isinstance(l, adm._Res)}
    assert set(records()["adm/a/bf16"]["blocks"][0]) == want
    assert len(records()["sd_unet/f16/flash/cond_grad"]["blocks"][0]) == 3 + 2 + 6 and len(records()["vae_decoder/bf16"]["blocks"][0]) == 2 + 4


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"] and sys.argv[1:2] != ["--full"]:
        sys.exit("usage: python tests/test_engine_calls_cpu.py --record | --full FILE")
    os.makedirs(os.path.dirname(SNAPSHOT), exist_ok=True)
    with open(SNAPSHOT if sys.argv[1] == "--record" else sys.argv[2], "w") as f:
        f.write(dump_snapshot(records()) if sys.argv[1] == "--record" else dump(records()))
    print({cid: (len(r["forward"]), len(r["train"])) for cid, r in _RECORDS.items()}, "->", f.name)
