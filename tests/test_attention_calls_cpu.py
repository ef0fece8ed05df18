"""CPU: what the attention family of perceptor_amd/engine/ops.py hands to the library, call by call, against a recorded snapshot
(tests/snapshots/attention_calls.json).

Built on the Recorder / recording() of tests/test_igemm_calls_cpu.py: the entry points run on CPU tensors with the launches recorded instead
of run, and the host queries (pmi_attn_flash_workspace, pmi_attn_flash_bwd_workspace, pmi_attn_flash_bwd_kv_workspace) are the library's
own.  What differs from the igemm snapshot, because this one has to hold still while the code between the entry points and the launches is
rearranged:

  * only the tensors a case itself makes have names (qkv, q, kv, d_out, da): a view that one ops function hands to another is an offset
    into its tensor (qkv+128), whatever parameter it travels through;
  * the buffers ops allocates are numbered in the order in which a launch first names them, not in the order of allocation: moving a
    torch.empty does not show;
  * a record also holds, per returned tensor, shape, dtype, stride and the buffer it is, and the shapes of everything kept in `saved`.

    python tests/test_attention_calls_cpu.py --record       # regenerate after an INTENDED change, and review the diff
"""
import contextlib
import json
import os
import re
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SNAPSHOT = os.path.join(HERE, "snapshots", "attention_calls.json")
if __name__ == "__main__":
    sys.path[:0] = [HERE, os.path.dirname(HERE)]

import test_igemm_calls_cpu as IG

N, H = 2, 3
TS = (5, 33)                    # one token count below a pad unit of 8, one above a 32-row tile
TT = ((5, 7), (33, 77))         # (T, Tk) of the cross-attention cases


def _as_ptr(a, tab):
    """an address an entry point computed itself (data_ptr() + offset) instead of taking it from ops.ptr: an int that lies inside a tensor
    the case made or ops allocated (tab: Recorder.table() at the time of the call)"""
    return IG._Ptr(a) if type(a) is int and any(base <= a < base + span for base, span, _ in tab) else a


def _renumber(calls, allocs):
    """alloc<i> in allocation order -> alloc<j> in the order of first use by a launch; -> (calls, the allocations in that order, the
    substitution for further roles).  A buffer that no launch names has no number and is not listed: the library never sees it."""
    order = {}

    def sub(role):
        m = re.match(r"alloc(\d+)", role)
        if not m:
            return role
        return f"alloc{order.setdefault(int(m.group(1)), len(order))}" + role[m.end():]

    def walk(v):
        if isinstance(v, str):
            return sub(v)
        if isinstance(v, dict):
            return {k: walk(x) for k, x in v.items()}
        return [walk(x) for x in v] if isinstance(v, list) else v
    calls = [[c[0]] + [walk(a) for a in c[1:]] for c in calls]
    return calls, [allocs[i] for i in order], sub


def replay(case):
    """one case -> its record.  case(mk) makes its inputs with mk(role, shape, dtype) and returns {name: what an entry point returned};
    names that start with "saved" hold what a *_train call keeps for its backward"""
    _, ops = _ops()
    unwrapped = {name: getattr(ops, name) for name in IG.ENTRY_POINTS}
    with IG.recording("off") as rec:
        for name, fn in unwrapped.items():      # recording() wraps these to name their tensor arguments: here only the case names tensors
            setattr(ops, name, fn)              # (recording() puts back what it found on the way out)
        ops.call = lambda name, *args: rec.call(name, *[_as_ptr(a, rec.table()) for a in args])

        def mk(role, shape, dtype):
            t = torch.zeros(shape, dtype=dtype)
            rec.name(t, role)
            return t
        ret = case(mk)
        calls, allocs, sub = _renumber(rec.finish(), rec.allocs)
        tab = rec.table()

        def describe(v, shapes_only):
            if isinstance(v, torch.Tensor):
                if shapes_only:
                    return list(v.shape)
                return {"shape": list(v.shape), "dtype": IG.DTN[v.dtype], "stride": list(v.stride()), "at": sub(rec.resolve(v.data_ptr(), tab))}
            return [describe(x, shapes_only) for x in v] if isinstance(v, (tuple, list)) else v
        return {"calls": calls, "allocs": allocs, "ret": {k: describe(v, k.startswith("saved")) for k, v in ret.items()}}


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _ops():
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    return _hip, ops


@contextlib.contextmanager
def _flash(enabled):
    _, ops = _ops()
    old, ops.FLASH_ENABLED = ops.FLASH_ENABLED, enabled
    try:
        yield
    finally:
        ops.FLASH_ENABLED = old


def _attention(mk, T, d, order, dtype, causal=False, flash=True):
    """dtype "precise": DT_F16X2 on a precise [N, T, 2*3C] tensor"""
    _hip, ops = _ops()
    c = H * d
    qkv = mk("qkv", (N, T, 6 * c), torch.float16) if dtype == "precise" else mk("qkv", (N, T, 3 * c), IG.TD[dtype])
    with _flash(flash):
        return {"out": ops.attention(qkv, H, order, _hip.dtype_code(dtype), causal=causal)}


def _cross(mk, T, Tk, d, dtype, flash=True):
    _hip, ops = _ops()
    c = H * d
    q, kv = mk("q", (N, T, c), IG.TD[dtype]), mk("kv", (N, Tk, 2 * c), IG.TD[dtype])
    with _flash(flash):
        return {"out": ops.cross_attention(q, kv, H, _hip.dtype_code(dtype))}


def _train_backward(mk, T, d, dtype):
    _hip, ops = _ops()
    c, dt = H * d, _hip.dtype_code(dtype)
    qkv = mk("qkv", (N, T, 3 * c), IG.TD[dtype])
    out, p = ops.attention_train(qkv, H, dt)
    return {"out": out, "p": p, "dqkv": ops.attention_backward(qkv, p, mk("d_out", (N, T, c), IG.TD[dtype]), H, dt)}


def _cross_train_backward(mk, T, Tk, d, dtype, with_q):
    _hip, ops = _ops()
    c, dt = H * d, _hip.dtype_code(dtype)
    q, kv = mk("q", (N, T, c), IG.TD[dtype]), mk("kv", (N, Tk, 2 * c), IG.TD[dtype])
    out, p = ops.cross_attention_train(q, kv, H, dt)
    return {"out": out, "p": p,
            "grad": ops.cross_attention_backward(kv, p, mk("d_out", (N, T, c), IG.TD[dtype]), H, dt, q=q if with_q else None)}


def _flash_family(mk, kind, T, Tk, d, dtype):
    """flash_attention, flash_attention_train and flash_attention_backward on one set of operands.  kind "self": the three slices of one qkv;
    "cross_dq": q and the two halves of one kv, dq_only; "cross_kv": the same without dq_only (pmi_attn_flash_bwd_kv)"""
    _hip, ops = _ops()
    c, dt = H * d, _hip.dtype_code(dtype)
    if kind == "self":
        qkv = mk("qkv", (N, T, 3 * c), IG.TD[dtype])
        q, k, v = qkv, qkv[..., c:], qkv[..., 2 * c:]
    else:
        q, kv = mk("q", (N, T, c), IG.TD[dtype]), mk("kv", (N, Tk, 2 * c), IG.TD[dtype])
        k, v = kv, kv[..., c:]
    plain = ops.flash_attention(q, k, v, H, d, dt)
    out, saved = ops.flash_attention_train(q, k, v, H, d, dt)
    grad = ops.flash_attention_backward(saved, mk("d_out", (N, T, c), IG.TD[dtype]), H, d, dt, dq_only=kind == "cross_dq")
    return {"plain": plain, "out": out, "saved": saved, "grad": grad}


def _self_train_backward(mk, T, d, dtype):
    _hip, ops = _ops()
    c, dt = H * d, _hip.dtype_code(dtype)
    w, td = (2, torch.float16) if dtype == "precise" else (1, IG.TD[dtype])
    a, saved = ops.self_attention_train(mk("qkv", (N * T, w * 3 * c), td), N, T, H, dt)
    return {"a": a, "saved": saved, "dqkv": ops.self_attention_backward(saved, mk("da", (N * T, w * c), td), N, T, H, dt)}


def _precise_train_backward(mk, T, d):
    _hip, ops = _ops()
    c = H * d
    out, saved = ops.attention_precise_train(mk("qkv", (N * T, 6 * c), torch.float16), N, T, H)
    return {"out": out, "saved": saved, "dqkv": ops.attention_precise_backward(saved, mk("da", (N * T, 2 * c), torch.float16), N, T, H)}


def _cases():
    """id -> case(mk).  bf16 throughout, f16 once per entry point (dt is only passed through)"""
    cs = {}

    def add(cid, fn, *a, **kw):
        cs[cid] = lambda mk: fn(mk, *a, **kw)
    for T in TS:
        for order in (0, 1):
            add(f"attention/d64/order{order}/T{T}/bf16", _attention, T, 64, order, "bf16")
            add(f"attention/precise/order{order}/T{T}", _attention, T, 32, order, "precise")
        add(f"attention/d32/order0/T{T}/bf16", _attention, T, 32, 0, "bf16")
        add(f"attention/d32/order1/flash/T{T}/bf16", _attention, T, 32, 1, "bf16")
        add(f"attention/d32/order1/gemm/T{T}/bf16", _attention, T, 32, 1, "bf16", flash=False)
        add(f"attention/d168/order1/T{T}/bf16", _attention, T, 168, 1, "bf16")
        add(f"attention_train/d32/T{T}/bf16", _train_backward, T, 32, "bf16")
        add(f"attention_train/d168/T{T}/bf16", _train_backward, T, 168, "bf16")
        add(f"self_attention_train/d64/T{T}/bf16", _self_train_backward, T, 64, "bf16")
        add(f"self_attention_train/d32/T{T}/bf16", _self_train_backward, T, 32, "bf16")
        add(f"self_attention_train/precise/T{T}", _self_train_backward, T, 32, "precise")
        add(f"flash/self/d40/T{T}/bf16", _flash_family, "self", T, T, 40, "bf16")
    add("attention/d64/causal/T77/bf16", _attention, 77, 64, 1, "bf16", causal=True)
    add("attention/d32/order0/T33/f16", _attention, 33, 32, 0, "f16")
    add("attention_train/d32/T33/f16", _train_backward, 33, 32, "f16")
    add("self_attention_train/d32/T33/f16", _self_train_backward, 33, 32, "f16")
    add("flash/self/d40/T33/f16", _flash_family, "self", 33, 33, 40, "f16")
    add("attention_precise_train/d32/T33", _precise_train_backward, 33, 32)
    for T, Tk in TT:
        add(f"cross_attention/d40/flash/T{T}x{Tk}/bf16", _cross, T, Tk, 40, "bf16")
        add(f"cross_attention/d40/gemm/T{T}x{Tk}/bf16", _cross, T, Tk, 40, "bf16", flash=False)
        add(f"cross_attention/d168/T{T}x{Tk}/bf16", _cross, T, Tk, 168, "bf16")
        add(f"cross_attention_train/d40/dq/T{T}x{Tk}/bf16", _cross_train_backward, T, Tk, 40, "bf16", False)
        add(f"cross_attention_train/d40/dq_dkv/T{T}x{Tk}/bf16", _cross_train_backward, T, Tk, 40, "bf16", True)
        add(f"flash/cross_dq/d40/T{T}x{Tk}/bf16", _flash_family, "cross_dq", T, Tk, 40, "bf16")
        add(f"flash/cross_kv/d40/T{T}x{Tk}/bf16", _flash_family, "cross_kv", T, Tk, 40, "bf16")
    add("cross_attention/d40/gemm/T33x77/f16", _cross, 33, 77, 40, "f16", flash=False)
    add("cross_attention_train/d40/dq_dkv/T33x77/f16", _cross_train_backward, 33, 77, 40, "f16", True)
    return cs


CASES = _cases()
_RECORDS = {}


def records():
    if not _RECORDS:
        for cid, case in CASES.items():
            _RECORDS[cid] = replay(case)
    return _RECORDS


# ---- tests ------------------------------------------------------------------------------------------------------------------------
def test_calls_match_the_snapshot():
    with open(SNAPSHOT) as f:
        want = json.load(f)
    got = json.loads(IG.dump(records()))
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    for cid in want:
        assert got[cid] == want[cid], f"{cid}:\n  recorded {json.dumps(want[cid])}\n  now      {json.dumps(got[cid])}"


def test_every_pointer_has_a_role():
    for cid, r in records().items():
        assert '"?"' not in json.dumps([r["calls"], r["ret"]]), (cid, r)
        # and no address slipped through as a number
        assert not re.search(r"[\[,:]\d{10,}[\],}]", json.dumps(r["calls"], separators=(",", ":"))), (cid, r["calls"])


def test_buffer_numbers_follow_the_launches():
    """the numbering itself: a buffer allocated first and used last is the last number, one no launch names is not listed"""
    calls = [["k0", "alloc2+8", 3, "qkv+4"], ["k1", {"A0": "alloc0", "D": "alloc2"}]]
    got, allocs, sub = _renumber(calls, ["f32[1]", "bf16[2]", "bf16[3]"])
    assert got == [["k0", "alloc0+8", 3, "qkv+4"], ["k1", {"A0": "alloc1", "D": "alloc0"}]]
    assert allocs == ["bf16[3]", "f32[1]"]
    assert sub("alloc0+16") == "alloc1+16" and sub("kv+2") == "kv+2"


def test_the_replay_covers_the_family():
    """every library entry point the attention family launches appears in some record"""
    seen = {c[0] for r in records().values() for c in r["calls"]}
    need = {"pmi_qkv_split", "pmi_attn_d64", "pmi_igemm", "pmi_softmax_fwd", "pmi_softmax_causal_fwd", "pmi_softmax_bwd", "pmi_transpose_16",
            "pmi_attn_flash", "pmi_attn_flash_train", "pmi_attn_flash_bwd", "pmi_attn_flash_bwd_kv", "pmi_vit_attn_fwd", "pmi_vit_attn_bwd",
            "pmi_split_to_f32", "pmi_gemm_f32", "pmi_softmax_f32", "pmi_softmax_bwd_f32", "pmi_split_from_f32"}
    assert seen == need, sorted(seen ^ need)


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_attention_calls_cpu.py --record")
    os.makedirs(os.path.dirname(SNAPSHOT), exist_ok=True)
    with open(SNAPSHOT, "w") as f:
        f.write(IG.dump(records()))
    print(f"{len(_RECORDS)} records -> {SNAPSHOT}")
