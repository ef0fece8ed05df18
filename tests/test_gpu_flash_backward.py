"""GPU: the flash attention backward (csrc/attn_flash.hip: pmi_attn_flash_bwd in its self-attention and dq_only forms, pmi_attn_flash_bwd_kv
with flash_kv_reduce_kernel) and the training forward's lse, against the float64 model and the per-element bounds of
tests/_flash_bwd_ref64.py, at every head dim (all ten (KQ, DB) instantiations of each family, both dtypes) and at ragged lengths.

The C entry points are called directly.  Every buffer a call writes -- forward workspace, lse, out, backward workspace, delta, gradients
-- is NaN beforehand; q | k | v (self) or q and k | v (cross) are views with a row pitch above heads * d; the gradients land in column
slices of wider NaN buffers with a guard row before and after, which must still be NaN afterwards, every written element finite.  Per
case: two runs give the same bits, sample 1 alone gives the same bits, the kv form's dq is the dq_only form's dq bit for bit, and dQ, dK,
dV, lse and delta sit inside their bounds (printed as err/bound).  tests/test_flash_backward_bounds_cpu.py shows on the CPU that an fp32
emulation of the kernels' arithmetic is inside these bounds at the same cases and that the listed defects are outside them.
"""
import functools
import math

import pytest
import torch

import _flash_bwd_ref64 as FB
import _ref64 as R
from test_gpu_attention import _dev, _heads_to_tokens, _nan, _tokens_to_heads

pytestmark = pytest.mark.gpu

DTYPES = FB.DTYPES
LN2 = math.log(2.0)


def _id(case):
    return "-".join(str(x) for x in case)


@functools.lru_cache(maxsize=None)
def _operands(case, dtype, do_scale=1.0):
    return FB.operands(case, dtype, do_scale)


@functools.lru_cache(maxsize=None)
def _model(case, dtype, do_scale=1.0, fp32_kv=False, S=1):
    return FB.model(*_operands(case, dtype, do_scale), dtype, fp32_kv=fp32_kv, S=S)


def _device_operands(case, dtype, do_scale, cross):
    """(q, k, v) views and a contiguous dO on the device.  Self: the three slices of one [N, T, 3C] tensor.  Cross: q the first C columns
    of a [N, T, C + 8] tensor whose other columns are NaN, k | v the halves of [N, Tk, 2C] with 19 NaN rows behind the last sample."""
    d, T, Tk, N, H, _ = case
    dev, td, C = _dev(), R.TD[dtype], H * d
    q, k, v, dO = _operands(case, dtype, do_scale)
    qt, kt, vt = (_heads_to_tokens(z, N, H) for z in (q, k, v))
    if not cross:
        buf = torch.cat([qt, kt, vt], -1).to(td).to(dev)
        views = (buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:])
    else:
        qb = _nan((N, T, C + 8), td, dev)
        qb[..., :C] = qt.to(td).to(dev)
        flat = _nan((N * Tk + 19, 2 * C), td, dev)
        flat[:N * Tk] = torch.cat([kt, vt], -1).reshape(N * Tk, 2 * C).to(td).to(dev)
        kv = flat[:N * Tk].view(N, Tk, 2 * C)
        views = (qb[..., :C], kv[..., :C], kv[..., C:])
    return views, _heads_to_tokens(dO, N, H).to(td).to(dev).contiguous()


def _guarded(rows, cols, dtype, dev):
    """NaN buffer [rows + 2, cols + 8]; the payload is rows 1 .. rows, columns 4 .. cols + 4.  -> (buffer, payload view, payload pointer)"""
    g = _nan((rows + 2, cols + 8), dtype, dev)
    return g, g[1:rows + 1, 4:cols + 4], g.data_ptr() + (cols + 8 + 4) * g.element_size()


def _check_guards(g, what):
    inner = g[1:-1, 4:-4]
    assert bool(torch.isfinite(inner).all()), f"{what}: an element was left unwritten or is not finite"
    assert bool(torch.isnan(g[0]).all() and torch.isnan(g[-1]).all() and torch.isnan(g[:, :4]).all() and torch.isnan(g[:, -4:]).all()), \
        f"{what}: written outside its slice"


def _forward(views, N, T, Tk, H, d, dtype):
    """pmi_attn_flash_train with NaN workspace, lse and out -> (out, ws, lse)"""
    from perceptor_amd import _hip
    from perceptor_amd._hip import call, dtype_code, ptr
    q, k, v = views
    dev, td = q.device, q.dtype
    kib = _hip.lib().pmi_attn_flash_workspace(N, T, Tk, H, d)
    assert kib > 0
    ws = _nan((kib * 512,), td, dev)
    lse = _nan((N * H, (T + 31) // 32 * 32), torch.float32, dev)
    out = _nan((N, T, H * d), td, dev)
    call("pmi_attn_flash_train", q.data_ptr(), q.stride(1), k.data_ptr(), v.data_ptr(), k.stride(1), ptr(out), ptr(ws), ptr(lse), N, T, Tk, H, d,
         float(d) ** -0.5, dtype_code(dtype))
    return out, ws, lse


def _backward(form, views, dout, N, T, Tk, H, d, dtype):
    """Training forward, then the backward in one form: 'self' (dq_only = 0), 'dq' (dq_only = 1) or 'kv' (pmi_attn_flash_bwd_kv).
    -> dict of out, lse, delta, dq [N, T, C] and, but for 'dq', dk, dv [N, Tk, C] (fp32 for 'kv')"""
    from perceptor_amd import _hip
    from perceptor_amd._hip import call, dtype_code, ptr
    q, k, v = views
    dev, td, C, lib, dt = q.device, q.dtype, H * d, _hip.lib(), dtype_code(dtype)
    out, ws, lse = _forward(views, N, T, Tk, H, d, dtype)
    delta = _nan(tuple(lse.shape), torch.float32, dev)
    kib = lib.pmi_attn_flash_bwd_kv_workspace(N, T, Tk, H, d) if form == "kv" else lib.pmi_attn_flash_bwd_workspace(N, T, Tk, H, d, int(form == "dq"))
    assert kib > 0
    wsb = _nan((kib * 512,), td, dev)
    head = (q.data_ptr(), q.stride(1), k.data_ptr(), v.data_ptr(), k.stride(1), ptr(out), ptr(dout), ptr(ws), ptr(lse), ptr(wsb), ptr(delta))
    tail = (N, T, Tk, H, d, float(d) ** -0.5)
    res = dict(out=out, lse=lse, delta=delta)
    if form == "self":
        g, pay, p = _guarded(N * T, 3 * C, td, dev)
        es = g.element_size()
        call("pmi_attn_flash_bwd", *head, p, 3 * C + 8, p + C * es, p + 2 * C * es, 3 * C + 8, *tail, 0, dt)
        torch.cuda.synchronize()
        _check_guards(g, "dq | dk | dv")
        res.update(dq=pay[:, :C], dk=pay[:, C:2 * C], dv=pay[:, 2 * C:])
    else:
        g, pay, p = _guarded(N * T, C, td, dev)
        if form == "dq":
            call("pmi_attn_flash_bwd", *head, p, C + 8, None, None, 0, *tail, 1, dt)
        else:
            g32, pay32, p32 = _guarded(N * Tk, 2 * C, torch.float32, dev)
            call("pmi_attn_flash_bwd_kv", *head, p, C + 8, p32, p32 + 4 * C, 2 * C + 8, *tail, dt)
        torch.cuda.synchronize()
        _check_guards(g, "dq")
        res.update(dq=pay)
        if form == "kv":
            _check_guards(g32, "dk | dv")
            res.update(dk=pay32[:, :C], dv=pay32[:, C:])
    res = {n: x.cpu() for n, x in res.items()}
    for n, rows in (("dq", T), ("dk", Tk), ("dv", Tk)):
        if n in res:
            res[n] = res[n].reshape(N, rows, C)
    return res


def _same_bits(a, b, what):
    for n in a:
        assert torch.equal(a[n], b[n]), f"{what}: {n} differs"


def _check(tag, res, case, dtype, do_scale=1.0, fp32_kv=False, S=1):
    d, T, Tk, N, H, _ = case
    q, k, v, dO = _operands(case, dtype, do_scale)
    r = _model(case, dtype, do_scale, fp32_kv, S)
    worst = {}
    for n in ("dQ", "dK", "dV"):
        if n.lower() in res:
            worst[n] = FB.check(f"{tag} {n}", _tokens_to_heads(res[n.lower()], N, H), r[n], r["b" + n[1]])
    lse = res["lse"]
    assert bool((lse[:, T:] == 0).all()), "lse rows t >= T must be written as 0"
    worst["lse"] = FB.check(f"{tag} lse", lse[:, :T].double() * LN2, r["lse"], r["blse"])
    assert bool(torch.isfinite(res["out"]).all())
    delta = res["delta"]
    assert bool((delta[:, T:] == 0).all()), "delta rows t >= T must be written as 0"
    want, bound = FB.delta_bound(dO, _tokens_to_heads(res["out"], N, H), d)
    worst["delta"] = FB.check(f"{tag} delta", delta[:, :T], want, bound)
    return worst


def _family(form, case, dtype, do_scale=1.0, S=1):
    """one case of one family: run twice, sample 1 alone, the bounds"""
    d, T, Tk, N, H, regime = case
    views, dout = _device_operands(case, dtype, do_scale, cross=form != "self")
    res = _backward(form, views, dout, N, T, Tk, H, d, dtype)
    _same_bits(res, _backward(form, views, dout, N, T, Tk, H, d, dtype), "two identical launches")
    if N >= 2:      # nothing reduces across (sample, head): sample 1 alone must give the same bits
        one = _backward(form, tuple(z[1:2] for z in views), dout[1:2].contiguous(), 1, T, Tk, H, d, dtype)
        for n in one:      # lse and delta are [N * H, Tp], the others [N, rows, C]
            both = res[n][H:2 * H] if n in ("lse", "delta") else res[n][1:2]
            assert torch.equal(one[n], both), f"sample 1 alone: {n} differs"
    _check(f"flash_bwd {form} d={d} T={T} Tk={Tk} {N}x{H} {regime} {dtype}" + (f" dO*{do_scale:g}" if do_scale != 1.0 else "") + (f" S={S}" if form == "kv" else ""),
           res, case, dtype, do_scale, fp32_kv=form == "kv", S=S)
    return res, views, dout


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", FB.SELF_CASES, ids=_id)
def test_flash_backward_self(case, dtype):
    """attn_flash_bwd_kernel<.., DQ_ONLY = false>: the dQ and dK / dV roles in one launch, on ragged sequences."""
    _family("self", case, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", FB.CROSS_CASES, ids=_id)
def test_flash_backward_cross_dq_only(case, dtype):
    """attn_flash_bwd_kernel<.., DQ_ONLY = true>; the NaN rows behind the keys must not reach the result."""
    _family("dq", case, dtype)


def _kv(case, dtype, S_want, do_scale=1.0):
    from perceptor_amd import _hip
    d, T, Tk, N, H, _ = case
    S = _hip.lib().pmi_attn_flash_bwd_kv_chunks(N, T, Tk, H, d)
    assert S == S_want, f"flash_kv_chunks gives {S} chunks, the case names {S_want}"
    res, views, dout = _family("kv", case, dtype, do_scale, S=S)
    dq = _backward("dq", views, dout, N, T, Tk, H, d, dtype)
    for n in ("dq", "out", "lse", "delta"):
        assert torch.equal(dq[n], res[n]), f"kv form against dq_only = 1: {n} differs"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", FB.CROSS_CASES, ids=_id)
def test_flash_backward_kv_one_chunk(case, dtype):
    """attn_flash_bwd_kv_kernel with S = 1: the accumulators go straight to the fp32 dK | dV."""
    _kv(case, dtype, 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("opt", [0, 1, 2])
@pytest.mark.parametrize("case", FB.KV_SPLIT_CASES, ids=_id)
def test_flash_backward_kv_split(case, opt, dtype):
    """The key role split over query chunks and flash_kv_reduce_kernel; pmi_set_option(14, 1 / 2) caps the chunks and stays inside the
    same bound."""
    from perceptor_amd import _hip
    d, T, Tk, N, H, _ = case
    S_want = FB.KV_SPLIT_S[(T, Tk)] if opt == 0 else min(opt, FB.KV_SPLIT_S[(T, Tk)])
    assert FB.kv_chunks(N, T, Tk, H, opt)[0] == S_want
    _hip.lib().pmi_set_option(14, opt)
    try:
        _kv(case, dtype, S_want)
    finally:
        _hip.lib().pmi_set_option(14, 0)


@pytest.mark.parametrize("family", ["self", "cross", "kv"])
def test_flash_backward_f16_subnormal_gradients(family):
    """f16 with dO scaled by 2^-14: dS and the outputs are subnormal, the sub term of the bound is what holds them."""
    case = FB.SUBNORMAL_CASES[family]
    d, T, Tk, N, H, _ = case
    assert float(_model(case, "f16", 2.0 ** -14)["dS"].abs().max()) < 2.0 ** -14      # every dS is an f16 subnormal
    if family == "kv":
        _kv(case, "f16", FB.kv_chunks(N, T, Tk, H)[0], 2.0 ** -14)
    else:
        _family("self" if family == "self" else "dq", case, "f16", 2.0 ** -14)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,T,N,H,regime,qt", FB.LSE_CASES)
def test_flash_train_lse_through_each_forward_kernel(d, T, N, H, regime, qt, dtype):
    """pmi_attn_flash_train's lse under pmi_set_option(9, 0 / 1 / 2): the one-wave kernel with one and two query tiles per wave, and the
    LDS kernel the automatic rule takes from 64 query tiles.  Pad rows are 0, live rows inside the bound, two runs the same bits."""
    from perceptor_amd import _hip
    case = (d, T, T, N, H, regime)
    views, _ = _device_operands(case, dtype, 1.0, cross=False)
    _hip.lib().pmi_set_option(9, qt)
    try:
        out, _, lse = _forward(views, N, T, T, H, d, dtype)
        out2, _, lse2 = _forward(views, N, T, T, H, d, dtype)
        torch.cuda.synchronize()
    finally:
        _hip.lib().pmi_set_option(9, 0)
    assert torch.equal(out, out2) and torch.equal(lse, lse2), "two identical launches differ"
    assert bool(torch.isfinite(out).all()) and bool((lse[:, T:] == 0).all())
    q, k, v, _ = _operands(case, dtype)
    r = R.attn_ref(q, k, v, None, d ** -0.5)
    tag = f"flash_train d={d} T={T} {N}x{H} {regime} qt={qt} {dtype}"
    smax = float((q.abs() @ k.abs().transpose(-1, -2)).max()) * d ** -0.5
    FB.check(f"{tag} lse", lse[:, :T].cpu().double() * LN2, r["lse"], 2.0 ** -19 * (1.0 + smax + float(r["lse"].abs().max())))
    R.check(f"{tag} out", _tokens_to_heads(out.cpu(), N, H), r["O"], R.attn_tol(r, "O", dtype))
