"""GPU: the attention kernels one at a time against float64 torch on the same pre-rounded 16-bit operands.

A. pmi_vit_attn_fwd / pmi_vit_attn_bwd (flash, head dim 64, with the input gradient: ViT, ADM and v-diffusion guidance gradients).
B. pmi_attn_flash (head dims 8..160, Tk != T, one-wave and LDS kernels: StableDiffusion self- and cross-attention).
C. the batched-GEMM path for head dims != 64 (attention_train / attention_backward, cross_attention_train / cross_attention_backward,
   causal attention), the softmax kernels,
   the precise-mode softmax and pmi_transpose_16.

Bounds (tests/_ref64.py): max|got - ref| <= 1.5 u S per output, u the unit roundoff of the 16-bit type and S the elementwise worst-case
sum of the roundings the kernel performs -- P rounded to 16 bit before P.V and P^T.dO, dS rounded to 16 bit before dS.K and dS^T.Q, delta
taken from the 16-bit O -- evaluated in float64.  test_*_bounds_reject_defects checks, on the CPU, that the listed plausible defects
exceed these bounds by at least 2x at the tested shapes.  Every output and caller-owned scratch buffer is filled with NaN before a call.
"""
import contextlib

import pytest
import torch

import _ref64 as R

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
REGIMES = ["flat", "peaked", "last", "first"]


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _heads_to_tokens(x, N, H):
    """[N*H, T, d] -> [N, T, H*d]"""
    B, T, d = x.shape
    return x.view(N, H, T, d).permute(0, 2, 1, 3).reshape(N, T, H * d)


def _tokens_to_heads(x, N, H):
    """[N, T, H*d] -> [N*H, T, d]"""
    N_, T, C = x.shape
    return x.reshape(N, T, H, C // H).permute(0, 2, 1, 3).reshape(N * H, T, C // H)


# ============================================ A. ViT flash attention, head dim 64 ============================================
def _vit_attn(qkv, dout, N, T, H, dtype):
    from perceptor_amd._hip import call, dtype_code, ptr
    dev = qkv.device
    td = R.TD[dtype]
    tp32 = (T + 31) // 32 * 32
    scale = 64 ** -0.5
    aws = _nan((6, N * H, tp32, 64), td, dev)          # the buffer shapes engine/vit.py allocates
    lse = _nan((N * H, tp32), torch.float32, dev)
    out = _nan((N, T, H * 64), td, dev)
    call("pmi_vit_attn_fwd", ptr(qkv), ptr(aws), ptr(lse), ptr(out), N, T, H, scale, dtype_code(dtype))
    bws = _nan((2, N * H, tp32, 64), td, dev)
    delta = _nan((N * H, tp32), torch.float32, dev)
    dqkv = _nan((N, T, 3 * H * 64), td, dev)
    call("pmi_vit_attn_bwd", ptr(aws), ptr(lse), ptr(out), ptr(dout), ptr(bws), ptr(delta), ptr(dqkv), N, T, H, scale, dtype_code(dtype))
    torch.cuda.synchronize()
    return out, lse, dqkv


VIT_CASES = [(T, 3, 2, reg) for T in (1, 16, 31, 32, 33, 50, 64, 65, 257, 1024) for reg in REGIMES] + [
    (257, 8, 16, "flat"),      # ViT-L/14: 9 key tiles (odd), one live row in the last; 9 x 128 workgroups
    (257, 1, 16, "last"),
    (50, 1, 1, "peaked"),      # 2 workgroups: fewer than the 8 XCDs
    (64, 1, 1, "first"),
    (2049, 1, 1, "last"),      # 65 key tiles, one live row in the last
    (2049, 1, 1, "peaked"),
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,N,H,regime", VIT_CASES)
def test_vit_attn_fwd_bwd(T, N, H, regime, dtype):
    dev = _dev()
    td = R.TD[dtype]
    q, k, v = R.attn_inputs(N * H, T, 64, regime, dtype, seed=T * 7 + N * H)
    g = torch.Generator().manual_seed(T + 1)
    dO = R.rnd(torch.randn(N * H, T, 64, generator=g, dtype=torch.float64), dtype)
    qkv = torch.cat([_heads_to_tokens(z, N, H) for z in (q, k, v)], -1).to(td).to(dev)
    dout = _heads_to_tokens(dO, N, H).to(td).to(dev)
    out, lse, dqkv = _vit_attn(qkv, dout, N, T, H, dtype)
    out2, lse2, dqkv2 = _vit_attn(qkv, dout, N, T, H, dtype)
    for a, b in ((out, out2), (lse, lse2), (dqkv, dqkv2)):
        assert torch.equal(a, b), "two identical launches differ"
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all() and torch.isfinite(lse).all()
    assert (lse[:, T:] == 0).all(), "lse rows t >= T must be written as 0"

    r = R.attn_ref(q, k, v, dO, 64 ** -0.5)
    tag = f"vit_attn T={T} {N}x{H} {regime} {dtype}"
    R.check(f"{tag} out", _tokens_to_heads(out.cpu(), N, H), r["O"], R.attn_tol(r, "O", dtype))
    dq, dk, dv = (_tokens_to_heads(z, N, H) for z in dqkv.cpu().split(H * 64, -1))
    R.check(f"{tag} dQ", dq, r["dQ"], R.attn_tol(r, "dQ", dtype))
    R.check(f"{tag} dK", dk, r["dK"], R.attn_tol(r, "dK", dtype))
    R.check(f"{tag} dV", dv, r["dV"], R.attn_tol(r, "dV", dtype))
    # lse = logsumexp(scale q k^T): fp32 scores of exact 16-bit products, hardware exp / log: a few fp32 ulps of the score scale
    smax = float((q.abs() @ k.abs().transpose(-1, -2)).max()) * 64 ** -0.5
    R.check(f"{tag} lse", lse[:, :T].cpu(), r["lse"], 2.0 ** -19 * (1.0 + smax + float(r["lse"].abs().max())))

    if N >= 3:   # nothing reduces across (n, head): sample n alone must give the same bits
        n = N - 2
        C3 = 3 * H * 64
        o1, l1, d1 = _vit_attn(qkv[n:n + 1].contiguous(), dout[n:n + 1].contiguous(), 1, T, H, dtype)
        assert torch.equal(o1[0], out[n]) and torch.equal(d1[0], dqkv[n]) and d1.shape[-1] == C3
        assert torch.equal(l1, lse[n * H:(n + 1) * H])


def _margins(T, d, dtype="bf16", Tk=None, cross=False, extra=None):
    """worst-case bound vs each defect's deviation, best over the regimes, at one shape (B = 1)"""
    best = {}
    for reg in REGIMES:
        q, k, v = R.attn_inputs(1, T, d, reg, dtype, seed=3, Tk=Tk)
        if extra:
            q, k = extra(q, k)
        g = torch.Generator().manual_seed(5)
        dO = None if cross else R.rnd(torch.randn(1, T, d, generator=g, dtype=torch.float64), dtype)
        r, defects = R.defect_outputs(q, k, v, dO, d ** -0.5)
        for name, (key, val) in defects.items():
            m = R.max_err(val, r[key]) / R.attn_tol(r, key, dtype)
            if m > best.get(name, (-1.0, ""))[0]:
                best[name] = (m, reg)
    return best


@pytest.mark.parametrize("T", [1, 16, 31, 32, 33, 50, 64, 65, 257, 1024, 2049])
def test_vit_attn_bounds_reject_defects(T):
    """CPU: each listed defect of the ViT attention kernels moves its output by >= 2x the bound (bf16, the looser type) at this T, in at
    least one of the tested score regimes.  A defect that cannot occur at a shape (no padded key when T % 32 == 0, no rescale with one key
    tile, no query gradient with one key) is not listed there."""
    best = _margins(T, 64)
    for name, (m, reg) in best.items():
        if name == "alpha rescale skipped" and T <= 32:
            continue
        if name == "last query row's gradients zeroed" and T == 1:
            continue
        print(f"[sensitivity] vit_attn T={T}: {name}: {m:.1f}x the bound ({reg})")
        assert m >= 2.0, f"T={T}: the bound lets '{name}' through ({m:.2f}x)"


# ============================================ B. pmi_attn_flash ============================================================
def _flash(q, k, v, H, d, dtype):
    """pmi_attn_flash as ops.flash_attention calls it, with NaN-filled workspace and output"""
    from perceptor_amd import _hip
    from perceptor_amd._hip import call, dtype_code, ptr
    N, T = q.shape[:2]
    Tk = k.shape[1]
    kib = _hip.lib().pmi_attn_flash_workspace(N, T, Tk, H, d)
    assert kib > 0
    ws = _nan((kib * 512,), q.dtype, q.device)
    out = _nan((N, T, H * d), q.dtype, q.device)
    call("pmi_attn_flash", q.data_ptr(), q.stride(1), k.data_ptr(), v.data_ptr(), k.stride(1), ptr(out), ptr(ws), N, T, Tk, H, d,
         float(d) ** -0.5, dtype_code(dtype))
    torch.cuda.synchronize()
    return out


def _last_channel_heavy(q, k):
    """channel d-1 of q and k scaled up (its product alone moves a score by ~1): a dropped last channel of a partial k-step shows"""
    q, k = q.clone(), k.clone()
    q[..., -1] = q[..., -1].sign() * 2.0 + q[..., -1]
    k[..., -1] = k[..., -1] * 4.0
    return q, k


FLASH_D = [8, 16, 24, 40, 64, 72, 80, 96, 104, 128, 136, 160]      # (KQ, DB) = (ceil(d/16), ceil(d/32)): all ten instantiations
FLASH_CASES = [(d, 33, 33, 2, 3, "last", qt) for d in FLASH_D for qt in ((0, 1, 2) if d <= 64 else (0, 1))] + \
    [(d, T, T, 2, 2, reg, 0) for d in (40, 80, 160) for T, reg in ((1, "flat"), (257, "peaked"), (257, "first"))] + \
    [(d, 64, 77, 2, 3, "last", 0) for d in (40, 80, 160)] + \
    [(d, 1024, 77, 1, 2, "flat", 0) for d in (40, 160)] + \
    [(64, 2080, 2080, 1, 1, "last", 0), (72, 2080, 2080, 1, 1, "peaked", 0), (40, 4096, 4096, 1, 1, "peaked", 0)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,T,Tk,N,H,regime,qt", FLASH_CASES)
def test_attn_flash(d, T, Tk, N, H, regime, qt, dtype):
    """pmi_attn_flash on q / k / v views with ldq, ldkv > heads*d (a packed qkv tensor for self-attention, a (k | v) tensor for
    cross-attention, as ops.attention / ops.cross_attention pass them).  qt: pmi_set_option(9): 0 automatic (the LDS kernel from 64 query
    tiles), 1 / 2 the one-wave kernel with one / two query tiles per wave."""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    from perceptor_amd._hip import dtype_code
    dev = _dev()
    td = R.TD[dtype]
    q, k, v = R.attn_inputs(N * H, T, d, regime, dtype, seed=d + T, Tk=Tk)
    q, k = _last_channel_heavy(q, k)
    q, k = R.rnd(q, dtype), R.rnd(k, dtype)
    C = H * d
    if Tk == T:
        buf = torch.cat([_heads_to_tokens(z, N, H) for z in (q, k, v)], -1).to(td).to(dev)
        qv, kv_, vv = buf[..., :C], buf[..., C:2 * C], buf[..., 2 * C:]
    else:
        qv = _heads_to_tokens(q, N, H).to(td).to(dev)
        kvb = torch.cat([_heads_to_tokens(z, N, H) for z in (k, v)], -1).to(td).to(dev)
        kv_, vv = kvb[..., :C], kvb[..., C:]
    _hip.lib().pmi_set_option(9, qt)
    try:
        out = _flash(qv, kv_, vv, H, d, dtype)
        out2 = _flash(qv, kv_, vv, H, d, dtype)
        via_ops = ops.attention(buf, H, 1, dtype_code(dtype)) if Tk == T else ops.cross_attention(qv, kvb, H, dtype_code(dtype))
        torch.cuda.synchronize()
    finally:
        _hip.lib().pmi_set_option(9, 0)
    assert torch.equal(out, out2), "two identical launches differ"
    assert torch.isfinite(out).all()
    r = R.attn_ref(q, k, v, None, d ** -0.5)
    if qt == 0 and not (d == 64 and Tk == T):
        assert torch.equal(via_ops, out), "ops wrapper and direct call differ"
    elif qt == 0:   # ops.attention sends head dim 64 to pmi_attn_d64 instead: the same bound
        R.check(f"attn_d64 T={T} {N}x{H} {regime} {dtype} out", _tokens_to_heads(via_ops.cpu(), N, H), r["O"], R.attn_tol(r, "O", dtype))
    R.check(f"attn_flash d={d} T={T} Tk={Tk} {N}x{H} {regime} qt={qt} {dtype} out", _tokens_to_heads(out.cpu(), N, H), r["O"],
            R.attn_tol(r, "O", dtype))
    if N >= 2 and T <= 1024:      # batch independence: sample 1 alone
        n = 1
        o1 = _flash(qv[n:n + 1], kv_[n:n + 1], vv[n:n + 1], H, d, dtype)
        assert torch.equal(o1[0], out[n])


@pytest.mark.parametrize("d", FLASH_D)
def test_attn_flash_bounds_reject_defects(d):
    """CPU: at each head dim, the last key dropped (T = 33), the last channel of a partial k-step dropped (d % 16 != 0) and Tk treated as
    T in cross-attention (T = 64 and 1024 against Tk = 77) each exceed the flash bound by >= 2x in one of the tested regimes."""
    best = _margins(33, d, cross=True, extra=_last_channel_heavy)
    m, reg = best["last key dropped"]
    print(f"[sensitivity] attn_flash d={d}: last key dropped: {m:.1f}x the bound ({reg})")
    assert m >= 2.0
    if d % 16:
        m = 0.0
        for reg in REGIMES:
            q, k, v = R.attn_inputs(1, 33, d, reg, "bf16", seed=3)
            q, k = _last_channel_heavy(q, k)
            r = R.attn_ref(q, k, v, None, d ** -0.5)
            bad = R.attn_ref(q[..., :d - 1], k[..., :d - 1], v, None, d ** -0.5)["O"]
            m = max(m, R.max_err(bad, r["O"]) / R.attn_tol(r, "O", "bf16"))
        print(f"[sensitivity] attn_flash d={d}: last channel of the partial k-step dropped: {m:.1f}x the bound")
        assert m >= 2.0
    for T, reg in ((64, "last"), (1024, "flat")):
        q, k, v = R.attn_inputs(1, T, d, reg, "bf16", seed=3, Tk=77)
        r = R.attn_ref(q, k, v, None, d ** -0.5)
        if T < 77:
            bad = R.attn_ref(q, k[:, :T], v[:, :T], None, d ** -0.5)["O"]
        else:        # keys past Tk read as zero-padded (score 0, value 0)
            kz, vz = torch.zeros(1, T, d, dtype=torch.float64), torch.zeros(1, T, d, dtype=torch.float64)
            kz[:, :77], vz[:, :77] = k, v
            bad = R.attn_ref(q, kz, vz, None, d ** -0.5)["O"]
        m = R.max_err(bad, r["O"]) / R.attn_tol(r, "O", "bf16")
        print(f"[sensitivity] attn_flash d={d} T={T}: Tk treated as T: {m:.1f}x the bound")
        assert m >= 2.0


# ============================================ C. batched-GEMM attention, softmax, transpose ===============================
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [16, 32, 128])
@pytest.mark.parametrize("T", [5, 50, 256])
@pytest.mark.parametrize("N,H", [(1, 1), (2, 3)])
def test_attention_train_backward(d, T, N, H, dtype):
    """ops.attention_train + ops.attention_backward (the split path for head dims != 64) against float64 autograd; the saved P has zero
    pad columns."""
    from perceptor_amd.engine import ops
    from perceptor_amd._hip import dtype_code
    dev = _dev()
    td = R.TD[dtype]
    q, k, v = R.attn_inputs(N * H, T, d, "peaked" if T == 50 else "last", dtype, seed=T + d)
    g = torch.Generator().manual_seed(d)
    dO = R.rnd(torch.randn(N * H, T, d, generator=g, dtype=torch.float64), dtype)
    qkv = torch.cat([_heads_to_tokens(z, N, H) for z in (q, k, v)], -1).to(td).to(dev)
    out, p = ops.attention_train(qkv, H, dtype_code(dtype))
    dqkv = ops.attention_backward(qkv, p, _heads_to_tokens(dO, N, H).to(td).to(dev), H, dtype_code(dtype))
    torch.cuda.synchronize()
    assert (p[..., T:] == 0).all(), "P pad columns must be zero"
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all()
    r = R.attn_ref(q, k, v, dO, d ** -0.5)
    tag = f"attention_train d={d} T={T} {N}x{H} {dtype}"
    R.check(f"{tag} out", _tokens_to_heads(out.cpu(), N, H), r["O"], R.attn_tol(r, "O", dtype))
    R.check(f"{tag} P", p[..., :T].cpu(), r["P"], R.U[dtype] * float(r["P"].max()) * 1.01)
    dq, dk, dv = (_tokens_to_heads(z, N, H) for z in dqkv.cpu().split(H * d, -1))
    R.check(f"{tag} dQ", dq, r["dQ"], R.attn_tol(r, "dQ", dtype))
    R.check(f"{tag} dK", dk, r["dK"], R.attn_tol(r, "dK", dtype))
    R.check(f"{tag} dV", dv, r["dV"], R.attn_tol(r, "dV", dtype))


@contextlib.contextmanager
def _flash_off():
    from perceptor_amd.engine import ops
    old, ops.FLASH_ENABLED = ops.FLASH_ENABLED, False
    try:
        yield
    finally:
        ops.FLASH_ENABLED = old


# T and Tk each below one pad unit of 8; the prompt length (Tk = 77 -> 80); the head dim at which the engines take this route (> 160)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d,T,Tk,N,H", [(16, 5, 7, 2, 3), (40, 33, 77, 2, 3), (168, 50, 77, 1, 2)])
def test_cross_attention_train_backward(d, T, Tk, N, H, dtype):
    """ops.cross_attention_train + ops.cross_attention_backward (the batched-GEMM cross route: keys / values of another length, kv = (k | v))
    against float64 autograd, without q (dQ alone) and with it (dQ, fp32 dK | dV); the saved P is the float64 softmax rounded once (test_attention_train_backward's bound) with zero pad columns; ops.cross_attention
    with flash switched off is the same launches.  attn_tol is derived for 16-bit outputs, so it also bounds the fp32 dkv."""
    from perceptor_amd.engine import ops
    from perceptor_amd._hip import dtype_code
    dev = _dev()
    td, dt = R.TD[dtype], dtype_code(dtype)
    q, k, v = R.attn_inputs(N * H, T, d, "peaked" if T == 33 else "last", dtype, seed=T + d, Tk=Tk)
    g = torch.Generator().manual_seed(d)
    dO = R.rnd(torch.randn(N * H, T, d, generator=g, dtype=torch.float64), dtype)
    qd = _heads_to_tokens(q, N, H).to(td).to(dev)
    kv = torch.cat([_heads_to_tokens(z, N, H) for z in (k, v)], -1).to(td).to(dev)
    dOd = _heads_to_tokens(dO, N, H).to(td).to(dev)
    out, p = ops.cross_attention_train(qd, kv, H, dt)
    dq_only = ops.cross_attention_backward(kv, p, dOd, H, dt)
    dq, dkv = ops.cross_attention_backward(kv, p, dOd, H, dt, q=qd)
    with _flash_off():
        plain = ops.cross_attention(qd, kv, H, dt)
    torch.cuda.synchronize()
    assert tuple(p.shape) == (N * H, T, (Tk + 7) // 8 * 8) and (p[..., Tk:] == 0).all(), "P pad columns must be zero"
    assert torch.isfinite(out).all() and torch.isfinite(dq_only).all() and torch.isfinite(dkv).all()
    assert dkv.dtype == torch.float32 and tuple(dkv.shape) == (N, Tk, 2 * H * d)
    r = R.attn_ref(q, k, v, dO, d ** -0.5)
    tag = f"cross_attention_train d={d} T={T} Tk={Tk} {N}x{H} {dtype}"
    R.check(f"{tag} out", _tokens_to_heads(out.cpu(), N, H), r["O"], R.attn_tol(r, "O", dtype))
    R.check(f"{tag} P", p[..., :Tk].cpu(), r["P"], R.U[dtype] * float(r["P"].max()) * 1.01)
    R.check(f"{tag} dQ", _tokens_to_heads(dq_only.cpu(), N, H), r["dQ"], R.attn_tol(r, "dQ", dtype))
    assert torch.equal(dq, dq_only), "dq with q given differs from the dq-only call"
    dk, dv = (_tokens_to_heads(z, N, H) for z in dkv.cpu().split(H * d, -1))
    R.check(f"{tag} dK", dk, r["dK"], R.attn_tol(r, "dK", dtype))
    R.check(f"{tag} dV", dv, r["dV"], R.attn_tol(r, "dV", dtype))
    assert torch.equal(plain, out), "cross_attention (flash off) and cross_attention_train differ"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [5, 50])
def test_attention_gemm_route_is_attention_train(T, dtype):
    """ops.attention(order=1) at d = 32 with flash switched off is attention_train's launches: the same bits."""
    from perceptor_amd.engine import ops
    from perceptor_amd._hip import dtype_code
    dev = _dev()
    N, H, d = 2, 3, 32
    q, k, v = R.attn_inputs(N * H, T, d, "peaked", dtype, seed=T + d)
    qkv = torch.cat([_heads_to_tokens(z, N, H) for z in (q, k, v)], -1).to(R.TD[dtype]).to(dev)
    out, _ = ops.attention_train(qkv, H, dtype_code(dtype))
    with _flash_off():
        plain = ops.attention(qkv, H, 1, dtype_code(dtype))
    torch.cuda.synchronize()
    assert torch.isfinite(out).all()
    assert torch.equal(plain, out)


@pytest.mark.parametrize("dtype", DTYPES)
def test_causal_attention(dtype):
    """ops.attention(causal=True) at the text tower's shape (T = 77, d = 64) against a masked float64 softmax."""
    from perceptor_amd.engine import ops
    from perceptor_amd._hip import dtype_code
    dev = _dev()
    N, H, T, d = 2, 3, 77, 64
    q, k, v = R.attn_inputs(N * H, T, d, "peaked", dtype, seed=77)
    qkv = torch.cat([_heads_to_tokens(z, N, H) for z in (q, k, v)], -1).to(R.TD[dtype]).to(dev)
    out = ops.attention(qkv, H, 1, dtype_code(dtype), causal=True)
    r = R.attn_ref(q, k, v, None, d ** -0.5, causal=True)
    R.check(f"causal T=77 {dtype} out", _tokens_to_heads(out.cpu(), N, H), r["O"], R.attn_tol(r, "O", dtype))
    # sensitivity: the mask off by one key (query i seeing key i + 1) exceeds the bound
    bad = R.attn_ref(q, k, v, None, d ** -0.5, causal=False)["O"]
    assert R.max_err(bad, r["O"]) >= 2 * R.attn_tol(r, "O", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T,ld,mag", [(1, 8, 1.0), (77, 96, 1.0), (77, 80, 80.0), (200, 232, 80.0), (300, 300, 3.0)])
def test_softmax_kernels(T, ld, mag, dtype):
    """pmi_softmax_fwd / _causal_fwd / _bwd directly: ld_out > T with NaN in the pad columns beforehand (written zero), T = 1, and
    scores of magnitude ~80 after scaling, where only the max subtraction keeps exp finite.  Bounds: P is the fp32 softmax rounded once
    (u P + fp32 noise); dS = scale P16 (dP - sum dP P16) rounded once, with P16 the rounded P: u |dS| + u scale P (|dP - delta| + P|dP|)."""
    from perceptor_amd._hip import call, dtype_code, ptr
    dev = _dev()
    td = R.TD[dtype]
    rows, scale = 12 * T if T > 1 else 37, 0.125
    g = torch.Generator().manual_seed(T)
    s = torch.randn(rows, ld, generator=g) * (mag / scale)
    s[:, T:] = float("nan")                                 # columns >= T are never read
    dp = torch.randn(rows, ld, generator=g)
    dp[:, T:] = float("nan")
    sd, dpd = s.to(dev), dp.to(dev)
    for causal in (False, True):
        p = _nan((rows, ld), td, dev)
        call("pmi_softmax_causal_fwd" if causal else "pmi_softmax_fwd", ptr(sd), ptr(p), rows, T, ld, ld, scale, dtype_code(dtype))
        torch.cuda.synchronize()
        assert torch.isfinite(p).all() and (p[:, T:] == 0).all()
        s64 = s[:, :T].double() * scale
        if causal:
            s64 = s64.masked_fill(torch.arange(T)[None, :] > (torch.arange(rows) % T)[:, None], float("-inf"))
        pr = torch.softmax(s64, -1)
        R.check(f"softmax{'_causal' if causal else ''} T={T} ld={ld} mag={mag} {dtype}", p[:, :T].cpu(), pr,
                (1.01 * R.U[dtype] + 2.0 ** -20) * float(pr.max()))
    # backward from the (non-causal) probabilities the kernel wrote
    p = _nan((rows, ld), td, dev)
    call("pmi_softmax_fwd", ptr(sd), ptr(p), rows, T, ld, ld, scale, dtype_code(dtype))
    ds = _nan((rows, ld), td, dev)
    call("pmi_softmax_bwd", ptr(dpd), ptr(p), ptr(ds), rows, T, ld, ld, scale, dtype_code(dtype))
    torch.cuda.synchronize()
    assert torch.isfinite(ds).all() and (ds[:, T:] == 0).all()
    s64 = (s[:, :T].double() * scale).requires_grad_(True)
    with torch.enable_grad():
        pr = torch.softmax(s64, -1)
        (dsr,) = torch.autograd.grad(pr, s64, dp[:, :T].double())
    dsr = dsr * scale
    P, dP = pr.detach(), dp[:, :T].double()
    delta = (P * dP).sum(-1, keepdim=True)
    e = dsr.abs() + scale * P * ((dP - delta).abs() + (P * dP.abs()).sum(-1, keepdim=True))
    R.check(f"softmax_bwd T={T} ld={ld} mag={mag} {dtype}", ds[:, :T].cpu(), dsr, 2 * R.U[dtype] * float(e.max()))


def test_softmax_f32_and_attention_precise():
    """pmi_softmax_f32 (in place) and ops.attention_precise (the precise mode that carries the 1e-3 contract) at fp32-level bounds."""
    from perceptor_amd.engine import ops
    from perceptor_amd._hip import call, ptr
    dev = _dev()
    g = torch.Generator().manual_seed(9)
    for rows, T, ld, mag in ((40, 77, 80, 80.0), (9, 1, 4, 1.0), (300, 256, 256, 3.0)):
        s = torch.randn(rows, ld, generator=g) * mag * 8
        sd = s.to(dev)
        call("pmi_softmax_f32", ptr(sd), rows, T, ld, 0.125)
        torch.cuda.synchronize()
        ref = torch.softmax(s[:, :T].double() * 0.125, -1)
        R.check(f"softmax_f32 T={T} mag={mag}", sd[:, :T].cpu(), ref, 2.0 ** -19 * float(ref.max()) * (1 + mag))
    N, T, H, d = 2, 50, 2, 64
    q, k, v = (torch.randn(N * H, T, d, generator=g, dtype=torch.float64) * 0.6 for _ in range(3))
    qkv32 = torch.cat([_heads_to_tokens(z, N, H) for z in (q, k, v)], -1).float()
    hi = qkv32.half()
    lo = (qkv32 - hi.float()).half()
    c3 = qkv32.shape[-1]
    from perceptor_amd.engine.ops import split_group
    gs = split_group(c3)
    pr = torch.stack([hi.view(N, T, c3 // gs, gs), lo.view(N, T, c3 // gs, gs)], 3).reshape(N, T, 2 * c3)
    out = ops.attention_precise(pr.to(dev), H, 1).cpu()
    c = c3 // 3
    gs2 = split_group(c)
    o = out.view(N, T, c // gs2, 2, gs2)
    got = o[:, :, :, 0].float() + o[:, :, :, 1].float()
    got = got.reshape(N, T, c)
    qd, kd, vd = (_tokens_to_heads(z.double(), N, H) for z in (hi.float() + lo.float()).split(c, -1))
    r = R.attn_ref(qd, kd, vd, None, d ** -0.5)
    R.check("attention_precise out", _tokens_to_heads(got, N, H), r["O"], 2.0 ** -18 * r["sO"] + 2.0 ** -22)


def test_transpose_16():
    """pmi_transpose_16: R not a multiple of 8 (pad rows of the output zero over NaN), both batch strides, row pitch > Cc."""
    from perceptor_amd._hip import call, ptr
    dev = _dev()
    for Rr, Cc, ld, inner, batch in ((13, 40, 48, 3, 6), (77, 64, 200, 1, 2), (1, 8, 8, 2, 4), (257, 72, 216, 4, 8)):
        so, si = Rr * ld * inner, Rr * ld        # batch b -> (b // inner) * so + (b % inner) * si
        src = torch.randn(batch * Rr * ld + 64, generator=torch.Generator().manual_seed(Rr)).to(torch.bfloat16)
        rp = (Rr + 7) // 8 * 8
        srcd = src.to(dev)
        out = _nan((batch, Cc, rp), torch.bfloat16, dev)
        call("pmi_transpose_16", ptr(srcd), ptr(out), Rr, Cc, ld, so, si, inner, batch)
        torch.cuda.synchronize()
        for b in range(batch):
            off = (b // inner) * so + (b % inner) * si
            m = src[off:off + Rr * ld].view(Rr, ld)[:, :Cc]
            assert torch.equal(out[b, :, :Rr].cpu(), m.t()), (Rr, Cc, b)
        assert (out[..., Rr:] == 0).all()
