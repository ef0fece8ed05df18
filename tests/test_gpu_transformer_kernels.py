"""GPU: the transformer-block kernels one at a time against float64 torch on the same (pre-rounded) operands.

D. LayerNorm forward / input gradient (plain and fused with the split-K slab reduction), and the slab route through ops.igemm.
E. pmi_act_fwd / pmi_act_bwd and the weights-direct GEMM's fused MLP epilogues (pre_out, act_grad_of).
F. pmi_spherical_loss and pmi_l2norm_rows (the CLIP loss and its gradient).

fp32 kernels are bounded by a few fp32 roundings of the magnitudes they combine (E32 = 2^-24); 16-bit outputs add one rounding,
u |y| (u = 2^-11 for f16, 2^-8 for bf16).  Output buffers are NaN-filled before each call.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _ref64 as R

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
E32 = 2.0 ** -24


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _rowcheck(tag, got, ref, tol_rows):
    """per-row bound: max_c |got - ref| <= tol_rows[r]"""
    err = (got.double().cpu() - ref.double()).abs().amax(-1)
    i = int((err / tol_rows).argmax())
    ratio = float(err[i] / tol_rows[i])
    R.parity(tag, float(err[i]), float(tol_rows[i]))                # the row closest to its bound
    assert ratio <= 1.0, f"{tag}: error {ratio:.2f}x the bound"


def _ln_inputs(M, D, g, rows_ld=None):
    x = torch.randn(M, D, generator=g) * 2 + 0.5
    x[0] = 0.1                                                     # constant row: variance 0, y = beta
    if M > 1:
        x[1] = 300.0 + 0.05 * torch.randn(D, generator=g)          # large common offset: a one-pass variance would cancel away
    gamma = 1 + 0.2 * torch.randn(D, generator=g)
    beta = 0.1 * torch.randn(D, generator=g)
    return x, gamma, beta


def _ln_fwd_bounds(x, gamma, beta, eps=1e-5):
    x64 = x.double()
    mean = x64.mean(-1)
    rstd = 1 / torch.sqrt(x64.var(-1, unbiased=False) + eps)
    y = F.layer_norm(x64, (x.shape[-1],), gamma.double(), beta.double(), eps)
    # mean: E32 log2(D) |x|; x - mean then carries that error times rstd |gamma|
    t32 = 16 * E32 * (x64.abs().amax(-1) * rstd * gamma.abs().max() + beta.abs().max() + y.abs().amax(-1))
    return y, mean, rstd, t32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [64, 320, 768, 1024, 1280, 2304])
@pytest.mark.parametrize("M", [1, 3, 257, 2057])
def test_layernorm_fwd(M, D, dtype):
    """pmi_layernorm_fwd: y16 only, y32 only and both; ld_x = D and ld_x = 3 D (ln_post reads the class-token rows of [N, T, D])."""
    from perceptor_amd._hip import call, dtype_code, ptr
    dev = _dev()
    td = R.TD[dtype]
    g = torch.Generator().manual_seed(M * 31 + D)
    x, gamma, beta = _ln_inputs(M, D, g)
    y, mean, rstd, t32 = _ln_fwd_bounds(x, gamma, beta)
    gd, bd = gamma.to(dev), beta.to(dev)
    for ld in (D, 3 * D):
        xs = torch.randn(M, ld // D, D, generator=g)
        xs[:, 0] = x
        xd = xs.to(dev)
        for w16, w32 in ((True, False), (False, True), (True, True)):
            y16 = _nan((M, D), td, dev) if w16 else None
            y32 = _nan((M, D), torch.float32, dev) if w32 else None
            mr = _nan((2, M), torch.float32, dev)
            call("pmi_layernorm_fwd", ptr(xd), ld, ptr(gd), ptr(bd), ptr(y16), ptr(y32), ptr(mr), M, D, 1e-5, dtype_code(dtype))
            torch.cuda.synchronize()
            tag = f"layernorm_fwd M={M} D={D} ld={ld} {dtype}"
            assert torch.isfinite(mr).all()
            if w32:
                assert torch.isfinite(y32).all()
                _rowcheck(f"{tag} y32", y32, y, t32)
            if w16:
                assert torch.isfinite(y16).all()
                _rowcheck(f"{tag} y16", y16, y, t32 + R.U[dtype] * y.abs().amax(-1))
            _rowcheck(f"{tag} mean", mr[0][:, None], mean[:, None], 16 * E32 * x.double().abs().amax(-1))
            _rowcheck(f"{tag} rstd", mr[1][:, None], rstd[:, None], 64 * E32 * rstd)


def _ln_bwd_ref(x, gamma, dy, gres, eps=1e-5):
    x64 = x.double().requires_grad_(True)
    with torch.enable_grad():
        y = F.layer_norm(x64, (x.shape[-1],), gamma.double(), None, eps)
        (dx,) = torch.autograd.grad(y, x64, dy.double())
    mean = x.double().mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(x.double().var(-1, unbiased=False, keepdim=True) + eps)
    gy = dy.double() * gamma.double()
    xh = (x.double() - mean) * rstd
    s1 = gy.mean(-1, keepdim=True).abs()
    s2 = (gy * xh).mean(-1, keepdim=True).abs()
    # fp32 terms of rstd (gy - s1 - xh s2), plus the mean / rstd the forward kernel passed (each a few E32 off, scaled by rstd |s2|)
    t32 = (64 * E32 * rstd * (gy.abs().amax(-1, keepdim=True) + s1 + xh.abs().amax(-1, keepdim=True) * s2)
           + 64 * E32 * rstd * s2 * (1 + x.double().abs().amax(-1, keepdim=True) * rstd)).squeeze(-1)
    if gres is not None:
        dx = dx + gres.double()
        t32 = t32 + 2 * E32 * dx.abs().amax(-1)
    return dx, t32


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D,dy_ld,row_stride,M", [(768, 768, 1, 257), (1024, 1024, 1, 2057), (1024, 1028, 3, 5), (2048, 2048, 1, 3),
                                                  (320, 320, 1, 257), (2304, 2304, 1, 33), (1024, 1025, 1, 7), (320, 333, 4, 9)])
def test_layernorm_bwd(D, dy_ld, row_stride, M, dtype):
    """pmi_layernorm_bwd on the one-pass path (D % 256 == 0, D <= 2048, dy_ld % 4 == 0) and the generic one (D = 320, 2304, odd dy_ld),
    rows of x / gres / outputs at row_stride (rows in between keep their sentinel), gres present or absent, g32 or g16 alone."""
    from perceptor_amd._hip import call, dtype_code, ptr
    dev = _dev()
    td = R.TD[dtype]
    g = torch.Generator().manual_seed(D + M)
    xa, gamma, _ = _ln_inputs(M * row_stride, D, g)
    beta = torch.zeros(D)
    xr = xa[::row_stride]
    dyb = torch.randn(M, dy_ld, generator=g)
    dy = dyb[:, :D]
    gres_a = torch.randn(M * row_stride, D, generator=g)
    xd, gd, bd, dyd, gresd = xa.to(dev), gamma.to(dev), beta.to(dev), dyb.to(dev), gres_a.to(dev)
    # mean / rstd of the rows dy refers to, from the forward kernel (as the engine passes them)
    mr = _nan((2, M), torch.float32, dev)
    y32 = _nan((M, D), torch.float32, dev)
    call("pmi_layernorm_fwd", ptr(xd), row_stride * D, ptr(gd), ptr(bd), None, ptr(y32), ptr(mr), M, D, 1e-5, dtype_code(dtype))
    for with_gres in (False, True):
        ref, t32 = _ln_bwd_ref(xr, gamma, dy, gres_a[::row_stride] if with_gres else None)
        for w32, w16 in ((True, True), (True, False), (False, True)):
            g32 = torch.full((M * row_stride, D), 7.0, device=dev) if w32 else None
            g16 = torch.full((M * row_stride, D), 7.0, dtype=td, device=dev) if w16 else None
            call("pmi_layernorm_bwd", ptr(dyd), ptr(xd), ptr(gd), ptr(mr), ptr(gresd) if with_gres else None, ptr(g32), ptr(g16),
                 M, D, dy_ld, row_stride, dtype_code(dtype))
            torch.cuda.synchronize()
            tag = f"layernorm_bwd D={D} dy_ld={dy_ld} stride={row_stride} gres={int(with_gres)} {dtype}"
            for out, is16 in ((g32, False), (g16, True)):
                if out is None:
                    continue
                o = out.cpu()
                keep = torch.ones(M * row_stride, dtype=torch.bool)
                keep[::row_stride] = False
                assert (o[keep] == 7.0).all(), "rows between the strided rows must keep their contents"
                _rowcheck(f"{tag} {'g16' if is16 else 'g32'}", o[::row_stride], ref,
                          t32 + (R.U[dtype] * ref.abs().amax(-1) if is16 else 0))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nslab", [1, 2, 3, 4, 5, 8])
@pytest.mark.parametrize("D", [256, 1024, 2048])
def test_layernorm_slabs(nslab, D, dtype):
    """pmi_layernorm_fwd_slabs / _bwd_slabs: x_out must equal, bitwise, the fp32 sum of the slabs in slab order followed by the bias and
    then the residual (the determinism the kernel's comment claims); the LayerNorm outputs against float64."""
    from perceptor_amd._hip import call, dtype_code, ptr
    dev = _dev()
    td = R.TD[dtype]
    M = 259
    g = torch.Generator().manual_seed(nslab * 7 + D)
    ws = torch.randn(nslab, M, D, generator=g) * torch.tensor([10.0 ** (i % 3) for i in range(nslab)])[:, None, None]
    ws[:, 1] += 100.0 / nslab                              # a row with a large common offset
    bias = torch.randn(D, generator=g)
    res = torch.randn(M, D, generator=g) * 4
    gamma, beta = 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)
    wsd, gd, bd = ws.to(dev), gamma.to(dev), beta.to(dev)
    for with_bias in (False, True):
        for with_res in (False, True):
            want = ws[0].clone()
            for z in range(1, nslab):
                want = want + ws[z]
            if with_bias:
                want = want + bias
            if with_res:
                want = want + res
            xo = _nan((M, D), torch.float32, dev)
            y16 = _nan((M, D), td, dev)
            mr = _nan((2, M), torch.float32, dev)
            biasd, resd = bias.to(dev), res.to(dev)
            call("pmi_layernorm_fwd_slabs", ptr(wsd), nslab, M * D, ptr(biasd) if with_bias else None, ptr(resd) if with_res else None,
                 ptr(xo), ptr(gd), ptr(bd), ptr(y16), ptr(mr), M, D, 1e-5, dtype_code(dtype))
            torch.cuda.synchronize()
            assert torch.equal(xo.cpu(), want), "x_out is not the slab-order fp32 sum + bias + residual"
            y, mean, rstd, t32 = _ln_fwd_bounds(want, gamma, beta)
            tag = f"layernorm_fwd_slabs nslab={nslab} D={D} bias={int(with_bias)} res={int(with_res)} {dtype}"
            _rowcheck(f"{tag} y16", y16, y, t32 + R.U[dtype] * y.abs().amax(-1))
            _rowcheck(f"{tag} rstd", mr[1][:, None], rstd[:, None], 64 * E32 * rstd)
    # backward: dy = the slab-order sum of the slabs
    x = res
    xd = x.to(dev)
    mr = _nan((2, M), torch.float32, dev)
    call("pmi_layernorm_fwd", ptr(xd), D, ptr(gd), ptr(bd), None, ptr(_nan((M, D), torch.float32, dev)), ptr(mr), M, D, 1e-5, dtype_code(dtype))
    dy = ws[0].clone()
    for z in range(1, nslab):
        dy = dy + ws[z]
    gres = torch.randn(M, D, generator=g)
    gresd = gres.to(dev)
    for with_gres in (False, True):
        g32 = _nan((M, D), torch.float32, dev)
        g16 = _nan((M, D), td, dev)
        call("pmi_layernorm_bwd_slabs", ptr(wsd), nslab, M * D, ptr(xd), ptr(gd), ptr(mr), ptr(gresd) if with_gres else None, ptr(g32),
             ptr(g16), M, D, dtype_code(dtype))
        torch.cuda.synchronize()
        ref, t32 = _ln_bwd_ref(x, gamma, dy, gres if with_gres else None)
        tag = f"layernorm_bwd_slabs nslab={nslab} D={D} gres={int(with_gres)} {dtype}"
        _rowcheck(f"{tag} g32", g32, ref, t32)
        _rowcheck(f"{tag} g16", g16, ref, t32 + R.U[dtype] * ref.abs().amax(-1))


def _ulp_close(a, b, dtype):
    """|a - b| <= 1 ulp of the 16-bit type (2u of the larger magnitude, or the smallest normal spacing near 0)"""
    a, b = a.double().cpu(), b.double().cpu()
    tiny = 2.0 ** -24 if dtype == "f16" else 2.0 ** -133
    return bool(((a - b).abs() <= 2 * R.U[dtype] * torch.maximum(a.abs(), b.abs()) + tiny).all()), float((a - b).abs().max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("m", [2056, 257])
def test_igemm_defer_reduce_matches_reduced_route(m, dtype):
    """ops.igemm(..., defer_reduce=True) + pmi_layernorm_*_slabs against the non-deferred igemm + pmi_layernorm_fwd / _bwd at the ViT-L/14
    MLP output shape (K = 4096 -> N = 1024): x within fp32 reordering, y16 / g16 within 1 ulp."""
    from perceptor_amd.engine import ops
    from perceptor_amd._hip import call, dtype_code, ptr
    dev = _dev()
    td = R.TD[dtype]
    dt = dtype_code(dtype)
    K, N = 4096, 1024
    g = torch.Generator().manual_seed(m)
    a = R.rnd(torch.randn(m, K, generator=g), dtype).to(td).to(dev)
    w = R.rnd(torch.randn(N, K, generator=g) / K ** 0.5, dtype).float()
    b = torch.randn(N, generator=g) * 0.1
    lin = ops.PackedLinear(w, b, dt, dev)
    lin_nb = ops.PackedLinear(w, None, dt, dev)
    res = (torch.randn(m, N, generator=g) * 3).to(dev)
    gamma, beta = (1 + 0.2 * torch.randn(N, generator=g)).to(dev), (0.1 * torch.randn(N, generator=g)).to(dev)
    x_ref = ops.igemm(a, lin, residual=res, out_f32=True)
    y_ref = _nan((m, N), td, dev)
    mr_ref = _nan((2, m), torch.float32, dev)
    call("pmi_layernorm_fwd", ptr(x_ref), N, ptr(gamma), ptr(beta), ptr(y_ref), None, ptr(mr_ref), m, N, 1e-5, dt)
    sl = ops.igemm(a, lin, residual=res, out_f32=True, defer_reduce=True)
    dy_ref = ops.igemm(a, lin_nb, out_f32=True)
    gres = torch.randn(m, N, device=dev)
    g32_ref, g16_ref = _nan((m, N), torch.float32, dev), _nan((m, N), td, dev)
    call("pmi_layernorm_bwd", ptr(dy_ref), ptr(x_ref), ptr(gamma), ptr(mr_ref), ptr(gres), ptr(g32_ref), ptr(g16_ref), m, N, N, 1, dt)
    sl_b = ops.igemm(a, lin_nb, out_f32=True, defer_reduce=True)
    torch.cuda.synchronize()
    if not isinstance(sl, tuple):        # no split-K at this shape: nothing is deferred, the call is the plain route
        assert torch.equal(sl, x_ref) and not isinstance(sl_b, tuple)
        print(f"[parity] defer_reduce m={m}: not split, plain route")
        return
    _, ws, sk = sl
    xo, y16, mr = _nan((m, N), torch.float32, dev), _nan((m, N), td, dev), _nan((2, m), torch.float32, dev)
    call("pmi_layernorm_fwd_slabs", ptr(ws), sk, m * N, ptr(lin.b), ptr(res), ptr(xo), ptr(gamma), ptr(beta), ptr(y16), ptr(mr), m, N, 1e-5, dt)
    _, wsb, skb = sl_b
    g32, g16 = _nan((m, N), torch.float32, dev), _nan((m, N), td, dev)
    call("pmi_layernorm_bwd_slabs", ptr(wsb), skb, m * N, ptr(x_ref), ptr(gamma), ptr(mr_ref), ptr(gres), ptr(g32), ptr(g16), m, N, dt)
    torch.cuda.synchronize()
    # fp32 reordering: the K products summed in a different grouping, plus bias and residual: a few E32 of sum |a||w| + |b| + |res|
    mag = (a.float().abs().cpu() @ w.abs().t()) + b.abs() + res.abs().cpu()
    R.check(f"defer_reduce m={m} sk={sk} {dtype} x", xo.cpu(), x_ref.cpu(), float(64 * E32 * mag.max()))
    ok, e = _ulp_close(y16, y_ref, dtype)
    R.parity(f"defer_reduce m={m} {dtype} y16 (1 ulp)", e, 2 * R.U[dtype] * float(y_ref.float().abs().max()))
    assert ok, "y16 of the slab route differs by more than 1 ulp"
    magb = a.float().abs().cpu() @ w.abs().t()
    R.check(f"defer_reduce m={m} {dtype} dy->g32", g32.cpu(), g32_ref.cpu(),
            float(64 * E32 * (magb.max() * mr_ref[1].max().cpu() * gamma.abs().max().cpu() * 4 + gres.abs().max().cpu())))
    ok, e = _ulp_close(g16, g16_ref, dtype)
    R.parity(f"defer_reduce m={m} {dtype} g16 (1 ulp)", e, 2 * R.U[dtype] * float(g16_ref.float().abs().max()))
    assert ok, "g16 of the slab route differs by more than 1 ulp"


# ============================================ E. activations and fused MLP epilogues ========================================
ACTS = {"relu": 1, "silu": 2, "gelu": 3, "quickgelu": 4}


def _act_grid(dtype):
    x = torch.linspace(-12, 12, 8 * 1001 - 7, dtype=torch.float64)
    x = torch.cat([x, torch.tensor([0.0, 1e-3, -1e-3, 1e4, -1e4, 0.5, -0.5], dtype=torch.float64)])   # 8 x 1001 elements (an odd count)
    return R.rnd(x, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", list(ACTS))
def test_act_fwd_bwd(act, dtype):
    """pmi_act_fwd / pmi_act_bwd per element over [-12, 12] plus 0, +-1e-3, +-1e4.  Bound: 2u |ref| for the 16-bit output and the fp32
    exp / rcp, plus an absolute floor: fast_erff (A&S 7.1.26) is off by up to 1.5e-7 (absolute), which GELU multiplies by |x| / 2 and its
    derivative by 1/2; 2^-21 |x| (fwd) and 2^-21 (1 + |x|) |dh| (bwd) cover it with the fp32 arithmetic; f16 adds its subnormal spacing."""
    from perceptor_amd._hip import call, dtype_code, ptr
    dev = _dev()
    td = R.TD[dtype]
    a = ACTS[act]
    x = _act_grid(dtype)
    n = x.numel()
    assert n % 8 == 0 and (n // 8) % 2 == 1
    dh = R.rnd(torch.randn(n, generator=torch.Generator().manual_seed(a), dtype=torch.float64), dtype)
    xd, dhd = x.to(td).to(dev), dh.to(td).to(dev)
    y = _nan((n,), td, dev)
    call("pmi_act_fwd", ptr(xd), ptr(y), n, a, dtype_code(dtype))
    gx = _nan((n,), td, dev)
    call("pmi_act_bwd", ptr(dhd), ptr(xd), ptr(gx), n, a, dtype_code(dtype))
    torch.cuda.synchronize()
    sub = 2.0 ** -25 if dtype == "f16" else 0.0
    ref = R.act_ref(x, a)
    tol = 2 * R.U[dtype] * ref.abs() + 2.0 ** -21 * x.abs() + sub
    err = (y.double().cpu() - ref).abs()
    R.parity(f"act_fwd {act} {dtype}", float(err[int((err / tol).argmax())]), float(tol[int((err / tol).argmax())]))
    assert (err <= tol).all(), f"worst at x = {float(x[int((err / tol).argmax())])}"
    refb = dh * R.act_grad_ref(x, a)
    tolb = 2 * R.U[dtype] * refb.abs() + 2.0 ** -21 * (1 + x.abs()) * dh.abs() + sub
    errb = (gx.double().cpu() - refb).abs()
    R.parity(f"act_bwd {act} {dtype}", float(errb[int((errb / tolb).argmax())]), float(tolb[int((errb / tolb).argmax())]))
    assert (errb <= tolb).all(), f"worst at x = {float(x[int((errb / tolb).argmax())])}"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("act", ["gelu", "quickgelu"])
@pytest.mark.parametrize("K,N", [(1024, 4096), (768, 3072)])
@pytest.mark.parametrize("m", [64, 257, 2056])
def test_fused_mlp_epilogues(m, K, N, act, dtype):
    """The weights-direct GEMM's MLP epilogues at the ViT shapes.  Forward: act + pre_out against float64, and pre_out bitwise against a
    plain igemm (the same kernel and accumulation, act off).  Backward: act_grad_of / act_grad against float64 dh act'(h), and against the
    unfused igemm + pmi_act_bwd route, which rounds once more (the GEMM output to 16 bit before the multiply): within u |a| |act'| + u |ref|."""
    from perceptor_amd.engine import ops
    from perceptor_amd._hip import call, dtype_code, ptr
    dev = _dev()
    td = R.TD[dtype]
    dt = dtype_code(dtype)
    a_code = ACTS[act]
    g = torch.Generator().manual_seed(m + K)
    x = R.rnd(torch.randn(m, K, generator=g), dtype)
    w = R.rnd(torch.randn(N, K, generator=g) / K ** 0.5 * 1.5, dtype)
    b = (torch.randn(N, generator=g) * 0.1).double()
    lin = ops.PackedLinear(w.float(), b.float(), dt, dev)
    assert ops.fused_mlp_epilogues(lin, m), "the ViT MLP shape must take the fused epilogue route"
    xd = x.to(td).to(dev)
    hpre = _nan((m, N), td, dev)
    hact = ops.igemm(xd, lin, act=a_code, pre_out=hpre)
    plain = ops.igemm(xd, lin)
    torch.cuda.synchronize()
    pre = x @ w.t() + b.float().double()
    mag = x.abs() @ w.abs().t() + b.abs()
    tag = f"mlp_epilogue m={m} K={K} N={N} {act} {dtype}"
    R.check(f"{tag} pre_out", hpre.cpu(), pre, float((R.U[dtype] * pre.abs() + 16 * E32 * mag).max()))
    ref_act = R.act_ref(pre, a_code)
    err = (hact.double().cpu() - ref_act).abs()
    tol = 1.01 * R.U[dtype] * ref_act.abs() + 16 * E32 * mag * 1.2 + 2.0 ** -21 * pre.abs() + (2.0 ** -25 if dtype == "f16" else 0)
    R.parity(f"{tag} act", float(err.flatten()[(err / tol).argmax()]), float(tol.flatten()[(err / tol).argmax()]))
    assert (err <= tol).all()
    assert torch.equal(hpre, plain), "pre_out differs from the plain GEMM of the same operands"
    # backward: dh = (gy @ W2^T) * act'(hpre), W2: [N out, K in] of the weights-direct input-gradient GEMM
    gy = R.rnd(torch.randn(m, K, generator=g), dtype)
    w2 = R.rnd(torch.randn(N, K, generator=g) / K ** 0.5, dtype)
    lin2 = ops.PackedLinear(w2.float(), None, dt, dev)
    assert ops.fused_mlp_epilogues(lin2, m)
    gyd = gy.to(td).to(dev)
    dh = ops.igemm(gyd, lin2, act_grad_of=hpre, act_grad=a_code)
    dh_u = ops.igemm(gyd, lin2)
    call("pmi_act_bwd", ptr(dh_u), ptr(hpre), ptr(dh_u), dh_u.numel(), a_code, dt)
    torch.cuda.synchronize()
    aa = gy @ w2.t()
    h16 = hpre.double().cpu()
    dact = R.act_grad_ref(h16, a_code)
    ref = aa * dact
    mag2 = (gy.abs() @ w2.abs().t()) * dact.abs()
    # the epilogue stages the GEMM value as 16 bit before the multiply (csrc/gemm_wd.hip), as the unfused route does: two roundings
    tol = 1.01 * R.U[dtype] * (aa.abs() * dact.abs() + ref.abs()) + 16 * E32 * mag2 + 2.0 ** -21 * (1 + h16.abs()) * aa.abs() \
        + (2.0 ** -25 if dtype == "f16" else 0)
    err = (dh.double().cpu() - ref).abs()
    R.parity(f"{tag} act_grad", float(err.flatten()[(err / tol).argmax()]), float(tol.flatten()[(err / tol).argmax()]))
    assert (err <= tol).all()
    # the same arithmetic in the same order: equal up to the GEMM's accumulation, which pre_out showed to be the same -> 1 ulp at most
    ok, e = _ulp_close(dh, dh_u, dtype)
    R.parity(f"{tag} act_grad vs unfused (1 ulp; bitwise {bool(torch.equal(dh, dh_u))})", e, 2 * R.U[dtype] * float(dh_u.float().abs().max()))
    assert ok


# ============================================ F. CLIP spherical loss ========================================================
def _sph_ref(emb, tgt, wts, mult, gscale, n_total):
    from oracle.clip_vit import spherical_loss
    e = emb.double().clone().requires_grad_(True)
    with torch.enable_grad():
        # the oracle averages over its own batch: rescale to a shard's share of the n_total-sample mean
        loss = spherical_loss(F.normalize(e, dim=1), tgt.double(), wts.double(), mult) * (emb.shape[0] / n_total)
        (de,) = torch.autograd.grad(loss, e)
    return loss.detach(), de * gscale


def _sph_call(emb, tgt, wts, n_total, mult, gscale):
    from perceptor_amd._hip import call, ptr
    dev = emb.device
    loss = _nan((1,), torch.float32, dev)
    demb = _nan(emb.shape, torch.float32, dev)
    N, D = emb.shape
    call("pmi_spherical_loss", ptr(emb), ptr(tgt), ptr(wts), ptr(loss), ptr(demb), N, tgt.shape[0], D, n_total, mult, gscale)
    torch.cuda.synchronize()
    return loss.cpu(), demb.cpu()


@pytest.mark.parametrize("D", [512, 768, 1024])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("N", [1, 4])
def test_spherical_loss(N, K, D):
    """pmi_spherical_loss against float64 autograd of oracle.clip_vit.spherical_loss . F.normalize; weights negative / zero; a shard
    (n_total > N) reproduces its slice of the full-batch gradient bitwise and the shard losses sum to the full loss."""
    from perceptor_amd._hip import call, ptr
    dev = _dev()
    g = torch.Generator().manual_seed(N * 100 + K * 10 + D)
    emb = torch.randn(N, D, generator=g) * 3
    tgt = F.normalize(torch.randn(K, D, generator=g), dim=1)
    wts = torch.tensor([1.0, -0.5, 0.0][:K])
    mult, gscale = 1.7, 65536.0
    embd, tgtd, wtsd = emb.to(dev), tgt.to(dev), wts.to(dev)
    loss, demb = _sph_call(embd, tgtd, wtsd, N, mult, gscale)
    assert torch.isfinite(demb).all()
    lref, dref = _sph_ref(emb, tgt, wts, mult, gscale, N)
    # per (n, k): |e - t| from D fp32 products (~E32 sqrt(D) relative), asin / sqrt in fp32; gradient the same chain times gscale / |emb|
    R.check(f"spherical_loss N={N} K={K} D={D} loss", loss, lref.reshape(1), 64 * E32 * (abs(float(lref)) + mult * float(wts.abs().sum())))
    R.check(f"spherical_loss N={N} K={K} D={D} demb", demb, dref, 256 * E32 * float(dref.abs().max()) + 2.0 ** -30 * gscale)
    # shards of a batch of 2N: each shard's demb is its slice of the full-batch demb, bitwise; the losses sum to the full loss
    emb2 = torch.cat([emb, torch.randn(N, D, generator=g)], 0)
    emb2d = emb2.to(dev)
    lf, df = _sph_call(emb2d, tgtd, wtsd, 2 * N, mult, gscale)
    l0, d0 = _sph_call(emb2d[:N].contiguous(), tgtd, wtsd, 2 * N, mult, gscale)
    l1, d1 = _sph_call(emb2d[N:].contiguous(), tgtd, wtsd, 2 * N, mult, gscale)
    assert torch.equal(d0, df[:N]) and torch.equal(d1, df[N:])
    R.check(f"spherical_loss N={N} K={K} D={D} shard loss sum", l0 + l1, lf, 4 * E32 * (abs(float(lf)) + mult * float(wts.abs().sum())))
    # pmi_l2norm_rows = scale * F.normalize
    y = _nan((N, D), torch.float32, dev)
    call("pmi_l2norm_rows", ptr(embd), ptr(y), N, D, 2.5)
    torch.cuda.synchronize()
    R.check(f"l2norm_rows N={N} D={D}", y.cpu(), 2.5 * F.normalize(emb.double(), dim=1), 8 * E32 * 2.5)


def test_spherical_loss_parallel_and_antipodal():
    """An embedding parallel to its target (u = 0: zero contribution, the kernel's `u > 1e-12 ? ... : 0`) and one antipodal
    (u = 2: asin'(1) is infinite; the kernel clamps sqrt(1 - u^2/4) at 1e-6): finite outputs, the documented loss, and gradients
    bounded by the clamp (the tangential part of e - t vanishes up to |e|^2 - 1 ~ E32 D)."""
    dev = _dev()
    D = 768
    g = torch.Generator().manual_seed(1)
    t = F.normalize(torch.randn(1, D, generator=g), dim=1)
    wts = torch.tensor([1.0])
    for sign, ref_loss in ((1.0, 0.0), (-1.0, 2 * (math.pi / 2) ** 2)):
        emb = sign * 2.0 * t
        loss, demb = _sph_call(emb.to(dev), t.to(dev), wts.to(dev), 1, 1.0, 1.0)
        assert torch.isfinite(loss).all() and torch.isfinite(demb).all()
        R.check(f"spherical_loss sign={sign:+.0f} loss", loss, torch.tensor([ref_loss]), 1e-3 * (1 + ref_loss))
        coef = 2 * (math.pi / 2) / (1e-6 * 2) if sign < 0 else 2.0
        R.check(f"spherical_loss sign={sign:+.0f} demb", demb, torch.zeros(1, D), coef * 2 * 64 * E32 * math.sqrt(D) / 2.0)
