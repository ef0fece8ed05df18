"""GPU parity of the CLIP ResNet image towers (engine/resnet.py, csrc/resnet.hip) against float64 references.

Kernel level: the attention-pool kernels against tests/_ref64.py's float64 attention with its elementwise worst-case rounding bounds, the
input-staging and token kernels against float64 and against their adjoints; then their edge shapes (every length at which the
attention kernels' loops change shape, T = 1 and RN_TMAX, the token and staging adjoints per element, more items than the elementwise kernels'
capped grids hold), outputs inside guard bands, refusals with nothing written.  Tower level: tests/_rn_ref64.py (unfolded BatchNorm, float64)
with the ViT bounds of tests/test_gpu_clip.py: embedding rel-L2 <= 1e-2 against the exact tower, image-gradient rel-L2 <= 2e-2 and cosine
>= 0.9995 against the float64 tower pinned to the engine's ReLU masks (why: _tower_case).  RN50x64 (too slow for a float64 CPU pass in a
test) is checked by properties: determinism, batch independence and bf16 / f16 agreement.
"""
import pytest
import torch
import torch.nn.functional as F

import _ref64 as R64
import _rn_ref64 as RN

pytestmark = pytest.mark.gpu

TINY = (64, (1, 1, 1, 1), 16, 8, 64)            # width 16: attention pool C = 512, 8 heads
ATTN_SHAPES = [(50, 2048), (82, 2560), (145, 3072), (197, 4096)]
DT = {"bf16": 1, "f16": 0}


def _rel(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())


def _cos(a, b):
    return float(F.cosine_similarity(a.double().cpu().flatten(), b.double().cpu().flatten(), dim=0))


def _call(name, *args):
    from perceptor_amd._hip import call
    call(name, *args)


def _p(t):
    return t.data_ptr()


# ---- kernel level --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n", [2, 3])
@pytest.mark.parametrize("T,C", ATTN_SHAPES)
def test_attnpool_attention_vs_fp64(T, C, n, dtype):
    heads = C // 64
    td = R64.TD[dtype]
    regime = "peaked" if n == 3 else "flat"
    q, k, v = R64.attn_inputs(n * heads, 1, 64, regime, dtype, seed=T + n, Tk=T, scale=0.125)     # [n*heads, 1|T, 64] float64, 16-bit exact
    g = torch.Generator().manual_seed(C + n)
    dout = R64.rnd(torch.randn(n * heads, 1, 64, generator=g, dtype=torch.float64), dtype)
    r = R64.attn_ref(q, k, v, dout, scale=0.125)
    qd = q.view(n, C).to(td).cuda()
    kv = torch.cat([k.view(n, heads, T, 64).permute(0, 2, 1, 3).reshape(n * T, C),
                    v.view(n, heads, T, 64).permute(0, 2, 1, 3).reshape(n * T, C)], dim=1).to(td).cuda().contiguous()
    o = torch.empty((n, C), dtype=td, device="cuda")
    P = torch.empty((n * heads, T), dtype=torch.float32, device="cuda")
    _call("pmi_rn_attn_fwd", _p(qd), _p(kv), _p(o), _p(P), n, T, C, heads, 0.125, DT[dtype])
    R64.check(f"rn attn O T={T} C={C} n={n} {dtype}", o.view(n * heads, 1, 64), r["O"], R64.attn_tol(r, "O", dtype))
    R64.check(f"rn attn P T={T} C={C} n={n} {dtype}", P.view(n * heads, 1, T), r["P"], 1e-5 * float(r["P"].max()))
    do = dout.view(n, C).to(td).cuda()
    dq = torch.empty((n, C), dtype=td, device="cuda")
    dkv = torch.empty((n * T, 2 * C), dtype=td, device="cuda")
    _call("pmi_rn_attn_bwd", _p(qd), _p(kv), _p(P), _p(do), _p(dq), _p(dkv), n, T, C, heads, 0.125, DT[dtype])
    dk = dkv[:, :C].reshape(n, T, heads, 64).permute(0, 2, 1, 3).reshape(n * heads, T, 64)
    dv = dkv[:, C:].reshape(n, T, heads, 64).permute(0, 2, 1, 3).reshape(n * heads, T, 64)
    R64.check(f"rn attn dQ T={T} C={C} n={n} {dtype}", dq.view(n * heads, 1, 64), r["dQ"], R64.attn_tol(r, "dQ", dtype))
    R64.check(f"rn attn dK T={T} C={C} n={n} {dtype}", dk, r["dK"], R64.attn_tol(r, "dK", dtype))
    R64.check(f"rn attn dV T={T} C={C} n={n} {dtype}", dv, r["dV"], R64.attn_tol(r, "dV", dtype))


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n,hw", [(2, 50), (3, 33)])
def test_stage_input_vs_fp64_and_adjoint(n, hw, dtype):
    from perceptor_amd.engine.vit import CLIP_MEAN, CLIP_STD
    from perceptor_amd.utils.synth import seeded_noise
    td, u = R64.TD[dtype], R64.U[dtype]
    h, w = hw, hw + 6
    img = seeded_noise((n, 3, h, w), 3) * 0.25 + 0.5
    mean, std = torch.tensor(CLIP_MEAN).cuda(), torch.tensor(CLIP_STD).cuda()
    x = torch.empty((n, h, w, 8), dtype=td, device="cuda")
    img_d = img.cuda()                    # named: a temporary's memory could be handed to the next allocation before the launch
    _call("pmi_rn_stage_input", _p(img_d), _p(mean), _p(std), _p(x), n, h, w, DT[dtype])
    want = RN.normalize(img).permute(0, 2, 3, 1)
    R64.check(f"rn stage_input {n}x{h}x{w} {dtype}", x[..., :3], want, u * float(want.abs().max()) * 1.01)
    assert float(x[..., 3:].abs().max()) == 0.0
    # adjoint of the linear part x -> x / std: <A img, y> = <img, A^T y>
    y = seeded_noise((n, h, w, 4), 4).cuda()
    g = torch.empty((n, 3, h, w), dtype=torch.float32, device="cuda")
    _call("pmi_rn_stage_input_bwd", _p(y), 4, _p(std), _p(g), n, h, w, 0.5)
    lin = img.double().cuda() / std.double().view(1, 3, 1, 1)
    lhs = float((lin.permute(0, 2, 3, 1) * y[..., :3].double()).sum()) * 0.5
    rhs = float((img.double().cuda() * g.double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * (abs(lhs) + float((lin.abs().permute(0, 2, 3, 1) * y[..., :3].abs().double()).sum())), (lhs, rhs)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("n,hw,C", [(2, 49, 2048), (3, 81, 2560), (2, 144, 3072), (3, 196, 4096), (2, 4, 512)])
def test_tokens_vs_fp64_and_adjoint(n, hw, C, dtype):
    td, u = R64.TD[dtype], R64.U[dtype]
    g = torch.Generator().manual_seed(hw)
    x = R64.rnd(torch.randn(n, hw, C, generator=g, dtype=torch.float64), dtype)
    pos = torch.randn(hw + 1, C, generator=g, dtype=torch.float64).float()
    tok = torch.empty((n * (hw + 1), C), dtype=td, device="cuda")
    x_d, pos_d = x.to(td).cuda(), pos.cuda()
    _call("pmi_rn_tokens", _p(x_d), _p(pos_d), _p(tok), n, hw, C, DT[dtype])
    want = torch.cat([x.mean(dim=1, keepdim=True), x], dim=1) + pos.double()[None]
    scale = torch.cat([x.abs().mean(dim=1, keepdim=True), x.abs()], dim=1) + pos.double().abs()[None]
    err = (tok.view(n, hw + 1, C).double().cpu() - want).abs()
    R64.parity(f"rn tokens n={n} hw={hw} C={C} {dtype}", float(err.max()), float((1.01 * u * scale).max()))
    assert bool((err <= 1.01 * u * scale + 1e-6 * scale).all())
    # adjoint (the linear part, pos = 0) in fp32 storage terms: <A x, y> = <x, A^T y>, with the query path's gradient of row 0 added
    y = R64.rnd(torch.randn(n, hw + 1, C, generator=g, dtype=torch.float64), dtype)
    dq0 = torch.randn(n, C, generator=g, dtype=torch.float64).float()
    dx = torch.empty((n, hw, C), dtype=td, device="cuda")
    y_d, dq0_d = y.to(td).cuda().view(n * (hw + 1), C), dq0.cuda()
    _call("pmi_rn_tokens_bwd", _p(y_d), _p(dq0_d), _p(dx), n, hw, C, DT[dtype])
    ax = torch.cat([x.mean(dim=1, keepdim=True), x], dim=1)
    lhs = float((ax * y).sum() + (x.mean(dim=1) * dq0.double()).sum())
    rhs = float((x * dx.double().cpu()).sum())
    bound = u * float((x.abs() * (y[:, 1:].abs() + (y[:, :1].abs() + dq0.double().abs()[:, None]) / hw)).sum()) * 1.01
    assert abs(lhs - rhs) <= bound, (lhs, rhs, bound)


# ---- kernel level: edge shapes, guard bands, refusals ---------------------------------------------------------------------------------------
GRID_ITEMS = 8192 * 256           # grid_for() caps the elementwise kernels' grids at 8192 workgroups of 256 threads: more items than this
PAD = 256                         # and a thread takes a second step of its grid-stride loop.  PAD: guard bytes on each side of an output
FILL = 0x7B                       # 0x7B7B = 6.1e4 in f16, 1.3e36 in bf16; 0x7B7B7B7B = 1.3e36 in fp32: nothing a kernel under test writes


def _guarded(shape, td):
    """an output tensor inside guard bands of FILL bytes, itself pre-filled with them: (tensor, whole buffer)"""
    nbytes = torch.empty((), dtype=td).element_size()
    for d in shape:
        nbytes *= d
    buf = torch.full((PAD + nbytes + PAD,), FILL, dtype=torch.uint8, device="cuda")
    return buf[PAD:PAD + nbytes].view(td).view(shape), buf


def _bands_intact(buf):
    return bool((buf[:PAD] == FILL).all()) and bool((buf[-PAD:] == FILL).all())


def _untouched(buf):
    return bool((buf == FILL).all())


def _refused(name, *args):
    with pytest.raises(RuntimeError, match="bad argument"):
        _call(name, *args)


ATTN_EDGE_T = [1, 2, 5, 31, 32, 33, 255, 256, 257, 513, 1024]       # idle row groups (< 32), one row, the second step of the t += 256 loops, RN_TMAX


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("T", ATTN_EDGE_T)
def test_attnpool_attention_edge_lengths(T, dtype):
    """pmi_rn_attn_fwd / _bwd at every length where their loops change shape, heads 1 and 8, n 1 and 3, four score regimes (mass spread,
    near one-hot, on the first key, on the last key), outputs inside guard bands; at T = 1 the softmax is 1 and dK is 0 exactly"""
    td = R64.TD[dtype]
    for heads, n, regime in [(h, n, r) for h in (1, 8) for n in (1, 3) for r in ("flat", "peaked", "first", "last")]:
        C, B = 64 * heads, n * heads
        tag = f"T={T} heads={heads} n={n} {regime} {dtype}"
        q, k, v = R64.attn_inputs(B, 1, 64, regime, dtype, seed=T + 7 * heads + n, Tk=T, scale=0.125)
        g = torch.Generator().manual_seed(T + heads + n)
        dout = R64.rnd(torch.randn(B, 1, 64, generator=g, dtype=torch.float64), dtype)
        r = R64.attn_ref(q, k, v, dout, scale=0.125)
        if regime in ("first", "last") and T > 1:
            top = r["P"].argmax(dim=-1)
            assert bool((top == (0 if regime == "first" else T - 1)).all()), tag
        tok = lambda z: z.view(n, heads, T, 64).permute(0, 2, 1, 3).reshape(n * T, C)
        qd = q.view(n, C).to(td).cuda()
        kv = torch.cat([tok(k), tok(v)], dim=1).to(td).cuda().contiguous()
        o, o_buf = _guarded((n, C), td)
        P, p_buf = _guarded((B, T), torch.float32)
        _call("pmi_rn_attn_fwd", _p(qd), _p(kv), _p(o), _p(P), n, T, C, heads, 0.125, DT[dtype])
        torch.cuda.synchronize()
        assert _bands_intact(o_buf) and _bands_intact(p_buf), tag
        R64.check(f"rn attn edge O {tag}", o.view(B, 1, 64), r["O"], R64.attn_tol(r, "O", dtype))
        R64.check(f"rn attn edge P {tag}", P.view(B, 1, T), r["P"], 1e-5 * float(r["P"].max()))
        do = dout.view(n, C).to(td).cuda()
        dq, dq_buf = _guarded((n, C), td)
        dkv, dkv_buf = _guarded((n * T, 2 * C), td)
        _call("pmi_rn_attn_bwd", _p(qd), _p(kv), _p(P), _p(do), _p(dq), _p(dkv), n, T, C, heads, 0.125, DT[dtype])
        torch.cuda.synchronize()
        assert _bands_intact(dq_buf) and _bands_intact(dkv_buf), tag
        heads_of = lambda z: z.reshape(n, T, heads, 64).permute(0, 2, 1, 3).reshape(B, T, 64)
        dk, dv = heads_of(dkv[:, :C]), heads_of(dkv[:, C:])
        R64.check(f"rn attn edge dQ {tag}", dq.view(B, 1, 64), r["dQ"], R64.attn_tol(r, "dQ", dtype))
        R64.check(f"rn attn edge dK {tag}", dk, r["dK"], R64.attn_tol(r, "dK", dtype))
        R64.check(f"rn attn edge dV {tag}", dv, r["dV"], R64.attn_tol(r, "dV", dtype))
        if T == 1:
            assert bool((P == 1.0).all()) and bool((dk == 0).all()), tag
            assert torch.equal(o.view(B, 64), v.view(B, 64).to(td).cuda())          # the one value row, as stored


def test_attnpool_attention_refuses_without_writing():
    """T = 0, T = RN_TMAX + 1, C != 64 heads and an unknown dtype are refused before any launch: no output byte changes"""
    n, heads, T = 2, 2, 1025
    C = 64 * heads
    q = torch.zeros((n, C), dtype=torch.bfloat16, device="cuda")
    kv = torch.zeros((n * T, 2 * C), dtype=torch.bfloat16, device="cuda")
    do = torch.zeros((n, C), dtype=torch.bfloat16, device="cuda")
    Pin = torch.zeros((n * heads, T), dtype=torch.float32, device="cuda")
    o, o_buf = _guarded((n, C), torch.bfloat16)
    P, p_buf = _guarded((n * heads, T), torch.float32)
    dq, dq_buf = _guarded((n, C), torch.bfloat16)
    dkv, dkv_buf = _guarded((n * T, 2 * C), torch.bfloat16)
    for t_, c_, h_, dt_ in [(0, C, heads, 1), (1025, C, heads, 1), (50, C + 64, heads, 1), (50, C - 8, heads, 1), (50, C, 0, 1), (50, C, heads, 2), (50, C, heads, 7)]:
        _refused("pmi_rn_attn_fwd", _p(q), _p(kv), _p(o), _p(P), n, t_, c_, h_, 0.125, dt_)
        _refused("pmi_rn_attn_bwd", _p(q), _p(kv), _p(Pin), _p(do), _p(dq), _p(dkv), n, t_, c_, h_, 0.125, dt_)
    _call("pmi_rn_attn_fwd", _p(q), _p(kv), _p(o), _p(P), n, 1024, C, heads, 0.125, 1)       # RN_TMAX itself is taken
    torch.cuda.synchronize()
    assert _bands_intact(o_buf) and not _untouched(o_buf)
    assert _untouched(dq_buf) and _untouched(dkv_buf)
    o2, o2_buf = _guarded((n, C), torch.bfloat16)
    P2, p2_buf = _guarded((n * heads, T), torch.float32)
    _refused("pmi_rn_attn_fwd", _p(q), _p(kv), _p(o2), _p(P2), n, 1025, C, heads, 0.125, 1)
    torch.cuda.synchronize()
    assert _untouched(o2_buf) and _untouched(p2_buf)


def _tokens_bwd_case(n, hw, C, dtype, seed, with_dq0):
    """pmi_rn_tokens_bwd per element: dx = dtok[1 + p] + (dtok[0] + dq0) / HW within 1.01 u |terms| (the one 16-bit rounding) + 2^-21 |terms|
    (the fp32 steps: 1 / HW, two sums, one product), the output inside guard bands"""
    td, u = R64.TD[dtype], R64.U[dtype]
    g = torch.Generator().manual_seed(seed)
    y = R64.rnd(torch.randn(n, hw + 1, C, generator=g, dtype=torch.float64), dtype)
    dq0 = torch.randn(n, C, generator=g, dtype=torch.float64).float()
    y_d, dq0_d = y.to(td).cuda().view(n * (hw + 1), C), dq0.cuda()
    dx, buf = _guarded((n, hw, C), td)
    _call("pmi_rn_tokens_bwd", _p(y_d), _p(dq0_d) if with_dq0 else None, _p(dx), n, hw, C, DT[dtype])
    torch.cuda.synchronize()
    assert _bands_intact(buf)
    row0 = y[:, :1] + (dq0.double()[:, None] if with_dq0 else 0.0)
    want = y[:, 1:] + row0 / hw
    terms = y[:, 1:].abs() + (y[:, :1].abs() + (dq0.double().abs()[:, None] if with_dq0 else 0.0)) / hw
    err = (dx.double().cpu() - want).abs()
    tol = (1.01 * u + 2.0 ** -21) * terms
    tag = f"rn tokens_bwd n={n} hw={hw} C={C} dq0={'given' if with_dq0 else 'NULL'} {dtype}"
    R64.parity(tag, float((err / tol).max()), 1.0)
    assert bool((err <= tol).all()), tag
    return err, tol


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("C", [8, 512, 2560])
@pytest.mark.parametrize("hw", [1, 4, 9, 49])
def test_tokens_bwd_per_element(hw, C, dtype):
    for with_dq0 in (True, False):
        _tokens_bwd_case(3, hw, C, dtype, hw * 31 + C, with_dq0)


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("ldc", [4, 8])
@pytest.mark.parametrize("mul", [1.0, 2.0 ** -16])
def test_stage_input_bwd_per_element(mul, ldc, dtype):
    """pmi_rn_stage_input_bwd per element against float64: dimg = dx / std * mul, two fp32 roundings; the channels past the third of dx (the
    convolution's pad channels) hold NaN and are never read.  (No 16-bit type in this kernel: dtype picks the seed only.)"""
    from perceptor_amd.engine.vit import CLIP_STD
    n, h, w = (2, 33, 39) if dtype == "bf16" else (3, 50, 56)
    g = torch.Generator().manual_seed(ldc + n)
    dx = torch.randn(n, h, w, ldc, generator=g, dtype=torch.float64).float()
    dx[..., 3:] = float("nan")
    std = torch.tensor(CLIP_STD)
    dx_d, std_d = dx.cuda(), std.cuda()
    out, buf = _guarded((n, 3, h, w), torch.float32)
    _call("pmi_rn_stage_input_bwd", _p(dx_d), ldc, _p(std_d), _p(out), n, h, w, mul)
    torch.cuda.synchronize()
    assert _bands_intact(buf)
    want = dx[..., :3].double().permute(0, 3, 1, 2) / std.double().view(1, 3, 1, 1) * mul
    err = (out.double().cpu() - want).abs()
    tol = 2.02 * 2.0 ** -24 * want.abs()
    R64.parity(f"rn stage_input_bwd n={n} {h}x{w} ldc={ldc} mul={mul:g}", float((err / tol.clamp_min(1e-300)).max()), 1.0)
    assert bool((err <= tol).all())
    _refused("pmi_rn_stage_input_bwd", _p(dx_d), 2, _p(std_d), _p(out), n, h, w, mul)


def _first_last(err, tol, tag):
    e, t = err.flatten(), tol.flatten()
    assert float(e[0]) <= float(t[0]) and float(e[-1]) <= float(t[-1]), (tag, float(e[0]), float(t[0]), float(e[-1]), float(t[-1]))


def test_stage_input_grid_stride():
    """n * h * w = 8192 * 256 + 1 items: the smallest count at which a thread of pmi_rn_stage_input takes a second grid-stride step"""
    from perceptor_amd.engine.vit import CLIP_MEAN, CLIP_STD
    from perceptor_amd.utils.synth import seeded_noise
    n, h, w = 1, 1, GRID_ITEMS + 1
    u = R64.U["bf16"]
    img = seeded_noise((n, 3, h, w), 5) * 0.25 + 0.5
    mean, std = torch.tensor(CLIP_MEAN).cuda(), torch.tensor(CLIP_STD).cuda()
    img_d = img.cuda()
    x, buf = _guarded((n, h, w, 8), torch.bfloat16)
    _call("pmi_rn_stage_input", _p(img_d), _p(mean), _p(std), _p(x), n, h, w, DT["bf16"])
    torch.cuda.synchronize()
    assert _bands_intact(buf)
    want = RN.normalize(img).permute(0, 2, 3, 1)
    err = (x[..., :3].double().cpu() - want).abs()
    # one 16-bit rounding and the fp32 subtraction and division; absolute where x is near its channel's mean: the fp32 constants' own
    # rounding, 2^-25 mean / std <= 2^-24 (mean / std < 1.9)
    tol = (1.01 * u + 2.0 ** -21) * want.abs() + 2.0 ** -24 * (1.0 + 2.0 ** -7)
    R64.parity(f"rn stage_input grid stride {n}x{h}x{w}", float((err / tol).max()), 1.0)
    assert bool((err <= tol).all())
    _first_last(err, tol, "stage_input")
    assert float(x[..., 3:].abs().max()) == 0.0


def test_stage_input_bwd_grid_stride():
    """n * 3 * h * w = 8192 * 256 + 1 items"""
    from perceptor_amd.engine.vit import CLIP_STD
    from perceptor_amd.utils.synth import seeded_noise
    n, h, w = 1, 1, (GRID_ITEMS + 1) // 3
    assert n * 3 * h * w == GRID_ITEMS + 1
    dx = seeded_noise((n, h, w, 4), 6)
    std = torch.tensor(CLIP_STD)
    dx_d, std_d = dx.cuda(), std.cuda()
    out, buf = _guarded((n, 3, h, w), torch.float32)
    _call("pmi_rn_stage_input_bwd", _p(dx_d), 4, _p(std_d), _p(out), n, h, w, 0.5)
    torch.cuda.synchronize()
    assert _bands_intact(buf)
    want = dx[..., :3].double().permute(0, 3, 1, 2) / std.double().view(1, 3, 1, 1) * 0.5
    err = (out.double().cpu() - want).abs()
    tol = 2.02 * 2.0 ** -24 * want.abs()
    R64.parity(f"rn stage_input_bwd grid stride {n}x{h}x{w}", float((err / tol.clamp_min(1e-300)).max()), 1.0)
    assert bool((err <= tol).all())
    _first_last(err, tol, "stage_input_bwd")


def test_tokens_grid_stride():
    """n * (hw + 1) * C / 8 = 6554 * 320 > 8192 * 256 items at the product's widest-but-one C = 2560 (6553 * 320 is below)"""
    n, hw, C, dtype = 1, 6553, 2560, "bf16"
    assert n * hw * (C // 8) <= GRID_ITEMS < n * (hw + 1) * (C // 8)
    td, u = R64.TD[dtype], R64.U[dtype]
    g = torch.Generator().manual_seed(hw)
    x = R64.rnd(torch.randn(n, hw, C, generator=g, dtype=torch.float64), dtype)
    pos = torch.randn(hw + 1, C, generator=g, dtype=torch.float64).float()
    x_d, pos_d = x.to(td).cuda(), pos.cuda()
    tok, buf = _guarded((n * (hw + 1), C), td)
    _call("pmi_rn_tokens", _p(x_d), _p(pos_d), _p(tok), n, hw, C, DT[dtype])
    torch.cuda.synchronize()
    assert _bands_intact(buf)
    want = torch.cat([x.mean(dim=1, keepdim=True), x], dim=1) + pos.double()[None]
    scale = torch.cat([x.abs().mean(dim=1, keepdim=True), x.abs()], dim=1) + pos.double().abs()[None]
    err = (tok.view(n, hw + 1, C).double().cpu() - want).abs()
    tol = (1.01 * u + (hw + 2) * 2.0 ** -24) * scale          # one 16-bit rounding + the worst case of an fp32 sum of hw terms in order
    R64.parity(f"rn tokens grid stride n={n} hw={hw} C={C}", float((err / tol).max()), 1.0)
    assert bool((err <= tol).all())
    _first_last(err, tol, "tokens")


def test_tokens_bwd_grid_stride():
    """n * hw * C / 8 = 6554 * 320 > 8192 * 256 items"""
    n, hw, C = 1, 6554, 2560
    assert n * (hw - 1) * (C // 8) <= GRID_ITEMS < n * hw * (C // 8)
    err, tol = _tokens_bwd_case(n, hw, C, "bf16", 11, True)
    _first_last(err, tol, "tokens_bwd")


# ---- tower level ------------------------------------------------------------------------------------------------------------------------
_REF = {}


def _tower_case(name, cfg, n, in_hw, dtype, seed=21):
    """HIP embedding and input gradient (of <emb, d_emb>) and their float64 references: the exact tower's embedding, and the input gradient
    of the float64 tower pinned to the engine's own ReLU masks (its saved post-ReLU activations).  The input gradient of a ReLU network is
    piecewise constant: any 16-bit forward moves some pre-activations across zero, and the exact tower's gradient differs from it by far
    more than the rounding; with the masks pinned, what remains is the arithmetic of the engine's roundings."""
    from perceptor_amd import models
    from perceptor_amd.engine.resnet import blocks as resnet_blocks
    from perceptor_amd.transforms import resize, resize_backward
    from perceptor_amd.utils.synth import seeded_noise
    kw = dict(rn_config=cfg) if name.startswith("rn-") else {}
    model = models.OpenCLIP(name, "synthetic", {"bf16": "bf16", "f16": "fp16"}[dtype], **kw).to("cuda")
    eng = model.engine
    res, out = cfg[0], cfg[4]
    img = (seeded_noise((n, 3) + in_hw, seed) * 0.25 + 0.5).cuda()
    d_emb = seeded_noise((n, out), seed + 1) * 1e-2              # loss-gradient scale (f16 multiplies it by gscale = 2^16 on the way in)
    emb = eng.forward(img, save=True)
    sv = eng.saved
    masks = [(t > 0).permute(0, 3, 1, 2).cpu().double() for t in list(sv["stem"]) + [t for tr in sv["tape"] for t in tr]]
    layer = [p.split(".")[0] for p, *_ in resnet_blocks(cfg)]
    ends = [i for i in range(len(layer)) if i + 1 == len(layer) or layer[i + 1] != layer[i]]
    st_hip = [sv["tape"][i][2].permute(0, 3, 1, 2).cpu() for i in ends]             # each layer's output (its last block's)
    grad = eng.backward(d_emb.cuda() * eng.gscale)
    sd = {k: v.cpu() for k, v in model.visual_state_dict().items()}
    resized = in_hw != (res, res)
    r = resize(img, (res, res)).cpu() if resized else img.cpu()
    key = (name, n, in_hw, seed)
    if key not in _REF:
        st64 = []
        _REF[key] = (RN.tower(sd, cfg, RN.normalize(r), stages=st64), st64[1:])
    e64, st64 = _REF[key]
    x64 = r.double().requires_grad_(True)
    with torch.enable_grad():
        (RN.encode(sd, cfg, x64, masks=masks) * d_emb.double()).sum().backward()
    g_pin = resize_backward(x64.grad.float().cuda(), in_hw).cpu().double() if resized else x64.grad
    return emb, grad, e64, g_pin, st_hip, st64


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name,n,in_hw", [("rn-tiny", 3, (64, 64)), ("RN50", 2, (224, 224)), ("RN101", 2, (224, 224)),
                                          ("RN50x4", 2, (256, 256)), ("RN50x16", 1, (384, 384))])
def test_tower_vs_fp64(name, n, in_hw, dtype):
    from perceptor_amd.engine import resnet
    cfg = TINY if name == "rn-tiny" else resnet.RN_CONFIGS[name]
    emb, grad, e64, g_pin, st_hip, st64 = _tower_case(name, cfg, n, in_hw, dtype)
    assert emb.shape == (n, cfg[4]) and grad.shape == (n, 3) + in_hw
    e_rel, g_rel, g_cos = _rel(emb, e64), _rel(grad, g_pin), _cos(grad, g_pin)
    stages = " ".join(f"{_rel(a, b):.1e}" for a, b in zip(st_hip, st64))
    print(f"[parity] rn clip {name} {dtype} n={n} in={in_hw}: emb rel-L2={e_rel:.3e}; grad vs mask-pinned fp64 rel-L2={g_rel:.3e}, "
          f"cos={g_cos:.6f}; layer1-4 output rel-L2 {stages}")
    assert e_rel <= 1e-2
    assert g_rel <= 2e-2 and g_cos >= 0.9995


def _tape_masks(eng, cfg):
    """Per layer: the 0/1 ReLU masks of the saved forward (the post-ReLU activations of its blocks), concatenated per image."""
    from perceptor_amd.engine.resnet import blocks
    layer = [p.split(".")[0] for p, *_ in blocks(cfg)]
    out = {}
    for name, tr in zip(layer, eng.saved["tape"]):
        out.setdefault(name, []).extend((t > 0).flatten(1) for t in tr)
    return {k: torch.cat(v, dim=1) for k, v in out.items()}


def test_rn50x64_properties():
    """Determinism, batch independence and bf16 / f16 agreement.  The embedding is continuous in the rounding and meets tight bounds; the
    image gradient is piecewise constant: a batch of 1 and of 4 run differently split sums (pmi_igemm picks split-K and kernels by M), as do
    bf16 and f16, and every ReLU mask that flips changes it.  The per-layer flip fractions are printed with the numbers; the
    gradient bounds are those measurements with a margin -- the mask-pinned comparisons of test_tower_vs_fp64 bound its arithmetic."""
    from perceptor_amd.engine import resnet
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    cfg = resnet.RN_CONFIGS["RN50x64"]
    sd = synth_state_dict(resnet.rn_state_dict_shapes(cfg), 0)
    img = (seeded_noise((4, 3, 448, 448), 31) * 0.25 + 0.5).cuda()
    demb = seeded_noise((4, cfg[4]), 32).cuda() * 1e-2
    res, masks = {}, {}
    for dt in ("bf16", "f16"):
        eng = resnet.ResNetEngine(cfg, sd, "cuda", dt)

        def run(x, d, keep=None):
            e = eng.forward(x, save=True)
            if keep is not None:
                keep.append(_tape_masks(eng, cfg))
            return e, eng.backward(d * eng.gscale)

        e1, g1 = run(img[:2], demb[:2])
        assert e1.shape == (2, 1024) and g1.shape == (2, 3, 448, 448)
        assert bool(torch.isfinite(e1).all()) and bool(torch.isfinite(g1).all()) and float(g1.abs().max()) > 0
        e2, g2 = run(img[:2], demb[:2])
        assert torch.equal(e1, e2) and torch.equal(g1, g2), f"{dt}: two calls differ"
        k4, k1 = [], []
        e4, g4 = run(img, demb, k4)
        one = [run(img[i:i + 1], demb[i:i + 1], k1) for i in range(4)]
        eb, gb = torch.cat([o[0] for o in one]), torch.cat([o[1] for o in one])
        flips = {L: float((torch.cat([k[L] for k in k1]) != k4[0][L]).float().mean()) for L in k4[0]}
        masks[dt] = k4[0]
        res[dt] = (e1, g1, _rel(eb, e4), _rel(gb, g4), _cos(gb, g4))
        print(f"[parity] rn clip RN50x64 {dt} batch-1 x4 vs batch-4: emb rel-L2={res[dt][2]:.3e}, grad rel-L2={res[dt][3]:.3e}, "
              f"cos={res[dt][4]:.6f}; ReLU masks flipped per layer " + " ".join(f"{L} {v:.1e}" for L, v in flips.items()))
        del eng
    (eb_, gb_, *_), (eh, gh, *_) = res["bf16"], res["f16"]
    flips = " ".join(f"{L} {float((masks['bf16'][L] != masks['f16'][L]).float().mean()):.1e}" for L in masks["bf16"])
    print(f"[parity] rn clip RN50x64 bf16 vs f16: emb rel-L2={_rel(eh, eb_):.3e}, grad rel-L2={_rel(gh, gb_):.3e}, cos={_cos(gh, gb_):.6f}; "
          f"ReLU masks flipped per layer {flips}")
    assert res["bf16"][2] <= 3e-3 and res["f16"][2] <= 1e-3               # measured 1.4e-3 / 1.9e-4
    assert res["bf16"][4] >= 0.97 and res["f16"][4] >= 0.995             # measured 0.984 / 0.998
    assert _rel(eh, eb_) <= 2e-2 and _cos(gh, gb_) >= 0.96               # measured 3.5e-3, 0.974


# ---- losses ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_clip_loss_rn50x4_paths_and_sharding(precision):
    from perceptor_amd import losses
    from perceptor_amd.utils.synth import seeded_noise
    loss = losses.CLIP("RN50x4", precision, weights="synthetic").to("cuda")
    loss.add_encodings_(seeded_noise((3, 640), 7), weights=[1.0, 0.5, 2.0])
    img = (seeded_noise((4, 3, 200, 240), 9) * 0.25 + 0.5).cuda()
    val, grad = loss.loss_and_grad(img)
    assert grad.shape == img.shape and bool(torch.isfinite(grad).all()) and float(grad.abs().max()) > 0
    x = img.clone().requires_grad_(True)
    with torch.enable_grad():
        lv = loss(x)
        lv.backward()
    lv = float(lv.detach())
    # two ranks holding half the batch each reproduce the full-batch gradient
    _, g_a = loss.loss_and_grad(img[:2], n_total=4)
    _, g_b = loss.loss_and_grad(img[2:], n_total=4)
    gs = torch.cat([g_a, g_b])
    print(f"[parity] rn clip loss RN50x4 {precision}: loss {float(val):.6f} vs autograd path {lv:.6f}, grad rel-L2={_rel(x.grad, grad):.3e} "
          f"cos={_cos(x.grad, grad):.6f}; sharded grad rel-L2={_rel(gs, grad):.3e} cos={_cos(gs, grad):.6f}")
    assert abs(lv - float(val)) <= 1e-4 * abs(float(val))
    assert _rel(x.grad, grad) <= 2e-2 and _cos(x.grad, grad) >= 0.9995
    # n_total scales the shard's gradient by an exact power of two: the same batch-2 call without it gives twice the values -- bit for bit in
    # bf16; in f16 the halved gradients reach the subnormal range in places, which rounds differently
    _, g_a2 = loss.loss_and_grad(img[:2])
    _, g_b2 = loss.loss_and_grad(img[2:])
    r2 = max(_rel(g_a * 2, g_a2), _rel(g_b * 2, g_b2))
    print(f"[parity] rn clip loss RN50x4 {precision}: shard x 2 vs batch-2 call rel-L2={r2:.3e}")
    if precision == "bf16":
        assert torch.equal(g_a * 2, g_a2) and torch.equal(g_b * 2, g_b2)
    else:
        assert r2 <= 1e-2
    # against the full batch: the shards run differently split sums and flip ReLU masks (test_rn50x64_properties); measured cos 0.9964
    # (bf16), 0.9992 (f16)
    assert _cos(gs, grad) >= (0.99 if precision == "bf16" else 0.998)


def test_add_texts_rn50x4_text_tower():
    from oracle import clip_text
    from perceptor_amd import losses
    from perceptor_amd.engine import text as text_engine
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    from perceptor_amd.utils.tokenizer import ClipTokenizer
    tcfg = text_engine.TEXT_CONFIGS["RN50x4"]
    assert tcfg == (77, 49408, 640, 12, 10, 640)
    loss = losses.CLIP("RN50x4", weights="synthetic").to("cuda")
    loss.model._tokenizer = ClipTokenizer(merges=[("a", "b"), ("ab", "c</w>"), ("c", "a")])
    prompts = ["abc cab", "b", "a cab abc"]
    loss.add_texts_(prompts, weights=[1.0, 0.5, 2.0])
    assert loss.encodings.shape == (3, 640)
    ids = loss.model.tokenize(prompts)
    sd = synth_state_dict(clip_text.text_state_dict_shapes(tcfg), 0)
    _, want = clip_text.text_forward(sd, tcfg, ids, True)
    rel = _rel(loss.encodings.data, F.normalize(want))
    # the same tower in f16 (GEMM operands carry 3 more bits): test_gpu_text.py's f16 bound
    t16 = text_engine.TextEngine(tcfg, sd, "cuda", "f16", quick_gelu=True)
    rel16 = _rel(F.normalize(t16.forward(ids)[1]), F.normalize(want))
    print(f"[parity] rn clip text tower RN50x4 (width 640): normalised pooled rel-L2 bf16={rel:.3e}, f16={rel16:.3e}")
    assert rel < 1.5e-2 and rel16 < 2e-3
    img = (seeded_noise((2, 3, 288, 288), 52) * 0.25 + 0.5).cuda()
    val, grad = loss.loss_and_grad(img)
    assert bool(torch.isfinite(val)) and grad.shape == img.shape and float(grad.abs().max()) > 0
