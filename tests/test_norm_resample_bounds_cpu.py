"""CPU: the bounds of tests/test_gpu_norm_resample.py are tight enough to catch plausible kernel defects, and not vacuous.

Each defect is restated in float64 at a GPU test's shape, seed and inputs; the restated output must land at least 2x outside the bound
the GPU test asserts.  In the benign regime (N(0.3, 1.5^2) inputs) the GroupNorm output bound stays within 4 u max|y|.
"""
import os
import re

import pytest
import torch

import _norm_ref64 as R
import test_gpu_norm_resample as T

MARGIN = 2.0
DTYPES = ["f16", "bf16"]


def _margin(tag, defect, ref, tol):
    m = R.defect_ratio(defect, ref, tol)
    print(f"[margin] {tag}: {m:.1f}x the bound")
    assert m >= MARGIN, f"{tag}: the defect lands only {m:.2f}x outside the bound"


def _fwd_setup(name, dist, dtype, seed=0):
    """the inputs _run_gn_forward builds, on the CPU"""
    cs = T.GN_CASES[name]
    N, H, W, C0, C1, G = cs["N"], cs["H"], cs["W"], cs["C0"], cs.get("C1", 0), cs["G"]
    C = C0 + C1
    x = R.gn_input(N, H, W, C, G, dist, seed, dtype)
    gamma, beta, film = T._gn_params(cs, C, seed, "cpu")
    res = R.round_to(torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64), dtype) \
        if cs.get("res") else None
    return cs, x, gamma, beta, film, res


def _y_from_moments(x, G, mean, var, eps, gamma, beta, film, act, pool=False, res=None, film_plus_one=True):
    """act(((x - mean) / sqrt(var + eps)) gamma + beta [FiLM]) [pool] [+ res] with given per-(sample, group) moments [N, G]"""
    N, H, W, C = x.shape
    cpg = C // G
    m = mean.repeat_interleave(cpg, 1)[:, None, None, :]
    v = var.repeat_interleave(cpg, 1)[:, None, None, :]
    y = (x - m) / torch.sqrt(v.clamp_min(0) + eps)
    if gamma is not None:
        y = y * gamma.double() + beta.double()
    if film is not None:
        f = film.double()
        s = f[:, None, None, :C]
        y = y * ((1 + s) if film_plus_one else s) + f[:, None, None, C:2 * C]
    y = R.act_ref(y, act)
    if pool:
        y = y.reshape(N, H // 2, 2, W // 2, 2, C).mean((2, 4))
    return y + res if res is not None else y


def _moments(xg_sum, xg_sq, cnt):
    mean = xg_sum / cnt
    return mean, xg_sq / cnt - mean * mean


def _fwd_ref_tol(cs, x, gamma, beta, film, res, dtype):
    N, H, W, C = x.shape
    co = R.gn_coeffs_ref(x, cs["G"], cs.get("eps", 1e-5), gamma, beta, film, 2 * C + 8, depth=R.standalone_depth(N, H * W, C))
    return R.gn_apply_ref(x, co, cs["act"], cs.get("pool", False), res, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gn_forward_defect_margins(dtype):
    # count, chunk, straddle, FiLM: cat104_88 (cpg 6, group 17 straddles the sources at channel 104, FiLM, SiLU)
    cs, x, gamma, beta, film, res = _fwd_setup("cat104_88", "normal", dtype)
    N, H, W, C = x.shape
    G, eps, act, C0 = cs["G"], cs.get("eps", 1e-5), cs["act"], cs["C0"]
    cpg = C // G
    ref, tol = _fwd_ref_tol(cs, x, gamma, beta, film, res, dtype)
    xg = x.reshape(N, H * W, G, cpg)
    S1, S2 = xg.sum((1, 3)), (xg * xg).sum((1, 3))
    mean, var = _moments(S1, S2, H * W * cpg)
    y = lambda m, v, **k: _y_from_moments(x, G, m, v, eps, gamma, beta, film, act, **k)    # noqa: E731
    _margin(f"count HW instead of HW cpg {dtype}", y(*_moments(S1, S2, H * W)), ref, tol)
    nchunk = R.gn_nchunk(N, H * W)
    ppc = -(-H * W // nchunk)
    keep = xg[:, :(nchunk - 1) * ppc]
    _margin(f"last pixel chunk dropped {dtype}", y(*_moments(keep.sum((1, 3)), (keep * keep).sum((1, 3)), H * W * cpg)), ref, tol)
    xs = x.clone()
    g_st = C0 // cpg                                           # the group that straddles the boundary
    hi = (g_st + 1) * cpg
    xs[..., C0:hi] = x[..., C0 + 8:hi + 8]                     # its second-source channels read 8 channels off
    xsg = xs.reshape(N, H * W, G, cpg)
    _margin(f"straddling group reads the other source off by 8 {dtype}",
            y(*_moments(xsg.sum((1, 3)), (xsg * xsg).sum((1, 3)), H * W * cpg)), ref, tol)
    _margin(f"FiLM scale s instead of 1 + s {dtype}", y(mean, var, film_plus_one=False), ref, tol)

    # pool before the activation: adm128_pool
    cs, x, gamma, beta, film, res = _fwd_setup("adm128_pool", "normal", dtype)
    ref, tol = _fwd_ref_tol(cs, x, gamma, beta, film, res, dtype)
    N, H, W, C = x.shape
    xg = x.reshape(N, H * W, 32, C // 32)
    mean, var = _moments(xg.sum((1, 3)), (xg * xg).sum((1, 3)), xg[0, :, 0].numel())
    z = _y_from_moments(x, 32, mean, var, 1e-5, gamma, beta, None, R.ACT_NONE, pool=True)
    _margin(f"pool before the activation {dtype}", R.act_ref(z, cs["act"]), ref, tol)

    # eps: the var ~ eps group of the 'edge' distribution, eps 1e-6 asked (sd320_8) and 1e-5 (adm128_pool)
    for name, wrong in (("sd320_8", 1e-5), ("adm128_pool", 0.0), ("sd320_8", 0.0)):
        cs, x, gamma, beta, film, res = _fwd_setup(name, "edge", dtype, seed=11)
        ref, tol = _fwd_ref_tol(cs, x, gamma, beta, film, res, dtype)
        N, H, W, C = x.shape
        xg = x.reshape(N, H * W, 32, C // 32)
        mean, var = _moments(xg.sum((1, 3)), (xg * xg).sum((1, 3)), xg[0, :, 0].numel())
        d = _y_from_moments(x, 32, mean, var, wrong, gamma, beta, film, cs["act"], pool=cs.get("pool", False), res=res)
        if wrong == 0.0:
            d = torch.nan_to_num(d, nan=0.0)                   # the constant group divides 0 by 0: any finite answer is as wrong
        _margin(f"eps {wrong:g} instead of {cs.get('eps', 1e-5):g} ({name}) {dtype}", d, ref, tol)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gn_finalize_slice_dropped_margin(dtype):
    """vd256_32_b1: GroupNorm(1, 256) at 32x32 batch 1 takes S = 64 slices; drop the partial rows one slice walks"""
    cs, x, gamma, beta, film, res = _fwd_setup("vd256_32_b1", "normal", dtype)
    N, H, W, C = x.shape
    nchunk = R.gn_nchunk(N, H * W)
    S = R.finalize_slices(N, 1, C, nchunk)
    assert S == 64
    ref, tol = _fwd_ref_tol(cs, x, gamma, beta, film, res, dtype)
    ppc = -(-H * W // nchunk)
    xp = x.reshape(N, H * W, C)
    part = torch.stack([xp[:, i * ppc:(i + 1) * ppc].sum(1) for i in range(nchunk)], 1)           # [N, P, C] partial sums
    partq = torch.stack([(xp[:, i * ppc:(i + 1) * ppc] ** 2).sum(1) for i in range(nchunk)], 1)
    w2 = C // 2                                                 # the two-channel walk: item i = (row i // w2, channel pair i % w2)
    items = torch.arange(nchunk * w2)
    dropped = (items // 256) % S == 0                           # slice 0's items
    mask = torch.ones(nchunk, C, dtype=torch.float64)
    for i in items[dropped].tolist():
        mask[i // w2, 2 * (i % w2):2 * (i % w2) + 2] = 0
    S1, S2 = (part * mask).sum((1, 2))[:, None], (partq * mask).sum((1, 2))[:, None]
    mean, var = _moments(S1, S2, H * W * C)
    d = _y_from_moments(x, 1, mean, var, 1e-5, gamma, beta, film, cs["act"], res=res)
    _margin(f"one finalize slice's partial dropped {dtype}", d, ref, tol)


def _bwd_setup(name, dtype):
    cs = T.BWD_CASES[name]
    N, H, W, C0, C1 = cs["N"], cs["H"], cs["W"], cs["C0"], cs.get("C1", 0)
    C = C0 + C1
    x = R.gn_input(N, H, W, C, 32, "normal", 21, dtype)
    gamma, beta, film = T._gn_params(cs, C, 21, "cpu")
    g = torch.Generator().manual_seed(22)
    dy = R.rnd(torch.randn(N, H, W, C, generator=g, dtype=torch.float64), dtype)
    ga = R.rnd(torch.randn(N, H, W, C, generator=g, dtype=torch.float64), dtype)
    gadd = torch.zeros_like(ga)
    for src in cs.get("gadd", ()):
        sl = slice(0, C0) if src == 0 else slice(C0, C)
        gadd[..., sl] = ga[..., sl]
    eps = cs.get("eps", 1e-5)
    depth = R.standalone_depth(N, H * W, C)
    co = R.gn_coeffs_ref(x, 32, eps, gamma, beta, film, 2 * C + 8, depth=depth)
    ref, tol = R.gn_backward_ref(x, dy, 32, eps, gamma, beta, film, cs["act"], co, depth, R.gn_stats_depth(N, H * W, C),
                                 gadd=gadd if cs.get("gadd") else None, dtype=dtype)
    return cs, x, dy, ga, gadd, co, ref, tol


def _bwd_terms(x, dt, co, G=32):
    """r gamma' dt, r m1, r xhat m2 per element for a given dt (the pieces of dx = a dt - r m1 - r xhat m2)"""
    N, H, W, C = x.shape
    cpg = C // G
    gp = (co["gm"] * co["sc"])[:, None, None, :]
    r = co["r"][:, None, None, :]
    xg = x.reshape(N, H * W, G, cpg)
    mu = xg.mean((1, 3)).repeat_interleave(cpg, 1)[:, None, None, :]
    xh = (x - mu) * r
    gsum = lambda t: t.reshape(N, H * W, G, cpg).mean((1, 3)).repeat_interleave(cpg, 1)[:, None, None, :]    # noqa: E731
    m1, m2 = gsum(gp * dt), gsum(gp * dt * xh)
    return r * gp * dt, r * m1, r * xh * m2


@pytest.mark.parametrize("dtype", DTYPES)
def test_gn_backward_defect_margins(dtype):
    for name in ("c64_film_silu", "cat104_88_gadd2"):
        cs, x, dy, ga, gadd, co, ref, tol = _bwd_setup(name, dtype)
        a = co["a"][:, None, None, :]
        z = x * a + co["b"][:, None, None, :]
        t0, t1, t2 = _bwd_terms(x, dy * R.act_grad_ref(z, cs["act"]), co)
        assert R.defect_ratio(t0 - t1 - t2 + gadd, ref, tol) < 0.05          # the restatement is the reference
        _margin(f"backward without the m1 term ({name}) {dtype}", t0 - t2 + gadd, ref, tol)
        _margin(f"backward without the m2 term ({name}) {dtype}", t0 - t1 + gadd, ref, tol)
        d0, d1, d2 = _bwd_terms(x, dy * R.act_grad_ref(x, cs["act"]), co)
        _margin(f"backward with act' at x ({name}) {dtype}", d0 - d1 - d2 + gadd, ref, tol)
    cs, x, dy, ga, gadd, co, ref, tol = _bwd_setup("cat128_64_gadd0", dtype)
    wrong = torch.zeros_like(ga)
    wrong[..., cs["C0"]:] = ga[..., cs["C0"]:]
    _margin(f"gadd added to the wrong source {dtype}", ref - gadd + wrong, ref, tol)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", T.RS_SHAPES[:4] + [T.RS_SHAPES[5]], ids=str)
def test_resample_defect_margins(shape, dtype):
    N, H, W, C = shape
    x = R.round_to(torch.randn(*shape, generator=torch.Generator().manual_seed(H * W + C), dtype=torch.float64) * 1.5 + 0.3, dtype)
    ref, tol = R.bilinear_ref(x, dtype)
    _margin(f"bilinear border clamped to zero {shape} {dtype}", R.bilinear_ref(x, dtype, zero_border=True)[0], ref, tol)
    dy = R.round_to(torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(8 + C), dtype=torch.float64) * 1.5 + 0.3, dtype)
    ref, tol = R.avgpool_bwd_ref(dy, dtype)
    _margin(f"avgpool adjoint without its 0.25 {shape} {dtype}", R.avgpool_bwd_ref(dy, dtype, scale=1.0)[0], ref, tol)
    dy2 = R.round_to(torch.randn(N, 2 * H, 2 * W, C, generator=torch.Generator().manual_seed(9 + C), dtype=torch.float64), dtype)
    ref, tol = R.nearest_bwd_ref(dy2, dtype)
    _margin(f"nearest adjoint summing 2 taps {shape} {dtype}", R.nearest_bwd_ref(dy2, dtype, taps=2)[0], ref, tol)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", [n for n in T.GN_CASES if n not in ("vae128_512", "tiny1x1")])
def test_gn_bound_not_vacuous(name, dtype):
    """benign inputs: the forward bound is at most 4 u max|y| (tiny1x1 is not benign: two values per group, var can sit at eps)"""
    cs, x, gamma, beta, film, res = _fwd_setup(name, "normal", dtype)
    ref, tol = _fwd_ref_tol(cs, x, gamma, beta, film, res, dtype)
    r = float(tol.max() / (4 * R.U[dtype] * ref.abs().max()))
    print(f"[bound] {name} {dtype}: max tol / (4 u max|y|) = {r:.3f}")
    assert r <= 1.0


def test_finalize_slice_rule_restated():
    """the S rule of pmi_gn_finalize as _norm_ref64 restates it, at the shapes the issue names"""
    assert R.finalize_slices(1, 1, 256, R.gn_nchunk(1, 32 * 32)) == 64            # v-diffusion GroupNorm(1, 256) at 32^2
    assert R.finalize_slices(1, 1, 32, R.gn_nchunk(1, 128 * 128)) == 8            # any C >= 32 at 128^2 batch 1
    assert R.finalize_slices(2, 32, 256, R.gn_nchunk(2, 64 * 64)) == 1            # 32 groups: cpg * P too small
    assert R.finalize_slices(1, 8, 72, 4096) == 1                                 # odd cpg never slices
    for c in T.FIN_CASES:
        assert R.finalize_slices(c["N"], c["G"], c["C0"] + c.get("C1", 0), c["P0"], c.get("P1", 0)) == c["S"]


def test_every_kernel_is_covered():
    from perceptor_amd import _hip
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_norm_resample.py")).read()
    names = [n for n in _hip._PROTOS if re.search(r"pmi_(gn|avgpool|upsample|nchw|nhwc|timestep|fourier)", n)]
    assert len(names) >= 18
    missing = [n for n in names if not re.search(r"\b" + n + r"\b", src)]
    assert not missing, f"not exercised by tests/test_gpu_norm_resample.py: {missing}"
