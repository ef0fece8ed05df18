"""GPU: GroupNorm (forward, finalize, conv-epilogue statistics, backward, GroupNorm(1, C) backward), resampling, layout and
time-embedding kernels one at a time against float64 torch on the same rounded operands (bounds: tests/_norm_ref64.py).

Every call runs on NaN-filled outputs and scratch with a NaN guard past the logical end: outputs must come back finite, guards
untouched.  Two launches give the same bits; where the per-sample launch geometry does not depend on N (apply passes, gn1 backward,
resampling, embeddings) one sample run alone gives the same bits too.
"""
import contextlib
import math

import pytest
import torch
import torch.nn.functional as F

import _norm_ref64 as R

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
GUARD = 64


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


class _Guarded:
    """buffers that start as NaN with a NaN guard of GUARD elements after the logical end"""

    def __init__(self):
        self.bufs = []

    def __call__(self, shape, dtype, device):
        numel = math.prod(shape)
        buf = torch.full((numel + GUARD,), float("nan"), dtype=dtype, device=device)
        self.bufs.append((buf, numel))
        return buf[:numel].view(shape)

    def verify(self, tag, full=True):
        torch.cuda.synchronize()
        for buf, numel in self.bufs:
            assert torch.isnan(buf[numel:].float()).all(), f"{tag}: a kernel wrote past the end of a buffer"
            if full:
                assert torch.isfinite(buf[:numel].float()).all(), f"{tag}: output / scratch not fully written"


@contextlib.contextmanager
def _guarded_ops(tag):
    """route every ops-level allocation through _Guarded"""
    from perceptor_amd.engine import ops
    g = _Guarded()
    old = ops._empty
    ops._empty = g
    try:
        yield g
    finally:
        ops._empty = old
    g.verify(tag)


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype in (torch.float32, torch.float64) else t.contiguous().view(torch.int16)


def _same_bits(tag, a, b):
    assert torch.equal(_bits(a), _bits(b)), f"{tag}: results differ bitwise"


def _store(x64, dtype):
    """float64 NHWC -> the kernel's storage tensor on the device"""
    if dtype == "precise":
        return R.to_split16(x64.float()).contiguous()
    return x64.to(R.TD[dtype]).contiguous()


def _load(t, dtype):
    return R.from_split16(t) if dtype == "precise" else t.double()


def _dt(dtype):
    from perceptor_amd._hip import dtype_code
    return dtype_code(dtype)


# ---- 1. GroupNorm forward through ops --------------------------------------------------------------------------------------------------
GN_CASES = {
    "adm96": dict(N=2, H=16, W=16, C0=96, G=32, act=2, film=True),                 # cpg 3: odd, one-channel finalize walk
    "adm128_pool": dict(N=2, H=16, W=16, C0=128, G=32, act=2, pool=True),
    "adm256_res": dict(N=2, H=8, W=8, C0=256, G=32, act=0, res=True),
    "cat256_128": dict(N=2, H=16, W=16, C0=256, C1=128, G=32, act=2),
    "cat104_88": dict(N=2, H=16, W=16, C0=104, C1=88, G=32, act=2, film=True),     # cpg 6: group 17 straddles the boundary at 104
    "sd320_64": dict(N=1, H=64, W=64, C0=320, G=32, act=2, eps=1e-6),
    "sd640_320_64": dict(N=1, H=64, W=64, C0=640, C1=320, G=32, act=2, eps=1e-6),
    "sd1280_1280_8": dict(N=2, H=8, W=8, C0=1280, C1=1280, G=32, act=2, eps=1e-6),
    "sd320_8": dict(N=2, H=8, W=8, C0=320, G=32, act=2, eps=1e-6),
    "vae128_512": dict(N=1, H=512, W=512, C0=128, G=32, act=2, eps=1e-6),
    "vae512_128": dict(N=1, H=128, W=128, C0=512, G=32, act=2, eps=1e-6),
    "vd256_32_b1": dict(N=1, H=32, W=32, C0=256, G=1, act=1, film=True, res=True, affine=False),     # S = 64 finalize slices
    "vd128_128_b1": dict(N=1, H=128, W=128, C0=128, G=1, act=1, film=True, affine=False),
    "vd128_64_b2": dict(N=2, H=64, W=64, C0=128, G=1, act=1, film=True, res=True),
    "tiny1x1": dict(N=2, H=1, W=1, C0=64, G=32, act=2),
    "tiny2x2_pool": dict(N=2, H=2, W=2, C0=64, G=32, act=2, pool=True),
    "tiny7x5": dict(N=3, H=7, W=5, C0=96, G=32, act=1),
}
DIST_CASES = ["adm128_pool", "cat104_88", "vd256_32_b1", "sd320_8"]
DISTS = ["off4", "off16", "off64", "spread", "edge", "big"]
ACC_LIMIT = 16.0          # the standalone route meets the coefficient accuracy requirement for |mean| / std <= 16


def _gn_params(cs, C, seed, dev):
    g = torch.Generator().manual_seed(seed + 1)
    affine = cs.get("affine", True)
    gamma = (1 + 0.2 * torch.randn(C, generator=g)).to(dev) if affine else None
    beta = (0.2 * torch.randn(C, generator=g)).to(dev) if affine else None
    film = (0.3 * torch.randn(cs["N"], 2 * C + 8, generator=g)).to(dev) if cs.get("film") else None
    return gamma, beta, film


def _run_gn_forward(name, dist, dtype, seed=0):
    from perceptor_amd._hip import call, ptr
    from perceptor_amd.engine import ops
    dev = _dev()
    cs = GN_CASES[name]
    N, H, W, C0, C1, G = cs["N"], cs["H"], cs["W"], cs["C0"], cs.get("C1", 0), cs["G"]
    C, eps, act, pool = C0 + C1, cs.get("eps", 1e-5), cs["act"], cs.get("pool", False)
    x = R.gn_input(N, H, W, C, G, dist, seed, dtype, dev)
    gamma, beta, film = _gn_params(cs, C, seed, dev)
    film_ld = 2 * C + 8
    res = R.round_to(torch.randn(N, H, W, C, generator=torch.Generator().manual_seed(seed + 2), dtype=torch.float64), dtype).to(dev) \
        if cs.get("res") else None
    xs0 = _store(x[..., :C0], dtype)
    xs1 = _store(x[..., C0:], dtype) if C1 else None
    dt = _dt(dtype)
    kw = dict(x1=xs1, film=film, film_ld=film_ld, eps=eps)
    tag = f"gn {name} {dist} {dtype}"
    with _guarded_ops(tag):
        y = ops.group_norm(xs0, gamma, beta, G, dt, residual=_store(res, dtype) if res is not None else None, act=act, pool=pool, **kw)
        ca, cb = ops.group_norm_coeffs(xs0, gamma, beta, G, dt, **kw)
    y2 = ops.group_norm(xs0, gamma, beta, G, dt, residual=_store(res, dtype) if res is not None else None, act=act, pool=pool, **kw)
    _same_bits(tag + " repeat", y, y2)
    co = R.gn_coeffs_ref(x, G, eps, gamma, beta, film, film_ld, depth=R.standalone_depth(N, H * W, C))
    ra, rb = R.coeff_bound_ratio(ca, cb, co)
    R.parity(tag + " coef a", ra, 1.0)
    R.parity(tag + " coef b", rb, 1.0)
    assert ra <= 1 and rb <= 1, (ra, rb)
    if dtype != "precise":
        acc = R.coeff_accuracy(ca, cb, co, R.U[dtype], ACC_LIMIT)
        if acc is not None:
            R.parity(tag + " accuracy a (u/4)", acc[0], 1.0)
            R.parity(tag + " accuracy b (u/4)", acc[1], 1.0)
            assert max(acc) <= 1.0, f"{tag}: statistics cost more than a quarter of the output rounding: {acc}"
    yref, tol = R.gn_apply_ref(x, co, act, pool, res, dtype)
    R.echeck(tag, _load(y, dtype), yref, tol)
    # the apply pass alone on sample 0: its launch geometry per sample does not depend on N (the statistics' does)
    ys = torch.full_like(y[:1], float("nan"))
    call("pmi_gn_apply", ptr(xs0[:1]), ptr(xs1[:1] if xs1 is not None else None), C0, ptr(ca[:1].contiguous()), ptr(cb[:1].contiguous()),
         ptr(_store(res, dtype)[:1] if res is not None else None), ptr(ys), 1, H, W, C, act, int(pool), dt)
    _same_bits(tag + " one sample", ys, y[:1])
    return x, co


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(GN_CASES))
def test_gn_forward_shapes(name, dtype):
    _run_gn_forward(name, "normal", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dist", DISTS)
@pytest.mark.parametrize("name", DIST_CASES)
def test_gn_forward_distributions(name, dist, dtype):
    _run_gn_forward(name, dist, dtype, seed=11)


@pytest.mark.parametrize("name,dist", [("adm128_pool", "normal"), ("cat256_128", "normal"), ("vd256_32_b1", "normal"), ("sd320_8", "off16"),
                                       ("adm256_res", "normal")])
def test_gn_forward_precise(name, dist):
    _run_gn_forward(name, dist, "precise", seed=5)


@pytest.mark.parametrize("dtype", DTYPES + ["precise"])
@pytest.mark.parametrize("case", [dict(N=2, H=16, W=16, C=128, act=2, dist="normal"), dict(N=1, H=64, W=32, C=256, act=0, dist="off4"),
                                  dict(N=2, H=2, W=2, C=64, act=2, dist="normal"), dict(N=2, H=8, W=8, C=64, act=0, dist="tiny")])
def test_gn_pool_skip(case, dtype):
    """pmi_gn_apply_pool_skip: y = AvgPool2d(2)(act(GN(x))) and y_raw = AvgPool2d(2)(x) from one pass ('tiny': values near 1e-4)."""
    from perceptor_amd.engine import ops
    dev = _dev()
    N, H, W, C, act = case["N"], case["H"], case["W"], case["C"], case["act"]
    if case["dist"] == "tiny":
        g = torch.Generator().manual_seed(3)
        x = R.round_to(1e-4 * (1 + 0.5 * torch.randn(N, H, W, C, generator=g, dtype=torch.float64)), dtype).to(dev)
    else:
        x = R.gn_input(N, H, W, C, 32, case["dist"], 3, dtype, dev)
    gamma, beta, _ = _gn_params(dict(N=N), C, 3, dev)
    xs = _store(x, dtype)
    tag = f"gn pool_skip {N}x{H}x{W}x{C} {case['dist']} {dtype}"
    with _guarded_ops(tag):
        y, y_raw = ops.group_norm_pool_skip(xs, gamma, beta, 32, _dt(dtype), act=act)
    y2, y_raw2 = ops.group_norm_pool_skip(xs, gamma, beta, 32, _dt(dtype), act=act)
    _same_bits(tag + " repeat", torch.cat([y, y_raw]), torch.cat([y2, y_raw2]))
    co = R.gn_coeffs_ref(x, 32, 1e-5, gamma, beta, depth=R.standalone_depth(N, H * W, C))
    yref, tol = R.gn_apply_ref(x, co, act, True, None, dtype)
    R.echeck(tag + " y", _load(y, dtype), yref, tol)
    rref, rtol = R.avgpool_ref(x, dtype)
    R.echeck(tag + " y_raw", _load(y_raw, dtype), rref, rtol)


# ---- 2. pmi_gn_finalize on synthetic partials -------------------------------------------------------------------------------------------
FIN_CASES = [
    dict(N=1, G=1, C0=256, P0=128, S=64),
    dict(N=1, G=8, C0=256, P0=1024, S=8),
    dict(N=1, G=8, C0=64, P0=4096, S=2),
    dict(N=1, G=8, C0=72, P0=4096, S=1),                  # cpg 9: odd, never sliced
    dict(N=2, G=32, C0=256, P0=64, S=1),
    dict(N=1, G=16, C0=64, P0=4096, C1=64, P1=1024, S=2),  # two sources, different P
    dict(N=1, G=16, C0=60, P0=4096, C1=68, P1=512, S=2),   # a group straddles the sources (C0 not a multiple of cpg)
    dict(N=1, G=16, C0=61, P0=2048, C1=83, P1=4096, S=1),  # cpg 9, odd source widths
]


def _int_partials(N, P, C, g):
    """fp32 partials whose every sum is an exact integer: s = k, q = k^2 + m (k in [-8, 8], m in [0, 16])"""
    k = torch.randint(-8, 9, (N, P, C), generator=g).double()
    m = torch.randint(0, 17, (N, P, C), generator=g).double()
    return torch.stack([k, k * k + m], -1)


def _halve_rows(p):
    """the same statistics in half the rows (adjacent rows added: still exact), so the slice rule picks S = 1"""
    N, P, C, _ = p.shape
    return p.reshape(N, P // 2, 2, C, 2).sum(2)


@pytest.mark.parametrize("case", FIN_CASES, ids=lambda c: f"N{c['N']}G{c['G']}C{c['C0']}+{c.get('C1', 0)}S{c['S']}")
def test_gn_finalize_slices(case):
    from perceptor_amd._hip import call, ptr
    dev = _dev()
    N, G, C0, P0, C1, P1 = case["N"], case["G"], case["C0"], case["P0"], case.get("C1", 0), case.get("P1", 0)
    C, cpg = C0 + C1, (C0 + C1) // G
    S = R.finalize_slices(N, G, C, P0, P1)
    assert S == case["S"], f"the slice rule gives S = {S}"
    g = torch.Generator().manual_seed(C + P0)
    p0 = _int_partials(N, P0, C0, g)
    p1 = _int_partials(N, P1, C1, g) if C1 else None
    HW = max(P0, P1)                        # one pixel per partial row of the longer source (the count only scales the moments)
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    film = 0.3 * torch.randn(N, 2 * C, generator=g)
    tot = torch.cat([p0.sum(1), p1.sum(1)], 1) if C1 else p0.sum(1)        # [N, C, 2], exact
    S1 = tot[..., 0].reshape(N, G, cpg).sum(-1)
    S2 = tot[..., 1].reshape(N, G, cpg).sum(-1)
    co = R.coeffs_from_sums(S1, S2, float(HW * cpg), cpg, 1e-5, gamma, beta, film)
    gd, bd, fd = gamma.to(dev), beta.to(dev), film.to(dev)
    outs = []
    for rows_halved in (False, True):
        if rows_halved and S == 1:
            continue
        q0 = _halve_rows(p0) if rows_halved else p0
        q1 = (_halve_rows(p1) if rows_halved else p1) if C1 else None
        if rows_halved:
            assert R.finalize_slices(N, G, C, q0.shape[1], q1.shape[1] if C1 else 0) == 1
        g_ = _Guarded()
        ca, cb = g_((N, C), torch.float32, dev), g_((N, C), torch.float32, dev)
        s0 = q0.float().to(dev).contiguous()
        s1 = q1.float().to(dev).contiguous() if C1 else None
        call("pmi_gn_finalize", ptr(s0), s0.shape[1], C0, ptr(s1), s1.shape[1] if C1 else 0, C1, ptr(gd), ptr(bd), ptr(fd), 2 * C,
             ptr(ca), ptr(cb), N, HW, G, 1e-5)
        tag = f"finalize N{N} G{G} C{C0}+{C1} S{1 if rows_halved else S}"
        g_.verify(tag)                      # includes the coef_b slots the S > 1 path borrows: fully overwritten
        R.echeck(tag + " a", ca, co["a"], R.C_B * co["da"])
        R.echeck(tag + " b", cb, co["b"], R.C_B * co["db"])
        outs.append((ca.clone(), cb.clone()))
    if len(outs) == 2:        # exact sums: the sliced and unsliced combinations agree to the bit
        _same_bits(f"finalize S{S} vs S1", torch.cat(outs[0]), torch.cat(outs[1]))


# ---- 3. statistics from the conv epilogue ------------------------------------------------------------------------------------------------
FUSED_CASES = [
    dict(N=2, H=16, W=32, cin=64, cout=256, G=32, force_cfg=0, dist="normal"),
    dict(N=2, H=16, W=64, cin=64, cout=256, G=32, force_cfg=6, dist="off4"),
    dict(N=2, H=8, W=16, cin=64, cout=64, G=32, k=1, dist="off4"),              # generic kernel, hw % BM == 0 rows
    dict(N=2, H=16, W=32, cin=64, cout=256, G=32, force_cfg=0, dist="normal", cat=64),     # two producers, group 25 straddles
    dict(N=1, H=256, W=128, cin=64, cout=256, G=1, force_cfg=0, dist="normal"),  # N G < 128, 128 stats rows: S = 64 slices
    dict(N=2, H=16, W=32, cin=64, cout=256, G=32, force_cfg=0, dist="off16"),
]


def _conv_ref(x64, w64, b):
    """float64 conv on NHWC x and the fp32 accumulation bound of the kernel's output"""
    xc = x64.permute(0, 3, 1, 2)
    k = w64.shape[-1]
    y = F.conv2d(xc, w64, b.double(), padding=k // 2)
    ya = F.conv2d(xc.abs(), w64.abs(), b.double().abs(), padding=k // 2)
    K = w64.shape[1] * k * k
    return y.permute(0, 2, 3, 1), ((K + 2) * R.E32 * ya).permute(0, 2, 3, 1)


def _fused_input(case, dtype, g, dev):
    N, H, W, cin = case["N"], case["H"], case["W"], case["cin"]
    x = R.rnd(torch.randn(N, H, W, cin, generator=g, dtype=torch.float64), dtype)
    return x.to(dev)


def _fused_lin(cin, cout, k, dist, dtype, g, dev):
    from perceptor_amd.engine import ops
    w = R.rnd(torch.randn(cout, cin, k, k, generator=g, dtype=torch.float64) / (cin * k * k) ** 0.5, dtype)
    off = {"normal": 0.3, "off4": 4.0, "off16": 16.0}[dist]
    b = torch.full((cout,), off) + 0.1 * torch.randn(cout, generator=g)        # |group mean| / std ~ off: the conv output has std ~ 1
    return ops.PackedLinear(w.float(), b, _dt(dtype), dev), w.to(dev), b.to(dev)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", FUSED_CASES, ids=lambda c: f"{c['H']}x{c['W']}x{c['cout']}G{c['G']}cfg{c.get('force_cfg', 'g')}{'cat' if 'cat' in c else ''}{c['dist']}")
def test_gn_fused_statistics(case, dtype):
    """ops.igemm(want_stats=True) -> pmi_gn_finalize: coefficients against float64 statistics of the float64 conv on the same rounded
    operands.  Bound: the conv's fp32 accumulation, the 16-bit rounding the statistics may see, and the statistics runs."""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    dev = _dev()
    g = torch.Generator().manual_seed(case["H"] * 7 + case["cout"])
    N, H, W, cin, cout, G, k = case["N"], case["H"], case["W"], case["cin"], case["cout"], case["G"], case.get("k", 3)
    x = _fused_input(case, dtype, g, dev)
    lin, w, b = _fused_lin(cin, cout, k, case["dist"], dtype, g, dev)
    xs = x.to(R.TD[dtype])
    _hip.lib().pmi_set_option(1, case.get("force_cfg", -1))
    try:
        y = ops.igemm(xs, lin, want_stats=True)
    finally:
        _hip.lib().pmi_set_option(1, -1)
    assert hasattr(y, "_pmi_stats"), "the route took no statistics epilogue"
    rows = y._pmi_stats[1]
    y64, acc = _conv_ref(x, w, b)
    C = cout
    x1 = None
    if "cat" in case:
        lin2, w2, b2 = _fused_lin(cin, case["cat"], k, case["dist"], dtype, g, dev)
        x1 = ops.igemm(xs, lin2, want_stats=True)
        assert hasattr(x1, "_pmi_stats")
        rows = min(rows, x1._pmi_stats[1])             # the two producers may take different tile configs: P0 != P1
        y642, acc2 = _conv_ref(x, w2, b2)
        y64, acc = torch.cat([y64, y642], -1), torch.cat([acc, acc2], -1)
        C += case["cat"]
    gamma, beta, film = _gn_params(dict(N=N, film=True), C, 9, dev)
    u = R.U[dtype]
    pert = acc + u * (y64.abs() + acc)             # statistics of the fp32 values, or of the stored 16-bit ones
    co = R.gn_coeffs_ref(y64, G, 1e-5, gamma, beta, film, 2 * C + 8, depth=R.fused_depth(H * W, rows), pert=pert)
    tag = f"fused stats {H}x{W}x{C} G{G} rows {rows} {case['dist']} {dtype}"
    with _guarded_ops(tag):
        ca, cb = ops.group_norm_coeffs(y, gamma, beta, G, _dt(dtype), x1=x1, film=film, film_ld=2 * C + 8)
    ca2, cb2 = ops.group_norm_coeffs(y, gamma, beta, G, _dt(dtype), x1=x1, film=film, film_ld=2 * C + 8)
    _same_bits(tag + " repeat", torch.cat([ca, cb]), torch.cat([ca2, cb2]))
    ra, rb = R.coeff_bound_ratio(ca, cb, co)
    R.parity(tag + " coef a", ra, 1.0)
    R.parity(tag + " coef b", rb, 1.0)
    assert ra <= 1 and rb <= 1, (ra, rb)
    if case["dist"] != "off16":    # the fused route's accuracy requirement covers |mean| / std <= 4
        acc_r = R.coeff_accuracy(ca, cb, co, u, 4.0)
        if acc_r is not None:
            R.parity(tag + " accuracy a (u/4)", acc_r[0], 1.0)
            R.parity(tag + " accuracy b (u/4)", acc_r[1], 1.0)
            assert max(acc_r) <= 1.0, acc_r
    else:
        acc_r = R.coeff_accuracy(ca, cb, co, u, 1e9)
        print(f"[info] {tag}: accuracy ratio at |mean|/std ~ 16: a {acc_r[0]:.3f} b {acc_r[1]:.3f}")


# ---- 4. GroupNorm backward -------------------------------------------------------------------------------------------------------------
BWD_CASES = {
    "c64_film_silu": dict(N=2, H=16, W=16, C0=64, act=2, film=True),
    "c96_none": dict(N=2, H=12, W=16, C0=96, act=0),
    "cat104_88_gadd2": dict(N=2, H=16, W=16, C0=104, C1=88, act=2, film=True, gadd=(0, 1)),
    "cat128_64_gadd0": dict(N=2, H=8, W=8, C0=128, C1=64, act=0, gadd=(0,)),
    "cat128_64_gadd1": dict(N=1, H=8, W=8, C0=128, C1=64, act=2, gadd=(1,), eps=1e-6),
    "sd320_32": dict(N=1, H=32, W=32, C0=320, act=2, eps=1e-6),
    "sd640_320_16": dict(N=2, H=16, W=16, C0=640, C1=320, act=2, film=True, eps=1e-6),
}
BWD_DISTS = ["normal", "off4", "off16", "spread", "edge"]


def _run_gn_backward(name, dist, dtype):
    from perceptor_amd._hip import call, ptr
    from perceptor_amd.engine import ops
    dev = _dev()
    cs = BWD_CASES[name]
    N, H, W, C0, C1 = cs["N"], cs["H"], cs["W"], cs["C0"], cs.get("C1", 0)
    C, G, eps, act = C0 + C1, 32, cs.get("eps", 1e-5), cs["act"]
    x = R.gn_input(N, H, W, C, G, dist, 21, dtype, dev)
    gamma, beta, film = _gn_params(cs, C, 21, dev)
    film_ld = 2 * C + 8
    g = torch.Generator().manual_seed(22)
    dy = R.rnd(torch.randn(N, H, W, C, generator=g, dtype=torch.float64), dtype).to(dev)
    gadd = torch.zeros(N, H, W, C, dtype=torch.float64, device=dev)
    ga = R.rnd(torch.randn(N, H, W, C, generator=g, dtype=torch.float64), dtype).to(dev)
    for src in cs.get("gadd", ()):
        sl = slice(0, C0) if src == 0 else slice(C0, C)
        gadd[..., sl] = ga[..., sl]
    td = R.TD[dtype]
    xs0, xs1 = x[..., :C0].to(td).contiguous(), (x[..., C0:].to(td).contiguous() if C1 else None)
    g0 = gadd[..., :C0].to(td).contiguous() if 0 in cs.get("gadd", ()) else None
    g1 = gadd[..., C0:].to(td).contiguous() if 1 in cs.get("gadd", ()) else None
    dys = dy.to(td).contiguous()
    dt = _dt(dtype)
    tag = f"gn bwd {name} {dist} {dtype}"
    kw = dict(x1=xs1, film=film, film_ld=film_ld, eps=eps)
    with _guarded_ops(tag + " coeffs"):
        ca, cb, parts = ops.group_norm_coeffs_train(xs0, gamma, beta, G, dt, **kw)
    depth = R.standalone_depth(N, H * W, C)
    co = R.gn_coeffs_ref(x, G, eps, gamma, beta, film, film_ld, depth=depth)
    dx_ref, tol = R.gn_backward_ref(x, dy, G, eps, gamma, beta, film, act, co, depth, R.gn_stats_depth(N, H * W, C),
                                    gadd=gadd if cs.get("gadd") else None, dtype=dtype)
    # the three passes by hand on guarded buffers (the same calls as ops.group_norm_backward), then ops itself for the same bits
    nchunk = R.gn_nchunk(N, H * W)
    gd = _Guarded()
    wsb = gd((N, nchunk, C, 2), torch.float32, dev)
    cp, cq = gd((N, C), torch.float32, dev), gd((N, C), torch.float32, dev)
    dx0, dx1 = gd(xs0.shape, td, dev), (gd(xs1.shape, td, dev) if C1 else None)
    call("pmi_gn_bwd_stats", ptr(xs0), ptr(xs1), C0, ptr(dys), ptr(ca), ptr(cb), act, ptr(wsb), N, H * W, C, nchunk, dt)
    call("pmi_gn_bwd_finalize", ptr(parts[0]), parts[1], parts[2], ptr(parts[3]), parts[4], parts[5], ptr(wsb), nchunk, ptr(gamma), ptr(film),
         film_ld, ptr(cp), ptr(cq), N, H * W, G, eps)
    call("pmi_gn_bwd_apply", ptr(xs0), ptr(xs1), C0, ptr(dys), ptr(ca), ptr(cb), ptr(cp), ptr(cq), act, ptr(g0), ptr(g1), ptr(dx0), ptr(dx1),
         N, H * W, C, dt)
    gd.verify(tag)
    got = torch.cat([dx0, dx1], -1) if C1 else dx0
    R.echeck(tag, got.double(), dx_ref, tol)
    o0, o1 = ops.group_norm_backward(xs0, dys, ca, cb, parts, gamma, G, dt, x1=xs1, film=film, film_ld=film_ld, act=act, gadd0=g0, gadd1=g1,
                                     eps=eps)
    _same_bits(tag + " ops / repeat", got, torch.cat([o0, o1], -1) if C1 else o0)
    # the apply pass alone on sample 0 (its geometry per sample does not depend on N; the stats / finalize passes' does)
    s0, s1 = torch.full_like(dx0[:1], float("nan")), (torch.full_like(dx1[:1], float("nan")) if C1 else None)
    call("pmi_gn_bwd_apply", ptr(xs0[:1]), ptr(xs1[:1] if C1 else None), C0, ptr(dys[:1]), ptr(ca[:1]), ptr(cb[:1]), ptr(cp[:1]), ptr(cq[:1]), act,
         ptr(g0[:1] if g0 is not None else None), ptr(g1[:1] if g1 is not None else None), ptr(s0), ptr(s1), 1, H * W, C, dt)
    _same_bits(tag + " one sample", torch.cat([s0, s1], -1) if C1 else s0, got[:1])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(BWD_CASES))
def test_gn_backward_shapes(name, dtype):
    _run_gn_backward(name, "normal", dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("dist", BWD_DISTS[1:])
@pytest.mark.parametrize("name", ["c64_film_silu", "cat104_88_gadd2"])
def test_gn_backward_distributions(name, dist, dtype):
    _run_gn_backward(name, dist, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [dict(cfg=0, cat=0), dict(cfg=0, cat=64)])
def test_gn_backward_fused_parts(case, dtype):
    """group_norm_coeffs_train on conv-epilogue partials (the parts tuple the forward of a training step hands the backward)"""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    dev = _dev()
    g = torch.Generator().manual_seed(31)
    N, H, W, cin, cout = 2, 16, 32, 64, 256
    x = R.rnd(torch.randn(N, H, W, cin, generator=g, dtype=torch.float64), dtype).to(dev)
    lin, _, _ = _fused_lin(cin, cout, 3, "normal", dtype, g, dev)
    lin2, _, _ = _fused_lin(cin, 64, 3, "normal", dtype, g, dev)
    xs = x.to(R.TD[dtype])
    _hip.lib().pmi_set_option(1, case["cfg"])
    try:
        y = ops.igemm(xs, lin, want_stats=True)
        y1 = ops.igemm(xs, lin2, want_stats=True) if case["cat"] else None
    finally:
        _hip.lib().pmi_set_option(1, -1)
    assert hasattr(y, "_pmi_stats")
    rows = y._pmi_stats[1]
    yv = torch.cat([y, y1], -1).double() if y1 is not None else y.double()      # the stored operand the backward differentiates at
    C = yv.shape[-1]
    gamma, beta, film = _gn_params(dict(N=N, film=True), C, 31, dev)
    dy = R.rnd(torch.randn(N, H, W, C, generator=g, dtype=torch.float64), dtype).to(dev)
    ca, cb, parts = ops.group_norm_coeffs_train(y, gamma, beta, 32, _dt(dtype), x1=y1, film=film, film_ld=2 * C + 8)
    assert parts[1] == rows
    # the partials are statistics of the un-rounded conv outputs: within u |y| of the stored operand per element
    pert = R.U[dtype] * yv.abs() * (1 + R.U[dtype])
    depth = R.fused_depth(H * W, rows)
    co = R.gn_coeffs_ref(yv, 32, 1e-5, gamma, beta, film, 2 * C + 8, depth=depth, pert=pert)
    dx_ref, tol = R.gn_backward_ref(yv, dy, 32, 1e-5, gamma, beta, film, 2, co, depth, R.gn_stats_depth(N, H * W, C), dtype=dtype)
    d0, d1 = ops.group_norm_backward(y, dy.to(R.TD[dtype]).contiguous(), ca, cb, parts, gamma, 32, _dt(dtype), x1=y1, film=film, film_ld=2 * C + 8, act=2)
    got = torch.cat([d0, d1], -1) if y1 is not None else d0
    R.echeck(f"gn bwd fused parts rows {rows} cat {case['cat']} {dtype}", got.double(), dx_ref, tol)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [dict(N=2, hw=128 * 128, C=256, ld=0, add=0.0, res=False), dict(N=2, hw=128 * 128, C=256, ld=512, add=1.0, res=True),
                                  dict(N=2, hw=64, C=64, ld=0, add=0.0, res=True), dict(N=1, hw=64, C=64, ld=128, add=1.0, res=False),
                                  dict(N=2, hw=32 * 32, C=128, ld=256, add=1.0, res=False, dist="off16")])
def test_gn1_backward(case, dtype):
    """pmi_gn1_bwd: GroupNorm(1, C) backward, shared affine weight (gamma_ld 0) or FiLM scale (gamma_ld > 0, gamma_add 1), residual"""
    from perceptor_amd._hip import call, lib, ptr
    dev = _dev()
    N, hw, C, ld, gadd = case["N"], case["hw"], case["C"], case["ld"], case["add"]
    P = lib().pmi_gn1_bwd_partials(hw, C)
    assert P == max(1, min(256, hw * (C // 8) // 4096))
    g = torch.Generator().manual_seed(hw + C)
    x = R.gn_input(N, 1, hw, C, 1, case.get("dist", "normal"), hw + C, dtype).reshape(N, hw, C).to(dev)
    dy = R.rnd(torch.randn(N, hw, C, generator=g, dtype=torch.float64), dtype).to(dev)
    res = R.rnd(torch.randn(N, hw, C, generator=g, dtype=torch.float64), dtype).to(dev) if case["res"] else None
    gam = (0.3 * torch.randn(max(N * ld, C), generator=g)).float() + (1.0 - gadd)
    gamma_nc = (gam[:C][None].expand(N, C) if ld == 0 else gam[:N * ld].reshape(N, ld)[:, :C]).double() + gadd
    td = R.TD[dtype]
    xs, dys = x.to(td).contiguous(), dy.to(td).contiguous()
    rs = res.to(td).contiguous() if res is not None else None
    gd = gam.to(dev)
    dx_ref, tol = R.gn1_backward_ref(x, dy, gamma_nc, 1e-5, res, dtype)
    tag = f"gn1 bwd N{N} hw{hw} C{C} P{P} ld{ld} {dtype}"
    outs = []
    for rep in range(2):
        gbuf = _Guarded()
        part = gbuf((N * P * 4,), torch.float64, dev)
        dx = gbuf((N, hw, C), td, dev)
        call("pmi_gn1_bwd", ptr(xs), ptr(dys), ptr(gd), ld, gadd, ptr(rs), ptr(dx), ptr(part), N, hw, C, 1e-5, _dt(dtype))
        gbuf.verify(tag)
        outs.append(dx)
    R.echeck(tag, outs[0].double(), dx_ref, tol)
    _same_bits(tag + " repeat", outs[0], outs[1])
    part1 = torch.full((P * 4,), float("nan"), dtype=torch.float64, device=dev)
    dx1 = torch.full((1, hw, C), float("nan"), dtype=td, device=dev)
    call("pmi_gn1_bwd", ptr(xs[:1]), ptr(dys[:1]), ptr(gd), ld, gadd, ptr(rs[:1] if rs is not None else None), ptr(dx1), ptr(part1), 1, hw, C,
         1e-5, _dt(dtype))
    _same_bits(tag + " one sample", dx1, outs[0][:1])


# ---- 5. resampling -------------------------------------------------------------------------------------------------------------------------
RS_SHAPES = [(2, 6, 10, 8), (1, 5, 7, 24), (2, 16, 16, 320), (1, 4, 4, 2560), (1, 1, 1, 64), (2, 1, 9, 16)]
BIG = {"avgpool2": (1, 512, 512, 320), "up": (1, 128, 128, 320)}      # > 8192 * 256 output items: the grid-stride loops run


def _rs_input(shape, dtype, seed, dev, tiny=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(*shape, generator=g, dtype=torch.float64) * 1.5 + 0.3
    if tiny:
        x = 1e-4 * x
    return R.round_to(x, dtype).to(dev)


def _resample(name, xs, dtype):
    """pmi_avgpool2, pmi_upsample_bilinear2 and pmi_upsample_nearest2 through their ops wrappers"""
    from perceptor_amd.engine import ops
    if name == "avgpool2":
        return ops.avgpool2(xs, _dt(dtype))
    if name == "bilinear":
        return ops.upsample_bilinear2(xs, _dt(dtype))
    return ops.upsample_nearest2(xs)


def _resample_case(name, shape, dtype, tiny=False):
    dev = _dev()
    N, H, W, C = shape
    x = _rs_input(shape, dtype, H * W + C, dev, tiny)
    xs = _store(x, dtype)
    tag = f"{name} {'x'.join(map(str, shape))} {dtype}{' tiny' if tiny else ''}"
    with _guarded_ops(tag):
        y = _resample(name, xs, dtype)
    _same_bits(tag + " repeat", y, _resample(name, xs, dtype))
    _same_bits(tag + " one sample", _resample(name, xs[:1].contiguous(), dtype), y[:1])
    if name == "avgpool2":
        ref, tol = R.avgpool_ref(x, dtype)
    elif name == "bilinear":
        ref, tol = R.bilinear_ref(x, dtype)
    else:
        assert torch.equal(_bits(y), _bits(R.nearest_ref(xs.double()).to(xs.dtype))), f"{tag}: not an exact copy"
        R.parity(tag + " (bitwise)", 0.0, 0.0)
        return
    R.echeck(tag, _load(y, dtype), ref, tol)


@pytest.mark.parametrize("dtype", DTYPES + ["precise"])
@pytest.mark.parametrize("shape", RS_SHAPES + [BIG["up"]], ids=str)
def test_upsample_bilinear_forward(shape, dtype):
    _resample_case("bilinear", shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES)          # (nearest copies 16-byte words: it has no precise variant)
@pytest.mark.parametrize("shape", RS_SHAPES + [BIG["up"]], ids=str)
def test_upsample_nearest_forward(shape, dtype):
    _resample_case("nearest", shape, dtype)


@pytest.mark.parametrize("dtype", DTYPES + ["precise"])
@pytest.mark.parametrize("shape", [(2, 6, 10, 8), (1, 4, 8, 24), (2, 16, 16, 320), (1, 4, 4, 2560), BIG["avgpool2"]], ids=str)
def test_avgpool2_forward(shape, dtype):
    _resample_case("avgpool2", shape, dtype)


def test_avgpool2_precise_tiny():
    _resample_case("avgpool2", (2, 8, 8, 64), "precise", tiny=True)
    _resample_case("bilinear", (2, 5, 7, 64), "precise", tiny=True)


def _adjoint(name, dy, dtype):
    from perceptor_amd._hip import call, ptr
    N, Ho, Wo, C = dy.shape
    H, W = (Ho * 2, Wo * 2) if name == "avgpool2" else (Ho // 2, Wo // 2)
    dx = torch.full((N, H, W, C), float("nan"), dtype=dy.dtype, device=dy.device)
    kern = {"avgpool2": "pmi_avgpool2_bwd", "bilinear": "pmi_upsample_bilinear2_bwd", "nearest": "pmi_upsample_nearest2_bwd"}[name]
    call(kern, ptr(dy), ptr(dx), N, H, W, C, _dt(dtype))
    return dx


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", [(2, 6, 10, 8), (1, 5, 7, 24), (2, 16, 16, 320), (1, 4, 4, 2560), (1, 1, 1, 64), (2, 1, 9, 16), (1, 128, 128, 320)],
                         ids=str)
@pytest.mark.parametrize("name", ["avgpool2", "bilinear", "nearest"])
def test_resample_adjoints(name, shape, dtype):
    """the _bwd kernels against float64 adjoints, and <A x, dy> = <x, A^T dy> on the kernels' own outputs within the sum of the bounds"""
    dev = _dev()
    N, H, W, C = shape
    if name == "avgpool2":
        H, W = 2 * H, 2 * W                # the pooling input: always even
    x = _rs_input((N, H, W, C), dtype, 7 + C, dev)
    xs = _store(x, dtype)
    y = _resample(name, xs, dtype)
    dy = _rs_input(tuple(y.shape), dtype, 8 + C, dev)
    dys = _store(dy, dtype)
    tag = f"{name}_bwd {N}x{H}x{W}x{C} {dtype}"
    dx = _adjoint(name, dys, dtype)
    _same_bits(tag + " repeat", dx, _adjoint(name, dys, dtype))
    _same_bits(tag + " one sample", _adjoint(name, dys[:1].contiguous(), dtype), dx[:1])
    if name == "avgpool2":
        ref, tol = R.avgpool_bwd_ref(dy, dtype)
        _, tol_f = R.avgpool_ref(x, dtype)
    elif name == "bilinear":
        ref, tol = R.bilinear_bwd_ref(dy, dtype, H, W)
        _, tol_f = R.bilinear_ref(x, dtype)
    else:
        ref, tol = R.nearest_bwd_ref(dy, dtype)
        tol_f = torch.zeros_like(dy)
    R.echeck(tag, dx.double(), ref, tol)
    lhs = float((y.double() * dy).sum())
    rhs = float((x * dx.double()).sum())
    bound = float((dy.abs() * tol_f).sum() + (x.abs() * tol).sum())
    R.parity(tag + " adjoint identity", abs(lhs - rhs), bound)
    assert abs(lhs - rhs) <= bound


# ---- 6. layout and embeddings ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES + ["precise"])
@pytest.mark.parametrize("case", [dict(N=2, C=3, H=5, W=7, Cpad=8, mul=2.0, add=-1.0), dict(N=1, C=4, H=8, W=8, Cpad=32, mul=1 / 0.18215, add=0.0),
                                  dict(N=1, C=3, H=512, W=512, Cpad=16, mul=2.0, add=-1.0)], ids=lambda c: f"{c['C']}to{c['Cpad']}_{c['H']}")
def test_nchw_to_nhwc(case, dtype):
    from perceptor_amd._hip import call, ptr
    dev = _dev()
    N, C, H, W, Cpad, mul, add = (case[k] for k in ("N", "C", "H", "W", "Cpad", "mul", "add"))
    g = torch.Generator().manual_seed(C * H)
    inp = torch.rand(N, C, H, W, generator=g).to(dev)
    phys = 2 * Cpad if dtype == "precise" else Cpad
    tag = f"nchw_to_nhwc {N}x{C}x{H}x{W} pad {Cpad} {dtype}"
    outs = []
    for _ in range(2):
        gb = _Guarded()
        x = gb((N, H, W, phys), torch.float16 if dtype != "bf16" else torch.bfloat16, dev)
        call("pmi_nchw_to_nhwc", ptr(inp), ptr(x), N, C, H, W, Cpad, mul, add, _dt(dtype))
        gb.verify(tag)
        outs.append(x)
    _same_bits(tag + " repeat", outs[0], outs[1])
    got = _load(outs[0], dtype)
    ref = inp.double().permute(0, 2, 3, 1) * mul + add
    tol = R.C_B * (2 * R.E32 * ((inp.double().permute(0, 2, 3, 1) * mul).abs() + abs(add)) + R.out_round(ref, dtype))
    R.echeck(tag, got[..., :C], ref, tol)
    assert bool((got[..., C:] == 0).all()), f"{tag}: pad channels not exactly zero"


@pytest.mark.parametrize("case", [dict(N=2, H=5, W=7, ld=8, cout=3, mul=0.5, add=0.5), dict(N=1, H=64, W=64, ld=16, cout=4, mul=5.4899, add=0.0),
                                  dict(N=1, H=1024, W=1024, ld=8, cout=3, mul=0.5, add=0.5)], ids=lambda c: f"{c['H']}ld{c['ld']}")
def test_nhwc_to_nchw(case):
    from perceptor_amd._hip import call, ptr
    dev = _dev()
    N, H, W, ld, cout, mul, add = (case[k] for k in ("N", "H", "W", "ld", "cout", "mul", "add"))
    g = torch.Generator().manual_seed(H + ld)
    y = torch.randn(N, H, W, ld, generator=g)
    y[..., cout:] = float("nan")                  # channels past cout must not be read
    y = y.to(dev)
    tag = f"nhwc_to_nchw {N}x{H}x{W} ld {ld} cout {cout}"
    gb = _Guarded()
    out = gb((N, cout, H, W), torch.float32, dev)
    call("pmi_nhwc_to_nchw", ptr(y), ld, ptr(out), N, H, W, cout, mul, add)
    gb.verify(tag)
    out2 = torch.empty_like(out)
    call("pmi_nhwc_to_nchw", ptr(y), ld, ptr(out2), N, H, W, cout, mul, add)
    _same_bits(tag + " repeat", out, out2)
    yv = y[..., :cout].double().permute(0, 3, 1, 2)
    ref = yv * mul + add
    R.echeck(tag, out.double(), ref, R.C_B * 2 * R.E32 * ((yv * mul).abs() + abs(add) + ref.abs()))


@pytest.mark.parametrize("dtype", DTYPES + ["precise"])
@pytest.mark.parametrize("dim", [128, 320])
def test_timestep_embedding(dim, dtype):
    from perceptor_amd._hip import call, ptr
    dev = _dev()
    g = torch.Generator().manual_seed(dim)
    t = torch.cat([torch.tensor([0.0, 999.0, 1.0, 0.5]), torch.rand(60, generator=g) * 999]).float().to(dev)
    N = t.numel()
    tag = f"timestep_embedding dim {dim} {dtype}"

    def run(tt):
        gb = _Guarded()
        o = gb((tt.numel(), dim), torch.float32 if dtype == "precise" else R.TD[dtype], dev)
        call("pmi_timestep_embedding", ptr(tt), ptr(o), tt.numel(), dim, 10000.0, _dt(dtype))
        gb.verify(tag)
        return o
    out = run(t)
    _same_bits(tag + " repeat", out, run(t))
    _same_bits(tag + " one sample", run(t[:1].contiguous()), out[:1])
    ref, tol = R.timestep_embedding_ref(t, dim, 10000.0, dtype)
    R.echeck(tag, out.double(), ref, tol)
    assert out.shape == (N, dim)


@pytest.mark.parametrize("half", [8, 128])
def test_fourier_features(half):
    from perceptor_amd._hip import call, ptr
    dev = _dev()
    g = torch.Generator().manual_seed(half)
    t = torch.rand(9, generator=g).to(dev)
    w = (16 * torch.randn(half, generator=g)).to(dev)
    tag = f"fourier_features half {half}"
    gb = _Guarded()
    out = gb((9, 2 * half), torch.float32, dev)
    call("pmi_fourier_features", ptr(t), ptr(w), ptr(out), 9, half)
    gb.verify(tag)
    out2 = torch.empty_like(out)
    call("pmi_fourier_features", ptr(t), ptr(w), ptr(out2), 9, half)
    _same_bits(tag + " repeat", out, out2)
    out1 = torch.empty_like(out[:1])
    call("pmi_fourier_features", ptr(t[:1]), ptr(w), ptr(out1), 1, half)
    _same_bits(tag + " one sample", out1, out[:1])
    ref, tol = R.fourier_ref(t, w)
    R.echeck(tag, out.double(), ref, tol)


# ---- 7. argument checks ------------------------------------------------------------------------------------------------------------------
def test_argument_checks_launch_nothing():
    from perceptor_amd._hip import DT_F16, DT_F16X2, lib, stream_ptr
    dev = _dev()
    L, s = lib(), stream_ptr()
    x = torch.zeros(2 * 8 * 8 * 4096, dtype=torch.float16, device=dev)
    out = torch.full((2 * 8 * 8 * 4096,), float("nan"), dtype=torch.float32, device=dev)
    o16 = torch.full((2 * 8 * 8 * 4096,), float("nan"), dtype=torch.float16, device=dev)
    ca = torch.ones(2 * 4096, device=dev)
    X, O, O16, A = x.data_ptr(), out.data_ptr(), o16.data_ptr(), ca.data_ptr()
    rcs = {
        "gn_stats C > 4096": L.pmi_gn_stats(X, None, 0, O, 1, 4, 4104, 8, 1, DT_F16, s),
        "gn_stats C % 8": L.pmi_gn_stats(X, None, 0, O, 1, 4, 68, 4, 1, DT_F16, s),
        "gn_stats C % G": L.pmi_gn_stats(X, None, 0, O, 1, 4, 64, 24, 1, DT_F16, s),
        "gn_stats C0 % 8": L.pmi_gn_stats(X, X, 12, O, 1, 4, 64, 8, 1, DT_F16, s),
        "gn_apply pool odd H": L.pmi_gn_apply(X, None, 0, A, A, None, O16, 1, 5, 4, 64, 0, 1, DT_F16, s),
        "gn_apply pool odd W": L.pmi_gn_apply(X, None, 0, A, A, None, O16, 1, 4, 7, 64, 0, 1, DT_F16, s),
        "avgpool2 odd H": L.pmi_avgpool2(X, O16, 1, 5, 4, 64, DT_F16, s),
        "avgpool2 odd W": L.pmi_avgpool2(X, O16, 1, 4, 7, 64, DT_F16, s),
        "timestep_embedding odd dim": L.pmi_timestep_embedding(A, O16, 2, 127, 10000.0, DT_F16, s),
        "gn_bwd_stats precise": L.pmi_gn_bwd_stats(X, None, 64, X, A, A, 0, O, 1, 4, 64, 1, DT_F16X2, s),
        "gn_bwd_apply precise": L.pmi_gn_bwd_apply(X, None, 64, X, A, A, A, A, 0, None, None, O16, None, 1, 4, 64, DT_F16X2, s),
    }
    torch.cuda.synchronize()
    for k, rc in rcs.items():
        R.parity(f"argcheck {k} rc {rc}", 0.0, 0.0)
        assert rc == -1, f"{k}: returned {rc}"
    assert torch.isnan(out).all() and torch.isnan(o16).all(), "a rejected call wrote its output"
