"""Up-sampling 3x3 convolutions by output phase (tile config 9, csrc/conv_up_wd.hip) against float64.

A 3x3 convolution over nearest-x2(x) is four 2x2 convolutions over x, one per output parity, with sums of the 3x3 taps as weights
(PackedLinear.frag16_up).  Every case runs on the phased route twice (same bits) and once on the gather route (config 6), and is held to
  A  the kernel's own arithmetic: float64 convolution of the phase weights AS PACKED (summed in fp32, rounded once) with the 16-bit
     operand (with a prologue: float64 silu(a x + b) rounded to the compute type).  Per element, u the type's unit roundoff,
     S = sum |w_eff| |operand|:  u |ref| + 4 Cin 2^-24 S  (output rounding + worst-case fp32 accumulation over 4 Cin terms),
     + 2 u S with a prologue (the kernel's fp32 exp2 / rcp SiLU may land one ulp from the float64 one on any operand);
  B  the contract: float64 3x3 convolution of the UNROUNDED fp32 weights over the nearest-x2 operand, tolerance A + u sum |w| |operand|
     (weight rounding).  Both routes must meet B.
Statistics rows of the phased route go through ops.group_norm_coeffs and are compared with float64 statistics of the route's own output
(helper and criterion of tests/test_gpu_norm_resample.py's fused-route cases).  The eligibility rule is checked on filled IgemmArgs.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import _norm_ref64 as NR
import _ref64 as R

DTYPES = ["bf16", "f16"]

CASES = {
    # one tile touching all four borders, a single chunk, all four phases
    "border_1chunk": dict(n=1, h=8, w=32, cin=64, cout=256, bias=True),
    # 2 x 2 tiles (seams), odd chunk count (double-buffer wrap, window period), two channel tiles, SiLU prologue with per-image
    # coefficients and b != 0 everywhere (un-zeroed padding would show as silu(b)), per-sample bias, statistics
    "seams_pro_stats": dict(n=2, h=16, w=64, cin=192, cout=512, bias=True, pro=True, nbias=True, stats=True),
    # the input is a channel slice of a wider tensor: lda0 > C0
    "slice_lda": dict(n=1, h=8, w=32, cin=128, cout=256, bias=True, wide=192, off=32),
}


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _same_bits(tag, a, b):
    assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), f"{tag}: results differ bitwise"


_CACHE = {}


def _run(name, dtype):
    """One case: outputs of both routes, references and tolerances (computed once per (case, dtype), shared and left unchanged)."""
    if (name, dtype) in _CACHE:
        return _CACHE[(name, dtype)]
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    cs = CASES[name]
    dev = _dev()
    dt = _hip.dtype_code(dtype)
    td = R.TD[dtype]
    u = R.U[dtype]
    n, h, w, cin, cout = cs["n"], cs["h"], cs["w"], cs["cin"], cs["cout"]
    g = torch.Generator().manual_seed(1000 + h * 3 + cin)
    wide = cs.get("wide", cin)
    xw = torch.randn(n, h, w, wide, generator=g).to(td).to(dev)
    x = xw[..., cs.get("off", 0):cs.get("off", 0) + cin]                  # a view: stride(-2) = wide
    w32 = (torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).float()        # unrounded fp32 weights
    bias = (0.3 * torch.randn(cout, generator=g)).float() if cs.get("bias") else None
    nbias = (0.3 * torch.randn(n, cout, generator=g)).float().to(dev) if cs.get("nbias") else None
    lin = ops.PackedLinear(w32, bias, dt, dev, up_phase=True)
    assert lin.frag16_up(64) is not None
    pro = None
    op64 = x.double()
    if cs.get("pro"):
        ca = (1.0 + 0.3 * torch.randn(n, cin, generator=g)).float().to(dev)
        cb = (0.5 + 0.25 * torch.rand(n, cin, generator=g)).float().to(dev) * torch.where(torch.rand(n, cin, generator=g) < 0.5, -1.0, 1.0).to(dev)
        pro = (ca, cb, 2)
        t = op64 * ca.double()[:, None, None, :] + cb.double()[:, None, None, :]
        op64 = R.rnd(t * torch.sigmoid(t), dtype)

    def route(cfg):
        _hip.lib().pmi_set_option(1, cfg)
        try:
            y = ops.igemm(x, lin, up=True, nbias=nbias, prologue=pro, want_stats=bool(cs.get("stats")))
            torch.cuda.synchronize()
        finally:
            _hip.lib().pmi_set_option(1, -1)
        return y

    traced = []
    ops.KERNEL_EVENTS = traced
    try:
        y9 = route(9)
    finally:
        ops.KERNEL_EVENTS = None
    assert traced and " cfg9" in traced[0][4], f"the call did not take tile config 9: {traced}"
    y9b = route(9)
    y6 = route(6)

    add = torch.zeros(n, 1, 1, cout, dtype=torch.float64, device=dev)
    if bias is not None:
        add = add + bias.double().to(dev)[None, None, None, :]
    if nbias is not None:
        add = add + nbias.double()[:, None, None, :]
    # reference A: per phase a 2x2 convolution of the packed phase weights on the zero-padded low-resolution operand
    weff = lin.up_weights().double()                                      # [N, a, b, u, v, Cin] as packed
    opc = F.pad(op64.permute(0, 3, 1, 2), (1, 1, 1, 1))
    ref_a = torch.zeros(n, 2 * h, 2 * w, cout, dtype=torch.float64, device=dev)
    s_a = torch.zeros_like(ref_a)
    for a_ in range(2):
        for b_ in range(2):
            k = weff[:cout, a_, b_].permute(0, 3, 1, 2)                    # [N, Cin, u, v]
            sl = opc[:, :, a_:a_ + h + 1, b_:b_ + w + 1]
            ref_a[:, a_::2, b_::2] = F.conv2d(sl, k).permute(0, 2, 3, 1)
            s_a[:, a_::2, b_::2] = F.conv2d(sl.abs(), k.abs()).permute(0, 2, 3, 1)
    ref_a = ref_a + add
    acc = 4 * cin * 2.0 ** -24 + (2 * u if pro is not None else 0.0)
    tol_a = u * ref_a.abs() + acc * s_a
    # reference B: the 3x3 convolution of the unrounded weights over the nearest-x2 operand
    opu = op64.permute(0, 3, 1, 2).repeat_interleave(2, 2).repeat_interleave(2, 3)
    w64 = w32.double().to(dev)
    ref_b = F.conv2d(opu, w64, padding=1).permute(0, 2, 3, 1) + add
    s_b = F.conv2d(opu.abs(), w64.abs(), padding=1).permute(0, 2, 3, 1)
    tol_b = u * ref_b.abs() + acc * s_a + u * s_b
    out = dict(y9=y9, y9b=y9b, y6=y6, ref_a=ref_a, tol_a=tol_a, ref_b=ref_b, tol_b=tol_b)
    _CACHE[(name, dtype)] = out
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(CASES))
def test_up_phase_conv(name, dtype):
    """Cases 1-3: phased route against its own arithmetic (A) and the contract (B), bit-identical repeats; the gather route against B."""
    r = _run(name, dtype)
    tag = f"up-phase {name} {dtype}"
    _same_bits(tag + " repeat", r["y9"], r["y9b"])
    NR.echeck(tag + " cfg9 vs A (packed phase weights)", r["y9"].double(), r["ref_a"], r["tol_a"])
    NR.echeck(tag + " cfg9 vs B (unrounded 3x3)", r["y9"].double(), r["ref_b"], r["tol_b"])
    NR.echeck(tag + " cfg6 vs B (unrounded 3x3)", r["y6"].double(), r["ref_b"], r["tol_b"])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_up_phase_statistics(dtype):
    """Case 4: the statistics rows of case 2 through ops.group_norm_coeffs against float64 statistics of the route's own output."""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    r = _run("seams_pro_stats", dtype)
    y = r["y9"]
    dev = y.device
    assert hasattr(y, "_pmi_stats"), "the phased route took no statistics epilogue"
    n, hh, ww, c = y.shape
    rows = y._pmi_stats[1]
    assert rows == (hh // 8) * (ww // 32)
    _same_bits("statistics rows repeat", y._pmi_stats[0].view(torch.int16), r["y9b"]._pmi_stats[0].view(torch.int16))
    g = torch.Generator().manual_seed(5)
    gamma = (1 + 0.2 * torch.randn(c, generator=g)).to(dev)
    beta = (0.2 * torch.randn(c, generator=g)).to(dev)
    yv = y.double()
    u = R.U[dtype]
    pert = u * yv.abs() * (1 + u)            # the partials are statistics of the un-rounded outputs: within u |y| of the stored ones
    co = NR.gn_coeffs_ref(yv, 32, 1e-5, gamma, beta, None, 0, depth=NR.fused_depth(hh * ww, rows), pert=pert)
    ca, cb = ops.group_norm_coeffs(y, gamma, beta, 32, _hip.dtype_code(dtype))
    ra, rb = NR.coeff_bound_ratio(ca, cb, co)
    R.parity(f"up-phase statistics {dtype} coef a", ra, 1.0)
    R.parity(f"up-phase statistics {dtype} coef b", rb, 1.0)
    assert ra <= 1 and rb <= 1, (ra, rb)


def _args(n=8, hin=32, win=64, cin=64, cout=256, **kw):
    from perceptor_amd._hip import IgemmArgs
    a = IgemmArgs()
    a.H, a.W, a.Hin, a.Win = 2 * hin, 2 * win, hin, win
    a.hw = a.H * a.W
    a.M, a.N, a.K, a.C0, a.C1 = n * a.H * a.W, cout, 9 * cin, cin, 0
    a.lda0, a.ldb, a.ldd = cin, 9 * cin, cout
    a.taps, a.stride, a.up, a.alpha = 9, 1, 1, 1.0
    a.batch, a.batch_inner, a.dtype = 1, 1, 1
    a.Bf = 1                                  # marker: fragment-ordered weights exist
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_up_phase_eligibility():
    """Case 5: pmi_conv3x3_halo_config on filled arguments (host logic of the library)."""
    from perceptor_amd import _hip
    q = lambda a: _hip.lib().pmi_conv3x3_halo_config(C.byref(a))
    _hip.lib().pmi_set_option(1, -1)
    assert q(_args()) == 9                                             # 8 x 4 x 2 tiles x 4 phases = 256 workgroups >= 192
    # refused, and the call keeps the config it has without the phased route
    assert q(_args(A1=1, C1=64, lda1=64, K=9 * 128)) == 6              # a second source
    assert q(_args(R=1, ldr=256)) == 6                                 # a residual
    assert q(_args(split_in=1, split_out=32, dtype=2)) == 6            # split in / out
    assert q(_args(win=48)) == 6                                       # Win % 32 != 0 (W = 96 still tiles the gather route)
    assert q(_args(cout=128)) == 7                                     # N % 256 != 0
    s2 = _args(stride=2)
    s2.H, s2.W = s2.H // 2, s2.W // 2
    s2.M = 8 * s2.H * s2.W
    assert q(s2) == -1                                                 # stride 2
    assert q(_args(reserved3=2)) == 6                                  # the caller holds no phase weights
    assert q(_args(n=1, hin=8, win=32)) != 9                           # 4 workgroups: below the threshold unless forced
    _hip.lib().pmi_set_option(1, 9)
    try:
        assert q(_args(n=1, hin=8, win=32)) == 9
    finally:
        _hip.lib().pmi_set_option(1, -1)
    for forced in (6, 7):                                              # forcing the gather configs keeps the gather route
        _hip.lib().pmi_set_option(1, forced)
        try:
            assert q(_args(cout=256 if forced == 6 else 128)) == forced
        finally:
            _hip.lib().pmi_set_option(1, -1)
    _hip.lib().pmi_set_option(15, 0)                                   # the A/B option
    try:
        assert q(_args()) == 6
    finally:
        _hip.lib().pmi_set_option(15, 1)
    assert q(_args()) == 9
