"""GPU: pmi_conv3x3_skip -- a ResBlock's conv2 with its two-source 1x1 skip convolution folded into the K loop (csrc/conv_wd.hip, skip
segment) -- against float64, called through ctypes.

Reference (float64, from the 16-bit-rounded operands): y = conv3x3(silu(a h + b)) + W_s (x0 | x1) + bias, zero padding after the activation.
Elementwise bound, each term a rounding the kernel performs, written out in float64:
  u |y|                                        the output's one rounding to 16 bit
  (u + 2^-21) conv3x3(|silu(a h + b)|, |W|)    the activated operand is rounded once to 16 bit before its MFMA (u each); 2^-21 covers the fp32
                                               prologue arithmetic (fma, v_exp, v_rcp: a few fp32 ulp)
  (9 cin + C0 + C1) 2^-24 S                    fp32 accumulation over all products of one output, S = conv3x3(|act|, |W|) + |W_s| (|x0| | |x1|) + |bias|
The skip operands are staged raw: no rounding term of their own.  The two-launch route rounds the skip tensor and the conv output to 16
bit as well: its bound adds u |W_s x + b_s| + u |conv + b|, and the two routes must agree within the sum of both bounds.
Statistics are fp32 sums of the 16-bit outputs: |err| <= (hw + 1) 2^-24 sum |v| against the float64 sums of the same outputs.
"""
import ctypes as C

import pytest
import torch

from _ref64 import TD, U

pytestmark = pytest.mark.gpu

N, H, W = 2, 16, 64       # 2 x 2 tiles of 8 x 32 pixels: every image border and an interior seam in both directions
# (tile config, cout = conv2's cin, C0, C1)
CASES = [(7, 128, 128, 128), (7, 128, 256, 128), (6, 256, 256, 256), (6, 256, 256, 128)]
IDS = [f"cfg{c[0]}-{c[1]}-{c[2]}+{c[3]}" for c in CASES]
DTYPES = ["bf16", "f16"]


def _params(idx):
    """(case, dtype) pairs of the given cases.  The 128-channel tiles exist in bf16 only: their f16 instantiation does not compile without
    scratch, so it is not built and the call is refused (test_f16_on_128_channel_tiles_is_refused)."""
    return [pytest.param(CASES[i], dt, id=f"{IDS[i]}-{dt}") for i in idx for dt in DTYPES if not (CASES[i][0] == 7 and dt == "f16")]


def _dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _inputs(case, dtype, seed=0, zero_h_weights=False, zero_skip=False, sparse=False, hot_border=False):
    """float64 operands already rounded to the 16-bit type (weights, activations) or fp32 (coefficients, biases)"""
    _, cout, c0, c1 = case
    g = torch.Generator().manual_seed(1000 * seed + cout + c0 + 7 * c1)
    r16 = lambda t: t.to(TD[dtype]).double()
    d = {}
    d["h"] = r16(torch.randn(N, H, W, cout, generator=g))
    d["x0"] = r16(torch.randn(N, H, W, c0, generator=g))
    d["x1"] = r16(torch.randn(N, H, W, c1, generator=g))
    d["ca"] = (0.5 + torch.rand(N, cout, generator=g)).float()
    d["cb"] = (torch.rand(N, cout, generator=g) - 0.5).float()
    d["w"] = r16(torch.randn(cout, cout, 3, 3, generator=g) / (3.0 * cout ** 0.5))
    d["ws"] = r16(torch.randn(cout, c0 + c1, generator=g) / (c0 + c1) ** 0.5)
    d["bw"], d["bs"] = torch.randn(cout, generator=g).float(), torch.randn(cout, generator=g).float()
    if zero_h_weights:
        d["w"].zero_()
    if zero_skip:
        d["ws"].zero_(); d["bs"].zero_()
    if sparse:        # x0 only in its first 32 channels, x1 only in its last 32: a wrong source switch or chunk order moves the product
        d["x0"][..., 32:] = 0
        d["x1"][..., :-32] = 0
    if hot_border:    # large values on the pixels around every tile seam and image border: a halo pixel leaking into the centre tap shows
        for t in (d["x0"], d["x1"]):
            for y in (0, 7, 8, 15):
                t[:, y] *= 64.0
            for x in (0, 31, 32, 63):
                t[:, :, x] *= 64.0
    return d


def _reference(d, dtype):
    u = U[dtype]
    cout = d["w"].shape[0]
    k = 9 * cout + d["ws"].shape[1]
    t = d["ca"].double()[:, None, None, :] * d["h"] + d["cb"].double()[:, None, None, :]
    act = (t * torch.sigmoid(t)).permute(0, 3, 1, 2)
    conv = torch.nn.functional.conv2d(act, d["w"], padding=1).permute(0, 2, 3, 1)
    conv_abs = torch.nn.functional.conv2d(act.abs(), d["w"].abs(), padding=1).permute(0, 2, 3, 1)
    x = torch.cat([d["x0"], d["x1"]], -1)
    skip = x @ d["ws"].t()
    skip_abs = x.abs() @ d["ws"].abs().t()
    bias = d["bw"].double() + d["bs"].double()
    y = conv + skip + bias
    tol = u * y.abs() + (u + 2.0 ** -21) * conv_abs + k * 2.0 ** -24 * (conv_abs + skip_abs + bias.abs())
    tol_two = tol + u * (skip + d["bs"].double()).abs() + u * (conv + d["bw"].double()).abs()
    return y, tol, tol_two


class _Dev:
    """the operands on the device, the packed layers, and one fused launch through ctypes"""

    def __init__(self, d, case, dtype, pad=True):
        from perceptor_amd import _hip
        from perceptor_amd.engine import ops
        self.cfg, cout, c0, c1 = case
        self.dt = _hip.dtype_code(dtype)
        dev, td = _dev(), TD[dtype]
        self.h = d["h"].to(device=dev, dtype=td).contiguous()

        def padded(t, extra):      # padded NHWC: the row pitch is larger than the channel count
            if not pad:
                return t.to(device=dev, dtype=td).contiguous()
            full = torch.full(t.shape[:-1] + (t.shape[-1] + extra,), 777.0, dtype=td, device=dev)
            full[..., :t.shape[-1]] = t.to(device=dev, dtype=td)
            return full[..., :t.shape[-1]]
        self.x0, self.x1 = padded(d["x0"], 16), padded(d["x1"], 8)
        self.ca, self.cb = d["ca"].to(dev).contiguous(), d["cb"].to(dev).contiguous()
        self.conv = ops.PackedLinear(d["w"].float(), d["bw"], self.dt, dev)
        self.skip = ops.PackedLinear(d["ws"].float()[:, :, None, None], d["bs"], self.dt, dev, sources=[c0, c1])
        self.bias = ops.fused_skip_bias(self.conv, self.skip)

    def args(self):
        from perceptor_amd import _hip
        n, hh, ww, c = self.h.shape
        a, k = _hip.IgemmArgs(), _hip.SkipArgs()
        out = torch.empty((n, hh, ww, self.conv.n_p), dtype=self.h.dtype, device=self.h.device)
        st = torch.zeros((n, (hh // 8) * (ww // 32), self.conv.n_p, 2), dtype=torch.float32, device=self.h.device)
        a.A0, a.B, a.Bf, a.bias, a.D = self.h.data_ptr(), self.conv.w.data_ptr(), self.conv.frag16(64 if self.cfg == 6 else 32).data_ptr(), self.bias.data_ptr(), out.data_ptr()
        a.pro_a, a.pro_b, a.pro_act = self.ca.data_ptr(), self.cb.data_ptr(), _hip.ACT_SILU
        a.M, a.N, a.K, a.C0, a.lda0, a.ldb, a.ldd = n * hh * ww, self.conv.n_p, self.conv.K, c, self.h.stride(-2), self.conv.K, out.stride(-2)
        a.H = a.Hin = hh
        a.W = a.Win = ww
        a.taps, a.stride, a.alpha, a.batch, a.batch_inner, a.dtype, a.hw = 9, 1, 1.0, 1, 1, self.dt, hh * ww
        a.stats, a.stats_p = st.data_ptr(), st.shape[1]
        k.X0, k.X1, k.Wf = self.x0.data_ptr(), self.x1.data_ptr(), self.skip.frag_skip().data_ptr()
        k.C0, k.C1, k.ld0, k.ld1 = self.x0.shape[-1], self.x1.shape[-1], self.x0.stride(-2), self.x1.stride(-2)
        return a, k, out, st

    def forced(self):
        from perceptor_amd import _hip
        lib = _hip.lib()

        class _F:
            def __enter__(s):          # the tile config under test
                lib.pmi_set_option(1, self.cfg)

            def __exit__(s, *e):
                lib.pmi_set_option(1, -1)
        return _F()

    def fused(self):
        from perceptor_amd import _hip
        a, k, out, st = self.args()
        with self.forced():
            assert _hip.lib().pmi_conv3x3_skip_eligible(C.byref(a), C.byref(k)) == self.cfg
            rc = _hip.lib().pmi_conv3x3_skip(C.byref(a), C.byref(k), _hip.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        return out, st

    def two_launch(self):
        from perceptor_amd import _hip
        from perceptor_amd.engine import ops
        with self.forced():
            r = ops.igemm(self.x0, self.skip, a1=self.x1)
            out = ops.igemm(self.h, self.conv, residual=r, prologue=(self.ca, self.cb, _hip.ACT_SILU), want_stats=True)
        torch.cuda.synchronize()
        return out

    def conv_only(self):
        from perceptor_amd import _hip
        from perceptor_amd.engine import ops
        with self.forced():
            out = ops.igemm(self.h, self.conv, prologue=(self.ca, self.cb, _hip.ACT_SILU), want_stats=True)
        torch.cuda.synchronize()
        return out


def _ratio(got, ref, tol):
    return float(((got.double().cpu() - ref).abs() / tol).max())


WORST = {}


@pytest.mark.parametrize("case,dtype", _params([0, 1, 2, 3]))
def test_fused_matches_float64_and_the_two_launch_route(case, dtype):
    d = _inputs(case, dtype)
    y, tol, tol_two = _reference(d, dtype)
    dv = _Dev(d, case, dtype)
    got, st = dv.fused()
    r = _ratio(got, y, tol)
    two = dv.two_launch()
    r2 = _ratio(two, y, tol_two)
    rab = float(((got.double().cpu() - two.double().cpu()).abs() / (tol + tol_two)).max())
    print(f"[conv_skip] {IDS[CASES.index(case)]} {dtype}: fused err/tol {r:.3f}, two-launch err/tol {r2:.3f}, fused vs two-launch {rab:.3f}")
    WORST[(case, dtype)] = r
    assert r <= 1.0, f"fused launch outside its float64 bound: {r:.3f} x tol"
    assert r2 <= 1.0, f"two-launch route outside its float64 bound: {r2:.3f} x tol"
    assert rab <= 1.0, f"the two routes disagree: {rab:.3f} x (sum of both bounds)"
    # output statistics (sum, sum of squares per channel) see conv + skip: fp32 sums of the 16-bit outputs
    g = got.double().cpu().reshape(N, H * W, -1)
    s = st.double().cpu().sum(1)
    for j, v in enumerate((g, g * g)):
        tol_s = (H * W + 1) * 2.0 ** -24 * v.abs().sum(1)
        rs = float(((s[..., j] - v.sum(1)).abs() / tol_s).max())
        print(f"[conv_skip] statistics {'sum' if j == 0 else 'sumsq'} err/tol {rs:.3f}")
        assert rs <= 1.0, (j, rs)


@pytest.mark.parametrize("case,dtype", _params([1, 3]))
def test_segment_is_neither_lost_nor_misplaced(case, dtype):
    # h weights zero: the skip product alone
    d = _inputs(case, dtype, seed=1, zero_h_weights=True)
    y, tol, _ = _reference(d, dtype)
    got, _ = _Dev(d, case, dtype).fused()
    r = _ratio(got, y, tol)
    print(f"[conv_skip] zero conv weights: err/tol {r:.3f}")
    assert r <= 1.0
    assert float(y.abs().max()) > 1.0
    # x0 only in its first 32 channels, x1 only in its last 32
    d = _inputs(case, dtype, seed=2, sparse=True)
    y, tol, _ = _reference(d, dtype)
    r = _ratio(_Dev(d, case, dtype).fused()[0], y, tol)
    print(f"[conv_skip] sparse sources: err/tol {r:.3f}")
    assert r <= 1.0
    # large values around every tile seam and image border
    d = _inputs(case, dtype, seed=3, hot_border=True)
    y, tol, _ = _reference(d, dtype)
    r = _ratio(_Dev(d, case, dtype).fused()[0], y, tol)
    print(f"[conv_skip] hot borders: err/tol {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("case,dtype", _params([0, 2]))
def test_zero_skip_weights_are_bit_identical_to_the_plain_conv(case, dtype):
    d = _inputs(case, dtype, seed=4, zero_skip=True)
    dv = _Dev(d, case, dtype)
    got, st = dv.fused()
    plain = dv.conv_only()
    assert torch.equal(got, plain)
    assert torch.equal(st, plain._pmi_stats[0])


@pytest.mark.parametrize("case,dtype", _params([1, 2]))
def test_deterministic_and_batch_order_free(case, dtype):
    d = _inputs(case, dtype, seed=5)
    a1, s1 = _Dev(d, case, dtype).fused()
    a2, s2 = _Dev(d, case, dtype, pad=False).fused()        # (dense rows: the pitch is no part of the result)
    assert torch.equal(a1, a2) and torch.equal(s1, s2)
    sw = {k: (v.flip(0) if k in ("h", "x0", "x1", "ca", "cb") else v) for k, v in d.items()}
    a3, s3 = _Dev(sw, case, dtype).fused()
    assert torch.equal(a3, a1.flip(0)) and torch.equal(s3, s1.flip(0))


def test_refusals_do_not_launch():
    from perceptor_amd import _hip
    lib = _hip.lib()
    d = _inputs(CASES[0], "bf16", seed=6)
    dv = _Dev(d, CASES[0], "bf16")
    a, k, out, _ = dv.args()
    out.fill_(3.0)
    ws = torch.zeros(8, device=out.device)
    with dv.forced():
        assert lib.pmi_conv3x3_skip_eligible(C.byref(a), C.byref(k)) == 7
        for field, bad in (("splitk", 2), ("res_up", 1), ("split_in", 1), ("split_in", 2), ("N", 160), ("N", 96), ("act", _hip.ACT_SILU)):
            good = getattr(a, field)
            setattr(a, field, bad)
            if field == "splitk":
                a.ws = ws.data_ptr()
            assert lib.pmi_conv3x3_skip_eligible(C.byref(a), C.byref(k)) == 0, field
            assert lib.pmi_conv3x3_skip(C.byref(a), C.byref(k), _hip.stream_ptr()) == -1, field
            setattr(a, field, good)
            a.ws = None
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())                          # nothing ran


@pytest.mark.parametrize("forced", [False, True])
def test_f16_on_128_channel_tiles_is_refused(forced):
    """cout % 256 != 0 in f16: no launch (the two-launch route keeps such layers), with and without the tile config forced; the same layer in
    bf16 is taken, and an f16 layer with cout % 256 == 0 runs the 256-channel tiles"""
    from perceptor_amd import _hip
    lib = _hip.lib()
    dv = _Dev(_inputs(CASES[1], "f16", seed=7), CASES[1], "f16")
    a, k, out, _ = dv.args()
    out.fill_(3.0)
    if forced:
        lib.pmi_set_option(1, 7)
    try:
        assert lib.pmi_conv3x3_skip_eligible(C.byref(a), C.byref(k)) == 0
        assert lib.pmi_conv3x3_skip(C.byref(a), C.byref(k), _hip.stream_ptr()) == -1
    finally:
        lib.pmi_set_option(1, -1)
    torch.cuda.synchronize()
    assert bool((out == 3.0).all())
    a.dtype = _hip.DT_BF16
    assert lib.pmi_conv3x3_skip_eligible(C.byref(a), C.byref(k)) == 7
    a6, k6, _, _ = _Dev(_inputs(CASES[3], "f16", seed=7), CASES[3], "f16").args()
    assert lib.pmi_conv3x3_skip_eligible(C.byref(a6), C.byref(k6)) == 6


def test_engine_route_is_the_same_for_a_shard_and_the_whole_batch():
    """ops.igemm(skip=...) on a 64x64 map with 512 channels (a level the ADM engine fuses): one image and eight take the same route, and
    image 0 of the batch is bit-identical to the single-image call"""
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops
    dev, td = _dev(), torch.bfloat16
    g = torch.Generator().manual_seed(11)
    c, c0, c1, n = 512, 512, 256, 8
    h = torch.randn(n, 64, 64, c, generator=g).to(device=dev, dtype=td)
    x0 = torch.randn(n, 64, 64, c0, generator=g).to(device=dev, dtype=td)
    x1 = torch.randn(n, 64, 64, c1, generator=g).to(device=dev, dtype=td)
    ca, cb = (0.5 + torch.rand(n, c, generator=g)).to(dev), (torch.rand(n, c, generator=g) - 0.5).to(dev)
    conv = ops.PackedLinear(torch.randn(c, c, 3, 3, generator=g) / (3.0 * c ** 0.5), torch.randn(c, generator=g), _hip.DT_BF16, dev)
    skip = ops.PackedLinear(torch.randn(c, c0 + c1, 1, 1, generator=g) / (c0 + c1) ** 0.5, torch.randn(c, generator=g), _hip.DT_BF16, dev, sources=[c0, c1])
    sb = ops.fused_skip_bias(conv, skip)
    ops.KERNEL_EVENTS = []
    try:
        full = ops.igemm(h, conv, prologue=(ca, cb, _hip.ACT_SILU), want_stats=True, skip=(skip, x0, x1, sb))
        one = ops.igemm(h[:1], conv, prologue=(ca[:1], cb[:1], _hip.ACT_SILU), want_stats=True, skip=(skip, x0[:1], x1[:1], sb))
        torch.cuda.synchronize()
        descs = [e[4] for e in ops.KERNEL_EVENTS]
    finally:
        ops.KERNEL_EVENTS = None
    assert len(descs) == 2 and all(" cfg6 pro skip 512+256" in d_ for d_ in descs), descs
    assert torch.equal(full[:1], one)
