"""CPU: the host side of the fused conv2 + skip launch (pmi_conv3x3_skip): PackedLinear.frag_skip's fragment order against a plain index
formula, the fp32 bias sum of ops.fused_skip_bias, and the host-only eligibility query's refusals (no launch, no GPU)."""
import ctypes as C

import pytest
import torch

from perceptor_amd import _hip
from perceptor_amd.engine import ops


@pytest.mark.parametrize("dt", [_hip.DT_F16, _hip.DT_BF16])
@pytest.mark.parametrize("cout,srcs", [(128, (128, 64)), (256, (64, 192)), (160, (64,))])
def test_frag_skip_order(dt, cout, srcs):
    g = torch.Generator().manual_seed(cout + sum(srcs))
    k = sum(srcs)
    w = torch.randn(cout, k, 1, 1, generator=g)
    lin = ops.PackedLinear(w, None, dt, "cpu", sources=list(srcs))
    f = lin.frag_skip()
    assert f.shape == (cout // 32, k // 32, 2, 4, 16, 8) and f.is_contiguous()
    flat = f.reshape(-1)
    wr = w[:, :, 0, 0].to(_hip.TORCH_DTYPE[dt])
    # the kernel's address arithmetic: wave nb, 32-deep k-step ks, 16-channel block cb, lane = 16 q + r, element j of the lane's 16 bytes
    idx = torch.arange(flat.numel())
    j, r, q, cb, ks, nb = idx % 8, (idx // 8) % 16, (idx // 128) % 4, (idx // 512) % 2, (idx // 1024) % (k // 32), idx // (1024 * (k // 32))
    assert torch.equal(flat, wr[nb * 32 + cb * 16 + r, ks * 32 + q * 8 + j])
    # one 1 KB fragment per (k-step, channel block), a wave's stream contiguous in loop order
    assert f[1, 1, 1].numel() * f.element_size() == 1024


def test_frag_skip_is_the_gemm_order_where_both_exist():
    w = torch.randn(256, 384, 1, 1, generator=torch.Generator().manual_seed(3))
    lin = ops.PackedLinear(w, None, _hip.DT_BF16, "cpu")
    assert torch.equal(lin.frag_skip().reshape(-1), lin.frag_gemm().reshape(-1))


def test_fused_bias_is_the_fp32_sum():
    g = torch.Generator().manual_seed(5)
    bc, bs = torch.randn(128, generator=g) * 3.0, torch.randn(128, generator=g) * 1e-4
    conv = ops.PackedLinear(torch.randn(128, 128, 3, 3, generator=g), bc, _hip.DT_BF16, "cpu")
    skip = ops.PackedLinear(torch.randn(128, 192, 1, 1, generator=g), bs, _hip.DT_BF16, "cpu")
    b = ops.fused_skip_bias(conv, skip)
    assert b.dtype == torch.float32 and torch.equal(b, bc + bs)
    assert not torch.equal(b, (bc.bfloat16() + bs.bfloat16()).float())            # (a 16-bit sum would have lost the small addend)
    assert torch.equal(ops.fused_skip_bias(conv, ops.PackedLinear(torch.randn(128, 192, 1, 1, generator=g), None, _hip.DT_BF16, "cpu")), bc)


def test_eligibility_query_refuses_on_the_host():
    lib = _hip.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)                                   # never dereferenced: the query reads the structs only
    a, k = _hip.IgemmArgs(), _hip.SkipArgs()
    a.A0 = a.B = a.Bf = a.D = a.bias = a.pro_a = a.pro_b = p
    a.M, a.N, a.K, a.C0, a.lda0, a.ldb, a.ldd = 2 * 16 * 64, 128, 9 * 128, 128, 128, 9 * 128, 128
    a.H = a.Hin = 16
    a.W = a.Win = 64
    a.taps, a.stride, a.alpha, a.batch, a.batch_inner, a.dtype, a.pro_act, a.hw = 9, 1, 1.0, 1, 1, _hip.DT_BF16, _hip.ACT_SILU, 16 * 64
    k.X0 = k.X1 = k.Wf = p
    k.C0, k.C1, k.ld0, k.ld1 = 128, 64, 128, 72
    q = lambda: lib.pmi_conv3x3_skip_eligible(C.byref(a), C.byref(k))
    _refusals(lib, a, k, q, p)
    try:
        lib.pmi_set_option(16, 0)
        assert q() == 0                                    # the A/B switch: callers keep the separate skip GEMM
    finally:
        lib.pmi_set_option(16, 1)
    assert q() == 7


def _refusals(lib, a, k, q, p):
    assert q() == 7                                        # cout 128: the 128-channel tiles (bf16)
    for field, bad in (("splitk", 2), ("res_up", 1), ("split_in", 1), ("split_out", 32), ("N", 160), ("N", 96), ("R", p), ("up", 1), ("out_f32", 1),
                       ("pro_act", _hip.ACT_RELU), ("alpha", 0.5), ("dtype", _hip.DT_F16X2), ("dtype", _hip.DT_F16), ("W", 48), ("act", _hip.ACT_SILU), ("A0", p + 8)):
        good = getattr(a, field)
        setattr(a, field, bad)
        assert q() == 0, field
        assert lib.pmi_conv3x3_skip(C.byref(a), C.byref(k), None) == -1, field      # refused before any launch
        setattr(a, field, good)
    for field, bad in (("C0", 96), ("C1", 32), ("ld1", 60), ("X0", None), ("Wf", None)):
        good = getattr(k, field)
        setattr(k, field, bad)
        assert q() == 0, field
        setattr(k, field, good)
    assert q() == 7


def test_route_and_tile_config_do_not_depend_on_the_batch():
    """the same layer and map at batch 1, 2, 3, 8, 64: one answer.  A 64x64 map with 512 channels is the case where the plain launch's
    split-K rule (workgroup count) changes between 2 and 3 images; neither it nor any other workgroup count enters the query."""
    lib = _hip.lib()
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    for dt, cout, hw, want in ((_hip.DT_BF16, 512, 64, 6), (_hip.DT_F16, 512, 64, 6), (_hip.DT_BF16, 128, 512, 7), (_hip.DT_F16, 128, 512, 0),
                               (_hip.DT_BF16, 256, 32, 6), (_hip.DT_BF16, 384, 64, 7)):
        got = []
        for n in (1, 2, 3, 8, 64):
            a, k = _hip.IgemmArgs(), _hip.SkipArgs()
            a.A0 = a.B = a.Bf = a.D = a.bias = a.pro_a = a.pro_b = p
            a.M, a.N, a.K, a.C0, a.lda0, a.ldb, a.ldd = n * hw * hw, cout, 9 * cout, cout, cout, 9 * cout, cout
            a.H = a.Hin = a.W = a.Win = hw
            a.taps, a.stride, a.alpha, a.batch, a.batch_inner, a.dtype, a.pro_act, a.hw = 9, 1, 1.0, 1, 1, dt, _hip.ACT_SILU, hw * hw
            k.X0 = k.X1 = k.Wf = p
            k.C0, k.C1, k.ld0, k.ld1 = cout, cout // 2, cout, cout // 2
            got.append(lib.pmi_conv3x3_skip_eligible(C.byref(a), C.byref(k)))
        assert got == [want] * 5, (dt, cout, hw, got)
