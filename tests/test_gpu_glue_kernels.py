"""GPU: the staging, token, layout and sampler glue kernels, each called by its own name through perceptor_amd._hip.call and compared with
the plain restatements of tests/_glue_ref64.py.

Every output lies inside a larger NaN-filled buffer with a guard band in front of and behind it: the kernel must write the whole output
and leave both bands untouched.  Pure data movement and single fp32 operations are compared exactly with the CPU expression; arithmetic
kernels against float64 with the bound derived in the test's docstring (u = 2^-24).  tests/test_glue_bounds_cpu.py requires the same
bound functions to reject seeded defects at these inputs.
"""
import math

import numpy as np
import pytest
import torch

import _glue_ref64 as R

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
GUARD = 64

ASSEMBLE_CASES = [(1, 2, 4), (2, 5, 48), (3, 50, 64)]
EMBED_CASES = [(2, 7, 24, 11), (1, 77, 64, 100)]
GATHER_CASES = [(3, 20, 20, 9), (5, 64, 72, 6), (1, 1, 1, 1)]
CHW = [1, 5, 3 * 67 * 67]
SORT_N = [1, 2, 4095, 4096, 4097, 8193]
PATCH_CASES = [(2, 28, 14, 592), (1, 32, 8, 192), (2, 12, 4, 48)]             # (N, R, P, Kp): the first has pad columns, Kp > 3 P^2
BAND_CASES = [(40, 64, "cubic"), (100, 48, "cubic"), (300, 20, "lanczos3"), (4, 9, "cubic"), (5, 11, "cubic")]
QUANT_N = [1, 2, 3, 4097]
WASS_N = [1, 2, 4097]
RESIZE2 = [("40x100_64x48", (1, 3, 40, 100), (64, 48)), ("37x53_64x64", (1, 3, 37, 53), (64, 64)), ("4x5_9x11", (1, 3, 4, 5), (9, 11)),
           ("75x100_32x100", (1, 3, 75, 100), (32, 100)), ("64x64_63x65", (2, 3, 64, 64), (63, 65))]


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


class _Guarded:
    """outputs that start as NaN inside a larger NaN buffer: GUARD elements in front of and behind the logical extent"""

    def __init__(self):
        self.bufs = []

    def __call__(self, shape, dtype=torch.float32):
        numel = math.prod(shape)
        buf = torch.full((numel + 2 * GUARD,), float("nan"), dtype=dtype, device=_dev())
        self.bufs.append((buf, numel))
        return buf[GUARD:GUARD + numel].view(shape)

    def verify(self, tag):
        torch.cuda.synchronize()
        for buf, numel in self.bufs:
            assert torch.isnan(buf[:GUARD].float()).all(), f"{tag}: a kernel wrote in front of its output"
            assert torch.isnan(buf[GUARD + numel:].float()).all(), f"{tag}: a kernel wrote past the end of its output"


def _call(name, *args):
    from perceptor_amd import _hip
    _hip.call(name, *[a.data_ptr() if torch.is_tensor(a) else a for a in args])


def _refused(name, *args):
    with pytest.raises(RuntimeError, match="bad argument"):
        _call(name, *args)


def _report(tag, got, ref, tol):
    m = R.worst(got, ref, tol)
    print(f"[glue] {tag}: worst |got - ref| / bound = {m:.3f}")
    assert m <= 1.0, f"{tag}: {m:.3f}x the bound"


# ---- input builders (shared with tests/test_glue_bounds_cpu.py) --------------------------------------------------------------------
def patchify_inputs(case):
    N, Rr, P, Kp = case
    img = torch.rand(N, 3, Rr, Rr, generator=R.rng(Rr * P))
    return img, torch.tensor(R.CLIP_MEAN), torch.tensor(R.CLIP_STD)


def unpatchify_inputs(case):
    N, Rr, P, Kp = case
    g = Rr // P
    dcol = torch.randn(N * g * g, Kp, generator=R.rng(Kp + P))
    dcol[:, 3 * P * P:] = float("nan")
    return dcol, torch.tensor(R.CLIP_STD), 0.37


def lincomb_inputs(chw):
    g = R.rng(chw + 5)
    a, b = torch.randn(3 * chw, generator=g), torch.randn(3 * chw, generator=g) * 3
    return a, b, torch.tensor([0.8, -1.7, 3.1]), torch.tensor([-0.45, 2.2, 0.07]), torch.tensor([0.5, -6.0, 11.0])


def hand_tables(which):
    if which == 0:                                   # (outer, in_sz, inner, out_sz, taps) = (3, 7, 5, 4, 3)
        idx = torch.tensor([[-1, 0, 1], [2, 3, 4], [-1, -1, -1], [5, 6, -1]], dtype=torch.int32)
        return (3, 7, 5, 4, 3), idx, torch.randn(4, 3, generator=R.rng(70))
    g = R.rng(71)                                    # the W-axis form, inner = 1: (6, 9, 1, 13, 4), repeated and skipped rows
    idx = torch.randint(-1, 9, (13, 4), generator=g, dtype=torch.int32)
    return (6, 9, 1, 13, 4), idx, torch.randn(13, 4, generator=g)


def band_input(shape, seed):
    return torch.rand(*shape, generator=R.rng(seed))


def _apply_band(x, idx, w, out_sz, tag):
    """x [outer][in_sz][inner] on the CPU -> pmi_resize_apply's output on the CPU"""
    outer, in_sz, inner = x.shape
    G = _Guarded()
    out = G((outer, out_sz, inner))
    d = _dev()
    _call("pmi_resize_apply", x.to(d), out, idx.to(d).contiguous(), w.to(d).contiguous(), outer, in_sz, inner, out_sz, idx.shape[1], 0, 0)
    G.verify(tag)
    return out.cpu()


# ---- pure data movement / one fp32 operation: exact --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ASSEMBLE_CASES, ids=str)
def test_vit_assemble(case):
    N, T, D = case
    g = R.rng(T)
    emb, cls, pos = torch.randn(N, T - 1, D, generator=g), torch.randn(D, generator=g), torch.randn(T, D, generator=g)
    G = _Guarded()
    x = G((N, T, D))
    d = _dev()
    _call("pmi_vit_assemble", emb.to(d), cls.to(d), pos.to(d), x, N, T, D, 0)
    G.verify(f"vit_assemble {case}")
    assert torch.equal(x.cpu(), R.vit_assemble32(emb, cls, pos))
    _refused("pmi_vit_assemble", emb.to(d), cls.to(d), pos.to(d), x, N, 1, D, 0)


@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("case", EMBED_CASES, ids=str)
def test_embed_tokens(case, with_pos):
    """ids hold 0, vocab - 1, repeats, and -1 / vocab, which the kernel clamps to rows 0 / vocab - 1 (inside the table)"""
    N, T, D, vocab = case
    g = R.rng(vocab)
    ids = torch.randint(0, vocab, (N, T), generator=g)
    ids[0, :6] = torch.tensor([0, vocab - 1, 3, 3, -1, vocab])
    tok, pos = torch.randn(vocab, D, generator=g), torch.randn(T, D, generator=g)
    G = _Guarded()
    x = G((N, T, D))
    d = _dev()
    _call("pmi_embed_tokens", ids.to(d), tok.to(d), pos.to(d) if with_pos else None, x, N, T, D, vocab)
    G.verify(f"embed_tokens {case}")
    want = R.embed_tokens32(ids, tok, pos if with_pos else None)
    assert torch.equal(want[0, 4], tok[0] + (pos[4] if with_pos else 0)) and torch.equal(want[0, 5], tok[vocab - 1] + (pos[5] if with_pos else 0))
    assert torch.equal(x.cpu(), want)


@pytest.mark.parametrize("case", GATHER_CASES, ids=str)
def test_gather_rows(case):
    """repeated indices, -1 and src_rows clamp; the columns D..ld of the source hold NaN and must not reach dst"""
    Rr, D, ld, rows = case
    src = torch.randn(rows, ld, generator=R.rng(ld))
    src[:, D:] = float("nan")
    idx = torch.tensor([rows, -1, rows // 2, rows // 2, rows - 1][:Rr] if Rr > 1 else [-1])
    G = _Guarded()
    dst = G((Rr, D))
    d = _dev()
    _call("pmi_gather_rows", src.to(d), idx.to(d), dst, Rr, D, ld, rows)
    G.verify(f"gather_rows {case}")
    assert torch.equal(dst.cpu(), R.gather_rows32(src, idx, D))


@pytest.mark.parametrize("chw", CHW)
def test_clamp_and_clamp_grad(chw):
    """per-sample bounds that all differ; inputs on a bound, +-0, +-inf and NaN.  Expected: the torch expressions x.clamp(lo, hi) and
    grad * (grad * (x - x.clamp(lo, hi)) >= 0) on the CPU, NaN for NaN."""
    x, grad, lo, hi = R.clamp_inputs(3, chw, 90 + chw)
    d = _dev()
    G = _Guarded()
    out, gout = G((3, chw)), G((3, chw))
    _call("pmi_clamp", x.to(d), lo.to(d), hi.to(d), out, 3, chw)
    _call("pmi_clamp_grad", x.to(d), grad.to(d), lo.to(d), hi.to(d), gout, 3, chw)
    G.verify(f"clamp chw {chw}")
    want, gwant = R.clamp32(x, lo, hi), R.clamp_grad32(x, grad, lo, hi)
    assert want.isnan().any()
    bad = ~((out.cpu() == want) | (out.cpu().isnan() & want.isnan()))
    assert not bad.any(), f"pmi_clamp: x {x[bad][:4]} -> {out.cpu()[bad][:4]}, expected {want[bad][:4]}"
    bad = ~((gout.cpu() == gwant) | (gout.cpu().isnan() & gwant.isnan()))
    assert not bad.any(), f"pmi_clamp_grad: x {x[bad][:4]} grad {grad[bad][:4]} -> {gout.cpu()[bad][:4]}, expected {gwant[bad][:4]}"


def _padded(n):
    from perceptor_amd import _hip
    return _hip.lib().pmi_sort_rows_padded(n)


@pytest.mark.parametrize("n", SORT_N)
def test_sort_rows(n):
    """+-0, +-inf, subnormals and heavy ties: the first n columns equal torch.sort, the padding n..npad is all +inf"""
    npad = _padded(n)
    assert npad == max(4096, 1 << (n - 1).bit_length())
    x = R.sort_rows_input(n, n)
    G = _Guarded()
    work = G((3, npad))
    _call("pmi_sort_rows", x.to(_dev()), work, 3, n)
    G.verify(f"sort_rows {n}")
    got = work.cpu()
    assert torch.equal(got[:, :n], x.sort(1)[0])
    assert bool((got[:, n:] == float("inf")).all())


def test_sort_rows_padded_range():
    for n in (0, -1, 2 ** 30 + 1):
        assert _padded(n) == -1
    assert _padded(2 ** 30) == 2 ** 30


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("dtype", DTYPES)
def test_qkv_split_layout(dtype, order):
    """qkv filled with a counter of distinct non-zero 16-bit patterns: every (n, h, t < T, d) sits at the restated rfrag / tfrag offset of Q, K
    and V^T, every other element of the three [N heads][Tp][64] buffers is exactly zero"""
    d = _dev()
    for T in (1, 31, 32, 33):
        for heads in (1, 3):
            for N in (1, 2):
                Tp = (T + 31) // 32 * 32
                qkv = R.counter16((N, T, 3 * heads * 64))
                G = _Guarded()
                q, k, vt = (G((N * heads * Tp * 64,), R.TORCH16[dtype]) for _ in range(3))
                _call("pmi_qkv_split", qkv.to(d), q, k, vt, N, T, heads, order, R.DT_CODE[dtype])
                tag = f"qkv_split T {T} heads {heads} N {N} order {order} {dtype}"
                G.verify(tag)
                for name, got, want in zip(("Q", "K", "V^T"), (q, k, vt), R.qkv_split_ref(qkv, heads, order)):
                    assert torch.equal(got.view(torch.int16).cpu(), want), f"{tag}: {name} differs"


@pytest.mark.parametrize("C", [8, 16, 24, 32, 64])
@pytest.mark.parametrize("rows", [1, 5])
def test_split_convert(rows, C):
    """to_split = 1: hi is the input bit for bit and lo is zero in the [C / G][hi G | lo G] grouping; to_split = 0: hi + lo in float64
    rounded once to f16 (the fp32 sum of two f16 values near a rounding boundary of f16 is exact, so the kernel rounds once too)"""
    g = R.rng(rows * 100 + C)
    d = _dev()
    x = torch.randn(rows, C, generator=g).half()
    x.view(-1)[:4] = torch.tensor([0.0, -0.0, 6e-8, -65504.0]).half()
    G = _Guarded()
    out = G((rows, 2 * C), torch.float16)
    _call("pmi_split_convert", x.to(d), out, rows, C, 1)
    G.verify(f"split_convert to_split {rows}x{C}")
    assert torch.equal(out.view(torch.int16).cpu(), R.split_layout(x, torch.zeros_like(x)).view(torch.int16))
    hi = torch.randn(rows, C, generator=g).half()
    lo = (hi.float() * (torch.rand(rows, C, generator=g) - 0.5) * 2.0 ** -10).half()
    lo[:, ::3] = (torch.randn(rows, C, generator=g).half())[:, ::3]            # and pairs that are no split of one value
    G = _Guarded()
    plain = G((rows, C), torch.float16)
    _call("pmi_split_convert", R.split_layout(hi, lo).to(d), plain, rows, C, 0)
    G.verify(f"split_convert to_plain {rows}x{C}")
    assert torch.equal(plain.view(torch.int16).cpu(), R.split_to_plain_bits(hi, lo))


@pytest.mark.parametrize("C", [4, 40])
def test_split_convert_refuses(C):
    d = _dev()
    buf = torch.zeros(4 * C, dtype=torch.float16, device=d)
    _refused("pmi_split_convert", buf, torch.zeros_like(buf), 1, C, 1)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 7, 4099])
def test_cast_f32_to_16(n, dtype):
    """bitwise x.to(dtype): ties between 16-bit neighbours on the even-below and even-above side, +-0, f16 subnormals, 65504 / 65520 / 1e6
    (inf in f16, finite in bf16), +-inf; NaN compared as NaN"""
    sp = R.cast_specials(dtype)
    x = torch.cat([sp, torch.randn(max(0, 4099 - len(sp)), generator=R.rng(3)) * 50])[:n] if n > 7 else sp[:n]
    if n > 7:
        assert x.isnan().any() and x.isinf().any()
    G = _Guarded()
    out = G((n,), R.TORCH16[dtype])
    _call("pmi_cast_f32_to_16", x.to(_dev()), out, n, 0, R.DT_CODE[dtype])
    G.verify(f"cast {n} {dtype}")
    got, want = out.cpu(), x.to(R.TORCH16[dtype])
    assert torch.equal(got.isnan(), want.isnan())
    keep = ~want.isnan()
    bad = (got.view(torch.int16) != want.view(torch.int16)) & keep
    assert not bad.any(), f"cast {dtype}: {x[bad][:6].tolist()} -> {got[bad][:6].tolist()}, expected {want[bad][:6].tolist()}"


# ---- arithmetic kernels: float64 with derived bounds -------------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1])
def test_resize_apply_hand_tables(which):
    """rows with skipped (-1) entries at either end and one row of nothing but -1 (which must give 0); inner = 1 is the W-axis form.
    Bound (R.band_tol): taps products and taps - 1 additions in fp32, every partial sum below S = sum_t |w x|: (taps + 1) u S."""
    (outer, in_sz, inner, out_sz, taps), idx, w = hand_tables(which)
    x = band_input((outer, in_sz, inner), 72 + which) * 2 - 1
    got = _apply_band(x, idx, w, out_sz, f"resize_apply hand {which}")
    ref, absum = R.band_apply(x, idx, w)
    if which == 0:
        assert bool((got[:, 2] == 0).all())
    _report(f"resize_apply hand table {which}", got, ref, R.band_tol(absum, taps))


@pytest.mark.parametrize("case", BAND_CASES, ids=str)
def test_resize_apply_band_tables(case):
    """band_tables forward and transposed, along H (inner = W) and along W (inner = 1) of a (2, 3, H, W) tensor, each within
    (taps + 1) u sum_t |w x|; and the adjoint identity <A x, y> = <x, A^T y> in float64 from the two GPU results within
    4 taps u sum |y| |A| |x| (R.adjoint_tol: each side carries at most (taps + 1) u of that sum)"""
    from perceptor_amd.transforms.resize import band_tables
    in_sz, out_sz, method = case
    idx, w, idx_t, w_t = band_tables(in_sz, out_sz, method)
    other = 5
    for axis in (2, 3):
        shp_in = (6, in_sz, other) if axis == 2 else (6 * other, in_sz, 1)
        shp_out = (shp_in[0], out_sz, shp_in[2])
        x, y = band_input(shp_in, in_sz + axis), band_input(shp_out, out_sz + axis) * 2 - 1
        tag = f"{in_sz}->{out_sz} {method} axis {axis}"
        ax = _apply_band(x, idx, w, out_sz, tag)
        ref, absum = R.band_apply(x, idx, w)
        _report(f"resize_apply {tag}", ax, ref, R.band_tol(absum, idx.shape[1]))
        aty = _apply_band(y, idx_t, w_t, in_sz, tag + " transposed")
        ref_t, absum_t = R.band_apply(y, idx_t, w_t)
        _report(f"resize_apply {tag} transposed", aty, ref_t, R.band_tol(absum_t, idx_t.shape[1]))
        lhs, rhs = float((ax.double() * y.double()).sum()), float((x.double() * aty.double()).sum())
        tol = R.adjoint_tol(x, y, R.dense_band(idx, w, in_sz)[1], max(idx.shape[1], idx_t.shape[1]))
        print(f"[glue] adjoint {tag}: |<Ax,y> - <x,A^T y>| / bound = {abs(lhs - rhs) / tol:.3f}")
        assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize("tag,shape,target", RESIZE2, ids=[c[0] for c in RESIZE2])
def test_resize_matches_reference_fixture(load_golden, tag, shape, target):
    """resize() against the full outputs of the reference's resize_right.resize (tests/golden/clip_resize2.npz): mixed direction, inputs
    shorter than the kernel support, an axis with scale 1.  5e-6 as for the existing fixture: the host tables restated densely in
    float64 are within 1e-6 of it on the CPU (tests/test_glue_bounds_cpu.py), the rest is the kernel's fp32 sums."""
    from perceptor_amd.transforms.resize import resize
    from perceptor_amd.utils.synth import seeded_noise
    want = load_golden("clip_resize2")["rz_" + tag]
    img = seeded_noise(shape, 51) * 0.25 + 0.5
    got = resize(img.to(_dev()), target).cpu()
    assert got.shape == want.shape
    err = float((got - want).abs().max())
    print(f"[glue] resize {tag}: max |got - reference| = {err:.3e}")
    assert err <= 5e-6


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", PATCH_CASES, ids=str)
def test_patchify(case, dtype):
    """(x - mean) / std with the CLIP constants, rounded to 16 bits: |got - ref64| <= 1/2 ulp16(ref64) (1 + 2^-10) + 4 u |ref64|
    (R.patchify_tol: two fp32 roundings, then one to the 16-bit format); the pad columns 3 P^2 .. Kp are exact zeros"""
    N, Rr, P, Kp = case
    img, mean, std = patchify_inputs(case)
    g = Rr // P
    G = _Guarded()
    col = G((N * g * g, Kp), R.TORCH16[dtype])
    d = _dev()
    _call("pmi_patchify", img.to(d), mean.to(d), std.to(d), col, N, Rr, P, Kp, 0, R.DT_CODE[dtype])
    G.verify(f"patchify {case} {dtype}")
    got = col.cpu()
    assert bool((got[:, 3 * P * P:].view(torch.int16) == 0).all()), "pad columns must be +0"
    ref = R.patchify64(img, mean, std, P, Kp)
    _report(f"patchify {case} {dtype}", got, ref, R.patchify_tol(ref, dtype))


def test_patchify_refuses():
    d = _dev()
    img, mean, std = (t.to(d) for t in patchify_inputs(PATCH_CASES[0]))
    col = torch.zeros(2 * 4 * 600, dtype=torch.float16, device=d)
    _refused("pmi_patchify", img, mean, std, col, 2, 28, 14, 590, 0, 0)
    _refused("pmi_patchify", img, mean, std, col, 2, 28, 8, 192, 0, 0)


@pytest.mark.parametrize("case", PATCH_CASES, ids=str)
def test_unpatchify(case):
    """dcol / std * mul is two fp32 roundings: finite (the NaN planted in dcol's pad columns never arrives) and within 3 u |ref64|;
    adjoint of the linear part of patchify: <patchify64(x; mean 0), d> = <x, unpatchify(d)> / mul within 4 u sum |x ref| / mul"""
    N, Rr, P, Kp = case
    dcol, std, mul = unpatchify_inputs(case)
    G = _Guarded()
    dimg = G((N, 3, Rr, Rr))
    d = _dev()
    _call("pmi_unpatchify", dcol.to(d), std.to(d), dimg, N, Rr, P, Kp, mul)
    G.verify(f"unpatchify {case}")
    got = dimg.cpu()
    assert bool(torch.isfinite(got).all())
    ref = R.unpatchify64(dcol, std, N, Rr, P, float(np.float32(mul)))
    _report(f"unpatchify {case}", got, ref, R.unpatchify_tol(ref))
    x = patchify_inputs(case)[0]
    lhs = float((R.patchify64(x, torch.zeros(3), std, P, Kp)[:, :3 * P * P] * dcol.double()[:, :3 * P * P]).sum())
    rhs = float((x.double() * got.double()).sum()) / float(np.float32(mul))
    tol = 4 * R.U * float((x.double() * ref).abs().sum()) / mul
    print(f"[glue] unpatchify adjoint {case}: |lhs - rhs| / bound = {abs(lhs - rhs) / tol:.3f}")
    assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize("with_cc", [False, True])
@pytest.mark.parametrize("with_b", [False, True])
@pytest.mark.parametrize("chw", CHW)
def test_lincomb2(chw, with_b, with_cc):
    """ca[n] a + cb[n] b + cc[n] with three different coefficient sets: at most three fp32 roundings on a path, each relative to a
    partial result below |ca a| + |cb b| + |cc| -> 3 u (|ca a| + |cb b| + |cc|), with or without FMA contraction"""
    a, b, ca, cb, cc = lincomb_inputs(chw)
    d = _dev()
    G = _Guarded()
    out = G((3 * chw,))
    _call("pmi_lincomb2", a.to(d), b.to(d) if with_b else None, ca.to(d), cb.to(d) if with_b else None, cc.to(d) if with_cc else None,
          out, 3, chw)
    G.verify(f"lincomb2 {chw}")
    ref, mag = R.lincomb64(a, b if with_b else None, ca, cb, cc if with_cc else None, chw)
    _report(f"lincomb2 chw {chw} b {with_b} cc {with_cc}", out.cpu(), ref, R.lincomb_tol(mag))


def _quantile(x, q):
    G = _Guarded()
    out = G((x.shape[0],))
    _call("pmi_quantile_abs", x.to(_dev()), out, x.shape[0], x.shape[1], q)
    G.verify(f"quantile n {x.shape[1]} q {q}")
    return out.cpu()


@pytest.mark.parametrize("n", QUANT_N)
def test_quantile_abs(n):
    """rows: N(0, 1) with -0.0 and subnormals, log-uniform over e^-10 .. e^10 with +inf, all equal.  Expected indices from the fp32 rank
    q (n - 1) as the kernel and torch.quantile form it; the order statistics are exact (checked wherever one is returned as it is: w = 0
    or a = b) and the lerp is within 2 u max(|a|, |b|) of a + w (b - a) in float64 (R.quantile_tol: a subtraction, a product and an
    addition on values of at most that magnitude).  q = 1 is bitwise |x|.amax(1)."""
    x = R.quantile_rows(n, 40 + n)
    for q in [0.0, 0.5, 0.95, 1.0] + ([1.0 / (n - 1)] if n > 1 else []):
        got = _quantile(x, q)
        a, b, w, ref = R.quantile_parts(x, q)
        print(f"[glue] quantile n {n} q {q:.6f}: w {w:.6f} got {got.tolist()} ref {ref.tolist()}")
        assert R.quantile_ok(got, a, b, w, ref), f"quantile n {n} q {q}"
    amax = x.abs().amax(1)
    assert torch.equal(_quantile(x, 1.0).view(torch.int32), amax.view(torch.int32))
    assert bool(torch.isinf(amax[1]))


def test_quantile_abs_refuses():
    d = _dev()
    x, out = torch.zeros(3, 8, device=d), torch.zeros(3, device=d)
    for q in (-0.1, 1.5, float("nan")):
        _refused("pmi_quantile_abs", x, out, 3, 8, q)
    _refused("pmi_quantile_abs", x, out, 3, 0, 0.5)


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("n", WASS_N)
def test_wasserstein(n, power):
    """Rows sorted by pmi_sort_rows, then the mean against Normal(0, 1).icdf(linspace(0.5 / n, 1 - 0.5 / n, n)).  Kernel and reference both
    evaluate linspace and erfinv in fp32, so the allowance is MEASURED on the reference, not derived: R.wasserstein_tol evaluates the
    reference's own fp32 torch expression on the CPU against the float64 restatement at these rows and allows four times that error (the
    factor covers another reduction order) plus n u mean for the fp32 sum.  |ref32 - ref64| at these inputs (power 1 / power 2):
    n = 1: 2.0e-08 / 2.1e-08;  n = 2: 1.4e-08 / 4.0e-08;  n = 4097: 2.9e-08 / 6.8e-08 ("Glue kernel tests")."""
    x = R.wasserstein_rows(n, 60 + n)
    npad = _padded(n)
    d = _dev()
    G = _Guarded()
    work, partial, out = G((3, npad)), G((1024,)), G((1,))
    _call("pmi_sort_rows", x.to(d), work, 3, n)
    _call("pmi_wasserstein", work, 3, n, power, partial, out)
    G.verify(f"wasserstein {n} power {power}")
    srt = x.sort(1)[0]
    assert torch.equal(work.cpu()[:, :n], srt)
    tol, err = R.wasserstein_tol(srt, power)
    ref = float(R.wasserstein64(srt, power))
    got = float(out.cpu())
    print(f"[glue] wasserstein n {n} power {power}: got {got:.9g} ref64 {ref:.9g} |ref32 - ref64| {err:.3e} bound {tol:.3e} "
          f"|got - ref64| {abs(got - ref):.3e}")
    assert abs(got - ref) <= tol
