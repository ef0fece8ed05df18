"""float64 restatement, bounds and defect models of the precise-mode (dtype 2: hi + lo f16 pairs) GEMMs and convolutions
(csrc/igemm.hip generic kernel + split-K reduce, csrc/conv_wd.hip configs 6 / 7 / 8, csrc/conv3x3.hip config 3 plain_k,
csrc/f32gemm.hip) and of the split conversions (csrc/elementwise.hip).  Same conventions as _norm_ref64.py.

What the kernels multiply (ops.PackedLinear, dt = DT_F16X2): the input is a split tensor (hi, lo per logical channel, groups of
G = ops.split_group(C) channels), the f16 weights W_hi = f16(W) are duplicated along K, and fp32 weights that f16 cannot hold get
W_lo = f16(W - W_hi) as a second K block over the same input with its lo half zeroed (self_concat).  Exact reference:
    y = act( sum W_hi (x_hi + x_lo) + sum W_lo x_hi + b (+ nbias) ) (+ residual as hi + lo, or fp32)
Contract reference: the true fp32 weights times the logical value hi + lo.  The two differ by sum W_lo x_lo (dropped) and by what
W_lo = f16(W - W_hi) does not hold (relative 2^-11 of W_lo, or absolute 2^-25 where W_lo is an f16 subnormal):
    |exact - contract| <= 2 * 2^-22 * sum |W x| + 2^-25 * sum |x|            (CONTRACT_REL, CONTRACT_ABS below)

Bounds, elementwise |got - ref| <= tol:
  accumulation  every f16 x f16 product is exact in fp32 (11 + 11 significant bits); nothing is assumed about the MFMA's internal
                order or width beyond at most one fp32 rounding per added term, so an accumulator that receives L terms is off by at
                most L E32 sum|p|.  L = K (physical K, the self_concat block included) for one accumulator over the whole K -- the
                generic kernel (BK = 64 per step, one accumulator per output across all steps) and the weights-direct configs alike;
                split-K: ceil(K / S) per slab plus S for the reduce kernel's fp32 sum of the slabs.
  epilogue      one fp32 rounding per op: bias, nbias (E32 of the running sum), residual (hi + lo summed, then added: 2 E32 of
                |act| + |r|); SiLU: ACT_HW relative; ReLU exact.
  output        split: 2^-22 |y| + 2^-25 (UN / SPLIT_FLOOR); fp32: E32 |y|.
  tol = C_B * (the sum above).

Tight regime (COHERENT): a worst-case bound on mixed-sign data is too loose at long K to see a lost lo part.  With non-negative
weights and inputs whose lo parts all have the sign of their hi parts (hi in [0.5, 1), lo = f16(hi * r * 2^-12), r in [0.6, 0.95])
sum |W x| = |y|, and a dropped low part moves y by ~1.6e-4 relative -- several bounds at the K of the defect cases.
"""
from __future__ import annotations

import math
from fractions import Fraction

import torch
import torch.nn.functional as F

from _norm_ref64 import ACT_HW, ACT_LIP, ACT_NONE, ACT_RELU, ACT_SILU, C_B, E32, SPLIT_FLOOR, UN, act_ref, from_split16  # noqa: F401

U_SPLIT = UN["precise"]
CONTRACT_REL = 2.0 * 2.0 ** -22
CONTRACT_ABS = 2.0 ** -25


# ---- split tensors with an explicit grouping ---------------------------------------------------------------------------------------
def group_of(c: int) -> int:
    """ops.split_group restated (device: common.h split_group)"""
    if c % 32 == 0:
        return 32
    assert c <= 32 and c % 8 == 0, c
    return c


def join_split(hi: torch.Tensor, lo: torch.Tensor) -> torch.Tensor:
    """(hi, lo) f16 [..., C] -> the physical [..., 2C] f16 layout (groups of group_of(C)).  Unlike _norm_ref64.to_split16, which derives
    lo = f16(x - hi) from a float, the parts are given: the coherent operands choose their lo parts."""
    C = hi.shape[-1]
    G = group_of(C)
    sh = hi.shape[:-1] + (C // G, G)
    return torch.stack([hi.reshape(sh), lo.reshape(sh)], -2).reshape(hi.shape[:-1] + (2 * C,))


def parts(t: torch.Tensor):
    """physical [..., 2C] -> (hi, lo) float64 [..., C] (_norm_ref64.from_split16 gives their sum)"""
    C = t.shape[-1] // 2
    G = group_of(C)
    v = t.double().reshape(t.shape[:-1] + (C // G, 2, G))
    return v[..., 0, :].reshape(t.shape[:-1] + (C,)), v[..., 1, :].reshape(t.shape[:-1] + (C,))


# ---- operands of the two regimes ---------------------------------------------------------------------------------------------------
def coherent_hi_lo(shape, seed, scale=1.0):
    """hi in [0.5, 1) * scale (f16), lo = f16(hi * r * 2^-12), r in [0.6, 0.95]: lo below half an ulp of hi, same sign"""
    g = torch.Generator().manual_seed(seed)
    hi = ((torch.rand(shape, generator=g) * 0.5 + 0.5) * scale).half()
    r = torch.rand(shape, generator=g) * 0.35 + 0.6
    lo = (hi.float() * r * 2.0 ** -12).half()
    return hi, lo


def mixed_hi_lo(shape, seed, scale=1.0):
    """fp32 normal values split as the kernels split them: hi = f16(x), lo = f16(x - hi)"""
    x = torch.randn(shape, generator=torch.Generator().manual_seed(seed)) * scale
    hi = x.half()
    return hi, (x - hi.float()).half()


def weights(shape, seed, regime, kind, scale=None):
    """fp32 weights [Cout, Cin, kh, kw]: kind "f16" (exactly f16-representable) or "f32" (a low part f16 cannot hold).
    coherent: positive, W = W_hi (1 + r 2^-12); mixed: normal * scale (default 1 / sqrt(fan-in))."""
    g = torch.Generator().manual_seed(seed)
    if regime == "coherent":
        hi = (torch.rand(shape, generator=g) * 0.5 + 0.5).half().float()
        if kind == "f16":
            return hi
        r = torch.rand(shape, generator=g) * 0.35 + 0.6
        return hi * (1 + r * 2.0 ** -12)
    fan = math.prod(shape[1:])
    w = torch.randn(shape, generator=g) * (scale if scale is not None else fan ** -0.5)
    return w.half().float() if kind == "f16" else w


def vector(n, seed, regime, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    if regime == "coherent":
        return (torch.rand(n, generator=g) * 0.5 + 0.5) * scale
    return torch.randn(n, generator=g) * scale


# ---- the weight parts the kernel multiplies -------------------------------------------------------------------------------------
def weight_parts(w: torch.Tensor, self_concat: bool):
    """W_hi = f16(W), W_lo = f16(W - W_hi) (zero unless the layer carries the second K block), float64"""
    w = w.float()
    hi = w.half().float()
    lo = (w - hi).half().double() if self_concat else torch.zeros_like(hi, dtype=torch.float64)
    return hi.double(), lo


# ---- geometry ------------------------------------------------------------------------------------------------------------------
def conv64(v: torch.Tensor, w: torch.Tensor, *, stride=1, up=False) -> torch.Tensor:
    """v [N, H, W, C] (or [M, C] for a linear) float64, w [Cout, C, k, k] -> [N, h, w, Cout]: the implicit GEMM of ops.igemm
    (k = 3: zero padding 1; up: nearest x2 of the input first; stride 2: pixel (2y + dy, 2x + dx))."""
    if v.ndim == 2:
        return v @ w.reshape(w.shape[0], -1).double().T
    x = v.permute(0, 3, 1, 2)
    if up:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    k = w.shape[-1]
    y = F.conv2d(x, w.double(), stride=stride, padding=k // 2)
    return y.permute(0, 2, 3, 1)


def res_grid(r: torch.Tensor, res_up: bool) -> torch.Tensor:
    return r.repeat_interleave(2, 1).repeat_interleave(2, 2) if res_up else r


def precise_ref(x_hi, x_lo, w, *, self_concat, bias=None, nbias=None, residual=None, res_up=False, act=ACT_NONE,
                stride=1, up=False, split_out=True, chain=None):
    """Exact and contract references and the bound of one precise convolution / linear.
    x_hi, x_lo: float64 logical tensors [N, H, W, C] (sources already concatenated); w: fp32 weights [Cout, C, k, k];
    bias [Cout] fp32, nbias [N, Cout] fp32, residual: float64 logical value at the output grid (or its half when res_up);
    chain: accumulation depth (see module doc).  Returns (exact, contract, tol, tol_contract, sabs)."""
    wh, wl = weight_parts(w, self_concat)
    v = x_hi + x_lo
    acc = conv64(v, wh, stride=stride, up=up) + conv64(x_hi, wl, stride=stride, up=up)
    sabs = conv64(v.abs(), wh.abs(), stride=stride, up=up) + conv64(x_hi.abs(), wl.abs(), stride=stride, up=up)
    acc_c = conv64(v, w.double(), stride=stride, up=up)
    sabs_c = conv64(v.abs(), w.double().abs(), stride=stride, up=up)
    xsum = conv64(v.abs(), torch.ones_like(w, dtype=torch.float64), stride=stride, up=up)

    def epi(z):
        extra = torch.zeros_like(z)
        if bias is not None:
            z = z + bias.double()
            extra = extra + bias.double().abs()
        if nbias is not None:
            nb = nbias.double()
            nb = nb[:, None, None, :] if z.ndim == 4 else nb
            z = z + nb
            extra = extra + nb.abs()
        return z, extra

    z, extra = epi(acc)
    zc, _ = epi(acc_c)
    a, ac = act_ref(z, act), act_ref(zc, act)
    n_add = int(bias is not None) + int(nbias is not None)
    z_err = chain * E32 * sabs + n_add * E32 * (sabs + extra)
    y_err = ACT_LIP[act] * z_err + ACT_HW[act] * a.abs()
    y, yc = a, ac
    if residual is not None:
        r = res_grid(residual.double(), res_up)
        y, yc = a + r, ac + r
        y_err = y_err + 2 * E32 * (a.abs() + r.abs())
    out = (U_SPLIT * y.abs() + SPLIT_FLOOR) if split_out else E32 * y.abs()
    tol = C_B * (y_err + out)
    tol_c = tol + ACT_LIP[act] * (CONTRACT_REL * sabs_c + CONTRACT_ABS * xsum)
    return y, yc, tol, tol_c, sabs


def chain_len(K: int, splitk: int) -> int:
    """accumulation depth of one output (module doc): K terms, or ceil(K / S) per slab + S for the reduce"""
    return K if splitk <= 1 else -(-K // splitk) + splitk


def generic_splitk(M: int, N: int, K: int) -> int:
    """pmi_igemm_splitk for the generic kernel (igemm.hip, BM = BN = 128, BK = 64), restated"""
    tiles = -(-M // 128) * -(-N // 128)
    nk = -(-K // 64)
    if tiles >= 384 or nk < 16:
        return 1
    s = min(512 // tiles, nk // 8, 16)
    return s if s >= 2 else 1


def margin(got: torch.Tensor, ref: torch.Tensor, tol: torch.Tensor) -> float:
    """max |got - ref| / tol"""
    err = (got.double() - ref.double()).abs()
    return float(torch.where(err == 0, torch.zeros_like(err), err / tol).max())


# ---- exact fp32 rounding for the gemm_f32 emulation ----------------------------------------------------------------------------
def round_f32(q: Fraction) -> Fraction:
    """q rounded to the nearest fp32 (ties to even), subnormals included; no overflow handling (the tests stay in range)"""
    if q == 0:
        return Fraction(0)
    s = -1 if q < 0 else 1
    a = abs(q)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    e = max(e, -126)                       # 2^e <= a < 2^(e+1) (or the subnormal range)
    scale = Fraction(2) ** (e - 23)
    m = a / scale
    fl = m.numerator // m.denominator
    rem = m - fl
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and fl % 2):
        fl += 1
    return s * fl * scale


def fma_chain_f32(a_row, b_col) -> float:
    """acc = fmaf(a_k, b_k, acc) for k = 0, 1, ... from acc = 0, exactly (a_k, b_k fp32 values as Python floats)"""
    acc = Fraction(0)
    for x, y in zip(a_row, b_col):
        acc = round_f32(Fraction(x) * Fraction(y) + acc)
    return float(acc)
