"""float64 references, operand regimes, per-element bounds, fp32 emulations and defect models of the kernel paths only dtype='mixed' runs:
conv3x3_wd_kernel's split-input staging (csrc/conv_wd.hip SIN = 1: doubled operand, SIN = 2: single operand; tile configs 6 / 7) with the
split epilogue, its fallback (apply pass + generic split convolution), and the attention projection from plain f16 operands back onto the
split stream (ops.igemm(plain, plain weights, residual=split, split_out=True)).  Conventions and constants of _precise_ref64.py,
_routes16_ref64.py and _norm_ref64.py; no constant here is fitted to a measurement.

Common to the convolution routes: the logical input is v = hi + lo, the operand p = silu(a v + b) with fp32 coefficients a, b per sample
and channel, and zero padding AFTER the activation; y = conv(p', w) + bias + nbias + residual, stored as a hi + lo pair.

What the device does to one operand element (conv_wd.hip unpack_piece / finish_piece; the apply pass of the fallback does the same in
plain fp32): v32 = hi + lo (one rounding, E32 |v|), the coefficients times -log2(e) (one rounding each), u = fma(v32, a', b') (one
rounding), p = u rcp(fma(exp2(u), k, k)) (ACT_HW[SiLU] relative).  Against the float64 u:
    du    = E32 (2 |a v| + |b| + |u|)
    delta = C_B ((|silu'(u)| + 0.5 du) du + ACT_HW |p|)            local slope; 0.5 = max |silu''| (ACT_LIP2) covers the interval u +- du
The local slope matters: with the global 1.1 every small negative output (silu' ~ 0 near u = -1.28, outputs on f16's finest grids) would
count as uncertain.

Doubled operand (split_in 1, and every fallback): p32 is split again, yh = f16(p32), yl = f16(p32 - yh).  The reference multiplies the
float64 p;   tol = C_B (chain_len(18 Cin) + N_EPI) E32 S + conv(tin, |w|) + epilogue,
tin = delta + C_B (U_SPLIT |p| + SPLIT_FLOOR) (+ SUB where |p| < 2^-14: yh is then subnormal and yl cannot hold what it lost).

Single operand (split_in 2): the reference operand is x' = rnd_f16(p) computed from the float64 p.  The device's fp32 value can round to
the NEIGHBOURING f16 only where p lies within delta of a rounding midpoint; those elements are marked `amb` and the prologue term is
conv(amb ulp16(x'), |w|) -- not the blanket 2 u sum |x'| |w| of the 16-bit routes, which is what hides a dropped low part.
    tol = C_B (chain_len(9 Cin) + N_EPI) E32 S + conv(amb ulp16(x'), |w|) + epilogue
Every case asserts its amb share (AMB_CAP): a case that marks more than 1 % (10 % in the wide regime) would be a bound with a hole in it.

Epilogue (conv_wd.hip split epilogue, igemm.hip generic / reduce epilogues): acc + (bias + nbias) in fp32 (N_EPI), the residual either a
split pair (two fp32 additions: 2 E32 (|z| + |r|)) or fp32 (one: E32 |y|), through res_grid when up-sampled; the fallback converts an fp32
residual to a pair first (U_SPLIT |r| + SPLIT_FLOOR).  Output: U_SPLIT |y| + SPLIT_FLOOR.  Fused statistics: test_precise_igemm_route's
form against float64 sums of the kernel's own output (stats_check).

Projection: f16 operands, K-term chain (chain_len(K, splitk): slabs + reduce under split-K), + bias, the split residual in fp32, split out.

Regimes:
  coherent      inputs P.coherent_hi_lo (positive, lo the sign of hi), coefficients positive: p > 0, positive weights: S = |y|, the bound is as
                tight as it gets and a dropped INPUT low part moves every term the same way
  coherent_act  the same one stage later: inputs chosen (silu inverted in float64) so that p = ph (1 + r 2^-12) with ph on f16's grid and
                r in [0.6, 0.95] -- the low parts yl the doubled staging forms all have the sign of yh.  In `coherent` the yl are the
                rounding residuals of arbitrary values, uniform within half an ulp of yh: relative rms between 2^-12 / sqrt(3) and
                2^-11 / sqrt(3).  A dropped yl is then a random-sign sum of 9 Cin terms, rms (1.4 .. 2.8)e-4 / sqrt(9 Cin) of S, against
                the accumulation term C_B (18 Cin + N_EPI) E32 of S.  Cin = 32: (0.8 .. 1.7)e-5 against 5.2e-5, the largest of a few
                thousand outputs lands at the edge of the bound; Cin = 8: (1.7 .. 3.3)e-5 against 1.3e-5, clearly outside -- where
                the CPU test asserts the defect in `coherent`.  coherent_act rejects it at any Cin of the GPU cases.
  mixed         P.mixed_hi_lo normal inputs, a ~ 1 + 0.2 N, b ~ 0.3 N
  wide          inputs x4: u = a v + b has std ~ 5 and spans +-16; SiLU outputs reach f16's subnormals (yh, yl, pack8 of tiny values)
In every regime b has entries of magnitude >= 1 (silu(b) in a padding pixel is O(1)) and the samples' coefficients differ by O(1).
"""
from __future__ import annotations

import math

import torch

import _precise_ref64 as P
from _norm_ref64 import ACT_HW, ACT_SILU, C_B, E32, SPLIT_FLOOR, from_split16  # noqa: F401
from _precise_ref64 import U_SPLIT, chain_len, conv64, generic_splitk, join_split, margin, parts, res_grid  # noqa: F401
from _routes16_ref64 import N_EPI, SUB, SUB_BELOW, pow2

AMB_CAP = {"coherent": 0.01, "coherent_act": 0.01, "mixed": 0.01, "wide": 0.10}
WIDE_SCALE = 4.0


def silu64(u):
    return u * torch.sigmoid(u)


def silu_grad64(u):
    s = torch.sigmoid(u)
    return s * (1 + u * (1 - s))


def silu_inverse(p):
    """u > 0 with silu(u) = p for p > 0 (float64 Newton; silu is increasing and convex there)"""
    u = p + 0.7
    for _ in range(60):
        u = u - (silu64(u) - p) / silu_grad64(u)
    return u


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def coefficients(n, cin, seed, regime):
    """fp32 a, b [n, cin]: entries of |b| >= 1 in every regime, and an O(1) difference between the samples"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.arange(n, dtype=torch.float32)[:, None]
    if regime.startswith("coherent"):
        a = 0.5 + torch.rand((n, cin), generator=g) + 0.5 * idx
        b = 0.5 + torch.rand((n, cin), generator=g) + 0.5 * idx
        return a, b
    a = (1 + 0.2 * torch.randn((n, cin), generator=g)) * (1 + 0.5 * idx)
    b = (1.5 if regime == "wide" else 0.3) * torch.randn((n, cin), generator=g)
    sign = torch.where(torch.rand((n, cin), generator=g) < 0.5, -1.0, 1.0)
    b[:, ::4] += 1.5 * sign[:, ::4]
    return a, b + 0.7 * idx * sign


def build_inputs(cs):
    """CPU operands of one convolution case (the GPU test and the CPU bound tests build theirs here).  cs: n, h, w (input grid), srcs
    (logical channels per source), cout, up, res (None / "split" / "f32"), res_up, nbias, regime, seed."""
    seed, reg = cs["seed"], cs["regime"]
    n, cin, cout = cs["n"], sum(cs["srcs"]), cs["cout"]
    lead = (n, cs["h"], cs["w"])
    a, b = coefficients(n, cin, seed * 100 + 14, reg)
    his, los, o = [], [], 0
    for i, c in enumerate(cs["srcs"]):
        if reg == "coherent":
            hi, lo = P.coherent_hi_lo(lead + (c,), seed * 100 + i)
        elif reg == "coherent_act":
            ph, r = P.coherent_hi_lo(lead + (c,), seed * 100 + i, scale=2.0)
            r = r.double() / ph.double() * 2.0 ** 12                                # the generator's r in [0.6, 0.95] (to f16's accuracy)
            u = silu_inverse(ph.double() * (1 + r * 2.0 ** -12))
            v = ((u - b[:, None, None, o:o + c].double()) / a[:, None, None, o:o + c].double()).float()
            hi = v.half()
            lo = (v - hi.float()).half()
        else:
            hi, lo = P.mixed_hi_lo(lead + (c,), seed * 100 + i, WIDE_SCALE if reg == "wide" else 1.0)
        his.append(hi)
        los.append(lo)
        o += c
    wreg = "coherent" if reg.startswith("coherent") else "mixed"
    w = P.weights((cout, cin, 3, 3), seed * 100 + 10, wreg, "f16")
    bias = P.vector(cout, seed * 100 + 11, wreg)
    nbias = P.vector(n * cout, seed * 100 + 12, wreg).view(n, cout) if cs["nbias"] else None
    res = rh = rl = None
    if cs["res"]:
        ho, wo = (2 * cs["h"], 2 * cs["w"]) if cs["up"] else (cs["h"], cs["w"])
        rshape = (n, ho // 2, wo // 2, cout) if cs["res_up"] else (n, ho, wo, cout)
        scale = pow2(9 * cin) if wreg == "coherent" else 1.0                    # the residual the size of the product
        if cs["res"] == "split":
            rh, rl = (P.coherent_hi_lo if wreg == "coherent" else P.mixed_hi_lo)(rshape, seed * 100 + 13, scale)
            res = join_split(rh, rl)
        else:
            res = P.vector(math.prod(rshape), seed * 100 + 13, wreg, scale).view(rshape)
    return dict(srcs=[join_split(h_, l_) for h_, l_ in zip(his, los)], hi=torch.cat(his, -1).double(), lo=torch.cat(los, -1).double(),
                a=a, b=b, w=w, bias=bias, nbias=nbias, res=res, res_hi=rh, res_lo=rl)


# ---- the operand and its uncertainty --------------------------------------------------------------------------------------------------
def activated(d):
    """float64 p = silu(a v + b) of the logical input and delta, the bound of the device's fp32 value against it (module doc)"""
    v = d["hi"] + d["lo"]
    a, b = d["a"].double()[:, None, None, :], d["b"].double()[:, None, None, :]
    u = a * v + b
    p = silu64(u)
    du = E32 * (2 * (a * v).abs() + b.abs() + u.abs())
    delta = C_B * ((silu_grad64(u).abs() + 0.5 * du) * du + ACT_HW[ACT_SILU] * p.abs())
    return p, delta


def ulp16(x):
    """spacing of the f16 grid at |x| (x on the grid), subnormals included"""
    _, e = torch.frexp(x.abs().clamp_min(2.0 ** -24))
    return torch.ldexp(torch.ones_like(x), (e - 1).clamp_min(-14) - 10)


def ambiguous(p, delta):
    """x' = rnd_f16(p), its grid spacing, and the mask of the elements whose fp32 value (within delta of p) may round to the other
    neighbour: p within delta of the midpoint on its side of x'.  Below a power of two the grid is twice as fine."""
    x = p.half().double()
    ulp = ulp16(x)
    m, e = torch.frexp(x.abs())
    inner = (p.abs() < x.abs()) & (m == 0.5) & (e - 1 > -14)
    side = torch.where(inner, ulp / 2, ulp)
    return x, ulp, (side / 2 - (p - x).abs()) <= delta


# ---- references and bounds ------------------------------------------------------------------------------------------------------------
def conv_ref(d, cs, operand, *, fallback=False, splitk=1):
    """(y, tol, info) of one conv3x3_mixed call.  operand "single" / "dbl"; fallback: the apply pass + split convolution (doubled
    arithmetic whatever the operand; an fp32 residual converted to a pair first); splitk: of the fallback's generic kernel."""
    p, delta = activated(d)
    w = d["w"].double()
    cin, up = sum(cs["srcs"]), cs["up"]
    if operand == "dbl" or fallback:
        x, K = p, 18 * cin
        tin = delta + C_B * (U_SPLIT * p.abs() + SPLIT_FLOOR) + torch.where(p.abs() < SUB_BELOW, SUB, 0.0)
        pro, share = conv64(tin, w.abs(), up=up), 0.0
    else:
        x, ulp, amb = ambiguous(p, delta)
        K = 9 * cin
        pro, share = conv64(amb.double() * ulp, w.abs(), up=up), float(amb.double().mean())
    z = conv64(x, w, up=up) + d["bias"].double()
    S = conv64(x.abs(), w.abs(), up=up) + d["bias"].double().abs()
    if d["nbias"] is not None:
        nb = d["nbias"].double()[:, None, None, :]
        z, S = z + nb, S + nb.abs()
    err = (chain_len(K, splitk) + N_EPI) * E32 * S
    y = z
    if d["res"] is not None:
        r = res_grid(from_split16(d["res"]) if cs["res"] == "split" else d["res"].double(), cs["res_up"])
        y = z + r
        if cs["res"] == "split" or fallback:
            err = err + 2 * E32 * (z.abs() + r.abs())
        else:
            err = err + E32 * y.abs()
        if cs["res"] == "f32" and fallback:
            err = err + U_SPLIT * r.abs() + SPLIT_FLOOR
    tol = C_B * (err + U_SPLIT * y.abs() + SPLIT_FLOOR) + pro
    return y, tol, dict(amb=share, p=p, x=x, S=S, pro=pro)


def stats_check(st, got, n):
    """fused (sum, sum of squares) rows against float64 sums of the kernel's own output (test_precise_igemm_route's form): the largest
    err / tol of the two"""
    s = st.double().cpu().sum(1)                                # [n, N, 2]
    y = got.reshape(n, -1, got.shape[-1])
    hw = y.shape[1]
    worst = 0.0
    for j, yy in enumerate((y, y * y)):
        tol = C_B * (hw * E32 + 2 * U_SPLIT) * yy.abs().sum(1) + hw * SPLIT_FLOOR * (1 + 2 * y.abs().max())
        worst = max(worst, float(((s[..., j] - yy.sum(1)).abs() / tol).max()))
    return worst


def proj_inputs(cs):
    """plain f16 rows [M, K], f16-exact weights [N, K], bias, split residual (hi, lo) [M, N]; res_scale: a power of two on the residual"""
    g = torch.Generator().manual_seed(cs["seed"])
    M, K, N = cs["m"], cs["k"], cs["n"]
    if cs["regime"] == "coherent":
        x = (torch.rand((M, K), generator=g) * 0.5 + 0.5).half()
        w = P.weights((N, K, 1, 1), cs["seed"] + 1, "coherent", "f16") / pow2(K)
        rh, rl = P.coherent_hi_lo((M, N), cs["seed"] + 2, cs["res_scale"])
    else:
        x = torch.randn((M, K), generator=g).half()
        w = P.weights((N, K, 1, 1), cs["seed"] + 1, "mixed", "f16")
        rh, rl = P.mixed_hi_lo((M, N), cs["seed"] + 2, cs["res_scale"])
    bias = P.vector(N, cs["seed"] + 3, "mixed")
    return dict(x=x, w=w, bias=bias, res_hi=rh, res_lo=rl, res=join_split(rh, rl))


def proj_ref(d, splitk=1):
    x, w = d["x"].double(), d["w"].reshape(d["w"].shape[0], -1).double()
    z = x @ w.T + d["bias"].double()
    S = x.abs() @ w.abs().T + d["bias"].double().abs()
    r = d["res_hi"].double() + d["res_lo"].double()
    y = z + r
    tol = C_B * ((chain_len(x.shape[1], splitk) + N_EPI) * E32 * S + 2 * E32 * (z.abs() + r.abs()) + U_SPLIT * y.abs() + SPLIT_FLOOR)
    return y, tol


# ---- fp32 emulation of the routes, with seeded defects (tests/test_mixed_bounds_cpu.py) -----------------------------------------------
def _split32(z):
    hi = z.half()
    return hi, (z - hi.float()).half()


def _finite(t):
    """a defect's garbage kept inside f16's range, so that it shows as an error and not as a NaN no comparison sees"""
    return torch.nan_to_num(t, nan=3e4, posinf=3e4, neginf=-3e4).clamp(-3e4, 3e4)


def _residual32(d, cs, z, *, res_drop_lo=False, res_f32_as_split=False):
    """z + residual in fp32 as the epilogues add it"""
    if d["res"] is None:
        return z
    if cs["res"] == "split":
        rh, rl = d["res_hi"].float(), d["res_lo"].float()
        r = rh if res_drop_lo else rh + rl
    elif res_f32_as_split:      # the fp32 rows' bytes (N fp32 = 2 N 16-bit words) read as [hi 32 | lo 32] f16 groups
        hi, lo = parts(d["res"].contiguous().view(torch.float16))
        r = _finite((hi + lo).float())
    else:
        r = d["res"]
    return z + res_grid(r, cs["res_up"])


def emulate_conv(d, cs, operand, *, chunk=32, drop_in_lo=False, drop_yl=False, pad_silu=False, same_coef=False, coef_shift=False,
                 trunc=False, res_drop_lo=False, res_f32_as_split=False, out_drop_lo=False):
    """hi + lo and the fma in fp32, SiLU as u / (1 + exp(-u)) in fp32, roundings by torch casts, exact products summed in fp32 per tap and
    chunk (yh then yl for the doubled operand), the split epilogue.  Returns the logical float64 output.  Defects (module doc of the test):
    drop_in_lo, drop_yl, pad_silu (padding pixels hold silu(b)), same_coef (sample 0's coefficients for all), coef_shift (the second
    source's coefficients read at the physical offset 2 C0), trunc (single: the operand rounding truncates toward zero), res_drop_lo,
    res_f32_as_split, out_drop_lo."""
    hi, lo = d["hi"].float(), d["lo"].float()
    v = hi if drop_in_lo else hi + lo
    a, b = d["a"].clone(), d["b"].clone()
    if same_coef:
        a[1:], b[1:] = a[0], b[0]
    if coef_shift:
        c0, cin = cs["srcs"][0], sum(cs["srcs"])
        for t in (a, b):
            src = torch.zeros_like(t[:, c0:])
            if 2 * c0 < cin:
                src[:, :cin - 2 * c0] = t[:, 2 * c0:]
            t[:, c0:] = src
    silu32 = lambda u: u / (1 + torch.exp(-u))               # noqa: E731
    p = silu32(torch.addcmul(b[:, None, None, :], v, a[:, None, None, :]))
    crop = False
    if pad_silu:
        assert not cs["up"]
        n, h, w_, c = p.shape
        pp = silu32(b)[:, None, None, :].expand(n, h + 2, w_ + 2, c).clone()
        pp[:, 1:-1, 1:-1] = p
        p, crop = pp, True
    if operand == "single":
        x = p.half()
        if trunc:
            away = x.double().abs() > p.double().abs()
            x = (x.view(torch.int16) - away.to(torch.int16)).view(torch.float16)
        xs = [x]
    else:
        yh, yl = _split32(p)
        xs = [yh] if drop_yl else [yh, yl]
    wf = d["w"].float()
    acc = None
    for c0 in range(0, wf.shape[1], chunk):
        for ty in range(3):
            for tx in range(3):
                wm = torch.zeros_like(wf)
                wm[:, c0:c0 + chunk, ty, tx] = wf[:, c0:c0 + chunk, ty, tx]
                for x in xs:
                    q = conv64(x.double(), wm.double(), up=cs["up"]).float()
                    acc = q if acc is None else acc + q
    if crop:
        acc = acc[:, 1:-1, 1:-1]
    bsum = d["bias"].float()[None, None, None, :]
    if d["nbias"] is not None:
        bsum = bsum + d["nbias"].float()[:, None, None, :]
    z = _residual32(d, cs, acc + bsum, res_drop_lo=res_drop_lo, res_f32_as_split=res_f32_as_split)
    oh, ol = _split32(z)
    return oh.double() if out_drop_lo else oh.double() + ol.double()


def emulate_proj(d, *, chunk=64, splitk=1, res_groups_swapped=False, res_drop_lo=False, out_drop_lo=False):
    """the projection in fp32: exact f16 products summed per chunk (per slab, then the slabs, under split-K), bias, hi then lo of the
    residual, split store.  res_groups_swapped: the residual read as [hi N | lo N] instead of [hi 32 | lo 32] per group."""
    x, w = d["x"].double(), d["w"].reshape(d["w"].shape[0], -1).double()
    K = x.shape[1]
    per = -(-K // splitk)
    slabs = []
    for s0 in range(0, K, per):
        acc = torch.zeros((x.shape[0], w.shape[0]))
        for c0 in range(s0, min(s0 + per, K), chunk):
            c1 = min(c0 + chunk, s0 + per, K)
            acc = acc + (x[:, c0:c1] @ w[:, c0:c1].T).float()
        slabs.append(acc)
    z = slabs[0]
    for s in slabs[1:]:
        z = z + s
    z = z + d["bias"].float()
    rh, rl = d["res_hi"].float(), d["res_lo"].float()
    if res_groups_swapped:
        N = rh.shape[-1]
        phys = d["res"].float()
        rh, rl = phys[:, :N], phys[:, N:]
    z = z + rh
    if not res_drop_lo:
        z = z + rl
    oh, ol = _split32(z)
    return oh.double() if out_drop_lo else oh.double() + ol.double()
