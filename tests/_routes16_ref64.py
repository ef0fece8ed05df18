"""float64 reference, operand regimes and per-element, per-route bounds of the 16-bit (f16 / bf16) routes behind pmi_igemm:
conv3x3_halo_kernel (csrc/conv3x3.hip, tile configs 0-3), conv3x3_wd_kernel (csrc/conv_wd.hip, configs 4 / 6 / 7 / 8), gemm_wd_kernel
(csrc/gemm_wd.hip, GEMM and conv mode), igemm_kernel and splitk_reduce_kernel (csrc/igemm.hip).  Conventions of _precise_ref64.py, whose
conv64 / chain_len / margin are used as they are.

Reference (float64, operands already rounded to the compute type):
    y = act(alpha * conv64(x', w) + bias + nbias) + residual,      x' = x, or with a fused prologue rnd16(act_p(a x + b))
with two sources concatenated along C, nearest-x2 input (up), stride 2 and an up-sampled residual (res_up) as ops.igemm defines them.

Bound, per element (u = 2^-11 f16, 2^-8 bf16; S = |alpha| sum |x'| |w| + |bias| + |nbias|; z the pre-activation value, a = act(z)):
  accumulation  C_B (chain_len(K, splitk) + N_EPI) E32 S.  chain_len: one fp32 rounding per added term, nothing assumed about the MFMA's
                internal order; N_EPI = 3 for the epilogue's own fp32 operations acc * alpha, + bias, + nbias (igemm.hip:315-317 and 440-441,
                conv3x3.hip:297-298, conv_wd.hip:786 and 801, gemm_wd.hip:236 and 319, the reduce kernel igemm.hip:502-506)
  prologue      2 u |alpha| sum |x'| |w|: the kernels' fp32 a x + b and fast exp / rcp SiLU (conv3x3.hip:130, conv_wd.hip:227-249) can land one
                16-bit ulp from the float64 one on any operand (derived in tests/test_gpu_conv_up_phase.py)
  activation    ACT_HW[act] |z| + ACT_LIP[act] (accumulation + prologue)
  residual add  C_B E32 |y|  (one fp32 addition)
  output        one term u |v| for every 16-bit rounding of a value v, plus SUB = 2^-25 where an f16 result may be subnormal
                (|v| < 2^-14: the subnormal grid's half spacing); nothing for an fp32 output beyond the addition above.
How often a route rounds to 16 bit (FORMS below names the form of every route):
  "one"  y rounded once, after the residual:  u |y|
           igemm_kernel's accumulator-layout epilogue (igemm.hip:443-467: the residual is added in fp32, then pack4<T>) -- taken when the
             output is fp32, the residual fp32 or up-sampled, or a pitch / N is not a multiple of 8 (the `fast` predicate, igemm.hip:294-295);
           splitk_reduce_kernel (igemm.hip:509-543) for every split-K route, whichever kernel wrote the slabs;
           conv3x3_halo_kernel config 3 (conv3x3.hip:236-256); gemm_wd_kernel with an fp32 output or an fp32 residual (gemm_wd.hip:319-333);
           the GEGLU epilogue (gemm_wd.hip:203-207: value * gelu(gate) rounded once, no residual).
  "two"  a = act(z) staged as a 16-bit LDS image, the 16-bit residual added to the staged value in fp32 and rounded again:  u (|a| + |y|);
         without a residual the staged image is the output (u |a| = u |y|, the same as "one")
           conv3x3_wd_kernel (conv_wd.hip:789 / 805 pack4<T> into stg, :817-826 unpack8 + residual + pack8)
           conv3x3_halo_kernel configs 0 / 1 / 2 (conv3x3.hip:301 pack4<T> into stg, :326-335)
           gemm_wd_kernel's 16-bit epilogue, GEMM and conv mode (gemm_wd.hip:241 pack4<T> into the image, :263-288)
           igemm_kernel's `fast` epilogue (igemm.hip:319 pack4<T> into stg, :339-348) -- every unsplit 16-bit call with aligned pitches
           whose residual, if any, is 16-bit and not up-sampled.
No constant here is fitted to a measurement; C_B = 1.5 is the suite's (first-order bound, second-order products of roundings).

Regimes (float64 values already rounded to the compute type):
  coherent  all operands positive, [0.5, 1) (weights times 2^-round(log2 K) so that y = O(1)): sum |x||w| = |sum x w|, the bound is as tight as
            it can be and bias / residual are the size of the product
  mixed     random signs, magnitudes [0.5, 1) 2^e with e uniform in -6 .. 6
  tiny      (f16 only) gradient-like inputs 2^-22 .. 2^-13 with random signs: inputs and outputs in f16's subnormal range, where the
            backward path's small elements land after f16_grad_scale
"""
from __future__ import annotations

import math

import torch

import _ref64
from _norm_ref64 import ACT_HW as _ACT_HW, ACT_LIP as _ACT_LIP, ACT_NONE, ACT_RELU, ACT_SILU, C_B, E32  # noqa: F401
from _precise_ref64 import chain_len, conv64, generic_splitk, margin, res_grid  # noqa: F401
from _ref64 import TD, U, rnd  # noqa: F401

ACT_GELU = 3
# exact GELU: fast_erff is Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 (common.h:146-154), halved by the 0.5 x factor, plus four fp32 operations
GELU_HW = 0.5 * 1.5e-7 + 4 * E32
ACT_HW = {**_ACT_HW, ACT_GELU: GELU_HW}
ACT_LIP = {**_ACT_LIP, ACT_GELU: 1.13}          # max |gelu'| = 1.1290
N_EPI = 3
SUB = 2.0 ** -25                                        # half the spacing of f16's subnormal grid
SUB_BELOW = 2.0 ** -14

# the 16-bit rounding form of every route (module doc); "generic" depends on the call: generic_form()
FORMS = {"halo0": "two", "halo1": "two", "halo2": "two", "halo3": "one", "wd4": "two", "wd6": "two", "wd7": "two", "wd8": "two",
         "gemm_wd": "two", "gemm_wd_f32": "one", "geglu": "one", "reduce": "one", "generic_fast": "two", "generic_slow": "one"}


def generic_form(*, out_f32, res, res_up, n_p, ldd, ldr):
    """igemm_kernel's `fast` predicate (igemm.hip:294-295) for a contiguous, 16-byte aligned tensor: which epilogue an unsplit call takes"""
    fast = not out_f32 and not res_up and ldd % 8 == 0 and n_p % 8 == 0 and (res is None or (res == "16" and ldr % 8 == 0))
    return "generic_fast" if fast else "generic_slow"


def act_ref(x: torch.Tensor, act: int) -> torch.Tensor:
    return x if act == ACT_NONE else _ref64.act_ref(x, act)


# ---- operands ---------------------------------------------------------------------------------------------------------------------
def operand(shape, seed, regime, dtype, *, scale=1.0, spread=6):
    """float64 values of one regime, rounded to the compute type (scale: a power of two, so the rounding commutes with it)"""
    g = torch.Generator().manual_seed(seed)
    m = torch.rand(shape, generator=g, dtype=torch.float64) * 0.5 + 0.5
    if regime == "coherent":
        return rnd(m, dtype) * scale
    sign = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0).double()
    if regime == "mixed":
        e = torch.randint(-spread, spread + 1, shape, generator=g).double()
    else:
        assert regime == "tiny" and dtype == "f16"
        e = torch.randint(-22, -12, shape, generator=g).double()
    return rnd(sign * m * 2.0 ** e * scale, dtype)


def pow2(v: float) -> float:
    return 2.0 ** round(math.log2(v))


def weights(shape, seed, regime, dtype):
    """[Cout, Cin, k, k] float64, rounded to the compute type; scaled so that the outputs stay O(1) .. O(100)"""
    K = math.prod(shape[1:])
    if regime == "coherent":
        return operand(shape, seed, "coherent", dtype, scale=1.0 / pow2(K))
    if regime == "mixed":
        return operand(shape, seed, "mixed", dtype, scale=0.25 / pow2(math.sqrt(K)))
    return operand(shape, seed, "mixed", dtype, scale=1.0 / pow2(math.sqrt(K)), spread=2)      # tiny: the inputs carry the scale


# ---- reference and bound -----------------------------------------------------------------------------------------------------------
def prologue_ref(x, ca, cb, pact, dtype):
    """rnd16(act(a x + b)) in float64: per-sample coefficients [N, C] on x [N, H, W, C]"""
    return rnd(act_ref(x * ca.double()[:, None, None, :] + cb.double()[:, None, None, :], pact), dtype)


def out_rounding(v, dtype):
    """bound of one round-to-nearest of v to the 16-bit type"""
    t = U[dtype] * v.abs()
    if dtype == "f16":
        t = t + torch.where(v.abs() < SUB_BELOW, SUB, 0.0)
    return t


def route_ref(x, w, *, dtype, form, K, splitk=1, alpha=1.0, bias=None, nbias=None, residual=None, res_up=False, act=ACT_NONE,
              stride=1, up=False, out_f32=False, prologue=False, flush_floor=None):
    """x [N, H, W, C] (or [M, C]) float64 operand as the MFMAs see it (prologue already applied), w [Cout, C, k, k] float64.
    bias [Cout], nbias [N, Cout], residual at the output grid (its half with res_up), all float64.
    form: a FORMS key.  Returns (y, tol, parts): parts holds z, a, S for the defect models."""
    u = U[dtype]
    conv = conv64(x, w, stride=stride, up=up)
    sxw = abs(alpha) * conv64(x.abs(), w.abs(), stride=stride, up=up)
    z, S = alpha * conv, sxw.clone()
    if bias is not None:
        z, S = z + bias, S + bias.abs()
    if nbias is not None:
        nb = nbias[:, None, None, :] if z.ndim == 4 else nbias
        z, S = z + nb, S + nb.abs()
    z_err = C_B * (chain_len(K, splitk) + N_EPI) * E32 * S
    if prologue:
        z_err = z_err + 2 * u * sxw
    a = act_ref(z, act)
    tol = ACT_HW[act] * z.abs() + ACT_LIP[act] * z_err
    y = a
    if residual is not None:
        y = a + res_grid(residual, res_up)
        tol = tol + C_B * E32 * y.abs()
    if out_f32:
        tol = tol + C_B * E32 * y.abs()
    elif FORMS[form] == "two" and residual is not None:
        tol = tol + out_rounding(a, dtype) + out_rounding(y, dtype)
    else:
        tol = tol + out_rounding(y, dtype)
    if flush_floor is not None:
        tol = tol + flush_floor
    return y, tol, dict(z=z, a=a, S=S, z_err=z_err)


def geglu_ref(x, w, bias, *, dtype, K):
    """the GEGLU epilogue (gemm_wd.hip:196-217) on weights already interleaved by ops.interleave_geglu: per 32 columns 16 value | 16 gate"""
    u = U[dtype]
    w2 = w.reshape(w.shape[0], -1)
    zz = x @ w2.T + bias
    S = x.abs() @ w2.abs().T + bias.abs()
    e = C_B * (chain_len(K, 1) + N_EPI) * E32 * S
    zz, e = zz.reshape(x.shape[0], -1, 2, 16), e.reshape(x.shape[0], -1, 2, 16)
    v, g, ev, eg = zz[:, :, 0], zz[:, :, 1], e[:, :, 0], e[:, :, 1]
    gg = act_ref(g, ACT_GELU)
    y = (v * gg).reshape(x.shape[0], -1)
    tol = gg.abs() * ev + v.abs() * (ACT_LIP[ACT_GELU] * eg + GELU_HW * g.abs())
    tol = tol.reshape(x.shape[0], -1) + C_B * E32 * y.abs() + out_rounding(y, dtype)
    return y, tol


def stats_bound(y, dtype, hw):
    """fused (sum, sum x^2) rows against float64 sums of the route's own 16-bit output y [n, hw, N]: the form of test_precise_igemm_route with the
    16-bit u (the kernels sum the values before their last rounding: within u |y| of the stored ones, 2 u y^2 for the squares)"""
    u = U[dtype]
    out = []
    for yy in (y, y * y):
        out.append((yy.sum(1), C_B * (hw * E32 + 2 * u) * yy.abs().sum(1) + hw * SUB * (1 + 2 * y.abs().max())))
    return out


# ---- fp32 emulation of a route (tests/test_routes16_bounds_cpu.py) ----------------------------------------------------------------
def emulate(x, w, *, dtype, form, chunk=128, alpha=1.0, bias=None, nbias=None, residual=None, res_up=False, act=ACT_NONE, stride=1,
            up=False, out_f32=False, trunc=False, chunk_round=False, force_two=False):
    """fp32 products summed in chunk order (per tap, `chunk` channels at a time), then the route's roundings with torch's round-to-nearest
    casts.  Seeded defects: trunc (the last rounding truncates toward zero), chunk_round (the running sum rounded to 16 bit after every
    chunk), force_two (the two-rounding arithmetic whatever the form)."""
    td = TD[dtype]
    xf, wf = x.float(), w.float()
    C = xf.shape[-1]
    k = wf.shape[-1] if wf.ndim == 4 else 1
    acc = None
    for ty in range(k):
        for tx in range(k):
            for c0 in range(0, C, chunk):
                wm = torch.zeros_like(wf)
                if wf.ndim == 4:
                    wm[:, c0:c0 + chunk, ty, tx] = wf[:, c0:c0 + chunk, ty, tx]
                else:
                    wm[:, c0:c0 + chunk] = wf[:, c0:c0 + chunk]
                p = conv64(xf.double(), wm.double(), stride=stride, up=up).float()       # exact products, one fp32 rounding per chunk
                acc = p if acc is None else acc + p
                if chunk_round:
                    acc = acc.to(td).float()
    z = acc * torch.tensor(alpha, dtype=torch.float32)
    if bias is not None:
        z = z + bias.float()
    if nbias is not None:
        z = z + (nbias.float()[:, None, None, :] if z.ndim == 4 else nbias.float())
    a = act_ref(z.double(), act).float()
    two = FORMS[form] == "two" or force_two

    def last(v):
        if out_f32:
            return v.double()
        r = v.to(td)
        if trunc:       # one step toward zero where the nearest value lies further out: the bit pattern minus one (sign-magnitude)
            away = r.double().abs() > v.double().abs()
            r = (r.view(torch.int16) - away.to(torch.int16)).view(td)
        return r.double()

    if residual is None:
        return last(a)
    r = res_grid(residual, res_up).float()
    if two and not out_f32:
        a = a.to(td).float()
    return last(a + r)
