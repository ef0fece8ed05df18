"""float64 restatement of MonsterDiffusion's input gradient (engine/monster.py forward_train / backward), in this file's own words, on top of
tests/_monster_ref64.py; checked against the reference's autograd values in tests/golden/monster_diffusion_grad_reference.npz by
tests/test_monster_grad_cpu.py.

Backward, with cot = d loss / d denoised_xs and x = 2 img - 1:
  g_F      = c_out cot                                                    (the gradient entering the network at proj_out's output)
  gx       = d <F(xin), g_F> / d xin at xin = c_in x                      (through the network, weights frozen)
  d_images = 2 (c_skip cot + c_in gx)
  AdaGN    = the explicit GroupNorm backward: with z = xhat (1 + w) + b, dz = g act'(z), dxhat = dz (1 + w),
             dx = rstd (dxhat - mean_g(dxhat) - xhat mean_g(dxhat xhat)) over each (sample, group); act' is erf-GELU's Phi(z) + z phi(z)
  down^T   per axis dx[i] = sum over (o, t) with refl(2o - 1 + t) = i of k[t] dy[o], k = [1, 3, 3, 1] / 8: two direct outputs per i, the fold of
           padded -1 (output 0, tap 0) into i = 1 and of padded H (output H/2 - 1, tap 3) into i = H - 2
  up^T     per axis dx[i] = 3/4 dy[2i] + 3/4 dy[2i + 1] + 1/4 dy[2i + 2] (i < H - 1) + 1/4 dy[2i - 1] (i > 0), plus the folds 1/4 dy[0] into
           i = 1 and 1/4 dy[2H - 1] into i = H - 2
  everything else (convolutions, attention, the skips and the concat) is autograd over the same float64 expressions as network64.
The two adjoints are written in GATHER form as matrices [H, H_out] from the index rules above, not by transposing fir_down64 / fir_up64; the
CPU test checks them against autograd of those.

emulate = "f16" | "bf16": the forward rounds where network64 rounds; autograd then rounds the GRADIENT at the same storage points (the cast's
own backward casts the gradient), and the gradient entering the network is rounded once more (pmi_edm_stage_out_bwd stores 16 bit).  gx is
taken at the rounded network input as a leaf: proj_in's dX writes fp32.

The gradient at a block's input is taken on `t.view_as(t)`: the gradient through this block alone (its input tensor is also a stored skip).

GRAD_DEFECTS are the seeded faults of tests/test_monster_grad_cpu.py.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

import _monster_ref64 as M
from _monster_ref64 import C_B, E32, out_rounding
from _ref64 import U, rnd  # noqa: F401

GRAD_DEFECTS = ("down_bwd_clamp", "up_bwd_clamp", "down_bwd_no_fold", "up_bwd_no_fold", "down_bwd_avgpool", "up_bwd_bilinear",
                "adagn_bwd_no_mean", "adagn_bwd_no_plus1", "adagn_bwd_tanh_gelu", "skip_grad_dropped", "dx1_dropped", "attn_bwd_dropped",
                "cout_cin_swapped", "no_cskip_term", "no_factor_2")
COTANGENT_SEED = 31


# ---- FIR adjoints: gather-form matrices [n, n_out] per axis ---------------------------------------------------------------------------------
def down_bwd_matrix(n, defect=None):
    """dx[i] = sum_o B[i, o] dy[o], n even, dy has n / 2 samples"""
    no, k = n // 2, (1 / 8, 3 / 8, 3 / 8, 1 / 8)
    B = torch.zeros(n, no, dtype=torch.float64)
    if defect == "down_bwd_avgpool":                      # the adjoint of a 2 x 2 average pool: half of dy[i // 2] per axis
        for i in range(n):
            B[i, i // 2] = 0.5
        return B
    for i in range(n):
        for t in range(4):
            if (i + 1 - t) % 2 == 0 and 0 <= (i + 1 - t) // 2 < no:
                B[i, (i + 1 - t) // 2] += k[t]
    if defect != "down_bwd_no_fold":
        lo, hi = (0, n - 1) if defect == "down_bwd_clamp" else (1, n - 2)
        B[lo, 0] += k[0]
        B[hi, no - 1] += k[3]
    return B


def bwd_terms(which, n):
    """terms the gather sums per index of one axis (a fold that lands on an output the index already reads is a term of its own)"""
    if which == "down":
        t = torch.tensor([sum(1 for tap in range(4) if (i + 1 - tap) % 2 == 0 and 0 <= (i + 1 - tap) // 2 < n // 2) for i in range(n)])
    else:
        t = torch.tensor([2 + (i < n - 1) + (i > 0) for i in range(n)])
    t[1] += 1
    t[n - 2] += 1
    return t


def up_bwd_matrix(n, defect=None):
    """dx[i] = sum_o B[i, o] dy[o], n >= 2, dy has 2n samples.  (The adjoint of bilinear x2 is the clamped border: the same fault.)"""
    B = torch.zeros(n, 2 * n, dtype=torch.float64)
    for i in range(n):
        B[i, 2 * i] += 0.75
        B[i, 2 * i + 1] += 0.75
        if i < n - 1:
            B[i, 2 * i + 2] += 0.25
        if i > 0:
            B[i, 2 * i - 1] += 0.25
    if defect != "up_bwd_no_fold":
        lo, hi = (0, n - 1) if defect in ("up_bwd_clamp", "up_bwd_bilinear") else (1, n - 2)
        B[lo, 0] += 0.25
        B[hi, 2 * n - 1] += 0.25
    return B


def _matrices(which, h, w, defect):
    if which == "down":
        d = defect if defect in ("down_bwd_clamp", "down_bwd_no_fold", "down_bwd_avgpool") else None
        return down_bwd_matrix(h, d), down_bwd_matrix(w, d)
    d = defect if defect in ("up_bwd_clamp", "up_bwd_no_fold", "up_bwd_bilinear") else None
    return up_bwd_matrix(h, d), up_bwd_matrix(w, d)


def fir_bwd64(g, which, defect=None):
    """g NCHW float64 = d loss / d (resampler output) -> d loss / d (its input) NCHW: [N, C, 2 Ho, 2 Wo] (down) or [N, C, Ho / 2, Wo / 2] (up)"""
    h, w = (2 * g.shape[2], 2 * g.shape[3]) if which == "down" else (g.shape[2] // 2, g.shape[3] // 2)
    By, Bx = _matrices(which, h, w, defect)
    return torch.einsum("ih,nchw,jw->ncij", By, g, Bx)


def fir_bwd_ref(g, which, dtype, defect=None):
    """g NHWC float64 of the 16-bit type -> (dx NHWC float64, tol).  Every weight (1, 3, 9 over 64 resp. 16) times a 16-bit value is exact in
    fp32, so the kernel rounds once per addition -- n = the element's number of terms, at most 9 resp. 36 -- and once at the store: the
    forward kernels' rule, C_B n E32 sum |w g| + the output rounding."""
    gc = g.permute(0, 3, 1, 2)
    h, w = (2 * gc.shape[2], 2 * gc.shape[3]) if which == "down" else (gc.shape[2] // 2, gc.shape[3] // 2)
    dx = fir_bwd64(gc, which, defect).permute(0, 2, 3, 1)
    By, Bx = _matrices(which, h, w, None)
    S = torch.einsum("ih,nchw,jw->ncij", By, gc.abs(), Bx).permute(0, 2, 3, 1)
    terms = (bwd_terms(which, h)[:, None] * bwd_terms(which, w)[None, :]).double()[None, :, :, None]
    return dx, C_B * terms * E32 * S + out_rounding(dx, dtype)


def fir_bwd_shapes(which):
    """(dx shape, dy shape) NHWC at the dx shapes of the forward tests"""
    if which == "down":
        return [((n, h, w, c), (n, h // 2, w // 2, c)) for n, h, w, c in M.FIR_DOWN_SHAPES]
    return [((n, h, w, c), (n, 2 * h, 2 * w, c)) for n, h, w, c in M.FIR_UP_SHAPES]


ONES_UP = {2: [2.0, 2.0], 3: [1.75, 2.5, 1.75]}
ONES_DOWN = {2: [0.5, 0.5]}


def ones_closed_form(which, n):
    """the adjoint applied to all-ones, per axis"""
    if which == "up":
        return torch.tensor(ONES_UP.get(n, [1.75, 2.25] + [2.0] * (n - 4) + [2.25, 1.75]), dtype=torch.float64)
    return torch.tensor(ONES_DOWN.get(n, [0.375, 0.625] + [0.5] * (n - 4) + [0.625, 0.375]), dtype=torch.float64)


# ---- EDM adjoints with per-element fp32 bounds ------------------------------------------------------------------------------------------------
def edm_stage_out_bwd_ref(d, sigma, scale, dtype, defect=None):
    """d NCHW float64 (fp32 values) -> (g NCHW float64 = scale c_out d, tol).  c_out: sigma D, sigma^2 (+ D^2 exact for D = 0.5), the sum, the
    root, the division (5); scale c_out is exact for a power of two; the product (1); then the 16-bit rounding."""
    s = M.sig4(sigma, d.shape[0])
    k = (M.c_in64(s) if defect == "cout_cin_swapped" else M.c_out64(s)) * scale
    v = k * d
    return v, C_B * 6 * E32 * v.abs() + out_rounding(v, dtype)


def edm_stage_in_bwd_ref(d, gx, sigma, inv_scale, defect=None):
    """d, gx NCHW float64 (fp32 values; gx still scaled) -> (d_images, tol) = 2 (c_skip d + c_in inv_scale gx).  c_skip: sigma^2, the sum, the
    division (3) + the product (1); c_in: sigma^2, the sum, the root, the division (4), times inv_scale (1, exact for a power of two), the
    product (1); the sum (1); the factor 2 is exact."""
    s = M.sig4(sigma, d.shape[0])
    a, b = M.c_skip64(s), M.c_in64(s)
    if defect == "cout_cin_swapped":
        b = M.c_out64(s)
    t1 = torch.zeros_like(d) if defect == "no_cskip_term" else a * d
    t2 = b * inv_scale * gx
    y = (1.0 if defect == "no_factor_2" else 2.0) * (t1 + t2)
    return y, C_B * E32 * 2 * (4 * t1.abs() + 6 * t2.abs() + (t1 + t2).abs())


def edm_bwd_inputs(seed=9):
    g = torch.Generator().manual_seed(seed)
    z = lambda: torch.randn(M.EDM_SHAPE, generator=g, dtype=torch.float64).float().double()
    return dict(d=z(), gx=z() * 3)


# ---- the network with the explicit backward pieces -------------------------------------------------------------------------------------------
def _gelu_grad(z, tanh_form):
    if tanh_form:
        c = math.sqrt(2 / math.pi)
        u = c * (z + 0.044715 * z ** 3)
        t = torch.tanh(u)
        return 0.5 * (1 + t) + 0.5 * z * (1 - t * t) * c * (1 + 3 * 0.044715 * z * z)
    return 0.5 * (1 + torch.erf(z / math.sqrt(2))) + z * torch.exp(-0.5 * z * z) / math.sqrt(2 * math.pi)


class _AdaGN(torch.autograd.Function):
    """act(group_norm(t, groups, eps 1e-5) (1 + w) + b); the backward is the formula of the module doc, with its seeded faults"""

    @staticmethod
    def forward(ctx, t, wgt, b, groups, act, defect):
        n, c, hh, ww = t.shape
        tg = t.reshape(n, groups, -1)
        mu, var = tg.mean(-1, keepdim=True), tg.var(-1, unbiased=False, keepdim=True)
        rstd = (var + 1e-5).rsqrt()
        xhat = ((tg - mu) * rstd).reshape(t.shape)
        z = xhat * (1 + wgt)[:, :, None, None] + b[:, :, None, None]
        ctx.save_for_backward(xhat, rstd, z, wgt)
        ctx.groups, ctx.act, ctx.defect = groups, act, defect
        return F.gelu(z) if act else z

    @staticmethod
    def backward(ctx, g):
        xhat, rstd, z, wgt = ctx.saved_tensors
        d = ctx.defect
        dz = g * _gelu_grad(z, d == "adagn_bwd_tanh_gelu") if ctx.act else g
        dxh = dz * (wgt if d == "adagn_bwd_no_plus1" else 1 + wgt)[:, :, None, None]
        n = g.shape[0]
        a, xh = dxh.reshape(n, ctx.groups, -1), xhat.reshape(n, ctx.groups, -1)
        if d == "adagn_bwd_no_mean":
            dx = rstd * a
        else:
            dx = rstd * (a - a.mean(-1, keepdim=True) - xh * (a * xh).mean(-1, keepdim=True))
        return dx.reshape(g.shape), None, None, None, None, None


class _Fir(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, which, defect):
        ctx.which, ctx.defect = which, defect
        return M.fir_down64(t) if which == "down" else M.fir_up64(t)

    @staticmethod
    def backward(ctx, g):
        return fir_bwd64(g, ctx.which, ctx.defect), None, None


# ---- one AdaGN + GELU backward as the engine launches it (ops.group_norm_backward with gamma = None, a FiLM row, act = GELU): the
# element-wise check that tells erf-GELU's derivative from its tanh form, which the network-level gates cannot (0.06 of a bf16 gate).
# The bound is _norm_ref64.gn_backward_ref's, with GELU's two constants: max |gelu''| = 2 phi(0) = 0.798 -> 0.8, and the absolute error of
# act_grad's fp32 evaluation 0.5 (1 + erf(x / sqrt 2)) + x phi(x): fast_erff 1.5e-7 on erf -> 0.75e-7, its argument's rounding 0.15e-7,
# x * 0.3989 * __expf(-x^2 / 2) <= 0.242 with three products and __expf (2^-21 relative, plus the argument's rounding) 2.0e-7, the final sum
# 1.13 E32 = 0.7e-7: 3.6e-7 -> 5e-7. ---------------------------------------------------------------------------------------------------------
GELU_CODE, GELU_LIP2, GELU_GRAD_HW = 3, 0.8, 5e-7


def adagn_bwd_case(dtype, seed=33):
    """(x, film) of _monster_ref64.adagn_case and a unit-normal dy of the 16-bit type"""
    x, film = M.adagn_case(dtype)
    g = torch.Generator().manual_seed(seed)
    return x, film, rnd(torch.randn(x.shape, generator=g, dtype=torch.float64), dtype)


def adagn_bwd_ref(x, film, dy, dtype, defect=None):
    """x, dy NHWC float64 of the 16-bit type, film [N or 1, 2C] -> (dx, tol)"""
    from unittest import mock

    import _norm_ref64 as NR
    n, h, w, c = x.shape
    groups = max(1, c // 32)
    film = film.expand(n, -1)
    depth = NR.standalone_depth(n, h * w, c)
    co = NR.gn_coeffs_ref(x, groups, 1e-5, film=film, depth=depth)
    with mock.patch.dict(NR.ACT_LIP2, {GELU_CODE: GELU_LIP2}), mock.patch.dict(NR.ACT_HW, {GELU_CODE: GELU_GRAD_HW}):
        dx, tol = NR.gn_backward_ref(x, dy, groups, 1e-5, None, None, film, GELU_CODE, co, depth, NR.gn_stats_depth(n, h * w, c), dtype=dtype)
    # the explicit backward of this file gives the same values (and carries the seeded faults)
    t = x.permute(0, 3, 1, 2).contiguous().requires_grad_()
    with torch.enable_grad():
        y = _AdaGN.apply(t, film[:, :c], film[:, c:2 * c], groups, True, defect)
        (mine,) = torch.autograd.grad(y, t, dy.permute(0, 3, 1, 2))
    mine = mine.permute(0, 2, 3, 1)
    if defect is None:
        assert float((mine - dx).abs().max()) <= 1e-12 * float(dx.abs().max())
    return mine, tol


def network_grad64(sd, xin, cond, config, *, emulate=None, defect=None, views=None):
    """network64 with the explicit backward pieces: xin = c_in x NCHW float64 (a leaf that requires grad), cond [N or 1, feats] -> F.
    views: dict receiving, as d<i> / u<i>, the view of every block's input whose .grad is the gradient through that block alone."""
    q = (lambda t: rnd(t, emulate)) if emulate else (lambda t: t)

    def tap(key, t):
        if views is None:
            return t
        v = t.view_as(t)
        v.retain_grad()
        views[key] = v
        return v

    def conv(t, name, pad, bias=True):
        return q(F.conv2d(t, q(sd[name + ".weight"].double()), sd[name + ".bias"].double() if bias else None, padding=pad))

    def adagn(t, key, act):
        c = t.shape[1]
        m = cond @ sd[key + ".mapper.weight"].double().T + sd[key + ".mapper.bias"].double()
        m = m.expand(t.shape[0], -1)
        return q(_AdaGN.apply(t, m[:, :c], m[:, c:], max(1, c // 32), act, defect))

    def res(t, key, cin, cmid, cout):
        skip = conv(t, key + ".skip", 0, bias=False) if cin != cout else t
        if defect == "skip_grad_dropped":
            skip = skip.detach()
        h = conv(adagn(t, key + ".main.0", True), key + ".main.2", 1)
        h = conv(adagn(h, key + ".main.4", True), key + ".main.6", 1)
        return q(h + skip)

    def attn(t, key, c):
        n, _, hh, ww = t.shape
        heads, d = max(1, c // 64), c // max(1, c // 64)
        qkv = conv(adagn(t, key + ".norm_in", False), key + ".qkv_proj", 0)
        v5 = qkv.view(n, 3, heads, d, hh * ww)
        qq, kk, vv = v5[:, 0], v5[:, 1], v5[:, 2]
        p = q(((qq.transpose(2, 3) * d ** -0.25) @ (kk * d ** -0.25)).softmax(-1))
        y = q((p @ vv.transpose(2, 3)).transpose(2, 3).reshape(n, c, hh, ww))
        branch = conv(y, key + ".out_proj", 0)
        return q((branch.detach() if defect == "attn_bwd_dropped" else branch) + t)

    def run(prog, t):
        for l in prog:
            if l[0] == "res":
                t = res(t, *l[1:])
            elif l[0] == "attn":
                t = attn(t, *l[1:])
            else:
                t = q(_Fir.apply(t, l[0], defect))
        return t

    cond = cond.double()
    d_blocks, u_blocks = M.blocks(config)
    h = conv(xin, "proj_in", 0)
    skips = []
    for i, prog in enumerate(d_blocks):
        h = run(prog, tap(f"d{i}", h))
        skips.append(h)
    for i, prog in enumerate(u_blocks):
        if i > 0:
            s = skips[len(skips) - 1 - i]
            h = torch.cat([h, s.detach() if defect == "dx1_dropped" else s], dim=1)
        h = run(prog, tap(f"u{i}", h))
    return F.conv2d(h, q(sd["proj_out.weight"].double()), sd["proj_out.bias"].double())


def grad64(sd, images, sigma, config, cot, *, emulate=None, defect=None):
    """-> dict(denoised_xs, d_images, gx, d<i>, u<i>): NCHW float64.  cot = d loss / d denoised_xs."""
    n = images.shape[0]
    x = images.double() * 2 - 1
    s1 = torch.as_tensor(sigma, dtype=torch.float64).reshape(-1)
    s = M.sig4(s1, n)
    cond = M.cond64(sd, M.c_noise64(s1), None)
    q = (lambda t: rnd(t, emulate)) if emulate else (lambda t: t)
    xin = q(M.c_in64(s) * x).requires_grad_()
    views = {}
    with torch.enable_grad():
        f = network_grad64(sd, xin, cond, config, emulate=emulate, defect=defect, views=views)
        cot = cot.double()
        g_f = q((M.c_in64(s) if defect == "cout_cin_swapped" else M.c_out64(s)) * cot)
        (f * g_f).sum().backward()
    gx = xin.grad
    t1 = torch.zeros_like(cot) if defect == "no_cskip_term" else M.c_skip64(s) * cot
    t2 = (M.c_out64(s) if defect == "cout_cin_swapped" else M.c_in64(s)) * gx
    out = {k: v.grad for k, v in views.items()}
    out["gx"] = gx
    out["d_images"] = (1.0 if defect == "no_factor_2" else 2.0) * (t1 + t2)
    out["denoised_xs"] = (M.c_skip64(s) * x + M.c_out64(s) * f).detach()
    return out


def grad_keys(config):
    L = len(config[1])
    return ("gx",) + tuple(f"d{i}" for i in range(L)) + tuple(f"u{i}" for i in range(L)) + ("d_images",)


def cotangent(shape, seed=COTANGENT_SEED):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(shape, generator=g, dtype=torch.float64).float()


# ---- per-sample distances ---------------------------------------------------------------------------------------------------------------
def per_sample(got, ref):
    """rel-L2 of every sample, then of the batch: tuple of N + 1 values (full NCHW tensors)"""
    got, ref = got.double(), ref.double()
    return tuple(M.rel_l2(got[i], ref[i]) for i in range(ref.shape[0])) + (M.rel_l2(got, ref),)


def per_sample_sampled(got, g, name):
    """as per_sample, against the fixture's entry `name`, which may hold every s-th value of the flattened tensor: the values are told apart
    by the sample their flat index falls into"""
    ref = g[name].double()
    got = got.double().contiguous()
    n = got.shape[0]
    if name + "_stride" not in g:
        return per_sample(got, ref.reshape(got.shape))
    stride = int(g[name + "_stride"])
    idx = torch.arange(0, got.numel(), stride)
    owner = idx // (got.numel() // n)
    gv = got.reshape(-1)[idx]
    return tuple(M.rel_l2(gv[owner == i], ref[owner == i]) for i in range(n)) + (M.rel_l2(gv, ref),)


# ---- gates of tests/test_gpu_monster_grad.py: 2 x the rel-L2 of the emulated gradient (emulate=dtype) against the float64 gradient, per sample
# and (last entry) over the batch, at the fixture's inputs and cotangent; measured on the CPU, tests/test_monster_grad_cpu.py measures them again.
# No figure comes from a GPU result. ----------------------------------------------------------------------------------------------------------
EMU_GRAD = {
    ("A", "bf16"): {'gx': (0.006074239, 0.006512528, 0.00651051), 'd0': (0.00667089, 0.006538322, 0.006539025),
                    'd1': (0.009168098, 0.007091397, 0.008305061), 'd2': (0.00744727, 0.007484485, 0.007466687),
                    'u0': (0.006470601, 0.007276296, 0.00696349), 'u1': (0.005445512, 0.005601943, 0.005556779),
                    'u2': (0.003430578, 0.003635859, 0.003589859), 'd_images': (0.004512482, 0.006512814, 0.004570509)},
    ("A", "f16"): {'gx': (0.0008427764, 0.0007417191, 0.0007422334), 'd0': (0.0008383558, 0.0008642501, 0.0008641161),
                   'd1': (0.001053017, 0.001163704, 0.001103823), 'd2': (0.0007636054, 0.001102117, 0.0009551057),
                   'u0': (0.000793237, 0.001000414, 0.000922704), 'u1': (0.0007096909, 0.0007251363, 0.0007206663),
                   'u2': (0.0004453989, 0.0004707745, 0.0004650824), 'd_images': (0.0006260888, 0.0007417516, 0.000629101)},
    ("B", "bf16"): {'gx': (0.008790131, 0.009151469, 0.008675165, 0.008877745), 'd0': (0.009161865, 0.009371296, 0.00896348, 0.009169554),
                    'd1': (0.00869859, 0.008236958, 0.008530074, 0.008478334), 'd2': (0.01044789, 0.009851794, 0.008727304, 0.009756989),
                    'u0': (0.008877832, 0.008678789, 0.008359137, 0.00864847), 'u1': (0.007034405, 0.007317503, 0.007181588, 0.007181694),
                    'u2': (0.005886421, 0.006043721, 0.005851065, 0.005929345), 'd_images': (0.008801953, 0.00914224, 0.00866798, 0.008876346)},
    ("B", "f16"): {'gx': (0.001199257, 0.001040773, 0.001072019, 0.001106516), 'd0': (0.001202103, 0.001106781, 0.00112378, 0.00114564),
                   'd1': (0.001267421, 0.001062625, 0.001101678, 0.001145973), 'd2': (0.001499784, 0.001282876, 0.001263826, 0.001355811),
                   'u0': (0.001214372, 0.001062667, 0.001148072, 0.001139103), 'u1': (0.0009476402, 0.0009012148, 0.0009255684, 0.0009244762),
                   'u2': (0.0007647189, 0.0007560861, 0.0007518984, 0.0007576892), 'd_images': (0.001200869, 0.001039723, 0.001071131, 0.001106342)},
}
# product config at product_grad_case(): (sample 0, sample 1, batch)
EMU_GRAD_PRODUCT = {"bf16": {'gx': (0.007380368, 0.009012926, 0.008983221), 'd_images': (0.005840271, 0.009016087, 0.007207467)},
                    "f16": {'gx': (0.000943306, 0.001121719, 0.001118434), 'd_images': (0.0007464618, 0.001122112, 0.0009069732)}}


# the same images and cotangent at ONE sigma = 5 for the batch (one row of AdaGN coefficients, film_ld = 0)
PRODUCT_SCALAR_SIGMA = 5.0
EMU_GRAD_PRODUCT_SCALAR = {"bf16": {'gx': (0.01005854, 0.009012926, 0.009517904), 'd_images': (0.01006278, 0.009016087, 0.009521561)},
                           "f16": {'gx': (0.001194822, 0.001121719, 0.001156599), 'd_images': (0.001195326, 0.001122112, 0.001157043)}}


def product_grad_case():
    """(images [2, 3, 16, 16] float32, sigma [2], cotangent) of the product-config gradient test"""
    g = torch.Generator().manual_seed(16)
    return torch.rand((2, 3, 16, 16), generator=g), torch.tensor([0.5, 5.0]), cotangent((2, 3, 16, 16), 17)


def grad_gate(net, dtype, key, sample):
    return 2 * EMU_GRAD[(net, dtype)][key][sample]
