"""float64 references, error scales, launch-geometry restatements and defect models for the GroupNorm, resampling, layout and
time-embedding kernels (csrc/norm.hip, backward.hip, elementwise.hip).  Same conventions as _ref64.py: every reference is float64 torch
on operands already rounded to the kernel's storage type, gradients come from float64 autograd, and a bound is c = 1.5 times the
elementwise worst-case sum of the roundings the kernel performs.

fp32 summation: a sum of m terms in any order (serial run or tree) of depth d is off by at most d E32 sum|terms| (first order,
E32 = 2^-24).  The depth of each statistics sum is restated below from the launch code:
  pmi_gn_stats     nchunk = max(1, min(hw // 8, ceil(1024 / n)))       (ops.py), ppc = ceil(hw / nchunk) pixels per chunk;
                   TPP = min(C / 8, 256) threads per pixel, PPI = 256 / TPP pixel lanes; a lane sums ceil(ppc / PPI) pixels, then the
                   PPI lane slots are added in order: depth ceil(ppc / PPI) + PPI
  pmi_gn_finalize  fp32 runs of 32 two-channel loads (64 values) or 64 one-channel loads, then double: depth 64 on top of the partials.
                   The slice count S splits the rows over S workgroups, each with the same fp32 runs, added in double
  conv epilogue    one stats row sums at most hw / rows pixels in fp32 (any tree), then the same finalize
From the sums: mean = S1 / n, var = S2 / n - mean^2 (double), rstd = (var + eps)^-1/2 rounded to fp32, a = rstd gamma (1 + film_s),
b = (beta - mean a) (1 + film_s) + film_h in fp32.  The rstd error is evaluated on the interval var +- dvar (not linearised: with var ~ eps
the interval is wide), then carried into a and b.
"""
from __future__ import annotations

import math

import torch

import _ref64
from _ref64 import TD, U, check, max_err, parity, rnd  # noqa: F401  (re-exported for the tests)

E32 = 2.0 ** -24
C_B = 1.5
UN = dict(U, precise=2.0 ** -22)          # precise (split f16 hi + lo): hi + lo keeps ~22 significant bits
SPLIT_FLOOR = 2.0 ** -25                 # ... and an absolute floor where lo = f16(y - hi) falls into the f16 subnormals
FLOOR = {"f16": 2.0 ** -25, "bf16": 0.0, "precise": SPLIT_FLOOR}      # half the smallest f16 subnormal (bf16's sit at 1e-38)
ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2
ACT_LIP = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_SILU: 1.1}          # max |act'|  (SiLU: 1.0998)
ACT_LIP2 = {ACT_NONE: 0.0, ACT_RELU: 0.0, ACT_SILU: 0.5}         # max |act''| (SiLU: 0.5 at 0); ReLU' jumps, only used with act none / SiLU
ACT_HW = {ACT_NONE: 0.0, ACT_RELU: 0.0, ACT_SILU: 2.0 ** -21}    # __expf + v_rcp_f32 of act_apply / act_grad, relative


def act_ref(x: torch.Tensor, act: int) -> torch.Tensor:
    return x if act == ACT_NONE else _ref64.act_ref(x, act)


def act_grad_ref(x: torch.Tensor, act: int) -> torch.Tensor:
    return torch.ones_like(x) if act == ACT_NONE else _ref64.act_grad_ref(x, act)


def split_round(x: torch.Tensor) -> torch.Tensor:
    """x (float) as the precise type stores it: hi = f16(x), lo = f16(x - hi), value hi + lo (float64)."""
    x = x.float()
    hi = x.half()
    lo = (x - hi.float()).half()
    return hi.double() + lo.double()


def round_to(x: torch.Tensor, dtype: str) -> torch.Tensor:
    return split_round(x) if dtype == "precise" else rnd(x, dtype)


def out_round(y: torch.Tensor, dtype: str) -> torch.Tensor:
    """the storage rounding bound of an output of magnitude |y|"""
    return UN[dtype] * y.abs() + FLOOR[dtype]


def to_split16(x: torch.Tensor) -> torch.Tensor:
    """float [..., C] -> the precise layout [..., 2C] f16: per group of G = min(32, C) channels G high parts then G low parts."""
    C = x.shape[-1]
    G = 32 if C % 32 == 0 else C
    xf = x.float()
    hi = xf.half()
    lo = (xf - hi.float()).half()
    sh = x.shape[:-1] + (C // G, G)
    return torch.stack([hi.reshape(sh), lo.reshape(sh)], -2).reshape(x.shape[:-1] + (2 * C,))


def from_split16(t: torch.Tensor) -> torch.Tensor:
    C = t.shape[-1] // 2
    G = 32 if C % 32 == 0 else C
    v = t.double().reshape(t.shape[:-1] + (C // G, 2, G))
    return (v[..., 0, :] + v[..., 1, :]).reshape(t.shape[:-1] + (C,))


# ---- launch geometry (restated from ops.py / norm.hip / backward.hip) -----------------------------------------------------------------
def gn_nchunk(n: int, hw: int) -> int:
    return max(1, min(hw // 8, (1024 + n - 1) // n))


def gn_stats_geom(C: int):
    tpp = min(C // 8, 256)
    return tpp, 256 // tpp


def gn_stats_depth(n: int, hw: int, C: int) -> int:
    """fp32 depth of one (sample, chunk, channel) partial of gn_stats_kernel (and gn_bwd_stats_kernel)."""
    nchunk = gn_nchunk(n, hw)
    ppc = -(-hw // nchunk)
    _, ppi = gn_stats_geom(C)
    return -(-ppc // ppi) + ppi


FIN_RUN = 64          # gn_finalize_kernel: 32 float4 loads (64 values) or 64 float2 loads per fp32 run


def finalize_slices(N: int, G: int, C: int, P0: int, P1: int = 0) -> int:
    """pmi_gn_finalize's slice count S."""
    cpg = C // G
    S = 1
    if N * G < 128 and max(P0, P1) * cpg >= 32768 and cpg % 2 == 0:
        S = min(256 // (N * G), cpg // 4, 64)
        if S < 2:
            S = 1
    return S


def standalone_depth(n: int, hw: int, C: int) -> int:
    return gn_stats_depth(n, hw, C) + FIN_RUN


def fused_depth(hw: int, rows: int) -> int:
    return -(-hw // rows) + FIN_RUN


# ---- GroupNorm forward -------------------------------------------------------------------------------------------------------------
def _film_parts(film, film_ld, N, C, dev):
    if film is None:
        return torch.ones(N, C, dtype=torch.float64, device=dev), torch.zeros(N, C, dtype=torch.float64, device=dev)
    f = film.double().to(dev)
    return 1.0 + f[:, :C], f[:, C:2 * C]


def gn_coeffs_ref(x, G, eps, gamma=None, beta=None, film=None, film_ld=0, depth=64, pert=None):
    """x: float64 [N, H, W, C] (the rounded input).  Returns a dict of float64 [N, C] tensors: the exact coefficients a, b
    (norm(x) gamma + beta with FiLM = x a + b) and their bounds da, db, plus mean, std per channel (of the channel's group).
    pert: [N, H, W, C] bound of the difference between the values the statistics were taken from and x (the conv epilogue's
    fp32 accumulation and rounding against the float64 conv)."""
    N, H, W, C = x.shape
    dev = x.device
    cpg = C // G
    n = H * W * cpg
    xg = x.reshape(N, H * W, G, cpg)
    mean = xg.mean((1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean((1, 3))
    s1abs = xg.abs().sum((1, 3))
    s2 = (xg * xg).sum((1, 3))
    dmean = depth * E32 * s1abs / n
    dvar = (depth + 1) * E32 * s2 / n
    if pert is not None:
        pg = pert.reshape(N, H * W, G, cpg)
        dmean = dmean + pg.sum((1, 3)) / n
        dvar = dvar + (2 * xg.abs() * pg + pg * pg).sum((1, 3)) / n * (1 + 2 * (depth + 1) * E32)
    dvar = dvar + 2 * mean.abs() * dmean + dmean ** 2
    r = (var + eps) ** -0.5
    r_lo = (var + dvar + eps) ** -0.5
    r_hi = ((var - dvar).clamp_min(0) + eps) ** -0.5
    dr = torch.maximum(r_hi - r, r - r_lo) + 2 * E32 * r
    rep = lambda t: t.repeat_interleave(cpg, dim=1)                       # noqa: E731  [N, G] -> [N, C]
    mean_c, r_c, dr_c, dmean_c, std_c = rep(mean), rep(r), rep(dr), rep(dmean), rep(var.sqrt())
    gm = gamma.double().to(dev)[None] if gamma is not None else torch.ones(1, C, dtype=torch.float64, device=dev)
    bt = beta.double().to(dev)[None] if beta is not None else torch.zeros(1, C, dtype=torch.float64, device=dev)
    sc, sh = _film_parts(film, film_ld, N, C, dev)
    a0 = r_c * gm
    b0 = bt - mean_c * a0
    a = a0 * sc
    b = b0 * sc + sh
    da0 = gm.abs() * dr_c + 2 * E32 * a0.abs()
    db0 = mean_c.abs() * da0 + a0.abs() * (dmean_c + E32 * mean_c.abs()) + 2 * E32 * (mean_c * a0).abs() + E32 * b0.abs()
    da = sc.abs() * da0 + 2 * E32 * a.abs()
    db = sc.abs() * db0 + 2 * E32 * ((b0 * sc).abs() + b.abs())
    return dict(a=a, b=b, da=da, db=db, mean=mean_c, std=std_c, r=r_c, dr=dr_c, dmean=dmean_c, sc=sc, gm=gm)


def gn_apply_ref(x, co, act=ACT_NONE, pool=False, res=None, dtype="f16"):
    """y = act(x a + b) [-> 2x2 average] [+ res] on float64 NHWC, and its elementwise bound (C_B included)."""
    a, b = co["a"][:, None, None, :], co["b"][:, None, None, :]
    z = x * a + b
    y = act_ref(z, act)
    e = ACT_LIP[act] * (x.abs() * co["da"][:, None, None, :] + co["db"][:, None, None, :] + 2 * E32 * ((x * a).abs() + b.abs())) \
        + ACT_HW[act] * y.abs() + E32 * y.abs()
    if pool:
        N, H, W, C = y.shape
        pl = lambda t: t.reshape(N, H // 2, 2, W // 2, 2, C).mean((2, 4))     # noqa: E731
        y, ya = pl(y), pl(y.abs())
        e = pl(e) + 3 * E32 * ya
    if res is not None:
        y = y + res
        e = e + E32 * (y.abs() + res.abs())
    return y, C_B * (e + out_round(y, dtype))


def coeffs_from_sums(S1, S2, cnt, cpg, eps, gamma=None, beta=None, film=None):
    """float64 coefficients from exact group sums S1, S2 [N, G] (pmi_gn_finalize on synthetic partials) and their bound: the
    double combination, the fp32 rstd and the fp32 coefficient arithmetic only."""
    N, G = S1.shape
    C = G * cpg
    mean = S1 / cnt
    var = (S2 / cnt - mean * mean).clamp_min(0)
    rep = lambda t: t.repeat_interleave(cpg, dim=1)                       # noqa: E731
    r = rep((var + eps) ** -0.5)
    mean_c = rep(mean)
    gm = gamma.double()[None] if gamma is not None else torch.ones(1, C, dtype=torch.float64)
    bt = beta.double()[None] if beta is not None else torch.zeros(1, C, dtype=torch.float64)
    sc, sh = _film_parts(film, 0, N, C, "cpu")
    a0 = r * gm
    b0 = bt - mean_c * a0
    a, b = a0 * sc, b0 * sc + sh
    da0 = 3 * E32 * a0.abs()
    db0 = mean_c.abs() * da0 + 3 * E32 * (mean_c * a0).abs() + E32 * b0.abs()
    da = sc.abs() * da0 + 2 * E32 * a.abs()
    db = sc.abs() * db0 + 2 * E32 * ((b0 * sc).abs() + b.abs())
    return dict(a=a, b=b, da=da, db=db, mean=mean_c, std=rep(var.sqrt()))


def coeff_accuracy(ca, cb, co, u, limit):
    """ratios of the coefficient errors to the accuracy requirement |a - a64| <= u/4 |a64|, |b - b64| <= u/4 |a64| (|mean| + std),
    over the groups with |mean| <= limit std (the requirement's range; None if there is none)."""
    a64, b64 = co["a"], co["b"]
    m = co["mean"].abs() <= limit * co["std"]
    if not bool(m.any()):
        return None
    ra = ((ca.double().to(a64.device) - a64).abs() / (u / 4 * a64.abs()).clamp_min(1e-300))[m].max()
    scale_b = u / 4 * a64.abs() * (co["mean"].abs() + co["std"])
    rb = ((cb.double().to(b64.device) - b64).abs() / scale_b.clamp_min(1e-300))[m].max()
    return float(ra), float(rb)


def coeff_bound_ratio(ca, cb, co):
    a64, b64 = co["a"], co["b"]
    ra = ((ca.double().to(a64.device) - a64).abs() / (C_B * co["da"]).clamp_min(1e-300)).max()
    rb = ((cb.double().to(b64.device) - b64).abs() / (C_B * co["db"]).clamp_min(1e-300)).max()
    return float(ra), float(rb)


def echeck(tag, got, ref, tol):
    """elementwise bound: |got - ref| <= tol everywhere; prints the element closest to its bound."""
    d = (got.double().to(ref.device) - ref).abs()
    assert not torch.isnan(got).any(), f"{tag}: NaN in the output"
    ratio = d / tol.clamp_min(1e-300)
    i = int(ratio.flatten().argmax())
    parity(tag, float(d.flatten()[i]), float(tol.flatten()[i]))
    rmax = float(ratio.flatten()[i])
    assert rmax <= 1.0, f"{tag}: error {rmax:.3f}x its bound"
    return rmax


def defect_ratio(defect, ref, tol):
    """max |defect - ref| / tol: how far outside the bound a defect lands"""
    return float(((defect - ref).abs() / tol.clamp_min(1e-300)).max())


# ---- GroupNorm backward ------------------------------------------------------------------------------------------------------------
def gn_forward64(x, G, eps, gamma, beta, film, act):
    N, H, W, C = x.shape
    cpg = C // G
    xg = x.reshape(N, H * W, G, cpg)
    mean = xg.mean((1, 3), keepdim=True)
    var = ((xg - mean) ** 2).mean((1, 3), keepdim=True)
    xh = ((xg - mean) / torch.sqrt(var + eps)).reshape(N, H, W, C)
    gm = gamma.double().to(x.device) if gamma is not None else 1.0
    bt = beta.double().to(x.device) if beta is not None else 0.0
    y = xh * gm + bt
    if film is not None:
        f = film.double().to(x.device)
        y = y * (1 + f[:, None, None, :C]) + f[:, None, None, C:2 * C]
    return act_ref(y, act)


def gn_backward_ref(x, dy, G, eps, gamma, beta, film, act, co, fwd_depth, bwd_depth, gadd=None, dtype="f16"):
    """float64 autograd dx of act(GN(x) gamma (1 + s) + beta' ...) for dy, and the elementwise bound of the kernel's
    dx = a dt + P x + Q (+ gadd) with dt = dy act'(a x + b), P, Q from fp32 partials A = sum dt, B = sum dt x (depth bwd_depth)
    and the forward partials (depth fwd_depth, added in double per channel).  co: gn_coeffs_ref of the forward (depth fwd_depth)."""
    N, H, W, C = x.shape
    cpg = C // G
    n = H * W * cpg
    xr = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        y = gn_forward64(xr, G, eps, gamma, beta, film, act)
        (dx,) = torch.autograd.grad(y, xr, dy)
    a, b = co["a"][:, None, None, :], co["b"][:, None, None, :]
    da, db = co["da"][:, None, None, :], co["db"][:, None, None, :]
    z = x * a + b
    dt = dy * act_grad_ref(z, act)
    e_dt = dy.abs() * (ACT_LIP2[act] * (x.abs() * da + db + 2 * E32 * ((x * a).abs() + b.abs())) + ACT_HW[act]) + E32 * dt.abs()
    gp = co["gm"] * co["sc"]                                          # gamma' [N, C]
    gsum = lambda t: (t.reshape(N, H * W, G, cpg)).sum((1, 3))        # noqa: E731  [N, G]
    rep = lambda t: t.repeat_interleave(cpg, dim=1)                   # noqa: E731
    gp4 = gp[:, None, None, :]
    a1 = gsum(gp4 * dt)
    a2 = gsum(gp4 * dt * x)
    da1 = gsum(gp4.abs() * (bwd_depth * E32 * dt.abs() + e_dt)) + 2 * E32 * gsum((gp4 * dt).abs())
    da2 = gsum(gp4.abs() * ((bwd_depth + 1) * E32 * (dt * x).abs() + x.abs() * e_dt)) + 2 * E32 * gsum((gp4 * dt * x).abs())
    xg = x.reshape(N, H * W, G, cpg)
    mu = xg.mean((1, 3))
    r = co["r"][:, ::cpg]
    dr = co["dr"][:, ::cpg]
    dmu = co["dmean"][:, ::cpg]
    m1 = a1 / n
    m2 = r * (a2 - mu * a1) / n
    dm1 = da1 / n
    dm2 = m2.abs() * dr / r + r * (da2 + mu.abs() * da1 + a1.abs() * dmu) / n
    P = -r * r * m2
    Q = -r * m1 + r * r * mu * m2
    dP = 2 * r * dr * m2.abs() + r * r * dm2 + E32 * P.abs()
    dQ = dr * m1.abs() + r * dm1 + 2 * r * dr * (mu * m2).abs() + r * r * (dmu * m2.abs() + mu.abs() * dm2) \
        + 2 * E32 * (Q.abs() + (r * m1).abs() + (r * r * mu * m2).abs())
    P4, Q4, dP4, dQ4 = (rep(t)[:, None, None, :] for t in (P, Q, dP, dQ))
    e = da * dt.abs() + a.abs() * e_dt + x.abs() * dP4 + dQ4 + 2 * E32 * ((a * dt).abs() + (P4 * x).abs() + Q4.abs())
    if gadd is not None:
        dx = dx + gadd
        e = e + E32 * dx.abs()
    return dx, C_B * (e + out_round(dx, dtype))


def gn1_backward_ref(x, dy, gamma_nc, eps, res=None, dtype="f16"):
    """pmi_gn1_bwd: GroupNorm(1, C) backward with the per-(sample, channel) scale gamma_nc [N, C] (gamma[n * ld + c] + gamma_add);
    x, dy, res float64 [N, hw, C].  Returns float64 dx and the bound.  Partials: 8 values per thread in fp32, then double."""
    N, hw, C = x.shape
    cnt = hw * C
    gm = gamma_nc.double().to(x.device)[:, None, :]
    xr = x.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        mu = xr.mean((1, 2), keepdim=True)
        var = ((xr - mu) ** 2).mean((1, 2), keepdim=True)
        y = (xr - mu) / torch.sqrt(var + eps) * gm
        (dx,) = torch.autograd.grad(y, xr, dy)
    s = lambda t: t.sum((1, 2), keepdim=True)            # noqa: E731
    g = gm * dy
    mu = x.mean((1, 2), keepdim=True)
    var = ((x - mu) ** 2).mean((1, 2), keepdim=True)
    dmu = 8 * E32 * s(x.abs()) / cnt + E32 * mu.abs()
    dvar = 9 * E32 * s(x * x) / cnt + 2 * mu.abs() * dmu + dmu ** 2
    r = (var + eps) ** -0.5
    dr = torch.maximum(((var - dvar).clamp_min(0) + eps) ** -0.5 - r, r - (var + dvar + eps) ** -0.5) + 2 * E32 * r
    t2, t3 = s(g), s(g * x)
    dt2, dt3 = 10 * E32 * s(g.abs()), 11 * E32 * s((g * x).abs())
    m1 = t2 / cnt
    m2 = r * (t3 - mu * t2) / cnt
    dm1 = dt2 / cnt + E32 * m1.abs()
    dm2 = m2.abs() * dr / r + r * (dt3 + mu.abs() * dt2 + t2.abs() * dmu) / cnt + E32 * m2.abs()
    xh = (x - mu) * r
    inner = g - m1 - xh * m2
    e = dr * inner.abs() + r * (2 * E32 * g.abs() + dm1 + (x.abs() + mu.abs()) * 2 * E32 * r * m2.abs() + (x - mu).abs() * (dr * m2.abs() + r * dm2)) \
        + 4 * E32 * r * (g.abs() + m1.abs() + (xh * m2).abs())
    if res is not None:
        dx = dx + res
        e = e + E32 * dx.abs()
    return dx, C_B * (e + out_round(dx, dtype))


# ---- resampling ----------------------------------------------------------------------------------------------------------------------
def avgpool_ref(x, dtype):
    N, H, W, C = x.shape
    v = x.reshape(N, H // 2, 2, W // 2, 2, C)
    y = v.mean((2, 4))
    return y, C_B * (3 * E32 * v.abs().mean((2, 4)) + E32 * y.abs() + out_round(y, dtype))


def bilinear_taps(n: int, zero_border: bool = False) -> torch.Tensor:
    """[2n, n] matrix of F.interpolate(x2, bilinear, align_corners=False) along one axis (edge-clamped; zero_border: the defect)."""
    M = torch.zeros(2 * n, n, dtype=torch.float64)
    for o in range(2 * n):
        i = o // 2
        j = i - 1 if o % 2 == 0 else i + 1
        M[o, i] += 0.75
        if 0 <= j < n:
            M[o, j] += 0.25
        elif not zero_border:
            M[o, i] += 0.25
    return M


def bilinear_ref(x, dtype, zero_border=False):
    N, H, W, C = x.shape
    My, Mx = bilinear_taps(H, zero_border).to(x.device), bilinear_taps(W, zero_border).to(x.device)
    y = torch.einsum("oh,nhwc,pw->nopc", My, x, Mx)
    ya = torch.einsum("oh,nhwc,pw->nopc", My, x.abs(), Mx)
    return y, C_B * (5 * E32 * ya + out_round(y, dtype))


def bilinear_bwd_ref(dy, dtype, H, W):
    My, Mx = bilinear_taps(H).to(dy.device), bilinear_taps(W).to(dy.device)
    dx = torch.einsum("oh,nopc,pw->nhwc", My, dy, Mx)
    dxa = torch.einsum("oh,nopc,pw->nhwc", My, dy.abs(), Mx)
    return dx, C_B * (17 * E32 * dxa + out_round(dx, dtype))      # up to 16 taps: a product and an add each


def nearest_ref(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


def nearest_bwd_ref(dy, dtype, taps=4):
    N, Ho, Wo, C = dy.shape
    v = dy.reshape(N, Ho // 2, 2, Wo // 2, 2, C)
    dx = v.sum((2, 4)) if taps == 4 else v[:, :, 0].sum(3)
    return dx, C_B * (2 * E32 * v.abs().sum((2, 4)) + out_round(dx, dtype))


def avgpool_bwd_ref(dy, dtype, scale=0.25):
    dx = scale * nearest_ref(dy)
    return dx, C_B * (out_round(dx, dtype))


# ---- embeddings ----------------------------------------------------------------------------------------------------------------------
def timestep_embedding_ref(t, dim, max_period, dtype):
    """[N, dim] cos | sin of t freq_j, freq_j = exp(-ln(max_period) j / half); bound: the fp32 argument (t freq with freq from logf,
    a product, a division and expf: (3 + 2 |E|) E32 relative, E = the exponent), ocml cosf / sinf (2 ulp) and the output rounding."""
    half = dim // 2
    j = torch.arange(half, dtype=torch.float64, device=t.device)
    E = -math.log(max_period) * j / half
    arg = t.double()[:, None] * torch.exp(E)[None]
    ref = torch.cat([torch.cos(arg), torch.sin(arg)], 1)
    darg = arg.abs() * (3 + 2 * E.abs())[None] * E32 + arg.abs() * 2 * E32
    u = E32 if dtype == "precise" else U[dtype]
    e = torch.cat([darg, darg], 1) + 2 * E32 + u * ref.abs()
    return ref, C_B * e


def fourier_ref(t, w):
    arg = 2 * math.pi * t.double()[:, None] * w.double()[None]
    ref = torch.cat([torch.cos(arg), torch.sin(arg)], 1)
    darg = 3 * E32 * arg.abs()
    e = torch.cat([darg, darg], 1) + 2 * E32 + E32 * ref.abs()
    return ref, C_B * e


# ---- input distributions -------------------------------------------------------------------------------------------------------------
def gn_input(N, H, W, C, G, dist, seed, dtype, dev="cpu"):
    """float64 NHWC input rounded to the storage type.  dist: 'normal' N(0.3, 1.5^2); 'off4' / 'off16' / 'off64': per-group offsets at
    |mean| / std = 4 / 16 / 64; 'spread': a x100 per-channel scale spread inside each group; 'edge': group 0 constant (var = 0), group 1
    with var ~ eps, the rest normal; 'big': f16 values near 3e4."""
    g = torch.Generator().manual_seed(seed)
    cpg = C // G
    x = torch.randn(N, H, W, C, generator=g, dtype=torch.float64)
    if dist == "normal":
        x = 0.3 + 1.5 * x
    elif dist.startswith("off"):
        k = float(dist[3:])
        sign = torch.where(torch.rand(N, 1, 1, G, generator=g) < 0.5, -1.0, 1.0).double()
        std = torch.exp(torch.rand(N, 1, 1, G, generator=g, dtype=torch.float64) * 2 - 1)
        x = (x.reshape(N, H, W, G, cpg) * std[..., None] + (k * std * sign)[..., None]).reshape(N, H, W, C)
    elif dist == "spread":
        s = 10.0 ** (2 * torch.rand(C, generator=g, dtype=torch.float64) - 1)
        x = 0.2 + x * s
    elif dist == "edge":
        x = 0.3 + 1.5 * x
        x[..., :cpg] = 0.5
        if G > 1:
            x[..., cpg:2 * cpg] = 3e-3 * torch.sign(x[..., cpg:2 * cpg])
    elif dist == "big":
        x = 2.9e4 + 600 * x if dtype == "f16" else 3e4 + 600 * x
    else:
        raise ValueError(dist)
    return round_to(x, dtype).to(dev)
