"""float64 restatement of MonsterDiffusion (engine/monster.py, models/monster_diffusion): the k-diffusion UNet, the two FIR resamplers, the
EDM algebra and both samplers, in this file's own words; checked against the reference's values in tests/golden/monster_diffusion_reference.npz
by tests/test_monster_diffusion_cpu.py.

Network (config = (feats, depths, channels, self_attn, mapping_cond_dim); x = c_in (2 img - 1), NCHW):
  cond   = gelu(L2(gelu(L1([cos f | sin f] + aug Wc^T)))), f = 2 pi c_noise W^T, c_noise = ln(sigma) / 4          [rows, feats]
  AdaGN  = group_norm(x, C / 32 groups, eps 1e-5, no affine) * (1 + w) + b with (w | b) = mapper(cond)
  Res    = conv3x3(gelu(AdaGN(conv3x3(gelu(AdaGN(x)))))) + skip(x), skip = identity or a bias-free 1x1 conv where the widths differ
  Attn   = x + out(softmax(q^T k / sqrt(d)) v) on qkv = 1x1(AdaGN(x)) viewed as [3 * heads, d, hw]: q, k, v first, heads inside; d = 64
  DBlock = [down] + depth * (Res [+ Attn]);  UBlock = depth * (Res [+ Attn]) + [up], levels below the deepest reading cat([input, skip])
  down   = reflect-pad 1, depthwise (k k^T) with k = [1, 3, 3, 1] / 8, stride 2
  up     = per axis out[2y] = x[refl(y - 1)] / 4 + 3 x[y] / 4, out[2y + 1] = 3 x[y] / 4 + x[refl(y + 1)] / 4
  F      = proj_out(u_0(... u_deepest(d_deepest(... d_0(proj_in(x))))))
EDM (D = 0.5): denoised_xs = c_skip x + c_out F, c_skip = D^2 / (D^2 + s^2), c_out = s D / sqrt(D^2 + s^2), c_in = 1 / sqrt(D^2 + s^2);
  eps = (x - denoised) / s, step = decode(denoised + eps s_to), correction = decode(x_prev + (s - s_prev)(eps + eps_prev) / 2),
  inject_noise = decode(x + sqrt(s_rev^2 - s^2) noise S_noise), decode(x) = (x + 1) / 2.

emulate = "f16" | "bf16" rounds exactly where the engine stores 16 bit: the staged input c_in x, the convolution weights, proj_in's output,
every AdaGN + activation output (pmi_gn_apply), every convolution output (a convolution with a residual stages its own value in 16 bit,
adds the 16-bit residual in fp32 and rounds again: the "two" form of _routes16_ref64.py), the skip convolution, qkv, the attention
probabilities and output, both resamplers.  proj_out writes fp32; the conditioning (cond, the mappers) and the EDM algebra are fp32 in the
engine and exact here.  ROUNDINGS (roundings()) counts the 16-bit roundings along the longest path to every checkpoint.

DEFECTS are the seeded faults of tests/test_monster_diffusion_cpu.py.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from _ref64 import TD, U, rnd  # noqa: F401

SIGMA_DATA, SIGMA_MIN, SIGMA_MAX, RHO = 0.5, 1e-2, 80.0, 7.0
S_TMIN, S_TMAX, S_CHURN, S_NOISE = 0.05, 50.0, 80.0, 1.003
DEFECTS = ("down_clamp", "up_clamp", "taps_1221", "adagn_no_plus1", "adagn_swapped", "groups32", "heads_first", "tanh_gelu", "c_noise_ln",
           "cskip_cout_swapped", "heun_no_half")
NOOP_DEFECT = "scale_q_only"          # d^-1/2 on q alone is the same product as d^-1/4 on q and on k


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


# ---- resamplers -------------------------------------------------------------------------------------------------------------------------
def _border(i, n, clamp):
    """indices -1 .. n of an axis of n samples: reflected (x[-1] = x[1], x[n] = x[n - 2]) or, as a defect, clamped"""
    if clamp:
        return i.clamp(0, n - 1)
    return torch.where(i < 0, -i, torch.where(i >= n, 2 * (n - 1) - i, i))


def fir_down64(x, defect=None):
    """x NCHW float64, H and W even -> [N, C, H / 2, W / 2]"""
    taps = [1 / 6, 2 / 6, 2 / 6, 1 / 6] if defect == "taps_1221" else [1 / 8, 3 / 8, 3 / 8, 1 / 8]
    n, c, h, w = x.shape
    ri = _border(torch.arange(-1, h + 1), h, defect == "down_clamp")
    ci = _border(torch.arange(-1, w + 1), w, defect == "down_clamp")
    xp = x[:, :, ri][:, :, :, ci]
    out = torch.zeros(n, c, h // 2, w // 2, dtype=x.dtype)
    for a in range(4):
        for b in range(4):
            out = out + taps[a] * taps[b] * xp[:, :, a:a + h - 1:2, b:b + w - 1:2]
    return out


def _up_axis(x, dim, defect):
    n = x.shape[dim]
    near, far = (2 / 3, 1 / 3) if defect == "taps_1221" else (0.75, 0.25)
    i = torch.arange(n)
    lo = x.index_select(dim, _border(i - 1, n, defect == "up_clamp"))
    hi = x.index_select(dim, _border(i + 1, n, defect == "up_clamp"))
    even, odd = far * lo + near * x, near * x + far * hi
    shape = list(x.shape)
    shape[dim] = 2 * n
    return torch.stack([even, odd], dim=dim + 1).reshape(shape)


def fir_up64(x, defect=None):
    """x NCHW float64, H and W >= 2 -> [N, C, 2H, 2W]"""
    return _up_axis(_up_axis(x, 2, defect), 3, defect)


# ---- network ----------------------------------------------------------------------------------------------------------------------------
def blocks(config):
    """(d_blocks, u_blocks in running order): lists of ("down" | "up", key) / ("res", key, cin, cmid, cout) / ("attn", key, c)"""
    feats, depths, channels, attn, _ = config
    L = len(depths)

    def block(prefix, depth, c_in, c_mid, c_out, sa, down=False, up=False):
        prog, j = [], 0
        if down:
            prog.append(("down", f"{prefix}.{j}")); j += 1
        for i in range(depth):
            a, b = (c_in if i == 0 else c_mid), (c_mid if i < depth - 1 else c_out)
            prog.append(("res", f"{prefix}.{j}", a, c_mid, b)); j += 1
            if sa:
                prog.append(("attn", f"{prefix}.{j}", b)); j += 1
        if up:
            prog.append(("up", f"{prefix}.{j}"))
        return prog

    d = [block(f"u_net.d_blocks.{i}", depths[i], channels[max(i - 1, 0)], channels[i], channels[i], attn[i], down=i > 0) for i in range(L)]
    u = [block(f"u_net.u_blocks.{p}", depths[i], channels[i] * (2 if i < L - 1 else 1), channels[i], channels[max(i - 1, 0)], attn[i], up=i > 0)
         for p, i in enumerate(reversed(range(L)))]
    return d, u


def gelu64(x, defect=None):
    return F.gelu(x, approximate="tanh") if defect == "tanh_gelu" else F.gelu(x)


def cond64(sd, c_noise, aug, defect=None):
    w = sd["timestep_embed.weight"].double()
    f = 2 * math.pi * c_noise.double().reshape(-1, 1) @ w.T
    e = torch.cat([f.cos(), f.sin()], dim=-1)
    if aug is not None:
        e = e + aug.double() @ sd["mapping_cond.weight"].double().T
    for i in (0, 2):
        e = gelu64(e @ sd[f"mapping.{i}.weight"].double().T + sd[f"mapping.{i}.bias"].double(), defect)
    return e


def network64(sd, x, cond, config, *, emulate=None, defect=None, record=None):
    """sd: state dict (bare reference keys); x = c_in (2 img - 1) NCHW float64; cond [N or 1, feats] float64 -> F NCHW float64.
    record: dict receiving proj_in, d<i>, u<i> (running order) and proj_out, NCHW."""
    q = (lambda t: rnd(t, emulate)) if emulate else (lambda t: t)
    keep = (lambda k, t: record.__setitem__(k, t)) if record is not None else (lambda k, t: None)

    def conv(t, name, pad, bias=True):
        y = F.conv2d(t, q(sd[name + ".weight"].double()), sd[name + ".bias"].double() if bias else None, padding=pad)
        return q(y)

    def adagn(t, key, act):
        c = t.shape[1]
        m = cond @ sd[key + ".mapper.weight"].double().T + sd[key + ".mapper.bias"].double()
        wgt, b = m[:, :c], m[:, c:]
        if defect == "adagn_swapped":
            wgt, b = b, wgt
        g = 32 if defect == "groups32" else max(1, c // 32)
        y = F.group_norm(t, g, eps=1e-5) * ((wgt if defect == "adagn_no_plus1" else 1 + wgt)[:, :, None, None]) + b[:, :, None, None]
        return q(gelu64(y, defect) if act else y)

    def res(t, key, cin, cmid, cout):
        skip = conv(t, key + ".skip", 0, bias=False) if cin != cout else t
        h = conv(adagn(t, key + ".main.0", True), key + ".main.2", 1)
        h = conv(adagn(h, key + ".main.4", True), key + ".main.6", 1)
        return q(h + skip)

    def attn(t, key, c):
        n, _, hh, ww = t.shape
        heads, d = max(1, c // 64), c // max(1, c // 64)
        qkv = conv(adagn(t, key + ".norm_in", False), key + ".qkv_proj", 0)
        if defect == "heads_first":
            v5 = qkv.view(n, heads, 3, d, hh * ww)
            qq, kk, vv = v5[:, :, 0], v5[:, :, 1], v5[:, :, 2]
        else:
            v5 = qkv.view(n, 3, heads, d, hh * ww)
            qq, kk, vv = v5[:, 0], v5[:, 1], v5[:, 2]
        s = (qq.transpose(2, 3) * d ** -0.5) @ kk if defect == NOOP_DEFECT else (qq.transpose(2, 3) * d ** -0.25) @ (kk * d ** -0.25)
        p = q(s.softmax(-1))
        y = q((p @ vv.transpose(2, 3)).transpose(2, 3).reshape(n, c, hh, ww))
        return q(conv(y, key + ".out_proj", 0) + t)

    def run(prog, t):
        for l in prog:
            if l[0] == "res":
                t = res(t, *l[1:])
            elif l[0] == "attn":
                t = attn(t, *l[1:])
            elif l[0] == "down":
                t = q(fir_down64(t, defect))
            else:
                t = q(fir_up64(t, defect))
        return t

    cond = cond.double()
    d_blocks, u_blocks = blocks(config)
    h = conv(q(x.double()), "proj_in", 0)
    keep("proj_in", h)
    skips = []
    for i, prog in enumerate(d_blocks):
        h = run(prog, h)
        skips.append(h)
        keep(f"d{i}", h)
    for i, prog in enumerate(u_blocks):
        if i > 0:
            h = torch.cat([h, skips[len(skips) - 1 - i]], dim=1)
        h = run(prog, h)
        keep(f"u{i}", h)
    y = F.conv2d(h, q(sd["proj_out.weight"].double()), sd["proj_out.bias"].double())
    keep("proj_out", y)
    return y


def roundings(config):
    """16-bit roundings along the longest path to each checkpoint (module doc): input 1, proj_in 1, a Res 5 (two AdaGN applies, conv1, conv2's
    own value, the sum), an Attn 6 (AdaGN, qkv, probabilities, output, out_proj's own value, the sum), a resampler 1."""
    feats, depths, channels, attn, _ = config
    R, k = {"proj_in": 2}, 2
    d_blocks, u_blocks = blocks(config)
    for name, progs in (("d", d_blocks), ("u", u_blocks)):
        for i, prog in enumerate(progs):
            k += sum({"res": 5, "attn": 6, "down": 1, "up": 1}[l[0]] for l in prog)
            R[f"{name}{i}"] = k
    R["proj_out"] = k
    return R


# ---- EDM ----------------------------------------------------------------------------------------------------------------------------------
def sig4(sigma, n):
    s = torch.as_tensor(sigma, dtype=torch.float64).reshape(-1)
    return (s.expand(n) if s.numel() == 1 else s)[:, None, None, None]


def c_skip64(s):
    return SIGMA_DATA ** 2 / (SIGMA_DATA ** 2 + s ** 2)


def c_out64(s):
    return s * SIGMA_DATA / torch.sqrt(SIGMA_DATA ** 2 + s ** 2)


def c_in64(s):
    return 1 / torch.sqrt(SIGMA_DATA ** 2 + s ** 2)


def c_noise64(s, defect=None):
    return s.log().reshape(-1) * (1.0 if defect == "c_noise_ln" else 0.25)


def denoised64(sd, images, sigma, config, *, aug=None, emulate=None, defect=None, record=None):
    """images NCHW in [0, 1], sigma one value or one per sample -> denoised_xs NCHW float64"""
    n = images.shape[0]
    x = images.double() * 2 - 1
    s1 = torch.as_tensor(sigma, dtype=torch.float64).reshape(-1)
    s = sig4(s1, n)
    cond = cond64(sd, c_noise64(s1, defect), aug, defect)
    if record is not None:
        record["cond"] = cond
    f = network64(sd, c_in64(s) * x, cond, config, emulate=emulate, defect=defect, record=record)
    a, b = c_skip64(s), c_out64(s)
    if defect == "cskip_cout_swapped":
        a, b = b, a
    return a * x + b * f


def eps64(images, denoised, sigma):
    return ((images.double() * 2 - 1) - denoised) / sig4(sigma, images.shape[0])


def step64(images, denoised, sigma, to_sigma):
    return (denoised + eps64(images, denoised, sigma) * sig4(to_sigma, images.shape[0]) + 1) / 2


def correction64(images, denoised, sigma, prev_images, prev_sigma, prev_eps, defect=None):
    n = images.shape[0]
    half = 1.0 if defect == "heun_no_half" else 0.5
    return ((prev_images.double() * 2 - 1) + (sig4(sigma, n) - sig4(prev_sigma, n)) * (eps64(images, denoised, sigma) + prev_eps) * half + 1) / 2


def inject64(images, sigma, rev_sigma, noise):
    n = images.shape[0]
    return ((images.double() * 2 - 1) + (sig4(rev_sigma, n) ** 2 - sig4(sigma, n) ** 2).sqrt() * noise.double() * S_NOISE + 1) / 2


# ---- schedule and samplers ----------------------------------------------------------------------------------------------------------------------
def schedule64(n_steps):
    ramp = torch.linspace(0, 1, n_steps, dtype=torch.float64)
    lo, hi = SIGMA_MIN ** (1 / RHO), SIGMA_MAX ** (1 / RHO)
    return (hi + ramp * (lo - hi)) ** RHO


def gamma64(ts, n_steps):
    g = min(S_CHURN / n_steps, math.sqrt(2.0) - 1)
    return torch.where((ts >= S_TMIN) & (ts <= S_TMAX), torch.full_like(ts, g), torch.zeros_like(ts))


def reversed64(ts, n_steps):
    return ts + gamma64(ts, n_steps) * ts


def lms_coeff64(order, sigmas, from_index, to_index):
    """integral over [sigma_from, sigma_from+1] of the Lagrange basis polynomial of node from - to among the last `order` nodes: a polynomial of
    degree order - 1, integrated exactly by Gauss-Legendre with 4 points"""
    s = [float(v) for v in sigmas]
    a, b = s[from_index], s[from_index + 1]
    nodes, wts = [-0.8611363115940526, -0.3399810435848563, 0.3399810435848563, 0.8611363115940526], \
                 [0.3478548451374538, 0.6521451548625461, 0.6521451548625461, 0.3478548451374538]
    tot = 0.0
    for xg, wg in zip(nodes, wts):
        tau = 0.5 * (b - a) * xg + 0.5 * (a + b)
        prod = 1.0
        for k in range(order):
            if k != to_index:
                prod *= (tau - s[from_index - k]) / (s[from_index - to_index] - s[from_index - k])
        tot += wg * prod
    return 0.5 * (b - a) * tot


def elucidated64(denoise, images, n_evaluations, noises, defect=None):
    """The stochastic Heun sampler on denoise(images, sigma) -> denoised_xs, with the recorded noise draws in order: the yielded images"""
    n_steps = n_evaluations // 2
    ts = schedule64(n_steps)
    out, x, k = [], images.double(), 0
    for a, b in zip(ts[:-1], ts[1:]):
        r = reversed64(a, n_steps).clamp(max=SIGMA_MAX)
        xr = inject64(x, a, r, noises[k]); k += 1
        d = denoise(xr, r)
        e = eps64(xr, d, r)
        x = step64(xr, d, r, b)
        d = denoise(x, b)
        x = correction64(x, d, b, xr, r, e, defect)
        out.append(((d + 1) / 2).clamp(0, 1))
    r = reversed64(ts[-1], n_steps)
    x = inject64(x, ts[-1], r, noises[k])
    out.append(((denoise(x, r) + 1) / 2).clamp(0, 1))
    return out


def lms_sample64(denoise, images, n_evaluations, order=4, coeffs_out=None):
    ts = schedule64(n_evaluations)
    out, x, epses = [], images.double(), []
    for i, (a, b) in enumerate(zip(ts[:-1], ts[1:])):
        d = denoise(x, a)
        epses.append(eps64(x, d, a))
        if len(epses) > order:
            epses.pop(0)
        cs = [lms_coeff64(len(epses), ts, i, j) for j in range(len(epses))]
        if coeffs_out is not None:
            coeffs_out.append(cs)
        x = ((x * 2 - 1) + sum(c * e for c, e in zip(cs, reversed(epses))) + 1) / 2
        out.append(((d + 1) / 2).clamp(0, 1))
    out.append(((denoise(x, ts[-1]) + 1) / 2).clamp(0, 1))
    return out


# ---- kernel references with per-element bounds (conventions of _routes16_ref64.py: E32 = 2^-24 per fp32 rounding, C_B = 1.5 for the second-order
# terms, u |y| (+ SUB for an f16 subnormal) per 16-bit rounding; no constant is fitted to a measurement) ------------------------------------------
from _norm_ref64 import C_B, E32  # noqa: E402

SUB, SUB_BELOW = 2.0 ** -25, 2.0 ** -14
FIR_DOWN_SHAPES = ((1, 2, 2, 32), (2, 4, 6, 64), (1, 12, 20, 96), (3, 48, 48, 128))      # N, H, W, C
FIR_UP_SHAPES = ((1, 2, 2, 32), (2, 3, 5, 64), (1, 6, 10, 96), (2, 24, 24, 256))
EDM_SIGMAS = (0.01, 0.5, 80.0)
EDM_SHAPE = (3, 3, 8, 12)


def out_rounding(v, dtype):
    t = U[dtype] * v.abs()
    return t + torch.where(v.abs() < SUB_BELOW, SUB, 0.0) if dtype == "f16" else t


def fir_input(shape, seed, dtype):
    """NHWC float64 values of the 16-bit type: a smooth interior would hide a border fault, so every sample (the border rows and columns
    with them) is an independent normal draw"""
    g = torch.Generator().manual_seed(seed)
    return rnd(torch.randn(shape, generator=g, dtype=torch.float64), dtype)


def fir_ref(x, which, dtype, defect=None):
    """x NHWC float64 -> (y NHWC float64, tol).  The tap weights (1, 3, 9 over 64; 9, 3, 3, 1 over 16) times a 16-bit value are exact in fp32, so
    the kernel rounds once per addition -- 16 resp. 4 terms -- and once at the store."""
    fn, terms = (fir_down64, 16) if which == "down" else (fir_up64, 4)
    xc = x.permute(0, 3, 1, 2)
    y = fn(xc, defect).permute(0, 2, 3, 1)
    S = fn(xc.abs()).permute(0, 2, 3, 1)
    return y, C_B * terms * E32 * S + out_rounding(y, dtype)


def fir_torch(x, which):
    """the same operators as torch states them (layers.py:208-241): F.pad(reflect) + conv2d / conv_transpose2d with the depthwise kernel"""
    xc = x.permute(0, 3, 1, 2)
    c = xc.shape[1]
    k = torch.tensor([[1 / 8, 3 / 8, 3 / 8, 1 / 8]], dtype=torch.float64)
    if which == "down":
        y = F.conv2d(F.pad(xc, (1,) * 4, "reflect"), (k.T @ k).expand(c, 1, 4, 4), stride=2, groups=c)
    else:
        y = F.conv_transpose2d(F.pad(xc, (1,) * 4, "reflect"), ((2 * k).T @ (2 * k)).expand(c, 1, 4, 4), stride=2, padding=3, groups=c)
    return y.permute(0, 2, 3, 1)


def edm_inputs(seed=5):
    g = torch.Generator().manual_seed(seed)
    f32 = lambda t: t.float().double()
    r = lambda: f32(torch.rand(EDM_SHAPE, generator=g, dtype=torch.float64))
    z = lambda: f32(torch.randn(EDM_SHAPE, generator=g, dtype=torch.float64))
    return dict(img=f32(r() * 3 - 1), net=z(), den=z(), prev_img=r(), prev_eps=z(), noise=z(), eps=[z() for _ in range(4)])


def edm_sigma_cases():
    """(sigma, to, previous, reversed) as float32-exact float64 vectors: one per sample, then every value as a scalar"""
    f32 = lambda v: torch.tensor(v, dtype=torch.float32).double()
    s = f32(list(EDM_SIGMAS))
    cases = [(s, f32([0.01, 0.3, 60.0]), f32([0.0125, 0.625, 80.0]), f32([0.01, 0.7, 80.0]))]
    for v in EDM_SIGMAS:
        cases.append((f32([v]), f32([v * 0.6]), f32([v * 1.25]), f32([v * 1.4142135])))
    return cases


def edm_stage_in_ref(img, sigma, dtype, defect=None):
    s = sig4(sigma, img.shape[0])
    v = c_in64(s) * (img * 2 - 1)
    cn = c_noise64(torch.as_tensor(sigma, dtype=torch.float64).reshape(-1), defect)
    # 2 img - 1: one rounding; c_in: sigma^2, the sum, the square root, the division; the product: six in all.  logf is within one ulp = 2 E32
    return v, C_B * 6 * E32 * v.abs() + out_rounding(v, dtype), cn, C_B * 2 * E32 * cn.abs()


def edm_stage_out_ref(img, net, sigma, defect=None):
    s = sig4(sigma, img.shape[0])
    a, b = c_skip64(s), c_out64(s)
    if defect == "cskip_cout_swapped":
        a, b = b, a
    t1, t2 = a * (img * 2 - 1), b * net
    # c_skip: sigma^2, the sum, the division (3) + x (1) + the product (1); c_out: sigma^2, the sum, the root, the division (4) + the product (1); the sum
    return t1 + t2, C_B * E32 * (5 * t1.abs() + 5 * t2.abs() + (t1 + t2).abs())


def edm_predict_ref(img, den, sigma, to_sigma, prev_img, prev_sigma, prev_eps, defect=None):
    """-> (eps, tol), (step, tol), (correction, tol)"""
    n = img.shape[0]
    s, st, sp = sig4(sigma, n), sig4(to_sigma, n), sig4(prev_sigma, n)
    x = img * 2 - 1
    e = (x - den) / s
    e_err = E32 * (x.abs() / s + 2 * e.abs())                       # x, the difference, the division
    t = den + e * st
    step = (t + 1) / 2
    step_err = 0.5 * (e_err * st + E32 * ((e * st).abs() + t.abs() + (t + 1).abs()))
    half = 1.0 if defect == "heun_no_half" else 0.5
    xp, d, ss = prev_img * 2 - 1, s - sp, e + prev_eps
    c = xp + d * ss * half
    corr = (c + 1) / 2
    ss_err = e_err + E32 * ss.abs()
    prod_err = half * (d.abs() * ss_err + 2 * E32 * (d * ss).abs())   # sigma - sigma_prev, the product
    corr_err = 0.5 * (E32 * xp.abs() + prod_err + E32 * (c.abs() + (c + 1).abs()))
    return (e, C_B * e_err), (step, C_B * step_err), (corr, C_B * corr_err)


def edm_inject_ref(img, sigma, rev_sigma, noise):
    n = img.shape[0]
    s, r = sig4(sigma, n), sig4(rev_sigma, n)
    x, diff = img * 2 - 1, r ** 2 - s ** 2
    root = diff.sqrt()
    diff_err = E32 * (r ** 2 + s ** 2 + diff.abs())
    root_err = torch.where(diff > 0, diff_err / (2 * root.clamp_min(1e-300)) + E32 * root, torch.zeros_like(root))
    t = root * noise * S_NOISE
    # the noise product, S_noise as an fp32 constant and its product: three more on the term
    t_err = root_err * (noise * S_NOISE).abs() + 3 * E32 * t.abs()
    y = x + t
    return (y + 1) / 2, C_B * 0.5 * (E32 * x.abs() + t_err + E32 * (y.abs() + (y + 1).abs()))


def edm_lms_ref(img, coeffs, epses):
    x = img * 2 - 1
    acc = sum(c * e for c, e in zip(coeffs, epses))
    S = sum(abs(c) * e.abs() for c, e in zip(coeffs, epses))
    y = x + acc
    # per term: the coefficient as fp32, the product, the addition
    return (y + 1) / 2, C_B * 0.5 * (E32 * x.abs() + 3 * len(coeffs) * E32 * S + E32 * (y.abs() + (y + 1).abs()))


# ---- the engine tests' networks and inputs ---------------------------------------------------------------------------------------------------
NETS = {"A": ((64, [1, 2, 2], [32, 64, 128], [False, True, True], 9), (2, 3, 8, 12)),
        "B": ((64, [2, 1, 1], [64, 64, 128], [False, False, True], 9), (3, 3, 16, 16))}
PRODUCT = (256, [2, 4, 4], [128, 256, 512], [False, True, True], 9)
CHECKPOINTS = ("proj_in", "d0", "d1", "d2", "u0", "u1", "u2", "proj_out")


def synthetic_state_dict(config, seed=0):
    """the synthetic weights of models.MonsterDiffusion(weights="synthetic", seed=seed, config=config) and of the fixture"""
    from perceptor_amd.engine.monster import synthetic_state_dict as synth
    return synth(config, seed)


def product_case():
    """(images [2, 3, 48, 48] float32, sigma [2]) of the product-config test"""
    g = torch.Generator().manual_seed(48)
    return torch.rand((2, 3, 48, 48), generator=g), torch.tensor([0.5, 5.0])


def sampled(t, g, name):
    """t as the fixture stores `name`: every s-th value of the flattened tensor where it was larger than the cap"""
    return t.reshape(-1)[::int(g[name + "_stride"])] if name + "_stride" in g else t


def cond_ref(sd, sigma):
    """(cond, tol) of the engine's fp32 conditioning at zero augmentations, per element: the Fourier argument 2 pi c_noise w carries c_noise's
    two ulp-level errors and three roundings (6 E32 |f|), cos / sin one more; a linear layer adds C_B (K + 2) E32 (|W| |x| + |b|) to |W| err;
    GELU (fast_erff, _routes16_ref64.GELU_HW) adds GELU_HW |z| to 1.13 err"""
    gelu_hw, gelu_lip = 0.5 * 1.5e-7 + 4 * E32, 1.13
    c = c_noise64(torch.as_tensor(sigma, dtype=torch.float64).reshape(-1))
    f = 2 * math.pi * c.reshape(-1, 1) @ sd["timestep_embed.weight"].double().T
    x = torch.cat([f.cos(), f.sin()], dim=-1)
    err = torch.cat([6 * E32 * f.abs() + 2 * E32] * 2, dim=-1)
    for i in (0, 2):
        W, b = sd[f"mapping.{i}.weight"].double(), sd[f"mapping.{i}.bias"].double()
        z = x @ W.T + b
        err = err @ W.abs().T + C_B * (W.shape[1] + 2) * E32 * (x.abs() @ W.abs().T + b.abs())
        x, err = F.gelu(z), gelu_lip * err + gelu_hw * z.abs()
    return x, C_B * err


# ---- gates of tests/test_gpu_monster.py (its header states the rule).  rel-L2 of the emulated restatement (emulate=dtype) against the float64
# values, measured on the CPU; tests/test_monster_diffusion_cpu.py measures them again ---------------------------------------------------------
EMU = {  # rel-L2 of the emulated restatement against the fixture, per checkpoint
    ("A", "bf16"): {"proj_in": 2.205797e-03, "d0": 3.751052e-03, "d1": 4.642911e-03, "d2": 4.604879e-03, "u0": 4.318626e-03, "u1": 4.571544e-03,
                    "u2": 5.720625e-03, "proj_out": 4.318832e-03, "denoised_xs": 4.045637e-03},
    ("A", "f16"): {"proj_in": 3.014103e-04, "d0": 4.620737e-04, "d1": 6.013347e-04, "d2": 5.911704e-04, "u0": 5.271783e-04, "u1": 5.447367e-04,
                   "u2": 6.350594e-04, "proj_out": 5.303222e-04, "denoised_xs": 5.108709e-04},
    ("B", "bf16"): {"proj_in": 2.354723e-03, "d0": 5.178825e-03, "d1": 4.512581e-03, "d2": 3.643357e-03, "u0": 3.839799e-03, "u1": 4.366415e-03,
                    "u2": 6.168064e-03, "proj_out": 7.887155e-03, "denoised_xs": 7.935184e-03},
    ("B", "f16"): {"proj_in": 2.965535e-04, "d0": 6.603149e-04, "d1": 5.422980e-04, "d2": 4.718993e-04, "u0": 4.734859e-04, "u1": 5.726518e-04,
                   "u2": 7.720617e-04, "proj_out": 9.208297e-04, "denoised_xs": 9.396837e-04},
}
EMU_PRODUCT = {"bf16": 9.676955e-03, "f16": 1.164707e-03}          # emulated restatement against the float64 one, product config, product_case()
EMU_HEUN = {"bf16": (3.699635e-03, 7.842447e-03, 1.296212e-02), "f16": (5.745537e-04, 7.835820e-04, 1.364000e-03)}      # per yield, network A
EMU_LMS = {"bf16": (4.276146e-03, 3.149861e-03, 3.387839e-03, 3.156992e-03, 2.565888e-03, 2.510505e-03),
           "f16": (3.882820e-04, 3.851710e-04, 4.060732e-04, 4.352434e-04, 3.182510e-04, 3.116934e-04)}


def gate(net, dtype, key):
    """proj_in (before any normalisation): sqrt(R) u with R counted by roundings(); behind a GroupNorm or a softmax: 2 x the emulation's distance"""
    return math.sqrt(roundings(NETS[net][0])["proj_in"]) * U[dtype] if key == "proj_in" else 2 * EMU[(net, dtype)][key]


# ---- one AdaGN + GELU layer as the engine launches it (ops.group_norm with film, exact GELU): the element-wise check that tells erf-GELU from
# its tanh form, which the 16-bit checkpoints' gates cannot (it moves them by 0.02 - 0.4 of a gate) ------------------------------------------------
ADAGN_SHAPE = (2, 8, 12, 64)


def adagn_case(dtype, seed=21):
    """x NHWC float64 of the 16-bit type with values out to |x| ~ 4 after the norm (the tails are where the two GELU forms part), film [N, 2C]"""
    g = torch.Generator().manual_seed(seed)
    x = rnd(torch.randn(ADAGN_SHAPE, generator=g, dtype=torch.float64) * 1.5 + 0.3, dtype)
    film = (torch.randn((ADAGN_SHAPE[0], 2 * ADAGN_SHAPE[3]), generator=g, dtype=torch.float64) * 0.3).float().double()
    return x, film


def adagn_ref(x, film, dtype, defect=None):
    """(y, tol): the statistics and coefficient bounds are _norm_ref64.gn_coeffs_ref's (pmi_gn_stats + pmi_gn_finalize, standalone depth); then
    z = a x + b in fp32, GELU with fast_erff (|error| <= 1.5e-7 on erf, so 0.75e-7 |z| on the value, plus four fp32 operations), Lipschitz
    constant 1.13, and the store's rounding"""
    import _norm_ref64 as NR
    n, h, w, c = x.shape
    film = film.expand(n, -1)
    co = NR.gn_coeffs_ref(x, max(1, c // 32), 1e-5, film=film, depth=NR.standalone_depth(n, h * w, c))
    a, b = co["a"][:, None, None, :], co["b"][:, None, None, :]
    z = x * a + b
    ez = x.abs() * co["da"][:, None, None, :] + co["db"][:, None, None, :] + 2 * E32 * ((x * a).abs() + b.abs())
    y = gelu64(z, defect)
    return y, C_B * (1.13 * ez + 0.75e-7 * z.abs() + 4 * E32 * y.abs()) + out_rounding(y, dtype)
