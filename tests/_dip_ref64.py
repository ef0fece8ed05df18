"""float64 restatement of the DeepImagePrior skip network (engine/dip.py) and of each operator its kernels compute, in this file's own words;
checked against the reference module's own values in tests/golden/deep_image_prior_reference.npz by tests/test_deep_image_prior_cpu.py.

Network, per scale with input x (Cin = the latents' channels at scale 0, 192 below):
  skip    = lrelu(BN(conv1x1(x)))                                              4 channels
  deeper  = up(next(lrelu(BN(conv3x3(lrelu(BN(down(conv3x3(x)))))))))          192 channels; `next` is the next scale or nothing
  out     = lrelu(BN(conv1x1(lrelu(BN(conv3x3(BN(cat[skip | deeper])))))))
  picture = sigmoid(colcorr_t^T (conv1x1(out)))                                at the top
conv3x3 reflect-pads by 1; down = reflect-pad 3, 8-tap cubic k k^T, stride 2; up = reflect-pad 2, conv_transpose2d with (2k)(2k)^T, stride 2,
padding 7; BN is training-mode BatchNorm2d (biased variance in the normalisation, unbiased in the running statistics, momentum 0.1,
eps 1e-5); lrelu has slope 0.2.  Gradients are autograd over these float64 expressions.

emulate = "bf16" | "f16" (network64): every activation the engine STORES is rounded to that type -- the latents, each convolution's output,
each resampler's output, each BatchNorm + activation output -- and so is the gradient of each of them on the way back (the cast's own
backward rounds the cotangent, f16 under the engine's power-of-two scale); convolution weights are rounded where a convolution reads them
(forward and dX), never in the weight gradient's result.  Statistics, parameters and parameter gradients stay float64.  The deviation of
this mode from pure float64 is the FLOOR the GPU tolerances are set from: it is measured on the CPU, not on the code under test.

Per-kernel operators return (value, sum |terms|).  K, the fp32 roundings on the way to one result of a kernel as written (bound per element:
K 2^-24 sum|terms| + the 16-bit roundings of the inputs' and the output's type, u16 = 2^-8 bf16 / 2^-11 f16 -- the tests' inputs are
exactly representable, so only the output rounding is added: u16 |value|, or 2^-25 in f16's subnormal range):
  wgrad (MFMA route)   exact products; fp32 accumulation of P terms in the MFMA, <= 64 slabs, alpha         K = P_split + splits + 1
  wgrad (plain route)  one fma per term, <= 64 slabs, alpha                                               K = P_split + splits + 1
  bn_stats mean        partial sums of <= ceil(P / blocks) terms over R rows, blocks <= 256, 1 / P          K = P_blk + blocks + 1
  bn_stats rstd        d = x - mean (1), d^2 fma, sums as the mean, + eps, sqrt, 1 / .                     K = P_blk + blocks + 6   (relative, on var + eps)
  bn_apply             a = gamma rstd, b = fma, v = fma, slope                                            K = 4 (+ the statistics' own error through a, b)
  bn_bwd sums          dy' (1), xhat (2), fma, partial sums as above                                      K = P_blk + blocks + 4
  bn_bwd dx            a, dy', xhat, two means, two subtractions, product                                 K = 10
  fir8 down / up       64 resp. 16 fma terms, weights exact                                              K = 64 resp. 16 (+ 1 product rounding)
  fir8 adjoints        <= 144 resp. 576 gathered terms, one fma each                                     K = the term count + 1
  pad_fold             <= 10 terms                                                                        K = 10
  head fwd             Cin fma terms + bias + 3-term matrix + sigmoid (exp, add, divide: 4 ulp)          K = Cin + 8
The tests take K from kernel_k() below, which restates this table.

DEFECTS are the planted faults of the CPU test: each is a switch in the expressions below.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from perceptor_amd.engine import dip as E

DEFECTS = ("running_var_biased", "bn_bwd_no_mean", "bn_bwd_no_xhat", "lrelu_bwd_slope_1", "lrelu_bwd_slope_0", "border_clamp", "border_zero",
           "wgrad_kykx_swapped", "wgrad_no_ring", "up_kernel_not_doubled", "adjoint_no_folds", "concat_deeper_skip", "colour_transposed",
           "stale_weight_pack")
# the faults that change the whole network's values or gradients (the rest live in one kernel's backward arithmetic, which autograd replaces here)
NETWORK_DEFECTS = ("running_var_biased", "lrelu_bwd_slope_1", "lrelu_bwd_slope_0", "border_clamp", "border_zero", "wgrad_kykx_swapped",
                   "up_kernel_not_doubled", "concat_deeper_skip", "colour_transposed", "stale_weight_pack")
U16 = {"bf16": 2.0 ** -8, "f16": 2.0 ** -11}            # unit roundoff: 8 resp. 11 significant bits
TDT = {"bf16": torch.bfloat16, "f16": torch.float16}
K1 = torch.tensor(E.CUBIC, dtype=torch.float64)


def out_rounding(dt, v: torch.Tensor) -> torch.Tensor:
    """the rounding of a value stored in the 16-bit type: half an ulp, u16 |v| for a normal value and 2^-25 in f16's subnormal range
    (spacing 2^-24 below 2^-14; bf16's subnormals lie below 1e-38)"""
    return U16[dt] * v.abs() + (2.0 ** -25 if dt == "f16" else 0.0)


def rnd(x: torch.Tensor, dt) -> torch.Tensor:
    return x if dt is None else x.to(torch.float32).to(TDT[dt]).to(torch.float64)


class _Store(torch.autograd.Function):
    """A value the engine keeps in 16 bit: rounded forward, its cotangent rounded (under `scale`) backward."""

    @staticmethod
    def forward(ctx, x, dt, scale):
        ctx.dt, ctx.scale = dt, scale
        return rnd(x, dt)

    @staticmethod
    def backward(ctx, g):
        return rnd(g * ctx.scale, ctx.dt) / ctx.scale, None, None


class _LReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slope_bwd):
        ctx.save_for_backward(x)
        ctx.slope = slope_bwd
        return torch.where(x > 0, x, 0.2 * x)

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        return g * torch.where(x > 0, torch.ones_like(x), torch.full_like(x, ctx.slope)), None


def pad_mode(defect):
    return {"border_clamp": "replicate", "border_zero": "constant"}.get(defect, "reflect")


def down64(x, defect=None):
    """[N, C, H, W] -> [N, C, H/2, W/2]"""
    c = x.shape[1]
    k = torch.outer(K1, K1)[None, None].expand(c, 1, 8, 8)
    return F.conv2d(F.pad(x, (3,) * 4, pad_mode(defect)), k, stride=2, groups=c)


def up64(x, defect=None):
    """[N, C, H, W] -> [N, C, 2H, 2W]"""
    c = x.shape[1]
    k1 = K1 if defect == "up_kernel_not_doubled" else 2 * K1
    k = torch.outer(k1, k1)[None, None].expand(c, 1, 8, 8)
    return F.conv_transpose2d(F.pad(x, (2,) * 4, pad_mode(defect)), k, stride=2, padding=7, groups=c)


def adjoint64(op, shape, y, defect=None):
    """A^T y of the linear map `op` on inputs of `shape` -- for the defect, of the map without its reflection (zero border)."""
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    out = op(x, "border_zero" if defect == "adjoint_no_folds" else None)
    return torch.autograd.grad(out, x, y)[0]


def pad1(x, defect=None):
    return F.pad(x, (1,) * 4, pad_mode(defect))


def bn_train64(x, gamma, beta, act, slope_bwd=0.2):
    """(y, mean, biased var) of training-mode BatchNorm2d + optional LeakyReLU over [N, C, H, W]"""
    mean = x.mean(dim=(0, 2, 3))
    var = ((x - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
    y = (x - mean[None, :, None, None]) * torch.rsqrt(var + E.BN_EPS)[None, :, None, None] * gamma[None, :, None, None] + beta[None, :, None, None]
    return (_LReLU.apply(y, slope_bwd) if act else y), mean, var


def bn_bwd64(x, dy, gamma, beta, act, defect=None):
    """The explicit BatchNorm backward the kernels compute: (dx, dgamma, dbeta, sum|terms| of dgamma, of dbeta)"""
    p = x.shape[0] * x.shape[2] * x.shape[3]
    sh = (1, -1, 1, 1)
    mean = x.mean(dim=(0, 2, 3)).view(sh)
    var = ((x - mean) ** 2).mean(dim=(0, 2, 3)).view(sh)
    rstd = torch.rsqrt(var + E.BN_EPS)
    xh = (x - mean) * rstd
    pre = xh * gamma.view(sh) + beta.view(sh)
    slope = {"lrelu_bwd_slope_1": 1.0, "lrelu_bwd_slope_0": 0.0}.get(defect, 0.2)
    g = dy * torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope)) if act else dy
    s1, s2 = g.sum(dim=(0, 2, 3)), (g * xh).sum(dim=(0, 2, 3))
    m1 = 0.0 if defect == "bn_bwd_no_mean" else s1.view(sh) / p
    m2 = 0.0 if defect == "bn_bwd_no_xhat" else s2.view(sh) / p
    dx = gamma.view(sh) * rstd * (g - m1 - xh * m2)
    return dx, s2, s1, (g * xh).abs().sum(dim=(0, 2, 3)), g.abs().sum(dim=(0, 2, 3))


def wgrad64(dy, x, taps, defect=None):
    """dy [N, Co, H, W], x [N, Ci, H, W] -> (dW [Co, Ci, k, k], db [Co], sum|terms| of dW, of db) of a reflect-padded convolution"""
    n, co, h, w = dy.shape
    if taps == 1:
        return (torch.einsum("nohw,nihw->oi", dy, x)[:, :, None, None], dy.sum(dim=(0, 2, 3)),
                torch.einsum("nohw,nihw->oi", dy.abs(), x.abs())[:, :, None, None], dy.abs().sum(dim=(0, 2, 3)))
    xp = pad1(x, "border_zero" if defect == "wgrad_no_ring" else None)
    dW, aW = torch.zeros(co, x.shape[1], 3, 3, dtype=torch.float64), torch.zeros(co, x.shape[1], 3, 3, dtype=torch.float64)
    for ky in range(3):
        for kx in range(3):
            win = xp[:, :, ky:ky + h, kx:kx + w]
            dW[:, :, ky, kx] = torch.einsum("nohw,nihw->oi", dy, win)
            aW[:, :, ky, kx] = torch.einsum("nohw,nihw->oi", dy.abs(), win.abs())
    if defect == "wgrad_kykx_swapped":
        dW = dW.transpose(2, 3).contiguous()
    return dW, dy.sum(dim=(0, 2, 3)), aW, dy.abs().sum(dim=(0, 2, 3))


def head64(x, w, b, cm, sigmoid, defect=None):
    """x [N, C, H, W] -> the picture; cm = colcorr_t or None"""
    z = F.conv2d(x, w, b)
    if cm is not None:
        z = torch.einsum("nchw,cd->ndhw", z, cm.T if defect == "colour_transposed" else cm)
    return torch.sigmoid(z) if sigmoid else z


def kernel_k(kind: str, p: int = 0, cin: int = 0) -> int:
    """K of the table in this file's docstring; p = the pixels a reduction runs over"""
    blocks = max(1, min(256, (p + 63) // 64))
    p_blk = -(-p // blocks) if p else 0
    if kind == "wgrad":
        return p + 64 + 1                      # (P_split <= P: the bound does not depend on the split count chosen)
    return {"bn_mean": p_blk + blocks + 1, "bn_rstd": p_blk + blocks + 6, "bn_apply": 4, "bn_bwd_sums": p_blk + blocks + 4, "bn_bwd_dx": 10,
            "down": 65, "up": 17, "down_bwd": 145, "up_bwd": 577, "fold": 10, "head": cin + 8}[kind]


def to64(sd, grad=True):
    out = {}
    for k, v in sd.items():
        if torch.is_floating_point(v):
            out[k] = v.detach().to(torch.float64).clone().requires_grad_(grad and not k.endswith(("running_mean", "running_var", "kernel", "colcorr_t")))
        else:
            out[k] = v.clone()
    return out


def network64(sd, latents, n_scales, *, sigmoid=True, decorrelate=True, train=True, defect=None, emulate=None, grad_scale=1.0, conv_sd=None,
              abs_terms=None):
    """(picture [N, Cout, H, W], {running-statistic name: updated value}).  sd: float64 tensors by reference key name (to64); conv_sd: the
    dictionary the convolutions read their weights from (the stale-pack fault passes the previous step's).  abs_terms: a dict that a backward
    pass fills with sum |cotangent| per channel of every convolution output (key <conv>.bias) and every BN(196) output (key <bn>.bias):
    the sum |terms| of the bias gradients that are analytically zero."""
    if defect == "stale_weight_pack" and conv_sd is None:
        raise ValueError("the stale-pack fault needs the previous step's weights in conv_sd")
    csd = sd if conv_sd is None or defect != "stale_weight_pack" else conv_sd
    slope = {"lrelu_bwd_slope_1": 1.0, "lrelu_bwd_slope_0": 0.0}.get(defect, 0.2)
    pdef = defect if defect in ("border_clamp", "border_zero") else None
    q = (lambda t: t) if emulate is None else (lambda t: _Store.apply(t, emulate, grad_scale))
    qw = (lambda t: t) if emulate is None else (lambda t: rnd(t.detach(), emulate) + (t - t.detach()))      # rounded value, gradient passed on
    stats = {}

    def conv(x, name, k):
        w, b = qw(csd[name + ".weight"]), csd[name + ".bias"]
        if defect == "wgrad_kykx_swapped" and k == 3:
            w = _SwapGrad.apply(w)
        y = F.conv2d(pad1(x, pdef) if k == 3 else x, w, b)
        if abs_terms is not None and y.requires_grad:
            y.register_hook(lambda g: abs_terms.__setitem__(name + ".bias", g.abs().sum(dim=(0, 2, 3))))
        return y

    def bn(x, name, act):
        if train:
            y, mean, var = bn_train64(x, sd[name + ".weight"], sd[name + ".bias"], act, slope)
            p = x.shape[0] * x.shape[2] * x.shape[3]
            unb = 1.0 if defect == "running_var_biased" else p / (p - 1)
            stats[name + ".running_mean"] = (0.9 * sd[name + ".running_mean"] + 0.1 * mean).detach()
            stats[name + ".running_var"] = (0.9 * sd[name + ".running_var"] + 0.1 * var * unb).detach()
            if abs_terms is not None and not act and y.requires_grad:
                y.register_hook(lambda g: abs_terms.__setitem__(name + ".bias", g.abs().sum(dim=(0, 2, 3))))
            return y
        sh = (1, -1, 1, 1)
        y = (x - sd[name + ".running_mean"].view(sh)) * torch.rsqrt(sd[name + ".running_var"].view(sh) + E.BN_EPS) * sd[name + ".weight"].view(sh) \
            + sd[name + ".bias"].view(sh)
        return _LReLU.apply(y, slope) if act else y

    def scale(i, p, x):
        sa = q(bn(q(conv(x, p + ".1.0.1.1", 1)), p + ".1.0.2", True))
        d = q(down64(q(conv(x, p + ".1.1.1.1", 3)), pdef))
        e = q(bn(q(conv(q(bn(d, p + ".1.1.2", True)), p + ".1.1.4.1", 3)), p + ".1.1.5", True))
        f = e if i == n_scales - 1 else scale(i + 1, p + ".1.1.7", e)
        u = q(up64(f, defect if defect == "up_kernel_not_doubled" else pdef))
        if defect == "concat_deeper_skip":
            cat = torch.cat([u, sa], 1)
        else:
            cat = torch.cat([sa, u], 1)
        g = q(bn(q(conv(q(bn(cat, p + ".2", False)), p + ".3.1", 3)), p + ".4", True))
        return q(bn(q(conv(g, p + ".6.1", 1)), p + ".7", True))

    feat = scale(0, "network", q(latents))
    out = head64(feat, csd["network.9.1.weight"] if defect == "stale_weight_pack" else sd["network.9.1.weight"], sd["network.9.1.bias"],
                 sd["network.10.colcorr_t"] if decorrelate else None, sigmoid, defect)
    return out, stats


class _SwapGrad(torch.autograd.Function):
    """The ky / kx fault: the value passes, the weight gradient comes back with its two tap axes exchanged."""

    @staticmethod
    def forward(ctx, w):
        return w.view_as(w)

    @staticmethod
    def backward(ctx, g):
        return g.transpose(2, 3).contiguous()


def is_conv(name):
    return name.rsplit(".", 2)[-2] == "1" and not name.startswith("network.9.")


def tensor_class(name):
    if name in ("out", "dlatents"):
        return name
    if name.endswith(("running_mean", "running_var")):
        return "stats"
    if name.startswith("network.9."):
        return "head"
    return "conv_w" if is_conv(name) else "bn"


def zero_gradient_names(sd):
    """Parameters whose gradient is analytically zero: every convolution bias that feeds a BatchNorm, and the biases of BN(196), which a
    reflect-padded convolution turns into a per-channel constant the next BatchNorm removes."""
    return [k for k in sd if (k.endswith(".bias") and is_conv(k)) or (k.endswith(".2.bias") and tuple(sd[k].shape) == (196,))]


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


# ---- the cases shared by the fixture generator and the tests ----------------------------------------------------------------------------------
CIN = 64
CASES = [(2, 16, 1), (2, 16, 2), (1, 8, 2), (3, 24, 1)]           # (n_scales, size, N): what tests/golden/deep_image_prior_reference.npz holds
GPU_CASES = CASES + [(2, 40, 1)]
# whole-network tolerance = floor x MARGIN per tensor class (floor: the 16-bit emulation's relative L2 deviation from float64, on the CPU);
# MARGIN = twice the largest GPU / floor ratio measured on an MI355X.  DRAWER_MARGIN: loss after 30 Adam steps.
# largest measured ratios: out 1.08, dlatents 1.18, conv_w 1.38, bn 2.33, stats 5.90, head 5.36
MARGIN = {"out": 2.16, "dlatents": 2.36, "conv_w": 2.76, "bn": 4.66, "stats": 11.8, "head": 10.72}
# GPU loss / restatement loss after 30 Adam steps, seeds 0, 1, 2: 0.974, 1.063, 1.060 -> 1 + twice the largest deviation from 1
DRAWER_MARGIN = 1.13
SMALL = 4096                                                     # parameters up to this many elements have their whole gradient in the fixture
STRIDE = 997


def case_name(case):
    return "s%d_%d_n%d" % case


def case_inputs(case):
    """(latents [N, CIN, S, S], cotangent [N, 3, S, S]) fp32, seeded; the loss is sum(picture * cotangent)"""
    from perceptor_amd.utils.synth import seeded_noise
    ns, size, n = case
    seed = 1000 * ns + 10 * size + n
    return 0.1 * seeded_noise((n, CIN, size, size), seed), seeded_noise((n, 3, size, size), seed + 1)


def contraction(name, grad):
    """(sum(grad * r), grad.flatten()[::STRIDE]) with r seeded from the parameter's name"""
    import zlib
    from perceptor_amd.utils.synth import seeded_noise
    r = seeded_noise(tuple(grad.shape), zlib.crc32(name.encode())).double()
    return (grad.double() * r).sum().reshape(1), grad.double().flatten()[::STRIDE].clone()


def run_case64(case, *, defect=None, emulate=None, sd=None, conv_sd=None, train=True):
    """The restatement on a fixture case: (picture, d latents, {name: gradient}, {name: running statistic})"""
    ns, size, n = case
    sd = to64(E.synthetic_state_dict(ns, CIN)) if sd is None else sd
    lat32, cot32 = case_inputs(case)
    lat = lat32.double().requires_grad_(True)
    cot = cot32.double()
    scale = 1.0
    if emulate == "f16":
        import math
        scale = 2.0 ** max(-24, min(24, -math.ceil(math.log2(float(cot.abs().max())))))
    out, stats = network64(sd, lat, ns, train=train, defect=defect, emulate=emulate, grad_scale=scale, conv_sd=conv_sd)
    names = [k for k, v in sd.items() if torch.is_floating_point(v) and v.requires_grad]
    grads = torch.autograd.grad((out * cot).sum(), [lat] + [sd[k] for k in names], allow_unused=True)
    g = {k: (torch.zeros_like(sd[k]) if v is None else v) for k, v in zip(names, grads[1:])}
    return out.detach(), grads[0], g, stats
