"""float64 restatement of Real-ESRGAN's U-Net discriminator path (engine/disc.py, losses/super_resolution_discriminator.py): network, loss and
image gradient, the seeded defects, and the per-element bounds of csrc/disc.hip's kernels.  Conventions of _routes16_ref64.py, whose
operand regimes, chain_len and out_rounding are used as they are.

Network (own words; lrelu = LeakyReLU(0.2), up = bilinear x2 with align_corners=False, written as a matrix per axis: out[2i] = x[i-1] / 4 +
3 x[i] / 4, out[2i+1] = 3 x[i] / 4 + x[i+1] / 4 with the index clamped at the border):
  x0 = lrelu(conv0(x)), x1 = lrelu(conv1(x0)), x2 = lrelu(conv2(x1)), x3 = lrelu(conv3(x2))      conv1-3: 4x4, stride 2, pad 1
  x4 = lrelu(conv4(up x3)) + x2, x5 = lrelu(conv5(up x4)) + x1, x6 = lrelu(conv6(up x5)) + x0
  logits = conv9(lrelu(conv8(lrelu(conv7(x6)))));  loss = -0.001 sum(logits) / (n_total H W)
with conv1 .. conv8's weights weight_orig / (u . weight_orig v).  The gradient is written out by hand: each 3x3 adjoint is the convolution
with transposed, flipped weights, the up-sampler's adjoint the transposed matrix, and the adjoint of a 4x4 stride-2 convolution is taken BY
PHASE as csrc/disc.hip does: hi-res pixel (2p + a, 2q + b) gets taps ky = 3 - 2u (a = 0) or 2 - 2u (a = 1) from the low-res gradient at
p + a - 1 + u (kx alike), zero outside.

Against tests/golden/sr_discriminator_reference.npz (the reference's own module in float64, eval mode, autograd), measured when this file
was written: logits rel-L2 <= 1.5e-15, loss rel <= 2.0e-16, gradient rel-L2 <= 7.9e-16 over the three cases.

emulate = "f16" | "bf16" rounds exactly where the engine stores 16 bit: the staged input, the weights, every convolution's output
(pmi_rdb_conv3x3, on conv6 .. conv8 at F = 64 and conv5 .. conv8 at F = 32, stores lrelu(z), ops.igemm stores z and pmi_lrelu_add the activation), every up-sampling,
every skip addition, and in the backward the seed, every adjoint convolution, mask and up-sampler adjoint.  ROUNDINGS counts them along the
longest path: 20 to the logits (input 1, conv0 2, conv1-3 2 each, then up + conv + add 3 per decoder level, conv7, conv8), 19 in the backward
(seed, conv9^T, 2 x (mask, conv^T), then mask + conv^T + up^T 3 per level, the mask of x3, three pmi_convt4x4s2).  The gradient is piecewise
linear in the signs alone, so with pinned signs no forward rounding reaches it.

Bound of one pmi_convt4x4s2 call, per element (u = 2^-11 f16, 2^-8 bf16; S = sum |g| |w| over the phase's 4 Cout terms):
  accumulation  C_B chain_len(4 Cout, 1) E32 S
  addition      C_B E32 |acc + R| where R is present
  mask          the terms above times |slope| where Y < 0, plus E32 |D| for that multiplication
  output        u |D| (+ SUB where an f16 result may be subnormal); nothing for an fp32 D
No constant is fitted to a measurement.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from _routes16_ref64 import C_B, E32, TD, U, chain_len, margin, operand, out_rounding, rnd, weights  # noqa: F401

SLOPE, LOSS_SCALE = 0.2, 0.001
SN = tuple(range(1, 9))
ROUNDINGS = {"logits": 20, "grad": 19}
TAPE_ROUNDINGS = {"x0": 3, "x1": 5, "x2": 7, "x3": 9, "s4": 11, "x4": 12, "s5": 14, "x5": 15, "s6": 17, "x6": 18, "s7": 19, "s8": 20}
GRAD_ROUNDINGS = {"d_a8": 2, "d_a7": 4, "d_x6": 6, "d_x5": 9, "d_x4": 12, "d_x3": 15, "d_z3": 16, "d_z2": 17, "d_z1": 18, "d_z0": 19}
DEFECTS = ("sigma_kept", "skip_before_lrelu", "align_corners", "ky_flipped", "slope1_mask", "skip_grad_dropped", "nearest_adjoint",
           "mean_n", "scale_missing", "sign_missing")


def grad_scale(dtype, count):
    """the engine's power-of-two factor on the backward's 16-bit tensors: 1 in bf16; in f16 the one that brings |d logits| = 0.001 / count
    into (0.5, 1], at most 2^24 (ops.f16_grad_scale, restated)"""
    if dtype != "f16":
        return 1.0
    return 2.0 ** max(-24, min(24, -math.ceil(math.log2(LOSS_SCALE / count))))


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


def fused_layers(num_feat):
    """the decoder layers engine/disc.py gives to pmi_rdb_conv3x3 (Cin % 32 == 0, 32 .. 192, N in {32, 64}): conv6 .. conv8 at F = 64, conv5 ..
    conv8 at F = 32"""
    f = num_feat
    shapes = {4: (8 * f, 4 * f), 5: (4 * f, 2 * f), 6: (2 * f, f), 7: (f, f), 8: (f, f)}
    return tuple(k for k, (cin, n) in shapes.items() if cin % 32 == 0 and 32 <= cin <= 192 and n in (32, 64))


def fold64(sd, defect=None):
    """{k: weight of conv k in float64} with the eval-mode spectral norm divided out, and the two biases"""
    W = {}
    for k in range(10):
        if k in SN:
            w = sd[f"conv{k}.weight_orig"].double()
            sigma = sd[f"conv{k}.weight_u"].double() @ (w.reshape(w.shape[0], -1) @ sd[f"conv{k}.weight_v"].double())
            W[k] = w if (defect == "sigma_kept" and k == 5) else w / sigma
        else:
            W[k] = sd[f"conv{k}.weight"].double()
    return W, sd["conv0.bias"].double(), sd["conv9.bias"].double()


# ---- pieces (NHWC float64) ---------------------------------------------------------------------------------------------------------
def conv(x, w, stride=1):
    return F.conv2d(x.permute(0, 3, 1, 2), w, stride=stride, padding=1).permute(0, 2, 3, 1)


def conv_t3(g, w):
    """adjoint of the 3x3 pad-1 convolution with weights w [Cout, Cin, 3, 3]: the convolution with transposed, flipped weights"""
    return conv(g, w.permute(1, 0, 2, 3).flip(2, 3))


def up_matrix(n, kind="bilinear"):
    M = torch.zeros(2 * n, n, dtype=torch.float64)
    for i in range(n):
        if kind == "nearest":
            M[2 * i, i] = M[2 * i + 1, i] = 1.0
        elif kind == "bilinear":
            M[2 * i, max(i - 1, 0)] += 0.25
            M[2 * i, i] += 0.75
            M[2 * i + 1, i] += 0.75
            M[2 * i + 1, min(i + 1, n - 1)] += 0.25
    if kind == "align_corners":
        for o in range(2 * n):
            s = o * (n - 1) / (2 * n - 1) if n > 1 else 0.0
            i0 = min(int(s), n - 1)
            i1 = min(i0 + 1, n - 1)
            M[o, i0] += 1.0 - (s - i0)
            M[o, i1] += s - i0
    return M


def up2(x, kind="bilinear"):
    return torch.einsum("oh,pw,nhwc->nopc", up_matrix(x.shape[1], kind), up_matrix(x.shape[2], kind), x)


def up2_t(g, kind="bilinear"):
    return torch.einsum("oh,pw,nopc->nhwc", up_matrix(g.shape[1] // 2, kind), up_matrix(g.shape[2] // 2, kind), g)


def ky(a, u, flipped=False):
    if flipped:
        u = 1 - u
    return 3 - 2 * u if a == 0 else 2 - 2 * u


def convt_phase(g, w, flipped=False):
    """adjoint of Conv2d(Cin, Cout, 4, 2, 1) by output phase: g [N, h, w, Cout], w [Cout, Cin, 4, 4] -> [N, 2h, 2w, Cin]"""
    n, h, wd, _ = g.shape
    gp = F.pad(g, (0, 0, 1, 1, 1, 1))
    out = torch.zeros((n, 2 * h, 2 * wd, w.shape[1]), dtype=torch.float64)
    for a in (0, 1):
        for b in (0, 1):
            acc = 0.0
            for u in (0, 1):
                for v in (0, 1):
                    acc = acc + gp[:, a + u:a + u + h, b + v:b + v + wd] @ w[:, :, ky(a, u, flipped), ky(b, v)]
            out[:, a::2, b::2] = acc
    return out


# ---- network, loss, gradient -----------------------------------------------------------------------------------------------------------
def net64(sd, images, *, n_total=None, emulate=None, fused=(), signs=None, defect=None, gscale=1.0, record=None):
    """sd: the reference's state dict; images NCHW.  signs: {tape name: tensor} whose sign replaces the restatement's own at every LeakyReLU
    (forward and backward).  Returns (logits NCHW, loss, gradient NCHW); record receives the tape and the backward's tensors as NHWC."""
    q = (lambda t: rnd(t, emulate)) if emulate else (lambda t: t)
    Wd, b0, b9 = fold64(sd, defect)
    W = {k: q(w) for k, w in Wd.items()}
    T, G = {}, {}

    def pos(name, z):
        return (signs[name].double().cpu() if signs is not None else z) >= 0

    def lrelu(z, name):
        return torch.where(pos(name, z), z, SLOPE * z)

    kind = "align_corners" if defect == "align_corners" else "bilinear"
    x = q(images.double().permute(0, 2, 3, 1))
    n, h, w, _ = x.shape
    T["x0"] = q(lrelu(q(conv(x, W[0]) + b0), "x0"))
    for k in (1, 2, 3):
        T[f"x{k}"] = q(lrelu(q(conv(T[f"x{k - 1}"], W[k], 2)), f"x{k}"))
    y = T["x3"]
    for k, skip in ((4, "x2"), (5, "x1"), (6, "x0")):
        c = conv(q(up2(y, kind)), W[k])
        if defect == "skip_before_lrelu" and k == 5:
            T[f"s{k}"] = q(c)
            y = q(lrelu(T[f"s{k}"] + T[skip], f"s{k}"))
        elif k in fused:
            T[f"s{k}"] = q(lrelu(c, f"s{k}"))
            y = q(T[f"s{k}"] + T[skip])
        else:
            T[f"s{k}"] = q(c)
            y = q(lrelu(T[f"s{k}"], f"s{k}") + T[skip])
        T[f"x{k}"] = y
    for k in (7, 8):
        c = conv(y, W[k])
        if k in fused:
            y = T[f"s{k}"] = q(lrelu(c, f"s{k}"))
        else:
            T[f"s{k}"] = q(c)
            y = q(lrelu(T[f"s{k}"], f"s{k}"))
    logits = conv(y, W[9]) + b9
    count = float((n if (n_total is None or defect == "mean_n") else n_total) * h * w)
    coef = (1.0 if defect == "sign_missing" else -1.0) * (1.0 if defect == "scale_missing" else LOSS_SCALE) / count
    loss = coef * logits.sum()

    one, slope = torch.tensor(1.0, dtype=torch.float64), torch.tensor(SLOPE, dtype=torch.float64)
    mask = lambda name: torch.where(pos(name, T[name]), one, slope)
    tkind = "nearest" if defect == "nearest_adjoint" else kind
    g = q(torch.full((n, h, w, 1), coef * gscale, dtype=torch.float64))
    G["d_a8"] = q(conv_t3(g, W[9]))
    G["d_a7"] = q(conv_t3(q(G["d_a8"] * mask("s8")), W[8]))
    G["d_x6"] = q(conv_t3(q(G["d_a7"] * (1.0 if defect == "slope1_mask" else mask("s7"))), W[7]))
    G["d_x5"] = q(up2_t(q(conv_t3(q(G["d_x6"] * mask("s6")), W[6])), tkind))
    G["d_x4"] = q(up2_t(q(conv_t3(q(G["d_x5"] * mask("s5")), W[5])), tkind))
    G["d_x3"] = q(up2_t(q(conv_t3(q(G["d_x4"] * mask("s4")), W[4])), tkind))
    G["d_z3"] = q(G["d_x3"] * mask("x3"))
    G["d_z2"] = q((convt_phase(G["d_z3"], W[3], defect == "ky_flipped") + G["d_x4"]) * mask("x2"))
    G["d_z1"] = q((convt_phase(G["d_z2"], W[2]) + (0.0 if defect == "skip_grad_dropped" else G["d_x5"])) * mask("x1"))
    G["d_z0"] = q((convt_phase(G["d_z1"], W[1]) + G["d_x6"]) * mask("x0"))
    grad = conv_t3(G["d_z0"], W[0]) / gscale
    if record is not None:
        record.update(T)
        record.update(G)
    return logits.permute(0, 3, 1, 2), loss, grad.permute(0, 3, 1, 2)


def engine_inputs(shape, seed=7):
    """the images of the engine tests and of the seeded defects: uniform in [0, 1), fp32"""
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed + shape[-1]), dtype=torch.float32)


ENGINE_CASES = ((64, (2, 3, 16, 24)), (64, (1, 3, 8, 40)), (32, (2, 3, 16, 24)), (32, (1, 3, 8, 40)))


# ---- kernels ---------------------------------------------------------------------------------------------------------------------------
def convt_operands(grid, cout, cin, seed, regime, dtype, *, with_r=False, with_y=False):
    """g [images, h, w, cout], w [cout, cin, 4, 4], R / Y [images, 2h, 2w, cin] (or None), float64 rounded to the compute type"""
    images, h, wd = grid
    g = operand((images, h, wd, cout), seed, regime, dtype)
    w = weights((cin, cout, 4, 4), seed + 1, regime, dtype).permute(1, 0, 2, 3).contiguous()     # scaled by the adjoint's reduction, over Cout
    r =operand((images, 2 * h, 2 * wd, cin), seed + 2, regime, dtype) if with_r else None
    y = operand((images, 2 * h, 2 * wd, cin), seed + 3, "mixed", dtype) if with_y else None
    return g, w, r, y


def convt_ref(g, w, r, y, *, slope, dtype, out_f32=False):
    """(D, tol) of one pmi_convt4x4s2 call (module doc)"""
    acc = convt_phase(g, w)
    S = convt_phase(g.abs(), w.abs())
    err = C_B * chain_len(4 * w.shape[0], 1) * E32 * S
    v = acc
    if r is not None:
        v = v + r
        err = err + C_B * E32 * v.abs()
    if y is not None:
        neg = y < 0
        v = torch.where(neg, slope * v, v)
        err = torch.where(neg, abs(slope) * err + E32 * v.abs(), err)
    if not out_f32:
        err = err + out_rounding(v, dtype)
    return v, err


def lrelu_bwd_ref(g, g2, y, slope, dtype):
    """(dz, tol): one fp32 addition, one multiplication, one rounding at the store"""
    v = g if g2 is None else g + g2
    d = torch.where(y >= 0, v, slope * v)
    return d, C_B * 2 * E32 * d.abs() + out_rounding(d, dtype)


def lrelu_add_ref(z, r, slope, dtype):
    a = torch.where(z >= 0, z, slope * z)
    v = a if r is None else a + r
    return v, C_B * E32 * (a.abs() + v.abs()) + out_rounding(v, dtype)


def mean_ref(x, scale):
    """(value, tol): 256 ranges of ceil(n / 256) values summed 256 at a stride, two trees of 8 levels, the scale"""
    n = x.numel()
    per = -(-n // 256)
    depth = -(-per // 256) + 8 + 8 + 1
    return scale * x.double().sum(), C_B * depth * E32 * abs(scale) * x.double().abs().sum()
