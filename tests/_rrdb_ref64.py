"""float64 restatement of the Real-ESRGAN RRDBNet path (engine/rrdb.py, models / transforms / losses.SuperResolution), the seeded inputs and
the per-element bound of pmi_rdb_conv3x3 (csrc/rrdb.hip).  Conventions of _routes16_ref64.py, whose operand regimes, conv64, chain_len and
out_rounding are used as they are.

Network (own words; checked against the reference's values in tests/golden/super_resolution_reference.npz by
tests/test_super_resolution_cpu.py).  All convolutions 3x3, pad 1, with bias; lrelu = LeakyReLU(0.2):
  scale 2: images are reflect-padded on the right / bottom to even H, W, then pixel-unshuffled by 2 (channel c * 4 + 2 dh + dw)
  feat = conv_first(x)
  RDB(x):  x1 = lrelu(conv1(x)), x2 = lrelu(conv2(x | x1)), x3 = lrelu(conv3(x | x1 | x2)), x4 = lrelu(conv4(x | x1 | x2 | x3)),
           0.2 conv5(x | x1 | x2 | x3 | x4) + x
  RRDB(x): 0.2 RDB3(RDB2(RDB1(x))) + x
  y = feat + conv_body(RRDB_B(... RRDB_1(feat))); per up-sampling step y = lrelu(conv_up(nearest x2 (y))); out = conv_last(lrelu(conv_hr(y)))
  scale 2: the rows / columns that came from the pad are cropped from the bottom / right of the output.
emulate = "f16" | "bf16" rounds exactly where the engine stores 16 bit: the staged input, the weights, conv_first's output, x1 .. x4, each
RDB's output (the third RDB's after BOTH residuals: pmi_rdb_conv3x3 adds R1 and R2 in fp32 and rounds once), conv_body + skip, each
up-sampling step and conv_hr.  conv_last writes fp32.  ROUNDINGS counts them along the longest path to a checkpoint.

Bound of one pmi_rdb_conv3x3 call, per element (u = 2^-11 f16, 2^-8 bf16; S = sum |x| |w| + |bias|; z = conv + bias, a = lrelu_slope(z),
v = alpha a + R1, y = beta v + R2):
  accumulation   C_B (chain_len(9 Cin, 1) + N_EPI) E32 S, N_EPI = 6: the epilogue's fp32 operations + bias, * slope, * alpha, + R1, * beta, + R2
  LeakyReLU      E32 |z| for the multiplication by the slope (none at slope 1), Lipschitz constant max(1, |slope|) on the accumulation term
  residual adds  C_B E32 |v| where R1 is present, C_B E32 |y| where R2 is: one fp32 addition each, of values S does not bound; scaled by
                 |alpha|, |beta| like the values they act on
  output         u |y| + SUB where an f16 result may be subnormal: the kernel rounds ONCE, at the store (rrdb.hip: pack4<T> from fp32)
No constant is fitted to a measurement.
"""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from _routes16_ref64 import C_B, E32, TD, U, chain_len, conv64, operand, out_rounding, rnd, weights  # noqa: F401

N_EPI = 6
SLOPE = 0.2
NUM_FEAT, NUM_GROW = 64, 32
DEFECTS = ("lrelu_dropped", "lrelu_on_conv5", "scale_on_x", "rrdb_scale_missing", "r1_r2_swapped", "slices_order", "unshuffle_order",
           "replicate_pad", "crop_wrong_side", "up_shift")


def lrelu(z, slope=SLOPE):
    return torch.where(z >= 0, z, slope * z)


# ---- one kernel call ------------------------------------------------------------------------------------------------------------------
def kernel_ref(x, w, bias, *, dtype, slope=1.0, alpha=1.0, beta=1.0, r1=None, r2=None, up=False):
    """x [N, Hin, Win, Cin], w [Cout, Cin, 3, 3], bias [Cout], r1 / r2 at the output grid, all float64 (x, w, r1, r2 already rounded to the
    compute type).  Returns (y, tol)."""
    K = 9 * w.shape[1]
    z = conv64(x, w, up=up) + bias
    S = conv64(x.abs(), w.abs(), up=up) + bias.abs()
    z_err = C_B * (chain_len(K, 1) + N_EPI) * E32 * S
    a = lrelu(z, slope)
    a_err = max(1.0, abs(slope)) * z_err + (E32 * z.abs() if slope != 1.0 else 0.0)
    v = alpha * a
    v_err = abs(alpha) * a_err
    if r1 is not None:
        v = v + r1
        v_err = v_err + C_B * E32 * v.abs()
    y = beta * v
    y_err = abs(beta) * v_err
    if r2 is not None:
        y = y + r2
        y_err = y_err + C_B * E32 * y.abs()
    return y, y_err + out_rounding(y, dtype)


def kernel_operands(grid, cin, n, seed, regime, dtype, *, up=False, residuals=0):
    """Seeded operands of one call: x [images, Hin, Win, cin], w [n, cin, 3, 3], bias [n], r1, r2 (None beyond ``residuals``)."""
    images, h, wd = grid
    hin, win = (h // 2, wd // 2) if up else (h, wd)
    x = operand((images, hin, win, cin), seed, regime, dtype)
    w = weights((n, cin, 3, 3), seed + 1, regime, dtype)
    bias = operand((n,), seed + 2, regime, "bf16").float().double()
    r = [operand((images, h, wd, n), seed + 3 + i, regime, dtype) for i in range(residuals)] + [None, None]
    return x, w, bias, r[0], r[1]


# ---- network -----------------------------------------------------------------------------------------------------------------------------
def unshuffle2(x, swapped=False):
    b, c, hh, hw = x.shape
    v = x.reshape(b, c, hh // 2, 2, hw // 2, 2)
    return v.permute(0, 1, 5, 3, 2, 4).reshape(b, c * 4, hh // 2, hw // 2) if swapped else v.permute(0, 1, 3, 5, 2, 4).reshape(b, c * 4, hh // 2, hw // 2)


def _up2(y, shift=False):
    """nearest x2 of NHWC: output (r, c) reads (r >> 1, c >> 1); shift: ((r + 1) >> 1, (c + 1) >> 1), clamped"""
    n, h, w, c = y.shape
    ri, ci = torch.arange(2 * h), torch.arange(2 * w)
    ri, ci = ((ri + 1) // 2).clamp(max=h - 1) if shift else ri // 2, ((ci + 1) // 2).clamp(max=w - 1) if shift else ci // 2
    return y[:, ri][:, :, ci]


def roundings(scale, blocks):
    """16-bit roundings along the longest path to each checkpoint (module doc)"""
    R = {"conv_first": 2}
    for i in range(blocks):
        R[f"rrdb{i}"] = 2 + 15 * (i + 1)
    k = R["conv_body"] = 2 + 15 * blocks + 1
    for j in range(3 if scale == 8 else 2):
        k = R[f"up{j + 1}"] = k + 1
    R["hr"] = R["out"] = k + 1
    return R


def network64(sd, x, scale, blocks, *, emulate=None, defect=None, record=None):
    """sd: float64 state dict (reference keys), x NCHW float64 with H, W the unshuffle divides -> NCHW float64.  record: dict receiving the
    checkpoints of engine/rrdb.py as NHWC float64."""
    q = (lambda t: rnd(t, emulate)) if emulate else (lambda t: t)
    W = lambda name: (q(sd[f"{name}.weight"].double()), sd[f"{name}.bias"].double())
    conv = lambda t, name: conv64(t, W(name)[0]) + W(name)[1]
    keep = (lambda k, t: record.__setitem__(k, t)) if record is not None else (lambda k, t: None)
    if scale == 2:
        x = unshuffle2(x, swapped=defect == "unshuffle_order")
    h = q(x.double().permute(0, 2, 3, 1))
    feat = q(conv(h, "conv_first"))
    keep("conv_first", feat)
    x = feat
    for i in range(blocks):
        x_rrdb = x
        for r in (1, 2, 3):
            xs = [x]
            for k in (1, 2, 3, 4):
                src = xs if not (defect == "slices_order" and k >= 3) else [xs[0]] + xs[1:][::-1]
                z = conv(torch.cat(src, -1), f"body.{i}.rdb{r}.conv{k}")
                xs.append(q(z if defect == "lrelu_dropped" else lrelu(z)))
            src = xs if defect != "slices_order" else [xs[0]] + xs[1:][::-1]
            x5 = conv(torch.cat(src, -1), f"body.{i}.rdb{r}.conv5")
            if defect == "lrelu_on_conv5":
                x5 = lrelu(x5)
            out = 0.2 * x + x5 if defect == "scale_on_x" else 0.2 * x5 + x
            if r == 3:
                if defect == "rrdb_scale_missing":
                    out = out + x_rrdb
                elif defect == "r1_r2_swapped":
                    out = 0.2 * (0.2 * x5 + x_rrdb) + x
                else:
                    out = 0.2 * out + x_rrdb
            x = q(out)
        keep(f"rrdb{i}", x)
    y = q(conv(x, "conv_body") + feat)
    keep("conv_body", y)
    for j in range(3 if scale == 8 else 2):
        y = q(lrelu(conv(_up2(y, shift=defect == "up_shift"), f"conv_up{j + 1}")))
        keep(f"up{j + 1}", y)
    y = q(lrelu(conv(y, "conv_hr")))
    keep("hr", y)
    return conv(y, "conv_last").permute(0, 3, 1, 2)


def upsample64(sd, images, scale, blocks, *, emulate=None, defect=None, record=None):
    """RealESRGANer.enhance for tile = 0, pre_pad = 0, restated"""
    x = images.double()
    ph = pw = 0
    if scale == 2:
        ph, pw = x.shape[2] % 2, x.shape[3] % 2
        if ph or pw:
            x = F.pad(x, (0, pw, 0, ph), "replicate" if defect == "replicate_pad" else "reflect")
    out = network64(sd, x, scale, blocks, emulate=emulate, defect=defect, record=record)
    H, Wd = out.shape[2], out.shape[3]
    if defect == "crop_wrong_side":
        return out[:, :, ph * scale:, pw * scale:]
    return out[:, :, :H - ph * scale, :Wd - pw * scale]


# ---- resize (transforms/resize.py's tables in float64) and the loss ----------------------------------------------------------------------------------
def band64(in_sz, out_sz, method):
    """The band of transforms.resize.band_tables as a dense float64 matrix [out, in] (same steps, float64 grid)"""
    from perceptor_amd.transforms.resize import _EPS, _METHODS
    fn, support = _METHODS[method]
    scale = out_sz / in_sz
    grid = torch.arange(out_sz, dtype=torch.float64) / scale + (in_sz - 1) / 2 - (out_sz - 1) / (2 * scale)
    if scale < 1.0:
        cur, f = support / scale, (lambda a: scale * fn(scale * a))
    else:
        cur, f = support, fn
    left = (grid - cur / 2 - _EPS).ceil().long()
    fov = left[:, None] + torch.arange(math.ceil(cur - _EPS))
    pad0 = -int(fov[0, 0])
    w = f((grid + pad0)[:, None] - (fov + pad0).double())
    s = w.sum(1, keepdim=True)
    s[s == 0] = 1
    w = w / s
    M = torch.zeros(out_sz, in_sz, dtype=torch.float64)
    for t in range(fov.shape[1]):
        ok = (fov[:, t] >= 0) & (fov[:, t] < in_sz)
        rows = torch.nonzero(ok)[:, 0]
        M[rows, fov[rows, t]] += w[rows, t]
    return M


def resize64(x, out_hw, method):
    """transforms.resize(x, out_hw, resample=method) in float64 (method "cubic" | "lanczos3"): the axis with the smaller scale first"""
    dims = sorted([(out_hw[0] / x.shape[2], 2, x.shape[2], out_hw[0]), (out_hw[1] / x.shape[3], 3, x.shape[3], out_hw[1])], key=lambda z: z[0])
    x = x.double()
    for s, axis, i, o in dims:
        if s == 1.0:
            continue
        M = band64(i, o, method)
        x = torch.einsum("oi,nciw->ncow", M, x) if axis == 2 else torch.einsum("oi,nchi->ncho", M, x)
    return x


def loss64(sd, images, blocks, *, scale=2, pre_downscale=None, method="cubic", emulate=None):
    """losses.SuperResolution restated: (loss, gradient, down-sized images, up-sampled images before the resize back)"""
    x = images.double()
    p = scale if pre_downscale is None else pre_downscale
    h, w = x.shape[2:]
    down = resize64(x, (h // p, w // p), method)
    raw = up = upsample64(sd, down, scale, blocks, emulate=emulate)
    if tuple(up.shape[2:]) != (h, w):
        up = resize64(up, (h, w), method)
    d = x - up
    return d.square().mean(), 2 * d / d.numel(), down, raw


def rel_l2(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())
