"""Float64 restatement of the differentiable JPEG codec (include/perceptor_hip.h: pmi_jpeg_encode / pmi_jpeg_decode / pmi_jpeg_decode_bwd) and
the bound every comparison in tests/test_gpu_drawers.py asserts.  tests/test_drawers_cpu.py holds these restatements to the reference's own
float64 values (tests/golden/drawers_reference.npz) and requires the bounds to reject planted defects.

CPU torch only; no engine import and nothing of the reference.  Every function returns, per output element, the value AND the sum of the
absolute values of the terms that make it up ("absum"), with every constant the kernel adds (the 128 level shift) counted as a term.

The bound is  K * u * absum,  u = 2^-24,  K = 32, from the longest chain of fp32 roundings in csrc/jpeg.hip as written (each rounding moves
a partial result by at most u times its magnitude, and every partial result is bounded by absum):

  decode, per output      table * alpha * alpha * factor (3) and its product with the coefficient (1), the rounded alpha literal (1)   5
                          first 8-term pass: rounded cosine literal (1) + 8 fused multiply-adds (8)                                       9
                          second 8-term pass                                                                                               9
                          * 0.25 exact; + 128                                                                                             1
                          colour row: rounded matrix literals (1) + two fused multiply-adds (2)                                           3
                          clamp exact; / 255                                                                                              1
                                                                                                                              total     28
  adjoint, per output     d_out / 255 (1), colour column: literals (1), product (1), fused multiply-add / two additions (2)             5
                          2 x 2 sum: one addition in the colour stage, one in the first pass                                            2
                          two 8-term passes as above                                                                                    18
                          table * alpha * alpha * factor * 0.25 (3 + literal 1) and the final product (1)                                5
                                                                                                                              total     30
  encode, per output      * 255 (1), colour row: literals (1) + product and two fused multiply-adds (3), - 128 or the pair sum (1)        6
                          vertical pair sum (chroma)                                                                                      1
                          two 8-term passes                                                                                             18
                          alpha * alpha * 0.25 / (table * factor): literal (1), product (1), table * factor (1), division (1), product (1)  5
                                                                                                                              total     30

K = 32 covers all three with the second-order terms.  The cubic rounding multiplies an error e of the quotient by at most
|d/dx (x - r)^3| = 3 (x - r)^2 <= 0.75 on top of e itself (r is constant between half-integers): 1.75 K u absum after rounding.

``defect=`` plants one fault (see DEFECTS); the clean functions are what the kernels are held to.
"""
import math

import numpy as np
import torch

U = 2.0 ** -24
K = 32
F64 = torch.float64

SHAPES = ((1, 16, 16), (2, 16, 32), (2, 32, 16), (3, 32, 48), (1, 16, 80))    # (1, 16, 80): five macroblocks across, one workgroup takes four
FACTORS = (1.0, 2.5)
SIGMA = 0.6                                                                   # coefficient noise of the decode cases

DEFECTS = ("table_not_transposed", "cbcr_swapped", "alpha_missing", "blocks_column_major", "block_transposed", "chroma_wrong_2x2",
           "no_255", "no_factor", "mask_ignored", "half_away")

_LUMA = [[16, 11, 10, 16, 24, 40, 51, 61], [12, 12, 14, 19, 26, 58, 60, 55], [14, 13, 16, 24, 40, 57, 69, 56], [14, 17, 22, 29, 51, 87, 80, 62],
         [18, 22, 37, 56, 68, 109, 103, 77], [24, 35, 55, 64, 81, 104, 113, 92], [49, 64, 78, 87, 103, 121, 120, 101], [72, 92, 95, 98, 112, 100, 103, 99]]
_CHROMA4 = [[17, 18, 24, 47], [18, 21, 26, 66], [24, 26, 56, 99], [47, 66, 99, 99]]

# YCbCr -> RGB rows (R, G, B) over (Y, Cb - 128, Cr - 128) and RGB -> YCbCr rows (Y, Cb - 128, Cr - 128) over (R, G, B): the JFIF numbers
# as the reference holds them, i.e. rounded to fp32 first
_TO_RGB = torch.tensor([[1.0, 0.0, 1.402], [1.0, -0.344136, -0.714136], [1.0, 1.772, 0.0]], dtype=torch.float32).double()
_TO_YCC = torch.tensor([[0.299, 0.587, 0.114], [-0.168736, -0.331264, 0.5], [0.5, -0.418688, -0.081312]], dtype=torch.float32).double()


def tables(defect=None):
    """(luma, chroma) [8, 8] float64: the factor that element [i][j] of a block is multiplied by on decoding"""
    qy = torch.tensor(_LUMA, dtype=F64)
    if defect != "table_not_transposed":
        qy = qy.T.contiguous()
    qc = torch.full((8, 8), 99.0, dtype=F64)
    qc[:4, :4] = torch.tensor(_CHROMA4, dtype=F64).T
    return qy, qc


def _alpha(defect=None):
    a = torch.ones(8, dtype=F64)
    if defect != "alpha_missing":
        a[0] = 1.0 / math.sqrt(2.0)
    return torch.outer(a, a).float().double()          # the reference holds the outer product in fp32


def _basis():
    """D[kx][ky][nx][ny] = cos((2 nx + 1) kx pi / 16) cos((2 ny + 1) ky pi / 16), frequencies first: the reference holds the PRODUCT
    rounded to fp32 (its 8 x 8 x 8 x 8 tensordot operand), so this restatement does too; the kernels' separable fp32 cosines differ from
    it by roundings the bound counts"""
    k = np.arange(8, dtype=np.float64)[:, None]
    n = np.arange(8, dtype=np.float64)[None, :]
    c = np.cos((2 * n + 1) * k * np.pi / 16)
    return torch.from_numpy(np.einsum("xu,yv->xyuv", c, c).astype(np.float32)).double()


def merge(blocks, h, w, defect=None):
    """[N, (h/8)(w/8), 8, 8] -> [N, h, w]"""
    n = blocks.shape[0]
    if defect == "block_transposed":
        blocks = blocks.transpose(2, 3)
    if defect == "blocks_column_major":
        return blocks.reshape(n, w // 8, h // 8, 8, 8).permute(0, 2, 3, 1, 4).reshape(n, h, w)
    return blocks.reshape(n, h // 8, w // 8, 8, 8).permute(0, 1, 3, 2, 4).reshape(n, h, w)


def split(plane, defect=None):
    """[N, h, w] -> [N, (h/8)(w/8), 8, 8]"""
    n, h, w = plane.shape
    b = plane.reshape(n, h // 8, 8, w // 8, 8)
    b = b.permute(0, 3, 1, 2, 4) if defect == "blocks_column_major" else b.permute(0, 1, 3, 2, 4)
    b = b.reshape(n, -1, 8, 8)
    return b.transpose(2, 3) if defect == "block_transposed" else b


def _up2(p, defect=None):
    p = p.repeat_interleave(2, 1).repeat_interleave(2, 2)
    if defect == "chroma_wrong_2x2":          # every pixel takes the chroma sample of the 2 x 2 cell to its right
        p = torch.roll(p, -2, 2)
    return p


def _sum2(p, defect=None):
    """adjoint of _up2: [N, h, w] -> [N, h/2, w/2]"""
    if defect == "chroma_wrong_2x2":
        p = torch.roll(p, 2, 2)
    n, h, w = p.shape
    return p.reshape(n, h // 2, 2, w // 2, 2).sum((2, 4))


def _planes(y, cb, cr, h, w, factor, defect=None):
    """sample planes before the colour matrix and their absums; chroma WITHOUT the +128 (it cancels against the matrix's -128)"""
    qy, qc = tables(defect)
    f = 1.0 if defect == "no_factor" else float(factor)
    a, B = _alpha(defect), _basis()
    if defect == "cbcr_swapped":
        cb, cr = cr, cb
    out = []
    for c, q, hh, ww, lift in ((y, qy, h, w, 128.0), (cb, qc, h // 2, w // 2, 0.0), (cr, qc, h // 2, w // 2, 0.0)):
        s = c.double() * (q * a * f)
        v = 0.25 * torch.einsum("nbxy,xyuv->nbuv", s, B) + lift
        va = 0.25 * torch.einsum("nbxy,xyuv->nbuv", s.abs(), B.abs()) + lift
        out.append((merge(v, hh, ww, defect), merge(va, hh, ww, defect)))
    return out


def decode(y, cb, cr, h, w, factor, defect=None):
    """-> (images [N, 3, h, w] in [0, 1], absum, pre, pre_absum): pre = the value on the 0 .. 255 scale before the clamp.
    Bound of images: K u absum; of pre: K u pre_absum."""
    (Y, Ya), (Cb, Cba), (Cr, Cra) = _planes(y, cb, cr, h, w, factor, defect)
    ycc = torch.stack([Y, _up2(Cb, defect), _up2(Cr, defect)], 1)
    ycca = torch.stack([Ya, _up2(Cba, defect), _up2(Cra, defect)], 1)
    pre = torch.einsum("rk,nkhw->nrhw", _TO_RGB, ycc)
    prea = torch.einsum("rk,nkhw->nrhw", _TO_RGB.abs(), ycca)
    s = 1.0 if defect == "no_255" else 255.0
    return pre.clamp(0.0, 255.0) / s, prea / s, pre, prea


def clamp_margin(pre):
    """distance of every pre-clamp value from the nearer clamp edge"""
    return torch.minimum(pre.abs(), (pre - 255.0).abs())


def decode_adjoint(y, cb, cr, d_out, factor, defect=None):
    """-> ((d_y, d_cb, d_cr), (absums)): the gradient of sum(decode(y, cb, cr) * d_out); passes where 0 < pre < 255"""
    n, _, h, w = d_out.shape
    _, _, pre, _ = decode(y, cb, cr, h, w, factor, None if defect == "mask_ignored" else defect)
    mask = torch.ones_like(pre) if defect == "mask_ignored" else ((pre > 0) & (pre < 255)).double()
    s = 1.0 if defect == "no_255" else 255.0
    g = mask * d_out.double() / s
    gycc = torch.einsum("rk,nrhw->nkhw", _TO_RGB, g)
    gycca = torch.einsum("rk,nrhw->nkhw", _TO_RGB.abs(), g.abs())
    qy, qc = tables(defect)
    f = 1.0 if defect == "no_factor" else float(factor)
    a, B = _alpha(defect), _basis()
    vals, sums = [], []
    for k, q in ((0, qy), (1, qc), (2, qc)):
        p, pa = gycc[:, k], gycca[:, k]
        if k:
            p, pa = _sum2(p, defect), _sum2(pa, defect)
        b, ba = split(p, defect), split(pa, defect)
        scale = 0.25 * q * a * f
        vals.append(torch.einsum("nbuv,xyuv->nbxy", b, B) * scale)
        sums.append(torch.einsum("nbuv,xyuv->nbxy", ba, B.abs()) * scale)
    if defect == "cbcr_swapped":
        vals[1], vals[2], sums[1], sums[2] = vals[2], vals[1], sums[2], sums[1]
    return tuple(vals), tuple(sums)


def diff_round(x, defect=None):
    """round half to even plus the cube of the remainder"""
    r = torch.sign(x) * torch.floor(x.abs() + 0.5) if defect == "half_away" else torch.round(x)
    return r + (x - r) ** 3


def encode(images, factor, rounding=True, defect=None, dct_to_f32=False):
    """-> ((y, cb, cr), (absums of the quotients BEFORE rounding), (the quotients before rounding)).
    dct_to_f32: round the DCT output to fp32 before the division, as the reference's quantisers do whatever the module's dtype
    (``image.float()``, compression.py:132 / :154) -- only for the comparison with the reference's own float64 run; the kernels are held
    to the unrounded value (the two differ by less than u |DCT|, one more rounding of the chain)."""
    s = 1.0 if defect == "no_255" else 255.0
    x = images.double() * s
    ycc = torch.einsum("kr,nrhw->nkhw", _TO_YCC, x)
    ycca = torch.einsum("kr,nrhw->nkhw", _TO_YCC.abs(), x.abs())
    qy, qc = tables(defect)
    f = 1.0 if defect == "no_factor" else float(factor)
    a, B = _alpha(defect), _basis()
    vals, sums = [], []
    for k, q in ((0, qy), (1, qc), (2, qc)):
        p, pa = ycc[:, k], ycca[:, k]
        if k:
            p, pa = _sum2(p, defect) / 4, _sum2(pa, defect) / 4           # the +128 of the chroma and the DCT's -128 cancel
        else:
            p, pa = p - 128.0, pa + 128.0
        b, ba = split(p, defect), split(pa, defect)
        d = torch.einsum("nbuv,xyuv->nbxy", b, B) * (0.25 * a)
        if dct_to_f32:
            d = d.float().double()
        vals.append(d / (q * f))
        sums.append(torch.einsum("nbuv,xyuv->nbxy", ba, B.abs()) * (0.25 * a) / (q * f))
    if defect == "cbcr_swapped":
        vals[1], vals[2], sums[1], sums[2] = vals[2], vals[1], sums[2], sums[1]
    out = tuple(diff_round(v, defect) for v in vals) if rounding else tuple(vals)
    return out, tuple(sums), tuple(vals)


def half_margin(q):
    """distance of every quotient from the nearest half-integer"""
    return ((q - torch.floor(q)) - 0.5).abs()


def tol(absum, k=1.0):
    return k * K * U * absum


def within(got, ref, bound):
    d = (got.double() - ref.double()).abs()
    return bool((d <= bound).all())


def worst(got, ref, bound):
    """max |got - ref| / bound: the figure the tests print before they assert (inf for a non-finite difference)"""
    d = (got.double() - ref.double()).abs()
    if not bool(torch.isfinite(d).all()):
        return float("inf")
    r = torch.where(d == 0, torch.zeros_like(d), d / bound.clamp_min(1e-300))
    return float(r.max())


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------------
# (image seed, noise seed) per case, searched when this file was written (the loop is in the docstring of `case_margins`): the image seed
# keeps every unrounded quotient of encode() at least 1e-4 from a half-integer, the noise seed every pre-clamp value of decode() well away
# from 0 and 255.  The tests assert both preconditions on the float64 values before they look at a kernel's output.
SEEDS = {((1, 16, 16), 1.0): (119, 18), ((1, 16, 16), 2.5): (140, 11), ((2, 16, 32), 1.0): (20, 35), ((2, 16, 32), 2.5): (198, 1),
         ((2, 32, 16), 1.0): (127, 39), ((2, 32, 16), 2.5): (130, 16), ((3, 32, 48), 1.0): (167, 33), ((3, 32, 48), 2.5): (127, 22),
         ((1, 16, 80), 1.0): (49, 14), ((1, 16, 80), 2.5): (71, 10)}


def image(shape, factor):
    """white-noise fp32 image [N, 3, H, W] in [0, 1)"""
    n, h, w = shape
    return torch.rand((n, 3, h, w), generator=torch.Generator().manual_seed(SEEDS[shape, factor][0]), dtype=torch.float32)


def noisy_coefficients(shape, factor, noise_seed=None):
    """fp32 coefficients of the decode cases: the rounded encoding of image(shape, factor) plus SIGMA-Gaussian noise"""
    (y, cb, cr), _, _ = encode(image(shape, factor), factor)
    g = torch.Generator().manual_seed(SEEDS[shape, factor][1] if noise_seed is None else noise_seed)
    return tuple((c + SIGMA * torch.randn(c.shape, generator=g, dtype=F64)).float() for c in (y, cb, cr))


def weights(shape):
    n, h, w = shape
    return torch.randn((n, 3, h, w), generator=torch.Generator().manual_seed(2000 + h * w), dtype=torch.float32)


def case_margins(shape, factor, noise_seed=None):
    """(min over quotients of half_margin / bound, min half_margin, min over pixels of clamp_margin / bound, min clamp_margin)

    The search that filled SEEDS: for image seeds 0 .. 199 keep those with min half_margin >= 1e-4 and take the largest first ratio; then
    for noise seeds 0 .. 39 take the largest third."""
    _, sums, q = encode(image(shape, factor), factor)
    c = noisy_coefficients(shape, factor, noise_seed)
    _, _, pre, prea = decode(*c, shape[1], shape[2], factor)
    return (min(float((half_margin(x) / tol(a)).min()) for x, a in zip(q, sums)), min(float(half_margin(x).min()) for x in q),
            float((clamp_margin(pre) / tol(prea)).min()), float(clamp_margin(pre).min()))


# ---- the reference's decoder as its sequence of stock torch ops, any dtype / device (tools/jpeg_probe.py times it) ----------------------
class TorchDecoder:
    """dequantise, alpha, 64 x 64 tensordot + 128, merge, repeat chroma, cat, shift + colour tensordot, permute, two-sided clamp, / 255"""

    def __init__(self, h, w, factor, device="cpu", dtype=torch.float32):
        qy, qc = tables()
        B = _basis()
        self.h, self.w = h, w
        self.qy, self.qc = (qy * factor).to(device, dtype), (qc * factor).to(device, dtype)
        self.alpha = _alpha().to(device, dtype)
        self.basis4 = B.to(device, dtype)
        self.matrix = _TO_RGB.T.contiguous().to(device, dtype)
        self.shift = torch.tensor([0.0, -128.0, -128.0]).to(device, dtype)

    def _plane(self, c, q, h, w):
        v = 0.25 * torch.tensordot(c * q * self.alpha, self.basis4, dims=2) + 128
        n = v.shape[0]
        return v.view(n, h // 8, w // 8, 8, 8).permute(0, 1, 3, 2, 4).contiguous().view(n, h, w)

    @staticmethod
    def _repeat(p):
        n, h, w = p.shape
        return p[:, :, None, :, None].repeat(1, 1, 2, 1, 2).reshape(n, h * 2, w * 2)

    def __call__(self, y, cb, cr):
        h, w = self.h, self.w
        Y = self._plane(y, self.qy, h, w)
        Cb, Cr = self._repeat(self._plane(cb, self.qc, h // 2, w // 2)), self._repeat(self._plane(cr, self.qc, h // 2, w // 2))
        img = torch.cat([Y.unsqueeze(3), Cb.unsqueeze(3), Cr.unsqueeze(3)], dim=3)
        img = torch.tensordot(img + self.shift, self.matrix, dims=1).permute(0, 3, 1, 2)
        img = torch.min(255 * torch.ones_like(img), torch.max(torch.zeros_like(img), img))
        return img / 255
