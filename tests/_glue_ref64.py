"""Float64 / CPU restatements of the staging, token, layout and sampler glue kernels (include/perceptor_hip.h), one plain function
per operation, and the bound every comparison in tests/test_gpu_glue_kernels.py asserts.  tests/test_glue_bounds_cpu.py seeds defects
into these restatements and requires the same bound functions to reject them.

No engine import and nothing of the reference: numpy and CPU torch only.  u = 2^-24 is the fp32 unit roundoff.
"""
import numpy as np
import torch

U = 2.0 ** -24
NAN16 = {"f16": 0x7E00, "bf16": 0x7FC0}
TORCH16 = {"f16": torch.float16, "bf16": torch.bfloat16}
DT_CODE = {"f16": 0, "bf16": 1}
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def rng(seed):
    return torch.Generator().manual_seed(seed)


def same(a, b):
    """elementwise equality in which NaN equals NaN (and -0 equals +0, as torch.equal has it)"""
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def within(got, ref, tol):
    """every |got - ref| <= tol; a non-finite difference never passes"""
    d = (got.double() - ref.double()).abs()
    return bool((d <= tol).all())


def worst(got, ref, tol):
    """max |got - ref| / tol (inf when a difference is not finite): the figure the tests print before they assert"""
    d = (got.double() - ref.double()).abs()
    r = d / tol.clamp_min(1e-300) if torch.is_tensor(tol) else d / max(tol, 1e-300)
    r = torch.where(d == 0, torch.zeros_like(r), r)
    return float("inf") if not bool(torch.isfinite(r).all()) else float(r.max())


# ---- banded operator (pmi_resize_apply) -------------------------------------------------------------------------------------------
def dense_band(idx, w, in_sz):
    """idx / w [out_sz][taps] -> the dense operator A [out_sz][in_sz] in float64 and sum_t |w| scattered alike; idx < 0 skipped"""
    idx, w = idx.long(), w.double()
    out_sz, taps = idx.shape
    A = torch.zeros(out_sz, in_sz, dtype=torch.float64)
    Aabs = torch.zeros_like(A)
    for j in range(out_sz):
        for t in range(taps):
            r = int(idx[j, t])
            if r >= 0:
                A[j, r] += w[j, t]
                Aabs[j, r] += w[j, t].abs()
    return A, Aabs


def band_apply(x, idx, w, drop_border_tap=False):
    """out[o][j][i] = sum_t w[j][t] * x[o][idx[j][t]][i] for x [outer][in_sz][inner]; returns (out, sum_t |w x|) in float64.
    drop_border_tap: the defect of a kernel that loses the last valid tap of every row that has a skipped (border) entry."""
    idx = idx.clone()
    if drop_border_tap:
        for j in range(idx.shape[0]):
            valid = (idx[j] >= 0).nonzero().flatten()
            if len(valid) and len(valid) < idx.shape[1]:
                idx[j, valid[-1]] = -1
    A, Aabs = dense_band(idx, w, x.shape[1])
    x = x.double()
    return torch.einsum("jr,ori->oji", A, x), torch.einsum("jr,ori->oji", Aabs, x.abs())


def band_tol(absum, taps):
    """taps products and taps - 1 additions in fp32, in any order and with or without FMA contraction: every partial sum is below
    sum_t |w x|, so the error is at most (taps + 1) u sum_t |w x| to first order"""
    return (taps + 1) * U * absum


def adjoint_tol(x, y, Aabs, taps):
    """<A x, y> against <x, A^T y> in float64 from two fp32 results: each side carries at most (taps + 1) u and the float64 dot
    nothing visible -- 4 taps u sum |y| |A| |x| covers both sides for taps >= 1"""
    return 4 * taps * U * float(torch.einsum("oji,jr,ori->", y.double().abs(), Aabs, x.double().abs()))


# ---- patchify / unpatchify --------------------------------------------------------------------------------------------------------
def patchify64(img, mean, std, P, Kp, swap_pypx=False):
    """img [N][3][R][R] -> col [N g g][Kp] float64, k = c P^2 + py P + px, m = n g^2 + gy g + gx, (x - mean[c]) / std[c]; columns
    3 P^2 .. Kp are zero.  swap_pypx: the defect k = c P^2 + px P + py."""
    N, _, R, _ = img.shape
    g = R // P
    v = (img.double() - mean.double()[None, :, None, None]) / std.double()[None, :, None, None]
    v = v.reshape(N, 3, g, P, g, P)                                   # n c gy py gx px
    v = v.permute(0, 2, 4, 1, 5, 3) if swap_pypx else v.permute(0, 2, 4, 1, 3, 5)
    col = torch.zeros(N * g * g, Kp, dtype=torch.float64)
    col[:, :3 * P * P] = v.reshape(N * g * g, 3 * P * P)
    return col


def unpatchify64(dcol, std, N, R, P, mul, std0_everywhere=False):
    """dcol [N g g][Kp] -> dimg [N][3][R][R] = dcol[m][c P^2 + py P + px] / std[c] * mul (the pad columns are never read).
    std0_everywhere: the defect of dividing every channel by std[0]."""
    g = R // P
    s = std.double()
    if std0_everywhere:
        s = s[:1].expand(3)
    v = dcol.double()[:, :3 * P * P].reshape(N, g, g, 3, P, P).permute(0, 3, 1, 4, 2, 5).reshape(N, 3, R, R)
    return v / s[None, :, None, None] * mul


def ulp16(v, dtype):
    """spacing of the 16-bit format at |v| (float64 tensor): 2^(e - 10) for f16 with e >= -14, 2^(e - 7) for bf16 with e >= -126"""
    mant, emin = (10, -14) if dtype == "f16" else (7, -126)
    e = torch.floor(torch.log2(v.abs().clamp_min(2.0 ** (emin - 1)))).clamp_min(emin)
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - mant)


def patchify_tol(ref, dtype):
    """(x - mean) / std is two fp32 roundings (2 u |ref|; 4 u asked) and one rounding to 16 bits: half an ulp16 of the fp32 value, which can
    sit one binade above ref64's only by the relative 2^-10 the factor allows"""
    return 0.5 * ulp16(ref, dtype) * (1 + 2.0 ** -10) + 4 * U * ref.abs()


def unpatchify_tol(ref):
    """a division and a multiplication in fp32: 2 u |ref| to first order, 3 u asked"""
    return 3 * U * ref.abs()


# ---- token assembly, fp32 (one addition: exact against the CPU) -------------------------------------------------------------------
def vit_assemble32(emb, cls, pos):
    """x[n][0] = cls + pos[0], x[n][1 + p] = emb[n][p] + pos[1 + p]"""
    N = emb.shape[0]
    return torch.cat([cls[None, None, :].expand(N, 1, -1), emb], 1) + pos[None]


def embed_tokens32(ids, tok, pos):
    """x[n][t] = tok[clamp(ids[n][t], 0, vocab - 1)] + pos[t] (pos may be None)"""
    x = tok[ids.clamp(0, tok.shape[0] - 1)]
    return x + pos[None] if pos is not None else x


def gather_rows32(src, idx, D):
    """dst[r] = src[clamp(idx[r], 0, rows - 1)][:D] for src rows of pitch ld >= D"""
    return src[idx.clamp(0, src.shape[0] - 1), :D].contiguous()


# ---- casts ------------------------------------------------------------------------------------------------------------------------
def cast16_bits(x, dtype, truncate=False):
    """int16 bit patterns of x (fp32) in the 16-bit format, round to nearest even; truncate: the defect of chopping toward zero"""
    if not truncate:
        return x.to(TORCH16[dtype]).view(torch.int16)
    if dtype == "bf16":
        return (x.view(torch.int32) >> 16).to(torch.int16)
    h = x.to(torch.float16)
    over = h.float().abs() > x.abs()                                  # rounded away from zero: step the magnitude back by one
    return torch.where(over, h.view(torch.int16) - 1, h.view(torch.int16))


def cast_specials(dtype):
    """fp32 inputs for the rounding edges of the 16-bit format: midpoints between neighbours on the even-below and the even-above side (normal
    and, for f16, subnormal), +-0, f16 subnormals, 65504 / 65520 / 1e6, +-inf and NaN"""
    t16 = TORCH16[dtype]
    lo_bits = []
    for base in ((0x3C00, 0x3C01, 0x4BFE, 0x4BFF, 0x0400, 0x0001, 0x0002, 0x03FE, 0x03FF, 0x7BFE) if dtype == "f16" else
                 (0x3F80, 0x3F81, 0x42FE, 0x42FF, 0x0080, 0x3EFF, 0x7F7E)):
        lo_bits += [base, base | 0x8000 if base < 0x8000 else base]
    a = torch.tensor(lo_bits, dtype=torch.int32).to(torch.int16).view(t16).double()
    b = (torch.tensor(lo_bits, dtype=torch.int32) + 1).to(torch.int16).view(t16).double()
    mid = ((a + b) / 2).float()                                        # exact in fp32: one more mantissa bit than the 16-bit format
    assert bool((mid.double() == (a + b) / 2).all())
    sub = torch.tensor([2.0 ** -24, -2.0 ** -24, 3 * 2.0 ** -24, 1023 * 2.0 ** -24, 2.0 ** -14, 2.0 ** -25, 1.5 * 2.0 ** -25, 2.0 ** -26])
    edge = torch.tensor([0.0, -0.0, 65504.0, 65519.996, 65520.0, -65520.0, 1e6, -1e6, float("inf"), -float("inf"), float("nan")])
    return torch.cat([mid, sub.float(), edge])


def split_layout(hi, lo):
    """logical [rows][C] high and low halves -> the precise layout [rows][C / G][hi G | lo G], G = min(C, 32)"""
    rows, C = hi.shape
    G = min(C, 32)
    return torch.stack([hi.reshape(rows, C // G, G), lo.reshape(rows, C // G, G)], 2).reshape(rows, 2 * C)


def split_to_plain_bits(hi, lo):
    """hi + lo in float64, rounded once to f16 (int16 patterns)"""
    return torch.from_numpy((hi.double().numpy() + lo.double().numpy()).astype(np.float16)).view(torch.int16)


# ---- sampler algebra --------------------------------------------------------------------------------------------------------------
def lincomb64(a, b, ca, cb, cc, chw, bad_sample_index=False):
    """out = ca[n] a + cb[n] b + cc[n] over flat a / b [N chw], n = i // chw; returns (out, |ca a| + |cb b| + |cc|) in float64.
    bad_sample_index: the defect n = i // (chw + 1)."""
    i = torch.arange(a.numel())
    n = i // (chw + 1) if bad_sample_index else i // chw
    out = ca.double()[n] * a.double()
    mag = out.abs()
    if b is not None:
        t = cb.double()[n] * b.double()
        out, mag = out + t, mag + t.abs()
    if cc is not None:
        out, mag = out + cc.double()[n], mag + cc.double()[n].abs()
    return out, mag


def lincomb_tol(mag):
    """two products and two additions in fp32, with or without FMA contraction: every partial result is below |ca a| + |cb b| + |cc|
    and each of the at most three roundings on a path is relative u"""
    return 3 * U * mag


def clamp32(x, lo, hi):
    """Tensor.clamp with per-sample bounds on x [N][chw] (fp32, the reference's own expression: NaN propagates)"""
    return x.clamp(lo[:, None], hi[:, None])


def clamp_grad32(x, grad, lo, hi):
    """backward of clamp_with_grad: grad * (grad * (x - x.clamp(lo, hi)) >= 0)"""
    return grad * (grad * (x - x.clamp(lo[:, None], hi[:, None])) >= 0)


def clamp_inputs(N, chw, seed):
    """x, grad [N][chw] with values on each sample's bounds, +-0, +-inf and NaN planted, and per-sample bounds that all differ"""
    g = rng(seed)
    lo = torch.tensor([-0.75, -1.5, 0.0])[:N].clone()
    hi = torch.tensor([0.5, 2.25, 1.0])[:N].clone()
    x = torch.randn(N, chw, generator=g) * 2
    grad = torch.randn(N, chw, generator=g)
    special = [float("nan"), float("inf"), -float("inf"), 0.0, -0.0]
    if chw == 1:
        x[:, 0] = torch.tensor([float("nan"), float(hi[1]), -float("inf")])[:N]
    for n in range(N if chw > 1 else 0):
        for k, v in enumerate(special + [float(lo[n]), float(hi[n])]):
            if chw > k:
                x[n, (k * 7 + n) % chw] = v
    if chw > 16:
        for n in range(N):
            grad[n, (3 + n) % chw] = float("nan")
            grad[n, (11 + n) % chw] = float("inf")
            grad[n, (12 + n) % chw] = 0.0
            grad[n, (13 + n) % chw] = -0.0
            x[n, (11 + n) % chw] = 0.25          # inside every interval: x - clamp(x) = 0 and inf * 0 = NaN fails the mask
    return x, grad, lo, hi


# ---- quantile ---------------------------------------------------------------------------------------------------------------------
def quantile_parts(x, q, ceil_for_lower=False):
    """per row of |x| [N][n]: the order statistics a = s[floor(r)], b = s[ceil(r)] at the fp32 rank r = fp32(q) * fp32(n - 1), the
    weight w = r - floor(r) (exact in fp32) and a + w (b - a) in float64.  ceil_for_lower: the defect a = s[ceil(r)]."""
    n = x.shape[1]
    s = x.abs().sort(1)[0]
    r = float(np.float32(q) * np.float32(n - 1))
    k_lo, k_hi = int(np.floor(r)), int(np.ceil(r))
    w = r - np.floor(r)
    a, b = s[:, k_hi if ceil_for_lower else k_lo], s[:, k_hi]
    return a, b, w, a.double() + w * (b.double() - a.double())


def quantile_tol(a, b):
    """at::lerp in fp32 is one subtraction, one product and one addition on values of magnitude at most max(|a|, |b|): 2 u max(|a|, |b|)"""
    return 2 * U * torch.maximum(a.abs(), b.abs()).double()


def quantile_ok(got, a, b, w, ref):
    """order statistics exact where they are returned as they are (w = 0 or a = b), the lerp within quantile_tol elsewhere; rows whose
    float64 value is not finite follow the fp32 at::lerp expression (torch.lerp on the CPU)"""
    for n in range(len(got)):
        if w == 0 or float(a[n]) == float(b[n]):
            ok = same(got[n].view(1), a[n].view(1))
        elif not bool(torch.isfinite(ref[n])):
            ok = same(got[n].view(1), torch.lerp(a[n], b[n], float(np.float32(w))).view(1))
        else:
            ok = within(got[n], ref[n], quantile_tol(a[n], b[n]))
        if not ok:
            return False
    return True


def quantile_rows(n, seed):
    """three rows with different distributions: N(0, 1) with -0.0 and subnormals, a wide log-uniform row with +inf, an all-equal row"""
    g = rng(seed)
    x = torch.empty(3, n)
    x[0] = torch.randn(n, generator=g)
    x[1] = torch.exp(torch.rand(n, generator=g) * 20 - 10) * torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0)
    x[2] = -0.37
    x[0, 0] = -0.0
    if n > 2:
        x[0, 1] = 1e-40          # subnormals only where an order statistic is returned as it is (q = 0, 1 / (n - 1); n = 3: q = 0.5):
    if n > 3:                    # the lerp bound 2 u max(|a|, |b|) has no underflow term
        x[0, 2] = -3e-42
    x[1, n // 2] = float("inf")
    return x


# ---- sort / Wasserstein -----------------------------------------------------------------------------------------------------------
def sort_rows_input(n, seed):
    """three rows: heavy ties with +-0, +-inf and subnormals; N(0, 1); a descending ramp"""
    g = rng(seed)
    x = torch.empty(3, n)
    x[0] = torch.randint(-3, 4, (n,), generator=g).float()
    pool = [0.0, -0.0, float("inf"), -float("inf"), 1e-40, -1e-40, 1.4e-45, -0.0, 0.0]
    for k, v in enumerate(pool[:n]):
        x[0, (k * 5) % n] = v
    x[1] = torch.randn(n, generator=g)
    x[2] = torch.arange(n, 0, -1).float()
    return x


def wasserstein64(sorted_rows, power, unit_linspace=False):
    """mean over rows and columns of |sorted - Normal(0, 1).icdf(linspace(0.5 / n, 1 - 0.5 / n, n))|^power in float64.
    unit_linspace: the defect linspace(0, 1, n)."""
    n = sorted_rows.shape[1]
    p = torch.linspace(0.0, 1.0, n, dtype=torch.float64) if unit_linspace else \
        torch.linspace(0.5 / n, 1 - 0.5 / n, n, dtype=torch.float64)
    expect = torch.special.erfinv(2 * p - 1) * np.sqrt(2.0)
    d = (sorted_rows.double() - expect[None]).abs()
    return (d if power == 1 else d * d).mean()


def wasserstein_ref32(sorted_rows, power):
    """the reference's own fp32 expression (guided_diffusion/predictions.py:184-198) on the CPU"""
    n = sorted_rows.shape[1]
    margin = 0.5 / n
    points = torch.linspace(margin, 1 - margin, n)
    expected = torch.distributions.Normal(0, 1).icdf(points)
    d = sorted_rows - expected[None].to(sorted_rows)
    return d.abs().mean() if power == 1 else d.square().mean()


def wasserstein_tol(sorted_rows, power):
    """four times the error of the reference's fp32 expression against float64 at this input (the fp32 linspace and erfinv admit no hand
    bound; 4 covers another reduction order) plus n u mean for the kernel's fp32 sum"""
    ref = wasserstein64(sorted_rows, power)
    err = abs(float(wasserstein_ref32(sorted_rows, power)) - float(ref))
    return 4 * err + sorted_rows.shape[1] * U * float(ref), err


def wasserstein_rows(n, seed):
    """three rows near N(0, 1), N(0.3, 1.5^2) and U(-2, 2): different distances, all finite"""
    g = rng(seed)
    return torch.stack([torch.randn(n, generator=g), torch.randn(n, generator=g) * 1.5 + 0.3, torch.rand(n, generator=g) * 4 - 2])


# ---- qkv re-tiling (rfrag / tfrag of csrc/attn.hip) -------------------------------------------------------------------------------
def rfrag_offset(bh, t, d, Tp):
    """Q / K element (bh, t, d): [bh][t / 32][kk = d / 16][lhi = (d / 8) & 1][t & 31][d & 7]"""
    ntb = Tp // 32
    return (((((bh * ntb + t // 32) * 4 + d // 16) * 2 + ((d // 8) & 1)) * 32 + (t & 31)) * 8) + (d & 7)


def tfrag_offset(bh, t, d, Tp):
    """V^T element (bh, t, d): [bh][t / 32][ks = tl / 16][db = d / 32][lhi = (tl / 4) & 1][d & 31][j], tl = t & 31 and
    j = 4 ((tl / 8) & 1) + (tl & 3): a lane's eight tokens are {16 ks + 4 lhi + 0..3} and {16 ks + 8 + 4 lhi + 0..3}"""
    ntb = Tp // 32
    tl = t & 31
    ks, lhi, j = tl // 16, (tl // 4) & 1, 4 * ((tl // 8) & 1) + (tl & 3)
    return ((((((bh * ntb + t // 32) * 2 + ks) * 2 + d // 32) * 2 + lhi) * 32 + (d & 31)) * 8) + j


def qkv_channel(which, h, d, heads, order):
    """channel of q / k / v (which = 0 / 1 / 2) of head h in the [3 C] axis: order 0 = (head, which, d), 1 = (which, head, d)"""
    return h * 192 + which * 64 + d if order == 0 else which * heads * 64 + h * 64 + d


def qkv_split_ref(qkv, heads, order):
    """qkv [N][T][3 C] int16 patterns -> (Q, K, V^T) flat [N heads Tp 64] int16, zero wherever no (n, h, t < T, d) lands"""
    N, T, _ = qkv.shape
    Tp = (T + 31) // 32 * 32
    n, h, t, d = np.meshgrid(np.arange(N), np.arange(heads), np.arange(T), np.arange(64), indexing="ij")
    bh = n * heads + h
    src = qkv.numpy()
    outs = []
    for which, off in ((0, rfrag_offset), (1, rfrag_offset), (2, tfrag_offset)):
        o = off(bh, t, d, Tp)
        assert len(np.unique(o)) == o.size and o.max() < N * heads * Tp * 64
        buf = np.zeros(N * heads * Tp * 64, dtype=np.int16)
        buf[o.ravel()] = src[n, t, qkv_channel(which, h, d, heads, order)].ravel()
        outs.append(torch.from_numpy(buf))
    return outs


def counter16(shape):
    """distinct non-zero 16-bit patterns 1, 2, 3, ... (fewer than 65536 elements)"""
    numel = int(np.prod(shape))
    assert numel < 65536
    return torch.from_numpy(np.arange(1, numel + 1, dtype=np.uint16).view(np.int16).copy()).reshape(shape)
