"""Float64 restatements of the guidance-loss kernels of csrc/losses.hip (pmi_head_loss in its four modes, pmi_smoothness,
pmi_sqdiff_loss), each with its analytic gradient, and the bounds tests/test_gpu_losses.py asserts.  tests/test_losses_cpu.py holds
the restatements to the reference's own values (tests/golden/losses_reference.npz), seeds defects into them and requires the same
bound functions to reject those.

Nothing of the reference and no engine import: CPU torch only.  U = 2^-24 is the fp32 unit roundoff.  Every evaluation function takes
a dtype: float64 is the reference, float32 the "same formula in fp32 on the CPU" the bounds must accept with room to spare.

How the bounds are built.  A bound is a multiple of U times a magnitude the float64 evaluation computes: the sum of the absolute terms
of the reduction for a loss, the per-element sum of absolute terms for a gradient.  Where a result depends on an earlier rounded result
(the loss and the gradient of a head depend on its outputs l), the earlier bound is carried forward to first order through the float64
derivative (|dterm/dl| for the loss, the Hessian |d2 term / dl dl| for the gradient), never through the code under test.
The multiples count roundings on the longest path and are not tuned on the kernels:
  SUM (68): a sum of fp32 terms of one sign in ANY tree of depth <= 64 (sequential runs of a few dozen, shuffle trees, slot sums) is off by
      at most depth * U * sum|terms|; 4 more for forming a term ((a - b)^2: two roundings) and the final scale.
  HEAD_OUT (48): e = emb / |emb| carries <= 12 U (a sum of D squares in a tree, sqrt, divide), the dot W.e a tree of depth <= 22 for D <= 1024
      plus the products, sqrt(D), bias: < 48 U (sum_d |W e| sq + |b|).
  HEAD_TERM (32): softmax in fp32 (expf to 2 ulp, K <= 16 additions, a division: <= 24 U relative), the product with k + 1, the square, the
      sum over n.
  HEAD_GRAD (64): two factors e (12 U each), the K-term sum W^T dl (16), the dot e.g over D (12), the final products (4) < 64.
  SMOOTH_GRAD (32): per element four differences (1 each, relative to the difference), two rounded coefficients, the products and three
      additions: 8 roundings on a path, every partial result below the sum of the absolute terms; times 4, because an evaluation that
      takes all 8 must still sit at a quarter of the bound.
  SQDIFF_GRAD (12): difference, rounded coefficient 2 / count, product: 3 roundings, times 4 for the same reason.

Observed ratios |fp32 CPU - float64| / bound at the inputs of tests/test_gpu_losses.py (worst case over every case; the bounds must
accept them with at least 4x room, tests/test_losses_cpu.py asserts <= 0.25):
  head out 0.037, head loss 0.061, head demb 0.038, smoothness loss 0.017, smoothness grad 0.105, sqdiff loss 0.018, sqdiff g 0.179
"""
import numpy as np
import torch

U = 2.0 ** -24
SUM, HEAD_OUT, HEAD_TERM, HEAD_GRAD, SMOOTH_GRAD, SQDIFF_GRAD = 68, 48, 32, 64, 32, 12
MODE_NAMES = {0: "simulacra", 1: "logit", 2: "expected", 3: "probability"}


def rng(seed):
    return torch.Generator().manual_seed(seed)


def within(got, ref, tol):
    d = (got.double() - ref.double()).abs()
    return bool((d <= tol).all())


def worst(got, ref, tol):
    """max |got - ref| / tol (inf when a difference is not finite): the figure the tests print before they assert"""
    d = (got.double() - ref.double()).abs()
    tol = tol if torch.is_tensor(tol) else torch.tensor(float(tol), dtype=torch.float64)
    r = torch.where(d == 0, torch.zeros_like(d), d / tol.clamp_min(1e-300))
    return float("inf") if not bool(torch.isfinite(r).all()) else float(r.max())


# ---- linear probe on the un-normalised embedding (pmi_head_loss) ---------------------------------------------------------------------
def _head_terms(l, mode, target, defect=None):
    """per-sample loss terms [N] (before mult / n_total) and dterm/dl [N][K] from the head outputs l [N][K], in l's dtype"""
    K = l.shape[1]
    idx = int(target) if defect == "index_without_minus_1" else int(target) - 1
    ks = torch.arange(1, K + 1, dtype=l.dtype)
    if mode == 0:
        df = l[:, 0] - target
        return df * df, (2 * df)[:, None]
    if mode == 1:
        dl = torch.zeros_like(l)
        dl[:, idx] = -0.01
        return -0.01 * l[:, idx], dl
    m = l.max(dim=1, keepdim=True).values
    p = torch.exp(l - m)
    p = p / p.sum(dim=1, keepdim=True)
    if mode == 2:
        if defect == "sum_before_square":
            f = (p * ks).sum(dim=1) - target
            term, gp = 0.01 * f * f, (0.02 * f)[:, None] * ks[None]
        else:
            f = p * ks - target
            term, gp = (0.01 / K) * (f * f).sum(dim=1), (0.02 / K) * f * ks
    else:
        term = -p[:, idx]
        gp = torch.zeros_like(p)
        gp[:, idx] = -1.0
    return term, p * (gp - (p * gp).sum(dim=1, keepdim=True))


def head_eval(emb, W, b, mode, target, n_total, mult, gscale, dtype=torch.float64, defect=None):
    """(out [N][K], loss, demb [N][D]) of pmi_head_loss evaluated in ``dtype``.  defect: None, "no_sqrt_d" (mode 0),
    "sum_before_square" (mode 2), "index_without_minus_1" (modes 1, 3), "n_for_n_total"."""
    emb, W, b = emb.to(dtype), W.to(dtype), b.to(dtype)
    N, D = emb.shape
    sq = float(D) ** 0.5 if (mode == 0 and defect != "no_sqrt_d") else 1.0
    nrm = emb.norm(dim=1, keepdim=True).clamp_min(1e-12)
    e = emb / nrm
    l = sq * (e @ W.t()) + b
    term, dl = _head_terms(l, mode, target, defect)
    count = N if defect == "n_for_n_total" else n_total
    loss = mult * term.sum() / count
    ge = sq * (dl @ W)
    demb = (mult * gscale / count) * (ge - e * (e * ge).sum(dim=1, keepdim=True)) / nrm
    return l, loss, demb


def head_loss_autograd64(emb, W, b, mode, target, n_total, mult):
    """the same loss by float64 autograd from the embedding: (loss, dloss/demb) -- the check on the analytic gradient above"""
    x = emb.double().clone().requires_grad_(True)
    with torch.enable_grad():
        e = torch.nn.functional.normalize(x, dim=1)
        l = (float(x.shape[1]) ** 0.5 if mode == 0 else 1.0) * (e @ W.double().t()) + b.double()
        K = l.shape[1]
        if mode == 0:
            loss = mult * ((l[:, 0] - target) ** 2).sum() / n_total
        elif mode == 1:
            loss = -0.01 * mult * l[:, int(target) - 1].sum() / n_total
        elif mode == 2:
            p = torch.softmax(l, dim=1) * torch.arange(1, K + 1, dtype=torch.float64)
            loss = 0.01 * mult * ((p - target) ** 2).sum() / (n_total * K)
        else:
            loss = -mult * torch.softmax(l, dim=1)[:, int(target) - 1].sum() / n_total
        (g,) = torch.autograd.grad(loss, x)
    return loss.detach(), g


def head_tol(emb, W, b, mode, target, n_total, mult, gscale):
    """(out_tol [N][K], loss_tol, demb_tol [N][D]) at this input, from float64 quantities only (see the module docstring)"""
    emb, W, b = emb.double(), W.double(), b.double()
    N, D = emb.shape
    K = W.shape[0]
    sq = float(D) ** 0.5 if mode == 0 else 1.0
    nrm = emb.norm(dim=1, keepdim=True).clamp_min(1e-12)
    e = emb / nrm
    out_tol = HEAD_OUT * U * (sq * (e.abs() @ W.abs().t()) + b.abs())
    l = (sq * (e @ W.t()) + b).requires_grad_(True)
    with torch.enable_grad():
        term, dl = _head_terms(l, mode, target)
        H = torch.zeros(N, K, K, dtype=torch.float64)             # H[n][k][j] = d dl[n][k] / d l[n][j]
        if dl.requires_grad:
            for k in range(K):
                (H[:, k, :],) = torch.autograd.grad(dl[:, k].sum(), l, retain_graph=True)
    l, term, dl = l.detach(), term.detach(), dl.detach()
    # absolute terms of a sample's loss term and of dl
    ks = torch.arange(1, K + 1, dtype=torch.float64)
    if mode >= 2:
        p = torch.softmax(l, dim=1)
    if mode == 2:
        f = p * ks - target
        fa = f.abs() + 2 * p * ks
        term_abs = (0.01 / K) * (f.abs() * fa).sum(dim=1)
        gp_abs = (0.02 / K) * ks * fa
    elif mode == 3:
        term_abs = term.abs()
        gp_abs = torch.zeros_like(p)
        gp_abs[:, int(target) - 1] = 1.0
    else:
        term_abs = term.abs()
    dl_abs = dl.abs() if mode < 2 else p * (gp_abs + (p * gp_abs).sum(dim=1, keepdim=True))
    cl = abs(mult) / n_total
    loss_tol = cl * float((dl.abs() * out_tol).sum()) + HEAD_TERM * U * cl * float(term_abs.sum())
    ddl = torch.einsum("nkj,nj->nk", H.abs(), out_tol) + HEAD_TERM * U * dl_abs

    def through(v):     # |c / nrm| sq (|W|^T v + |e| (|e| . |W|^T v)) for a non-negative v [N][K]
        g = sq * (v @ W.abs())
        return abs(mult * gscale) / n_total * (g + e.abs() * (e.abs() * g).sum(dim=1, keepdim=True)) / nrm

    demb_tol = through(ddl) + HEAD_GRAD * U * through(dl.abs())
    return out_tol, loss_tol, demb_tol


def head_inputs(N, D, K, seed):
    g = rng(seed)
    emb = torch.randn(N, D, generator=g) * 3
    W = torch.randn(K, D, generator=g) * (float(D) ** -0.5 if K == 1 else 1.0)
    b = torch.randn(K, generator=g) * 0.05 + (5.0 if K == 1 else 0.0)
    return emb, W, b


# ---- smoothness (pmi_smoothness) -------------------------------------------------------------------------------------------------------
def smoothness_eval(x, n_total, gscale, dtype=torch.float64, defect=None):
    """(loss, grad, grad_mag): loss = sum dh^2 / (n_total C (H-1) W) + sum dw^2 / (n_total C H (W-1)); grad = gscale dloss/dx with every
    element reading its four neighbours; grad_mag = the per-element sum of the absolute terms.  defect: "both_over_hw" (both sums divided
    by n_total C H W), "grad_misses_last_row", "grad_misses_last_col" (the backward difference into the last row / column is lost)."""
    x = x.to(dtype)
    N, C, H, W = x.shape
    dh, dw = x[:, :, 1:] - x[:, :, :-1], x[:, :, :, 1:] - x[:, :, :, :-1]
    ch, cw = n_total * C * (H - 1) * W, n_total * C * H * (W - 1)
    if defect == "both_over_hw":
        ch = cw = n_total * C * H * W
    loss = (dh * dh).sum() / ch + (dw * dw).sum() / cw
    gh, gw = 2.0 * gscale / ch, 2.0 * gscale / cw
    grad, mag = torch.zeros_like(x), torch.zeros_like(x)
    grad[:, :, :-1] -= gh * dh; mag[:, :, :-1] += gh * dh.abs()
    grad[:, :, :, :-1] -= gw * dw; mag[:, :, :, :-1] += gw * dw.abs()
    hs = slice(1, H - 1) if defect == "grad_misses_last_row" else slice(1, H)
    ws = slice(1, W - 1) if defect == "grad_misses_last_col" else slice(1, W)
    grad[:, :, hs] += gh * dh[:, :, :hs.stop - 1]; mag[:, :, 1:] += gh * dh.abs()
    grad[:, :, :, ws] += gw * dw[:, :, :, :ws.stop - 1]; mag[:, :, :, 1:] += gw * dw.abs()
    return loss, grad, mag


def smoothness_tol(x, n_total, gscale):
    loss, _, mag = smoothness_eval(x, n_total, gscale)
    return SUM * U * float(loss), SMOOTH_GRAD * U * mag


def smoothness_input(shape, seed):
    return torch.rand(shape, generator=rng(seed)) * 1.2 - 0.1


# ---- squared difference (pmi_sqdiff_loss) ------------------------------------------------------------------------------------------------
def sqdiff_eval(a, b, n_total_count, dtype=torch.float64, defect=None):
    """(loss, g_a, g_b): loss = sum (a - b)^2 / n_total_count, g_a = 2 (a - b) / n_total_count, g_b = -g_a.
    defect: "b_gradient_sign" (g_b = +g_a)."""
    a, b = a.to(dtype), b.to(dtype)
    d = a - b
    g = (2.0 / n_total_count) * d
    return (d * d).sum() / n_total_count, g, (g if defect == "b_gradient_sign" else -g)


def sqdiff_tol(a, b, n_total_count):
    loss, g, _ = sqdiff_eval(a, b, n_total_count)
    return SUM * U * float(loss), SQDIFF_GRAD * U * g.abs()


def sqdiff_inputs(count, seed):
    g = rng(seed)
    return torch.randn(count, generator=g), torch.randn(count, generator=g) * 0.5 + 0.1


# ---- the resize loss through the product's own band tables (losses.Resize against the fixture) ---------------------------------------------
def _dense(idx, w, in_sz):
    """idx / w [out][taps] -> (A, |A|, mask of valid taps) [out][in] in float64"""
    out_sz, taps = idx.shape
    A = torch.zeros(out_sz, in_sz, dtype=torch.float64)
    M = torch.zeros_like(A)
    for j in range(out_sz):
        for t in range(taps):
            r = int(idx[j, t])
            if r >= 0:
                A[j, r] += float(w[j, t])
                M[j, r] = 1.0
    return A, A.abs(), M


TABLE = 16      # an fp32 tap weight (|w| <= 1: sin / polynomial in fp32, then the normalisation) against the exact one: <= 16 U absolute


def band_chain_tol(x_abs, x_err, passes):
    """A chain of banded passes y = A x along an axis, each computed in fp32 from fp32 tables: carries the incoming error bound x_err and
    the magnitude x_abs forward; a pass adds (taps + 1) U |A| |x| for its arithmetic (tests/_glue_ref64.band_tol) and TABLE U mask |x| for
    its table.  passes: [(axis, A, |A|, mask, taps)]; returns (|y| bound, error bound)."""
    for axis, _, Aabs, M, taps in passes:
        eq = "jr,ncrw->ncjw" if axis == 2 else "jr,nchr->nchj"
        x_err = torch.einsum(eq, Aabs, x_err) + U * torch.einsum(eq, (taps + 1) * Aabs + TABLE * M, x_abs)
        x_abs = torch.einsum(eq, Aabs, x_abs)
    return x_abs, x_err


def resize_passes(in_hw, out_hw, adjoint=False):
    """the passes of transforms.resize (adjoint: of transforms.resize_backward) as (axis, A, |A|, mask, taps), from the product's host tables"""
    import importlib
    rz = importlib.import_module("perceptor_amd.transforms.resize")
    method, dims = rz._plan(int(in_hw[0]), int(in_hw[1]), tuple(int(v) for v in out_hw))
    passes = []
    for _, axis, i, o in dims:
        idx, w, idx_t, _ = rz.band_tables(i, o, method)
        A, Aabs, M = _dense(idx, w, i)
        passes.append((axis, A.t().contiguous(), Aabs.t().contiguous(), M.t().contiguous(), idx_t.shape[1]) if adjoint
                      else (axis, A, Aabs, M, idx.shape[1]))
    return passes[::-1] if adjoint else passes


def resize64(x, size):
    """transforms.resize in float64 with the product's fp32 tables"""
    x = x.double()
    for axis, A, _, _, _ in resize_passes(x.shape[2:], size):
        x = torch.einsum("jr,ncrw->ncjw" if axis == 2 else "jr,nchr->nchj", A, x)
    return x


def resize_loss_tol(a, b, size):
    """(loss_tol, grad_a_tol, grad_b_tol) of losses.Resize at (a, b, size).  The resized values' error bounds go to first order through
    the squared difference (2 |d| (err_a + err_b) / count) and through the adjoint passes."""
    ra64, rb64 = resize64(a, size), resize64(b, size)
    count = ra64.numel()
    _, ea = band_chain_tol(a.double().abs(), torch.zeros_like(a, dtype=torch.float64), resize_passes(a.shape[2:], size))
    _, eb = band_chain_tol(b.double().abs(), torch.zeros_like(b, dtype=torch.float64), resize_passes(b.shape[2:], size))
    d = ra64 - rb64
    loss_tol = float((2 * d.abs() * (ea + eb)).sum()) / count + SUM * U * float((d * d).sum()) / count
    g_abs = 2 * d.abs() / count
    g_err = 2 * (ea + eb) / count + SQDIFF_GRAD * U * g_abs
    _, ga = band_chain_tol(g_abs, g_err, resize_passes(a.shape[2:], size, adjoint=True))
    _, gb = band_chain_tol(g_abs, g_err, resize_passes(b.shape[2:], size, adjoint=True))
    return loss_tol, ga, gb
