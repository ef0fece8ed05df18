"""GPU: models.OWLViT / losses.OWLViT -- the head kernels of csrc/owlvit.hip by name, VitEngine.backward_tokens, the engine and the classes
against the reference's own numbers (tests/golden/owlvit_reference_{a,b}.npz), the product configuration.

A. Kernels against float64, per element.  Every output sits in a NaN-filled buffer with NaN guard bands on both sides, and every kernel
   runs twice: the bands stay NaN and the two runs are bit-equal.  Bounds are running-error bounds in the convention of DESIGN.md
   section 17, n u A with u = 2^-24: A is the same formula evaluated on absolute values (for a chain of stages, the first-order
   propagation of the previous stage's A through the next stage's |Jacobian|), n the number of fp32 roundings on the longest path -- a
   W-term reduction is W / 64 sequential adds per lane + 6 shuffle steps, + 10 for the point-wise operations of a stage (division, rsqrt,
   exp / log / expm1 at a few ulp each).  No fitted constant.  16-bit outputs add the type's u |ref|.
     merge fwd / bwd   (N, T, W) = (2, 10, 128), (1, 17, 128), (1, 577, 768); bwd teacher-forced on the forward kernel's own mean / rstd;
                       feats16 == round(feats32) bit for bit
     class fwd / bwd   P in {9, 576} x D in {32, 512} x Q in {1, 3, 5}
     top-k loss        P in {4, 5, 9, 576}, k = 5 (P < k, P = k, P > k, several elements per thread); the selected set is read off dlogits
     box out           grid 3, 4, 24
B. VitEngine.backward_tokens at fixture (a)'s tower, bf16 and f16: block by block, teacher-forced, at the sqrt(k) u gates of
   tests/test_gpu_vit_tower.py (K_MLP_BWD, K_ATTN_BWD_FLASH, K_STEM_BWD: the roundings on each piece's path), and a gradient that is
   non-zero on the class rows only against backward() for the d_emb it came from, within the whole-tower gate.
C. OwlVitEngine and the classes against the fixtures.  Tolerance = 2 x the distance of the EMULATED float64 restatement
   (tests/_owlvit_ref64.py, emulate=dtype) from the fixture, measured on the CPU (max abs for logits, boxes and the loss; max |err| /
   max |ref| for gradients):
                      logits     boxes      loss       d/d hidden  d loss/d images  d scores.mean()/d images
       (a) bf16       2.710e-02  1.268e-03  8.916e-06  1.202e-02   3.499e-02        1.071e-02
       (a) f16        2.521e-03  1.604e-04  2.219e-06  1.823e-03   2.576e-03        9.553e-04
       (b) bf16       2.808e-02  1.839e-03  1.017e-05  6.876e-03   1.116e-02        5.633e-03
       (b) f16        1.535e-03  1.473e-04  2.405e-06  6.559e-04   2.204e-03        7.759e-04
   The top-k set pmi_owl_topk_loss selected on that run, read off its dlogits, must equal the float64 one in every (image, query) column
   (tests/test_owlvit_cpu.py holds the gap condition).
   Seeded defects: the ENGINE's outputs at these inputs are farther than 2 x the gate from the float64 restatement carrying each defect of
   _owlvit_ref64.DEFECTS (multiples printed), i.e. the engine has none of them.  ``query eps inside`` moves the logits by 2.4e-6 and cannot
   be seen at a 16-bit gate; it is checked where it lives: prepare_queries' output minus pooled / |pooled| of the engine's own pooled rows is
   1e-6 in EVERY component to fp32 rounding (the library's form would give -1e-6 q / |q|, which varies by component and sign).
D. The product configuration, synthetic weights, N = 1: forward and loss_and_grad, shapes and finiteness only.

Measured on one MI355X: the [bound] lines this module prints; the table is DESIGN.md section 31.
"""
import functools
import math

import numpy as np
import pytest
import torch

import _owlvit_ref64 as O
import _vit_ref64 as V

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
DTYPES = ["bf16", "f16"]
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
GUARD = 256
MEASURED = {   # section C of the module doc
    ("a", "bf16"): dict(logits=2.710e-02, boxes=1.268e-03, loss=8.916e-06, grad_hidden=1.202e-02, grad_images=3.499e-02, grad_scores=1.071e-02),
    ("a", "f16"): dict(logits=2.521e-03, boxes=1.604e-04, loss=2.219e-06, grad_hidden=1.823e-03, grad_images=2.576e-03, grad_scores=9.553e-04),
    ("b", "bf16"): dict(logits=2.808e-02, boxes=1.839e-03, loss=1.017e-05, grad_hidden=6.876e-03, grad_images=1.116e-02, grad_scores=5.633e-03),
    ("b", "f16"): dict(logits=1.535e-03, boxes=1.473e-04, loss=2.405e-06, grad_hidden=6.559e-04, grad_images=2.204e-03, grad_scores=7.759e-04),
}


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


class _Guarded:
    """a NaN-filled device buffer with NaN guard bands; .t is the interior view handed to the kernel"""

    def __init__(self, shape, dev, dtype=torch.float32):
        n = int(torch.Size(shape).numel())
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=dtype, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(shape)

    def ok(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all() and torch.isfinite(self.t).all())


def _twice(run):
    """run() -> tuple of _Guarded; twice: bands intact, interiors finite, equal bits"""
    a, b = run(), run()
    torch.cuda.synchronize()
    assert all(o.ok() for o in a + b)
    assert all(torch.equal(p.t, q.t) for p, q in zip(a, b)), "two runs differ"
    return a


def _worst(tag, err, tol):
    ratio = float((err / tol).max())
    print(f"[bound] owlvit {tag}: worst error {ratio:.3f} of its bound (max abs error {float(err.max()):.3e})")
    return ratio


def _chain(w):
    return w / 64 + 6 + 10


# ---- A. merge ---------------------------------------------------------------------------------------------------------------------------------
MERGE_SHAPES = [(2, 10, 128), (1, 17, 128), (1, 577, 768)]


@functools.lru_cache(maxsize=None)
def _merge_inputs(shape):
    n, t, w = shape
    g = torch.Generator().manual_seed(n * 100000 + t * 1000 + w)
    r = lambda *s: torch.randn(*s, generator=g)
    return dict(x=r(n, t, w) * 1.5 + 0.3, g1=1 + 0.2 * r(w), b1=0.1 * r(w), g2=1 + 0.2 * r(w), b2=0.1 * r(w), df=r(n * (t - 1), w))


def _merge_fwd(I, shape, dtype, dev):
    from perceptor_amd import _hip
    from perceptor_amd._hip import call, ptr
    n, t, w = shape
    d = {k: v.to(dev) for k, v in I.items()}
    f32, f16 = _Guarded((n * (t - 1), w), dev), _Guarded((n * (t - 1), w), dev, TD[dtype])
    mr1, mr2 = _Guarded((2, n * t), dev), _Guarded((2, n * (t - 1)), dev)
    call("pmi_owl_merge_ln_fwd", ptr(d["x"]), ptr(d["g1"]), ptr(d["b1"]), ptr(d["g2"]), ptr(d["b2"]), ptr(f32.t), ptr(f16.t), ptr(mr1.t), ptr(mr2.t),
         n, t, w, 1e-5, _hip.dtype_code(dtype))
    return f32, f16, mr1, mr2


def _ln_abs(x, mean, rstd, gamma, beta):
    """(x_hat, y, A_y): the running-error companion of a LayerNorm output"""
    xh = (x - mean) * rstd
    return xh, xh * gamma + beta, (x.abs() + mean.abs()) * rstd * gamma.abs() + beta.abs()


def _jac_abs(a, xh, rstd, gamma):
    """|Jacobian of LayerNorm| applied to a non-negative tensor, times |gamma| (forward) -- also the companion of its vjp with a = |gy|"""
    return rstd * (a + a.mean(-1, keepdim=True) + xh.abs() * (xh.abs() * a).mean(-1, keepdim=True))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", MERGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_merge_ln_fwd_bwd(shape, dtype):
    """pmi_owl_merge_ln_fwd, pmi_owl_merge_ln_bwd"""
    from perceptor_amd import _hip
    from perceptor_amd._hip import call, ptr
    n, t, w = shape
    dev, I = _dev(), _merge_inputs(shape)
    f32, f16, mr1, mr2 = _twice(lambda: _merge_fwd(I, shape, dtype, dev))
    tag = f"merge {shape} {dtype}"
    D = {k: v.double() for k, v in I.items()}
    x = D["x"]
    mean1 = x.mean(-1, keepdim=True)
    rstd1 = ((x - mean1).square().mean(-1, keepdim=True) + 1e-5).rsqrt()
    xh, y, Ay = _ln_abs(x, mean1, rstd1, D["g1"], D["b1"])
    m = y[:, 1:] * y[:, :1]
    Am = Ay[:, 1:] * Ay[:, :1]
    mean2 = m.mean(-1, keepdim=True)
    rstd2 = ((m - mean2).square().mean(-1, keepdim=True) + 1e-5).rsqrt()
    mh, f, Af0 = _ln_abs(m, mean2, rstd2, D["g2"], D["b2"])
    Af = Af0 + D["g2"].abs() * _jac_abs(Am, mh, rstd2, 1.0)
    nfw = 3 * _chain(w)
    got = f32.t.cpu().double().view(n, t - 1, w)
    assert _worst(f"{tag} feats", (got - f).abs(), nfw * U32 * Af) <= 1.0
    assert torch.equal(f16.t, f32.t.to(TD[dtype])), "feats16 is not the rounded feats32"
    assert _worst(f"{tag} mean1", (mr1.t[0].cpu().double() - mean1.reshape(-1)).abs(), _chain(w) * U32 * x.abs().mean(-1).reshape(-1)) <= 1.0
    assert _worst(f"{tag} rstd1", (mr1.t[1].cpu().double() - rstd1.reshape(-1)).abs(), 2 * _chain(w) * U32 * ((x.abs() + mean1.abs()).square().mean(-1, keepdim=True) * rstd1 ** 3).reshape(-1)) <= 1.0
    # ---- backward, teacher-forced on the kernel's own statistics
    d = {k: v.to(dev) for k, v in I.items()}
    m1c, m2c = mr1.t.contiguous(), mr2.t.contiguous()
    nblk = _hip.lib().pmi_owl_merge_bwd_blocks(t)
    assert nblk == (t - 1 + 7) // 8

    def bwd():
        dx, part = _Guarded((n, t, w), dev), _Guarded((n, nblk, w), dev)
        call("pmi_owl_merge_ln_bwd", ptr(d["df"]), ptr(d["x"]), ptr(d["g1"]), ptr(d["b1"]), ptr(d["g2"]), ptr(m1c), ptr(m2c), ptr(dx.t), ptr(part.t), n, t, w)
        return dx, part

    dx, _ = _twice(bwd)
    k1, r1 = m1c[0].cpu().double().view(n, t, 1), m1c[1].cpu().double().view(n, t, 1)
    k2, r2 = m2c[0].cpu().double().view(n, t - 1, 1), m2c[1].cpu().double().view(n, t - 1, 1)
    xh, y, Ay = _ln_abs(x, k1, r1, D["g1"], D["b1"])
    mh = (y[:, 1:] * y[:, :1] - k2) * r2
    gy = D["df"].view(n, t - 1, w) * D["g2"]
    dm = r2 * (gy - gy.mean(-1, keepdim=True) - mh * (gy * mh).mean(-1, keepdim=True))
    Adm = _jac_abs(gy.abs(), mh, r2, 1.0)
    dy = torch.cat([(dm * y[:, 1:]).sum(1, keepdim=True), dm * y[:, :1]], dim=1)
    Ady = torch.cat([(Adm * Ay[:, 1:]).sum(1, keepdim=True), Adm * Ay[:, :1]], dim=1)
    gy1 = dy * D["g1"]
    ref = r1 * (gy1 - gy1.mean(-1, keepdim=True) - xh * (gy1 * xh).mean(-1, keepdim=True))
    Adx = _jac_abs(Ady * D["g1"].abs(), xh, r1, 1.0)
    nbw = 3 * _chain(w) + (t - 1) / 8 + 8                                   # + the class row's sum over blocks (and two rows, four waves, inside one)
    assert float(ref.abs().max()) > 0
    assert _worst(f"{tag} dx patch rows", (dx.t.cpu().double() - ref).abs()[:, 1:], (nbw * U32 * Adx)[:, 1:]) <= 1.0
    assert _worst(f"{tag} dx class row", (dx.t.cpu().double() - ref).abs()[:, 0], (nbw * U32 * Adx)[:, 0]) <= 1.0


# ---- A. class head ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _class_inputs(p, d, q):
    g = torch.Generator().manual_seed(p * 10000 + d * 10 + q)
    r = lambda *s: torch.randn(*s, generator=g)
    ld = (d + 2 + 31) // 32 * 32
    gg = r(2 * p, ld)
    gg[:, d + 1] = gg[:, d + 1] * 2                                          # the ELU argument on both sides of 0
    qq = torch.nn.functional.normalize(r(q, d)) + 1e-6
    return dict(g=gg, q=qq, dl=r(2 * p, q) * 0.01)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("q", [1, 3, 5])
@pytest.mark.parametrize("d", [32, 512])
@pytest.mark.parametrize("p", [9, 576])
def test_class_logits_fwd_bwd(p, d, q, dtype):
    """pmi_owl_class_logits_fwd, pmi_owl_class_logits_bwd"""
    from perceptor_amd import _hip
    from perceptor_amd._hip import call, ptr
    dev, I = _dev(), _class_inputs(p, d, q)
    m, ld = I["g"].shape
    G = {k: v.to(dev) for k, v in I.items()}

    def fwd():
        lg, ce = _Guarded((m, q), dev), _Guarded((m, d), dev)
        call("pmi_owl_class_logits_fwd", ptr(G["g"]), ld, ptr(G["q"]), ptr(lg.t), ptr(ce.t), m, d, q)
        return lg, ce

    lg, ce = _twice(fwd)
    tag = f"class P={p} D={d} Q={q} {dtype}"
    g64, q64, dl = I["g"].double(), I["q"].double(), I["dl"].double()
    e, sh, s = g64[:, :d], g64[:, d:d + 1], g64[:, d + 1:d + 2]
    nrm = e.norm(dim=-1, keepdim=True)
    inv = 1 / (nrm + 1e-6)
    eh, sc = e * inv, O.elu1(s)
    dot = eh @ q64.t()
    n1 = _chain(d)
    assert _worst(f"{tag} class_embeds", (ce.t.cpu().double() - eh).abs(), n1 * U32 * eh.abs()) <= 1.0
    A = (eh.abs() @ q64.abs().t() + sh.abs()) * sc
    assert _worst(f"{tag} logits", (lg.t.cpu().double() - (dot + sh) * sc).abs(), 2 * n1 * U32 * A) <= 1.0

    def bwd():
        dg = _Guarded((m, ld), dev, TD[dtype])
        call("pmi_owl_class_logits_bwd", ptr(G["dl"]), ptr(G["g"]), ld, ptr(G["q"]), ptr(dg.t), m, d, q, _hip.dtype_code(dtype))
        return (dg,)

    (dg,) = _twice(bwd)
    deh = (dl * sc) @ q64
    Adeh = (dl.abs() * sc) @ q64.abs()
    t = (deh * e).sum(-1, keepdim=True)
    de = deh * inv - e * t * inv * inv / nrm
    Ade = Adeh * inv + e.abs() * (Adeh * e.abs()).sum(-1, keepdim=True) * inv * inv / nrm
    dsh, Adsh = (dl * sc).sum(-1, keepdim=True), (dl.abs() * sc).sum(-1, keepdim=True)
    ds = (dl * (dot + sh)).sum(-1, keepdim=True) * O.elu1_grad(s)
    Ads = (dl.abs() * (eh.abs() @ q64.abs().t() + sh.abs())).sum(-1, keepdim=True) * O.elu1_grad(s)
    ref = torch.cat([de, dsh, ds, torch.zeros(m, ld - d - 2, dtype=torch.float64)], dim=-1)
    Aref = torch.cat([Ade, Adsh, Ads, torch.zeros(m, ld - d - 2, dtype=torch.float64)], dim=-1)
    tol = V.U[TD[dtype]] * ref.abs() + (3 * n1 + q) * U32 * Aref + 2.0 ** -25
    got = dg.t.cpu().double()
    assert torch.equal(got[:, d + 2:], torch.zeros(m, ld - d - 2, dtype=torch.float64)), "the GEMM's pad columns are not zero"
    assert _worst(f"{tag} dg", (got - ref).abs(), tol) <= 1.0


# ---- A. top-k loss ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [4, 5, 9, 576])
def test_topk_loss(p):
    """pmi_owl_topk_loss"""
    from perceptor_amd._hip import call, ptr
    dev = _dev()
    n, q, k = 2, 3, 5
    g = torch.Generator().manual_seed(p)
    logits = torch.randn(n, p, q, generator=g) * 2
    w = torch.tensor([1.0, 0.5, 2.0])
    L, Wd = logits.to(dev), w.to(dev)

    def run(mul=1.0):
        dl, part = _Guarded((n, p, q), dev), _Guarded((n * q,), dev)
        call("pmi_owl_topk_loss", ptr(L), ptr(Wd), ptr(dl.t), ptr(part.t), n, p, q, k, mul)
        return dl, part

    dl, part = _twice(run)
    x = logits.double()
    loss, ref = O.topk_loss(x, w.double(), k)
    ke = min(k, p)
    lse = torch.logsumexp(x, dim=1, keepdim=True)
    sel = O.topk_sets(x, k)
    coef = (0.01 * w.double() / (n * ke)).view(1, 1, q)
    nn_ = p / 256 + 8 + 10
    got = dl.t.cpu().double()
    tol = coef * (ke * torch.exp(x - lse) * nn_ * U32 * (1 + x.abs() + lse.abs()) + 4 * U32 * (sel.double() - ke * torch.exp(x - lse)).abs() + 4 * U32)
    assert _worst(f"topk P={p} dlogits", (got - ref).abs(), tol) <= 1.0
    got_sel = (got - coef * ke * torch.exp(x - lse)).abs() > coef / 2                 # the indicator's share of dlogits
    assert torch.equal(got_sel, sel), "the selected set differs from the float64 one"
    parts = -coef.view(q) * ((x - lse) * sel).sum(dim=1)                              # [n, q]
    Aparts = coef.view(q) * ((x.abs() + lse.abs()) * sel).sum(dim=1)
    assert _worst(f"topk P={p} partials", (part.t.cpu().double().view(n, q) - parts).abs(), (nn_ + ke) * U32 * Aparts) <= 1.0
    assert abs(float(part.t.sum()) - float(loss)) <= float(((nn_ + ke + n * q) * U32 * Aparts).sum())
    dl2, _ = run(65536.0)
    torch.cuda.synchronize()
    assert float(((dl2.t.cpu().double() / 65536.0 - got).abs() / (2 * U32 * ref.abs() + 1e-30)).max()) <= 1.0, "mul is not a plain factor"


# ---- A. box out -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("grid,w", [(3, 128), (4, 128), (24, 768)])
def test_box_out(grid, w, dtype):
    """pmi_owl_box_out"""
    from perceptor_amd import _hip
    from perceptor_amd._hip import call, ptr
    from perceptor_amd.engine.owlvit import box_bias
    dev = _dev()
    p = grid * grid
    m = 2 * p
    g = torch.Generator().manual_seed(grid * 1000 + w)
    h = torch.randn(m, w, generator=g).to(TD[dtype])
    w2, b2 = torch.randn(4, w, generator=g) * w ** -0.5, torch.randn(4, generator=g) * 0.1
    bias = box_bias(grid)
    assert torch.equal(bias.double(), O.box_bias(grid))
    H, W2, B2, BB = h.to(dev), w2.to(dev), b2.to(dev), bias.to(dev)

    def run():
        out = _Guarded((m, 4), dev)
        call("pmi_owl_box_out", ptr(H), w, ptr(W2), ptr(B2), ptr(BB), ptr(out.t), m, p, w, _hip.dtype_code(dtype))
        return (out,)

    (out,) = _twice(run)
    z = h.double() @ w2.double().t() + b2.double() + bias.double().repeat(2, 1)
    Az = h.double().abs() @ w2.double().abs().t() + b2.double().abs() + bias.double().abs().repeat(2, 1)
    tol = 0.25 * (w / 64 + 6 + 4) * U32 * Az + 8 * U32
    assert _worst(f"box grid={grid} W={w} {dtype}", (out.t.cpu().double() - torch.sigmoid(z)).abs(), tol) <= 1.0


# ---- B / C. the engine ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fixture(name):
    sd, R = O.load_fixture(name)
    return sd, R, torch.from_numpy(R["images8"]).double() / 255, torch.from_numpy(R["ids"]), torch.from_numpy(R["weights"]), int(R["top_k"])


@functools.lru_cache(maxsize=None)
def _engine(name, dtype):
    from perceptor_amd.engine.owlvit import OwlVitEngine
    sd, R, *_ = _fixture(name)
    _dev()
    return OwlVitEngine(tuple(int(c) for c in R["cfg"]), tuple(int(c) for c in R["text_cfg"]), {k: v.float() for k, v in sd.items()}, "cuda:0", dtype)


@functools.lru_cache(maxsize=None)
def _emulated(name, dtype):
    sd, R, img, ids, w, k = _fixture(name)
    m = O.OwlVit(sd, R["cfg"], R["text_cfg"], emulate=TD[dtype])
    return m, m.forward(img, ids)


def _unfrag(wt, n, heads, t):
    nh, tp32, _ = wt.shape
    return wt.reshape(nh, tp32 // 32, 4, 2, 32, 8).permute(0, 1, 4, 2, 3, 5).reshape(nh, tp32, 64)[:, :t].reshape(n, heads, t, 64)


@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_tokens_block_by_block(dtype):
    """VitEngine.backward_tokens at fixture (a)'s tower: teacher-forced at the block-boundary gates of tests/test_gpu_vit_tower.py"""
    _, R, img, ids, w, k = _fixture("a")
    eng = _engine("a", dtype).vit
    ref = _emulated("a", dtype)[0].tower
    u = V.U[TD[dtype]]
    res, patch, width, layers, heads, out = eng.cfg
    n, t = img.shape[0], (res // patch) ** 2 + 1
    gen = torch.Generator().manual_seed(5)
    d_hidden = (torch.randn(n, t, width, generator=gen) * 1e-3 * eng.gscale).cuda()
    x = img.float().cuda()
    eng.forward(x, save=True)
    sv, rec = eng.saved, {}
    grad = eng.backward_tokens(d_hidden, record=rec)
    torch.cuda.synchronize()
    assert torch.isfinite(grad).all() and grad.shape == x.shape and eng.saved is None
    c = lambda z: z.detach().cpu().double()
    tok = lambda z: c(z).reshape(n, t, -1)
    gs = eng.gscale
    g32, gm32 = [tok(g) / gs for g in rec["g32"]], [tok(g) / gs for g in rec["gm32"]]
    assert torch.equal(rec["g32"][0].view(n, t, width), d_hidden)
    checks = []
    for j, i in enumerate(reversed(range(layers))):
        L = sv["layers"][i]
        q, kk, v = (c(_unfrag(L["aws"][z], n, heads, t)) for z in range(3))
        lay = dict(q=q, k=kk, v=v)
        checks.append((f"block{i} mlp bwd", V.row_stat(gm32[j] - g32[j], ref.mlp_vjp(i, g32[j], tok(L["x_mid"]), tok(L["hpre"]))), V.K_MLP_BWD))
        checks.append((f"block{i} attn bwd", V.row_stat(g32[j + 1] - gm32[j], ref.attn_vjp(i, gm32[j], tok(L["x_in"]), lay)), V.K_ATTN_BWD_FLASH))
    g0, dcol, dimg = ref.stem_vjp(g32[-1], c(sv["x0"]), n)
    checks.append(("stem g0", V.row_stat(c(rec["g0"]).reshape(g0.shape) / gs, g0), V.K_STEM_BWD))
    checks.append(("stem grad per patch", V.row_stat(V.patches(c(grad), patch), V.patches(dimg, patch)), V.K_STEM_BWD))
    for name, st, kq in checks:
        print(f"[bound] owlvit backward_tokens {dtype} {name}: {st / u:.3f} u, gate sqrt({kq}) u ({st / (u * kq ** 0.5):.2f} of it)")
    assert all(st <= u * kq ** 0.5 for _, st, kq in checks), checks
    # ---- a gradient on the class rows only reproduces backward()
    emb = eng.forward(x, save=True)
    sv2 = eng.saved
    d_emb = (torch.randn(n, out, generator=gen) * 1e-3 * gs).cuda()
    rec2 = {}
    want = eng.backward(d_emb, record=rec2)
    cls_only = rec2["g32"][0].view(n, t, width).clone()
    assert float(cls_only[:, 1:].abs().max()) == 0.0 and float(cls_only[:, 0].abs().max()) > 0
    eng.saved = sv2
    got = eng.backward_tokens(cls_only)
    torch.cuda.synchronize()
    st, depth = V.rel_l2(got.cpu(), want.cpu()), V.depth_grad(layers, True)
    print(f"[bound] owlvit backward_tokens {dtype} class rows only vs backward: rel-L2 {st:.3e} (bit-equal: {torch.equal(got, want)}), gate sqrt({depth}) u = {u * depth ** 0.5:.3e}")
    assert st <= u * depth ** 0.5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["a", "b"])
def test_engine_against_the_reference(name, dtype):
    """OwlVitEngine forward, pmi_owl_topk_loss and backward against the fixture, at 2 x the emulated restatement's distance"""
    _, R, img, ids, w, k = _fixture(name)
    eng, tol = _engine(name, dtype), MEASURED[(name, dtype)]
    T = lambda a: torch.as_tensor(np.asarray(a)).double()
    rel = lambda a, b: float((a.detach().cpu().double() - T(b)).abs().max() / T(b).abs().max())
    queries = eng.prepare_queries(ids)
    out = eng.forward(img.float().cuda(), queries, save=True)
    loss, dl = eng.topk_loss(out["logits"], w, k, eng.gscale)
    rec = {}
    grad = eng.backward(dl, record=rec)
    torch.cuda.synchronize()
    figs = dict(logits=float((out["logits"].cpu().double() - T(R["logits"])).abs().max()), boxes=float((out["boxes"].cpu().double() - T(R["pred_boxes"])).abs().max()),
                loss=abs(float(loss) - float(R["loss"])), grad_hidden=rel(rec["d_hidden"] / eng.gscale, R["grad_hidden"]))
    figs["grad_images"] = rel(grad, R["grad_images"])
    out2 = eng.forward(img.float().cuda(), queries, save=True)
    gsc = O.scores_mean_grad(out2["logits"].cpu().double()).float().cuda() * eng.gscale
    figs["grad_scores"] = rel(eng.backward(gsc), R["grad_scores_images"])
    for key, v in figs.items():
        print(f"[bound] owlvit engine {name} {dtype} {key}: {v:.3e}, gate 2 x {tol[key]:.3e} ({v / (2 * tol[key]):.2f} of it)")
    # the set pmi_owl_topk_loss selected on this run, read off its dlogits: dlogits = -c ([p in S] - k softmax_p), c = 0.01 w_q gscale / (N k)
    x = out["logits"].cpu().double()
    n_, p_, _ = x.shape
    c = (0.01 * w / (n_ * min(k, p_)) * eng.gscale).view(1, 1, -1)
    picked = (dl.cpu().double() - c * min(k, p_) * torch.softmax(x, dim=1)).abs() > c / 2
    assert torch.equal(picked, O.topk_sets(T(R["logits"]), k)), "the top-k set the kernel selected differs from the float64 one"
    assert all(v <= 2 * tol[key] for key, v in figs.items()), figs
    assert float((out["class_embeds"].cpu().double() - T(R["class_embeds"])).abs().max()) <= 2 * tol["logits"]


@pytest.mark.parametrize("dtype", DTYPES)
def test_classes_against_the_reference(dtype):
    """models.OWLViT / losses.OWLViT on fixture (a): loss_and_grad, forward + autograd, scores.mean().backward(), the record"""
    from perceptor_amd import losses, models
    sd, R, img, ids, w, k = _fixture("a")
    tol = MEASURED[("a", dtype)]
    T = lambda a: torch.as_tensor(np.asarray(a)).double()
    rel = lambda a, b: float((a.detach().cpu().double() - T(b)).abs().max() / T(b).abs().max())
    loss = losses.OWLViT(config=tuple(int(c) for c in R["cfg"]), text_config=tuple(int(c) for c in R["text_cfg"]), dtype=dtype)
    loss.model.model.load_state_dict({k_: v.float() for k_, v in sd.items()})
    loss.to("cuda")
    enc = loss.model.encode_texts(ids)
    loss.add_encodings_(enc, weights=w.tolist())
    x = img.float().cuda()
    value, grad = loss.loss_and_grad(x, top_k=k)
    xg = x.clone().requires_grad_(True)
    value2 = loss(xg, top_k=k)
    value2.backward()
    pred = loss.model(xg.detach().requires_grad_(True), enc)
    figs = dict(loss=abs(float(value) - float(R["loss"])), loss_forward=abs(float(value2.detach()) - float(R["loss"])), grad_images=rel(grad, R["grad_images"]),
                grad_autograd=rel(xg.grad, R["grad_images"]))
    x2 = x.clone().requires_grad_(True)
    p2 = loss.model(x2, enc)
    p2.scores.mean().backward()
    figs["grad_scores"] = rel(x2.grad, R["grad_scores_images"])
    gate = dict(loss=tol["loss"], loss_forward=tol["loss"], grad_images=tol["grad_images"], grad_autograd=tol["grad_images"], grad_scores=tol["grad_scores"])
    for key, v in figs.items():
        print(f"[bound] owlvit classes a {dtype} {key}: {v:.3e}, gate 2 x {gate[key]:.3e} ({v / (2 * gate[key]):.2f} of it)")
    assert all(v <= 2 * gate[key] for key, v in figs.items()), figs
    boxes, scores, labels = O.post_process(pred.logits.detach().cpu().double(), T(R["pred_boxes"]), (96, 96))
    assert pred.logits.shape == (2, 9, 3) and not pred.boxes.requires_grad and pred.texts == enc.texts
    assert torch.equal(pred.labels.cpu(), labels) and float((pred.scores.detach().cpu().double() - scores).abs().max()) <= 1e-6
    assert float((pred.boxes.cpu().double() - boxes).abs().max()) <= 2 * 96 * tol["boxes"]


DEFECT_METRIC = {"merge row 1": "logits", "elu no +1": "logits", "shift after scale": "logits", "mean over k": "loss", "box xy swapped": "boxes",
                 "eos last": "logits"}


@pytest.mark.parametrize("dtype", DTYPES)
def test_engine_has_none_of_the_seeded_defects(dtype):
    """the engine at fixture (a) against the float64 restatement WITH each defect: farther than 2 x the gate of section C"""
    sd, R, img, ids, w, k = _fixture("a")
    eng, tol = _engine("a", dtype), MEASURED[("a", dtype)]
    queries = eng.prepare_queries(ids)
    out = eng.forward(img.float().cuda(), queries)
    loss, _ = eng.topk_loss(out["logits"], w, k)
    torch.cuda.synchronize()
    got = dict(logits=out["logits"].cpu().double(), boxes=out["boxes"].cpu().double(), loss=loss.cpu().double())
    m = O.OwlVit(sd, R["cfg"], R["text_cfg"])
    for defect, metric in DEFECT_METRIC.items():
        bad = m.forward(img, ids, defect)
        bad = dict(logits=bad["logits"], boxes=bad["pred_boxes"], loss=O.topk_loss(bad["logits"], w, k, defect)[0])
        dist, gate = float((got[metric] - bad[metric]).abs().max()), 2 * tol[metric]
        print(f"[defect] owlvit engine {dtype} {defect}: {metric} {dist:.3e} from the defective restatement = {dist / gate:.1f} x the gate {gate:.3e}")
        assert dist > 2 * gate, (defect, dist, gate)
    # ---- the query quirk: + 1e-6 on every component
    _, pooled = eng.text.forward(ids, lengths=ids.argmax(dim=1) + 1)
    p64 = pooled.cpu().double()
    unit = p64 / p64.norm(dim=-1, keepdim=True)
    off = queries.cpu().double() - unit
    slack = 4 * U32 * (unit.abs() + 1e-6)                                    # norm, divide, add in fp32
    print(f"[defect] owlvit engine {dtype} query eps: offset in [{float(off.min()):.3e}, {float(off.max()):.3e}], worst {float(((off - 1e-6).abs() / slack).max()):.2f} of its fp32 slack; "
          f"the library's form would be {float((-1e-6 * unit - 1e-6).abs().min() / slack.max()):.1f} x the slack away at the least")
    assert bool(((off - 1e-6).abs() <= slack).all())
    assert float((-1e-6 * unit - 1e-6).abs().min()) > 2 * float(slack.max())


# ---- D. the product configuration -------------------------------------------------------------------------------------------------------------
def test_product_configuration_smoke():
    from perceptor_amd import losses
    _dev()
    loss = losses.OWLViT().to("cuda")
    assert loss.model.size == (768, 768)
    ids = torch.zeros(3, 16, dtype=torch.int64)
    for i, body in enumerate(([320, 1125], [320, 1929, 539, 320, 2368], list(range(1000, 1014)))):
        row = [49406] + body + [49407]
        ids[i, :len(row)] = torch.tensor(row)
    loss.add_encodings_(loss.model.encode_texts(ids), weights=[1.0, 0.5, 2.0])
    x = torch.rand(1, 3, 480, 480, generator=torch.Generator().manual_seed(0)).cuda()
    pred = loss.model(x, loss.encodings)
    value, grad = loss.loss_and_grad(x)
    torch.cuda.synchronize()
    assert pred.logits.shape == (1, 576, 3) and pred.boxes.shape == (1, 576, 4) and pred.scores.shape == (1, 576) and pred.labels.shape == (1, 576)
    assert grad.shape == x.shape and value.ndim == 0
    assert all(bool(torch.isfinite(z).all()) for z in (pred.logits, pred.boxes, pred.scores, value, grad)) and float(grad.abs().max()) > 0
