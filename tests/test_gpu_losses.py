"""GPU: the guidance-loss kernels of csrc/losses.hip (pmi_head_loss, pmi_smoothness, pmi_sqdiff_loss) against the float64 restatements
and bounds of tests/_losses_ref64.py, the five loss classes on tiny towers and against the reference's own values
(tests/golden/losses_reference.npz), losses.tower_loss_and_grad (one tower pass for several losses) and a 577-token ViT tower.

Every comparison prints its worst |got - ref| / bound before it asserts.  The case lists are module constants:
tests/test_losses_cpu.py runs the bounds and the seeded defects at exactly these inputs.
"""
import itertools

import pytest
import torch
import torch.nn.functional as F

import _losses_ref64 as R
from conftest import golden

pytestmark = pytest.mark.gpu

HEAD_N, HEAD_D = (1, 3, 8), (64, 512, 640, 1024)
HEAD_TARGETS, HEAD_GSCALES = (1, 5, 10), (1.0, 65536.0)
HEAD_MULT = {0: 0.001, 1: 1.7, 2: 1.7, 3: 1.7}
SMOOTH_CASES = [((2, 3, 5, 7), 2), ((1, 1, 2, 2), 1), ((2, 2, 5, 8), 2), ((2, 3, 64, 130), 5), ((1, 3, 512, 512), 1)]   # (shape, n_total)
SQDIFF_COUNTS = (1, 255, 4097, 3 * 224 * 224)
VIT_TINY = (32, 8, 128, 2, 2, 64)
RN_TINY = (64, (1, 1, 1, 1), 16, 8, 64)            # the smallest tower of tests/test_gpu_rn_clip.py
VIT_577 = (192, 8, 128, 2, 2, 64)                  # 24 x 24 patches + the class token


def head_cases(mode, N, D):
    """(inputs, [(target, n_total, gscale)]) of one (mode, N, D) case"""
    K = 1 if mode == 0 else 10
    return R.head_inputs(N, D, K, 1000 * mode + 10 * N + D), list(itertools.product(HEAD_TARGETS, (N, 2 * N + 1), HEAD_GSCALES))


def _report(tag, got, ref, tol):
    w = R.worst(got, ref, tol)
    print(f"[bound] {tag}: worst |got - ref| / bound = {w:.3e}")
    return w <= 1.0


def _lib_call(name, *args):
    from perceptor_amd._hip import call
    call(name, *args)
    torch.cuda.synchronize()


# ================================================ pmi_head_loss ============================================================================
SENTINEL = -12345.5


def _head_run(emb, W, b, mode, target, n_total, mult, gscale, extra_rows=2):
    from perceptor_amd._hip import ptr
    N, D = emb.shape
    K = W.shape[0]
    dev = "cuda"
    e, w, bb = emb.to(dev), W.to(dev), b.to(dev)
    loss = torch.full((1,), float("nan"), device=dev)
    demb = torch.full((N + extra_rows, D), SENTINEL, device=dev)
    out = torch.full((N + extra_rows, K), SENTINEL, device=dev)
    partial = torch.full((N,), float("nan"), device=dev)
    _lib_call("pmi_head_loss", ptr(e), ptr(w), ptr(bb), ptr(loss), ptr(demb), ptr(out), ptr(partial), N, K, D, mode, float(target),
              n_total, mult, gscale)
    return loss.cpu(), demb.cpu(), out.cpu()


@pytest.mark.parametrize("D", HEAD_D)
@pytest.mark.parametrize("N", HEAD_N)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_head_loss_vs_float64(mode, N, D):
    """pmi_head_loss: loss, demb and out within the float64 bounds at every (target, n_total, gscale); two runs bit-equal; rows beyond N of
    a larger demb / out buffer keep their sentinel."""
    (emb, W, b), combos = head_cases(mode, N, D)
    mult = HEAD_MULT[mode]
    ok = True
    for target, n_total, gscale in combos:
        loss, demb, out = _head_run(emb, W, b, mode, target, n_total, mult, gscale)
        loss2, demb2, out2 = _head_run(emb, W, b, mode, target, n_total, mult, gscale)
        assert torch.equal(loss, loss2) and torch.equal(demb, demb2) and torch.equal(out, out2), "two runs differ"
        assert bool((demb[N:] == SENTINEL).all()) and bool((out[N:] == SENTINEL).all()), "rows beyond N were written"
        o64, l64, d64 = R.head_eval(emb, W, b, mode, target, n_total, mult, gscale)
        o_tol, l_tol, d_tol = R.head_tol(emb, W, b, mode, target, n_total, mult, gscale)
        tag = f"head_loss {R.MODE_NAMES[mode]} N={N} D={D} target={target} n_total={n_total} gscale={gscale:g}"
        ok &= _report(tag + " out", out[:N], o64, o_tol)
        ok &= _report(tag + " loss", loss, l64.reshape(1), l_tol)
        ok &= _report(tag + " demb", demb[:N], d64, d_tol)
    assert ok


def test_head_loss_argument_guards():
    from perceptor_amd._hip import lib, ptr
    t = torch.zeros(64, device="cuda")
    p = ptr(t)
    f = lib().pmi_head_loss
    assert f(p, p, p, p, p, p, p, 1, 17, 64, 1, 1.0, 1, 1.0, 1.0, None) == -1      # K > 16
    assert f(p, p, p, p, p, p, p, 1, 10, 4097, 1, 1.0, 1, 1.0, 1.0, None) == -1    # D > 4096
    assert f(p, p, p, p, p, p, p, 1, 10, 64, 1, 11.0, 1, 1.0, 1.0, None) == -1     # class 11 of 10
    assert f(p, p, p, p, p, p, p, 1, 10, 64, 0, 5.0, 1, 1.0, 1.0, None) == -1      # mode 0 is a K = 1 probe
    assert f(p, p, p, p, p, p, p, 2, 1, 64, 0, 5.0, 1, 1.0, 1.0, None) == -1       # n_total < N
    torch.cuda.synchronize()
    assert bool((t == 0).all())


# ================================================ pmi_smoothness ===========================================================================
def _smooth_run(x, n_total, gscale):
    from perceptor_amd._hip import ptr
    N, C, H, W = x.shape
    xd = x.cuda()
    loss = torch.full((1,), float("nan"), device="cuda")
    grad = torch.full_like(xd, float("nan"))
    partial = torch.full((2048,), float("nan"), device="cuda")
    _lib_call("pmi_smoothness", ptr(xd), ptr(loss), ptr(grad), ptr(partial), N, C, H, W, n_total, gscale)
    return loss.cpu(), grad.cpu()


@pytest.mark.parametrize("case", SMOOTH_CASES, ids=str)
def test_smoothness_vs_float64(case):
    shape, n_total = case
    x = R.smoothness_input(shape, sum(shape))
    ok = True
    for gscale in (1.0, 65536.0):
        loss, grad = _smooth_run(x, n_total, gscale)
        loss2, grad2 = _smooth_run(x, n_total, gscale)
        assert torch.equal(loss, loss2) and torch.equal(grad, grad2), "two runs differ"
        l64, g64, _ = R.smoothness_eval(x, n_total, gscale)
        l_tol, g_tol = R.smoothness_tol(x, n_total, gscale)
        ok &= _report(f"smoothness {shape} n_total={n_total} gscale={gscale:g} loss", loss, l64.reshape(1), l_tol)
        ok &= _report(f"smoothness {shape} n_total={n_total} gscale={gscale:g} grad", grad, g64, g_tol)
    assert ok


def test_smoothness_single_row_is_an_error():
    """(1, 3, 1, 8): the reference's mean over an empty difference is NaN; pmi_smoothness returns an error code without a launch"""
    from perceptor_amd._hip import lib, ptr
    x = torch.ones(1, 3, 1, 8, device="cuda")
    loss, grad, partial = torch.full((1,), 7.0, device="cuda"), torch.full_like(x, 7.0), torch.zeros(2048, device="cuda")
    assert lib().pmi_smoothness(ptr(x), ptr(loss), ptr(grad), ptr(partial), 1, 3, 1, 8, 1, 1.0, None) == -1
    assert lib().pmi_smoothness(ptr(x), ptr(loss), ptr(grad), ptr(partial), 1, 3, 8, 1, 1, 1.0, None) == -1
    torch.cuda.synchronize()
    assert float(loss) == 7.0 and bool((grad == 7.0).all())


# ================================================ pmi_sqdiff_loss ==========================================================================
def _sqdiff_run(a, b, n_total_count, offset=0):
    """offset: elements by which the device tensors are shifted off their 16-byte alignment (the element-by-element route)"""
    from perceptor_amd._hip import ptr
    count = a.numel()
    pad = lambda t: torch.cat([torch.zeros(offset), t]).cuda()[offset:]
    ad, bd = pad(a), pad(b)
    g = torch.full((count + offset,), float("nan"), device="cuda")[offset:]
    loss = torch.full((1,), float("nan"), device="cuda")
    partial = torch.full((1024,), float("nan"), device="cuda")
    _lib_call("pmi_sqdiff_loss", ptr(ad), ptr(bd), ptr(loss), ptr(g), ptr(partial), count, n_total_count)
    return loss.cpu(), g.cpu()


@pytest.mark.parametrize("count", SQDIFF_COUNTS)
def test_sqdiff_loss_vs_float64(count):
    a, b = R.sqdiff_inputs(count, count)
    ok = True
    for n_total_count, offset in ((count, 0), (3 * count, 0), (count, 1)):
        loss, g = _sqdiff_run(a, b, n_total_count, offset)
        loss2, g2 = _sqdiff_run(a, b, n_total_count, offset)
        assert torch.equal(loss, loss2) and torch.equal(g, g2), "two runs differ"
        l64, g64, _ = R.sqdiff_eval(a, b, n_total_count)
        l_tol, g_tol = R.sqdiff_tol(a, b, n_total_count)
        ok &= _report(f"sqdiff count={count} n_total_count={n_total_count} offset={offset} loss", loss, l64.reshape(1), l_tol)
        ok &= _report(f"sqdiff count={count} n_total_count={n_total_count} offset={offset} g", g, g64, g_tol)
    assert ok


# ================================================ classes ==================================================================================
@pytest.fixture(scope="module")
def towers():
    from perceptor_amd import models
    return {"vit": models.OpenCLIP("losses-tiny", "synthetic", quick_gelu=True, config=VIT_TINY).to("cuda"),
            "rn": models.OpenCLIP("rn-losses-tiny", "synthetic", rn_config=RN_TINY).to("cuda")}


class _Recorder:
    """wraps engine.forward / engine.backward: counts the calls, keeps the embedding that left and the dL/d emb that entered"""

    def __init__(self, eng):
        self.eng, self.emb, self.demb = eng, [], []
        self._f, self._b = eng.forward, eng.backward
        eng.forward, eng.backward = self.forward, self.backward

    def forward(self, *a, **k):
        out = self._f(*a, **k)
        self.emb.append((out[0] if isinstance(out, tuple) else out).detach().clone())
        return out

    def backward(self, d):
        self.demb.append(d.detach().clone())
        return self._b(d)

    def close(self):
        del self.eng.forward, self.eng.backward


def _term(kind, tower):
    from perceptor_amd import losses
    if kind == "simulacra":
        return losses.SimulacraAesthetic("losses-tiny", 7, model=tower, seed=3).to("cuda")
    return losses.AestheticVisualAssessment(4, kind, model=tower, seed=3).to("cuda")


@pytest.mark.parametrize("kind", ["simulacra", "logit", "expected", "probability"])
@pytest.mark.parametrize("tower", ["vit", "rn"])
def test_head_classes_forward_backward_equals_loss_and_grad(towers, tower, kind):
    """forward(images).backward() (the tower's autograd function + torch on [N, D]) and loss_and_grad(images) (pmi_head_loss) differ only in
    fp32 head arithmetic: both losses, and both dL/d emb as they enter the same engine.backward, sit within the head bounds of the float64
    evaluation at the tower's embedding.  (No bound is derived for pixels: the tower backward is linear in dL/d emb but rounds it to 16 bits.)"""
    from perceptor_amd.utils.synth import seeded_noise
    term = _term(kind, towers[tower])
    eng = term.model._need_engine()
    img = (seeded_noise((3, 3, 40, 56), 31) * 0.25 + 0.5).cuda()
    rec = _Recorder(eng)
    try:
        l_fused, g_fused = term.loss_and_grad(img)
        x = img.clone().requires_grad_(True)
        with torch.enable_grad():
            l_auto = term(x)
            l_auto.backward()
    finally:
        rec.close()
    assert len(rec.emb) == 2 and len(rec.demb) == 2 and torch.equal(rec.emb[0], rec.emb[1])
    assert g_fused.shape == img.shape and x.grad.shape == img.shape and bool(torch.isfinite(x.grad).all())
    lin, mode, target = term._head()
    args = (rec.emb[0].cpu(), lin.weight.detach().cpu(), lin.bias.detach().cpu(), mode, target, 3, term.multiplier, eng.gscale)
    _, l64, d64 = R.head_eval(*args)
    _, l_tol, d_tol = R.head_tol(*args)
    tag = f"{type(term).__name__} {kind} on {tower}"
    ok = _report(tag + " loss_and_grad loss", l_fused.cpu().reshape(1), l64.reshape(1), l_tol)
    ok &= _report(tag + " forward loss", l_auto.detach().cpu().reshape(1), l64.reshape(1), l_tol)
    ok &= _report(tag + " loss_and_grad demb", rec.demb[0].cpu(), d64, d_tol)
    ok &= _report(tag + " forward/backward demb", rec.demb[1].cpu(), d64, d_tol)
    assert ok
    if kind == "simulacra":     # models.SimulacraAesthetic.forward returns the [N, 1] ratings
        r = term.aesthetic_model(img)
        o64, _, _ = R.head_eval(*args)
        assert r.shape == (3, 1) and _report(tag + " ratings", r.cpu(), o64, R.head_tol(*args)[0])


def test_smoothness_and_resize_classes_match_the_reference_values():
    from perceptor_amd import losses
    g = golden("losses_reference")
    ok = True
    # Smoothness: forward + backward, and the fused call
    x = g["smooth_x"].float()
    assert torch.equal(x.double(), g["smooth_x"])               # the fixture's inputs are fp32 values stored as float64
    l_tol, g_tol = R.smoothness_tol(x, x.shape[0], 1.0)
    xd = x.cuda().requires_grad_(True)
    with torch.enable_grad():
        loss = losses.Smoothness()(xd)
        loss.backward()
    lf, gf = losses.Smoothness().loss_and_grad(x.cuda())
    ok &= _report("Smoothness forward loss", loss.detach().cpu().reshape(1), g["smooth_loss"], l_tol)
    ok &= _report("Smoothness backward grad", xd.grad.cpu(), g["smooth_grad"], g_tol)
    ok &= _report("Smoothness loss_and_grad loss", lf.cpu().reshape(1), g["smooth_loss"], l_tol)
    ok &= _report("Smoothness loss_and_grad grad", gf.cpu(), g["smooth_grad"], g_tol)
    # Resize: both arguments' gradients, against the reference's own values
    a, b, size = g["resize_a"].float(), g["resize_b"].float(), tuple(int(v) for v in g["resize_size"])
    l_tol, ga_tol, gb_tol = R.resize_loss_tol(a, b, size)
    assert torch.equal(a.double(), g["resize_a"]) and torch.equal(b.double(), g["resize_b"])
    ad, bd = a.cuda().requires_grad_(True), b.cuda().requires_grad_(True)
    with torch.enable_grad():
        loss = losses.Resize()(ad, bd, size)
        loss.backward()
    lf, gaf = losses.Resize(size).loss_and_grad(a.cuda(), b.cuda())
    ok &= _report("Resize forward loss", loss.detach().cpu().reshape(1), g["resize_loss"], l_tol)
    ok &= _report("Resize backward grad a", ad.grad.cpu(), g["resize_grad_a"], ga_tol)
    ok &= _report("Resize backward grad b", bd.grad.cpu(), g["resize_grad_b"], gb_tol)
    ok &= _report("Resize loss_and_grad loss", lf.cpu().reshape(1), g["resize_loss"], l_tol)
    ok &= _report("Resize loss_and_grad grad a", gaf.cpu(), g["resize_grad_a"], ga_tol)
    assert ok


class _StubTower(torch.nn.Module):
    """encode_images returns F.normalize of what it is given: the fixture's "images" are embeddings"""

    def encode_images(self, images):
        return F.normalize(images)


def test_spherical_distance_matches_the_reference_values_through_stub_embeddings():
    """losses.SphericalDistance.forward on the fixture's stub tower (differentiated to both arguments), and the fused path's arithmetic
    (pmi_spherical_loss with the second batch as unit-weight targets) on the same embeddings, against the reference's own values with the
    bounds tests/test_gpu_transformer_kernels.py::test_spherical_loss applies to that kernel."""
    import test_gpu_transformer_kernels as TK
    from perceptor_amd import losses
    from perceptor_amd._hip import ptr
    g = golden("losses_reference")
    ea, eb = g["sph_a"].float(), g["sph_b"].float()
    assert torch.equal(ea.double(), g["sph_a"]) and torch.equal(eb.double(), g["sph_b"])
    l_tol = 64 * TK.E32 * (abs(float(g["sph_loss"])) + 1.0)
    tol = lambda ref: 256 * TK.E32 * float(ref.abs().max()) + 2.0 ** -30
    a, b = ea.cuda().requires_grad_(True), eb.cuda().requires_grad_(True)
    with torch.enable_grad():
        loss = losses.SphericalDistance(_StubTower())(a, b)
        loss.backward()
    ok = _report("SphericalDistance forward loss", loss.detach().cpu().reshape(1), g["sph_loss"], l_tol)
    ok &= _report("SphericalDistance grad a", a.grad.cpu(), g["sph_grad_a"], tol(g["sph_grad_a"]))
    ok &= _report("SphericalDistance grad b", b.grad.cpu(), g["sph_grad_b"], tol(g["sph_grad_b"]))
    # the fused path: targets = normalised second batch, unit weights, mean over N x K
    tgt, wts = F.normalize(eb).cuda(), torch.ones(eb.shape[0], device="cuda")
    lk, dk = torch.empty(1, device="cuda"), torch.empty_like(a.detach())
    _lib_call("pmi_spherical_loss", ptr(a.detach()), ptr(tgt), ptr(wts), ptr(lk), ptr(dk), ea.shape[0], eb.shape[0], ea.shape[1], ea.shape[0], 1.0, 1.0)
    ok &= _report("SphericalDistance fused loss", lk.cpu(), g["sph_loss"], l_tol)
    ok &= _report("SphericalDistance fused grad a", dk.cpu(), g["sph_grad_a"], tol(g["sph_grad_a"]))
    assert ok


def test_spherical_distance_on_a_tower(towers):
    """the class on a real tower: forward differentiates to both image batches; loss_and_grad returns the same loss and gradient to the first
    batch up to the head arithmetic (compared as dL/d emb entering engine.backward, as above)"""
    from perceptor_amd import losses
    from perceptor_amd.utils.synth import seeded_noise
    import test_gpu_transformer_kernels as TK
    model = towers["vit"]
    sd = losses.SphericalDistance(model)
    ia, ib = (seeded_noise((2, 3, 32, 32), 41) * 0.25 + 0.5).cuda(), (seeded_noise((3, 3, 48, 40), 42) * 0.25 + 0.5).cuda()
    rec = _Recorder(model._need_engine())
    try:
        lf, gf = sd.loss_and_grad(ia, ib)
        a, b = ia.clone().requires_grad_(True), ib.clone().requires_grad_(True)
        with torch.enable_grad():
            la = sd(a, b)
            la.backward()
    finally:
        rec.close()
    assert a.grad.shape == ia.shape and b.grad.shape == ib.shape and float(b.grad.abs().max()) > 0 and gf.shape == ia.shape
    # calls: fused = forward(b), forward(a), backward(a); autograd = forward(a), forward(b), backward(b), backward(a)
    assert len(rec.emb) == 4 and len(rec.demb) == 3
    ea, eb = rec.emb[1].cpu(), rec.emb[0].cpu()
    e = ea.double().requires_grad_(True)
    with torch.enable_grad():
        l64 = (F.normalize(e)[:, None] - F.normalize(eb.double())[None]).norm(dim=2).div(2).arcsin().square().mul(2).mean()
        (d64,) = torch.autograd.grad(l64, e)
    l64, d64 = l64.detach(), d64 * model.engine.gscale
    l_tol = 64 * TK.E32 * (abs(float(l64)) + 1.0)
    d_tol = 256 * TK.E32 * float(d64.abs().max()) + 2.0 ** -30 * model.engine.gscale
    ok = _report("SphericalDistance tower fused loss", lf.cpu().reshape(1), l64.reshape(1), l_tol)
    ok &= _report("SphericalDistance tower forward loss", la.detach().cpu().reshape(1), l64.reshape(1), l_tol)
    ok &= _report("SphericalDistance tower fused demb a", rec.demb[0].cpu(), d64, d_tol)
    ok &= _report("SphericalDistance tower autograd demb a", rec.demb[2].cpu(), d64, d_tol)
    assert ok


# ================================================ one tower pass for several losses ========================================================
def test_tower_loss_and_grad_shares_one_pass():
    from perceptor_amd import losses
    from perceptor_amd.utils.synth import seeded_noise
    clip = losses.CLIP("losses-tiny-shared", "bf16", weights="synthetic", quick_gelu=True, config=VIT_TINY).to("cuda")
    clip.add_encodings_(F.normalize(seeded_noise((2, VIT_TINY[5]), 7)), [1.0, 0.5])
    sim = losses.SimulacraAesthetic("losses-tiny-shared", 7, model=clip.model, seed=3).to("cuda")
    assert sim.model is clip.model
    eng = clip.model._need_engine()
    img = (seeded_noise((3, 3, 40, 56), 33) * 0.25 + 0.5).cuda()
    la, _ = clip.loss_and_grad(img)
    ls, _ = sim.loss_and_grad(img)
    rec = _Recorder(eng)
    try:
        total, grad, per = losses.tower_loss_and_grad(img, [clip, sim])
    finally:
        rec.close()
    assert len(rec.emb) == 1 and len(rec.demb) == 1, "tower_loss_and_grad ran the tower more than once"
    assert len(per) == 2 and torch.equal(per[0], la) and torch.equal(per[1], ls)
    assert torch.equal(total, la + ls)
    # the tower backward is linear in dL/d emb: by hand from the two terms
    emb = eng.forward(img, save=True).contiguous()
    assert torch.equal(emb, rec.emb[0])
    _, da = clip._embedding_loss_and_grad(emb, None)
    _, db = sim._embedding_loss_and_grad(emb, None)
    assert torch.equal(rec.demb[0], da + db)
    assert torch.equal(grad, eng.backward(da + db))
    other = losses.SimulacraAesthetic("losses-tiny-other", 7, weights="synthetic", quick_gelu=True, config=VIT_TINY).to("cuda")
    with pytest.raises(ValueError):
        losses.tower_loss_and_grad(img, [clip, other])


# ================================================ a 577-token tower ========================================================================
def _embedding_bound_of_test_gpu_clip():
    """the embedding rel-L2 bound tests/test_gpu_clip.py asserts for its tiny towers, read from that test so that no copy can drift"""
    import inspect
    import re
    import test_gpu_clip as TC
    m = re.search(r"assert e_rel <= ([0-9.e+-]+) and en_rel", inspect.getsource(TC.test_vit_embedding_and_gradient_vs_reference_golden))
    assert m, "tests/test_gpu_clip.py no longer states its embedding bound in this form"
    return float(m.group(1))


def test_vit_577_tokens_vs_oracle():
    """(192, 8, ...): 24 x 24 patches + class token = 577 tokens, the token count of ViT-L-14-336, through the fused attention kernels
    (pmi_vit_attn_fwd / pmi_vit_attn_bwd, head dim 64).  Loss, image gradient (rel-L2 and cosine), a sharded call and forward().backward()
    are held to oracle.clip_vit by tests/test_gpu_clip.py's own test of its tiny towers, run on this tower; the embedding by the bound that
    file asserts for them.  No tolerance is written here."""
    from oracle import clip_vit
    from perceptor_amd import models
    from perceptor_amd.engine import vit
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    import test_gpu_clip as TC
    assert vit.VIT_CONFIGS["ViT-L-14-336"] == (336, 14, 1024, 24, 16, 768) and (336 // 14) ** 2 + 1 == 577 == (VIT_577[0] // VIT_577[1]) ** 2 + 1
    tag = "losses-577"
    assert tag not in TC.TINY
    TC.TINY[tag] = VIT_577
    try:
        TC.test_loss_and_grad_vs_oracle_and_sharding(tag, False)
    finally:
        del TC.TINY[tag]
    model = models.OpenCLIP(tag, "synthetic", quick_gelu=True, config=VIT_577).to("cuda")
    img = seeded_noise((2, 3, 200, 184), 9) * 0.25 + 0.5
    emb = model.encode_images(img.cuda(), normalize=False)
    e_ref = clip_vit.encode_images(synth_state_dict(clip_vit.vit_state_dict_shapes(VIT_577), 0), VIT_577, img, True, normalize=False)
    e_rel, bound = TC._rel(emb.cpu(), e_ref), _embedding_bound_of_test_gpu_clip()
    print(f"[parity] 577-token tower: emb rel-L2={e_rel:.3e} (bound {bound:g})")
    assert e_rel <= bound
