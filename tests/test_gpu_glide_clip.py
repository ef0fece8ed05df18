"""GPU: models.GlideCLIP -- the fused stem kernels by name, GlideImageEngine block by block and as a whole, GlideTextEngine, the model.

A. pmi_glide_embed_fwd / pmi_glide_embed_bwd at (N, R, P, W, n_timestep) = (3, 16, 4, 128, 8), (2, 8, 4, 768, 8), (1, 64, 4, 256, 1000): one
   row tile with a tail, a width of three channels per thread, and the real 16 x 16 grid (257 rows, 33 workgroups, a one-row tail).
   Outputs sit in NaN-filled buffers with NaN guard bands on both sides.  ts holds 0, the last row and a repeated value; -1 and
   n_timestep must give the clamped rows bit for bit.  Gates (u = 2^-24; derivations in tests/_glide_ref64.py):
     x0 token 0      == fp32(w_t[t] + pos[0]) exactly
     x0 patch rows   |err| <= (3 P^2 + 3) u sum_k |a_k w_jk| + u sum_k |w_jk| 255 |x_k| / s_k + u |x0_j|          (x0_tol)
     x, mean, rstd   float64 LayerNorm of the kernel's OWN x0, at test_layernorm_fwd's gates for the fp32 output, mean and rstd
     dimg            teacher-forced: the float64 LN-vjp, projection and scale of the kernel's own inputs (g, x0, its mean / rstd, w, std,
                     mul), element-wise within the derived bound dimg_tol; with mul = 1 and with g scaled by 65536 and mul = 2^-16 (f16)
     adjoint         <J dx, g> = <dx, J^T g> in float64 with the kernel's dimg as J^T g, J dx evaluated forward (L^T A dx), to within
                     sum |dx| dimg_tol
   Refusals return PMI_ERR_ARG and write nothing: N <= 0, R % P, P <= 0, P != 4, W not a multiple of 64, W > 2048, n_timestep <= 0.
B. GlideImageEngine, bf16 and f16, synthetic weights: tiny (16, 4, 128, 2 blocks, 2 heads) at N = 3; (64, 4, 128, 1 block, 2 heads) at
   N = 1 -- 257 tokens on the attention route the product shape takes; (8, 4, 768, 1 block, 12 heads) at N = 2 -- the product width's
   LayerNorm and MLP routes.  Blocks and head teacher-forced at sqrt(k) u with _vit_ref64's K constants, the whole tower at
   sqrt(depth) u with the two stem roundings removed (_glide_ref64.depth_fwd / depth_grad: derived counts, not measurements); the
   stem inside the engine at the kernel gates above.
C. GlideTextEngine at (12, 64, 128, 2 blocks, 2 heads of 64, 32) with lengths 2, 7 and 12 against the float64 tower.
D. models.GlideCLIP(weights="synthetic"): autograd equals the engine's gradient, two live graphs, a permuted batch (ts permuted along)
   bit for bit, cond_fn within the whole-tower gate of the float64 one, encode_texts behind a three-merge toy tokenizer.

Measured on one MI355X: the [bound] lines this module prints; the table is DESIGN.md section 30.
"""
import functools

import pytest
import torch

import _glide_ref64 as G
import _vit_ref64 as V
import _vit_routes as VR

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f16"]
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
GUARD = 256                     # floats of NaN on either side of an output (a multiple of 4: the interior stays 16-byte aligned)
KERNEL_SHAPES = [(3, 16, 4, 128, 8), (2, 8, 4, 768, 8), (1, 64, 4, 256, 1000)]
ENGINE_ROWS = {"tiny": ((16, 4, 128, 2, 2, 32, 8), 3), "t257": ((64, 4, 128, 1, 2, 32, 1000), 1), "w768": ((8, 4, 768, 1, 12, 64, 8), 2)}


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


class _Guarded:
    """a NaN-filled device buffer with NaN guard bands; .t is the interior view handed to the kernel"""

    def __init__(self, shape, dev):
        n = int(torch.Size(shape).numel())
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(shape)

    def bands_intact(self):
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[-GUARD:]).all())

    def untouched(self):
        return bool(torch.isnan(self.buf).all())


@functools.lru_cache(maxsize=None)
def _kernel_inputs(shape):
    """seeded CPU inputs of one kernel shape, shared and never modified"""
    N, R, P, W, nt = shape
    T = (R // P) ** 2 + 1
    g = torch.Generator().manual_seed(N * 1000 + R * 10 + W)
    r = lambda *s: torch.randn(*s, generator=g)
    img = (r(N, 3, R, R) * 0.25 + 0.5).clamp(0, 1)
    img[0, :, 0, :4] = torch.tensor(G.MEAN).view(3, 1) / 255           # mid-grey pixels: 255 x cancels against the channel mean
    ts = torch.tensor([0, nt - 1, nt - 1][:N]) if N > 1 else torch.tensor([nt - 1])
    return dict(img=img, ts=ts, w=r(W, G.K) * G.K ** -0.5, w_t=r(nt, W) * W ** -0.5, pos=r(T, W) * W ** -0.5, gamma=1 + 0.2 * r(W), beta=0.1 * r(W),
                g=r(N, T, W), dx=r(N, 3, R, R), mean=torch.tensor(G.MEAN), std=torch.tensor(G.STD))


def _fwd(I, shape, ts, dev):
    from perceptor_amd._hip import call, ptr
    N, R, P, W, nt = shape
    T = (R // P) ** 2 + 1
    d = {k: I[k].to(dev) for k in ("img", "mean", "std", "w", "w_t", "pos", "gamma", "beta")}
    tsd = ts.to(dev)
    x0, x, mr = _Guarded((N, T, W), dev), _Guarded((N * T, W), dev), _Guarded((2, N * T), dev)
    call("pmi_glide_embed_fwd", ptr(d["img"]), ptr(d["mean"]), ptr(d["std"]), ptr(d["w"]), ptr(tsd), ptr(d["w_t"]), ptr(d["pos"]), ptr(d["gamma"]),
         ptr(d["beta"]), ptr(x0.t), ptr(x.t), ptr(mr.t), N, R, P, W, nt, 1e-5)
    torch.cuda.synchronize()
    return x0, x, mr, d


def _worst(tag, err, tol):
    ratio = float((err / tol).max())
    print(f"[bound] glide {tag}: worst error {ratio:.3f} of its bound (max abs error {float(err.max()):.3e})")
    return ratio


# ---- A. the kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_glide_embed_fwd(shape):
    """pmi_glide_embed_fwd"""
    N, R, P, W, nt = shape
    T = (R // P) ** 2 + 1
    dev, I = _dev(), _kernel_inputs(shape)
    x0, x, mr, _ = _fwd(I, shape, I["ts"], dev)
    tag = f"embed_fwd {shape}"
    for o in (x0, x, mr):
        assert o.bands_intact() and torch.isfinite(o.t).all(), tag
    got0 = x0.t.cpu()
    # token 0: the timestep row + position 0, the fp32 expression exactly
    assert torch.equal(got0[:, 0], I["w_t"][I["ts"]] + I["pos"][0])
    # patch rows
    a = V.patches((255.0 * I["img"].double() - I["mean"].double().view(1, 3, 1, 1)) / I["std"].double().view(1, 3, 1, 1), P)
    want = a @ I["w"].double().t() + I["pos"][1:].double()
    tol = G.x0_tol(I["img"], I["w"], I["pos"][1:], I["mean"], I["std"], want)
    assert _worst(f"{tag} x0 patch rows", (got0[:, 1:].double() - want).abs(), tol) <= 1.0
    # LayerNorm of the kernel's own x0
    y, mean, rstd, ty, tm, tr = G.ln_fwd_tol(got0.reshape(N * T, W), I["gamma"], I["beta"])
    assert _worst(f"{tag} x", (x.t.cpu().double() - y).abs().amax(-1), ty) <= 1.0
    assert _worst(f"{tag} mean", (mr.t[0].cpu().double() - mean).abs(), tm) <= 1.0
    assert _worst(f"{tag} rstd", (mr.t[1].cpu().double() - rstd).abs(), tr) <= 1.0
    # ts outside the table is clamped: the same bits as the clamped rows
    first0 = I["ts"].clone(); first0[0] = 0
    first_neg = first0.clone(); first_neg[0] = -1
    last_over = I["ts"].clone(); last_over[-1] = nt
    for ts_bad, ts_ok in ((last_over, I["ts"]), (first_neg, first0), (torch.full((N,), -1), torch.zeros(N, dtype=torch.int64)),
                          (torch.full((N,), 2 ** 40), torch.full((N,), nt - 1))):
        b, c = _fwd(I, shape, ts_bad, dev), _fwd(I, shape, ts_ok, dev)
        assert all(torch.equal(p.buf.nan_to_num(7.0), q.buf.nan_to_num(7.0)) for p, q in zip(b[:3], c[:3])), (tag, ts_bad.tolist())


@pytest.mark.parametrize("gscale", [1.0, 65536.0], ids=["mul1", "f16scale"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_glide_embed_bwd(shape, gscale):
    """pmi_glide_embed_bwd, teacher-forced on the forward kernel's own x0 / mean / rstd"""
    from perceptor_amd._hip import call, ptr
    N, R, P, W, nt = shape
    dev, I = _dev(), _kernel_inputs(shape)
    x0, _, mr, d = _fwd(I, shape, I["ts"], dev)
    x0c, mrc = x0.t.contiguous(), mr.t.contiguous()
    g = (I["g"] * gscale).to(dev)
    mul = 1.0 / gscale
    dimg = _Guarded((N, 3, R, R), dev)
    call("pmi_glide_embed_bwd", ptr(g), ptr(x0c), ptr(d["gamma"]), ptr(mrc), ptr(d["w"]), ptr(d["std"]), ptr(dimg.t), N, R, P, W, mul)
    torch.cuda.synchronize()
    tag = f"embed_bwd {shape} mul=1/{gscale:g}"
    assert dimg.bands_intact() and torch.isfinite(dimg.t).all(), tag
    got = dimg.t.cpu().double()
    mean, rstd = mrc[0].cpu().reshape(N, -1), mrc[1].cpu().reshape(N, -1)
    ref, tol = G.dimg_tol(g.cpu(), x0c.cpu(), I["gamma"], mean, rstd, I["w"], I["std"], mul)
    assert float(ref.abs().max()) > 0
    assert _worst(f"{tag} dimg", (got - ref).abs(), tol) <= 1.0
    # adjoint identity, J dx evaluated forward in float64 from the same inputs: J = L^T A
    dx = I["dx"].double()
    A = V.patches(dx * 255.0 / I["std"].double().view(1, 3, 1, 1), P) @ I["w"].double().t()                 # d x0 patch rows
    xh = (x0c.cpu().double()[:, 1:] - mean.double()[:, 1:, None]) * rstd.double()[:, 1:, None]
    Jdx = I["gamma"].double() * rstd.double()[:, 1:, None] * (A - A.mean(-1, keepdim=True) - xh * (xh * A).mean(-1, keepdim=True))
    lhs = float((Jdx * g.cpu().double()[:, 1:]).sum()) * mul
    rhs = float((dx * got).sum())
    slack = float((dx.abs() * tol).sum())
    print(f"[bound] glide {tag} adjoint: <J dx, g> {lhs:.9e}, <dx, J^T g> {rhs:.9e}, difference {abs(lhs - rhs):.2e} of the allowed {slack:.2e}")
    assert abs(lhs - rhs) <= slack


def test_glide_embed_refusals():
    """pmi_glide_embed_fwd / pmi_glide_embed_bwd return PMI_ERR_ARG before any launch"""
    from perceptor_amd import _hip
    from perceptor_amd._hip import ptr
    dev = _dev()
    shape = (3, 16, 4, 128, 8)
    N, R, P, W, nt = shape
    T = (R // P) ** 2 + 1
    I = _kernel_inputs(shape)
    d = {k: I[k].to(dev) for k in ("img", "mean", "std", "w", "w_t", "pos", "gamma", "beta", "g")}
    ts = I["ts"].to(dev)
    lib, s = _hip.lib(), _hip.stream_ptr()
    x0, x, mr, dimg = _Guarded((N, T, W), dev), _Guarded((N * T, W), dev), _Guarded((2, N * T), dev), _Guarded((N, 3, R, R), dev)
    x0in, mrin = torch.zeros(N, T, W, device=dev), torch.ones(2, N * T, device=dev)
    bad = [dict(N=0), dict(N=-1), dict(R=18), dict(P=0), dict(P=-4), dict(P=8), dict(P=2), dict(W=96), dict(W=0), dict(W=2112), dict(nt=0), dict(nt=-3)]
    for kw in bad:
        a = dict(N=N, R=R, P=P, W=W, nt=nt); a.update(kw)
        rc = lib.pmi_glide_embed_fwd(ptr(d["img"]), ptr(d["mean"]), ptr(d["std"]), ptr(d["w"]), ptr(ts), ptr(d["w_t"]), ptr(d["pos"]), ptr(d["gamma"]),
                                     ptr(d["beta"]), ptr(x0.t), ptr(x.t), ptr(mr.t), a["N"], a["R"], a["P"], a["W"], a["nt"], 1e-5, s)
        assert rc == -1, ("fwd", kw, rc)
        if "nt" not in kw:
            rc = lib.pmi_glide_embed_bwd(ptr(d["g"]), ptr(x0in), ptr(d["gamma"]), ptr(mrin), ptr(d["w"]), ptr(d["std"]), ptr(dimg.t),
                                         a["N"], a["R"], a["P"], a["W"], 1.0, s)
            assert rc == -1, ("bwd", kw, rc)
    assert lib.pmi_glide_embed_fwd(None, ptr(d["mean"]), ptr(d["std"]), ptr(d["w"]), ptr(ts), ptr(d["w_t"]), ptr(d["pos"]), ptr(d["gamma"]),
                                   ptr(d["beta"]), ptr(x0.t), ptr(x.t), ptr(mr.t), N, R, P, W, nt, 1e-5, s) == -1
    assert lib.pmi_glide_embed_bwd(ptr(d["g"]), ptr(x0in), ptr(d["gamma"]), ptr(mrin), ptr(d["w"]), ptr(d["std"]), ptr(dimg.t), N, R, P, W, float("nan"), s) == -1
    torch.cuda.synchronize()
    assert all(o.untouched() for o in (x0, x, mr, dimg)), "a refused call wrote to an output"


# ---- B. the engine ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _engine_inputs(name):
    from perceptor_amd.engine import glide
    from perceptor_amd.utils.synth import seeded_noise
    cfg, n = ENGINE_ROWS[name]
    sd = glide.glide_synth_state_dict(glide.glide_image_state_dict_shapes(cfg), 0)
    img = (seeded_noise((n, 3, cfg[0], cfg[0]), 52) * 0.25 + 0.5).clamp(0, 1)
    probe = torch.nn.functional.normalize(seeded_noise((n, cfg[5]), 7))
    ts = torch.tensor([0, cfg[6] - 1, 3][:n])
    return sd, img, probe, ts


@functools.lru_cache(maxsize=None)
def _engine(name, dtype):
    from perceptor_amd.engine.glide import GlideImageEngine
    _dev()
    return GlideImageEngine(ENGINE_ROWS[name][0], _engine_inputs(name)[0], "cuda:0", dtype)


@functools.lru_cache(maxsize=None)
def _reference(name, dtype):
    cfg, n = ENGINE_ROWS[name]
    sd, img, probe, ts = _engine_inputs(name)
    R = VR.host_routes(cfg[:6], n, dtype)
    assert R["flash"]
    ref = G.GlideTower(sd, cfg, emulate=TD[dtype], flash=True, fused_mlp=R["fused_fc"], fused_mlp_bwd=R["fused_pr"]).at(ts)
    return ref, ref.run(img, probe)


def _d_emb(emb, probe, gscale):
    nrm = emb.norm(dim=1, keepdim=True)
    e = emb / nrm
    return ((probe - e * (e * probe).sum(dim=1, keepdim=True)) / nrm * gscale).contiguous()


def _run(eng, img, ts, probe, record=True):
    emb = eng.forward(img.cuda(), ts.cuda(), save=True)
    sv = eng.saved
    d_emb = _d_emb(emb, probe.cuda(), eng.gscale)
    rec = {} if record else None
    grad = eng.backward(d_emb, record=rec) if record else eng.backward(d_emb)
    torch.cuda.synchronize()
    return emb, grad, sv, rec, d_emb


def _unfrag(w, n, heads, t):
    """one of Q, K, V in the attention kernels' row-fragment order [n heads][tp32 / 32][c / 16][(c / 8) & 1][t & 31][c & 7] -> [n, heads, t, 64]"""
    nh, tp32, _ = w.shape
    return w.reshape(nh, tp32 // 32, 4, 2, 32, 8).permute(0, 1, 4, 2, 3, 5).reshape(nh, tp32, 64)[:, :t].reshape(n, heads, t, 64)


def _as_checked(eng, emb, grad, sv, rec, d_emb):
    res, patch, width, layers, heads, out = eng.cfg
    n = sv["n"]
    t = (res // patch) ** 2 + 1
    c = lambda z: z.detach().cpu()
    tok = lambda z: c(z).reshape(n, t, -1)
    Ls = []
    for L in sv["layers"]:
        q, k, v = (_unfrag(c(L["aws"][i]), n, heads, t) for i in range(3))
        Ls.append(dict(x_in=tok(L["x_in"]), x_mid=tok(L["x_mid"]), hpre=tok(L["hpre"]), q=q, k=k, v=v))
    return dict(n=n, gscale=eng.gscale, emb=c(emb), grad=c(grad), d_emb=c(d_emb), x0=c(sv["x0"]), x_final=tok(sv["x_final"]), layers=Ls,
                g32=[c(g) for g in rec["g32"]], gm32=[c(g) for g in rec["gm32"]])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(ENGINE_ROWS))
def test_engine_block_by_block(name, dtype):
    cfg, n = ENGINE_ROWS[name]
    u = V.U[TD[dtype]]
    _, img, probe, ts = _engine_inputs(name)
    eng = _engine(name, dtype)
    assert eng.gscale == VR.GSCALE[dtype] and eng.act == 3 and eng.cls is None
    emb, grad, sv, rec, d_emb = _run(eng, img, ts, probe)
    assert torch.isfinite(emb).all() and torch.isfinite(grad).all() and tuple(grad.shape) == tuple(img.shape)
    assert "g0" not in rec and "dcol" not in rec                          # the fused adjoint makes neither tensor
    emb2, grad2, _, _, _ = _run(eng, img, ts, probe, record=False)
    assert torch.equal(emb, emb2) and torch.equal(grad, grad2), "record= changed an output"
    ref, whole = _reference(name, dtype)
    got = _as_checked(eng, emb, grad, sv, rec, d_emb)
    tag = f"{name} {dtype}"
    worst = (0.0, "")
    bad = []
    for cname, st, k in G.tower_checks(ref, img, probe, got, whole):
        gate = u * k ** 0.5
        print(f"[bound] glide {tag} {cname}: {st:.3e} = {st / u:.3f} u, gate sqrt({k}) u = {gate:.3e} ({st / gate:.2f} of it)")
        worst = max(worst, (st / gate, cname))
        if not st <= gate:
            bad.append((cname, st / u, k))
    for cname, ratio in G.stem_ratios(ref, img, got, mean_rstd=sv["mr_pre"].cpu()):
        print(f"[bound] glide {tag} {cname}: {ratio:.3f} of its fp32 bound")
        if not ratio <= 1.0:
            bad.append((cname, ratio, "fp32 bound"))
    print(f"[bound] glide {tag} worst 16-bit check: {worst[0]:.2f} of its gate ({worst[1]})")
    assert not bad, (tag, bad)


def test_engine_errors():
    eng = _engine("tiny", "bf16")
    _, img, probe, ts = _engine_inputs("tiny")
    with pytest.raises(ValueError, match="16 x 16"):
        eng.forward(torch.zeros(3, 3, 32, 32, device="cuda"), ts.cuda())
    with pytest.raises(ValueError):
        eng.forward(img.cuda(), ts[:2].cuda())
    with pytest.raises(ValueError):
        eng.forward(img.cuda(), ts.int().cuda())
    _run(eng, img, ts, probe, record=False)
    with pytest.raises(RuntimeError, match="forward"):
        eng.backward(torch.zeros(3, 32, device="cuda"))


# ---- C. the text engine -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_text_engine_pools_at_lengths(dtype):
    from perceptor_amd.engine import glide
    _dev()
    cfg = (12, 64, 128, 2, 2, 32)
    u = V.U[TD[dtype]]
    sd = glide.glide_synth_state_dict(glide.glide_text_state_dict_shapes(cfg), 0)
    lengths = torch.tensor([2, 7, 12])
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, 62, (3, 12), generator=g)
    ids[:, 0] = 62
    for i, ln in enumerate(lengths.tolist()):
        ids[i, ln - 1] = 63
        ids[i, ln:] = 0
    ids[1, 3] = 63                                                        # the largest id earlier than the end: argmax pooling would take row 3
    eng = glide.GlideTextEngine(cfg, sd, "cuda:0", dtype)
    hidden, pooled = eng.forward(ids, lengths=lengths)
    _, pooled_argmax = eng.forward(ids)
    torch.cuda.synchronize()
    ref = G.GlideText(sd, cfg, emulate=TD[dtype])
    want, want_hidden = ref.forward(ids, lengths)
    st, gate = V.row_stat(pooled.cpu(), want), u * G.depth_text(cfg[3]) ** 0.5
    sh = V.row_stat(hidden.cpu(), want_hidden)
    print(f"[bound] glide text {dtype}: pooled {st:.3e} = {st / u:.3f} u, hidden {sh / u:.3f} u, gate sqrt({G.depth_text(cfg[3])}) u = {gate:.3e}")
    assert torch.isfinite(pooled).all() and st <= gate and sh <= gate
    assert torch.equal(pooled_argmax[0], pooled[0]) and torch.equal(pooled_argmax[2], pooled[2]) and not torch.equal(pooled_argmax[1], pooled[1])
    for bad in (torch.tensor([0, 7, 12]), torch.tensor([2, 7, 13]), torch.tensor([2, 7]), torch.tensor([2.0, 7.0, 12.0])):
        with pytest.raises(ValueError):
            eng.forward(ids, lengths=bad)


# ---- D. the model -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(dtype):
    from perceptor_amd import models
    _dev()
    return models.GlideCLIP("synthetic", config=ENGINE_ROWS["tiny"][0], text_config=(12, 520, 128, 2, 2, 32),
                            precision="fp16" if dtype == "f16" else "bf16").to("cuda")


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_autograd_is_the_engines_gradient(dtype):
    model = _model(dtype)
    _, img, probe, ts = _engine_inputs("tiny")
    eng = model.engine
    emb, grad, _, _, _ = _run(eng, img, ts, probe, record=False)

    def grad_of(first, first_ts, then=None, pr=probe):
        a = first.cuda().requires_grad_(True)
        with torch.enable_grad():
            ea = model.encode_images(a, first_ts)
            if then is not None:
                eb = model.encode_images(then.cuda().requires_grad_(True), ts[:then.shape[0]])      # a second live graph, never run backward
            (ea * pr[:a.shape[0]].cuda()).sum().backward()
        return ea.detach(), a.grad

    unit, alone = grad_of(img, ts)
    assert torch.equal(alone, grad), "autograd through encode_images is not the engine's gradient"
    assert torch.allclose(unit.norm(dim=1), torch.ones(3, device="cuda"), atol=1e-5)
    assert torch.equal(unit, model.encode_images(img.cuda(), ts))        # the no-grad path: the same bits; a CPU ts is moved, not refused
    # two live graphs
    assert torch.equal(grad_of(img, ts, then=img[:1])[1], alone)
    assert torch.equal(grad_of(img[:2], ts[:2], then=img)[1], grad_of(img[:2], ts[:2])[1])
    with pytest.raises(RuntimeError, match="forward"):
        eng.backward(torch.zeros(3, 32, device="cuda"))
    # a permuted batch, ts permuted along
    perm = torch.tensor([2, 0, 1])
    unit_p, grad_p = grad_of(img[perm], ts[perm], pr=probe[perm])
    assert torch.equal(unit_p, unit[perm.cuda()]) and torch.equal(grad_p, alone[perm.cuda()])
    with pytest.raises(ValueError, match="out of range"):
        model.encode_images(img.cuda(), torch.tensor([0, 8, 1]))
    with pytest.raises(NotImplementedError):
        model(img)


@pytest.mark.parametrize("dtype", DTYPES)
def test_model_cond_fn_and_texts(dtype):
    from perceptor_amd.utils.tokenizer import ClipTokenizer
    model = _model(dtype)
    cfg = ENGINE_ROWS["tiny"][0]
    u = V.U[TD[dtype]]
    _, img, _, ts = _engine_inputs("tiny")
    prompts = ["abc", "cab abc", "b"]
    model.tokenize(prompts, tokenizer=ClipTokenizer(merges=[("a", "b"), ("ab", "c</w>"), ("c", "a")]))
    z_t = model.encode_texts(prompts)
    ids, lengths = model.tokenize(prompts)
    assert lengths.tolist() == [3, 5, 3] and tuple(z_t.shape) == (3, 32) and torch.allclose(z_t.norm(dim=1), torch.ones(3, device="cuda"), atol=1e-5)
    want_t, _ = G.GlideText({k[len("model.text_encoder."):]: v.cpu() for k, v in model.state_dict().items() if k.startswith("model.text_encoder.")},
                            model.text_cfg, emulate=TD[dtype]).forward(ids, lengths)
    st = V.row_stat(z_t.cpu(), torch.nn.functional.normalize(want_t))
    gate_t = u * G.depth_text(2) ** 0.5
    print(f"[bound] glide model {dtype} encode_texts: {st:.3e} = {st / u:.3f} u, gate {gate_t:.3e}")
    assert st <= gate_t
    x = img * 2 - 1
    got = model.cond_fn(prompts, 3.0)(x.cuda(), ts.cuda())
    torch.cuda.synchronize()
    ref, _ = _reference("tiny", dtype)
    want = G.cond_fn_grad(ref, x, z_t.cpu().double(), model.logit_scale, 3.0)
    rel, gate = V.rel_l2(got.cpu(), want), u * G.depth_grad(cfg[3], True) ** 0.5
    print(f"[bound] glide model {dtype} cond_fn: grad rel-L2 {rel:.3e} = {rel / u:.3f} u, gate sqrt({G.depth_grad(cfg[3], True)}) u = {gate:.3e}")
    assert torch.isfinite(got).all() and tuple(got.shape) == tuple(x.shape) and float(got.abs().max()) > 0
    assert rel <= gate
    assert torch.equal(model.cond_fn(prompts, 6.0)(x.cuda(), ts.cuda()), got * 2)      # grad_scale is a plain factor (a power of two: exact)
