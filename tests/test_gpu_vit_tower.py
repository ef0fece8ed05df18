"""GPU: the CLIP ViT tower (engine/vit.py) block by block against the float64 emulated tower of tests/_vit_ref64.py, at the rows of
tests/_vit_routes.py -- 2-layer towers (one layer at t = 257) chosen so that every route of the engine runs: flash and batched-GEMM
attention (d = 64 / 80 / 96, tp > t), fused and unfused MLP epilogues, split-K slabs into pmi_layernorm_fwd_slabs / _bwd_slabs, padded
im2col rows, m < 64 -- in bf16 AND f16 (gscale = 65536, 1 / gscale in pmi_unpatchify).

Inputs: seeded_noise * 0.25 + 0.5 images at the tower's resolution, synth_state_dict weights, a unit probe on the normalised embedding.
u = 2^-8 (bf16), 2^-11 (f16).  A per-row statistic is max over rows of |got - ref|_2 / max(|ref|_2, rms over rows of |ref|_2).

Block by block, teacher-forced (_vit_ref64.tower_checks): every piece of the float64 tower is fed the ENGINE's own fp32 input of that piece
(eng.saved after forward(save=True); the gradients VitEngine.backward(record=) keeps), so each statistic holds the roundings of one piece
and is gated at sqrt(k) u, k the 16-bit roundings inside the piece (the K_* constants of _vit_ref64.py, counted from engine/vit.py):
  forward   stem x0 (1), per block the stored q / k / v (2), x_mid - x_in (4), the stored hpre (2), x_out - x_mid (3), emb from x_final (1)
  backward  g32 after the head (1), per block gm32 - g32_in (3) and g32_out - gm32 (5; 6 on the flash route), g0, dcol and the image
            gradient per 3 p p patch from the first block's g32 (1); all on grad / gscale
Whole tower: embedding and image gradient (every pixel) rel-L2 <= sqrt(depth) u against the emulated tower's own run, depth = 16 / 34 or
36 roundings for two layers (_vit_ref64.depth_fwd / depth_grad), the gradient also per patch; and the gradient under a probe scaled by
2^-14 (the size a guidance run's gradients have: what an f16 backward without the loss scale cannot hold).
tests/test_vit_tower_bounds_cpu.py checks on the CPU that each seeded defect exceeds twice one of these gates.

Measured on one MI355X (the [bound] lines this module prints; the full table is DESIGN.md section 20), multiples of u, largest over the
blocks of a row, smallest .. largest over the six rows, bf16 / f16:
  x0 0.00 / 0.02..0.15   q,k,v 0.00..0.50 / 0.13..0.57   attn fwd 0.00..0.41 / 0.13..0.67 (gate 2)   hpre 0.00..0.16 / 0.09..0.34
  mlp fwd 0.00..0.20 / 0.07..0.36 (gate 1.73)   emb from x_final <= 0.02   head bwd 0.37..0.47 / 0.39..0.45 (gate 1)
  mlp bwd 0.71..0.87 / 0.72..0.88 (gate 1.73)   attn bwd 1.10..1.44 / 1.17..1.31 (gate 2.24, flash 2.45)
  g0 0.41..0.47 / 0.40..0.48   dcol, gradient per patch 0.46..0.52 / 0.46..0.52 (gate 1)
  whole tower: emb rel-L2 2.1..3.2e-3 / 2.8..4.5e-4 (gate 1.56e-2 / 1.95e-3; tiny-odd bf16 6e-8: no value crosses a rounding boundary),
  gradient rel-L2 4.3..5.4e-3 / 5.5..7.5e-4 (gate 2.28..2.34e-2 / 2.85..2.93e-3; t257: 1.75e-2 / 2.18e-3), per patch 1.30..2.28 u /
  1.59..2.23 u (gate 5.83 u, flash 6 u; t257 4.47 u), small probe: the unit probe's figure to within 2 % of the gate.
The worst check of every row is a backward branch at 0.47..0.59 of its gate; the fp32 CPU stand-in with the backward's 16-bit tensors
restated forecasts 0.46..0.63.  The forward figures are small because the reference rounds where the engine rounds.

Also: the routes each row takes are observed on the device run; record= changes no output bit; stale device memory (NaN-filled buffers
freed just before a run, so that torch.empty tends to return them -- best effort: the caching allocator is not obliged to) changes no
output bit; a permuted batch gives bitwise the permuted outputs; two live autograd graphs through models.OpenCLIP do not disturb each
other; shards of a batch at route-bearing widths stay within the whole-tower gate of the reference's slice.
"""
import functools

import pytest
import torch

import _vit_ref64 as V
import _vit_routes as VR

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f16"]
NAMES = list(VR.ROWS)


@functools.lru_cache(maxsize=None)
def _engine(name, dtype):
    from perceptor_amd.engine.vit import VitEngine
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    sd, _, _ = VR.inputs(name)
    return VitEngine(VR.ROWS[name]["cfg"], sd, "cuda:0", dtype, quick_gelu=True)


def _d_emb(emb, probe, gscale):
    """gscale * d <emb / |emb|, probe> / d emb, fp32 on the device (what models.OpenCLIP's autograd bridge hands to VitEngine.backward)"""
    nrm = emb.norm(dim=1, keepdim=True)
    e = emb / nrm
    return ((probe - e * (e * probe).sum(dim=1, keepdim=True)) / nrm * gscale).contiguous()


def _run(eng, img, probe, record=True, probe_scale=1.0):
    """forward(save=True) + backward under the unit probe -> (emb, grad, saved state, record), device tensors"""
    emb = eng.forward(img.cuda(), save=True)
    sv = eng.saved
    d_emb = _d_emb(emb, probe.cuda() * probe_scale, eng.gscale)
    rec = {} if record else None
    grad = eng.backward(d_emb, record=rec) if record else eng.backward(d_emb)
    torch.cuda.synchronize()
    return emb, grad, sv, rec, d_emb


def _unfrag(w, n, heads, t):
    """one of Q, K, V in the flash kernels' row-fragment order [n heads][tp32 / 32][c / 16][(c / 8) & 1][t & 31][c & 7] -> [n, heads, t, 64]"""
    nh, tp32, _ = w.shape
    return w.reshape(nh, tp32 // 32, 4, 2, 32, 8).permute(0, 1, 4, 2, 3, 5).reshape(nh, tp32, 64)[:, :t].reshape(n, heads, t, 64)


def _as_checked(eng, emb, grad, sv, rec, d_emb):
    """the engine's tensors in the form _vit_ref64.tower_checks reads (CPU)"""
    res, patch, width, layers, heads, out = eng.cfg
    n = sv["n"]
    t = (res // patch) ** 2 + 1
    c = lambda z: z.detach().cpu()
    tok = lambda z: c(z).reshape(n, t, -1)
    Ls = []
    for L in sv["layers"]:
        if L["aws"] is not None:
            q, k, v = (_unfrag(c(L["aws"][i]), n, heads, t) for i in range(3))
        else:
            q, k, v = (z.reshape(n, t, heads, width // heads).transpose(1, 2) for z in tok(L["qkv"]).split(width, dim=-1))
        Ls.append(dict(x_in=tok(L["x_in"]), x_mid=tok(L["x_mid"]), hpre=tok(L["hpre"]), q=q, k=k, v=v))
    return dict(n=n, gscale=eng.gscale, emb=c(emb), grad=c(grad), d_emb=c(d_emb), x0=c(sv["x0"]), x_final=tok(sv["x_final"]), layers=Ls,
                g32=[c(g) for g in rec["g32"]], gm32=[c(g) for g in rec["gm32"]], g0=c(rec["g0"]), dcol=c(rec["dcol"]))


def _assert_gates(tag, checks, u):
    worst = (0.0, "")
    for name, st, k in checks:
        print(f"[bound] vit {tag} {name}: {st / u:.3f} u, gate sqrt({k}) u = {k ** 0.5:.2f} u ({st / (u * k ** 0.5):.2f} of it)" if "tower" not in name else
              f"[bound] vit {tag} {name}: {st:.3e} = {st / u:.3f} u, gate sqrt({k}) u = {u * k ** 0.5:.3e} ({st / (u * k ** 0.5):.2f} of it)")
        worst = max(worst, (st / (u * k ** 0.5), name))
    print(f"[bound] vit {tag} worst: {worst[0]:.2f} of its gate ({worst[1]})")
    bad = [(name, st / u, k) for name, st, k in checks if not st <= u * k ** 0.5]
    assert not bad, (tag, bad)


# ---- block by block + whole tower + routes ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_tower_block_by_block(name, dtype, monkeypatch):
    from perceptor_amd.engine import ops
    row, u = VR.ROWS[name], V.U[VR.TD[dtype]]
    R, layers = row["routes"], row["cfg"][3]
    _, img, probe = VR.inputs(name)
    eng = _engine(name, dtype)
    assert eng.gscale == VR.GSCALE[dtype]
    # ---- the routes, observed on this run
    seen = dict(ln_slabs=0, bwd_slabs=0, bwd_plain=0, fused=[])
    ln_slabs, ln_bwd_any, fme = eng._ln_slabs, eng._ln_bwd_any, ops.fused_mlp_epilogues

    def count_slabs(*a, **k):
        seen["ln_slabs"] += 1
        return ln_slabs(*a, **k)

    def count_bwd(dy, *a, **k):
        seen["bwd_slabs" if isinstance(dy, tuple) else "bwd_plain"] += 1
        return ln_bwd_any(dy, *a, **k)

    def note_fused(lin, m):
        seen["fused"].append(fme(lin, m))
        return seen["fused"][-1]

    monkeypatch.setattr(eng, "_ln_slabs", count_slabs, raising=False)
    monkeypatch.setattr(eng, "_ln_bwd_any", count_bwd, raising=False)
    monkeypatch.setattr(ops, "fused_mlp_epilogues", note_fused)
    emb, grad, sv, rec, d_emb = _run(eng, img, probe)
    monkeypatch.undo()
    assert seen["ln_slabs"] == (layers - 1) * R["slabs_pr"], seen
    assert seen["bwd_slabs"] == layers * (R["slabs_fc"] + R["slabs_qkv"]) and seen["bwd_slabs"] + seen["bwd_plain"] == 2 * layers, seen
    assert seen["fused"] == [R["fused_fc"]] * layers + [R["fused_pr"]] * layers, seen
    assert all((L["aws"] is not None) == R["flash"] and (L["p"] is None) == R["flash"] for L in sv["layers"])
    G = VR.geometry(row["cfg"], row["n"])
    assert (eng.kp != G["k"]) == R["kp_pad"] and (G["t"] % 8 != 0) == R["t_odd"] and (G["m"] < 64) == R["m_small"]
    assert torch.isfinite(emb).all() and torch.isfinite(grad).all()
    for key in ("g32", "gm32"):
        assert len(rec[key]) == layers + (key == "g32") and all(torch.isfinite(g).all() for g in rec[key])
    # ---- record= is a seam: the same bits without it
    emb2, grad2, _, _, _ = _run(eng, img, probe, record=False)
    assert torch.equal(emb, emb2) and torch.equal(grad, grad2), "record= changed an output"
    # ---- the gates
    ref, whole = VR.reference(name, dtype)
    checks = V.tower_checks(ref, img, probe, _as_checked(eng, emb, grad, sv, rec, d_emb), whole)
    _, grad_small, _, _, _ = _run(eng, img, probe, record=False, probe_scale=V.SMALL_PROBE)
    assert torch.isfinite(grad_small).all()
    checks.append(V.small_probe_check(ref, grad_small.cpu(), whole))
    _assert_gates(f"{name} {dtype}", checks, u)


def test_backward_needs_a_forward():
    eng = _engine("tiny-odd", "bf16")
    _, img, probe = VR.inputs("tiny-odd")
    _run(eng, img, probe, record=False)
    with pytest.raises(RuntimeError, match="forward"):
        eng.backward(torch.zeros(4, 48, device="cuda"))


# ---- stale memory ---------------------------------------------------------------------------------------------------------------------
def _prefill(value, nbytes):
    """Device buffers of `value` (16-bit pattern: NaN reads as NaN in bf16, f16 and fp32) allocated and freed: what torch.empty tends to hand
    out next.  One large block (split by the allocator for the engine's large buffers) and many small ones (its pool for < 1 MB)."""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    big = torch.full((nbytes // 2,), value, dtype=torch.bfloat16, device="cuda")
    small = [torch.full((sz,), value, dtype=torch.bfloat16, device="cuda") for sz in (256, 4096, 65536, 262144) for _ in range(16)]
    torch.cuda.synchronize()
    del big, small


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["w768-d96", "h14-d80", "tiny-odd"])       # batched-GEMM attention with tp > t; padded im2col rows
def test_stale_memory_is_never_read(name, dtype):
    """Best effort (the allocator may hand out other memory): NaN in every buffer the engine gets from torch.empty -- the fp32 score and dP
    matrices' pad columns, P / dS / the transposes' pads, the im2col pad columns, the flash kernels' workspaces -- must change no bit."""
    _, img, probe = VR.inputs(name)
    eng = _engine(name, dtype)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    _run(eng, img, probe, record=False)
    nbytes = 2 * (torch.cuda.max_memory_allocated() - base) + (16 << 20)
    outs = []
    for value in (0.0, float("nan")):
        _prefill(value, nbytes)
        emb, grad, _, _, _ = _run(eng, img, probe, record=False)
        outs.append((emb.clone(), grad.clone()))
    assert torch.isfinite(outs[1][0]).all() and torch.isfinite(outs[1][1]).all()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


# ---- batch permutation ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["w512", "w768-d96"])                     # one flash row, one batched-GEMM row
def test_batch_permutation_is_bit_exact(name, dtype):
    _, img, probe = VR.inputs(name)
    eng = _engine(name, dtype)
    perm = torch.tensor([2, 0, 3, 1])
    emb, grad, _, _, _ = _run(eng, img, probe, record=False)
    emb_p, grad_p, _, _, _ = _run(eng, img[perm], probe[perm], record=False)
    assert torch.equal(emb_p, emb[perm.cuda()]) and torch.equal(grad_p, grad[perm.cuda()])


# ---- two live graphs ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_two_live_graphs_do_not_disturb_each_other(dtype):
    from perceptor_amd import models
    _, img, probe = VR.inputs("w512")
    model = models.OpenCLIP("vit-tower-w512", "synthetic", "fp16" if dtype == "f16" else "bf16", quick_gelu=True, config=VR.ROWS["w512"]["cfg"]).to("cuda")

    def grad_of(first, then=None):
        a = first.cuda().requires_grad_(True)
        with torch.enable_grad():
            ea = model.encode_images(a)
            if then is not None:
                b = then.cuda().requires_grad_(True)
                eb = model.encode_images(b)            # a second live graph at another batch size, never run backward
            (ea * probe[:a.shape[0]].cuda()).sum().backward()
        return a.grad

    alone = grad_of(img)
    assert torch.isfinite(alone).all() and float(alone.abs().max()) > 0
    assert torch.equal(grad_of(img, then=img[:1]), alone)
    assert torch.equal(grad_of(img[:3], then=img), grad_of(img[:3]))
    with pytest.raises(RuntimeError, match="forward"):
        model.engine.backward(torch.zeros(4, 64, device="cuda"))


# ---- shards at route-bearing widths ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["w512", "w768-d96"])
def test_shards_within_the_gate_of_the_references_slice(name, dtype):
    from perceptor_amd import losses
    from perceptor_amd.utils.synth import seeded_noise
    cfg, n, u = VR.ROWS[name]["cfg"], VR.ROWS[name]["n"], V.U[VR.TD[dtype]]
    _, img, _ = VR.inputs(name)
    loss = losses.OpenCLIP(f"vit-tower-{name}", "synthetic", quick_gelu=True, config=cfg, dtype="fp16" if dtype == "f16" else "bf16").to("cuda")
    tg = torch.nn.functional.normalize(seeded_noise((3, cfg[5]), 7))
    w = torch.tensor([1.0, 0.5, 2.0])
    loss.add_encodings_(tg, w)
    l_full, g_full = loss.loss_and_grad(img.cuda())
    _, g_half = loss.loss_and_grad(img[n // 2:].cuda(), n_total=n)
    # float64: the emulated tower under the spherical loss, mean over n * k pairs
    ref, _ = VR.reference(name, dtype)
    emb, st = ref.forward(img)
    e = emb.detach().requires_grad_(True)
    with torch.enable_grad():
        d = (torch.nn.functional.normalize(e)[:, None] - tg.double()[None]).norm(dim=2).div(2).arcsin().square().mul(2)
        l_ref = (d * w.double()).mean()
        (d_emb,) = torch.autograd.grad(l_ref, e)
    g_ref = ref.backward(d_emb, st)
    gate = V.depth_grad(cfg[3], ref.flash) ** 0.5 * u
    r_full, r_half = V.rel_l2(g_full.cpu(), g_ref), V.rel_l2(g_half.cpu(), g_ref[n // 2:])
    same = torch.equal(g_half, g_full[n // 2:])
    print(f"[bound] vit shards {name} {dtype}: loss {float(l_full):.6f} vs {float(l_ref.detach()):.6f}; grad rel-L2 whole batch {r_full:.3e}, last half as a shard {r_half:.3e}, "
          f"gate {gate:.3e}; shard bitwise equal to its slice: {same}")
    assert torch.isfinite(g_full).all() and torch.isfinite(g_half).all()
    assert r_full <= gate and r_half <= gate
