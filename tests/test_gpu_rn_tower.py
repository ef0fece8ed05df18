"""GPU: the CLIP ResNet tower (engine/resnet.py, csrc/resnet.hip) piece by piece against the float64 emulated tower of tests/_rn_ref64.py
(Emu), at the rows of tests/_rn_routes.py -- six-bottleneck towers (layers 2, 2, 1, 1) of width 16 / 64 / 80 / 96 at 64 .. 160 pixels, n = 1
and 3, one row with images at another size -- in bf16 AND f16.

Inputs: seeded_noise * 0.25 + 0.5 images, synth_state_dict weights, a unit probe on the normalised embedding.  u = 2^-8 (bf16), 2^-11
(f16).  The statistic is _vit_ref64.row_stat, max over rows of |got - ref|_2 / max(|ref|_2, rms over rows of |ref|_2), rows = pixels
(tokens in the attention pool).

Piece by piece, teacher-forced (_rn_ref64.tower_checks): every piece of the float64 tower is fed the ENGINE's own stored input of that piece
(eng.saved and what forward(record=) keeps), a backward piece also the engine's own ReLU masks and recorded upstream gradient
(backward(record=)), and its output -- with the piece's LAST rounding left out, so that a statistic holds the engine's k roundings and none
of the reference's -- is compared with the engine's next stored tensor; gradients on grad / scale.  The gate is sqrt(k) u, k the 16-bit
roundings inside the piece (the K_* constants of _rn_ref64.py, counted from engine/resnet.py):
  forward   x0 (1); s1, s2, s3, pooled (1 each); per block h1 (1), h2 (1), y (identity skip 1, downsample 2, stride 2: 4); tok, kv, q, o (1
            each); emb from o (1: fp32, an upper count); P within 1e-5 of its largest value
  backward  d_o (2); dq, dkv (1); dtok (1), g at x_final (2); per block g_in from g_out (identity 3, downsample 4); the stem through its pool
            (1: exact operations, an upper count), conv3^T and conv2^T (1 each); dx, dres (1: fp32, an upper count)
Whole tower: embedding rel-L2 <= sqrt(depth_fwd) u against the emulated tower's own run; image gradient rel-L2 <= sqrt(depth_grad) u against
the emulated tower with its ReLU masks pinned to the engine's (depth = the sum of k along the path: 37 / 67 for the rows' six blocks); the
gradient also under a probe scaled by 2^-14, at the same gate.  tests/test_rn_tower_bounds_cpu.py checks on the CPU that an fp32 stand-in
stays inside these gates and that each seeded defect exceeds twice one of them.

Also: the pmi_igemm routes each row takes are observed on the device run (ops.GEMM_TRACE) and equal the host's list; record= changes no
output bit; two runs are bit-equal; a permuted batch gives bitwise the permuted outputs.

Measured on one MI355X: DESIGN.md section 24 (the [bound] lines this module prints).
"""
import functools

import pytest
import torch

import _rn_ref64 as RN
import _rn_routes as RR

pytestmark = pytest.mark.gpu

DTYPES = ["bf16", "f16"]
NAMES = list(RR.ROWS)


@functools.lru_cache(maxsize=None)
def _engine(name, dtype):
    from perceptor_amd.engine.resnet import ResNetEngine
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    sd, _, _ = RR.inputs(name)
    return ResNetEngine(RR.ROWS[name]["cfg"], sd, "cuda:0", dtype)


def _d_emb(emb, probe, gscale):
    """gscale * d <emb / |emb|, probe> / d emb, fp32 on the device (what models.OpenCLIP's autograd bridge hands to ResNetEngine.backward)"""
    nrm = emb.norm(dim=1, keepdim=True)
    e = emb / nrm
    return ((probe - e * (e * probe).sum(dim=1, keepdim=True)) / nrm * gscale).contiguous()


def _run(eng, img, probe, record=True, probe_scale=1.0):
    """forward(save=True) + backward under the unit probe -> (emb, grad, saved state, forward record, backward record, d_emb)"""
    rf, rb = ({}, {}) if record else (None, None)
    emb = eng.forward(img.cuda(), save=True, record=rf) if record else eng.forward(img.cuda(), save=True)
    sv = eng.saved
    d_emb = _d_emb(emb, probe.cuda() * probe_scale, eng.gscale)
    grad = eng.backward(d_emb, record=rb) if record else eng.backward(d_emb)
    torch.cuda.synchronize()
    return emb, grad, sv, rf, rb, d_emb


def _as_checked(eng, img, emb, grad, sv, rf, rb, d_emb):
    """the engine's tensors in the form _rn_ref64.tower_checks reads (CPU; maps NCHW, tokens [N, T, C])"""
    res, layers, width, heads, out = eng.cfg
    n, c = sv["n"], width * 32
    t = sv["feat_hw"][0] * sv["feat_hw"][1] + 1
    cpu = lambda z: z.detach().cpu()
    nchw = lambda z: cpu(z).permute(0, 3, 1, 2)
    s1, s2, s3 = sv["stem"]
    blocks = [dict(x_in=nchw(x), h1=nchw(h1), h2=nchw(h2), y=nchw(y)) for x, (h1, h2, y) in zip(rf["x_in"], sv["tape"])]
    scale = rb["scale"]
    return dict(n=n, gscale=scale, in_hw=tuple(img.shape[-2:]), resized=cpu(rf["resized"]), x0=nchw(rf["x0"][..., :3]), s1=nchw(s1), s2=nchw(s2),
                s3=nchw(s3), pooled=nchw(rf["pooled"]), blocks=blocks, tok=cpu(rf["tok"]).view(n, t, c), kv=cpu(sv["kv"]).view(n, t, 2 * c),
                q=cpu(sv["q"]), P=cpu(sv["P"]).view(n, heads, t), o=cpu(rf["o"]), emb=cpu(emb), d_emb=cpu(d_emb) * (scale / eng.gscale),
                d_o=cpu(rb["d_o"]), dq=cpu(rb["dq"]), dkv=cpu(rb["dkv"]).view(n, t, 2 * c), dtok=cpu(rb["dtok"]).view(n, t, c), dq0=cpu(rb["dq0"]),
                g=[nchw(g) for g in rb["g"]], stem=[nchw(g) for g in rb["stem"]], dx=nchw(rb["dx"][..., :3]), dres=cpu(rb["dres"]), grad=cpu(grad))


def _assert_gates(tag, checks, u):
    rs = RN.ratios(checks, u)
    for (name, st, k), (ratio, *_) in zip(checks, rs):
        if k is None:
            print(f"[bound] rn {tag} {name}: {ratio:.3f} of 1e-5 max P")
        elif "tower" in name:
            print(f"[bound] rn {tag} {name}: {st:.3e} = {st / u:.3f} u, gate sqrt({k}) u = {u * k ** 0.5:.3e} ({ratio:.2f} of it)")
        else:
            print(f"[bound] rn {tag} {name}: {st / u:.3f} u, gate sqrt({k}) u = {k ** 0.5:.2f} u ({ratio:.2f} of it)")
    worst = max(rs)
    print(f"[bound] rn {tag} worst: {worst[0]:.2f} of its gate ({worst[1]})")
    bad = [(name, ratio, k) for ratio, name, _, k in rs if not ratio <= 1.0]
    assert not bad, (tag, bad)


# ---- piece by piece + whole tower + routes ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_tower_piece_by_piece(name, dtype):
    from perceptor_amd.engine import ops
    row, u = RR.ROWS[name], RN.U[RR.TD[dtype]]
    nb = len(RN.block_table(row["cfg"]))
    _, img, probe = RR.inputs(name)
    eng = _engine(name, dtype)
    assert eng.gscale == RR.GSCALE[dtype]
    # ---- the routes, observed on this run
    with RR.trace(ops) as descs:
        emb, grad, sv, rf, rb, d_emb = _run(eng, img, probe)
        seen = [RR.signature(d) for d in descs()]
    want = RR.host_routes(row["cfg"], row["n"], dtype)
    assert seen == want, [(i, a, b) for i, (a, b) in enumerate(zip(seen, want)) if a != b] or (len(seen), len(want))
    assert emb.shape == (row["n"], row["cfg"][4]) and grad.shape == img.shape
    assert torch.isfinite(emb).all() and torch.isfinite(grad).all()
    assert len(rf["x_in"]) == nb and len(rb["g"]) == nb + 1 and len(rb["stem"]) == 3
    assert all(torch.isfinite(g).all() for g in rb["g"] + rb["stem"])
    if dtype == "bf16":
        assert rb["scale"] == 1.0
    else:               # f16: the largest |d_emb| as the backward stores it lies in (512, 1024]
        assert rb["scale"] == eng.gscale * RN.grad_scale(float(d_emb.abs().max()))
        assert 512.0 < float(d_emb.abs().max()) * rb["scale"] / eng.gscale <= 1024.0
    # ---- record= and the trace are seams: the same bits without them, and again
    emb2, grad2, *_ = _run(eng, img, probe, record=False)
    assert torch.equal(emb, emb2) and torch.equal(grad, grad2), "record= changed an output"
    emb3, grad3, *_ = _run(eng, img, probe, record=False)
    assert torch.equal(emb2, emb3) and torch.equal(grad2, grad3), "two runs differ"
    # ---- the gates
    ref, whole = RR.reference(name, dtype)
    got = _as_checked(eng, img, emb, grad, sv, rf, rb, d_emb)
    pinned = ref.run(img, probe, masks=RN.masks_of(got))
    checks = RN.tower_checks(ref, img, got, whole, pinned)
    _, grad_small, *_ = _run(eng, img, probe, record=False, probe_scale=RN.SMALL_PROBE)
    assert torch.isfinite(grad_small).all()
    checks.append(RN.small_probe_check(ref, grad_small.cpu(), pinned))
    _assert_gates(f"{name} {dtype}", checks, u)


def test_backward_needs_a_forward():
    eng = _engine("w16-r64", "bf16")
    _, img, probe = RR.inputs("w16-r64")
    _run(eng, img, probe, record=False)
    with pytest.raises(RuntimeError, match="forward"):
        eng.backward(torch.zeros(3, 64, device="cuda"))


# ---- batch permutation ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["w16-r64", "w64-r160", "w16-r96-in"])          # generic-kernel rows and the split-K weights-direct row
def test_batch_permutation_is_bit_exact(name, dtype):
    _, img, probe = RR.inputs(name)
    eng = _engine(name, dtype)
    perm = torch.tensor([2, 0, 1])
    emb, grad, *_ = _run(eng, img, probe, record=False)
    emb_p, grad_p, *_ = _run(eng, img[perm], probe[perm], record=False)
    assert torch.equal(emb_p, emb[perm.cuda()]) and torch.equal(grad_p, grad[perm.cuda()])
