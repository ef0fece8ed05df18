"""GPU: the input gradient in precise mode (hi + lo f16 pairs) for the ADM and v-diffusion UNets.

Kernel level: the pmi_split_* adjoints (csrc/backward.hip) and the fp32 attention backward against the float64 references and derived bounds
of tests/_precise_grad_ref64.py.  Engine level, every figure printed as `[grad] <case> precise: ...` (recorded in DESIGN section 7):
  * ADM (SiLU, smooth): rel-L2 against the float64 gradient of the restated oracle <= 16 F, F = the fp32 yardstick's own rel-L2 against that
    float64 gradient (fp32 yardstick: the reference's autograd fixture; for the 558 M net the float64 gradient is the sub-sampled fixture of
    tools/gen_adm_grad64_golden.py);
  * v-diffusion (ReLU): rel-L2 against the float64 backward PINNED to the engine's own ReLU masks (the signs of the post-ReLU tensors on
    the tape) <= 16 F_pinned, F_pinned = fp32 autograd against float64 under the same masks; unpinned only the structural condition;
  * every case: the precise gradient's rel-L2 against the fp32 yardstick is at most 1/3 of the f16 engine's.
"""
import pytest
import torch

import _precise_grad_ref64 as G
from _norm_ref64 import echeck, gn_coeffs_ref, gn_stats_depth, standalone_depth
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ADM_TINY = {
    "a": dict(image_size=64, model_channels=32, num_res_blocks=1, channel_mult=(1, 2, 2), attention_ds=(2, 4),
              num_head_channels=16, use_scale_shift_norm=True, resblock_updown=True),
    "b": dict(image_size=64, model_channels=32, num_res_blocks=2, channel_mult=(1, 2), attention_ds=(2,),
              num_heads=2, use_new_attention_order=True),
}
RS_SHAPES = [(2, 6, 10, 8), (1, 5, 7, 24), (2, 16, 16, 320), (1, 4, 4, 2560), (1, 1, 1, 64), (2, 1, 9, 16), (1, 128, 128, 256)]


def _vals(shape, seed, scale=1.0):
    return G.split_round(torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale)


def _dev(x):
    return G.to_split16(x).to(DEV).contiguous()


def _nan_like(shape):
    return torch.full(shape, float("nan"), dtype=torch.float16, device=DEV)


@pytest.mark.parametrize("shape", RS_SHAPES, ids=str)
@pytest.mark.parametrize("name", ["avgpool2", "upsample_nearest2", "upsample_bilinear2"])
def test_resample_adjoints_split(name, shape):
    from perceptor_amd._hip import call, ptr
    from perceptor_amd.engine import ops
    N, H, W, C = shape
    oshape = (N, H, W, C) if name == "avgpool2" else (N, 2 * H, 2 * W, C)
    ishape = (N, 2 * H, 2 * W, C) if name == "avgpool2" else (N, H, W, C)
    dy = _vals(oshape, 3)
    ref, tol = {"avgpool2": lambda: G.avgpool_bwd_ref(dy, "precise"), "upsample_nearest2": lambda: G.nearest_bwd_ref(dy, "precise"),
                "upsample_bilinear2": lambda: G.bilinear_bwd_ref(dy, "precise", H, W)}[name]()
    dyd = _dev(dy)
    outs = [_nan_like(ishape[:-1] + (2 * C,)) for _ in range(2)]
    for o in outs:
        call(f"pmi_split_{name}_bwd", ptr(dyd), ptr(o), N, ishape[1], ishape[2], C)
    echeck(f"{name} bwd split {shape}", G.from_split16(outs[0].cpu()), ref, tol)
    assert torch.equal(outs[0], outs[1])
    one = _nan_like((1,) + ishape[1:-1] + (2 * C,))
    call(f"pmi_split_{name}_bwd", ptr(dyd[:1].contiguous()), ptr(one), 1, ishape[1], ishape[2], C)
    assert torch.equal(one, outs[0][:1])
    # <A x, dy> = <x, A^T dy> against the precise forward (nearest x2 copies words: it runs on the physical tensor)
    x = _vals(ishape, 4)
    xd = _dev(x)
    fwd = {"avgpool2": lambda: ops.avgpool2(xd, 2), "upsample_nearest2": lambda: ops.upsample_nearest2(xd),
           "upsample_bilinear2": lambda: ops.upsample_bilinear2(xd, 2)}[name]()
    lhs = float((G.from_split16(fwd.cpu()) * dy).sum())
    rhs = float((x * G.from_split16(outs[0].cpu())).sum())
    slack = float((x.abs() * tol).sum()) + 1.5 * float((dy.abs() * (2.0 ** -21 * G.from_split16(fwd.cpu()).abs() + 2.0 ** -25)).sum())
    assert abs(lhs - rhs) <= slack, (lhs, rhs, slack)


def test_add_and_relu_mask_split():
    from perceptor_amd._hip import call, ptr
    for R0, R1, C in ((3, 17, 8), (3, 17, 24), (3, 17, 320), (2, 9, 2560), (2, 128 * 128, 256)):
        a, b = _vals((R0, R1, C), 5), _vals((R0, R1, C), 6)
        y = G.split_round(_vals((R0, R1, C), 7).clamp_min(0))
        ad, bd, yd = _dev(a), _dev(b), _dev(y)
        out, out2 = _nan_like(ad.shape), _nan_like(ad.shape)
        call("pmi_split_add", ptr(ad), ptr(bd), ptr(out), R0 * R1, C)
        call("pmi_split_add", ptr(ad), ptr(bd), ptr(out2), R0 * R1, C)
        echeck(f"add split C{C}", G.from_split16(out.cpu()), *G.add_ref(a, b))
        m, m1 = _nan_like(ad.shape), _nan_like(ad[:1].shape)
        call("pmi_split_relu_bwd", ptr(ad), ptr(yd), ptr(m), R0 * R1, C)
        call("pmi_split_relu_bwd", ptr(ad), ptr(yd), ptr(m1), R1, C)
        ref, _ = G.relu_mask_ref(a, y)
        assert torch.equal(G.from_split16(m.cpu()), ref)                      # a select: exact
        assert torch.equal(out, out2) and torch.equal(m1, m[:1])              # repeat call; sample 0 alone
        call("pmi_split_relu_bwd", ptr(ad), ptr(yd), ptr(ad), R0 * R1, C)     # in place, as VDiffEngine._mask calls it
        assert torch.equal(ad, m)
    # a positive value whose low half is negative keeps its gradient (the per-half mask of the 16-bit kernel would drop the low half)
    y = torch.full((1, 1, 8), 1.0 - 2.0 ** -13, dtype=torch.float64)
    g = _vals((1, 1, 8), 8)
    m = _nan_like((1, 1, 16))
    gd, yd = _dev(g), _dev(y)                                                  # named: a temporary's block is recycled by the next one
    call("pmi_split_relu_bwd", ptr(gd), ptr(yd), ptr(m), 1, 8)
    assert float(yd[0, 0, 8]) < 0 and torch.equal(G.from_split16(m.cpu()), g)


def test_argument_checks_launch_nothing():
    from perceptor_amd import _hip
    lib = _hip.lib()
    buf = _nan_like((2, 4, 4, 160))
    out = _nan_like((2, 8, 8, 160))
    s = _hip.stream_ptr()
    for C in (0, 12, 40, 72):                                                    # not a multiple of 8, or above 32 and not a multiple of 32
        assert lib.pmi_split_add(buf.data_ptr(), buf.data_ptr(), out.data_ptr(), 32, C, s) == -1
        assert lib.pmi_split_relu_bwd(buf.data_ptr(), buf.data_ptr(), out.data_ptr(), 32, C, s) == -1
        assert lib.pmi_split_avgpool2_bwd(buf.data_ptr(), out.data_ptr(), 2, 8, 8, C, s) == -1
        assert lib.pmi_split_upsample_nearest2_bwd(out.data_ptr(), buf.data_ptr(), 2, 4, 4, C, s) == -1
        assert lib.pmi_split_upsample_bilinear2_bwd(out.data_ptr(), buf.data_ptr(), 2, 4, 4, C, s) == -1
    # GroupNorm backward entry points: invalid split widths, a missing second source / output, a channel count the statistics tile cannot hold
    f = torch.zeros(4096 * 4, dtype=torch.float32, device=DEV)
    part = torch.full((64,), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.full((2 * 4 * 8192 * 2,), float("nan"), dtype=torch.float32, device=DEV)
    b, o, fp = buf.data_ptr(), out.data_ptr(), f.data_ptr()
    for C0, C, x1 in ((40, 40, None), (24, 64, b), (64, 96, None), (64, 104, b), (4128, 4128, None)):
        assert lib.pmi_split_gn_bwd_stats(b, x1, C0, b, fp, fp, 2, ws.data_ptr(), 2, 16, C, 4, s) == -1
    assert lib.pmi_split_gn_bwd_stats(b, None, 32, b, fp, fp, 2, ws.data_ptr(), 2, 16, 32, 0, s) == -1
    for C0, C, x1, dx1 in ((40, 40, None, None), (24, 64, b, o), (64, 96, None, o), (64, 96, b, None), (64, 104, b, o)):
        assert lib.pmi_split_gn_bwd_apply(b, x1, C0, b, fp, fp, fp, fp, 2, None, None, o, dx1, 2, 16, C, s) == -1
    assert lib.pmi_split_gn_bwd_apply(b, None, 32, b, fp, fp, fp, None, 2, None, None, o, None, 2, 16, 32, s) == -1
    for C in (0, 12, 40):
        assert lib.pmi_split_gn1_bwd(b, b, fp, 0, 0.0, None, o, part.data_ptr(), 2, 16, C, 1e-5, s) == -1
    assert lib.pmi_split_gn1_bwd(b, b, fp, -1, 0.0, None, o, part.data_ptr(), 2, 16, 32, 1e-5, s) == -1
    assert lib.pmi_split_gn1_bwd(b, b, fp, 0, 0.0, None, o, None, 2, 16, 32, 1e-5, s) == -1
    torch.cuda.synchronize()
    assert torch.isnan(ws).all() and torch.isnan(part).all()
    assert lib.pmi_split_avgpool2_bwd(buf.data_ptr(), out.data_ptr(), 2, 7, 8, 32, s) == -1
    assert lib.pmi_softmax_bwd_f32(out.data_ptr(), buf.data_ptr(), 4, 8, 4, 1.0, s) == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(buf).all()


@pytest.mark.parametrize("case", [dict(N=2, H=16, W=16, C0=64, act=2, film=True), dict(N=2, H=12, W=16, C0=96, act=0),
                                  dict(N=2, H=8, W=8, C0=128, C1=64, act=2, gadd=True), dict(N=1, H=32, W=32, C0=320, act=2),
                                  dict(N=2, H=16, W=16, C0=640, C1=320, act=2, film=True)], ids=str)
def test_group_norm_backward_split(case):
    from perceptor_amd.engine import ops
    N, H, W, C0, C1, act = case["N"], case["H"], case["W"], case["C0"], case.get("C1", 0), case["act"]
    C = C0 + C1
    g = torch.Generator().manual_seed(21)
    x, dy = _vals((N, H, W, C), 21, 1.5) + 0.3, _vals((N, H, W, C), 22)
    x = G.split_round(x)
    gamma, beta = (1 + 0.1 * torch.randn(C, generator=g)).to(DEV), (0.1 * torch.randn(C, generator=g)).to(DEV)
    film = (0.2 * torch.randn(N, 2 * C + 8, generator=g)).to(DEV) if case.get("film") else None
    gadd = _vals((N, H, W, C), 23) if case.get("gadd") else None
    xs0, xs1 = _dev(x[..., :C0]), (_dev(x[..., C0:]) if C1 else None)
    g0, g1 = (_dev(gadd[..., :C0]), _dev(gadd[..., C0:])) if gadd is not None else (None, None)
    kw = dict(x1=xs1, film=film, film_ld=2 * C + 8 if film is not None else 0)
    ca, cb, parts = ops.group_norm_coeffs_train(xs0, gamma, beta, 32, 2, **kw)
    depth = standalone_depth(N, H * W, C)
    co = gn_coeffs_ref(x.to(DEV), 32, 1e-5, gamma, beta, film, 2 * C + 8, depth=depth)
    ref, tol = G.gn_backward_ref(x.to(DEV), dy.to(DEV), 32, 1e-5, gamma, beta, film, act, co, depth, gn_stats_depth(N, H * W, C),
                                 gadd=gadd.to(DEV) if gadd is not None else None, dtype="precise")
    dyd = _dev(dy)
    outs = [ops.group_norm_backward(xs0, dyd, ca, cb, parts, gamma, 32, 2, act=act, gadd0=g0, gadd1=g1, **kw) for _ in range(2)]
    got = torch.cat([G.from_split16(o.cpu()) for o in outs[0] if o is not None], -1)
    echeck(f"gn bwd split {case}", got, ref.cpu(), tol.cpu())
    assert all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]) if a is not None)
    # the apply pass alone on sample 0 (its geometry per sample does not depend on N; the stats / finalize passes' does)
    from perceptor_amd._hip import call, ptr
    nchunk = max(1, min(H * W // 8, (1024 + N - 1) // N))
    wsb = torch.empty((N, nchunk, C, 2), dtype=torch.float32, device=DEV)
    cp, cq = torch.empty((N, C), dtype=torch.float32, device=DEV), torch.empty((N, C), dtype=torch.float32, device=DEV)
    call("pmi_split_gn_bwd_stats", ptr(xs0), ptr(xs1), C0, ptr(dyd), ptr(ca), ptr(cb), act, ptr(wsb), N, H * W, C, nchunk)
    call("pmi_gn_bwd_finalize", ptr(parts[0]), parts[1], parts[2], ptr(parts[3]), parts[4], parts[5], ptr(wsb), nchunk, ptr(gamma), ptr(film),
         kw["film_ld"], ptr(cp), ptr(cq), N, H * W, 32, 1e-5)
    s0, s1 = _nan_like((1,) + xs0.shape[1:]), (_nan_like((1,) + xs1.shape[1:]) if C1 else None)
    call("pmi_split_gn_bwd_apply", ptr(xs0), ptr(xs1), C0, ptr(dyd), ptr(ca), ptr(cb), ptr(cp), ptr(cq), act, ptr(g0), ptr(g1), ptr(s0), ptr(s1),
         1, H * W, C)
    assert torch.equal(s0, outs[0][0][:1]) and (not C1 or torch.equal(s1, outs[0][1][:1]))


@pytest.mark.parametrize("case", [dict(N=2, hw=128 * 128, C=256, ld=512, add=1.0, res=True), dict(N=2, hw=64, C=64, ld=0, add=0.0, res=True),
                                  dict(N=1, hw=64, C=24, ld=0, add=0.0, res=False)], ids=str)
def test_gn1_backward_split(case):
    from perceptor_amd._hip import call, lib, ptr
    N, hw, C, ld, add = case["N"], case["hw"], case["C"], case["ld"], case["add"]
    g = torch.Generator().manual_seed(hw + C)
    x, dy = G.split_round(_vals((N, hw, C), 1, 1.5) + 0.3), _vals((N, hw, C), 2)
    res = _vals((N, hw, C), 3) if case["res"] else None
    gam = (0.3 * torch.randn(max(N * ld, C), generator=g)).float() + (1.0 - add)
    gamma_nc = (gam[:C][None].expand(N, C) if ld == 0 else gam[:N * ld].reshape(N, ld)[:, :C]).double() + add
    ref, tol = G.gn1_backward_ref(x.to(DEV), dy.to(DEV), gamma_nc, 1e-5, res.to(DEV) if res is not None else None, "precise")
    P = lib().pmi_gn1_bwd_partials(hw, C)
    xd, dyd, rd, gd = _dev(x), _dev(dy), (_dev(res) if res is not None else None), gam.to(DEV)
    outs = []
    for _ in range(2):
        part = torch.empty((N * P * 4,), dtype=torch.float64, device=DEV)
        dx = _nan_like((N, hw, 2 * C))
        call("pmi_split_gn1_bwd", ptr(xd), ptr(dyd), ptr(gd), ld, add, ptr(rd), ptr(dx), ptr(part), N, hw, C, 1e-5)
        outs.append(dx)
    echeck(f"gn1 bwd split {case}", G.from_split16(outs[0].cpu()), ref.cpu(), tol.cpu())
    assert torch.equal(outs[0], outs[1])
    part1 = torch.empty((P * 4,), dtype=torch.float64, device=DEV)
    dx1 = _nan_like((1, hw, 2 * C))
    call("pmi_split_gn1_bwd", ptr(xd), ptr(dyd), ptr(gd), ld, add, ptr(rd), ptr(dx1), ptr(part1), 1, hw, C, 1e-5)
    assert torch.equal(dx1, outs[0][:1])


@pytest.mark.parametrize("T,d", [(16, 64), (64, 64), (256, 64), (1024, 64), (64, 16), (64, 128)])      # d 16: ADM tiny; 128: the wikiart net's heads
def test_attention_backward_precise(T, d):
    from perceptor_amd.engine import ops
    n, heads = 2, 2
    c = heads * d
    qkv = _vals((n * T, 3 * c), 40 + T, 0.7)
    do = _vals((n * T, c), 41 + T)
    qd, dod = _dev(qkv), _dev(do)
    out, saved = ops.attention_precise_train(qd, n, T, heads)
    dqkv = ops.attention_precise_backward(saved, dod, n, T, heads)
    assert torch.equal(dqkv, ops.attention_precise_backward(saved, dod, n, T, heads))
    hd = lambda t, k: t.reshape(n, T, -1, heads, d)[:, :, k].permute(0, 2, 1, 3).reshape(n * heads, T, d)      # noqa: E731
    q, k, v = (hd(qkv, i) for i in range(3))
    refs, tols = G.attn_backward_ref(q, k, v, hd(do, 0), d ** -0.5)
    got = G.from_split16(dqkv.cpu())
    for i, nm in enumerate("qkv"):
        echeck(f"precise attention backward T{T} d{nm}", hd(got, i), refs[i], tols[i])
    p = torch.softmax(q @ k.transpose(1, 2) * d ** -0.5, -1)
    assert G.rel_l2(G.from_split16(out.cpu()), (p @ v).reshape(n, heads, T, d).permute(0, 2, 1, 3).reshape(n * T, c)) <= 1e-6


# ---- engines -----------------------------------------------------------------------------------------------------------------------------------
def _adm(cfg_kw, dtype, x, t, probe, standard=False):
    from perceptor_amd.engine import adm
    from perceptor_amd.utils.synth import synth_state_dict
    cfg = adm.openimages_config() if standard else adm.AdmConfig(**cfg_kw)
    sd = synth_state_dict(adm.state_dict_shapes(cfg), 0)
    eng = adm.AdmEngine(cfg, sd, DEV, dtype)
    img = ((x + 1) / 2).to(DEV)
    y, tape = eng.forward_train(img, t.to(DEV), sd, out_channels=3)
    if dtype == "precise" and (standard or cfg.use_new_attention_order):
        # same kernels, same operands (the legacy attention order trains on reordered qkv rows: attention path aside, as the 16-bit test says)
        assert torch.equal(y, eng.forward(img, t.to(DEV), out_channels=3))
    return eng, tape, sd, eng.backward(tape, probe.to(DEV), sd).cpu() / 2.0


@pytest.mark.parametrize("tag", ["a", "b"])
def test_adm_tiny_precise_gradient(tag):
    from perceptor_amd.utils.synth import seeded_noise
    g0 = golden(f"adm_tiny_{tag}_grad")
    x, probe = seeded_noise((2, 3, 64, 64), 31), seeded_noise((2, 3, 64, 64), 61)
    eng, tape, sd, got = _adm(ADM_TINY[tag], "precise", x, g0["t"], probe)
    _, _, _, g16 = _adm(ADM_TINY[tag], "f16", x, g0["t"], probe)
    _, g64 = G.adm_grad(sd, ADM_TINY[tag], x, g0["t"], probe)
    F_ = G.rel_l2(g0["g"], g64)
    rel, rel16, rel64 = G.rel_l2(got, g0["g"]), G.rel_l2(g16, g0["g"]), G.rel_l2(got, g64)
    cos = float(torch.nn.functional.cosine_similarity(got.double().flatten(), g0["g"].double().flatten(), dim=0))
    print(f"[grad] adm_tiny_{tag} precise: rel-L2 {rel:.3e} cos {cos:.8f}  (vs float64 {rel64:.3e}, F {F_:.3e}, ratio {rel64 / F_:.2f}; f16 {rel16:.3e})")
    assert rel64 <= 16 * F_, (rel64, F_)
    assert rel <= rel16 / 3
    # scale invariance: the power-of-two input scale makes the arithmetic identical; a 1e-6 cotangent keeps the accuracy
    for f in (2.0 ** -20, 2.0 ** 10):
        assert torch.equal(eng.backward(tape, (probe * f).to(DEV), sd).cpu() / 2.0 / f, got)
    small = eng.backward(tape, (probe * 1e-6).to(DEV), sd).cpu() / 2.0
    assert G.rel_l2(small, g64 * 1e-6) <= 16 * F_
    # two walks over one tape agree; the tape survives another forward_train on the engine
    eng.forward_train(((probe + 1) / 2).to(DEV), g0["t"].to(DEV), sd, out_channels=3)
    assert torch.equal(eng.backward(tape, probe.to(DEV), sd).cpu() / 2.0, got)


def test_adm_conv_resample_precise_gradient():
    """A pixelart-style config (conv_resample: stride-2 convolution down, nearest x2 + convolution up -- the "resample" tape records and their
    zero-inserted split gradient; additive timestep conditioning; one legacy-order head).  No reference fixture exists for it: the fp32
    yardstick is fp32 autograd over the restated oracle, which equals the oracle in fp32 (tests/test_precise_grad_cpu.py)."""
    from perceptor_amd.utils.synth import seeded_noise
    kw = dict(image_size=64, model_channels=32, num_res_blocks=1, channel_mult=(1, 2, 2), attention_ds=(4,), num_heads=1)
    x, probe, t = seeded_noise((2, 3, 64, 64), 33), seeded_noise((2, 3, 64, 64), 63), torch.tensor([10, 500])
    eng, tape, sd, got = _adm(kw, "precise", x, t, probe)
    assert any(rec[0] == "resample" for tp in tape["inp"] + tape["out"] for rec in tp)
    g16 = _adm(kw, "f16", x, t, probe)[3]
    (_, g32), (_, g64) = G.adm_grad(sd, kw, x, t, probe, torch.float32), G.adm_grad(sd, kw, x, t, probe)
    F_, rel64, rel, rel16 = G.rel_l2(g32, g64), G.rel_l2(got, g64), G.rel_l2(got, g32), G.rel_l2(g16, g32)
    print(f"[grad] adm_conv_resample precise: rel-L2 {rel:.3e}  (vs float64 {rel64:.3e}, F {F_:.3e}, ratio {rel64 / F_:.2f}; f16 {rel16:.3e})")
    assert rel64 <= 16 * F_ and rel <= rel16 / 3
    assert torch.equal(eng.backward(tape, (probe * 2.0 ** -20).to(DEV), sd).cpu() / 2.0 * 2.0 ** 20, got)


def test_adm_standard_128_precise_gradient():
    from perceptor_amd.utils.synth import seeded_noise
    g0 = golden("adm_standard_128_grad")
    x, probe = seeded_noise((1, 3, 128, 128), 32), seeded_noise((1, 3, 128, 128), 62)
    got = _adm(None, "precise", x, g0["t"], probe, standard=True)[3]
    g16 = _adm(None, "f16", x, g0["t"], probe, standard=True)[3]
    rel, rel16 = G.rel_l2(got[:, :, ::2, ::2], g0["g_sub"]), G.rel_l2(g16[:, :, ::2, ::2], g0["g_sub"])
    g64 = golden("adm_standard_128_grad64")
    F_ = G.rel_l2(g0["g_sub"], g64["g_sub"])
    rel64 = G.rel_l2(got[:, :, ::2, ::2], g64["g_sub"])
    print(f"[grad] adm_standard_128 precise: rel-L2 {rel:.3e}  (vs float64 {rel64:.3e}, F {F_:.3e}, ratio {rel64 / F_:.2f}; f16 {rel16:.3e})")
    assert abs(F_ / float(g64["F"]) - 1) < 1e-6
    assert rel64 <= 16 * F_, (rel64, F_)
    assert rel <= rel16 / 3
    assert abs(float(got.flatten(1).double().norm()) / float(g0["g_mom"][0, 2]) - 1) < 1e-3


@pytest.mark.parametrize("name", ["tiny", "tiny_cond", "tinyw"])
def test_tiny_vnet_precise_gradient(name):
    from oracle import vdiff as ov
    from perceptor_amd.engine import vdiff
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    cond = name == "tiny_cond"
    kw = dict(head_dim=32, attn_norm=False, up_mode="nearest", t_input="log_snr", skip_first=True) if name == "tinyw" else {}
    okw = {k: v for k, v in kw.items() if k != "attn_norm"}
    spec = vdiff.make_spec(name, (3, 32, 32), [64, 128, 128], 2, 2, 4, 1, cond, **kw)
    sd = synth_state_dict(vdiff.state_dict_shapes(spec), 0, gain=0.7) if name == "tinyw" else synth_state_dict(vdiff.state_dict_shapes(spec), 0)
    x, t, probe = seeded_noise((2, 3, 32, 32), 5), torch.tensor([0.9, 0.3]), seeded_noise((2, 3, 32, 32), 8)
    ce = seeded_noise((2, 512), 6) if cond else None
    ospec = dict(ov.tiny_spec(cond), **okw)
    xr, cer = x.clone().requires_grad_(), (ce.clone().requires_grad_() if cond else None)
    with torch.enable_grad():                                                    # the yardstick: fp32 autograd over the oracle
        gs32 = torch.autograd.grad((ov.vdiff_forward.__wrapped__(sd, ospec, xr, t, cer) * probe).sum(), [xr] + ([cer] if cond else []))
    v64, g64, gce64 = G.vdiff_grad(sd, ospec, x, t, probe, ce)
    res = {}
    img, td, ced, pd = ((x + 1) / 2).to(DEV), t.to(DEV), (ce.to(DEV) if cond else None), probe.to(DEV)
    cg = (td, ced) if cond else None
    split = lambda out: (out[0].cpu() / 2, out[1].cpu()) if cond else (out.cpu() / 2, None)          # noqa: E731
    for dtype in ("f16", "precise"):
        eng = vdiff.VDiffEngine(spec, sd, DEV, dtype)
        v, tape = eng.forward_train(img, td, ced)
        res[dtype] = split(eng.backward(tape, pd, sd, cond_grad=cg))
    # the training forward keeps relu(conv2) as its own tensor before the skip add: one more split rounding than the fused epilogue
    assert G.rel_l2(v, eng.forward(img, td, ced)) <= 2e-6 and G.rel_l2(v, v64) <= 1e-5
    got, got_ce = res["precise"]
    rel, rel16 = G.rel_l2(got, gs32[0]), G.rel_l2(res["f16"][0], gs32[0])
    # float64 and fp32 backward pinned to the engine's own ReLU masks
    masks = G.tape_masks(tape, True)
    _, p64, pce64 = G.vdiff_grad(sd, ospec, x, t, probe, ce, torch.float64, masks)
    _, p32, pce32 = G.vdiff_grad(sd, ospec, x, t, probe, ce, torch.float32, masks)
    Fp, relp = G.rel_l2(p32, p64), G.rel_l2(got, p64)
    print(f"[grad] {name} precise: rel-L2 {rel:.3e}  (pinned: vs float64 {relp:.3e}, F_pinned {Fp:.3e}, ratio {relp / Fp:.2f}; "
          f"unpinned vs float64 {G.rel_l2(got, g64):.3e}; f16 {rel16:.3e})")
    assert relp <= 16 * Fp, (relp, Fp)
    assert rel <= rel16 / 3
    if cond:
        rc, rc16, Fc, rcp = G.rel_l2(got_ce, gs32[1]), G.rel_l2(res["f16"][1], gs32[1]), G.rel_l2(pce32, pce64), G.rel_l2(got_ce, pce64)
        print(f"[grad] {name} d clip_embed precise: rel-L2 {rc:.3e}  (pinned: vs float64 {rcp:.3e}, F_pinned {Fc:.3e}, ratio {rcp / Fc:.2f}; f16 {rc16:.3e})")
        assert rcp <= 16 * Fc and rc <= rc16 / 3
    # scale invariance (image and conditioning gradient, whose d_mod / scale undo is part of it); a 1e-6 cotangent keeps the bound
    for f in (2.0 ** -20, 2.0 ** 10):
        a, a_ce = split(eng.backward(tape, pd * f, sd, cond_grad=cg))
        assert torch.equal(a / f, got) and (not cond or torch.equal(a_ce / f, got_ce))
    small, small_ce = split(eng.backward(tape, pd * 1e-6, sd, cond_grad=cg))
    assert G.rel_l2(small, p64 * 1e-6) <= 16 * Fp and (not cond or G.rel_l2(small_ce, pce64 * 1e-6) <= 16 * Fc)
    # two walks over one tape agree; the tape survives another forward_train on the engine
    eng.forward_train(((probe + 1) / 2).to(DEV), td, ced)
    b, b_ce = split(eng.backward(tape, pd, sd, cond_grad=cg))
    assert torch.equal(b, got) and (not cond or torch.equal(b_ce, got_ce))


@pytest.mark.parametrize("case", [("yfcc_2", "vdiff_yfcc_2_128", 128, 46, {}), ("cc12m_1_cfg", "vdiff_cc12m_1_64", 64, 47, {}),
                                  ("wikiart", "vdiff_wikiart_64", 64, 48, dict(weight_gain=0.6))], ids=lambda c: c[0])
def test_full_vnets_precise_gradient(case):
    """Through the public surface: models.VelocityDiffusion(dtype="precise").velocities on an input that requires grad."""
    from perceptor_amd import models
    from perceptor_amd.utils.synth import seeded_noise
    name, fx, size, seed, kw = case
    g0, g = golden(fx), golden(fx + "_grad")
    probe = seeded_noise((1, 3, size, size), seed).to(DEV)
    ce = g0["clip_embed"] if "clip_embed" in g0 else None
    rels = {}
    for dtype in ("f16", "precise"):
        m = models.VelocityDiffusion(name, dtype=dtype, **kw).to(DEV)
        img = ((g0["x"] + 1) / 2).to(DEV).requires_grad_()
        args = (ce[:, None, :].to(DEV),) if ce is not None else ()
        with torch.enable_grad():
            (m.velocities(img, g["t"].to(DEV), *args) * probe).sum().backward()
        gx = img.grad.cpu() / 2
        rels[dtype] = G.rel_l2(gx[:, :, ::2, ::2], g["g_sub"]) if "g_sub" in g else G.rel_l2(gx, g["g"])
        if dtype == "precise":
            if "g_mom" in g:
                assert torch.allclose(gx.flatten(1).double().norm(dim=1).float(), g["g_mom"][:, 2], rtol=1e-3)
            # the engine's own tape gives the masks the float64 / fp32 backward is pinned to (CPU autograd over the restated oracle)
            _, tape = m.engine.forward_train(img.detach(), g["t"].to(DEV), ce.to(DEV) if ce is not None else None)
            masks = G.tape_masks(tape, True)
            sd = {k: v.detach().cpu() for k, v in m.model.state_dict().items()}
            del tape
        del m
        torch.cuda.empty_cache()
    from oracle import vdiff as ov
    ospec = {"yfcc_2": ov.yfcc2_spec, "cc12m_1_cfg": ov.cc12m1_spec, "wikiart": ov.wikiart_spec}[name]()
    _, p64, _ = G.vdiff_grad(sd, ospec, g0["x"], g["t"], probe.cpu(), ce, torch.float64, masks)
    _, p32, _ = G.vdiff_grad(sd, ospec, g0["x"], g["t"], probe.cpu(), ce, torch.float32, masks)
    Fp, relp = G.rel_l2(p32, p64), G.rel_l2(gx, p64)
    print(f"[grad] {fx} precise: rel-L2 {rels['precise']:.3e}  (pinned: vs float64 {relp:.3e}, F_pinned {Fp:.3e}, ratio {relp / Fp:.2f}; "
          f"f16 {rels['f16']:.3e})")
    assert relp <= 16 * Fp, (relp, Fp)
    assert rels["precise"] <= rels["f16"] / 3


def test_velocity_diffusion_precise_model_and_guided_resample():
    from perceptor_amd import losses, models
    from perceptor_amd.engine import vdiff
    from perceptor_amd.utils.synth import seeded_noise
    spec = vdiff.make_spec("tiny", (3, 32, 32), [64, 128, 128], 2, 2, 4, 1, False)
    m = models.VelocityDiffusion("yfcc_2", spec=spec, dtype="precise").to(DEV)
    img = ((seeded_noise((2, 3, 32, 32), 5) + 1) / 2).to(DEV).requires_grad_()
    t, w = torch.tensor([0.9, 0.3]).to(DEV), seeded_noise((2, 3, 32, 32), 8).to(DEV)
    with torch.enable_grad():
        (gr,) = torch.autograd.grad((m.velocities(img, t) * w).sum(), img)
    _, tape = m.engine.forward_train(img.detach(), t, None)
    assert torch.equal(gr, m.engine.backward(tape, w, m.model.state_dict()))
    # guided_resample_ on the precise model against the same chain written with autograd over the oracle (as tests/test_gpu_backward.py does)
    import math
    from oracle import sampling
    from oracle import vdiff as ov
    from perceptor_amd.engine import sampler
    sd = {k: v.detach().cpu() for k, v in m.model.state_dict().items()}
    den0, noise0 = seeded_noise((2, 3, 32, 32), 12) * 0.2 + 0.5, seeded_noise((2, 3, 32, 32), 13)
    target = seeded_noise((2, 3, 32, 32), 14) * 0.2 + 0.5
    loss = losses.VelocityDiffusion(m, noise0.clone().to(DEV), from_ts=0.5, resample_ts=0.3)
    torch.manual_seed(77)
    key = sampler.rng.next_key()
    torch.manual_seed(77)
    with loss.guided_resample_(den0.to(DEV), guidance_scale=0.5, clamp_value=1e-6) as dd:
        (dd - target.to(DEV)).square().mean().backward()
    a, s = math.cos(0.5 * math.pi / 2), math.sin(0.5 * math.pi / 2)
    nz = noise0.clone().requires_grad_()
    with torch.enable_grad():
        x_d = (den0 * 2 - 1) * a + nz * s
        v = ov.vdiff_forward.__wrapped__(sd, ov.tiny_spec(False), x_d, torch.full((2,), 0.5))
        ((((x_d * a - v * s) + 1) / 2) - target).square().mean().backward()
    u64 = lambda k: k & ((1 << 64) - 1)          # noqa: E731
    rn = sampling.device_randn((2, 3, 32, 32), u64(key[0]), u64(key[1]))
    v_g = sampling.guided(v.detach(), -nz.grad, torch.full((2,), s))
    want = sampling.resample_noise(x_d.detach() * s + v_g * a, torch.full((2,), s), torch.full((2,), math.sin(0.3 * math.pi / 2)), rn)
    sure = nz.grad.abs() > 0.25 * nz.grad.abs().mean()
    frac = float(((loss.noise.data.cpu() - want).abs() < 5e-2)[sure].float().mean())
    print(f"[parity] guided_resample_ precise: noise update agrees on {frac:.4f} of the {int(sure.sum())} elements with |grad| > mean/4")
    assert frac >= 0.98 and float(loss.noise.grad.abs().max()) == 0.0


def test_guided_diffusion_grad_mode_own():
    from perceptor_amd import models
    from perceptor_amd.engine import adm
    cfg = adm.AdmConfig(**ADM_TINY["a"])
    m = models.GuidedDiffusion(config=cfg, dtype="precise", grad_mode="own").to(DEV)
    img = torch.rand(2, 3, 64, 64, generator=torch.Generator().manual_seed(1)).to(DEV).requires_grad_()
    idx = torch.tensor([300, 20])
    w = torch.randn(2, 3, 64, 64, generator=torch.Generator().manual_seed(2)).to(DEV)
    eps = m.predicted_noise(img, idx)
    (gr,) = torch.autograd.grad((eps * w).sum(), img)
    assert m.grad_engine is m.engine and m.__dict__.get("_grad_engine") is None
    y, tape = m.engine.forward_train(img.detach(), idx.to(DEV), m.model.state_dict(), out_channels=3)
    assert torch.equal(eps.detach(), y) and torch.equal(gr, m.engine.backward(tape, w, m.model.state_dict()))
    # legacy attention order: the training forward's qkv rows are reordered; documented bound of the value against forward()
    assert G.rel_l2(y, m.engine.forward(img.detach(), idx.to(DEV), out_channels=3)) <= 1e-6
    # default grad_mode: still the f16 engine's bits
    md = models.GuidedDiffusion(config=cfg, dtype="precise").to(DEV)
    m16 = models.GuidedDiffusion(config=cfg, dtype="f16").to(DEV)
    gs = []
    for mm in (md, m16):
        im = img.detach().clone().requires_grad_()
        (g1,) = torch.autograd.grad((mm.predicted_noise(im, idx) * w).sum(), im)
        gs.append(g1)
    assert torch.equal(gs[0], gs[1]) and md.__dict__.get("_grad_engine") is not None
    assert G.rel_l2(gr, gs[0]) > 1e-5                                   # and "own" is a different (more accurate) gradient
