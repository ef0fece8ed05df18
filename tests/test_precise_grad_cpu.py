"""CPU: the precise-mode input gradient's host side.

  1. every new C entry point is declared in the header, exported by the library and bound in _hip._PROTOS with matching parameters;
  2. models.GuidedDiffusion(grad_mode=...) argument handling;
  3. ops.packed_dx with DT_F16X2: the packed operand against a physical split input equals W_hi^T (x_hi + x_lo) + W_lo^T x_hi;
  4. the float64 references of tests/_precise_grad_ref64.py: each bound rejects its defect model by >= 2x, and the float64 evaluation of
     the oracle UNets is the oracle's own function (its fp32 output agrees to fp32 rounding).
"""
import ctypes as C
import os

import pytest
import torch

import _precise_grad_ref64 as G
import _precise_ref64 as P
from test_abi import _header_decls, _kind

NEW_ENTRY_POINTS = ["pmi_split_add", "pmi_split_relu_bwd", "pmi_split_avgpool2_bwd", "pmi_split_upsample_bilinear2_bwd",
                    "pmi_split_upsample_nearest2_bwd", "pmi_split_gn1_bwd", "pmi_split_gn_bwd_stats", "pmi_split_gn_bwd_apply",
                    "pmi_softmax_bwd_f32"]
ADM_TINY_A = dict(image_size=64, model_channels=32, num_res_blocks=1, channel_mult=(1, 2, 2), attention_ds=(2, 4),
                  num_head_channels=16, use_scale_shift_norm=True, resblock_updown=True)


@pytest.mark.parametrize("name", NEW_ENTRY_POINTS)
def test_new_entry_points_in_header_library_and_protos(name):
    from perceptor_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        from perceptor_amd.csrc import build
        build.build()
    decls = _header_decls()
    assert name in decls, f"{name} is not declared in include/perceptor_hip.h"
    assert hasattr(C.CDLL(_hip.LIB_PATH), name), f"{name} is not exported"
    (args,) = _hip._PROTOS[name]
    assert [_kind(p) for p in decls[name]] == list(args)


def test_gemm_f32_args_layout_matches_header():
    import re
    from perceptor_amd import _hip
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "perceptor_hip.h")).read()
    body = src.split("} pmi_gemm_f32_args;")[0].rsplit("typedef struct {", 1)[1]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [re.findall(r"(\w+)\s*$", piece.strip())[0] for stmt in body.split(";") if stmt.strip() for piece in stmt.split(",")]
    assert names == [f[0] for f in _hip.GemmF32Args._fields_] and names[-1] == "transA"


def test_guided_diffusion_grad_mode_arguments():
    from perceptor_amd import models
    from perceptor_amd.engine import adm
    cfg = adm.AdmConfig(**ADM_TINY_A)
    m = models.GuidedDiffusion(config=cfg, dtype="precise", grad_mode="own")
    assert m.grad_mode == "own" and m.grad_engine is None          # no device: no engine yet
    assert models.GuidedDiffusion(config=cfg, dtype="precise").grad_mode == "f16"
    assert models.GuidedDiffusion(config=cfg, dtype="bf16", grad_mode="own").grad_mode == "own"
    with pytest.raises(ValueError):
        models.GuidedDiffusion(config=cfg, dtype="precise", grad_mode="bogus")
    with pytest.raises(NotImplementedError):
        models.GuidedDiffusion(config=cfg, dtype="mixed", grad_mode="own")


def _dx64(lin, xs, w_t, k):
    """the packed operand applied to the physical split input xs [N, H, W, lin.cin_p / (2 if self_concat)] as a convolution, float64"""
    n, h, wd, _ = xs.shape
    a = torch.cat([xs, xs], -1) if lin.self_concat else xs
    cols = torch.nn.functional.unfold(a.double().permute(0, 3, 1, 2), k, padding=k // 2)            # [N, Cp * taps, HW], channel-major
    cols = cols.reshape(n, a.shape[-1], k * k, h * wd).permute(0, 3, 2, 1).reshape(n, h * wd, -1)  # k = tap * Cp + c
    return (cols @ lin.w.double().T).reshape(n, h, wd, -1)


@pytest.mark.parametrize("case", ["3x3", "1x1", "slice", "cin_pad8"])
def test_packed_dx_precise_operand(case):
    from perceptor_amd._hip import DT_F16X2
    from perceptor_amd.engine import ops
    g = torch.Generator().manual_seed(7)
    cout, cin, k = (64, 32, 3) if case == "3x3" else (64, 96, 1) if case in ("1x1", "slice") else (6, 32, 3)
    w = torch.randn(cout, cin, k, k, generator=g) * 0.1                 # fp32 weights f16 cannot hold: the W_lo block is built
    wsrc = w[:, 32:64] if case == "slice" else w
    lin = ops.packed_dx({}, "k", wsrc, DT_F16X2, "cpu", cin_pad=8 if case == "cin_pad8" else None)
    cg = 8 if case == "cin_pad8" else cout                             # logical channels of the gradient tensor
    assert lin.split and lin.self_concat and lin.cin_p == 4 * cg
    hi, lo = P.coherent_hi_lo((1, 5, 6, cg), 11)
    if case == "cin_pad8":
        hi[..., cout:] = 0
        lo[..., cout:] = 0
    got = _dx64(lin, P.join_split(hi, lo), None, k)[..., :wsrc.shape[1]]
    wt = torch.zeros(cg, wsrc.shape[1], k, k)
    wt[:cout] = wsrc
    w_hi = wt.half().double()
    w_lo = (wt.double() - w_hi).float().half().double()               # PackedLinear stores the low block in f16
    conv_t = lambda v, ww: torch.nn.functional.conv_transpose2d(v.permute(0, 3, 1, 2), ww, padding=k // 2).permute(0, 2, 3, 1)   # noqa: E731
    want = conv_t(hi.double() + lo.double(), w_hi) + conv_t(hi.double(), w_lo)
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_elementwise_bounds_reject_their_defects():
    a, b = G.coherent((4, 16, 64), 1), G.coherent((4, 16, 64), 2)
    y, tol = G.add_ref(a, b)
    assert float(((G.split_round(y) - y).abs() / tol).max()) <= 1.0
    assert ((G.add_defect_halves(a, b) - y).abs() / tol).max() >= 2.0
    assert ((G.hi_of(y) - y).abs() / tol).max() >= 2.0                                       # output stored as hi only
    yv = G.split_round(torch.randn(4, 16, 64, generator=torch.Generator().manual_seed(3), dtype=torch.float64).clamp_min(0) * 3)
    yv = torch.where(yv > 0, yv, torch.zeros_like(yv))
    out, tol = G.relu_mask_ref(a, yv)
    assert ((G.relu_mask_defect_per_half(a, yv) - out).abs() / tol).max() >= 2.0
    assert ((torch.where(yv > 0, G.hi_of(a), torch.zeros_like(a)) - out).abs() / tol).max() >= 2.0   # lo half of g dropped


@pytest.mark.parametrize("name", ["avgpool", "nearest", "bilinear"])
def test_resample_adjoint_bounds_reject_their_defects(name):
    dy = G.coherent((2, 8, 12, 32), 5)
    ref = {"avgpool": lambda t: G.avgpool_bwd_ref(t, "precise"), "nearest": lambda t: G.nearest_bwd_ref(t, "precise"),
           "bilinear": lambda t: G.bilinear_bwd_ref(t, "precise", 4, 6)}[name]
    dx, tol = ref(dy)
    assert float(((G.split_round(dx) - dx).abs() / tol).max()) <= 1.0
    assert ((ref(G.hi_of(dy))[0] - dx).abs() / tol).max() >= 2.0                               # lo half of dy dropped
    assert ((G.hi_of(dx) - dx).abs() / tol).max() >= 2.0                                       # output stored as hi only


def test_gn1_backward_bound_rejects_its_defects():
    g = torch.Generator().manual_seed(9)
    x = G.split_round(torch.randn(2, 64, 64, generator=g, dtype=torch.float64) * 1.5 + 0.3)
    dy = G.coherent((2, 64, 64), 10)
    gamma = (1 + 0.2 * torch.randn(2, 64, generator=g)).double()
    dx, tol = G.gn1_backward_ref(x, dy, gamma, 1e-5, None, "precise")
    assert ((G.gn1_backward_ref(x, G.hi_of(dy), gamma, 1e-5, None, "precise")[0] - dx).abs() / tol).max() >= 2.0
    assert ((G.gn1_backward_ref(G.hi_of(x), dy, gamma, 1e-5, None, "precise")[0] - dx).abs() / tol).max() >= 2.0
    assert ((G.hi_of(dx) - dx).abs() / tol).max() >= 2.0


def test_softmax_and_attention_bounds_reject_their_defects():
    g = torch.Generator().manual_seed(12)
    p = torch.softmax(torch.randn(8, 256, generator=g, dtype=torch.float64) * 2, -1).float().double()
    dp = torch.randn(8, 256, generator=g, dtype=torch.float64).float().double()
    ds, tol = G.softmax_bwd_ref(dp, p, 0.125)
    assert ((G.softmax_bwd_defect_no_rowsum(dp, p, 0.125) - ds).abs() / tol).max() >= 2.0
    # small mixed-sign q, k (a worst-case bound over all-positive scores would swamp everything), coherent v and d out
    q, k = (G.split_round(torch.randn(2, 16, 16, generator=g, dtype=torch.float64) * 0.5) for _ in range(2))
    v, do = G.coherent((2, 16, 16), 15), G.coherent((2, 16, 16), 16)
    (dq, dk, dv), (tq, tk, tv) = G.attn_backward_ref(q, k, v, do, 0.25)
    (_, _, dv2), _ = G.attn_backward_ref(q, k, v, G.hi_of(do), 0.25)                           # lo half of d out dropped
    assert ((dv2 - dv).abs() / tv).max() >= 2.0
    assert ((G.hi_of(dv) - dv).abs() / tv).max() >= 2.0                                        # output stored as hi only


def test_attention_bound_rejects_wrong_dq_dk():
    """the hand-derived attention bound is tight enough to mean something: dQ / dK without the score scale, and dK from untransposed dS"""
    g = torch.Generator().manual_seed(17)
    q, k, v, do = (G.split_round(torch.randn(2, 16, 16, generator=g, dtype=torch.float64) * 0.5) for _ in range(4))
    (dq, dk, _), (tq, tk, _) = G.attn_backward_ref(q, k, v, do, 0.25)
    p = torch.softmax(q @ k.transpose(1, 2) * 0.25, -1)
    dp = do @ v.transpose(1, 2)
    ds_unscaled = p * (dp - (dp * p).sum(-1, keepdim=True))
    assert ((ds_unscaled @ k - dq).abs() / tq).max() >= 2.0 and ((ds_unscaled.transpose(1, 2) @ q - dk).abs() / tk).max() >= 2.0
    assert (((0.25 * ds_unscaled) @ q - dk).abs() / tk).max() >= 2.0


@pytest.mark.parametrize("case", [dict(C0=64, C1=0, film=True), dict(C0=64, C1=32, film=False)], ids=str)
def test_group_norm32_backward_bound_rejects_its_defects(case):
    """pmi_split_gn_bwd_stats / _apply (bound: gn_backward_ref with dtype "precise"): a dropped low half of dy, of x (either source) or of the
    skip-path gradient, and an output stored as hi only, on coherent operands"""
    from _norm_ref64 import gn_coeffs_ref, gn_stats_depth, standalone_depth
    N, H, W, C0, C1 = 2, 8, 8, case["C0"], case["C1"]
    C = C0 + C1
    g = torch.Generator().manual_seed(23)
    x = G.coherent((N, H, W, C), 24, 2.0) * torch.where(torch.rand(N, H, W, C, generator=g) < 0.5, -1.0, 1.0).double()
    dy, gadd = G.coherent((N, H, W, C), 25), G.coherent((N, H, W, C), 26)
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    film = 0.2 * torch.randn(N, 2 * C + 8, generator=g) if case["film"] else None
    depth, bdepth = standalone_depth(N, H * W, C), gn_stats_depth(N, H * W, C)

    def run(xv, dyv, ga):
        co = gn_coeffs_ref(xv, 32, 1e-5, gamma, beta, film, 2 * C + 8, depth=depth)
        return G.gn_backward_ref(xv, dyv, 32, 1e-5, gamma, beta, film, 2, co, depth, bdepth, gadd=ga, dtype="precise")

    dx, tol = run(x, dy, gadd)
    assert float(((G.split_round(dx) - dx).abs() / tol).max()) <= 1.0                         # the store itself is inside the bound
    worst = lambda d: float(((d - dx).abs() / tol).max())                                       # noqa: E731
    assert worst(run(x, G.hi_of(dy), gadd)[0]) >= 2.0                                          # lo half of dy dropped
    assert worst(run(G.hi_of(x), dy, gadd)[0]) >= 2.0                                          # lo half of x dropped
    assert worst(run(x, dy, G.hi_of(gadd))[0]) >= 2.0                                          # lo half of gadd dropped
    assert worst(G.hi_of(dx)) >= 2.0                                                           # output stored as hi only
    if C1:                                                                                     # lo half of the second source alone
        x1hi = torch.cat([x[..., :C0], G.hi_of(x[..., C0:])], -1)
        assert worst(run(x1hi, dy, gadd)[0]) >= 2.0


def test_restated_oracles_match_the_oracle_in_fp32():
    """tests/_precise_grad_ref64.py restates the oracle UNets without their fp32 casts; evaluated in fp32 the restatements reproduce the
    oracle's output to 1e-6 (relative L2), so their float64 evaluation is the same function"""
    from oracle import adm_unet as oa
    from oracle import vdiff as ov
    from perceptor_amd.engine import adm, vdiff
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    for kw in (ADM_TINY_A, dict(image_size=64, model_channels=32, num_res_blocks=2, channel_mult=(1, 2), attention_ds=(2,), num_heads=2,
                                use_new_attention_order=True),
               dict(image_size=64, model_channels=32, num_res_blocks=1, channel_mult=(1, 2), attention_ds=(2,), num_heads=1)):       # conv_resample
        sd = synth_state_dict(adm.state_dict_shapes(adm.AdmConfig(**kw)), 0)
        x, t = seeded_noise((1, 3, 64, 64), 31), torch.tensor([300.0])
        y32 = oa.adm_unet_forward(sd, oa.AdmConfig(**kw), x, t)
        assert G.rel_l2(G.adm_forward(sd, kw, x, t, torch.float32), y32) <= 1e-6
        y64, g64 = G.adm_grad(sd, kw, x, t, seeded_noise((1, 3, 64, 64), 61))
        assert y64.dtype == torch.float64 and g64.dtype == torch.float64 and G.rel_l2(y32, y64) <= 1e-4
    wk = dict(head_dim=32, up_mode="nearest", t_input="log_snr", skip_first=True)
    for cond, okw, ekw in ((False, {}, {}), (True, {}, {}), (False, wk, dict(wk, attn_norm=False))):
        spec = vdiff.make_spec("tiny", (3, 32, 32), [64, 128, 128], 2, 2, 4, 1, cond, **ekw)
        sdv = synth_state_dict(vdiff.state_dict_shapes(spec), 0)
        ospec = dict(ov.tiny_spec(cond), **okw)
        xv, tv, ce = seeded_noise((1, 3, 32, 32), 5), torch.tensor([0.9]), (seeded_noise((1, 512), 6) if cond else None)
        v32 = ov.vdiff_forward(sdv, ospec, xv, tv, ce)
        assert G.rel_l2(G.vdiff_forward(sdv, ospec, xv, tv, ce, torch.float32).detach(), v32) <= 1e-6
        v64, gx, _ = G.vdiff_grad(sdv, ospec, xv, tv, seeded_noise((1, 3, 32, 32), 8), ce)
        assert v64.dtype == torch.float64 and gx.shape == xv.shape and G.rel_l2(v32, v64) <= 1e-4
