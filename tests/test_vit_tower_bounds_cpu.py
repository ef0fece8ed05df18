"""CPU: the float64 restatement of the CLIP ViT tower (tests/_vit_ref64.py), the route table (tests/_vit_routes.py) and the gates of
tests/test_gpu_vit_tower.py, checked without a device.

1. Exactness.  Tower(emulate=None) reproduces oracle/clip_vit.py -- vit_forward and the gradient of encode_images -- at every table row
   (measured: embedding rel-L2 <= 5.9e-7, gradient <= 1.3e-6, the oracle's own fp32 noise) and the committed clip_vit_tiny / clip_vit_tiny-odd
   fixtures' embeddings.
2. Route table.  Every row takes the routes the table says, asked of the library's own host queries, and the rows together cover both
   values of every flag.  (t % 8 != 0 holds at EVERY square patch grid: t = g^2 + 1 and g^2 mod 8 is 0, 1 or 4 -- that flag has one value.)
3. Stand-in.  The same restatement in fp32 arithmetic stays within HALF of every gate at every row in both types (measured: at most 0.47
   of a gate, the stored q / k / v of w768-d96 in f16): a condition on the reference and the inputs -- the fp32 evaluation of the emulated tower does not, by itself, use up the
   gates -- not the device's number.  With the 16-bit tensors of the engine's backward restated as well (bwd=) the stand-in is a
   forecast of the device run and must stay within the gates themselves (measured: at most 0.63 of a gate, the attention backward's).
4. Seeded defects.  Each defect of _vit_ref64.DEFECTS, seeded in block 0 of the emulated tower, exceeds TWICE the gate of at least one
   check at every row it applies to, in both types.  Smallest margins (bf16; f16 margins are 8x these, the defects being absolute):
       pad keys 2.7x (t257: 7 pad keys against 257), last key 6.8x (t257), lost row 139x, head bwd 67x, slab 80x, bias twice 11.7x,
       patch shift 133x, pos last 7.6x, x_mid ln 6.9x  -- all on the per-block check of the piece that holds the defect; against the
       whole-tower gates bias twice reaches only 2.9-3.4x and pos last 1.5-4.6x.
   gscale (f16 only): with the unit probe the image gradient is ~1e-2 and an UNSCALED f16 backward is as good as the scaled one (0.5-1.04x
   of the gates): not detectable by any unit-probe check.  The small-probe check (probe x 2^-14: gradients of the size a guidance run
   sees) catches it at 98-458x the whole-tower gate.
"""
import pytest
import torch

import _vit_ref64 as V
import _vit_routes as VR

DTYPES = ["bf16", "f16"]
NAMES = list(VR.ROWS)


def _ratios(checks, u):
    return [(st / (u * k ** 0.5), name, st, k) for name, st, k in checks]


# ---- 1. exactness ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_exact_tower_reproduces_oracle(name):
    from oracle import clip_vit
    cfg = VR.ROWS[name]["cfg"]
    sd, img, probe = VR.inputs(name)
    got = V.Tower(sd, cfg).run(img, probe)
    x = img.clone().requires_grad_(True)
    with torch.enable_grad():
        e = clip_vit.encode_images(sd, cfg, x, True, normalize=False)
        (torch.nn.functional.normalize(e) * probe).sum().backward()
    e_rel, g_rel = V.rel_l2(e.detach(), got["emb"]), V.rel_l2(x.grad, got["grad"])
    print(f"[bound] vit ref64 vs oracle {name}: emb rel-L2 {e_rel:.2e}, grad rel-L2 {g_rel:.2e}")
    assert e_rel <= 2e-6 and g_rel <= 4e-6           # the fp32 oracle's own noise (measured 5.9e-7 / 1.3e-6 at most)
    assert V.rel_l2(clip_vit.vit_forward(sd, cfg, (img - torch.tensor(V.MEAN).view(1, 3, 1, 1)) / torch.tensor(V.STD).view(1, 3, 1, 1), True),
                    got["emb"]) <= 2e-6


@pytest.mark.parametrize("tag,cfg", [("tiny", (32, 8, 64, 2, 1, 32)), ("tiny-odd", (28, 14, 128, 2, 2, 48))])
def test_exact_tower_reproduces_committed_fixture(tag, cfg, load_golden):
    from oracle import clip_vit
    from perceptor_amd.engine.vit import vit_state_dict_shapes
    from perceptor_amd.utils.synth import synth_state_dict
    g = load_golden(f"clip_vit_{tag}")
    sd = synth_state_dict(vit_state_dict_shapes(cfg), 0)
    emb, _ = V.Tower(sd, cfg).forward(clip_vit.resize(g["img"].double(), (cfg[0], cfg[0])))
    rel = V.rel_l2(emb, g["emb"])
    print(f"[bound] vit ref64 vs fixture clip_vit_{tag}: emb rel-L2 {rel:.2e}")
    assert rel <= 2e-6


def test_written_out_gradient_is_the_towers_vjp():
    """Tower.backward (written out, no autograd) against float64 autograd through Tower.forward, both exact-GELU and QuickGELU"""
    sd, img, probe = VR.inputs("tiny-odd")
    for quick in (True, False):
        ref = V.Tower(sd, VR.ROWS["tiny-odd"]["cfg"], quick_gelu=quick)
        want = ref.run(img, probe)["grad"]
        x = img.double().requires_grad_(True)
        with torch.enable_grad():
            emb, _ = ref.forward(x)
            (torch.nn.functional.normalize(emb) * probe.double()).sum().backward()
        assert V.rel_l2(want, x.grad) <= 1e-12


# ---- 2. routes -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_route_table(dtype):
    seen = {f: set() for f in VR.FLAGS}
    for name, row in VR.ROWS.items():
        got = VR.host_routes(row["cfg"], row["n"], dtype)
        assert got == row["routes"], (name, dtype, {f: got[f] for f in VR.FLAGS if got[f] != row["routes"][f]})
        for f in VR.FLAGS:
            seen[f].add(got[f])
    for f in VR.FLAGS:
        assert seen[f] == ({True} if f == "t_odd" else {True, False}), (f, seen[f])
    for g in range(1, 64):                       # t % 8 == 0 needs g^2 = 7 (mod 8)
        assert (g * g + 1) % 8 != 0
    # the flags in the combinations the engine's code paths need
    rows = [r["routes"] for r in VR.ROWS.values()]
    assert any(not r["flash"] and r["kp_pad"] for r in rows)                        # batched-GEMM attention with padded im2col rows
    assert any(r["flash"] and VR.geometry(x["cfg"], x["n"])["t"] > 256 for r, x in zip(rows, VR.ROWS.values()))   # > 8 key tiles
    assert any(r["m_small"] and not r["fused_fc"] and x["cfg"][2] % 256 == 0 for r, x in zip(rows, VR.ROWS.values()))   # unfused MLP at a wide layer
    assert any(r["slabs_pr"] and r["slabs_fc"] and not r["slabs_qkv"] for r in rows)
    assert any(not any(r[f] for f in ("fused_fc", "fused_pr", "slabs_pr", "slabs_fc", "slabs_qkv")) for r in rows)


# ---- 3. fp32 stand-in --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_fp32_stand_in_within_half_of_every_gate(name, dtype):
    row, u, gs, dt = VR.ROWS[name], V.U[VR.TD[dtype]], VR.GSCALE[dtype], VR.TD[dtype]
    R = row["routes"]
    sd, img, probe = VR.inputs(name)
    ref, whole = VR.reference(name, dtype)
    t32 = V.Tower(sd, row["cfg"], emulate=dt, work=torch.float32, flash=R["flash"], fused_mlp=R["fused_fc"], fused_mlp_bwd=R["fused_pr"])
    for tag, bwd, limit in (("fp32 arithmetic", None, 0.5), ("fp32 arithmetic + 16-bit backward tensors", dt, 1.0)):
        got = t32.run(img, probe, bwd=bwd, gscale=gs)
        checks = V.tower_checks(ref, img, probe, got, whole)
        small = t32.run(img, probe * V.SMALL_PROBE, bwd=bwd, gscale=gs)["grad"]
        checks.append(V.small_probe_check(ref, small, whole))
        worst = max(_ratios(checks, u))
        D = dict((n_, s_) for n_, s_, _ in checks)
        print(f"[bound] vit stand-in {name} {dtype} ({tag}): worst {worst[0]:.3f} of its gate ({worst[1]}: {worst[2] / u:.3f} u vs sqrt({worst[3]}) u); "
              f"tower emb rel-L2 {D['tower emb']:.2e}, grad rel-L2 {D['tower grad']:.2e}")
        for ratio, cname, st, k in _ratios(checks, u):
            assert ratio <= limit, (name, dtype, tag, cname, st / u, k)


# ---- 4. seeded defects ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_seeded_defects_exceed_twice_a_gate(name, dtype):
    u, gs, dt = V.U[VR.TD[dtype]], VR.GSCALE[dtype], VR.TD[dtype]
    _, img, probe = VR.inputs(name)
    ref, whole = VR.reference(name, dtype)
    for defect in V.DEFECTS:
        if defect == "gscale":
            if dtype != "f16":
                continue
            unit = max(_ratios(V.tower_checks(ref, img, probe, ref.run(img, probe, bwd=dt, gscale=gs, defect=defect), whole), u))
            assert unit[0] <= 2.0, unit            # (documented: no unit-probe check sees it)
            small = ref.run(img, probe * V.SMALL_PROBE, bwd=dt, gscale=gs, defect=defect)["grad"]
            checks = [V.small_probe_check(ref, small, whole)]
            clean = V.small_probe_check(ref, ref.run(img, probe * V.SMALL_PROBE, bwd=dt, gscale=gs)["grad"], whole)
            assert clean[1] <= 0.5 * u * clean[2] ** 0.5, clean
        else:
            checks = V.tower_checks(ref, img, probe, ref.run(img, probe, bwd=dt, gscale=gs, defect=defect), whole)
        best = max(_ratios(checks, u))
        print(f"[bound] vit defect {name} {dtype} '{defect}': {best[0]:.1f}x the gate of '{best[1]}'")
        assert best[0] > 2.0, (name, dtype, defect, best)
