"""CPU: the teacher-forced float64 pieces of the CLIP ResNet tower (tests/_rn_ref64.py: Emu), the rows and routes of tests/_rn_routes.py and
the gates of tests/test_gpu_rn_tower.py, checked without a device.

1. Restatement.  Emu's written-out input gradient is the vjp of the emulated tower: it reproduces float64 autograd through
   _rn_ref64.tower(emulate=, masks=) to 1e-12, and Emu(emulate=None) the exact tower's embedding and gradient to the fp32 weights' 1e-6.
2. Routes.  The rows' pmi_igemm signatures (asked of the library's own host queries, nothing launched) cover those of the five product
   towers at n = 1, 2, 4, but for the entries of _rn_routes.UNREACHED, each of which names why no small shape reaches it and the full-size
   test whose tower takes it.
3. Stand-in.  The same pieces in fp32 arithmetic (torch's CPU convolutions: another accumulation order) with every 16-bit tensor of the
   forward AND the backward stored in 16 bit, the f16 loss scale included, stay within every gate at every row in both types.  A
   teacher-forced reference leaves the piece's last rounding out (store=False), so a k = 1 statistic is one rounding's relative error:
   at most u (1 - u) on a row that one element dominates, ~0.45 u on a wide row.  Measured (the [bound] lines): x0 (3 channels per pixel)
   0.94 .. 0.99 of its gate, the 8- and 16-channel maps of the width-16 rows 0.8 .. 0.97, k = 1 pieces of 32 channels and more <= 0.87,
   the attention pool 0.42 .. 0.46, blocks backward <= 0.58, whole-tower gradient 0.17 .. 0.22, embedding 0.04 .. 0.10, the small probe
   where the unit probe is.  The figures above 0.7 are k = 1 pieces with narrow rows: that is the count (one rounding cannot be counted
   lower), not a miscount.
   With the fixed f16 loss scale alone (gscale = 65536, what ResNetEngine.backward used before it chose a power of two from |d_emb|) the
   stand-in misses the small-probe gate at 2.07 of it (w80-r160): the gradient shrinks ~5000x from d_emb to the stem and lands among
   f16's subnormals.  test_f16_fixed_loss_scale_would_miss_the_small_probe keeps that measurement.
4. Seeded defects.  Each defect of _rn_ref64.DEFECTS exceeds TWICE the gate of at least one check at every row, in both types.  Smallest
   margins over the rows (bf16; f16: 8x these, the defects being absolute), each on the check of the piece that holds the defect:
       identity skip 222x, stem odd 480x, relu before add 180x, gs dropped 148x, pool bwd 0.25 109x, dq0 dropped 256x (the dq0 check),
       mean 1/HW 734x, pos shift 44x, attn scale 6222x (the P check), zero insert odd 1053x, std channel 14x, last pixel 126x
"""
import pytest
import torch

import _rn_ref64 as RN
import _rn_routes as RR

DTYPES = ["bf16", "f16"]
NAMES = list(RR.ROWS)


# ---- 1. restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w16-r64", "w16-r96-in"])
def test_written_out_gradient_is_the_towers_vjp(name):
    cfg = RR.ROWS[name]["cfg"]
    sd, img, probe = RR.inputs(name)
    ref, whole = RR.reference(name, "bf16")
    masks = RN.masks_of(whole)
    x = img.double().requires_grad_(True)
    with torch.enable_grad():
        emb = RN.tower(sd, cfg, RN.normalize(RN.resize64(x, (cfg[0], cfg[0])) if img.shape[-1] != cfg[0] else x), emulate=torch.bfloat16, masks=masks)
        (torch.nn.functional.normalize(emb) * probe.double()).sum().backward()
    assert RN.rel_l2(whole["emb"], emb.detach()) <= 1e-12 and RN.rel_l2(whole["grad"], x.grad) <= 1e-12
    assert torch.equal(ref.run(img, probe, masks=masks)["grad"], whole["grad"])          # its own masks pinned: the same run
    exact = RN.Emu(sd, cfg, None).run(img, probe)
    if img.shape[-1] == cfg[0]:
        e64, g64 = RN.encode_and_grad(sd, cfg, img, exact["d_emb"])
        assert RN.rel_l2(exact["emb"], e64) <= 1e-6 and RN.rel_l2(exact["grad"], g64) <= 1e-6     # (Emu holds its weights through fp32)


def test_depths_are_sums_of_k_over_the_blocks():
    cfg = RR.ROWS["w16-r64"]["cfg"]
    kinds = [(s, ds) for _, _, _, s, ds in RN.block_table(cfg)]
    assert kinds == [(1, True), (1, False), (2, True), (1, False), (2, True), (2, True)]      # ds, identity, s2, identity, s2, s2
    assert RN.depth_fwd(cfg) == 1 + 4 + (2 + 2) + (2 + 1) + (2 + 4) + (2 + 1) + (2 + 4) + (2 + 4) + 4
    assert RN.depth_grad(cfg) == RN.depth_fwd(cfg) + 2 + 1 + 2 + (4 + 3 + 4 + 3 + 4 + 4) + 1 + 2 + 1
    assert set(RN.FORWARD_DEFECTS) < set(RN.DEFECTS) and len(RN.DEFECTS) == 12


# ---- 2. routes ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_route_coverage(dtype):
    from perceptor_amd.engine import resnet
    assert [b[1:] for b in resnet.blocks(RR.ROWS["w16-r64"]["cfg"])] == RR.blocks(RR.ROWS["w16-r64"]["cfg"])
    rows = set()
    for name, row in RR.ROWS.items():
        sigs = RR.host_routes(row["cfg"], row["n"], dtype)
        assert len(sigs) == len(RR.igemm_calls(row["cfg"], row["n"]))
        rows |= set(sigs)
    product, x64 = set(), set()
    for name, cfg in resnet.RN_CONFIGS.items():
        for n in (1, 2, 4):
            sigs = set(RR.host_routes(cfg, n, dtype))
            product |= sigs
            if name == "RN50x64":
                x64 |= sigs
    missing = product - rows - set(RR.UNREACHED)
    print(f"[bound] rn routes {dtype}: {len(rows)} signatures at the rows, {len(product)} at the product towers, {len(product - rows)} unreached")
    assert not missing, f"product signatures no row reaches and UNREACHED does not explain: {sorted(missing, key=str)}"
    for sig, (why, test) in RR.UNREACHED.items():
        assert sig in product, f"{sig} is no product signature any more: drop it from UNREACHED"
        assert sig not in rows, f"{sig} is reached by a row now: drop it from UNREACHED"
        assert why and test == RR._X64 and sig in x64, sig
    # the properties the rows were chosen for
    kinds = lambda row: {(s, ds) for _, _, s, ds in RR.blocks(row["cfg"])}
    assert all(kinds(r) == {(1, True), (1, False), (2, True)} for r in RR.ROWS.values())
    assert {r["cfg"][2] for r in RR.ROWS.values()} >= {16, 64, 80} and {r["cfg"][0] for r in RR.ROWS.values()} >= {64, 96, 160}
    assert {r["n"] for r in RR.ROWS.values()} == {1, 3} and any(r["in_hw"] != (r["cfg"][0],) * 2 for r in RR.ROWS.values())
    assert any(r["n"] * (r["cfg"][0] // 32) ** 2 < 64 for r in RR.ROWS.values())
    assert any(s[3] and s[5] for s in rows) and any(s[3] and not s[5] for s in rows)          # split-K on both GEMM families
    assert any(s[1] == 9 and s[5] for s in rows) and any(s[2] for s in rows) and any(s[7] and s[5] for s in rows) and any(s[7] and not s[5] for s in rows)


# ---- 3. fp32 stand-in ----------------------------------------------------------------------------------------------------------------------
def _stand_in_checks(name, dtype, defect=None, work=torch.float32, whole_tower=True):
    row, dt, gs = RR.ROWS[name], RR.TD[dtype], RR.GSCALE[dtype]
    sd, img, probe = RR.inputs(name)
    ref, whole = RR.reference(name, dtype)
    run = RN.Emu(sd, row["cfg"], dt, work=work, defect=defect)
    got = run.run(img, probe, bwd=dt, gscale=gs, auto_scale=dtype == "f16")
    if not whole_tower:
        return RN.tower_checks(ref, img, got)
    pinned = ref.run(img, probe, masks=RN.masks_of(got))
    checks = RN.tower_checks(ref, img, got, whole, pinned)
    small = run.run(img, probe * RN.SMALL_PROBE, bwd=dt, gscale=gs, auto_scale=dtype == "f16")
    checks.append(RN.small_probe_check(ref, small["grad"], pinned))
    return checks


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_fp32_stand_in_within_every_gate(name, dtype):
    u = RN.U[RR.TD[dtype]]
    rs = sorted(RN.ratios(_stand_in_checks(name, dtype), u), reverse=True)
    D = {n_: r for r, n_, _, _ in rs}
    print(f"[bound] rn stand-in {name} {dtype}: worst " + ", ".join(f"{n_} {r:.2f}" for r, n_, _, _ in rs[:4])
          + f"; tower emb {D['tower emb']:.2f}, grad {D['tower grad']:.2f}, small probe {D['tower grad, small probe']:.2f}; above 0.7: "
          + (", ".join(n_ for r, n_, _, _ in rs if r > 0.7) or "none"))
    for ratio, cname, st, k in rs:
        assert ratio <= 1.0, (name, dtype, cname, st / u, k)


def test_f16_fixed_loss_scale_would_miss_the_small_probe():
    """why ResNetEngine.backward chooses its power of two from |d_emb|: with gscale = 65536 alone the gradients of the stem are f16
    subnormals under the small probe, and the stand-in misses the whole-tower gate (measured 2.07 of it at w80-r160)"""
    name, dt = "w80-r160", torch.float16
    sd, img, probe = RR.inputs(name)
    ref, whole = RR.reference(name, "f16")
    small = RN.Emu(sd, RR.ROWS[name]["cfg"], dt, work=torch.float32).run(img, probe * RN.SMALL_PROBE, bwd=dt, gscale=65536.0)
    name_, st, k = RN.small_probe_check(ref, small["grad"], ref.run(img, probe, masks=RN.masks_of(small)))
    print(f"[bound] rn stand-in {name} f16, fixed scale 65536: small probe {st / (RN.U[dt] * k ** 0.5):.2f} of its gate")
    assert st > RN.U[dt] * k ** 0.5


# ---- 4. seeded defects ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", NAMES)
def test_seeded_defects_exceed_twice_a_gate(name, dtype):
    u = RN.U[RR.TD[dtype]]
    for defect in RN.DEFECTS:
        best = max(RN.ratios(_stand_in_checks(name, dtype, defect, work=torch.float64, whole_tower=False), u))
        print(f"[bound] rn defect {name} {dtype} '{defect}': {best[0]:.1f}x the gate of '{best[1]}'")
        assert best[0] > 2.0, (name, dtype, defect, best)
