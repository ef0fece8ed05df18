"""CPU: the float64 restatement of the Real-ESRGAN discriminator path (tests/_disc_ref64.py) against the reference's own values
(tests/golden/sr_discriminator_reference.npz), the host-side pieces of engine/disc.py (sigma folding, phase packing, state-dict checks,
eligibility), the public class's argument errors, and the seeded defects at the engine test's inputs.

Seeded defects: each must move the emulated restatement's loss or gradient by more than 2 x the gate the GPU engine test holds the engine
to (rel-L2 sqrt(R) u, R = 20 for the loss and 19 for the gradient); the multiples are printed and recorded in DESIGN.md section 23.
"""
import math

import pytest
import torch
import torch.nn.functional as F

import _disc_ref64 as R
from conftest import golden

CASES = ("f64", "f32", "f64_shard")


@pytest.fixture(scope="module")
def fx():
    return golden("sr_discriminator_reference")


def _sd(feat, seed=0):
    from perceptor_amd.engine.disc import synth_disc_state_dict
    return synth_disc_state_dict(feat, seed)


# ---- restatement vs the reference ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_restatement_vs_fixture(fx, case):
    feat, n_total = int(fx[f"{case}_num_feat"]), int(fx[f"{case}_n_total"]) or None
    sd = _sd(feat, int(fx[f"{case}_seed"]))
    for k in R.SN:
        assert torch.equal(sd[f"conv{k}.weight_u"], fx[f"{case}_conv{k}_u"]) and torch.equal(sd[f"conv{k}.weight_v"], fx[f"{case}_conv{k}_v"])
    logits, loss, grad = R.net64(sd, fx[f"{case}_in"], n_total=n_total)
    ref = float(fx[f"{case}_loss"])
    rl, rv, rg = R.rel_l2(logits, fx[f"{case}_logits"]), abs(float(loss) - ref) / abs(ref), R.rel_l2(grad, fx[f"{case}_grad"])
    print(f"[measure] restatement vs fixture {case}: logits {rl:.3e}, loss {rv:.3e}, gradient {rg:.3e}")
    assert max(rl, rv, rg) <= 1e-14


@pytest.mark.parametrize("dtype", ("bf16", "f16"))
@pytest.mark.parametrize("case", CASES)
def test_emulated_restatement_vs_fixture(fx, case, dtype):
    """The figures behind the GPU test's FIXTURE_TOL (2 x these): they are re-measured here and must still be the recorded ones, within the
    factor 2 the tolerance itself allows."""
    from test_gpu_sr_discriminator import FIXTURE_TOL
    feat, n_total = int(fx[f"{case}_num_feat"]), int(fx[f"{case}_n_total"]) or None
    x = fx[f"{case}_in"]
    count = (n_total or x.shape[0]) * x.shape[2] * x.shape[3]
    logits, loss, grad = R.net64(_sd(feat), x, n_total=n_total, emulate=dtype, fused=R.fused_layers(feat), gscale=R.grad_scale(dtype, count))
    ref = float(fx[f"{case}_loss"])
    got = (R.rel_l2(logits, fx[f"{case}_logits"]), abs(float(loss) - ref) / abs(ref), R.rel_l2(grad, fx[f"{case}_grad"]))
    print(f"[measure] emulated {dtype} vs fixture {case}: logits {got[0]:.6e}, loss {got[1]:.6e}, gradient {got[2]:.6e}")
    for g, tol in zip(got, FIXTURE_TOL[(case, dtype)]):
        assert 0.25 * tol <= g <= tol


# ---- host-side pieces --------------------------------------------------------------------------------------------------------------------
def test_sigma_folding_equals_torch_eval_mode():
    from perceptor_amd.engine.disc import disc_state_dict_shapes, fold_sigma, map_state_dict
    sd = _sd(32)
    W = fold_sigma(map_state_dict(sd, 32), 32)
    for k in R.SN:
        cout, cin, ks, _ = disc_state_dict_shapes(32)[f"conv{k}.weight_orig"]
        conv = torch.nn.utils.spectral_norm(torch.nn.Conv2d(cin, cout, ks, 2 if ks == 4 else 1, 1, bias=False)).double()
        conv.load_state_dict({n: sd[f"conv{k}.{n}"].double() for n in ("weight_orig", "weight_u", "weight_v")})
        conv.eval()
        conv(torch.zeros((1, cin, 8, 8), dtype=torch.float64))
        assert float((conv.weight.detach() - W[f"conv{k}.weight"]).abs().max()) == 0.0, k
        assert 0.5 < float(torch.linalg.matrix_norm(W[f"conv{k}.weight"].reshape(cout, -1), 2)) < 1.25          # 8 power iterations: sigma is near the largest singular value
    # the restatement's own fold agrees
    W2, b0, b9 = R.fold64(sd)
    assert all(torch.equal(W2[k], W[f"conv{k}.weight"]) for k in range(10)) and torch.equal(b0, W["conv0.bias"]) and torch.equal(b9, W["conv9.bias"])


def test_phase_packing_vs_conv_transpose2d():
    from perceptor_amd.engine.disc import convt_phase_weights, pack_convt_weights
    g = torch.Generator().manual_seed(3)
    w = torch.randn((64, 32, 4, 4), generator=g, dtype=torch.float64)
    x = torch.randn((2, 3, 5, 64), generator=g, dtype=torch.float64)
    ref = F.conv_transpose2d(x.permute(0, 3, 1, 2), w, stride=2, padding=1).permute(0, 2, 3, 1)
    assert float((R.convt_phase(x, w) - ref).abs().max()) <= 1e-13
    P = convt_phase_weights(w)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    out = torch.zeros_like(ref)
    for a in (0, 1):
        for b in (0, 1):
            out[:, a::2, b::2] = sum(xp[:, a + u:a + u + 3, b + v:b + v + 5] @ P[a, b, u, v] for u in (0, 1) for v in (0, 1))
    assert float((out - ref).abs().max()) <= 1e-13
    # fragment order: [Cin / 16][phase][Cout / 32][2u + v][q][r][j] = W[32 chunk + 8 q + j][16 block + r][ky][kx]
    packed = pack_convt_weights(w).reshape(2, 4, 2, 4, 4, 16, 8)
    for blk, ph, ch, uv, q, r, j in ((0, 0, 0, 0, 0, 0, 0), (1, 3, 1, 2, 3, 15, 7), (1, 1, 0, 3, 2, 5, 1), (0, 2, 1, 1, 1, 9, 6)):
        a, b, u, v = ph >> 1, ph & 1, uv >> 1, uv & 1
        assert packed[blk, ph, ch, uv, q, r, j] == w[32 * ch + 8 * q + j, 16 * blk + r, R.ky(a, u), R.ky(b, v)]
    with pytest.raises(ValueError):
        pack_convt_weights(torch.zeros(48, 32, 4, 4))
    with pytest.raises(ValueError):
        convt_phase_weights(torch.zeros(64, 32, 3, 3))


def test_state_dict_errors():
    from perceptor_amd.engine.disc import disc_state_dict_shapes, map_state_dict
    sd = _sd(32)
    assert list(map_state_dict(sd, 32)) == list(disc_state_dict_shapes(32)) == list(map_state_dict({"params": sd}, 32))
    with pytest.raises(ValueError, match="missing"):
        map_state_dict({k: v for k, v in sd.items() if k != "conv3.weight_u"}, 32)
    with pytest.raises(ValueError, match="unexpected"):
        map_state_dict({**sd, "conv1.weight": sd["conv1.weight_orig"]}, 32)
    with pytest.raises(ValueError, match="shape"):
        map_state_dict({**sd, "conv2.weight_v": sd["conv2.weight_v"][:-1]}, 32)
    with pytest.raises(ValueError, match="shape"):
        map_state_dict(sd, 64)


def test_public_class_argument_errors():
    from perceptor_amd import losses
    from perceptor_amd.losses.super_resolution_discriminator import SuperResolutionDiscriminator
    with pytest.raises(ValueError, match="unknown name"):
        SuperResolutionDiscriminator("RealESRGAN_x2plus_netD")
    with pytest.raises(ValueError):
        SuperResolutionDiscriminator(weights="pretrained")
    with pytest.raises(ValueError):
        SuperResolutionDiscriminator(num_feat=48)
    with pytest.raises(ValueError):
        SuperResolutionDiscriminator(num_feat=96)
    loss = SuperResolutionDiscriminator(num_feat=32)
    assert isinstance(loss, losses.LossInterface) and isinstance(loss.model, torch.nn.Module)
    sd = loss.model.state_dict()
    ref = _sd(32)
    assert list(sd) == list(ref) and all(torch.equal(sd[k], ref[k]) for k in ref)
    assert not any(p.requires_grad for p in loss.model.parameters())
    with pytest.raises(ValueError, match="multiples of 8"):
        loss(torch.zeros((1, 3, 12, 20)))
    with pytest.raises(ValueError, match="multiples of 8"):
        loss.loss_and_grad(torch.zeros((1, 3, 16, 20)))
    for call in (loss, loss.loss_and_grad, loss.logits):
        with pytest.raises(RuntimeError, match="HIP device"):
            call(torch.zeros((1, 3, 16, 24)))


def test_eligibility_table():
    from perceptor_amd import _hip
    q = _hip.lib().pmi_convt4x4s2_eligible                     # (Cout, Cin, ldg, ldd, ldr, ldy, images, h, w, dtype)
    for f in (32, 64):                                         # the three adjoints of an image of 1024 x 1024, R and Y present
        for cout, cin, hw in ((2 * f, f, 512), (4 * f, 2 * f, 256), (8 * f, 4 * f, 128)):
            assert q(cout, cin, cout, cin, cin, cin, 1, hw, hw, 0) == 1 and q(cout, cin, cout, cin, cin, cin, 1, hw, hw, 1) == 1
    assert q(768, 384, 768, 384, 0, 0, 1, 128, 128, 0) == 0    # num_feat 96: conv3's Cout is beyond 512
    assert q(64, 32, 64, 32, 0, 0, 1, 1, 1, 0) == 1            # any h, w >= 1
    assert q(512, 256, 512, 256, 0, 0, 2, 2, 3, 1) == 1
    assert q(544, 256, 544, 256, 0, 0, 1, 4, 4, 0) == 0        # Cout beyond 512
    assert q(64, 48, 64, 48, 0, 0, 1, 4, 4, 0) == 0            # Cin no multiple of 32
    assert q(48, 32, 48, 32, 0, 0, 1, 4, 4, 0) == 0            # Cout no multiple of 32
    assert q(64, 32, 68, 32, 0, 0, 1, 4, 4, 0) == 0            # a pitch that is no multiple of 8
    assert q(64, 32, 64, 32, 24, 0, 1, 4, 4, 0) == 0           # R narrower than Cin
    assert q(64, 32, 64, 32, 0, 0, 1, 4, 4, 2) == 0            # the precise mode has no such kernel
    assert q(64, 32, 64, 32, 0, 0, 40000, 4, 4, 0) == 0        # more (image, phase) pairs than grid.z holds
    assert q(512, 256, 512, 256, 0, 0, 1, 2048, 1024, 0) == 0  # one image of g beyond a buffer resource
    from perceptor_amd.engine.disc import rdb_takes
    assert R.fused_layers(32) == (5, 6, 7, 8) and R.fused_layers(64) == (6, 7, 8) and R.fused_layers(96) == ()
    assert rdb_takes(128, 64) and rdb_takes(32, 32) and not rdb_takes(64, 128) and not rdb_takes(256, 64) and not rdb_takes(96, 96)


def test_kernel_mask_operand_has_no_ambiguous_sign():
    """The kernel tests' Y comes from the "mixed" regime: every |y| is at least 2^-7, far above the rounding unit of either type and f16's
    subnormal range, so the share of the mask that would have to be excluded is 0 (the issue's limit: 1 %)."""
    for dtype in ("bf16", "f16"):
        _, _, _, y = R.convt_operands((3, 8, 33), 64, 32, 11, "mixed", dtype, with_y=True)
        assert float(y.abs().min()) >= 2.0 ** -7
        assert float((y.abs() < R.U[dtype]).double().mean()) == 0.0


# ---- seeded defects ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ("bf16", "f16"))
@pytest.mark.parametrize("feat,shape", R.ENGINE_CASES[:1] + R.ENGINE_CASES[3:])
def test_seeded_defects_exceed_twice_the_gate(feat, shape, dtype):
    sd, x = _sd(feat), R.engine_inputs(shape)
    n = shape[0]
    gate_v, gate_g = math.sqrt(R.ROUNDINGS["logits"]) * R.U[dtype], math.sqrt(R.ROUNDINGS["grad"]) * R.U[dtype]
    kw = dict(emulate=dtype, fused=R.fused_layers(feat))
    clean = {nt: R.net64(sd, x, n_total=nt, gscale=R.grad_scale(dtype, (nt or n) * shape[2] * shape[3]), **kw) for nt in (None, 3 * n)}
    for defect in R.DEFECTS:
        nt = 3 * n if defect == "mean_n" else None
        _, loss, grad = R.net64(sd, x, n_total=nt, defect=defect, gscale=R.grad_scale(dtype, (nt or n) * shape[2] * shape[3]), **kw)
        _, loss0, grad0 = clean[nt]
        mv, mg = abs(float(loss) - float(loss0)) / abs(float(loss0)) / gate_v, R.rel_l2(grad, grad0) / gate_g
        print(f"[defect] F={feat} {shape} {dtype} {defect}: loss moves {mv:.1f} gates, gradient {mg:.1f} gates")
        assert max(mv, mg) > 2.0, defect
