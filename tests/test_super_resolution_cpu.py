"""CPU: the float64 restatement of the Real-ESRGAN RRDBNet path (tests/_rrdb_ref64.py) against the reference's own values
(tests/golden/super_resolution_reference.npz, tools/gen_super_resolution_golden.py), the state-dict mapping, every refusal of the public
classes, the resize tables the loss uses, and seeded defects at the GPU test's inputs."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _rrdb_ref64 as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "super_resolution_reference.npz")
NETS = ("x4", "x2", "x8")
NAME_TABLE = {"x2": (23, 2), "x4": (23, 4), "x8": (23, 8), "RealESRGAN_x4plus": (23, 4), "RealESRNet_x4plus": (23, 4),
              "RealESRGAN_x4plus_anime_6B": (6, 4), "RealESRGAN_x2plus": (23, 2)}


@pytest.fixture(scope="module")
def fx():
    return {k: torch.from_numpy(v) for k, v in np.load(FIXTURE).items()}


def _sd(blocks, scale, seed=0):
    from perceptor_amd.engine.rrdb import rrdb_state_dict_shapes
    from perceptor_amd.utils.synth import synth_state_dict
    return synth_state_dict(rrdb_state_dict_shapes(blocks, scale), seed, gain=2 ** 0.5)


# ---- restatement vs the reference's values -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NETS)
def test_restatement_matches_reference_network(fx, name):
    scale, blocks = (int(v) for v in fx[f"{name}_cfg"])
    x, ref = fx[f"{name}_in"], fx[f"{name}_out"]
    y = R.upsample64({k: v.double() for k, v in _sd(blocks, scale).items()}, x, scale, blocks)
    assert tuple(y.shape) == tuple(ref.shape) == (x.shape[0], 3, x.shape[2] * scale, x.shape[3] * scale)
    rel = R.rel_l2(y, ref)
    print(f"[fixture] {name}: restatement vs reference rel-L2 {rel:.3e}")
    assert rel <= 1e-10


@pytest.mark.parametrize("case", ("same", "resized"))
def test_restatement_matches_reference_loss(fx, case):
    x = fx[f"loss_{case}_in"]
    loss, grad, down, up = R.loss64({k: v.double() for k, v in _sd(1, 2).items()}, x, 1)
    ref = float(fx[f"loss_{case}_value"])
    rel = (abs(float(loss) - ref) / abs(ref), R.rel_l2(grad, fx[f"loss_{case}_grad"]), R.rel_l2(down, fx[f"loss_{case}_down"]),
           R.rel_l2(up, fx[f"loss_{case}_up"]))
    print(f"[fixture] loss {case}: value {rel[0]:.3e} gradient {rel[1]:.3e} down-sized {rel[2]:.3e} up-sampled {rel[3]:.3e}")
    assert max(rel) <= 1e-10
    assert tuple(up.shape[2:]) == (32, 24)


# ---- state dict -------------------------------------------------------------------------------------------------------------------------------
def test_state_dict_mapping_and_checkpoint_layouts(tmp_path):
    from perceptor_amd import models
    from perceptor_amd.engine.rrdb import map_state_dict, pack_rdb_weights, rrdb_state_dict_shapes
    sd = _sd(1, 8, seed=3)
    assert "conv_up3.weight" in sd and "conv_up3.weight" not in rrdb_state_dict_shapes(1, 4)
    assert rrdb_state_dict_shapes(1, 2)["conv_first.weight"] == (64, 12, 3, 3)
    assert rrdb_state_dict_shapes(2, 4)["body.1.rdb3.conv5.weight"] == (64, 192, 3, 3)
    other = {k: v + 1 for k, v in sd.items()}
    # precedence: params_ema, then params, then the bare dict
    for layout, want in (({"params_ema": sd, "params": other}, sd), ({"params": sd}, sd), (sd, sd)):
        got = map_state_dict(layout, 1, 8)
        assert list(got) == list(sd) and all(torch.equal(got[k], want[k]) for k in sd)
        path = tmp_path / "ckpt.pth"
        torch.save(layout, path)
        m = models.SuperResolution("x8", checkpoint=str(path), num_block=1)
        assert all(torch.equal(m.net.state_dict()[k], sd[k]) for k in sd)
    with pytest.raises(ValueError, match="missing"):
        map_state_dict({k: v for k, v in sd.items() if k != "conv_hr.bias"}, 1, 8)
    with pytest.raises(ValueError, match="unexpected"):
        map_state_dict(dict(sd, extra=torch.zeros(1)), 1, 8)
    with pytest.raises(ValueError, match="unexpected"):
        map_state_dict(sd, 1, 4)                             # conv_up3 on a scale-4 net
    with pytest.raises(ValueError, match="shape"):
        map_state_dict(dict(sd, **{"conv_last.weight": torch.zeros(3, 64, 1, 1)}), 1, 8)
    # fragment order: element [ch][tap][nb][q][r][j] = W[16 nb + r][32 ch + 8 q + j][ky][kx]
    w = torch.arange(64 * 96 * 9, dtype=torch.float32).reshape(64, 96, 3, 3)
    p = pack_rdb_weights(w).reshape(3, 9, 4, 4, 16, 8)
    for ch, tap, nb, q, r, j in ((0, 0, 0, 0, 0, 0), (2, 7, 3, 1, 15, 5), (1, 4, 2, 3, 9, 7)):
        assert p[ch, tap, nb, q, r, j] == w[16 * nb + r, 32 * ch + 8 * q + j, tap // 3, tap % 3]
    with pytest.raises(ValueError):
        pack_rdb_weights(torch.zeros(24, 64, 3, 3))


def test_names_and_refusals():
    from perceptor_amd import losses, models, transforms
    from perceptor_amd.engine.rrdb import RrdbEngine
    from perceptor_amd.models import super_resolution as msr
    assert msr.CONFIGS == NAME_TABLE
    for name, (blocks, scale) in NAME_TABLE.items():
        assert (blocks, scale) == msr.CONFIGS[name]
    m6 = models.SuperResolution("RealESRGAN_x4plus_anime_6B")
    assert (m6.num_block, m6.scale) == (6, 4) and len(m6.net.body) == 6
    m = models.SuperResolution("x2", num_block=1)
    assert m.scale == 2 and m.net.conv_first.weight.shape[1] == 12
    for name in ("RealESRGANv2-animevideo-xsx2", "RealESRGANv2-anime-xsx4", "RealESRGANv2-animevideo-xsx4-nousm"):
        with pytest.raises(NotImplementedError):
            models.SuperResolution(name)
    with pytest.raises(ValueError):
        models.SuperResolution("x3")
    with pytest.raises(ValueError):
        models.SuperResolution("x4", dtype="f32", num_block=1)
    with pytest.raises(ValueError):
        models.SuperResolution("x4", weights="pretrained", num_block=1)
    with pytest.raises(ValueError):
        RrdbEngine((64, 32, 1, 3), {}, "cpu")
    with pytest.raises(ValueError):
        RrdbEngine((48, 32, 1, 4), {}, "cpu")
    img = torch.zeros(1, 3, 8, 8)
    with pytest.raises(RuntimeError):
        m(img)
    with pytest.raises(RuntimeError):
        m.downsample(img)
    t = transforms.SuperResolution("x2", num_block=1)
    assert t.model.scale == 2
    with pytest.raises(RuntimeError):
        t.encode(img)
    with pytest.raises(RuntimeError):
        t.decode(img)
    loss = losses.SuperResolution(num_block=1)
    assert loss.pre_downscale == 2 and loss.mode == "bicubic" and loss.transform.model.name == "x2"
    assert losses.SuperResolution("x4", pre_downscale=3, num_block=1).pre_downscale == 3
    with pytest.raises(RuntimeError):
        loss(img)
    with pytest.raises(RuntimeError):
        loss.loss_and_grad(img)
    assert not hasattr(losses, "SuperResolutionDiscriminator")


# ---- tables ---------------------------------------------------------------------------------------------------------------------------------------
def _apply_band(x, idx, w, axis):
    """pmi_resize_apply on the CPU: out[j] = sum_t w[j][t] x[idx[j][t]] along ``axis`` (idx < 0 skipped)"""
    x = x.double().movedim(axis, -1)
    out = torch.zeros(x.shape[:-1] + (idx.shape[0],), dtype=torch.float64)
    for t in range(idx.shape[1]):
        ok = idx[:, t] >= 0
        out[..., ok] += x[..., idx[ok, t].long()] * w[ok, t].double()
    return out.movedim(-1, axis)


@pytest.mark.parametrize("sizes", [((36, 132), (9, 33)), ((18, 66), (9, 33)), ((40, 56), (7, 9)), ((8, 8), (8, 20)), ((5, 7), (5, 7))])
def test_bilinear_tables_match_interpolate(sizes):
    from perceptor_amd.transforms.resize import bilinear_tables
    (h, w), (oh, ow) = sizes
    x = torch.rand(2, 3, h, w, generator=torch.Generator().manual_seed(h * w), dtype=torch.float64)
    y = _apply_band(_apply_band(x, *bilinear_tables(h, oh), 2), *bilinear_tables(w, ow), 3)
    ref = F.interpolate(x, size=(oh, ow), mode="bilinear", align_corners=False)
    # the table's weights are fp32 values (2^-24 relative each) of convex combinations of values in [0, 1)
    assert float((y - ref).abs().max()) <= 4 * 2.0 ** -24


@pytest.mark.parametrize("case", ("same", "resized"))
def test_resample_tables_match_reference_resize(fx, case):
    """resize(resample="bicubic") as the loss uses it: the fp32 tap tables applied on the CPU against the reference's resize output.
    Bound: the tables' grid is fp32 at positions < 64 (a few roundings of half-ulp 2^-19: <= 2^-17), the cubic kernel's slope is at most
    1.5 and shrinking stretches it by the scale (< 1), so a weight is within 1.5 * 2^-17 of the float64 one; at most 9 taps of values in
    [0, 1): 9 * 1.5 * 2^-17 = 1.03e-4 per element."""
    from perceptor_amd.transforms.resize import _plan, band_tables
    x, ref = fx[f"loss_{case}_in"], fx[f"loss_{case}_down"]
    out_hw = tuple(ref.shape[2:])
    method, dims = _plan(x.shape[2], x.shape[3], out_hw, "bicubic")
    assert method == "cubic" and _plan(x.shape[2], x.shape[3], out_hw)[0] == "lanczos3" and _plan(8, 8, (4, 4), "lanczos3")[0] == "lanczos3"
    y = x.double()
    for _, axis, i, o in dims:
        idx, w, _, _ = band_tables(i, o, method)
        y = _apply_band(y, idx, w, axis)
    err = float((y - ref).abs().max())
    print(f"[tables] bicubic {tuple(x.shape[2:])} -> {out_hw}: max |table - reference| {err:.3e}")
    assert err <= 9 * 1.5 * 2.0 ** -17
    with pytest.raises(ValueError):
        _plan(8, 8, (4, 4), "nearest")


# ---- seeded defects at the GPU test's inputs ----------------------------------------------------------------------------------------------
DEFECT_NET = {d: "x4" for d in R.DEFECTS}
DEFECT_NET.update(unshuffle_order="x2", replicate_pad="x2", crop_wrong_side="x2")
_clean = {}


@pytest.mark.parametrize("defect", R.DEFECTS)
def test_seeded_defects_exceed_the_gate(fx, defect):
    """Each defect, in the emulated restatement at the input of test_gpu_rrdb.py's engine test, moves the output by more than twice that
    test's gate sqrt(R) u (bf16: the wider one)."""
    name = DEFECT_NET[defect]
    scale, blocks = (int(v) for v in fx[f"{name}_cfg"])
    sd = {k: v.double() for k, v in _sd(blocks, scale).items()}
    x = fx[f"{name}_in"]
    if name not in _clean:
        _clean[name] = R.upsample64(sd, x, scale, blocks, emulate="bf16")
    bad = R.upsample64(sd, x, scale, blocks, emulate="bf16", defect=defect)
    gate = math.sqrt(R.roundings(scale, blocks)["out"]) * R.U["bf16"]
    rel = R.rel_l2(bad, _clean[name]) / gate
    print(f"[defect] {defect} on {name}: {rel:.2f} x gate")
    assert rel > 2.0
