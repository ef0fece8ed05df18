"""CPU: the full-size reference fixtures (oracle/gen_golden.py: gen_fullsize, tools/gen_fullsize_floor64.py) that tests/test_gpu_fullsize_reference.py
compares the HIP engines with at the benchmark's own sizes.

  * integrity: shapes, finiteness, the sampled positions run through every residue mod 64 on both axes (so no power-of-two tile has an edge
    the fixture never reads), the float64 noise floor F of each fp32 fixture is <= 1e-4 (a tenth of the 1e-3 contract), moments and channel
    sums agree with the lattice to sampling accuracy;
  * the fp32 oracle reproduces adm_standard_256 at the sampled positions (the bound of test_oracle_golden.py for the 128 px fixture);
  * sensitivity: the comparison the GPU test applies (_fullsize_ref.compare) rejects a 2e-3 perturbation (twice the contract) of one tile-edge
    column, of one border row and of the ::32 lattice positions, on the float64 256 px forward -- and a comparison over y[:, :, ::32, ::32]
    alone, the slice first proposed for this check, accepts the tile-edge fault.
"""
import os

import pytest
import torch

import _fullsize_ref as FS
from conftest import GOLDEN, golden

FIXTURES = {"adm_standard_256": (6, 256), "adm_standard_512": (6, 512), "vdiff_yfcc_2_512": (3, 512), "vdiff_cc12m_1_256": (3, 256)}
F_MAX = 1e-4
NEW_FILES = [n + ".npz" for n in FIXTURES] + [n + "_floor64.npz" for n in FIXTURES] + ["sd_ldm_unet_v1_64.npz"]


@pytest.mark.parametrize("res", [256, 512])
def test_sampled_positions_cover_every_residue_mod_64(res):
    stride = FS.STRIDE[res]
    pos = FS.sampled_positions(res, stride)
    assert {p % 64 for p in range(0, res, stride)} == set(range(64))          # the lattice alone already does
    assert {0, 1, res - 2, res - 1} <= set(pos)
    # what the ::32 slice would have read: one residue
    assert {p % 32 for p in range(0, res, 32)} == {0}
    y = torch.arange(res * res, dtype=torch.float32).reshape(1, 1, res, res)
    s = FS.sample(y, stride)
    assert s["lat"].shape[-2:] == (len(range(0, res, stride)),) * 2 and s["rows"].shape[-2:] == (4, res) and s["cols"].shape[-2:] == (res, 4)
    assert FS.sampled_vector(y, stride).shape[2] == s["lat"][0, 0].numel() + 8 * res


def test_fixture_files_are_small():
    sizes = {f: os.path.getsize(os.path.join(GOLDEN, f)) for f in NEW_FILES}
    assert all(v < 512 * 1024 for v in sizes.values()), sizes
    assert sum(sizes.values()) < 2 * 1024 * 1024, sizes


@pytest.mark.parametrize("name", list(FIXTURES))
def test_fixture_integrity(name):
    c, res = FIXTURES[name]
    g = golden(name)
    stride = int(g["stride"])
    assert stride == FS.STRIDE[res] and tuple(g["x_shape"].tolist()) == (1, 3, res, res)
    k = len(range(0, res, stride))
    assert g["y_lat"].shape == (1, c, k, k) and g["y_rows"].shape == (1, c, 4, res) and g["y_cols"].shape == (1, c, res, 4)
    assert g["y_mom"].shape == (1, 3) and g["ch_sum"].shape == (1, c) and g["ch_sum"].dtype == torch.float64 and g["x_chk"].dtype == torch.float64
    for key in ("y_lat", "y_rows", "y_cols", "y_mom", "ch_sum", "x_chk", "t"):
        assert bool(torch.isfinite(g[key].double()).all()), key
    # the three samplings agree where they overlap: corners of the lattice are in the border rows and columns
    assert torch.equal(g["y_lat"][..., 0, :], g["y_rows"][..., 0, ::stride]) and torch.equal(g["y_lat"][..., :, 0], g["y_cols"][..., ::stride, 0])
    assert torch.equal(g["y_rows"][..., :, :2], g["y_cols"][..., FS.border_index(res), :2])
    # seeds, timesteps and the clip embedding differ from the 64-128 px fixtures'
    assert int(g["x_seed"]) not in (32, 41, 42) and float(g["t"]) not in (333.0, 0.3, 0.7)
    FS.rebuild(g["x_shape"], g["x_seed"], g["x_chk"])
    # moments and channel sums of the whole output against the lattice's, to sampling accuracy.  The outputs are spatially correlated (the
    # v-diffusion fields are smooth over tens of pixels), so the lattice mean's standard error is taken from the data: the spread of the
    # means of its 4 x 4 blocks, / sqrt(16); x 5 for the tails.  mean, std and norm of the whole output tie up exactly among themselves
    n = c * res * res
    mean, std, norm = (float(v) for v in g["y_mom"][0].double())
    assert abs(float(g["ch_sum"].sum()) / n - mean) <= 1e-5 * max(1.0, abs(mean)) + 1e-6
    assert abs((std ** 2 * (n - 1) / n + mean ** 2) ** 0.5 * n ** 0.5 - norm) <= 1e-5 * norm
    lat = g["y_lat"].double()
    b = k // 4
    blocks = lat[..., :4 * b, :4 * b].reshape(1, c, 4, b, 4, b).mean((3, 5)).flatten(2)
    stderr = blocks.std(2) / 4
    assert bool(((g["ch_sum"] / (res * res) - lat.mean((2, 3))).abs() <= 5 * stderr).all()), (g["ch_sum"] / (res * res), lat.mean((2, 3)), stderr)
    assert abs(float(lat.std()) / std - 1) <= 0.1 + abs(mean) / std
    # the yardstick's own noise floor
    f = golden(name + "_floor64")
    print(f"[floor] {name}: F = {float(f['F']):.3e}, F_sum = {float(f['F_sum']):.3e}")
    if "y64_lat" in f:       # F above the condition: the float64 values are this network's reference
        assert f["y64_lat"].shape == g["y_lat"].shape and f["y64_lat"].dtype == torch.float64
    else:
        assert float(f["F"]) <= F_MAX, float(f["F"])
    assert float((f["ch_sum"] - g["ch_sum"]).abs().max()) == pytest.approx(float(f["F_sum"]), rel=1e-9, abs=1e-12)
    # no condition of its own is set on F_sum (it is reported in DESIGN.md next to F): n elements each within F move a sum by at most n F
    assert float(f["F_sum"]) <= F_MAX * res * res


def test_sd_fixture_integrity():
    g = golden("sd_ldm_unet_v1_64")
    assert g["eps"].shape == (1, 4, 64, 64) and bool(torch.isfinite(g["eps"]).all()) and float(g["eps"].std()) > 1e-2
    assert int(g["t"]) != 981 and int(g["x_seed"]) != 71 and int(g["ctx_seed"]) != 72
    assert tuple(g["x_shape"].tolist()) == (1, 4, 64, 64) and tuple(g["ctx_shape"].tolist()) == (1, 77, 768)
    FS.rebuild(g["x_shape"], g["x_seed"], g["x_chk"])
    FS.rebuild(g["ctx_shape"], g["ctx_seed"], g["ctx_chk"])
    assert torch.allclose(FS.channel_sums(g["eps"]), g["ch_sum"], rtol=0, atol=1e-9) and torch.allclose(FS.moments(g["eps"]), g["y_mom"], rtol=1e-6)


@pytest.fixture(scope="module")
def adm256():
    from oracle import adm_unet
    from perceptor_amd.utils.synth import synth_state_dict
    g = golden("adm_standard_256")
    cfg = adm_unet.openimages_config()
    sd = synth_state_dict(adm_unet.state_dict_shapes(cfg), 0)
    x = FS.rebuild(g["x_shape"], g["x_seed"], g["x_chk"])
    return g, cfg, sd, x


def test_oracle_reproduces_adm_standard_256(adm256):
    """oracle/adm_unet.py (fp32) against the reference's own UNetModel at 256 x 256, sampled positions, moments and channel sums: the bound
    test_oracle_golden.py holds the 128 px fixture to (1e-5 of max(1, scale): same fp32 operations in another association order)."""
    from oracle import adm_unet
    g, cfg, sd, x = adm256
    y = adm_unet.adm_unet_forward(sd, cfg, x, g["t"])
    ref = FS.fixture_vector(g)
    scale = max(1.0, float(ref.abs().max()))
    err = float((FS.sampled_vector(y, int(g["stride"])).double() - ref.double()).abs().max())
    print(f"[parity] oracle adm_standard_256 vs reference golden: max|err|={err:.3e} (scale {scale:.3f})")
    assert err <= 1e-5 * scale, err
    assert float((FS.moments(y).double() - g["y_mom"].double()).abs().max()) <= 1e-5 * max(1.0, float(g["y_mom"].abs().max()))
    assert float((FS.channel_sums(y) - g["ch_sum"]).abs().max()) <= 1e-5 * scale * 256


def _rejects(y, g, stride, bound):
    try:
        FS.compare(y, g, stride, "sensitivity", bound)
    except AssertionError:
        return True
    return False


def test_comparison_rejects_tile_edge_border_and_lattice_faults(adm256):
    """The float64 256 px forward as a stand-in for an engine output: the GPU test's comparison accepts it at the contract bound, and rejects
    it once 2e-3 (twice the bound) is added to (i) one tile-edge column x = 31 (and, separately, to every column x = 31 mod 32), (ii) one
    border row, (iii) the positions y[:, :, ::32, ::32] reads.  A comparison over that slice alone accepts (i): it is blind to tile edges."""
    import _precise_grad_ref64 as G
    g, cfg, sd, x = adm256
    stride, bound, d = int(g["stride"]), 1e-3, 2e-3
    with torch.no_grad():
        y = G.adm_forward(sd, cfg, x, g["t"], torch.float64)
    assert not _rejects(y, g, stride, bound)
    # the element-wise part alone (sums taken from the perturbed tensor, so only the sampled positions can object): it carries every case here
    def elementwise_rejects(p):
        return _rejects(p, {**g, "ch_sum": FS.channel_sums(p.float())}, stride, bound)

    def slice32_accepts(p):
        return float((p[:, :, ::32, ::32] - y[:, :, ::32, ::32]).abs().max()) < bound

    one_col = y.clone()
    one_col[:, :3, :, 31] += d                       # eps channels, the last column of the first 32-wide tile
    assert elementwise_rejects(one_col)                                              # read by the border rows (31 is no multiple of 3)
    assert slice32_accepts(one_col)
    edge_cols = y.clone()
    edge_cols[:, :3, :, 31::32] += d
    assert _rejects(edge_cols, g, stride, bound) and elementwise_rejects(edge_cols)  # columns 63, 159, 255 are on the lattice
    assert slice32_accepts(edge_cols)
    interior = y.clone()
    interior[:, :3, 2:-2, 63] += d                   # a tile-edge column that stops short of the border rows: the lattice alone sees it
    assert elementwise_rejects(interior) and slice32_accepts(interior)
    row = y.clone()
    row[:, :3, 255, :] += d                          # the last row
    assert _rejects(row, g, stride, bound) and elementwise_rejects(row)
    row0 = y.clone()
    row0[:, :3, 0, :] += d
    assert elementwise_rejects(row0)
    lat32 = y.clone()
    lat32[:, :3, ::32, ::32] += d                    # what the ::32 slice reads: (0, 0), (0, 96), (96, 96) ... are on the stride-3 lattice too
    assert elementwise_rejects(lat32) and not slice32_accepts(lat32)
    # a single unsampled element off by 2e-3 is below what any sampled comparison can see; the channel sum moves by exactly that
    one = y.clone()
    one[0, 0, 100, 100] += d
    assert 100 % stride and not _rejects(one, g, stride, bound)
    assert float((FS.channel_sums(one) - FS.channel_sums(y)).abs().max()) == pytest.approx(d, rel=1e-6)
