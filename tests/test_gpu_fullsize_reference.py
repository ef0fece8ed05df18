"""GPU: the HIP engines against the REFERENCE's own outputs at the sizes the project is benchmarked on (BASELINE configs C1 ... C5).

The other full-size tests compare one HIP engine with another (test_gpu_fullsize_c2c3.py, test_gpu_mixed.py) or check properties
(test_gpu_fullsize.py, test_gpu_fullsize_c4.py); a defect all modes share at these sizes -- a halo fault in a tile config only large maps
select, a statistics overflow over 512 x 512 maps, a batch-index error in a route only batch 8 takes -- passes them.  The fixtures here come
from the reference's unmodified modules on the CPU (oracle/gen_golden.py: gen_fullsize; fp32, N = 1; float64 noise floor F <= 1e-4 per
fixture, tests/test_fullsize_golden_cpu.py), sampled so that every residue mod 64 of both axes, the image borders and the channel sums are
seen (tests/_fullsize_ref.py).

Batches: each engine runs at the benchmark's own batch, so the benchmark's routes are the ones compared -- ADM 256 px: 4, ADM 512 px: 8,
yfcc_2 512 px: 8, cc12m_1 256 px: 1, SD UNet: 8.  The fixture's input is one chain of the batch, NOT at index 0; the other chains are other
seeds at other timesteps, the fixture chain keeps its own t.  (cc12m_1 is benchmarked at batch 1: index 0 is the only one.)  The precise
engine runs at batch 2 (fixture chain at index 1), as test_gpu_mixed.py runs it: it is the yardstick mode, not a benchmarked one, and at
batch 8 x 512 px its hi + lo activations are four times the memory and time for the same kernels.

Bounds: none is new.
  precise                 test_gpu_precise._compare: 1e-3 absolute (2e-6 of the scale above |y| = 100)
  mixed (ADM)             1e-3 absolute (test_gpu_mixed.py)
  f16 / bf16 (ADM)        test_gpu_fullsize_c2c3.TOL_MAX x max|ref|
  f16 / bf16 yfcc_2@512   8e-3 / 6e-2 x max|ref| (test_gpu_fullsize_c2c3.py)
  f16 / bf16 cc12m_1      test_gpu_vdiff.TOL_MAX x max|ref| and TOL_L2
  SD f16                  test_gpu_sd.TOL["f16"]: 6e-3 x max|ref| and rel-L2 4e-3
  whole output            std and norm at rtol 5e-2 against the fixture's moments (as test_gpu_clip.py), channel sums at the element bound x the
                          element count (_fullsize_ref.compare says why not its square root)

Measured on MI355X: see DESIGN.md, "Full-size parity against the reference".
Engines are cached one at a time (the 558 M and 968 M models are packed once per mode); the cases are ordered by engine.
"""
import pytest
import torch

import _fullsize_ref as FS
from conftest import golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_ABS = 1e-3
BATCH = {("adm", 256): 4, ("adm", 512): 8, ("yfcc_2", 512): 8, ("cc12m_1", 256): 1}
_CACHE, _WEIGHTS = {}, {}


def _engine(net, mode):
    """one engine alive at a time"""
    if (net, mode) not in _CACHE:
        _CACHE.clear()
        torch.cuda.empty_cache()
        from perceptor_amd.utils.synth import synth_state_dict as synth

        def synth_state_dict(shapes, seed):          # the name-keyed weights of a net are drawn once for all its modes
            if net not in _WEIGHTS:
                _WEIGHTS.clear()
                _WEIGHTS[net] = synth(shapes, seed)
            return _WEIGHTS[net]

        if net == "adm":
            from perceptor_amd.engine import adm, adm_mixed
            cfg = adm.openimages_config()
            sd = synth_state_dict(adm.state_dict_shapes(cfg), 0)
            eng = adm_mixed.AdmMixedEngine(cfg, sd, DEV) if mode == "mixed" else adm.AdmEngine(cfg, sd, DEV, mode)
        elif net == "sd":
            from oracle import sd as osd
            from perceptor_amd.engine import sd
            cfg = sd.SdConfig(**osd.SD_V1.__dict__)
            eng = sd.SdUnetEngine(cfg, synth_state_dict(sd.unet_state_dict_shapes(cfg), 0), DEV, mode)
        else:
            from perceptor_amd.engine import vdiff
            spec = vdiff.yfcc2_spec() if net == "yfcc_2" else vdiff.cc12m1_spec()
            eng = vdiff.VDiffEngine(spec, synth_state_dict(vdiff.state_dict_shapes(spec), 0), DEV, mode)
        _CACHE[(net, mode)] = eng
    return _CACHE[(net, mode)]


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    _CACHE.clear()
    _WEIGHTS.clear()
    torch.cuda.empty_cache()


def _reference(name):
    """(fixture with the reference under y_*, its float64 noise floor F): the fp32 reference's values unless F missed 1e-4, in which case the
    floor file carries the float64 values and they are the reference (tools/gen_fullsize_floor64.py)"""
    g, f = golden(name), golden(name + "_floor64")
    if "y64_lat" in f:
        g = {**g, **{"y_" + k: f["y64_" + k] for k in ("lat", "rows", "cols")}, "ch_sum": f["ch_sum"]}
    return g, float(f["F"])


def _batch(g, n, pos, other_t):
    """n chains: the fixture's input (rebuilt from its seed, checksum asserted) at index pos, other seeds and timesteps elsewhere"""
    from perceptor_amd.utils.synth import seeded_noise
    shape = tuple(int(v) for v in g["x_shape"])
    x = torch.cat([FS.rebuild(shape, g["x_seed"], g["x_chk"]) if i == pos else seeded_noise(shape, 9100 + i) for i in range(n)])
    t = torch.stack([g["t"][0] if i == pos else torch.as_tensor(other_t[i % len(other_t)], dtype=g["t"].dtype) for i in range(n)])
    return ((x + 1) / 2).to(DEV), t.to(DEV)


def _precise_bound(scale):
    return TOL_ABS if scale <= 100 else 2e-6 * scale          # test_gpu_precise._compare


def _scale(g):
    return float(FS.fixture_vector(g).abs().max())


ADM_T = (900, 80, 450, 20, 700, 999, 250, 333)


@pytest.mark.parametrize("mode,res", [("precise", 256), ("precise", 512), ("mixed", 256), ("mixed", 512), ("f16", 256), ("f16", 512),
                                      ("bf16", 256), ("bf16", 512)])
def test_adm_standard_vs_reference(mode, res):
    """The shipped 'standard' ADM UNet at 256 px batch 4 (C2) and 512 px batch 8 (C5) against the reference's UNetModel.  mixed: every layer at
    >= 128 px must have taken the weights-direct route, so that a fallback passing by accident is not what was measured."""
    from perceptor_amd.engine import ops
    from test_gpu_fullsize_c2c3 import TOL_MAX
    g, f = _reference(f"adm_standard_{res}")
    n = 2 if mode == "precise" else BATCH[("adm", res)]
    pos = n - 1 if n == 2 else n // 2 + 1
    img, t = _batch(g, n, pos, ADM_T)
    eng = _engine("adm", mode)
    ops.MIXED_TRACE = [] if mode == "mixed" else None
    try:
        y = eng.forward(img, t)
        trace = ops.MIXED_TRACE
    finally:
        ops.MIXED_TRACE = None
    scale = _scale(g)
    bound = _precise_bound(scale) if mode == "precise" else TOL_ABS if mode == "mixed" else TOL_MAX[mode] * scale
    FS.compare(y[pos:pos + 1], g, int(g["stride"]), f"adm_standard_{res} x{n} (chain {pos}) {mode} vs reference golden (F={f:.1e})", bound)
    if mode == "mixed":
        assert all(r[0] == "wd" for r in trace if r[2][1] >= 128), [r for r in trace if r[0] != "wd" and r[2][1] >= 128]
        assert {r[1] for r in trace if r[0] == "wd"} == {"single", "dbl"} and sum(r[0] == "wd" for r in trace) >= (40 if res == 512 else 20)


@pytest.mark.parametrize("mode", ["precise", "f16", "bf16"])
def test_yfcc2_512_vs_reference(mode):
    """YFCC2Model at 512 px, batch 8 (C3).  No normalisation between its convolutions: the 16-bit bounds are those test_gpu_fullsize_c2c3.py
    holds these modes to at this size against the precise engine (8e-3 / 6e-2 of max|v|)."""
    g, f = _reference("vdiff_yfcc_2_512")
    n = 2 if mode == "precise" else BATCH[("yfcc_2", 512)]
    pos = n - 1 if n == 2 else 5
    img, t = _batch(g, n, pos, (0.9, 0.05, 0.3, 0.7, 0.45, 0.15, 0.8, 0.6))
    v = _engine("yfcc_2", mode).forward(img, t)
    scale = _scale(g)
    bound = _precise_bound(scale) if mode == "precise" else {"f16": 8e-3, "bf16": 6e-2}[mode] * scale
    FS.compare(v[pos:pos + 1], g, int(g["stride"]), f"yfcc_2@512 x{n} (chain {pos}) {mode} vs reference golden (F={f:.1e})", bound)


@pytest.mark.parametrize("mode", ["precise", "f16", "bf16"])
def test_cc12m1_256_vs_reference(mode):
    """The CLIP-conditioned CC12M1Model at 256 px, batch 1 as benchmarked (C1): the one chain is the fixture's."""
    from test_gpu_vdiff import TOL_L2, TOL_MAX
    g, f = _reference("vdiff_cc12m_1_256")
    img, t = _batch(g, 1, 0, (0.5,))
    v = _engine("cc12m_1", mode).forward(img, t, g["clip_embed"].to(DEV))
    scale = _scale(g)
    bound = _precise_bound(scale) if mode == "precise" else TOL_MAX[mode] * scale
    _, _, l2 = FS.compare(v, g, int(g["stride"]), f"cc12m_1@256 x1 {mode} vs reference golden (F={f:.1e})", bound)
    if mode != "precise":
        assert l2 <= TOL_L2[mode], l2


def test_sd_v1_unet_64_batch8_vs_reference():
    """The SD-v1 UNet at 64 x 64 latents with a 77-token context, UNet batch 8 (C4: 4 latents x the two CFG evaluations), f16 as the reference
    runs it, against the reference's vendored ldm UNetModel: the whole 4 x 64 x 64 output of the fixture chain (index 5)."""
    from perceptor_amd.utils.synth import seeded_noise
    from test_gpu_sd import TOL
    g = golden("sd_ldm_unet_v1_64")
    n, pos = 8, 5
    xs, cs = tuple(g["x_shape"].tolist()), tuple(g["ctx_shape"].tolist())
    x = torch.cat([FS.rebuild(xs, g["x_seed"], g["x_chk"]) if i == pos else seeded_noise(xs, 9200 + i) for i in range(n)])
    ctx = torch.cat([FS.rebuild(cs, g["ctx_seed"], g["ctx_chk"]) if i == pos else seeded_noise(cs, 9300 + i) for i in range(n)])
    t = torch.tensor([981, 20, 500, 250, 760, int(g["t"]), 100, 640])
    got = _engine("sd", "f16").forward(x.to(DEV), t.to(DEV), ctx.to(DEV))[pos:pos + 1].float().cpu()
    ref = g["eps"]
    scale = float(ref.abs().max())
    err, l2 = float((got - ref).abs().max()), float((got.double() - ref.double()).norm() / ref.double().norm())
    serr = float((FS.channel_sums(got) - g["ch_sum"]).abs().max())
    sbound = TOL["f16"][0] * scale * 64 * 64
    print(f"[parity] sd_v1 unet 64x64 x{n} (chain {pos}) f16 vs reference golden: max|err|={err:.3e} (scale {scale:.3f}), rel-L2={l2:.3e}, "
          f"max|channel-sum err|={serr:.3e} (bound {sbound:.3e})")
    assert err < TOL["f16"][0] * scale and l2 < TOL["f16"][1], (err, scale, l2)
    assert serr < sbound, (serr, sbound)
    assert torch.allclose(FS.moments(got)[:, 1:], g["y_mom"][:, 1:], rtol=5e-2, atol=0)
