"""Noise floor of the full-size reference fixtures (tests/golden/adm_standard_{256,512}.npz, vdiff_yfcc_2_512.npz, vdiff_cc12m_1_256.npz):
the fp32 reference output against the float64 restatement of the same network (tests/_precise_grad_ref64.py: adm_forward, vdiff_forward) on the
same input, at the fixture's sampled positions.  Writes tests/golden/<fixture>_floor64.npz:

    F        max |fp32 reference - float64| over the sampled positions (condition, tests/test_fullsize_golden_cpu.py: F <= 1e-4, a tenth of
             the 1e-3 contract, so the fp32 fixture is a fine enough yardstick)
    F_sum    max over channels of |fp32 channel sum - float64 channel sum|
    ch_sum   float64 channel sums of the float64 output
    y64_*    only if F > 1e-4: the float64 values at the sampled positions, which the tests then use as that network's reference

CPU only, float64 convolutions: minutes per fixture, up to ~25 GB at 512 x 512.

    python tools/gen_fullsize_floor64.py [fixture ...]
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIXTURES = ("adm_standard_256", "adm_standard_512", "vdiff_yfcc_2_512", "vdiff_cc12m_1_256")
F_MAX = 1e-4


def forward64(name, g, x):
    import _precise_grad_ref64 as G
    from perceptor_amd.utils.synth import synth_state_dict
    if name.startswith("adm_"):
        from oracle import adm_unet as oa
        cfg = oa.openimages_config()
        sd = synth_state_dict(oa.state_dict_shapes(cfg), 0)
        return G.adm_forward(sd, cfg, x, g["t"], torch.float64)
    from oracle import vdiff as ov
    spec = ov.yfcc2_spec() if "yfcc_2" in name else ov.cc12m1_spec()
    sd = synth_state_dict(ov.state_dict_shapes(spec), 0)
    return G.vdiff_forward(sd, spec, x, g["t"], g.get("clip_embed"), torch.float64)


def main(names):
    import _fullsize_ref as FS
    for name in names:
        with np.load(os.path.join(ROOT, "tests", "golden", name + ".npz")) as z:
            g = {k: torch.from_numpy(z[k]) for k in z.files}
        x = FS.rebuild(g["x_shape"], g["x_seed"], g["x_chk"])
        t0 = time.time()
        with torch.no_grad():
            y = forward64(name, g, x)
        stride = int(g["stride"])
        v64 = FS.sampled_vector(y, stride)
        f = float((FS.fixture_vector(g).double() - v64).abs().max())
        f_sum = float((g["ch_sum"] - FS.channel_sums(y)).abs().max())
        print(f"{name}: F = {f:.3e}, F_sum = {f_sum:.3e}, scale {float(v64.abs().max()):.3f} ({time.time() - t0:.0f} s)", flush=True)
        out = dict(F=np.float64(f), F_sum=np.float64(f_sum), ch_sum=FS.channel_sums(y).numpy())
        if f > F_MAX:
            out.update({"y64_" + k: v.numpy() for k, v in FS.sample(y, stride).items()})
        np.savez_compressed(os.path.join(ROOT, "tests", "golden", name + "_floor64.npz"), **out)


if __name__ == "__main__":
    main(sys.argv[1:] or FIXTURES)
