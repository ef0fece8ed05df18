"""Float64 input gradient of the shipped 558 M-parameter ADM UNet at 128 x 128 on the inputs of tests/golden/adm_standard_128_grad.npz, from the
dtype-generic restatement of the oracle in tests/_precise_grad_ref64.py (CPU, a few minutes, ~20 GB).  Writes
tests/golden/adm_standard_128_grad64.npz: g_sub = g[:, :, ::2, ::2] (float64), g_norm = |g|, F = rel-L2 of the fp32 fixture's g_sub against it
(the yardstick's own noise floor, tests/test_gpu_precise_backward.py).

    python tools/gen_adm_grad64_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import _precise_grad_ref64 as G
    from oracle import adm_unet as oa
    from perceptor_amd.engine import adm
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    with np.load(os.path.join(ROOT, "tests", "golden", "adm_standard_128_grad.npz")) as z:
        t, g_sub32 = torch.from_numpy(z["t"]), torch.from_numpy(z["g_sub"])
    sd = synth_state_dict(adm.state_dict_shapes(adm.openimages_config()), 0)
    x, probe = seeded_noise((1, 3, 128, 128), 32), seeded_noise((1, 3, 128, 128), 62)
    _, g = G.adm_grad(sd, oa.openimages_config(), x, t, probe, torch.float64)
    sub = g[:, :, ::2, ::2].contiguous()
    f = G.rel_l2(g_sub32, sub)
    print(f"adm_standard_128: F = {f:.3e}, |g| = {float(g.norm()):.9e}")
    np.savez(os.path.join(ROOT, "tests", "golden", "adm_standard_128_grad64.npz"), g_sub=sub.numpy(), g_norm=np.float64(g.norm()), F=np.float64(f))


if __name__ == "__main__":
    main()
