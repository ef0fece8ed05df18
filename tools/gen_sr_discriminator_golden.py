"""Writes tests/golden/sr_discriminator_reference.npz: inputs and outputs of the reference's own UNetDiscriminatorSN
(perceptor/losses/super_resolution/unet_discriminator_sn.py) and of the loss of discriminator.py:28-29, -model(images).mean() * 0.001,
with autograd to the images, run unmodified on the CPU in float64 and in eval mode (no power iteration: u and v are used as stored).

The module file imports only torch and is loaded by path: the package's __init__ imports basicsr, which is not needed for it.  The
checkpoint is unreachable, so the weights are this package's synthetic ones (engine/disc.py: synth_disc_state_dict); they regenerate from
the seed and are not written -- only u and v travel, so that a test can tell a changed power iteration from a changed network.  With
``n_total`` the mean is taken over n_total H W (the loss of a shard): the reference's value times N / n_total.

    python tools/gen_sr_discriminator_golden.py [--check]
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "sr_discriminator_reference.npz")

from oracle import _refimport as R                                  # noqa: E402
from perceptor_amd.engine.disc import SN_LAYERS, synth_disc_state_dict   # noqa: E402

SEED = 0
CASES = {"f64": (64, (2, 3, 16, 24), None), "f32": (32, (1, 3, 8, 40), None), "f64_shard": (64, (2, 3, 16, 24), 6)}     # num_feat, images, n_total


def _arch():
    path = os.path.join(R.REF_ROOT, "perceptor", "losses", "super_resolution", "unet_discriminator_sn.py")
    spec = importlib.util.spec_from_file_location("_ref_unet_discriminator_sn", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def build():
    arch = _arch()
    out = {}
    for i, (name, (feat, shape, n_total)) in enumerate(CASES.items()):
        net = arch.UNetDiscriminatorSN(num_in_ch=3, num_feat=feat, skip_connection=True).double()
        sd = synth_disc_state_dict(feat, SEED)
        assert set(sd) == set(net.state_dict()), sorted(set(sd) ^ set(net.state_dict()))
        net.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        net.eval()
        net.requires_grad_(False)
        g = torch.Generator().manual_seed(100 + (i % 2))
        x = torch.rand(shape, generator=g, dtype=torch.float64).float().double().requires_grad_(True)
        logits = net(x)
        loss = -logits.mean() * 0.001
        if n_total is not None:
            loss = loss * (shape[0] / n_total)
        loss.backward()
        out[f"{name}_seed"] = np.int64(SEED)
        out[f"{name}_num_feat"] = np.int64(feat)
        out[f"{name}_n_total"] = np.int64(n_total or 0)
        out[f"{name}_in"] = x.detach().float().numpy()
        out[f"{name}_logits"] = logits.detach().numpy()
        out[f"{name}_loss"] = np.float64(loss.detach())
        out[f"{name}_grad"] = x.grad.numpy()
        for k in SN_LAYERS:
            out[f"{name}_conv{k}_u"] = sd[f"conv{k}.weight_u"].numpy()
            out[f"{name}_conv{k}_v"] = sd[f"conv{k}.weight_v"].numpy()
    return out


def main():
    new = build()
    if "--check" in sys.argv:
        with np.load(OUT) as z:
            assert sorted(z.files) == sorted(new), "keys differ"
            for k in z.files:
                assert np.array_equal(z[k], new[k]), k
        print("sr_discriminator_reference.npz is up to date")
        return
    np.savez_compressed(OUT, **new)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
