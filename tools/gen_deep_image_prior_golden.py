"""Writes tests/golden/deep_image_prior_reference.npz: what the reference's own DeepImagePrior module computes, run unmodified on the CPU.

perceptor/models/deep_image_prior/deep_image_prior.py is loaded through oracle/_refimport.py with two more stand-ins set HERE (nothing under
oracle/ changes): lantern.module_device (the device of a module's first parameter) and an empty torchvision.ops carrying a DeformConv2d
attribute, which offset_type="none" never constructs.  The module is built with offset_type="none", cast to float64, loaded (strict) with the
name-keyed synthetic state dict of perceptor_amd.engine.dip.synthetic_state_dict -- the 1.86 M parameter values are regenerated from their
names by the tests, not stored -- and run in training mode on the seeded cases of tests/_dip_ref64.py.  Per case the file holds, in float64:
the picture, d loss / d latents for loss = sum(picture * cotangent) (every 4th channel and a seeded contraction of the whole tensor: all
of it would pass the repository's limit for one file), every BatchNorm's updated running statistics, the whole gradient of every
parameter of at most 4096 elements and, for the larger weights, one seeded contraction plus every 997th element.  The state dict's key names,
shapes and dtypes are stored once per n_scales.  Only numbers and names are written.

    python tools/gen_deep_image_prior_golden.py [--check]
"""
from __future__ import annotations

import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "deep_image_prior_reference.npz")

from oracle import _refimport as R                                  # noqa: E402
import _dip_ref64 as D                                              # noqa: E402
from perceptor_amd.engine import dip as E                           # noqa: E402


def _ref_class():
    R.install()
    sys.modules["lantern"].module_device = lambda m: next(m.parameters()).device
    ops = types.ModuleType("torchvision.ops")
    ops.DeformConv2d = None
    sys.modules["torchvision.ops"] = ops
    sys.modules["torchvision"].ops = ops
    R._shell("perceptor.models.deep_image_prior", os.path.join(R.REF_ROOT, "perceptor", "models", "deep_image_prior"))
    return R.ref("models.deep_image_prior.deep_image_prior").DeepImagePrior


def generate():
    cls = _ref_class()
    out = {}
    for case in D.CASES:
        ns, size, n = case
        torch.manual_seed(0)
        m = cls(shape=(D.CIN, size, size), offset_type="none", n_scales=ns).double()
        key = "keys_s%d" % ns
        if key not in out:
            sd0 = m.state_dict()
            out[key] = np.array(list(sd0))
            out["shapes_s%d" % ns] = np.array([",".join(map(str, v.shape)) for v in sd0.values()])
            out["dtypes_s%d" % ns] = np.array([str(v.dtype) for v in m.float().state_dict().values()])
            m = m.double()
        sd = E.synthetic_state_dict(ns, D.CIN)
        m.load_state_dict({k: (v.double() if torch.is_floating_point(v) else v) for k, v in sd.items()}, strict=True)
        m.train()
        lat32, cot32 = D.case_inputs(case)
        lat = lat32.double().requires_grad_(True)
        pic = m(lat)
        (pic * cot32.double()).sum().backward()
        c = D.case_name(case)
        out[c + "/out"] = pic.detach().numpy()
        out[c + "/dlatents4"] = lat.grad[:, ::4].contiguous().numpy()          # every 4th channel (the whole tensor would pass the size limit)
        out[c + "/dlatents_dot"] = D.contraction("latents", lat.grad)[0].numpy()
        for k, v in m.state_dict().items():
            if k.endswith(("running_mean", "running_var", "num_batches_tracked")):
                out[c + "/stat/" + k] = v.numpy()
        for k, p in m.named_parameters():
            if p.numel() <= D.SMALL:
                out[c + "/grad/" + k] = p.grad.numpy()
            else:
                s, smp = D.contraction(k, p.grad)
                out[c + "/dot/" + k] = s.numpy()
                out[c + "/sample/" + k] = smp.numpy()
    return out


def main():
    data = generate()
    buf = io.BytesIO()
    np.savez_compressed(buf, **data)
    raw = buf.getvalue()
    if "--check" in sys.argv:
        old = np.load(OUT)
        assert set(old.files) == set(data), set(old.files) ^ set(data)
        for k in data:
            assert np.array_equal(old[k], data[k]), k
        print("fixture matches")
        return
    assert len(raw) < 1 << 20, len(raw)
    with open(OUT, "wb") as f:
        f.write(raw)
    print(OUT, len(raw), "bytes,", len(data), "arrays")


if __name__ == "__main__":
    main()
