"""Writes tests/golden/super_resolution_reference.npz: inputs and outputs of the reference's own CustomRRDBNet
(perceptor/models/super_resolution/custom_rrdbnet_arch.py), RealESRGANer.enhance (real_esrganer.py) and losses.SuperResolution.forward
(perceptor/losses/super_resolution/super_resolution.py) + autograd, run unmodified on the CPU in float64 (torch's default dtype is set
to float64 while the reference runs, so its resize grids and scale factors are float64 too).

The checkpoints are unreachable and 23 blocks would make a large fixture, so the networks are tiny ones (1-2 blocks) with this package's
synthetic weights (utils.synth, gain sqrt(2)).  Stand-ins cover downloads and constructors only:
  * RealESRGANer loads its weights from ``model_path``: a temporary checkpoint file, written in the {"params_ema": ...} layout;
  * the reference's models.SuperResolution / transforms.SuperResolution constructors download and need basicsr and huggingface_hub: the
    loss gets a stand-in transform whose ``.model`` holds the tiny net (``scale``, ``upsample`` = RealESRGANer.enhance with tile = 0,
    pre_pad = 0, as models.SuperResolution builds it) and whose call is ``model.upsample``.  The reference's ``upsample`` ends in
    ``.float()`` and its loss asks for half = True: both are precision choices left out here, the fixture is float64 throughout.
No arithmetic of the reference is replaced.  Only numbers are written; needs the reference tree (oracle/_refimport.py).  Deterministic.

    python tools/gen_super_resolution_golden.py [--check]
"""
from __future__ import annotations

import importlib
import io
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "super_resolution_reference.npz")

from oracle import _refimport as R                                  # noqa: E402
from perceptor_amd.engine.rrdb import rrdb_state_dict_shapes        # noqa: E402
from perceptor_amd.utils.synth import synth_state_dict              # noqa: E402

SEED, GAIN = 0, 2 ** 0.5
NETS = {"x4": (4, 2, (2, 3, 9, 33)), "x2": (2, 1, (1, 3, 9, 33)), "x8": (8, 1, (1, 3, 5, 7))}          # scale, blocks, input
LOSSES = {"same": (2, 3, 32, 24), "resized": (2, 3, 33, 25)}                                              # loss "x2", 1 block


def _modules():
    R.install()
    base = os.path.join(R.REF_ROOT, "perceptor")
    R._shell("perceptor.models.super_resolution", os.path.join(base, "models", "super_resolution"))
    arch = importlib.import_module("perceptor.models.super_resolution.custom_rrdbnet_arch")
    esr = importlib.import_module("perceptor.models.super_resolution.real_esrganer")
    return arch, esr


def _upsampler(arch, esr, scale, blocks, tmp):
    net = arch.CustomRRDBNet(num_in_ch=3, num_out_ch=3, num_feat=64, num_block=blocks, num_grow_ch=32, scale=scale).double()
    sd = synth_state_dict(rrdb_state_dict_shapes(blocks, scale), SEED, gain=GAIN)
    assert list(sd) == list(net.state_dict())
    path = os.path.join(tmp, f"x{scale}_{blocks}.pth")
    torch.save({"params_ema": {k: v.double() for k, v in sd.items()}}, path)
    net.eval()
    net.requires_grad_(False)
    up = esr.RealESRGANer(scale=scale, model_path=path, model=net, tile=0, tile_pad=10, pre_pad=0, half=False)
    up.device = torch.device("cpu")
    up.model = up.model.to("cpu")
    return net, up


def _ref_loss(up, scale):
    base = os.path.join(R.REF_ROOT, "perceptor")
    R._shell("perceptor.losses", os.path.join(base, "losses"))
    R._shell("perceptor.losses.super_resolution", os.path.join(base, "losses", "super_resolution"))
    tr = sys.modules["perceptor.transforms"]
    tr.resize = R.ref("transforms.resize.resize_right").resize
    model = types.SimpleNamespace(scale=scale, upsample=lambda image: up.enhance(image, outscale=scale))

    class SuperResolution:                       # the constructor stand-in (module doc)
        def __init__(self, name="x4", half=False):
            self.name, self.model = name, model

        def __call__(self, images):
            return self.model.upsample(images)

    tr.SuperResolution = SuperResolution
    sys.modules["perceptor"].transforms = tr
    mod = importlib.import_module("perceptor.losses.super_resolution.super_resolution")
    return mod.SuperResolution(name="x2", half=False)


def generate():
    torch.set_default_dtype(torch.float64)
    try:
        arch, esr = _modules()
        g = np.random.Generator(np.random.Philox(key=777))
        img = lambda shape: torch.from_numpy(g.random(shape, dtype=np.float32)).double()
        out = {"seed": torch.tensor(SEED), "gain": torch.tensor(GAIN)}
        with tempfile.TemporaryDirectory() as tmp:
            for name, (scale, blocks, shape) in NETS.items():
                net, up = _upsampler(arch, esr, scale, blocks, tmp)
                x = img(shape)
                y = up.enhance(x, outscale=scale)
                assert tuple(y.shape[2:]) == (shape[2] * scale, shape[3] * scale)
                out[f"{name}_cfg"] = torch.tensor([scale, blocks])
                out[f"{name}_in"], out[f"{name}_out"] = x.float(), y
                if scale != 2:                   # the bare network on the same input (scale 2 needs even sizes: enhance pads)
                    assert torch.equal(net(x), y)
            net, up = _upsampler(arch, esr, 2, 1, tmp)
            loss = _ref_loss(up, 2)
            for name, shape in LOSSES.items():
                x = img(shape).requires_grad_(True)
                val = loss.forward(x)
                (grad,) = torch.autograd.grad(val, [x])
                with torch.no_grad():            # the intermediate tensors of forward(), by the same calls
                    tr = sys.modules["perceptor.transforms"]
                    small = torch.tensor(shape[2:]) // 2
                    down = tr.resize(x.detach(), (small / torch.tensor(shape[2:])).tolist(), small, resample="bicubic")
                    upd = up.enhance(down, outscale=2)
                out[f"loss_{name}_in"], out[f"loss_{name}_value"], out[f"loss_{name}_grad"] = x.detach().float(), val.detach(), grad
                out[f"loss_{name}_down"], out[f"loss_{name}_up"] = down, upd
        return {k: np.ascontiguousarray(v.detach().numpy()) for k, v in out.items()}
    finally:
        torch.set_default_dtype(torch.float32)


def to_bytes(arrays) -> bytes:
    buf = io.BytesIO()
    np.savez(buf, **arrays)
    return buf.getvalue()


if __name__ == "__main__":
    data = to_bytes(generate())
    if "--check" in sys.argv:
        same = open(OUT, "rb").read() == data
        print(f"{OUT}: {'reproduced bit for bit' if same else 'DIFFERS'}")
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as f:
        f.write(data)
    print(f"wrote {OUT} ({len(data)} bytes)")
