"""Writes tests/golden/style_transfer_reference.npz: inputs, encodings, Gram matrices, loss and autograd image gradients of the
reference's own losses.StyleTransfer (perceptor/losses/style_transfer.py), run unmodified on the CPU in float64.

The reference builds its tower with ``torchvision.models.vgg19(pretrained=True).features``.  torchvision is absent here and the
checkpoint unreachable, so a stand-in ``torchvision.models.vgg19`` is registered whose ``.features`` is an nn.Sequential of plain
torch.nn layers at torchvision's 37 indices (Conv2d 3x3 pad 1 / ReLU / MaxPool2d(2, 2)), with selectable widths and this package's
synthetic weights (utils.synth, gain sqrt(2)).  Everything else -- ``encode`` (with the reference's own resize), ``gram_matrix``,
``loss``, ``forward`` and autograd -- is the reference's code.  The reference resizes to 256 x 256; to keep the fixture small the
cases run the tiny tower at its own size 32, so ``encode``'s size constant is the one thing parametrised: the module's ``resize`` is
wrapped to target (size, size) and to pass inputs of that size through (see ``generate``).  Only numbers are written; needs the
reference tree (oracle/_refimport.py).  Deterministic.

    python tools/gen_style_transfer_golden.py [--check]
"""
from __future__ import annotations

import importlib
import io
import os
import sys
import types

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "style_transfer_reference.npz")

from oracle import _refimport as R                                  # noqa: E402
from perceptor_amd.utils.synth import synth_state_dict              # noqa: E402

WIDTHS, SIZE, SEED = (16, 16, 32, 32, 32), 32, 0
DEPTHS = (2, 2, 4, 4, 4)


def _features(widths):
    mods, cin = [], 3
    for depth, w in zip(DEPTHS, widths):
        for _ in range(depth):
            mods += [nn.Conv2d(cin, w, 3, padding=1), nn.ReLU(inplace=False)]
            cin = w
        mods.append(nn.MaxPool2d(2, 2))
    seq = nn.Sequential(*mods)
    assert len(seq) == 37
    shapes = {k: tuple(v.shape) for k, v in seq.state_dict().items()}
    seq.load_state_dict(synth_state_dict(shapes, SEED, gain=2 ** 0.5))
    return seq.double()


def _ref_style_transfer():
    R.install()
    base = os.path.join(R.REF_ROOT, "perceptor")
    R._shell("perceptor.losses", os.path.join(base, "losses"))
    tvm = R._shell("torchvision.models")
    tvm.vgg19 = lambda pretrained=True: types.SimpleNamespace(features=_features(WIDTHS))
    sys.modules["torchvision"].models = tvm
    sys.modules["perceptor.transforms.resize"].resize = R.ref("transforms.resize.resize_right").resize
    return importlib.import_module("perceptor.losses.style_transfer")


def generate():
    mod = _ref_style_transfer()
    ref_resize = mod.resize

    # encode() compares ``images.shape[-2:]`` with the constant (256, 256) and passes ``out_shape=(256, 256)`` to resize.  The tiny
    # tower runs at SIZE: the module-level ``resize`` is wrapped to target (SIZE, SIZE) and to return inputs already at that size
    # untouched -- the same decision the reference takes at 256.
    def resize(images, out_shape):
        if tuple(images.shape[-2:]) == (SIZE, SIZE):
            return images
        # .contiguous(): resize_right returns a permuted view for some axis orders and the reference's gram_matrix takes .view() of
        # every list entry, the image included; no arithmetic changes
        return ref_resize(images, out_shape=(SIZE, SIZE)).contiguous()

    mod.resize = resize
    loss = mod.StyleTransfer()
    g = np.random.Generator(np.random.Philox(key=4242))
    img = lambda n, h, w: torch.from_numpy(g.random((n, 3, h, w), dtype=np.float32)).double()
    out = {"widths": torch.tensor(WIDTHS), "size": torch.tensor(SIZE), "seed": torch.tensor(SEED)}
    for name, (h, w) in (("same", (SIZE, SIZE)), ("resized", (48, 40))):
        a, b = img(2, h, w).requires_grad_(True), img(2, h, w).requires_grad_(True)
        ea, eb = loss.encode(a), loss.encode(b)
        val = loss.loss(ea, eb)
        ga, gb = torch.autograd.grad(val, [a, b])
        fwd = loss.forward(a.detach(), b.detach())
        assert float(fwd.detach()) == float(val.detach())
        out[f"{name}_a"], out[f"{name}_b"] = a.float(), b.float()          # fp32 values: stored exactly
        out[f"{name}_loss"], out[f"{name}_grad_a"], out[f"{name}_grad_b"] = val, ga, gb
        for i, e in enumerate(ea):
            e = e.detach()
            out[f"{name}_enc{i}_shape"] = torch.tensor(e.shape)
            out[f"{name}_enc{i}_moments"] = torch.stack([e.mean(), e.abs().mean(), e.square().mean().sqrt(), e.max()])
            out[f"{name}_enc{i}_slice"] = e.flatten()[::37][:256]
        for i in (2, 3, 4):
            out[f"{name}_gram{i}"] = mod.gram_matrix(ea[i].detach())
    return {k: np.ascontiguousarray(v.detach().numpy()) for k, v in out.items()}


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
