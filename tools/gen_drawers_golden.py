"""Writes tests/golden/drawers_reference.npz: what the reference's own drawers code computes, run unmodified on the CPU.

  perceptor/drawers/jpeg/{compression,decompression,utils}.py   compress_jpeg / decompress_jpeg in float64 (.double())
  perceptor/transforms/resize/resize_right.py                   resize(..., resample="bilinear"), the call of drawers.Raw.encode
  perceptor/drawers/raw/init/{fractal,gradient}.py              the seeded initial images

Per JPEG case (shape, factor): the fp32 inputs (image, coefficient noise applied: ``coef_*``, gradient weights ``w``), compress_jpeg with
diff_round (``enc_*``) and with identity rounding (``encid_*``), decompress_jpeg of the PERTURBED coefficients coef = float32(enc + 0.6 N(0, 1))
(``dec``) and the autograd gradients of sum(dec * w) with respect to the three tensors (``grad_*``).  Inputs come from tests/_jpeg_ref64.py's
seeded generators (its SEEDS table keeps the cases away from rounding ties and clamp edges) so the tests can rebuild them.  Only numbers are written.

Size: every case stores 24 fp32 and 66 float64 bytes per pixel, so the cases are the three smallest shapes of the GPU tests at both factors
and (3, 32, 48) at factor 1 -- all five shapes at both factors would pass the repository's limit for one file.  The shapes left out run
against tests/_jpeg_ref64.py on the GPU like the others; this file pins that restatement to the reference.

    python tools/gen_drawers_golden.py [--check]
"""
from __future__ import annotations

import importlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "drawers_reference.npz")

from oracle import _refimport as R                                  # noqa: E402
import _jpeg_ref64 as J                                             # noqa: E402

CASES = [(s, f) for s in J.SHAPES[:3] for f in J.FACTORS] + [(J.SHAPES[3], 1.0)]


def case_name(shape, factor):
    return "n%d_%dx%d_f%s" % (*shape, str(factor).replace(".", "p"))


def _ref_drawers():
    R.install()
    base = os.path.join(R.REF_ROOT, "perceptor", "drawers")
    R._shell("perceptor.drawers", base)
    R._shell("perceptor.drawers.jpeg", os.path.join(base, "jpeg"))
    R._shell("perceptor.drawers.raw", os.path.join(base, "raw"))
    R._shell("perceptor.drawers.raw.init", os.path.join(base, "raw", "init"))
    mod = lambda name: importlib.import_module("perceptor.drawers." + name)
    return mod("jpeg.compression"), mod("jpeg.decompression"), mod("raw.init.fractal"), mod("raw.init.gradient")


def generate():
    comp, decomp, fractal, gradient = _ref_drawers()
    resize = R.ref("transforms.resize.resize_right").resize
    out = {}
    for shape, factor in CASES:
        n, h, w = shape
        name = case_name(shape, factor)
        img = J.image(shape, factor)
        wts = J.weights(shape)
        enc = comp.compress_jpeg(factor=factor).double()(img.double())
        encid = comp.compress_jpeg(rounding=lambda x: x, factor=factor).double()(img.double())
        g = torch.Generator().manual_seed(J.SEEDS[shape, factor][1])
        coef = [(c + J.SIGMA * torch.randn(c.shape, generator=g, dtype=torch.float64)).float() for c in enc]
        leaves = [c.double().requires_grad_(True) for c in coef]
        dec = decomp.decompress_jpeg(h, w, factor=factor).double()(*leaves)
        grads = torch.autograd.grad((dec * wts.double()).sum(), leaves)
        out[name + "_image"], out[name + "_w"] = img, wts
        for k, c in enumerate(("y", "cb", "cr")):
            out[f"{name}_enc_{c}"], out[f"{name}_encid_{c}"] = enc[k], encid[k]
            out[f"{name}_coef_{c}"], out[f"{name}_grad_{c}"] = coef[k], grads[k]
        out[name + "_dec"] = dec
    gen = torch.Generator().manual_seed(7)
    for tag, (ih, iw), (oh, ow) in (("down", (24, 40), (16, 32)), ("up", (16, 16), (32, 48))):
        x = torch.rand((2, 3, ih, iw), generator=gen, dtype=torch.float32)
        out[f"resize_{tag}_in"] = x
        out[f"resize_{tag}_out"] = resize(x.double(), out_shape=(oh, ow), resample="bilinear").contiguous()
    np.random.seed(11)
    out["fractal_seed11_1x3x24x40"] = fractal.fractal((1, 3, 24, 40))
    np.random.seed(12)
    out["gradient_seed12_2x3x16x24"] = gradient.gradient((2, 3, 16, 24))
    return {k: np.ascontiguousarray(v.detach().numpy()) for k, v in out.items()}


def to_bytes(arrays) -> bytes:
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
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
