"""Writes tests/golden/losses_reference.npz: inputs, losses and autograd gradients of the reference's own guidance losses
(perceptor/losses: Smoothness, Resize, SimulacraAesthetic, AestheticVisualAssessment in its three modes, SphericalDistance), run
unmodified on the CPU in float64.

Smoothness.forward and Resize.forward run as they are.  The two aesthetic losses and SphericalDistance are instantiated without
__init__ (their constructors download a tower and a head): the tower is a stub whose ``encode_images`` returns F.normalize of the
tensor it is given -- the "images" are un-normalised embeddings, so the stored gradients are dloss/d(embedding) -- and the heads
are nn.Linear modules filled from the values stored in the fixture.  Only numbers are written; needs the reference tree
(oracle/_refimport.py).  Deterministic: a second run reproduces the file bit for bit.

    python tools/gen_losses_golden.py [--check]
"""
from __future__ import annotations

import importlib
import io
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "losses_reference.npz")

from oracle import _refimport as R                      # noqa: E402
from perceptor_amd.utils.synth import seeded_noise      # noqa: E402


def _ref_losses():
    R.install()
    base = os.path.join(R.REF_ROOT, "perceptor")
    R._shell("perceptor.losses", os.path.join(base, "losses"))
    sys.modules["perceptor.transforms.resize"].resize = R.ref("transforms.resize.resize_right").resize
    mod = lambda name: importlib.import_module("perceptor." + name)
    return dict(smoothness=mod("losses.smoothness").Smoothness, resize=mod("losses.resize").Resize,
                simulacra=mod("losses.simulacra_aesthetic").SimulacraAesthetic,
                simulacra_model=mod("models.simulacra_aesthetic.simulacra_aesthetic").SimulacraAesthetic,
                ava=mod("losses.aesthetic_visual_assessment").AestheticVisualAssessment,
                spherical=mod("losses.spherical_distance").SphericalDistance)


class _StubTower(torch.nn.Module):
    def encode_images(self, images):
        return F.normalize(images)


def _bare(cls):
    obj = cls.__new__(cls)
    torch.nn.Module.__init__(obj)
    return obj


def _linear(w, b):
    lin = torch.nn.Linear(w.shape[1], w.shape[0]).double()
    with torch.no_grad():
        lin.weight.copy_(w)
        lin.bias.copy_(b)
    return lin.requires_grad_(False)


def _grad(fn, *xs):
    xs = [x.clone().requires_grad_(True) for x in xs]
    loss = fn(*xs)
    return (loss.detach(), *torch.autograd.grad(loss, xs))


def generate():
    C = _ref_losses()
    # every input is an fp32 value stored as float64: the fp32 product sees exactly what the reference saw
    d64 = lambda shape, seed, scale=1.0, shift=0.0: (seeded_noise(shape, seed) * scale + shift).double()
    out = {}
    # ---- Smoothness, Resize: as they are
    x = d64((2, 3, 5, 7), 101, 0.25, 0.5)
    out["smooth_x"] = x
    out["smooth_loss"], out["smooth_grad"] = _grad(C["smoothness"]().forward, x)
    a, b = d64((2, 3, 20, 24), 102, 0.25, 0.5), d64((2, 3, 18, 16), 103, 0.25, 0.5)
    size = (12, 12)
    out["resize_a"], out["resize_b"], out["resize_size"] = a, b, torch.tensor(size)
    out["resize_loss"], out["resize_grad_a"], out["resize_grad_b"] = _grad(lambda p, q: C["resize"]()(p, q, size), a, b)
    # Resize at the inputs' own size: the resize is the identity and what remains is the mean squared difference (pmi_sqdiff_loss)
    sa, sb = d64((2, 3, 6, 5), 111), d64((2, 3, 6, 5), 112, 0.5, 0.1)
    out["sq_a"], out["sq_b"] = sa, sb
    out["sq_loss"], out["sq_grad_a"], out["sq_grad_b"] = _grad(lambda p, q: C["resize"]((6, 5))(p, q), sa, sb)
    # ---- aesthetic heads on given embeddings
    dim = 64
    emb = d64((3, dim), 104, 3.0)
    out["head_emb"] = emb
    w1, b1 = d64((1, dim), 105, dim ** -0.5), d64((1,), 106, 0.05, 5.0)
    sim_model = _bare(C["simulacra_model"])
    sim_model.linear, sim_model.clip_model = _linear(w1, b1), _StubTower()
    sim = _bare(C["simulacra"])
    sim.aesthetic_target = torch.nn.Parameter(torch.as_tensor(7).double(), requires_grad=False)
    sim.model, sim.multiplier = sim_model, 0.001
    out["sim_w"], out["sim_b"], out["sim_target"], out["sim_multiplier"] = w1, b1, torch.tensor(7.0, dtype=torch.float64), torch.tensor(0.001, dtype=torch.float64)
    out["sim_ratings"] = sim_model(emb).detach()
    out["sim_loss"], out["sim_demb"] = _grad(sim.forward, emb)
    w10, b10 = d64((10, dim), 107), d64((10,), 108, 0.05)
    out["ava_w"], out["ava_b"], out["ava_target"] = w10, b10, torch.tensor(4)
    for mode in ("logit", "expected", "probability"):
        ava = _bare(C["ava"])
        ava.aesthetic_target, ava.mode, ava.model, ava.aesthetic_head = 4, mode, _StubTower(), _linear(w10, b10)
        out[f"ava_{mode}_loss"], out[f"ava_{mode}_demb"] = _grad(ava.forward, emb)
    out["ava_logits"] = _linear(w10, b10)(F.normalize(emb))
    # ---- SphericalDistance on given embeddings
    ea, eb = d64((3, dim), 109, 2.0), d64((2, dim), 110, 0.5)
    out["sph_a"], out["sph_b"] = ea, eb
    sph = C["spherical"](_StubTower())
    out["sph_loss"], out["sph_grad_a"], out["sph_grad_b"] = _grad(sph.forward, ea, eb)
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
