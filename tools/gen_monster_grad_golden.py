"""Writes tests/golden/monster_diffusion_grad_reference.npz: the input gradient of the reference's own MonsterDiffusion.denoised_
(perceptor/models/monster_diffusion/monster_diffusion.py:103-125 over base/model.py), run unmodified on the CPU in float64 with
diffused_images.requires_grad_(), through the stand-ins of tools/gen_monster_diffusion_golden.py.

Networks A and B of that tool with the existing fixture's weights, inputs and sigma (read back from
tests/golden/monster_diffusion_reference.npz, which this tool does not touch) and a seeded unit-normal cotangent on denoised_xs.  Stored per
network: the cotangent, d_images, the gradient with respect to the network input c_in * x (`gx`) and the gradient arriving at every d- and
u-block's input (`g_d<i>`, `g_u<i>`; a u-block below the deepest reads cat([input, skip]): its gradient is stored in that channel order).
A block's input tensor is also read elsewhere (a d-block's output is the next block's input and a stored skip), so a forward pre-hook hands
each block `t.view_as(t)` of its arguments and keeps that view's gradient: the gradient through this block alone.  No arithmetic of the
reference is replaced.  Tensors above 2048 values are stored as every s-th value plus the full tensor's norm, as the forward fixture does;
the per-sample norms are stored next to them.  Only numbers are written.  Deterministic.

    python tools/gen_monster_grad_golden.py [--check]
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "tests", "golden", "monster_diffusion_grad_reference.npz")
FWD = os.path.join(ROOT, "tests", "golden", "monster_diffusion_reference.npz")

import gen_monster_diffusion_golden as G                                      # noqa: E402

COTANGENT_SEED = 777


def _keep(out, name, t):
    t = t.detach().double().contiguous()
    out[name + "_sample_norms"] = t.flatten(1).norm(dim=1)
    G._keep(out, name, t)


def generate():
    torch.set_default_dtype(torch.float64)
    try:
        model_mod, md_mod = G._modules()
        fwd = np.load(FWD)
        out = {}
        for name, (config, shape, sigma) in G.NETS.items():
            m = G._wrapper(model_mod, md_mod, config)
            net = m.network
            x = torch.from_numpy(fwd[f"{name}_in"]).double().requires_grad_()
            assert tuple(x.shape) == tuple(shape)
            ts = torch.tensor(sigma)
            kept = {}

            def tapped(key):
                def hook(mod, args, kwargs):
                    views = []

                    def view(t):
                        if not torch.is_tensor(t) or t.ndim != 4:
                            return t
                        v = t.view_as(t)
                        v.retain_grad()
                        views.append(v)
                        return v

                    args = tuple(view(a) for a in args)
                    kwargs = {k: view(v) for k, v in kwargs.items()}
                    kept[key] = views
                    return args, kwargs
                return hook

            hooks = [net.proj_in.register_forward_pre_hook(tapped("gx"), with_kwargs=True)]
            for i, blk in enumerate(net.u_net.d_blocks):
                hooks.append(blk.register_forward_pre_hook(tapped(f"g_d{i}"), with_kwargs=True))
            for i, blk in enumerate(net.u_net.u_blocks):
                hooks.append(blk.register_forward_pre_hook(tapped(f"g_u{i}"), with_kwargs=True))
            with torch.enable_grad():
                den = m.denoised_(x, ts)
                g = np.random.Generator(np.random.Philox(key=COTANGENT_SEED + ord(name)))
                cot = torch.from_numpy(g.standard_normal(tuple(den.shape), dtype=np.float32)).double()
                (den * cot).sum().backward()
            for h in hooks:
                h.remove()
            assert float((den.detach() - torch.from_numpy(fwd[f"{name}_denoised_xs"])).abs().max()) == 0.0, "the forward fixture's run is not reproduced"
            out[f"{name}_cotangent"] = cot.float()
            out[f"{name}_d_images"] = x.grad.detach().clone()
            out[f"{name}_d_images_sample_norms"] = x.grad.flatten(1).norm(dim=1)
            for key, views in kept.items():
                _keep(out, f"{name}_{key}", torch.cat([v.grad for v in views], dim=1))
        return {k: np.ascontiguousarray(v.detach().numpy()) for k, v in out.items()}
    finally:
        torch.set_default_dtype(torch.float32)


if __name__ == "__main__":
    data = G.to_bytes(generate())
    if "--check" in sys.argv:
        same = open(OUT, "rb").read() == data
        print(f"{OUT}: {'reproduced bit for bit' if same else 'DIFFERS'}")
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as f:
        f.write(data)
    print(f"wrote {OUT} ({len(data)} bytes)")
