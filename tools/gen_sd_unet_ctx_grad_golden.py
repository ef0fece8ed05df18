#!/usr/bin/env python3
"""Writes tests/golden/sd_ldm_unet_{tiny,v1}_ctx_grad.npz: the gradient with respect to the CONTEXT (the prompt encodings) of the reference's
vendored CompVis openaimodel.UNetModel, the twin of tools/gen_sd_unet_grad_golden.py: same module, name-keyed synthetic weights, inputs,
timesteps and cotangent (seed 93), by its own fp32 autograd with the latents and the context both requiring grad.

    python tools/gen_sd_unet_ctx_grad_golden.py        (needs the reference tree; runs on the CPU; not used by tests or bench.py)

Stored: `grad_ctx` = VJP(eps)(cotangent) with respect to ctx [n, tokens, context_dim], and `grad`, the latent gradient of the same joint
call (it is the one sd_ldm_unet_{tag}_grad.npz holds).  Inputs and cotangent are read from that file by the tests.
tiny: 2 samples, 7 context tokens; SD-v1 (860 M parameters): 1 sample, 77 tokens."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import _refimport as R  # noqa: E402
from oracle import gen_golden as G  # noqa: E402
from oracle import sd as osd  # noqa: E402
from perceptor_amd.utils.synth import seeded_noise, synth_state_dict  # noqa: E402


def main():
    om = R.ref("models.latent_diffusion.ldm.modules.diffusionmodules.openaimodel")
    for tag, cfg, n, hw, tc in (("tiny", osd.SD_TINY, 2, 16, 7), ("v1", osd.SD_V1, 1, 16, 77)):
        bo = cfg.block_out
        m = om.UNetModel(image_size=hw, in_channels=cfg.in_channels, out_channels=cfg.out_channels, model_channels=bo[0],
                         attention_resolutions=[2 ** i for i, c in enumerate(cfg.cross_attn) if c], num_res_blocks=cfg.layers_per_block,
                         channel_mult=[c // bo[0] for c in bo], num_heads=cfg.heads, use_spatial_transformer=True, transformer_depth=1,
                         context_dim=cfg.context_dim, use_checkpoint=False, legacy=False).eval()
        sd = synth_state_dict(osd.unet_state_dict_shapes(cfg), 0)
        m.load_state_dict(G._ldm_unet_keys(cfg, sd), strict=True)
        for p in m.parameters():
            p.requires_grad_(False)
        x, ctx = seeded_noise((n, cfg.in_channels, hw, hw), 71), seeded_noise((n, tc, cfg.context_dim), 72)
        t = torch.tensor([981, 20][:n])
        xx, cc = x.clone().requires_grad_(), ctx.clone().requires_grad_()
        y = m(xx, t, context=cc)
        cot = seeded_noise(tuple(y.shape), 93)
        y.backward(cot)
        out = os.path.join(G.OUT, f"sd_ldm_unet_{tag}_ctx_grad.npz")
        np.savez_compressed(out, grad_ctx=cc.grad.numpy(), grad=xx.grad.numpy())
        print("wrote", out, os.path.getsize(out), "bytes", "|grad_ctx|max", float(cc.grad.abs().max()))


if __name__ == "__main__":
    main()
