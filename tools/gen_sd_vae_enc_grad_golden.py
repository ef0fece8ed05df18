#!/usr/bin/env python3
"""Writes tests/golden/sd_ldm_vae_enc_{tiny,v1}_grad.npz: the image gradient of the reference's vendored CompVis Encoder (the module
oracle/gen_golden.py gen_sd_ldm pins the VAE encoder's forward with), run in float64 on the name-keyed synthetic weights.

    python tools/gen_sd_vae_enc_grad_golden.py        (needs the reference tree; runs on the CPU; not used by tests or bench.py)

Stored: `x` [1, 3, hw, hw] (the encoder's input in [-1, 1]: the 2 * img - 1 of the class surface is not part of it), the moments
`mean` | `logvar`, a seeded cotangent of both of CLIP-like magnitude (1e-6) and `grad` = VJP(moments)(cotangent) with respect to x.
quant_conv is a plain conv2d (as in gen_sd_ldm: AutoencoderKL itself needs pytorch_lightning).  Small images keep the fixtures small:
tiny at 32 x 32, SD-v1 at 64 x 64.
"""
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
    mm = R.ref("models.latent_diffusion.ldm.modules.diffusionmodules.model")
    for tag, cfg, hw in (("tiny", osd.VAE_TINY, 32), ("v1", osd.VAE_V1, 64)):
        dd = dict(ch=cfg.block_out[0], out_ch=cfg.out_channels, ch_mult=tuple(c // cfg.block_out[0] for c in cfg.block_out),
                  num_res_blocks=cfg.layers_per_block, attn_resolutions=[], in_channels=cfg.out_channels, resolution=256,
                  z_channels=cfg.latent_channels)
        sd = synth_state_dict(osd.vae_encoder_state_dict_shapes(cfg), 0)
        enc = mm.Encoder(**dd, double_z=True).eval()
        enc.load_state_dict(G._ldm_vae_keys(cfg, sd, "encoder"), strict=True)
        enc = enc.double()
        x = seeded_noise((1, cfg.out_channels, hw, hw), 74) * 0.5
        x64 = x.double().requires_grad_()
        mom = torch.nn.functional.conv2d(enc(x64), sd["quant_conv.weight"].double(), sd["quant_conv.bias"].double())
        cot = seeded_noise(tuple(mom.shape), 93) * 1e-6
        mom.backward(cot.double())
        lc = cfg.latent_channels
        out = os.path.join(G.OUT, f"sd_ldm_vae_enc_{tag}_grad.npz")
        np.savez_compressed(out, x=x.numpy(), mean=mom[:, :lc].detach().float().numpy(), logvar=mom[:, lc:].detach().float().numpy(),
                            cotangent=cot.numpy(), grad=x64.grad.float().numpy(), hw=np.array(hw))
        print("wrote", out, os.path.getsize(out), "bytes", "|grad|max", float(x64.grad.abs().max()))


if __name__ == "__main__":
    main()
