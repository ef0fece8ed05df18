#!/usr/bin/env python3
"""Writes tests/golden/sd_ldm_vae_{tiny,v1}_grad.npz: the latent gradient of the reference's vendored CompVis Decoder (the module
oracle/gen_golden.py gen_sd_ldm pins the VAE decoder's forward with), run in float64 on the name-keyed synthetic weights.

    python tools/gen_sd_vae_grad_golden.py        (needs the reference tree; runs on the CPU; not used by tests or bench.py)

Stored: z [1, 4, hw, hw], the decoder's output `dec`, a seeded cotangent of CLIP-like magnitude (1e-6) and `grad` = VJP(dec)(cotangent)
with respect to z.  post_quant_conv is a plain conv2d (as in gen_sd_ldm: AutoencoderKL itself needs pytorch_lightning); the 1 / 0.18215
latent scale and (x + 1) / 2 are not part of it.  Small latents keep the fixtures small: tiny at 16 x 16, SD-v1 at 8 x 8 (64 x 64 images).
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
    for tag, cfg, hw in (("tiny", osd.VAE_TINY, 16), ("v1", osd.VAE_V1, 8)):
        dd = dict(ch=cfg.block_out[0], out_ch=cfg.out_channels, ch_mult=tuple(c // cfg.block_out[0] for c in cfg.block_out),
                  num_res_blocks=cfg.layers_per_block, attn_resolutions=[], in_channels=cfg.out_channels, resolution=256,
                  z_channels=cfg.latent_channels)
        sd = synth_state_dict(osd.vae_decoder_state_dict_shapes(cfg), 0)
        dec = mm.Decoder(**dd).eval()
        dec.load_state_dict(G._ldm_vae_keys(cfg, sd, "decoder"), strict=True)
        dec = dec.double()
        z = seeded_noise((1, cfg.latent_channels, hw, hw), 73)
        z64 = z.double().requires_grad_()
        y = dec(torch.nn.functional.conv2d(z64, sd["post_quant_conv.weight"].double(), sd["post_quant_conv.bias"].double()))
        cot = seeded_noise(tuple(y.shape), 92) * 1e-6
        y.backward(cot.double())
        out = os.path.join(G.OUT, f"sd_ldm_vae_{tag}_grad.npz")
        np.savez_compressed(out, z=z.numpy(), dec=y.detach().float().numpy(), cotangent=cot.numpy(), grad=z64.grad.float().numpy(),
                            hw=np.array(hw))
        print("wrote", out, os.path.getsize(out), "bytes", "|grad|max", float(z64.grad.abs().max()))


if __name__ == "__main__":
    main()
