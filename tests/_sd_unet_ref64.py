"""TEST INFRASTRUCTURE -- the SD UNet forward restated dtype-generically from oracle.sd's own block functions, so torch autograd gives the
latent gradient in float64.  oracle.sd.unet_forward builds its sinusoidal time embedding in fp32 whatever the weights' dtype; everything
else in it follows the dtype of its inputs.  Here the embedding follows the weights' dtype and the rest is the oracle's code, called
block by block in the oracle's order.  Pinned by tests/test_sd_unet_grad_cpu.py: in fp32 this reproduces oracle.sd.unet_forward exactly."""
import math

import torch
import torch.nn.functional as F

from oracle import sd as osd


def timestep_embedding(t, dim, dtype):
    half = dim // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=dtype) / half)
    a = t.to(dtype)[:, None] * freqs[None]
    return torch.cat([a.cos(), a.sin()], dim=-1)


def unet_forward(sd, cfg, sample, timesteps, context, drop_skip_grad=False):
    """oracle.sd.unet_forward in the dtype of `sd` / `sample`.  drop_skip_grad: the skip tensors reach the up path detached (a defect of the
    backward the CPU tests measure: the skip-concatenation gradient dropped)."""
    bo, g = cfg.block_out, cfg.groups
    dtype = sample.dtype
    emb = timestep_embedding(timesteps, bo[0], dtype)
    emb = F.linear(F.silu(F.linear(emb, sd["time_embedding.linear_1.weight"], sd["time_embedding.linear_1.bias"])),
                   sd["time_embedding.linear_2.weight"], sd["time_embedding.linear_2.bias"])
    es = F.silu(emb)
    h = osd._conv(sample, sd, "conv_in")
    skips = [h]
    for i in range(len(bo)):
        for j in range(cfg.layers_per_block):
            h = osd._resnet(sd, f"down_blocks.{i}.resnets.{j}", h, es, g, 1e-5)
            if cfg.cross_attn[i]:
                h = osd._transformer(sd, f"down_blocks.{i}.attentions.{j}", h, context, cfg.heads, g)
            skips.append(h)
        if i != len(bo) - 1:
            h = osd._conv(h, sd, f"down_blocks.{i}.downsamplers.0.conv", stride=2)
            skips.append(h)
    h = osd._resnet(sd, "mid_block.resnets.0", h, es, g, 1e-5)
    h = osd._transformer(sd, "mid_block.attentions.0", h, context, cfg.heads, g)
    h = osd._resnet(sd, "mid_block.resnets.1", h, es, g, 1e-5)
    ca = list(reversed(cfg.cross_attn))
    for i in range(len(bo)):
        for j in range(cfg.layers_per_block + 1):
            s = skips.pop()
            h = osd._resnet(sd, f"up_blocks.{i}.resnets.{j}", torch.cat([h, s.detach() if drop_skip_grad else s], dim=1), es, g, 1e-5)
            if ca[i]:
                h = osd._transformer(sd, f"up_blocks.{i}.attentions.{j}", h, context, cfg.heads, g)
        if i != len(bo) - 1:
            h = osd._conv(F.interpolate(h, scale_factor=2.0, mode="nearest"), sd, f"up_blocks.{i}.upsamplers.0.conv")
    return osd._conv(F.silu(osd._gn(h, sd, "conv_norm_out", g, 1e-5)), sd, "conv_out")


def latent_grad(sd32, cfg, x, timesteps, context, cot, dtype=torch.float64, **kw):
    """(eps, d <eps, cot> / d x) in `dtype` on the fp32 master weights."""
    w = {k: v.to(dtype) for k, v in sd32.items()}
    xx = x.to(dtype).clone().requires_grad_()
    eps = unet_forward(w, cfg, xx, timesteps, context.to(dtype), **kw)
    eps.backward(cot.to(dtype))
    return eps.detach(), xx.grad.detach()


def attention_tiled_backward(q, k, v, d_out, scale, tile=32):
    """float64 restatement of pmi_attn_flash_bwd for one head: q [T, d], k / v [Tk, d], d_out [T, d] -> (dq, dk, dv).  Keys are zero-padded
    to whole tiles; P is recomputed per tile from the log-sum-exp (exp2 domain) and delta = rowsum(dO o O); a padded key gets weight 0."""
    t, tk = q.shape[0], k.shape[0]
    sl2 = scale * 1.4426950408889634
    s2 = (q @ k.T) * sl2
    lse = torch.log2(torch.exp2(s2 - s2.max(1, keepdim=True).values).sum(1)) + s2.max(1).values
    out = torch.exp2(s2 - lse[:, None]) @ v
    delta = (d_out * out).sum(1)
    tkp = (tk + tile - 1) // tile * tile
    kp, vp = torch.zeros((tkp, q.shape[1]), dtype=q.dtype), torch.zeros((tkp, q.shape[1]), dtype=q.dtype)
    kp[:tk], vp[:tk] = k, v
    dq, dk, dv = torch.zeros_like(q), torch.zeros_like(kp), torch.zeros_like(vp)
    for s0 in range(0, tkp, tile):
        ks, vs = kp[s0:s0 + tile], vp[s0:s0 + tile]
        p = torch.exp2((q @ ks.T) * sl2 - lse[:, None])
        p[:, max(0, tk - s0):] = 0.0
        ds = p * (d_out @ vs.T - delta[:, None]) * scale
        dq += ds @ ks
        dk[s0:s0 + tile] = ds.T @ q
        dv[s0:s0 + tile] = p.T @ d_out
    return out, dq, dk[:tk], dv[:tk]
