"""HIP engines for OpenAI's GLIDE CLIP (the noise-aware CLIP of perceptor/models/glide_clip/): the image tower on the diffused 64x64
image and its timestep, with the gradient w.r.t. that image, and the text tower (forward only).

The image tower is engine/vit.py's tower between its two ends (encoders.py:459-544): 257 tokens, pre-LN blocks with the exact GELU,
fp32 residual stream, LayerNorm on token 0 and a bias-free projection.  The reference's padded block-sparse attention mask is plain
attention over the real tokens (the bias is 0 inside [:T, :T], -1e10 on the pad keys, and the pad query rows are sliced off).  What
differs is the stem (encoders.py:110-143): Normalize on the 0..255 scale, a 4x4 stride-4 patch convolution (K = 48), token 0 taken PER
SAMPLE from row t[n] of a [n_timestep, width] table, positions, LayerNorm, and no resize.  VitEngine's two stem seams are overridden with
the fused kernels of csrc/glide.hip: one launch per direction, fp32 throughout (no 16-bit patches, no 16-bit g0, no im2col tensors).
The key projection has no bias (encoders.py:168-175): the key map below writes zeros there.

State-dict keys are the GLIDE checkpoints' own (``blocks.input.*``, ``blocks.block_{i}.f_attn.*`` / ``f_mlp.*``, ``blocks.output.*``);
``image_state_dict_to_vit`` / ``text_state_dict_to_clip`` map them to the OpenAI-CLIP names VitEngine and TextEngine pack.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from .. import _hip
from .._hip import call, ptr
from ..utils.synth import synth_tensor
from .text import TextEngine
from .vit import VitEngine

# encoders.py:21-22 -- the OpenAI-CLIP constants on the 0..255 scale
GLIDE_MEAN = (122.77093945, 116.74601272, 104.09373519)
GLIDE_STD = (68.50053285, 66.63215831, 70.32316309)

# config.yml: (image, patch, width, layers, heads, out_dim, n_timestep) and (context, vocab, width, layers, heads, out_dim)
GLIDE_IMAGE_CONFIG = (64, 4, 768, 12, 12, 512, 1000)
GLIDE_TEXT_CONFIG = (77, 65536, 512, 12, 8, 512)
GLIDE_LOGIT_SCALE = 100.0


def _block_shapes(width: int, layers: int) -> Dict[str, Tuple[int, ...]]:
    S = {}
    for i in range(layers):
        a, m = f"blocks.block_{i}.f_attn.", f"blocks.block_{i}.f_mlp."
        S[a + "ln.g"] = (width,); S[a + "ln.b"] = (width,)
        S[a + "f_q.w"] = (width, width); S[a + "f_q.b"] = (width,)
        S[a + "f_k.w"] = (width, width)
        S[a + "f_v.w"] = (width, width); S[a + "f_v.b"] = (width,)
        S[a + "f_c.w"] = (width, width); S[a + "f_c.b"] = (width,)
        S[m + "ln.g"] = (width,); S[m + "ln.b"] = (width,)
        S[m + "f_1.w"] = (4 * width, width); S[m + "f_1.b"] = (4 * width,)
        S[m + "f_2.w"] = (width, 4 * width); S[m + "f_2.b"] = (width,)
    return S


def glide_image_state_dict_shapes(cfg) -> Dict[str, Tuple[int, ...]]:
    res, patch, width, layers, heads, out, n_timestep = cfg
    S = {"blocks.input.w_t": (n_timestep, width), "blocks.input.patch_proj": (width, 3, patch, patch),
         "blocks.input.w_pos": ((res // patch) ** 2 + 1, width), "blocks.input.ln.g": (width,), "blocks.input.ln.b": (width,)}
    S.update(_block_shapes(width, layers))
    S.update({"blocks.output.ln.g": (width,), "blocks.output.ln.b": (width,), "blocks.output.f.w": (out, width)})
    return S


def glide_text_state_dict_shapes(cfg) -> Dict[str, Tuple[int, ...]]:
    ctx, vocab, width, layers, heads, out = cfg
    S = {"blocks.input.w_voc": (vocab, width), "blocks.input.w_pos": (ctx, width)}
    S.update(_block_shapes(width, layers))
    S.update({"blocks.output.ln.g": (width,), "blocks.output.ln.b": (width,), "blocks.output.f.w": (out, width)})
    return S


def glide_synth_state_dict(shapes, seed: int = 0, rounding: str = "bf16") -> Dict[str, torch.Tensor]:
    """utils/synth.py under the checkpoints' names: it keys its scales on the leaf name, and the LayerNorm gains, ``weight`` there, are
    called ``g`` here."""
    return {k: synth_tensor(k[:-2] + ".weight" if k.endswith(".g") else k, shp, seed, rounding=rounding) for k, shp in shapes.items()}


def _map_blocks(sd, out) -> None:
    g = lambda k: sd[k].detach().float()
    i = 0
    while f"blocks.block_{i}.f_attn.ln.g" in sd:
        a, m, b = f"blocks.block_{i}.f_attn.", f"blocks.block_{i}.f_mlp.", f"transformer.resblocks.{i}."
        out[b + "attn.in_proj_weight"] = torch.cat([g(a + "f_q.w"), g(a + "f_k.w"), g(a + "f_v.w")], dim=0)
        out[b + "attn.in_proj_bias"] = torch.cat([g(a + "f_q.b"), torch.zeros_like(g(a + "f_q.b")), g(a + "f_v.b")], dim=0)   # no key bias
        out[b + "attn.out_proj.weight"], out[b + "attn.out_proj.bias"] = g(a + "f_c.w"), g(a + "f_c.b")
        out[b + "ln_1.weight"], out[b + "ln_1.bias"] = g(a + "ln.g"), g(a + "ln.b")
        out[b + "ln_2.weight"], out[b + "ln_2.bias"] = g(m + "ln.g"), g(m + "ln.b")
        out[b + "mlp.c_fc.weight"], out[b + "mlp.c_fc.bias"] = g(m + "f_1.w"), g(m + "f_1.b")
        out[b + "mlp.c_proj.weight"], out[b + "mlp.c_proj.bias"] = g(m + "f_2.w"), g(m + "f_2.b")
        i += 1


def image_state_dict_to_vit(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The GLIDE image encoder's state dict -> the OpenAI-CLIP ``visual.*`` names VitEngine packs, plus ``w_t`` (the timestep table, which
    has no counterpart there; ``class_embedding`` is absent for the same reason)."""
    g = lambda k: sd[k].detach().float()
    out = {"w_t": g("blocks.input.w_t"), "conv1.weight": g("blocks.input.patch_proj"), "positional_embedding": g("blocks.input.w_pos"),
           "ln_pre.weight": g("blocks.input.ln.g"), "ln_pre.bias": g("blocks.input.ln.b"),
           "ln_post.weight": g("blocks.output.ln.g"), "ln_post.bias": g("blocks.output.ln.b"), "proj": g("blocks.output.f.w").t().contiguous()}
    _map_blocks(sd, out)
    return out


def text_state_dict_to_clip(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The GLIDE text encoder's state dict -> the OpenAI-CLIP names TextEngine packs."""
    g = lambda k: sd[k].detach().float()
    out = {"token_embedding.weight": g("blocks.input.w_voc"), "positional_embedding": g("blocks.input.w_pos"),
           "ln_final.weight": g("blocks.output.ln.g"), "ln_final.bias": g("blocks.output.ln.b"),
           "text_projection": g("blocks.output.f.w").t().contiguous()}
    _map_blocks(sd, out)
    return out


class GlideImageEngine(VitEngine):
    def __init__(self, cfg, state_dict, device, dtype="bf16"):
        res, patch, width, layers, heads, out, n_timestep = cfg
        if patch != 4 or res % patch or width % 64 or width > 2048:
            raise ValueError("the GLIDE stem kernels take 4x4 patches and a width that is a multiple of 64 up to 2048")
        sd = image_state_dict_to_vit(state_dict)
        sd["class_embedding"] = torch.zeros(width)          # VitEngine packs one; this tower's token 0 comes from w_t instead
        super().__init__((res, patch, width, layers, heads, out), sd, device, dtype, quick_gelu=False)
        self.n_timestep = n_timestep
        self.cls = None
        dev = self.device
        self.w_t = sd["w_t"].to(dev).contiguous()
        self.w_patch = sd["conv1.weight"].reshape(width, 3 * patch * patch).to(dev).contiguous()    # fp32 [W][48], k = c P^2 + py P + px
        self.mean = torch.tensor(GLIDE_MEAN, device=dev)
        self.std = torch.tensor(GLIDE_STD, device=dev)
        self._ts = None

    def _embed(self, images):
        res, patch, width, layers, heads, out = self.cfg
        dev = self.device
        n = images.shape[0]
        t = (res // patch) ** 2 + 1
        images = images.float().contiguous()
        x0 = torch.empty((n, t, width), dtype=torch.float32, device=dev)
        x = torch.empty((n * t, width), dtype=torch.float32, device=dev)
        mr = torch.empty((2, n * t), dtype=torch.float32, device=dev)
        call("pmi_glide_embed_fwd", ptr(images), ptr(self.mean), ptr(self.std), ptr(self.w_patch), ptr(self._ts), ptr(self.w_t), ptr(self.pos),
             ptr(self.ln_pre[0]), ptr(self.ln_pre[1]), ptr(x0), ptr(x), ptr(mr), n, res, patch, width, self.n_timestep, 1e-5)
        return x0, x, mr

    def _embed_backward(self, g32, sv, record=None):
        res, patch, width, layers, heads, out = self.cfg
        n = sv["n"]
        dimg = torch.empty((n, 3, res, res), dtype=torch.float32, device=self.device)
        call("pmi_glide_embed_bwd", ptr(g32), ptr(sv["x0"]), ptr(self.ln_pre[0]), ptr(sv["mr_pre"]), ptr(self.w_patch), ptr(self.std), ptr(dimg),
             n, res, patch, width, 1.0 / self.gscale)
        return dimg

    @torch.no_grad()
    def forward(self, images: torch.Tensor, ts: torch.Tensor, save: bool = False):
        """images NCHW fp32 in [0,1] at exactly (image, image), ts int64 [N] -> un-normalised embeddings [N, out_dim] fp32.
        A ts outside [0, n_timestep) is clamped by the kernel (a device ts is never synchronised on)."""
        res = self.cfg[0]
        if images.ndim != 4 or images.shape[1] != 3:
            raise ValueError("input should be [N, 3, H, W]")
        if tuple(images.shape[2:]) != (res, res):
            raise ValueError(f"input is not {res} x {res}")
        if ts.ndim != 1 or ts.shape[0] != images.shape[0] or ts.dtype != torch.int64:
            raise ValueError("ts must be an int64 tensor of shape [N]")
        if not images.is_cuda:
            raise RuntimeError("GlideImageEngine runs on a HIP device only (no CPU fallback)")
        self._ts = ts.to(self.device).contiguous()
        try:
            return super().forward(images, save=save)
        finally:
            self._ts = None


class GlideTextEngine(TextEngine):
    """engine/text.TextEngine under the GLIDE checkpoint's key names: exact GELU, no key bias, pooled at row lengths - 1."""

    def __init__(self, cfg, state_dict, device, dtype="bf16"):
        super().__init__(cfg, text_state_dict_to_clip(state_dict), device, dtype, quick_gelu=False)
