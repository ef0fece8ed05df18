"""HIP engine for OWL-ViT open-vocabulary detection (perceptor/models/owlvit/modeling_owlvit.py, OwlViTForObjectDetection): class logits
of every patch token against a set of text queries, the predicted boxes, and the gradient of a loss on the logits w.r.t. the input image.

The image tower is engine/vit.py's CLIP ViT (pre_layernorm, QuickGELU blocks); what differs is its end.  Every CLIP loss here reads the
pooled class token; OWL-ViT reads ALL tokens of the last hidden state (modeling_owlvit.py:1396-1432):

  image_feats = layer_norm(post_layernorm(h)[1:] * post_layernorm(h)[0])            pmi_owl_merge_ln_fwd / _bwd   (csrc/owlvit.hip)
  class head    e = dense0(f); logits = (e / (|e| + 1e-6) . q + shift(f)) * (elu(scale(f)) + 1)
                dense0, logit_shift and logit_scale are linear in f: ONE ops.igemm with out_dim + 2 columns, then pmi_owl_class_logits_fwd
  box head      sigmoid(dense2(gelu(dense1(gelu(dense0(f))))) + box_bias): two ops.igemm with the exact-GELU epilogue, pmi_owl_box_out

backward(dlogits) is the class head's adjoint (pmi_owl_class_logits_bwd, the transposed-weight igemm), the merge's, and
VitEngine.backward_tokens.  The boxes carry no gradient (the reference's loss reads the logits only).

The queries are prepared once: TextEngine pooled at the EOS position (the arg-max id; the pad tokens come AFTER it and the mask is causal,
so they cannot reach the pooled row and the attention mask of the reference changes nothing there), text_projection, then
q / |q| + 1e-6 -- the 1e-6 is added to every component, the reference's operator precedence at modeling_owlvit.py:1270-1272, kept because
that is what it computes.

State-dict keys are transformers' ``OwlViTForObjectDetection`` names (``owlvit.vision_model.…``, ``owlvit.text_model.…``, ``class_head.…``,
``box_head.…``, ``layer_norm.…``); ``from_owlvit_vision_state_dict`` (engine/vit.py) / ``from_owlvit_text_state_dict`` (engine/text.py) map the towers to the OpenAI-CLIP names
VitEngine and TextEngine pack.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from .. import _hip
from .._hip import ACT_GELU, call, ptr
from . import ops
from .ops import PackedLinear
from .text import TextEngine, from_owlvit_text_state_dict, hf_text_state_dict_shapes
from .vit import VitEngine, _Lin, from_owlvit_vision_state_dict, hf_vision_state_dict_shapes

# google/owlvit-base-patch32: (image, patch, width, layers, heads, projection) and (context, vocab, width, layers, heads, projection)
OWLVIT_VISION_CONFIG = (768, 32, 768, 12, 12, 512)
OWLVIT_TEXT_CONFIG = (16, 49408, 512, 12, 8, 512)


def owlvit_state_dict_shapes(cfg, text_cfg) -> Dict[str, Tuple[int, ...]]:
    res, patch, width, layers, heads, out = cfg
    ctx, vocab, tw, tl, th, tout = text_cfg
    S = {"owlvit.logit_scale": ()}
    for k, shp in hf_text_state_dict_shapes(text_cfg, projection=False).items():
        S["owlvit." + k] = shp
    for k, shp in hf_vision_state_dict_shapes(cfg).items():
        if k != "visual_projection.weight":
            S["owlvit." + k.replace("pre_layrnorm", "pre_layernorm")] = shp
    S["owlvit.visual_projection.weight"] = (out, width)
    S["owlvit.text_projection.weight"] = (tout, tw)
    # the class head's dense0 maps to the TEXT width (modeling_owlvit.py:1249-1252) and is compared with the PROJECTED queries: the two agree
    S["class_head.dense0.weight"] = (tw, width); S["class_head.dense0.bias"] = (tw,)
    for nm in ("logit_shift", "logit_scale"):
        S[f"class_head.{nm}.weight"] = (1, width); S[f"class_head.{nm}.bias"] = (1,)
    for nm, o in (("dense0", width), ("dense1", width), ("dense2", 4)):
        S[f"box_head.{nm}.weight"] = (o, width); S[f"box_head.{nm}.bias"] = (o,)
    S["layer_norm.weight"] = (width,); S["layer_norm.bias"] = (width,)
    return S


def check_state_dict(sd, cfg, text_cfg) -> None:
    want = owlvit_state_dict_shapes(cfg, text_cfg)
    have = {k: v for k, v in sd.items() if not k.endswith("position_ids")}           # (buffers of older transformers versions)
    missing, extra = sorted(set(want) - set(have)), sorted(set(have) - set(want))
    if missing or extra:
        raise ValueError(f"OWL-ViT state dict: missing keys {missing[:4]}{'...' if len(missing) > 4 else ''}, "
                         f"unexpected keys {extra[:4]}{'...' if len(extra) > 4 else ''}")
    bad = [k for k in want if tuple(have[k].shape) != tuple(want[k])]
    if bad:
        raise ValueError(f"OWL-ViT state dict: {bad[0]} has shape {tuple(have[bad[0]].shape)}, expected {tuple(want[bad[0]])}")


def box_bias(grid: int) -> torch.Tensor:
    """[grid^2, 4] fp32 (modeling_owlvit.py:1311-1350): the logit of the normalised grid-corner coordinates ((x + 1) / grid, (y + 1) / grid,
    clipped to [0, 1]) and the logit of 1 / grid, both with the reference's 1e-4 guards; x runs fastest."""
    i = torch.arange(1, grid + 1, dtype=torch.float32)
    xy = torch.stack([i[None, :].expand(grid, grid), i[:, None].expand(grid, grid)], dim=-1) / torch.tensor([grid, grid], dtype=torch.float32)
    xy = xy.reshape(grid * grid, 2).clip(0.0, 1.0)
    coord = torch.log(xy + 1e-4) - torch.log1p(-xy + 1e-4)
    size = torch.full_like(coord, 1.0 / grid)
    return torch.cat([coord, torch.log(size + 1e-4) - torch.log1p(-size + 1e-4)], dim=-1).contiguous()


class OwlVitEngine:
    def __init__(self, cfg, text_cfg, state_dict, device, dtype="bf16"):
        self.cfg, self.text_cfg, self.device = tuple(cfg), tuple(text_cfg), torch.device(device)
        res, patch, width, layers, heads, out = self.cfg
        tw, tout = self.text_cfg[2], self.text_cfg[5]
        if tw != tout:
            raise ValueError(f"the class head compares dense0's output (the text width, {tw}) with the projected queries ({tout}): they must agree")
        if res % patch or width % 8 or width > 2048 or tw > 1024:
            raise ValueError("the OWL-ViT head kernels take a width that is a multiple of 8 up to 2048 and a class dimension up to 1024")
        check_state_dict(state_dict, self.cfg, self.text_cfg)
        sd = {k: v.detach().float() for k, v in state_dict.items()}
        self.vit = VitEngine(self.cfg, from_owlvit_vision_state_dict(sd), device, dtype, quick_gelu=True)
        self.text = TextEngine(self.text_cfg, from_owlvit_text_state_dict(sd), device, dtype, quick_gelu=True)
        self.dt, self.gscale = self.vit.dt, self.vit.gscale
        dev, dt = self.device, self.dt
        f32 = lambda k: sd[k].to(dev).contiguous()
        self.ln = (f32("layer_norm.weight"), f32("layer_norm.bias"))
        self.dim = tw
        # dense0 | logit_shift | logit_scale as ONE GEMM; rows padded with zeros to a multiple of 32 (the weights-direct GEMM's tile)
        npad = (tw + 2 + 31) // 32 * 32
        wc, bc = torch.zeros(npad, width), torch.zeros(npad)
        wc[:tw], bc[:tw] = sd["class_head.dense0.weight"], sd["class_head.dense0.bias"]
        wc[tw], bc[tw] = sd["class_head.logit_shift.weight"][0], sd["class_head.logit_shift.bias"][0]
        wc[tw + 1], bc[tw + 1] = sd["class_head.logit_scale.weight"][0], sd["class_head.logit_scale.bias"][0]
        self.cls = _Lin(wc, bc, dt, dev)
        self.box0 = PackedLinear(sd["box_head.dense0.weight"], sd["box_head.dense0.bias"], dt, dev)
        self.box1 = PackedLinear(sd["box_head.dense1.weight"], sd["box_head.dense1.bias"], dt, dev)
        self.box2 = (f32("box_head.dense2.weight"), f32("box_head.dense2.bias"))
        self._box_bias = {}
        self.saved = None

    # ---- text queries ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def prepare_queries(self, ids: torch.Tensor) -> torch.Tensor:
        """ids int64 [Q, T <= context], zero padded after the EOS token -> the prepared queries [Q, D] fp32: the EOS row (the arg-max id) of
        the text tower @ text_projection, then q / |q| + 1e-6 (module doc).  A query whose first id is 0 is a padded one in the reference
        (query_mask); those are refused."""
        if ids.ndim != 2 or ids.dtype != torch.int64:
            raise ValueError("ids must be an int64 tensor of shape [Q, T]")
        if bool((ids[:, 0] <= 0).any()):
            raise ValueError("a query starts with the pad id: padded queries (query_mask) are not supported")
        lengths = ids.argmax(dim=1) + 1
        _, pooled = self.text.forward(ids, lengths=lengths)
        return (pooled / torch.linalg.norm(pooled, dim=-1, keepdim=True) + 1e-6).contiguous()

    def box_bias(self, grid: int) -> torch.Tensor:
        if grid not in self._box_bias:
            self._box_bias[grid] = box_bias(grid).to(self.device)
        return self._box_bias[grid]

    # ---- heads, each on its own so that tests can drive one ----------------------------------------------------------------------------
    def merge(self, hidden: torch.Tensor):
        """hidden [N, T, W] fp32 -> (feats32 [N P, W], feats16, mr1 [2, N T], mr2 [2, N P])"""
        n, t, w = hidden.shape
        dev = hidden.device
        f32o = torch.empty((n * (t - 1), w), dtype=torch.float32, device=dev)
        f16o = torch.empty((n * (t - 1), w), dtype=_hip.TORCH_DTYPE[self.dt], device=dev)
        mr1 = torch.empty((2, n * t), dtype=torch.float32, device=dev)
        mr2 = torch.empty((2, n * (t - 1)), dtype=torch.float32, device=dev)
        call("pmi_owl_merge_ln_fwd", ptr(hidden), ptr(self.vit.ln_post[0]), ptr(self.vit.ln_post[1]), ptr(self.ln[0]), ptr(self.ln[1]),
             ptr(f32o), ptr(f16o), ptr(mr1), ptr(mr2), n, t, w, 1e-5, self.dt)
        return f32o, f16o, mr1, mr2

    def merge_backward(self, dfeats: torch.Tensor, hidden: torch.Tensor, mr1: torch.Tensor, mr2: torch.Tensor) -> torch.Tensor:
        n, t, w = hidden.shape
        dx = torch.empty_like(hidden)
        part = torch.empty((n, _hip.lib().pmi_owl_merge_bwd_blocks(t), w), dtype=torch.float32, device=hidden.device)
        call("pmi_owl_merge_ln_bwd", ptr(dfeats), ptr(hidden), ptr(self.vit.ln_post[0]), ptr(self.vit.ln_post[1]), ptr(self.ln[0]), ptr(mr1), ptr(mr2),
             ptr(dx), ptr(part), n, t, w)
        return dx

    def class_logits(self, f16: torch.Tensor, queries: torch.Tensor):
        """-> (logits [M, Q], class_embeds [M, D], g = the packed GEMM's output, kept for the backward)"""
        m, (q, d) = f16.shape[0], queries.shape
        g = ops.igemm(f16, self.cls.fwd, out_f32=True)
        logits = torch.empty((m, q), dtype=torch.float32, device=f16.device)
        ce = torch.empty((m, d), dtype=torch.float32, device=f16.device)
        call("pmi_owl_class_logits_fwd", ptr(g), g.shape[1], ptr(queries), ptr(logits), ptr(ce), m, d, q)
        return logits, ce, g

    def class_logits_backward(self, dlogits: torch.Tensor, g: torch.Tensor, queries: torch.Tensor) -> torch.Tensor:
        """dlogits [M, Q] fp32 (times gscale) -> dL/d image_feats [M, W] fp32 (times gscale)"""
        m, (q, d) = g.shape[0], queries.shape
        dg = torch.empty(g.shape, dtype=_hip.TORCH_DTYPE[self.dt], device=g.device)
        call("pmi_owl_class_logits_bwd", ptr(dlogits), ptr(g), g.shape[1], ptr(queries), ptr(dg), m, d, q, self.dt)
        return ops.igemm(dg, self.cls.bwd, out_f32=True)

    def boxes(self, f16: torch.Tensor, grid: int) -> torch.Tensor:
        """-> [M, 4] fp32 (cx, cy, w, h) in [0, 1]"""
        m, w = f16.shape
        h = ops.igemm(ops.igemm(f16, self.box0, act=ACT_GELU), self.box1, act=ACT_GELU)
        out = torch.empty((m, 4), dtype=torch.float32, device=f16.device)
        call("pmi_owl_box_out", ptr(h), h.shape[1], ptr(self.box2[0]), ptr(self.box2[1]), ptr(self.box_bias(grid)), ptr(out), m, grid * grid, w, self.dt)
        return out

    # ---- forward / backward -----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, images: torch.Tensor, queries: torch.Tensor, save: bool = False, boxes: bool = True):
        """images NCHW fp32 in [0, 1] (any size: resized to the tower's), queries [Q, D] from prepare_queries ->
        dict(logits [N, P, Q], boxes [N, P, 4] (cx, cy, w, h; None with boxes=False), class_embeds [N, P, D]), all fp32."""
        if not images.is_cuda:
            raise RuntimeError("OwlVitEngine runs on a HIP device only (no CPU fallback)")
        if queries.ndim != 2 or queries.shape[1] != self.dim or queries.dtype != torch.float32:
            raise ValueError(f"queries must be fp32 [Q, {self.dim}]")
        res, patch = self.cfg[:2]
        grid = res // patch
        queries = queries.to(self.device).contiguous()
        _, hidden, _ = self.vit.forward(images, save=save, features=True)
        hidden = hidden.contiguous()
        n, t, w = hidden.shape
        f32o, f16o, mr1, mr2 = self.merge(hidden)
        logits, ce, g = self.class_logits(f16o, queries)
        bx = self.boxes(f16o, grid).view(n, t - 1, 4) if boxes else None
        if save:
            self.saved = dict(vit=self.vit.saved, hidden=hidden, mr1=mr1, mr2=mr2, g=g, queries=queries)
        return dict(logits=logits.view(n, t - 1, -1), boxes=bx, class_embeds=ce.view(n, t - 1, -1), image_feats=f32o.view(n, t - 1, w))

    @torch.no_grad()
    def backward(self, dlogits: torch.Tensor, record=None) -> torch.Tensor:
        """dlogits: dL/d(logits) * self.gscale, fp32 [N, P, Q] -> dL/d(images), fp32 NCHW at the size forward() was given."""
        sv = self.saved
        if sv is None:
            raise RuntimeError("call forward(images, queries, save=True) before backward()")
        n, t, w = sv["hidden"].shape
        q = sv["queries"].shape[0]
        if dlogits.dtype != torch.float32 or tuple(dlogits.shape) != (n, t - 1, q):
            raise ValueError(f"dlogits must be fp32 [{n}, {t - 1}, {q}]")
        dl = dlogits.contiguous().view(n * (t - 1), q)
        dfeats = self.class_logits_backward(dl, sv["g"], sv["queries"])
        d_hidden = self.merge_backward(dfeats, sv["hidden"], sv["mr1"], sv["mr2"])
        if record is not None:
            record.update(dfeats=dfeats, d_hidden=d_hidden)
        self.vit.saved = sv["vit"]
        self.saved = None
        return self.vit.backward_tokens(d_hidden, record)

    @torch.no_grad()
    def topk_loss(self, logits: torch.Tensor, weights: torch.Tensor, top_k: int, mul: float = 1.0):
        """losses/owlvit.py:66-79 on logits [N, P, Q]: -> (loss, a 0-dim tensor; dloss/dlogits * mul)."""
        n, p, q = logits.shape
        logits = logits.contiguous()
        weights = weights.to(device=logits.device, dtype=torch.float32).contiguous()
        dl = torch.empty_like(logits)
        part = torch.empty(n * q, dtype=torch.float32, device=logits.device)
        call("pmi_owl_topk_loss", ptr(logits), ptr(weights), ptr(dl), ptr(part), n, p, q, int(top_k), float(mul))
        return part.sum(), dl
