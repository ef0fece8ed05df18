"""float64 torch restatement of OWL-ViT open-vocabulary detection (transformers' OwlViTForObjectDetection as the reference vendors it) on
top of tests/_vit_ref64.py's tower, of the reference's top-k loss and of its post-processing, written from the architecture:

  queries   CLIP text tower (causal, QuickGELU), the row of the EOS token (the largest id), @ text_projection; q / |q| + 1e-6 -- the 1e-6
            added to every component (the vendored file's operator precedence)
  merge     y = post_layernorm(h) on all T tokens; f = layer_norm(y[1:] * y[0])
  class     e = dense0(f); logits = (e / (|e| + 1e-6) . q + logit_shift(f)) * (elu(logit_scale(f)) + 1)
  box       sigmoid(dense2(gelu(dense1(gelu(dense0(f))))) + box_bias), box_bias = logit of ((x + 1) / g, (y + 1) / g) and of 1 / g with 1e-4
            guards, computed in fp32 as the reference does
  loss      -0.01 sum_q w_q mean_{n, the k largest p} log_softmax_p(logits[n, :, q]),  k = min(top_k, P)
  post      scores = sigmoid(max_q logits), labels = argmax_q, boxes = corners(cx, cy, w, h) * (W, H, W, H)

``OwlVit(sd, cfg, text_cfg, emulate=None)`` is exact.  ``emulate=torch.bfloat16 | torch.float16`` rounds where the HIP engine stores 16 bit:
everything V.Tower rounds, and image_feats as the GEMM operand, the box head's two hidden tensors, the text tower's tensors, and in the
backward (``bwd=``) the gradient at the packed class-head GEMM output and the tower's 16-bit gradients.  The gradients are written out
(no autograd), linearised at the stored values as in V.Tower.  ``defect=`` swaps in one seeded defect (DEFECTS).

Nothing here calls the library under test.
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch

import _vit_ref64 as V

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

DEFECTS = (
    "merge row 1",        # the merge multiplies by token 1 instead of the class token
    "query eps inside",   # q / (|q| + 1e-6): the library's form
    "elu no +1",          # elu(scale) without the + 1
    "shift after scale",  # logits = e . q * scale + shift
    "mean over k",        # the loss divided by k only, not by N k
    "box xy swapped",     # the box bias with x and y exchanged
    "eos last",           # the text tower pooled at the last position instead of the EOS token
)

# 16-bit roundings between the last hidden state and the logits / boxes, and back (the sqrt(k) u convention of _vit_ref64)
K_CLASS_FWD = 1       # feats16
K_BOX_FWD = 3         # feats16, the two hidden tensors
K_CLASS_BWD = 1       # dg16


def load_fixture(name: str):
    """-> (state dict under transformers' names, float64; the reference's arrays) of configuration 'a' or 'b'"""
    W, R = np.load(os.path.join(GOLDEN, "owlvit_weights.npz")), np.load(os.path.join(GOLDEN, f"owlvit_reference_{name}.npz"))
    sd = {k[2:]: torch.as_tensor(W[k].astype(np.float64) * 2.0 ** int(W["e:" + k[2:]]), dtype=torch.float64) for k in W.files if k.startswith("w:")}
    if name == "b":
        sd.update({k[3:]: torch.as_tensor(W[k].astype(np.float64) * 2.0 ** int(W["eb:" + k[3:]]), dtype=torch.float64) for k in W.files if k.startswith("wb:")})
    return sd, {k: R[k] for k in R.files}


def vision_to_clip(sd):
    p = "owlvit.vision_model."
    g = lambda k: sd[k].detach().double()
    out = {"class_embedding": g(p + "embeddings.class_embedding"), "conv1.weight": g(p + "embeddings.patch_embedding.weight"),
           "positional_embedding": g(p + "embeddings.position_embedding.weight"),
           "ln_pre.weight": g(p + "pre_layernorm.weight"), "ln_pre.bias": g(p + "pre_layernorm.bias"),
           "ln_post.weight": g(p + "post_layernorm.weight"), "ln_post.bias": g(p + "post_layernorm.bias"),
           "proj": g("owlvit.visual_projection.weight").t().contiguous()}
    _blocks(sd, p, out)
    return out


def text_to_clip(sd):
    p = "owlvit.text_model."
    g = lambda k: sd[k].detach().double()
    out = {"token_embedding.weight": g(p + "embeddings.token_embedding.weight"), "positional_embedding": g(p + "embeddings.position_embedding.weight"),
           "ln_final.weight": g(p + "final_layer_norm.weight"), "ln_final.bias": g(p + "final_layer_norm.bias"),
           "text_projection": g("owlvit.text_projection.weight").t().contiguous()}
    _blocks(sd, p, out)
    return out


def _blocks(sd, p, out):
    g = lambda k: sd[k].detach().double()
    i = 0
    while f"{p}encoder.layers.{i}.layer_norm1.weight" in sd:
        a, b = f"{p}encoder.layers.{i}.", f"transformer.resblocks.{i}."
        out[b + "attn.in_proj_weight"] = torch.cat([g(a + f"self_attn.{n}_proj.weight") for n in "qkv"])
        out[b + "attn.in_proj_bias"] = torch.cat([g(a + f"self_attn.{n}_proj.bias") for n in "qkv"])
        for src, dst in (("self_attn.out_proj", "attn.out_proj"), ("layer_norm1", "ln_1"), ("layer_norm2", "ln_2"), ("mlp.fc1", "mlp.c_fc"),
                         ("mlp.fc2", "mlp.c_proj")):
            out[b + dst + ".weight"], out[b + dst + ".bias"] = g(a + src + ".weight"), g(a + src + ".bias")
        i += 1


def box_bias(grid: int, swap_xy: bool = False) -> torch.Tensor:
    """fp32 arithmetic as the reference's numpy / torch float32 code, returned as float64"""
    i = np.arange(1, grid + 1)
    xy = np.stack(np.meshgrid(i, i), axis=-1).astype(np.float32)
    if swap_xy:
        xy = xy[..., ::-1].copy()
    xy /= np.array([grid, grid], np.float32)
    xy = torch.from_numpy(xy.reshape(grid * grid, 2)).clip(0.0, 1.0)
    coord = torch.log(xy + 1e-4) - torch.log1p(-xy + 1e-4)
    size = torch.full_like(coord, 1.0 / grid)
    return torch.cat([coord, torch.log(size + 1e-4) - torch.log1p(-size + 1e-4)], dim=-1).double()


def elu1(s):
    return torch.where(s > 0, s, torch.expm1(s)) + 1.0


def elu1_grad(s):
    return torch.where(s > 0, torch.ones_like(s), torch.exp(s))


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


# ---- the loss and its gradient, closed form -------------------------------------------------------------------------------------------
def topk_sets(logits: torch.Tensor, top_k: int) -> torch.Tensor:
    """[N, P, Q] -> bool [N, P, Q]: the k_eff = min(top_k, P) largest tokens of every (n, q) column"""
    k = min(top_k, logits.shape[1])
    idx = logits.topk(k, dim=1).indices
    return torch.zeros_like(logits, dtype=torch.bool).scatter_(1, idx, True)


def topk_gap(logits: torch.Tensor, top_k: int) -> torch.Tensor:
    """[N, Q]: the k-th largest minus the (k + 1)-th largest logit over the tokens (inf where P <= k)"""
    p = logits.shape[1]
    if p <= top_k:
        return torch.full((logits.shape[0], logits.shape[2]), float("inf"), dtype=logits.dtype)
    s = logits.sort(dim=1, descending=True).values
    return s[:, top_k - 1] - s[:, top_k]


def topk_loss(logits: torch.Tensor, weights: torch.Tensor, top_k: int, defect=None):
    """-> (loss, dloss / dlogits)"""
    n, p, q = logits.shape
    k = min(top_k, p)
    sel = topk_sets(logits, top_k).to(logits.dtype)
    lsm = torch.log_softmax(logits, dim=1)
    coef = -0.01 * weights.to(logits.dtype) / (k if defect == "mean over k" else n * k)
    loss = ((lsm * sel).sum(dim=(0, 1)) * coef).sum()
    return loss, coef * (sel - k * lsm.exp())


def scores_mean_grad(logits: torch.Tensor) -> torch.Tensor:
    """d mean(sigmoid(max_q logits)) / dlogits"""
    n, p, q = logits.shape
    mx, idx = logits.max(dim=-1, keepdim=True)
    s = torch.sigmoid(mx)
    return torch.zeros_like(logits).scatter_(2, idx, s * (1 - s) / (n * p))


def post_process(logits, pred_boxes, size):
    """-> (boxes [N, P, 4] corners in pixels, scores [N, P], labels [N, P]); size = (H, W)"""
    mx, labels = logits.max(dim=-1)
    cx, cy, w, h = pred_boxes.unbind(-1)
    boxes = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)
    return boxes * torch.tensor([size[1], size[0], size[1], size[0]], dtype=boxes.dtype), torch.sigmoid(mx), labels


# ---- text tower ---------------------------------------------------------------------------------------------------------------------------
class Text:
    """cfg = (context, vocab, width, layers, heads, out).  emulate: the 16-bit storage of engine/text.TextEngine on its batched-GEMM causal
    attention (weights; h, qkv, P, a, h2, hact, the pooled row)."""

    def __init__(self, sd_clip, cfg, emulate=None):
        self.cfg, self.dt = tuple(int(c) for c in cfg), emulate
        ctx, vocab, width, layers, heads, out = self.cfg
        self.d = width // heads
        f = lambda k: sd_clip[k].double()
        self.w16 = lambda w: w.double() if emulate is None else w.float().to(emulate).double()
        self.tok, self.pos = f("token_embedding.weight"), f("positional_embedding")
        self.ln_final, self.proj = (f("ln_final.weight"), f("ln_final.bias")), self.w16(sd_clip["text_projection"])
        self.blocks = []
        for i in range(layers):
            p = f"transformer.resblocks.{i}."
            lin = lambda k, s="": (self.w16(sd_clip[p + k + (s or ".") + "weight"]), f(p + k + (s or ".") + "bias"))
            self.blocks.append(dict(ln1=(f(p + "ln_1.weight"), f(p + "ln_1.bias")), ln2=(f(p + "ln_2.weight"), f(p + "ln_2.bias")),
                                    qkv=lin("attn.in_proj", "_"), out=lin("attn.out_proj"), fc=lin("mlp.c_fc"), pr=lin("mlp.c_proj")))

    def r(self, x):
        return x if self.dt is None else x.to(self.dt).double()

    def forward(self, ids, defect=None):
        """ids int64 [Q, T] -> the projected EOS rows [Q, out]"""
        ctx, vocab, width, layers, heads, out = self.cfg
        n, t = ids.shape
        x = self.tok[ids] + self.pos[:t]
        mask = torch.full((t, t), float("-inf"), dtype=torch.float64).triu(1)
        ln = V.Tower.ln
        for B in self.blocks:
            qkv = self.r(self.r(ln(x, B["ln1"])) @ B["qkv"][0].t() + B["qkv"][1])
            q, k, v = (z.reshape(n, t, heads, self.d).transpose(1, 2) for z in qkv.split(width, dim=-1))
            s = (q @ k.transpose(-1, -2)) * self.d ** -0.5 + mask
            a = self.r((self.r(torch.softmax(s, dim=-1)) @ v).transpose(1, 2).reshape(n, t, width))
            x = x + a @ B["out"][0].t() + B["out"][1]
            acc = self.r(ln(x, B["ln2"])) @ B["fc"][0].t() + B["fc"][1]
            x = x + self.r(acc * torch.sigmoid(1.702 * acc)) @ B["pr"][0].t() + B["pr"][1]
        pos = torch.full((n,), t - 1) if defect == "eos last" else ids.argmax(dim=1)
        return self.r(ln(x, self.ln_final)[torch.arange(n), pos]) @ self.proj


# ---- the detector ---------------------------------------------------------------------------------------------------------------------------
class OwlVit:
    def __init__(self, sd, cfg, text_cfg, emulate=None, fused_mlp=False, fused_mlp_bwd=False):
        self.cfg, self.text_cfg, self.dt = tuple(int(c) for c in cfg), tuple(int(c) for c in text_cfg), emulate
        self.tower = V.Tower(vision_to_clip(sd), self.cfg, emulate=emulate, quick_gelu=True, fused_mlp=fused_mlp, fused_mlp_bwd=fused_mlp_bwd)
        self.text = Text(text_to_clip(sd), self.text_cfg, emulate)
        g = lambda k: sd[k].detach().double()
        w16 = self.text.w16
        self.ln = (g("layer_norm.weight"), g("layer_norm.bias"))
        self.dim = self.text_cfg[2]
        self.wc = w16(torch.cat([g("class_head.dense0.weight"), g("class_head.logit_shift.weight"), g("class_head.logit_scale.weight")]))
        self.bc = torch.cat([g("class_head.dense0.bias"), g("class_head.logit_shift.bias"), g("class_head.logit_scale.bias")])
        self.box = [(w16(g(f"box_head.dense{i}.weight")), g(f"box_head.dense{i}.bias")) for i in (0, 1)]
        self.box2 = (g("box_head.dense2.weight"), g("box_head.dense2.bias"))       # fp32 on the device: not rounded

    def r(self, x, dt="fwd"):
        dt = self.dt if dt == "fwd" else dt
        return x if dt is None else x.to(dt).double()

    def queries(self, ids, defect=None):
        q = self.text.forward(ids, defect)
        nrm = torch.linalg.norm(q, dim=-1, keepdim=True)
        return q / (nrm + 1e-6) if defect == "query eps inside" else q / nrm + 1e-6

    def merge(self, hidden, defect=None):
        y = V.Tower.ln(hidden, self.tower.ln_post)
        row = y[:, 1:2] if defect == "merge row 1" else y[:, :1]
        return V.Tower.ln(y[:, 1:] * row, self.ln)

    def merge_vjp(self, dfeats, hidden):
        """dL / d image_feats [N, P, W] -> dL / d hidden [N, T, W]"""
        y = V.Tower.ln(hidden, self.tower.ln_post)
        m = y[:, 1:] * y[:, :1]
        dm = V.Tower.ln_vjp(dfeats, m, self.ln)
        dy = torch.cat([(dm * y[:, 1:]).sum(dim=1, keepdim=True), dm * y[:, :1]], dim=1)
        return V.Tower.ln_vjp(dy, hidden, self.tower.ln_post)

    def class_head(self, feats, q, defect=None):
        """feats [N, P, W] (unrounded) -> (logits [N, P, Q], class_embeds [N, P, D], g = the packed GEMM output)"""
        g = self.r(feats) @ self.wc.t() + self.bc
        d = self.dim
        e, sh, s = g[..., :d], g[..., d:d + 1], g[..., d + 1:d + 2]
        eh = e / (torch.linalg.norm(e, dim=-1, keepdim=True) + 1e-6)
        sc = elu1(s) - (1.0 if defect == "elu no +1" else 0.0)
        dot = eh @ q.t()
        return (dot * sc + sh if defect == "shift after scale" else (dot + sh) * sc), eh, g

    def class_head_vjp(self, dlogits, g, q, bwd=None):
        """dlogits [N, P, Q] -> dL / d image_feats [N, P, W]; the gradient at g is rounded (bwd) as the engine's GEMM operand"""
        d = self.dim
        e, sh, s = g[..., :d], g[..., d:d + 1], g[..., d + 1:d + 2]
        nrm = torch.linalg.norm(e, dim=-1, keepdim=True)
        inv = 1.0 / (nrm + 1e-6)
        eh, sc = e * inv, elu1(s)
        dot = eh @ q.t()
        deh = (dlogits * sc) @ q
        de = deh * inv - e * (deh * e).sum(-1, keepdim=True) * inv * inv / nrm
        dsh = (dlogits * sc).sum(-1, keepdim=True)
        ds = (dlogits * (dot + sh)).sum(-1, keepdim=True) * elu1_grad(s)
        return self.r(torch.cat([de, dsh, ds], dim=-1), bwd) @ self.wc

    def box_head(self, feats, grid, defect=None):
        h = self.r(gelu(self.r(feats) @ self.box[0][0].t() + self.box[0][1]))
        h = self.r(gelu(h @ self.box[1][0].t() + self.box[1][1]))
        return torch.sigmoid(h @ self.box2[0].t() + self.box2[1] + box_bias(grid, defect == "box xy swapped"))

    def forward(self, images, ids, defect=None):
        """images NCHW in [0, 1] at the tower's resolution -> dict(logits, pred_boxes, class_embeds, image_feats, hidden, queries, g, st)"""
        _, st = self.tower.forward(images)
        hidden = st["x_final"]
        q = self.queries(ids, defect)
        feats = self.merge(hidden, defect)
        logits, ce, g = self.class_head(feats, q, defect)
        boxes = self.box_head(feats, self.cfg[0] // self.cfg[1], defect)
        return dict(logits=logits, pred_boxes=boxes, class_embeds=ce, image_feats=feats, hidden=hidden, queries=q, g=g, st=st)

    def backward_tokens(self, d_hidden, st, bwd=None, gscale=1.0, record=None):
        """V.Tower.backward's walk from a gradient on every token of the last hidden state (times gscale) -> dL / d images"""
        T = self.tower
        g = d_hidden
        rec = dict(g32=[g], gm32=[])
        for i in reversed(range(len(T.blocks))):
            L = st["layers"][i]
            gm = g + T.mlp_vjp(i, g, L["x_mid"], L["hpre"], bwd)
            g = gm + T.attn_vjp(i, gm, L["x_in"], L, bwd)
            rec["gm32"].append(gm)
            rec["g32"].append(g)
        rec["g0"], rec["dcol"], dimg = T.stem_vjp(g, st["x0"], st["n"], bwd, gscale)
        if record is not None:
            record.update(rec)
        return dimg

    def backward(self, dlogits, fw, bwd=None, gscale=1.0, record=None):
        """dlogits (times gscale) and forward()'s dict -> (dL / d images, dL / d hidden times gscale)"""
        dfeats = self.class_head_vjp(dlogits, fw["g"], fw["queries"], bwd)
        d_hidden = self.merge_vjp(dfeats, fw["hidden"])
        return self.backward_tokens(d_hidden, fw["st"], bwd, gscale, record), d_hidden

    def loss_and_grad(self, images, ids, weights, top_k, defect=None, bwd=None):
        fw = self.forward(images, ids, defect)
        loss, dl = topk_loss(fw["logits"], weights, top_k, defect)
        gs = 65536.0 if bwd == torch.float16 else 1.0
        grad, d_hidden = self.backward(dl * gs, fw, bwd, gs)
        return dict(loss=loss, grad=grad, d_hidden=d_hidden / gs, dlogits=dl, **fw)
