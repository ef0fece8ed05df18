"""float64 torch restatement of OpenAI's GLIDE CLIP (the noise-aware CLIP), written from the architecture, under the GLIDE checkpoints'
own state-dict key names (``blocks.input.*``, ``blocks.block_{i}.f_attn.* / f_mlp.*``, ``blocks.output.*``):

  image stem   a = (255 x - mean_c) / std_c on the 0..255 scale; a 4x4 stride-4 convolution without bias as a GEMM over im2col rows
               (k = c*16 + py*4 + px); token 0 of sample n = row ts[n] of the timestep table w_t; + w_pos; LayerNorm
  blocks       _vit_ref64.Tower's, with the exact GELU and NO key bias; plain attention over the 1 + (image / 4)^2 real tokens
  head         LayerNorm on token 0, @ f.w^T (no bias)
  text tower   w_voc[ids] + w_pos, the same blocks under a causal mask, the row at lengths - 1, LayerNorm, @ f.w^T

``GlideTower`` subclasses ``_vit_ref64.Tower``: blocks, head and the written-out backward are inherited, the stem and its vjp are restated
in full precision -- the HIP stem is fp32 end to end, so where the ViT tower rounds the normalised patches and g0 to 16 bit this one does
not (K_STEM_FWD = K_STEM_BWD = 0 in the rounding counts below).  ``DEFECTS`` are seeded defects for tests/test_glide_clip_cpu.py.

The stem kernels' element-wise fp32 bounds (``x0_tol``, ``dimg_tol``) are derived here; u32 = 2^-24 is the fp32 unit roundoff.

Nothing here calls the library under test.
"""
from __future__ import annotations

import math

import torch

import _vit_ref64 as V

MEAN = (122.77093945, 116.74601272, 104.09373519)
STD = (68.50053285, 66.63215831, 70.32316309)
U32 = 2.0 ** -24
P = 4
K = 3 * P * P

DEFECTS = (
    "ts sample",         # the timestep rows taken from the wrong sample (ts rolled by one)
    "key bias",          # the key third of in_proj_bias not zeroed (the query bias copied there)
    "quick gelu",        # QuickGELU where the tower has the exact GELU
    "norm scale",        # Normalize on the 0..1 scale: (x - mean) / std without the factor 255
    "token0 grad",       # token 0's gradient row not dropped: the patch rows read one token early
    "pos last",          # the positional embedding of the last token omitted
)


# ---- roundings on the longest paths, the ViT tower's counts without its two stem roundings ----------------------------------------------
def depth_fwd(layers: int) -> int:
    return V.depth_fwd(layers) - V.K_STEM_FWD


def depth_grad(layers: int, flash: bool = False) -> int:
    return V.depth_grad(layers, flash) - V.K_STEM_FWD - V.K_STEM_BWD


# ---- key maps ---------------------------------------------------------------------------------------------------------------------------
_BLOCK = (("f_attn.ln.g", "ln_1.weight"), ("f_attn.ln.b", "ln_1.bias"), ("f_attn.f_c.w", "attn.out_proj.weight"), ("f_attn.f_c.b", "attn.out_proj.bias"),
          ("f_mlp.ln.g", "ln_2.weight"), ("f_mlp.ln.b", "ln_2.bias"), ("f_mlp.f_1.w", "mlp.c_fc.weight"), ("f_mlp.f_1.b", "mlp.c_fc.bias"),
          ("f_mlp.f_2.w", "mlp.c_proj.weight"), ("f_mlp.f_2.b", "mlp.c_proj.bias"))
_IMAGE_ENDS = (("blocks.input.w_t", "w_t"), ("blocks.input.w_pos", "positional_embedding"), ("blocks.input.ln.g", "ln_pre.weight"),
               ("blocks.input.ln.b", "ln_pre.bias"), ("blocks.output.ln.g", "ln_post.weight"), ("blocks.output.ln.b", "ln_post.bias"))
_TEXT_ENDS = (("blocks.input.w_voc", "token_embedding.weight"), ("blocks.input.w_pos", "positional_embedding"),
              ("blocks.output.ln.g", "ln_final.weight"), ("blocks.output.ln.b", "ln_final.bias"))


def _blocks_to_clip(sd, out):
    i = 0
    while f"blocks.block_{i}.f_attn.ln.g" in sd:
        a, b = f"blocks.block_{i}.", f"transformer.resblocks.{i}."
        for src, dst in _BLOCK:
            out[b + dst] = sd[a + src]
        q, k, v = (sd[a + f"f_attn.f_{z}.w"] for z in "qkv")
        out[b + "attn.in_proj_weight"] = torch.cat([q, k, v], dim=0)
        out[b + "attn.in_proj_bias"] = torch.cat([sd[a + "f_attn.f_q.b"], torch.zeros(k.shape[0], dtype=k.dtype), sd[a + "f_attn.f_v.b"]])
        i += 1
    return i


def _blocks_from_clip(sd, out):
    i = 0
    while f"transformer.resblocks.{i}.ln_1.weight" in sd:
        a, b = f"blocks.block_{i}.", f"transformer.resblocks.{i}."
        for dst, src in _BLOCK:
            out[a + dst] = sd[b + src]
        w = sd[b + "attn.in_proj_weight"]
        width = w.shape[1]
        out[a + "f_attn.f_q.w"], out[a + "f_attn.f_k.w"], out[a + "f_attn.f_v.w"] = w.split(width, dim=0)
        bq, bk, bv = sd[b + "attn.in_proj_bias"].split(width)
        assert not bk.any(), "the GLIDE key projection has no bias"
        out[a + "f_attn.f_q.b"], out[a + "f_attn.f_v.b"] = bq, bv
        i += 1


def image_to_vit_names(sd):
    out = {dst: sd[src] for src, dst in _IMAGE_ENDS}
    out["conv1.weight"], out["proj"] = sd["blocks.input.patch_proj"], sd["blocks.output.f.w"].t()
    _blocks_to_clip(sd, out)
    return out


def image_from_vit_names(sd):
    """the inverse of the image key map: OpenAI-CLIP ``visual.*`` names (+ w_t) -> the GLIDE checkpoint's"""
    out = {src: sd[dst] for src, dst in _IMAGE_ENDS}
    out["blocks.input.patch_proj"], out["blocks.output.f.w"] = sd["conv1.weight"], sd["proj"].t()
    _blocks_from_clip(sd, out)
    return out


def text_to_clip_names(sd):
    out = {dst: sd[src] for src, dst in _TEXT_ENDS}
    out["text_projection"] = sd["blocks.output.f.w"].t()
    _blocks_to_clip(sd, out)
    return out


def text_from_clip_names(sd):
    out = {src: sd[dst] for src, dst in _TEXT_ENDS}
    out["blocks.output.f.w"] = sd["text_projection"].t()
    _blocks_from_clip(sd, out)
    return out


# ---- image tower ------------------------------------------------------------------------------------------------------------------------
class GlideTower(V.Tower):
    """cfg = (image, patch, width, layers, heads, out_dim, n_timestep); ts is fixed per tower instance (``at(ts)``) so that the inherited
    forward / run / backward, which know nothing of timesteps, apply unchanged."""

    def __init__(self, sd, cfg, emulate=None, work=torch.float64, defect=None, **kw):
        assert cfg[1] == P
        vsd = dict(image_to_vit_names(sd))
        vsd["class_embedding"] = torch.zeros(cfg[2])
        if defect == "key bias":
            for i in range(cfg[3]):
                b = vsd[f"transformer.resblocks.{i}.attn.in_proj_bias"].clone()
                b[cfg[2]:2 * cfg[2]] = b[:cfg[2]]
                vsd[f"transformer.resblocks.{i}.attn.in_proj_bias"] = b
        super().__init__(vsd, cfg[:6], emulate, quick_gelu=defect == "quick gelu", work=work, **kw)
        self.n_timestep = cfg[6]
        self.wc = sd["blocks.input.patch_proj"].detach().float().reshape(cfg[2], K).to(work)        # fp32 in the stem kernels: not rounded
        self.w_t = sd["blocks.input.w_t"].detach().float().to(work)
        self.mean = torch.tensor(MEAN, dtype=torch.float32).to(work).view(1, 3, 1, 1)              # fp32 constants, as the kernel reads them
        self.std = torch.tensor(STD, dtype=torch.float32).to(work).view(1, 3, 1, 1)
        self.ts = None

    def at(self, ts):
        self.ts = ts.clamp(0, self.n_timestep - 1)
        return self

    def normalised(self, images, defect=None):
        x = images.to(self.work)
        return (x - self.mean) / self.std if defect == "norm scale" else (255.0 * x - self.mean) / self.std

    def stem(self, images, defect=None):
        ts = self.ts.roll(1) if defect == "ts sample" else self.ts
        pe = V.patches(self.normalised(images, defect), P) @ self.wc.t()
        pos = self.pos
        if defect == "pos last":
            pos = pos.clone()
            pos[-1] = 0
        return torch.cat([self.w_t[ts][:, None], pe], dim=1) + pos

    def stem_vjp(self, g, x0, n, bwd=None, gscale=1.0, defect=None):
        """-> (g0, dcol, image gradient); nothing is rounded.  Token 0's row goes nowhere: the table is frozen."""
        g0 = self.ln_vjp(g, x0, self.ln_pre)
        dcol = (g0[:, :-1] if defect == "token0 grad" else g0[:, 1:]) @ self.wc
        return g0, dcol, V.unpatches(dcol, n, self.cfg[0], P) * 255.0 / self.std / gscale

    def run(self, images, probe, bwd=None, gscale=1.0, defect=None):
        fwd = defect if defect in ("ts sample", "norm scale", "pos last") else None
        emb, st = self.forward(images, fwd)
        nrm = emb.norm(dim=1, keepdim=True)
        e = emb / nrm
        g = probe.to(self.work)
        d_emb = (g - e * (e * g).sum(dim=1, keepdim=True)) / nrm * gscale
        rec = {}
        grad = self.backward(d_emb, st, bwd, gscale, rec, defect if defect == "token0 grad" else None)
        return dict(emb=emb, d_emb=d_emb, gscale=gscale, grad=grad, **st, **rec)


def cond_fn_grad(tower: GlideTower, x, z_t, logit_scale, grad_scale):
    """model_creation.py:60-74 in float64: x in [-1, 1] -> grad_scale * d/dx [logit_scale * sum(z_t * z_i)], z_i the unit embedding."""
    emb, st = tower.forward((x.to(tower.work) + 1) * 0.5)
    nrm = emb.norm(dim=1, keepdim=True)
    e = emb / nrm
    g = logit_scale * z_t.to(tower.work).expand_as(e)
    d_emb = (g - e * (e * g).sum(dim=1, keepdim=True)) / nrm
    return tower.backward(d_emb, st) * (0.5 * grad_scale)


def tower_checks(ref: GlideTower, images, probe, got, whole=None):
    """_vit_ref64.tower_checks for this tower: the block and head pieces teacher-forced at sqrt(k) u, the whole tower at the depths above.
    The fp32 stem is held element-wise by x0_tol / dimg_tol instead (tests/test_gpu_glide_clip.py)."""
    res, patch, width, layers, heads, out = ref.cfg
    D = lambda z: z.double()
    n, gs = got["n"], got["gscale"]
    out_ = []
    add = lambda name, stat, k: out_.append((name, stat, k))
    Ls = got["layers"]
    for i, L in enumerate(Ls):
        x_in, x_mid = D(L["x_in"]), D(L["x_mid"])
        x_out = D(Ls[i + 1]["x_in"] if i + 1 < layers else got["x_final"])
        ua, sv = ref.attn(i, x_in)
        um, hpre = ref.mlp(i, x_mid)
        add(f"block{i} qkv", V.row_stat(torch.stack([D(L[z]) for z in "qkv"]), torch.stack([sv[z] for z in "qkv"])), V.K_QKV)
        add(f"block{i} attn fwd", V.row_stat(x_mid - x_in, ua), V.K_ATTN_FWD)
        add(f"block{i} mlp fwd", V.row_stat(x_out - x_mid, um), V.K_MLP_FWD)
        if L.get("hpre") is not None:
            add(f"block{i} hpre", V.row_stat(L["hpre"], hpre), V.K_HPRE)
    add("head emb", V.row_stat(got["emb"], ref.head(D(got["x_final"]))), V.K_HEAD_FWD)
    g32 = [D(g) / gs for g in got["g32"]]
    gm32 = [D(g) / gs for g in got["gm32"]]
    add("head bwd", V.row_stat(g32[0].reshape(n, -1, width)[:, 0], ref.head_vjp(D(got["d_emb"]) / gs, D(got["x_final"]))[:, 0]), V.K_HEAD_BWD)
    for j, i in enumerate(reversed(range(layers))):
        L = Ls[i]
        sh = L["x_in"].shape
        g_in, gm, g_out = g32[j].reshape(sh), gm32[j].reshape(sh), g32[j + 1].reshape(sh)
        sv = dict(q=D(L["q"]), k=D(L["k"]), v=D(L["v"]))
        add(f"block{i} mlp bwd", V.row_stat(gm - g_in, ref.mlp_vjp(i, g_in, D(L["x_mid"]), D(L["hpre"]))), V.K_MLP_BWD)
        add(f"block{i} attn bwd", V.row_stat(g_out - gm, ref.attn_vjp(i, gm, D(L["x_in"]), sv)), V.K_ATTN_BWD_FLASH if ref.flash else V.K_ATTN_BWD)
    if whole is not None:
        add("tower emb", V.rel_l2(got["emb"], whole["emb"]), depth_fwd(layers))
        add("tower grad", V.rel_l2(got["grad"], whole["grad"]), depth_grad(layers, ref.flash))
        add("tower grad per patch", V.row_stat(V.patches(D(got["grad"]), patch), V.patches(whole["grad"], patch)), depth_grad(layers, ref.flash))
    return out_


# ---- the stem kernels' fp32 bounds ------------------------------------------------------------------------------------------------------
def _g(n):
    """gamma_n = n u / (1 - n u): n successive fp32 roundings"""
    return n * U32 / (1 - n * U32)


def x0_tol(images, w, pos, mean, std, x0_ref):
    """Element-wise bound on the patch rows of x0 = sum_k a_k w_jk + pos_j computed in fp32 (pmi_glide_embed_fwd), [N, T - 1, W].

    a_k = (255 x_k - m) / s is three fp32 operations.  255 x_k carries u |255 x_k| (absent when the compiler fuses it into the
    subtraction); the subtraction rounds relative to its result, the division (correctly rounded, counted twice for a compiler that
    expands it) likewise, so |da_k| <= u 255 |x_k| / s + 3 u |a_k|.  The 48 products are summed by one chain of FMAs from zero:
    gamma_48 sum_k |a_k w_jk|; adding the position rounds once more, relative to the result.  Together
        |dx0_j| <= (48 + 3) u sum_k |a_k w_jk|  +  u sum_k |w_jk| 255 |x_k| / s_k  +  u |x0_j|
    i.e. (3 P^2 + 3) u sum_k |a_k w_k| + u |x0| of the issue's form, plus the cancellation term of the Normalize (255 x_k is near
    the channel mean for mid-grey pixels, where a_k is small and its error is not).  gamma_n is used for n u."""
    x = images.double()
    m, s = mean.double().view(1, 3, 1, 1), std.double().view(1, 3, 1, 1)
    a = V.patches((255.0 * x - m) / s, P).abs()                       # [N, G^2, 48]
    big = V.patches(255.0 * x.abs() / s, P)
    wa = w.double().abs().t()                                         # [48, W]
    return _g(K + 3) * (a @ wa) + _g(1) * (big @ wa) + _g(1) * x0_ref.abs()


def dimg_tol(g, x0, gamma, mean, rstd, w, std, mul):
    """Element-wise bound on pmi_glide_embed_bwd's image gradient against the float64 evaluation of the same expression on the kernel's
    OWN inputs (g, x0, gamma, the mean / rstd it is handed, w, std, mul) -- teacher-forced, so the forward's error is not in it.
    g, x0: [N, T, W]; mean, rstd: [N, T]; -> (reference image gradient, bound), both [N, 3, R, R] float64.

    Per patch row, W = width, fp32 unit roundoff u:
      gy_j = g_j gamma_j                       one rounding
      xh_j = (x0_j - mean) rstd                two roundings, each relative to its result
      s1 = mean_j gy_j, s2 = mean_j gy_j xh_j  per lane a chain of W / 64 adds, six butterfly levels, one division: D1 = W / 64 + 7
                                               roundings on top of the terms' own (1 for gy; 1 + 2 + 1 = 4 for gy xh)
        |ds1| <= gamma_{D1+1} mean|gy|,  |ds2| <= gamma_{D1+4} mean|gy xh|
      dx_j = rstd (gy_j - s1 - xh_j s2)        at most six roundings of magnitudes bounded by A_j = rstd (|gy_j| + |s1| + |xh_j s2|)
                                               (gy, xh twice, the product, two subtractions, the factor rstd; fusing removes some)
        |ddx_j| <= gamma_6 A_j + rstd (|ds1| + |xh_j| |ds2|)
      c_k = sum_j w_jk dx_j                    four chains of W / 4 FMAs and three adds: D2 = W / 4 + 3
        |dc_k| <= sum_j |w_jk| |ddx_j| + gamma_D2 sum_j |w_jk dx_j|
      dimg = c_k * (mul * 255 / s)             three roundings
        |ddimg| <= |sc| (|dc_k| + gamma_3 |c_k| + gamma_3 |dc_k|)"""
    g, x0, gamma, w = g.double(), x0.double(), gamma.double(), w.double()
    n, t, width = x0.shape
    res = int(round(math.sqrt(t - 1))) * P
    mean, rstd = mean.double()[..., None], rstd.double()[..., None]
    gy = g * gamma
    xh = (x0 - mean) * rstd
    s1, s2 = gy.mean(-1, keepdim=True), (gy * xh).mean(-1, keepdim=True)
    dx = rstd * (gy - s1 - xh * s2)
    d1 = width // 64 + 7
    ds1 = _g(d1 + 1) * gy.abs().mean(-1, keepdim=True)
    ds2 = _g(d1 + 4) * (gy * xh).abs().mean(-1, keepdim=True)
    A = rstd * (gy.abs() + s1.abs() + (xh * s2).abs())
    ddx = _g(6) * A + rstd * (ds1 + xh.abs() * ds2)
    c = dx[:, 1:] @ w
    dc = ddx[:, 1:] @ w.abs() + _g(width // 4 + 3) * (dx[:, 1:].abs() @ w.abs())
    sc = (mul * 255.0 / std.double()).view(1, 3, 1, 1)
    ref = V.unpatches(c, n, res, P) * sc
    tol = (V.unpatches(dc, n, res, P) * (1 + _g(3)) + _g(3) * V.unpatches(c.abs(), n, res, P)) * sc.abs()
    return ref, tol


def stem_ratios(ref: GlideTower, images, got, mean_rstd=None):
    """The stem gates on one run `got` (x0, grad, the first block's incoming g32, gscale; mean_rstd [2, N T] as the backward kernel was
    handed it, else float64 statistics of x0): -> [(name, worst error / bound)].  Token 0 must equal fp32(w_t[ts] + pos[0]) exactly."""
    res, patch, width = ref.cfg[:3]
    n, gs = got["n"], got["gscale"]
    x0 = got["x0"].double().reshape(n, -1, width)
    want = ref.stem(images)
    out = [("stem x0 patch rows", float(((x0[:, 1:] - want[:, 1:]).abs() / x0_tol(images, ref.wc, ref.pos[1:], ref.mean.flatten(), ref.std.flatten(), want[:, 1:])).max()))]
    tok0 = (ref.w_t[ref.ts].float() + ref.pos[0].float()).double()
    out.append(("stem x0 token 0 (exact)", 0.0 if torch.equal(x0[:, 0], tok0) else float("inf")))
    if mean_rstd is None:
        mean, rstd = x0.mean(-1), 1 / torch.sqrt(x0.var(-1, unbiased=False) + 1e-5)
    else:
        mean, rstd = (z.double().reshape(n, -1) for z in mean_rstd)
    g = got["g32"][-1].double().reshape(x0.shape)
    dref, tol = dimg_tol(g, x0, ref.ln_pre[0], mean, rstd, ref.wc, ref.std.flatten(), 1.0 / gs)
    out.append(("stem image gradient", float(((got["grad"].double() - dref).abs() / tol).max())))
    return out


def ln_fwd_tol(x0, gamma, beta, eps=1e-5):
    """tests/test_gpu_transformer_kernels.py::test_layernorm_fwd's gates for the fp32 output, mean and rstd, on float64 LayerNorm of x0:
    -> (y, mean, rstd, tol_y rows, tol_mean rows, tol_rstd rows)"""
    x = x0.double()
    mean = x.mean(-1)
    rstd = 1 / torch.sqrt(x.var(-1, unbiased=False) + eps)
    y = torch.nn.functional.layer_norm(x, (x.shape[-1],), gamma.double(), beta.double(), eps)
    ty = 16 * U32 * (x.abs().amax(-1) * rstd * gamma.double().abs().max() + beta.double().abs().max() + y.abs().amax(-1))
    return y, mean, rstd, ty, 16 * U32 * x.abs().amax(-1), 64 * U32 * rstd


# ---- text tower -------------------------------------------------------------------------------------------------------------------------
class GlideText:
    """cfg = (context, vocab, width, layers, heads, out_dim).  emulate: the 16-bit storage of engine/text.TextEngine (weights; h, qkv, P or
    exp(s - max), a, h2, hact, the pooled row)."""

    def __init__(self, sd, cfg, emulate=None, work=torch.float64, flash=None):
        self.cfg, self.dt, self.work = tuple(cfg), emulate, work
        ctx, vocab, width, layers, heads, out = self.cfg
        self.d = width // heads
        self.flash = (self.d == 64) if flash is None else flash
        c = text_to_clip_names(sd)
        f = lambda k: c[k].detach().float().to(work)
        w16 = lambda w: (w.detach().float() if emulate is None else w.detach().float().to(emulate)).to(work)
        self.tok, self.pos = f("token_embedding.weight"), f("positional_embedding")
        self.ln_final = (f("ln_final.weight"), f("ln_final.bias"))
        self.proj = w16(c["text_projection"])
        self.blocks = []
        for i in range(layers):
            p = f"transformer.resblocks.{i}."
            self.blocks.append(dict(ln1=(f(p + "ln_1.weight"), f(p + "ln_1.bias")), ln2=(f(p + "ln_2.weight"), f(p + "ln_2.bias")),
                                    qkv=(w16(c[p + "attn.in_proj_weight"]), f(p + "attn.in_proj_bias")),
                                    out=(w16(c[p + "attn.out_proj.weight"]), f(p + "attn.out_proj.bias")),
                                    fc=(w16(c[p + "mlp.c_fc.weight"]), f(p + "mlp.c_fc.bias")),
                                    pr=(w16(c[p + "mlp.c_proj.weight"]), f(p + "mlp.c_proj.bias"))))

    def r(self, x):
        return x if self.dt is None else x.to(self.dt).to(self.work)

    def forward(self, ids, lengths):
        """-> (pooled [N, out], hidden [N, T, width] after the final LayerNorm)"""
        ctx, vocab, width, layers, heads, out = self.cfg
        n, t = ids.shape
        x = self.tok[ids] + self.pos[:t]
        mask = torch.full((t, t), float("-inf"), dtype=self.work).triu(1)
        ln = V.Tower.ln
        for B in self.blocks:
            qkv = self.r(self.r(ln(x, B["ln1"])) @ B["qkv"][0].t() + B["qkv"][1])
            q, k, v = (z.reshape(n, t, heads, self.d).transpose(1, 2) for z in qkv.split(width, dim=-1))
            s = (q @ k.transpose(-1, -2)) * self.d ** -0.5 + mask
            if self.flash:
                e = torch.exp(s - s.max(-1, keepdim=True).values)
                o = (self.r(e) @ v) / e.sum(-1, keepdim=True)
            else:
                o = self.r(torch.softmax(s, dim=-1)) @ v
            a = self.r(o.transpose(1, 2).reshape(n, t, width))
            x = x + a @ B["out"][0].t() + B["out"][1]
            acc = self.r(ln(x, B["ln2"])) @ B["fc"][0].t() + B["fc"][1]
            hact = self.r(0.5 * acc * (1.0 + torch.erf(acc / math.sqrt(2.0))))
            x = x + hact @ B["pr"][0].t() + B["pr"][1]
        row = x[torch.arange(n), lengths - 1]                       # gather, then LayerNorm (encoders.py:334-342)
        return self.r(ln(row, self.ln_final)) @ self.proj, ln(x, self.ln_final)


K_TEXT_BLOCK = V.K_ATTN_FWD + V.K_MLP_FWD


def depth_text(layers: int) -> int:
    """16-bit roundings on the path ids -> pooled embedding: per block h, qkv, P, a and h2, hpre, hact; the pooled row"""
    return layers * K_TEXT_BLOCK + 1
