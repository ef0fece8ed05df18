"""float64 torch restatement of the CLIP ViT image tower (OpenAI-CLIP VisionTransformer) and of its input gradient, written from the
architecture, with open_clip's ``visual.*`` state-dict key names:

  stem    patch x patch stride-patch convolution without bias (3 -> width) as a GEMM over im2col rows (k = c*p*p + py*p + px), the class
          embedding prepended, + positional_embedding, ln_pre
  block   x_mid = x_in + out_proj(attention(in_proj(ln_1 x_in)));  x_out = x_mid + c_proj(act(c_fc(ln_2 x_mid)))
          attention: heads of d = width / heads channels, channels of in_proj's output ordered (q | k | v) x (head, d), scale d^-1/2
          act: QuickGELU x sigmoid(1.702 x) or the exact GELU
  head    ln_post on the class token, @ proj

``Tower(sd, cfg, emulate=None)`` is the exact tower.  ``emulate=torch.bfloat16 | torch.float16`` restates the 16-bit storage of the HIP
engine: the GEMM weights rounded to the type (through fp32), and every tensor the engine stores in 16 bit rounded where it is stored --
the normalised patches, h = ln_1(x), qkv, the attention probabilities P, the attention output a, h2 = ln_2(x), the MLP's hidden pair
hpre / hact and the class token y16 = ln_post(x).  The residual stream, LayerNorm statistics, the patch embedding, x0 and the embedding stay
unrounded (fp32 on the device).  Two route flags place roundings:

  flash      True (head dim 64, the flash kernels): exp(s - max) is rounded, un-normalised, before P.V and the sum of the UNROUNDED values
             divides the product.  False (batched-GEMM path): softmax(s) is rounded, normalised, before P.V.
  fused_mlp  True (activation in the GEMM epilogue): hact = round(act(acc)) from the unrounded accumulator; hpre = round(acc) is kept for
             the backward pass only.  False: hpre = round(acc), hact = round(act(hpre)).

No autograd: the gradient is written out (``backward``), so that a pass can take the engine's own saved tensors (teacher forcing) and so
that ``bwd=`` can restate the 16-bit tensors of the engine's backward (d16, g16, dh, gm16, da, P, dS, dqkv, g0; ``fused_mlp_bwd``: dh and
dh * act'(hpre) are one rounding instead of two).  ``bwd=None`` is the reference the gates are measured against: the vjp of the
emulated forward linearised at the STORED values (P from the stored q and k, act' at the stored hpre, LayerNorm at the fp32 stream), every
rounding passed straight through.  ``work=torch.float32`` runs the same statements in fp32 arithmetic: a
stand-in for a device of that accumulation precision.  ``defect=`` swaps in one seeded defect (DEFECTS).

Nothing here calls the library under test.
"""
from __future__ import annotations

import math

import torch

MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)

U = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}

# ---- 16-bit roundings between the fp32 tensors a check compares (the gates of tests/test_gpu_vit_tower.py are sqrt(k) u) --------------
K_STEM_FWD = 1        # the normalised patches                                              (x0 from the image)
K_ATTN_FWD = 4        # h, qkv, P, a                                                        (x_mid - x_in from x_in)
K_MLP_FWD = 3         # h2, hpre, hact  (the fused epilogue rounds hact from the accumulator: hpre drops out, the count stays an upper one)
K_HEAD_FWD = 1        # y16                                                                 (emb from x_final)
K_HEAD_BWD = 1        # d16 (g16 is a copy of the fp32 g32 the check reads)                 (g32 at the last block's output from d_emb)
K_MLP_BWD = 3         # g16, dh, dh * act'(hpre)  (one rounding where the epilogue is fused) (gm32 - g32_in from g32_in)
K_ATTN_BWD = 5        # gm16, da, P (in P^T dO), dS, dqkv                                   (g32_out - gm32 from gm32)
K_ATTN_BWD_FLASH = 6  # the same + a: the flash backward takes delta = rowsum(dO * O) from the stored 16-bit attention output
K_QKV = 2             # h, qkv                                                              (the stored q, k, v from x_in)
K_HPRE = 2            # h2, hpre                                                            (the stored hpre from x_mid)
K_STEM_BWD = 1        # g0                                                                  (the image gradient from the first block's g32)


def depth_fwd(layers: int) -> int:
    """roundings on the longest path image -> embedding"""
    return K_STEM_FWD + layers * (K_ATTN_FWD + K_MLP_FWD) + K_HEAD_FWD


def depth_grad(layers: int, flash: bool = False) -> int:
    """roundings on the longest path image -> embedding -> image gradient"""
    return depth_fwd(layers) + K_HEAD_BWD + layers * (K_MLP_BWD + (K_ATTN_BWD_FLASH if flash else K_ATTN_BWD)) + K_STEM_BWD


DEFECTS = (
    "pad keys",          # the tp - t pad key columns (score 0, value 0) counted in the softmax
    "last key",          # the last key dropped from the softmax
    "lost row",          # the last token row of an MLP update lost (left zero)
    "head bwd",          # one head's contribution missing from the attention backward
    "slab",              # one split-K slab (the last quarter of K) dropped in c_proj
    "bias twice",        # c_proj's bias added by the GEMM and again by the slab reduction
    "gscale",            # f16: the gradient formed without the 65536 loss scale (every 16-bit tensor of the backward holds unscaled values)
    "patch shift",       # the last pixel row of every patch of the image gradient written one row up
    "pos last",          # the positional embedding of the last token omitted
    "x_mid ln",          # x_mid instead of x_in as the input of the attention branch's LayerNorm backward
)


def row_stat(got: torch.Tensor, ref: torch.Tensor) -> float:
    """max over rows (last dim) of |got - ref|_2 / max(|ref|_2, rms over rows of |ref|_2): the per-row statistic of the block checks."""
    got, ref = got.double().reshape(-1, got.shape[-1]), ref.double().reshape(-1, ref.shape[-1])
    rn = ref.norm(dim=1)
    floor = rn.square().mean().sqrt()
    return float(((got - ref).norm(dim=1) / torch.maximum(rn, floor)).max())


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.double() - ref.double()).norm() / ref.double().norm())


def patches(x: torch.Tensor, p: int) -> torch.Tensor:
    """NCHW -> [N, (H/p)(W/p), C*p*p] rows in im2col order (k = c*p*p + py*p + px): also the 3*p*p blocks of the per-patch gradient gate."""
    n, c, hh, ww = x.shape
    return x.reshape(n, c, hh // p, p, ww // p, p).permute(0, 2, 4, 1, 3, 5).reshape(n, (hh // p) * (ww // p), c * p * p)


def unpatches(col: torch.Tensor, n: int, res: int, p: int) -> torch.Tensor:
    g = res // p
    return col.reshape(n, g, g, 3, p, p).permute(0, 3, 1, 4, 2, 5).reshape(n, 3, res, res)


class Tower:
    def __init__(self, sd, cfg, emulate=None, quick_gelu=True, work=torch.float64, flash=None, fused_mlp=False, fused_mlp_bwd=False):
        self.cfg, self.dt, self.work, self.quick = tuple(cfg), emulate, work, quick_gelu
        res, patch, width, layers, heads, out = self.cfg
        self.d = width // heads
        self.flash = (self.d == 64) if flash is None else flash
        self.fused_mlp, self.fused_mlp_bwd = fused_mlp, fused_mlp_bwd
        f = lambda k: sd[k].detach().float().to(work)                                        # fp32 parameters, as the engine holds them
        w16 = lambda w: (w.detach().float() if emulate is None else w.detach().float().to(emulate)).to(work)     # packed GEMM weights
        self.wc = w16(sd["conv1.weight"].reshape(width, 3 * patch * patch))
        self.cls, self.pos = f("class_embedding"), f("positional_embedding")
        self.ln_pre = (f("ln_pre.weight"), f("ln_pre.bias"))
        self.ln_post = (f("ln_post.weight"), f("ln_post.bias"))
        self.proj = w16(sd["proj"])                                                          # [width, out]
        self.blocks = []
        for i in range(layers):
            p = f"transformer.resblocks.{i}."
            self.blocks.append(dict(
                ln1=(f(p + "ln_1.weight"), f(p + "ln_1.bias")), ln2=(f(p + "ln_2.weight"), f(p + "ln_2.bias")),
                qkv=(w16(sd[p + "attn.in_proj_weight"]), f(p + "attn.in_proj_bias")),
                out=(w16(sd[p + "attn.out_proj.weight"]), f(p + "attn.out_proj.bias")),
                fc=(w16(sd[p + "mlp.c_fc.weight"]), f(p + "mlp.c_fc.bias")),
                pr=(w16(sd[p + "mlp.c_proj.weight"]), f(p + "mlp.c_proj.bias"))))
        self.mean = torch.tensor(MEAN, dtype=work).view(1, 3, 1, 1)
        self.std = torch.tensor(STD, dtype=work).view(1, 3, 1, 1)

    # ---- pieces -------------------------------------------------------------------------------------------------------------------
    def r(self, x, dt="fwd"):
        """x as a stored 16-bit tensor (dt: the type, None = not rounded; default the forward's)"""
        dt = self.dt if dt == "fwd" else dt
        return x if dt is None else x.to(dt).to(self.work)

    @staticmethod
    def ln(x, gb):
        mean = x.mean(-1, keepdim=True)
        rstd = ((x - mean).square().mean(-1, keepdim=True) + 1e-5).rsqrt()
        return (x - mean) * rstd * gb[0] + gb[1]

    @staticmethod
    def ln_vjp(dy, x, gb):
        """dx = rstd (gy - mean(gy) - xhat mean(gy xhat)), gy = dy gamma"""
        mean = x.mean(-1, keepdim=True)
        rstd = ((x - mean).square().mean(-1, keepdim=True) + 1e-5).rsqrt()
        xh, gy = (x - mean) * rstd, dy * gb[0]
        return rstd * (gy - gy.mean(-1, keepdim=True) - xh * (gy * xh).mean(-1, keepdim=True))

    def act(self, x):
        return x * torch.sigmoid(1.702 * x) if self.quick else 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))

    def act_grad(self, x):
        if self.quick:
            s = torch.sigmoid(1.702 * x)
            return s * (1.0 + 1.702 * x * (1.0 - s))
        return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)

    def heads_of(self, z):
        """[N, T, heads*d] -> [N, heads, T, d]"""
        n, t, _ = z.shape
        return z.reshape(n, t, self.cfg[4], self.d).transpose(1, 2)

    def tokens_of(self, z):
        """[N, heads, T, d] -> [N, T, heads*d]"""
        n, h, t, d = z.shape
        return z.transpose(1, 2).reshape(n, t, h * d)

    # ---- forward ------------------------------------------------------------------------------------------------------------------
    def stem(self, images, defect=None):
        """images NCHW in [0, 1] at the tower's resolution -> x0 [N, T, width] (class token + patch embeddings + positions)"""
        res, patch, width = self.cfg[:3]
        x = images.to(self.work)
        n = x.shape[0]
        col = self.r(patches((x - self.mean) / self.std, patch))
        pe = col @ self.wc.t()
        pos = self.pos
        if defect == "pos last":
            pos = pos.clone()
            pos[-1] = 0
        return torch.cat([self.cls.expand(n, 1, width), pe], dim=1) + pos

    def attn(self, i, x_in, defect=None):
        """-> (ua = x_mid - x_in, saved): saved holds q, k, v [N, heads, T, d] and a [N, T, width] as stored (16-bit values)"""
        B = self.blocks[i]
        n, t, width = x_in.shape
        h = self.r(self.ln(x_in, B["ln1"]))
        qkv = self.r(h @ B["qkv"][0].t() + B["qkv"][1])
        q, k, v = (self.heads_of(z) for z in qkv.split(width, dim=-1))
        s = (q @ k.transpose(-1, -2)) * self.d ** -0.5
        if defect == "last key":
            s, v_ = s[..., :t - 1], v[..., :t - 1, :]
        elif defect == "pad keys":
            tp = (t + 7) // 8 * 8
            s = torch.cat([s, s.new_zeros(s.shape[:-1] + (tp - t,))], dim=-1)
            v_ = torch.cat([v, v.new_zeros(v.shape[:-2] + (tp - t, self.d))], dim=-2)
        else:
            v_ = v
        if self.flash:
            e = torch.exp(s - s.max(-1, keepdim=True).values)
            o = (self.r(e) @ v_) / e.sum(-1, keepdim=True)
        else:
            o = self.r(torch.softmax(s, dim=-1)) @ v_
        a = self.r(self.tokens_of(o))
        return a @ B["out"][0].t() + B["out"][1], dict(q=q, k=k, v=v, a=a)

    def mlp(self, i, x_mid, defect=None):
        """-> (um = x_out - x_mid, hpre as stored)"""
        B = self.blocks[i]
        acc = self.r(self.ln(x_mid, B["ln2"])) @ B["fc"][0].t() + B["fc"][1]
        hpre = self.r(acc)
        hact = self.r(self.act(acc if self.fused_mlp else hpre))
        w = B["pr"][0]
        if defect == "slab":
            kq = w.shape[1] // 4
            um = hact[..., :3 * kq] @ w[:, :3 * kq].t() + B["pr"][1]
        else:
            um = hact @ w.t() + B["pr"][1]
        if defect == "bias twice":
            um = um + B["pr"][1]
        if defect == "lost row":
            um = um.clone()
            um[-1, -1] = 0
        return um, hpre

    def head(self, x_final):
        return self.r(self.ln(x_final[:, 0], self.ln_post)) @ self.proj

    def forward(self, images, defect=None, block=0):
        """-> (emb [N, out], state): state holds what the engine saves for its backward; a block defect is seeded in block `block`."""
        x0 = self.stem(images, defect)
        x = self.ln(x0, self.ln_pre)
        st = dict(n=x.shape[0], x0=x0, layers=[])
        for i in range(len(self.blocks)):
            df = defect if i == block else None
            ua, sv = self.attn(i, x, df)
            x_mid = x + ua
            um, hpre = self.mlp(i, x_mid, df)
            st["layers"].append(dict(x_in=x, x_mid=x_mid, hpre=hpre, **sv))
            x = x_mid + um
        st["x_final"] = x
        return self.head(x), st

    # ---- input gradient -------------------------------------------------------------------------------------------------------------
    def head_vjp(self, d_emb, x_final, bwd=None):
        """d_emb [N, out] -> g32 [N, T, width] at the last block's output (zero but for the class token's row)"""
        dy = self.r(d_emb.to(self.work), bwd) @ self.proj.t()
        g = torch.zeros_like(x_final)
        g[:, 0] = self.ln_vjp(dy, x_final[:, 0], self.ln_post)
        return g

    def mlp_vjp(self, i, g, x_mid, hpre, bwd=None):
        """g: gradient at the block's output -> the MLP branch's contribution gm32 - g (act' at the stored hpre)"""
        B = self.blocks[i]
        acc = self.r(g, bwd) @ B["pr"][0]
        dh = self.r(acc * self.act_grad(hpre), bwd) if self.fused_mlp_bwd else self.r(self.r(acc, bwd) * self.act_grad(hpre), bwd)
        return self.ln_vjp(dh @ B["fc"][0], x_mid, B["ln2"])

    def attn_vjp(self, i, gm, x_in, sv, bwd=None, defect=None, x_mid=None):
        """gm: gradient at x_mid -> the attention branch's contribution g32_out - gm, from the stored q, k, v (and a, for the flash delta)"""
        B = self.blocks[i]
        q, k, v = sv["q"], sv["k"], sv["v"]
        scale = self.d ** -0.5
        dO = self.heads_of(self.r(self.r(gm, bwd) @ B["out"][0], bwd))
        p = torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1)
        p16 = self.r(p, bwd)
        dP = dO @ v.transpose(-1, -2)
        if bwd is None:
            delta, pds = (dP * p).sum(-1, keepdim=True), p
        elif self.flash:           # delta from the stored 16-bit O, dS from the recomputed P
            delta, pds = (dO * self.heads_of(sv["a"])).sum(-1, keepdim=True), p
        else:                      # batched-GEMM path: the stored 16-bit P throughout
            p16 = self.r(p, self.dt)
            delta, pds = (dP * p16).sum(-1, keepdim=True), p16
        dS = self.r(scale * pds * (dP - delta), bwd)
        dV, dQ, dK = p16.transpose(-1, -2) @ dO, dS @ k, dS.transpose(-1, -2) @ q
        if defect == "head bwd":
            dV, dQ, dK = (torch.cat([torch.zeros_like(z[:, :1]), z[:, 1:]], dim=1) for z in (dV, dQ, dK))
        dqkv = self.r(torch.cat([self.tokens_of(z) for z in (dQ, dK, dV)], dim=-1), bwd)
        return self.ln_vjp(dqkv @ B["qkv"][0], x_mid if defect == "x_mid ln" else x_in, B["ln1"])

    def stem_vjp(self, g, x0, n, bwd=None, gscale=1.0, defect=None):
        """g: gradient (times gscale) at the first block's input -> (g0, dcol, image gradient NCHW, unscaled)"""
        res, patch = self.cfg[:2]
        g0 = self.ln_vjp(g, x0, self.ln_pre)
        g0 = self.r(g0, bwd)
        dcol = g0[:, 1:] @ self.wc
        dimg = unpatches(dcol, n, res, patch) / self.std / gscale
        if defect == "patch shift":
            rows = torch.arange(res)
            last = rows % patch == patch - 1
            dimg = dimg.clone()
            dimg[:, :, rows[last] - 1], dimg[:, :, rows[last]] = dimg[:, :, rows[last]], torch.zeros_like(dimg[:, :, rows[last]])
        return g0, dcol, dimg

    def backward(self, d_emb, st, bwd=None, gscale=1.0, record=None, defect=None, block=0):
        """d_emb [N, out] (dL / d emb times gscale) and a forward state -> dL / d images.  record (a dict) receives what the engine's
        record= receives: g32 at the block boundaries (last block's output first), gm32 per block (last first), g0, dcol."""
        g = self.head_vjp(d_emb, st["x_final"], bwd)
        rec = dict(g32=[g], gm32=[])
        for i in reversed(range(len(self.blocks))):
            L, df = st["layers"][i], (defect if i == block else None)
            gm = g + self.mlp_vjp(i, g, L["x_mid"], L["hpre"], bwd)
            g = gm + self.attn_vjp(i, gm, L["x_in"], L, bwd, df, L["x_mid"])
            rec["gm32"].append(gm)
            rec["g32"].append(g)
        rec["g0"], rec["dcol"], dimg = self.stem_vjp(g, st["x0"], st["n"], bwd, gscale, defect)
        if record is not None:
            record.update(rec)
        return dimg

    def run(self, images, probe, bwd=None, gscale=1.0, defect=None):
        """One forward + backward under the GPU tests' unit probe on the normalised embedding, L = <emb / |emb|, probe>, as the dict
        tower_checks reads: emb, the forward state, d_emb (times gscale), the backward's record and grad = dL / d images."""
        emb, st = self.forward(images, defect if defect in FORWARD_DEFECTS else None)
        nrm = emb.norm(dim=1, keepdim=True)
        e = emb / nrm
        g = probe.to(self.work)
        if defect == "gscale":
            gscale = 1.0
        d_emb = (g - e * (e * g).sum(dim=1, keepdim=True)) / nrm * gscale
        rec = {}
        grad = self.backward(d_emb, st, bwd, gscale, rec, defect if defect in BACKWARD_DEFECTS else None)
        return dict(emb=emb, d_emb=d_emb, gscale=gscale, grad=grad, **st, **rec)


FORWARD_DEFECTS = ("pad keys", "last key", "lost row", "slab", "bias twice", "pos last")
BACKWARD_DEFECTS = ("head bwd", "patch shift", "x_mid ln")
SMALL_PROBE = 2.0 ** -14       # the probe scaled to where an f16 gradient formed without the loss scale leaves the normal range


def tower_checks(ref: Tower, images, probe, got, whole=None):
    """Every check of the tower tests on one run `got` (Tower.run's dict, or the same tensors taken from the HIP engine), against the
    float64 emulated tower `ref`: -> [(name, statistic, k)], to be held to statistic <= sqrt(k) u.

    Block by block, teacher-forced: each piece of `ref` is fed the run's OWN fp32 input of that piece (x_in, x_mid, x_final; the incoming
    g32 / gm32 and the stored q, k, v, hpre), so a statistic holds the roundings of that piece alone.  Per-row statistics are row_stat's
    (rows = tokens, or the 3 p p pixels of a patch).  whole = Tower.run of `ref` itself (bwd=None) for the whole-tower checks."""
    cfg = ref.cfg
    res, patch, width, layers, heads, out = cfg
    D = lambda z: z.double()
    n, gs = got["n"], got["gscale"]
    out_ = []
    add = lambda name, stat, k: out_.append((name, stat, k))
    add("stem x0", row_stat(got["x0"], ref.stem(images)), K_STEM_FWD)
    Ls = got["layers"]
    for i, L in enumerate(Ls):
        x_in, x_mid = D(L["x_in"]), D(L["x_mid"])
        x_out = D(Ls[i + 1]["x_in"] if i + 1 < layers else got["x_final"])
        ua, sv = ref.attn(i, x_in)
        um, hpre = ref.mlp(i, x_mid)
        add(f"block{i} qkv", row_stat(torch.stack([D(L[z]) for z in "qkv"]), torch.stack([sv[z] for z in "qkv"])), K_QKV)
        add(f"block{i} attn fwd", row_stat(x_mid - x_in, ua), K_ATTN_FWD)
        add(f"block{i} mlp fwd", row_stat(x_out - x_mid, um), K_MLP_FWD)
        if L.get("hpre") is not None:
            add(f"block{i} hpre", row_stat(L["hpre"], hpre), K_HPRE)
    add("head emb", row_stat(got["emb"], ref.head(D(got["x_final"]))), K_HEAD_FWD)
    # ---- backward: everything divided by gscale
    g32 = [D(g) / gs for g in got["g32"]]
    gm32 = [D(g) / gs for g in got["gm32"]]
    add("head bwd", row_stat(g32[0].reshape(n, -1, width)[:, 0], ref.head_vjp(D(got["d_emb"]) / gs, D(got["x_final"]))[:, 0]), K_HEAD_BWD)
    for j, i in enumerate(reversed(range(layers))):
        L = Ls[i]
        sh = L["x_in"].shape
        g_in, gm, g_out = g32[j].reshape(sh), gm32[j].reshape(sh), g32[j + 1].reshape(sh)
        sv = dict(q=D(L["q"]), k=D(L["k"]), v=D(L["v"]))
        add(f"block{i} mlp bwd", row_stat(gm - g_in, ref.mlp_vjp(i, g_in, D(L["x_mid"]), D(L["hpre"]))), K_MLP_BWD)
        add(f"block{i} attn bwd", row_stat(g_out - gm, ref.attn_vjp(i, gm, D(L["x_in"]), sv)), K_ATTN_BWD_FLASH if ref.flash else K_ATTN_BWD)
    g0, dcol, dimg = ref.stem_vjp(g32[-1].reshape(Ls[0]["x_in"].shape), D(got["x0"]), n)
    add("stem g0", row_stat(D(got["g0"]).reshape(g0.shape) / gs, g0), K_STEM_BWD)
    add("stem dcol", row_stat(D(got["dcol"]).reshape(n, -1, got["dcol"].shape[-1])[..., :dcol.shape[-1]] / gs, dcol), K_STEM_BWD)
    add("stem grad per patch", row_stat(patches(D(got["grad"]), patch), patches(dimg, patch)), K_STEM_BWD)
    if whole is not None:
        add("tower emb", rel_l2(got["emb"], whole["emb"]), depth_fwd(layers))
        add("tower grad", rel_l2(got["grad"], whole["grad"]), depth_grad(layers, ref.flash))
        add("tower grad per patch", row_stat(patches(D(got["grad"]), patch), patches(whole["grad"], patch)), depth_grad(layers, ref.flash))
    return out_


def small_probe_check(ref: Tower, grad_small, whole):
    """the gradient under the probe times SMALL_PROBE, scaled back, against the whole-tower reference: (name, statistic, k)"""
    return ("tower grad, small probe", rel_l2(grad_small.double() / SMALL_PROBE, whole["grad"]), depth_grad(ref.cfg[3], ref.flash))
