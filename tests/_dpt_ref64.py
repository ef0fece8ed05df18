"""float64 restatement of the DPT depth network (MiDaS dpt_large family), written from the architecture: timm's ViT, the project readout, the
reassembly, the four fusion blocks and the depth head, with the reference's state-dict keys (perceptor_amd.engine.dpt.dpt_state_dict_shapes).

  Dpt64(sd, cfg).forward(images, masks=None)  -> dict of every stage, as torch float64 tensors on an autograd graph
  masks: {site: bool tensor} pins the ReLU decisions (the gradient is piecewise constant in them); sites are
         "u{unit}.{block}.x" / "u{unit}.{block}.t" (a residual unit's input and middle), "h" (the head's 32-channel map) and "z" (the output)
  emulate=torch.bfloat16 / torch.float16: values are rounded where the engine stores 16-bit tensors -- in BOTH directions: the same points
         round the gradient on the way back (times gs, the engine's gradient scale), as the engine's 16-bit gradient tensors do
  defect=<name in DEFECTS>: one deliberate mistake, to show that a test would see it

Dpt64.forward_backward is the hand-written backward: it takes the ReLU masks and the upstream gradient, uses no autograd, and is held to
float64 autograd over forward() on the CPU.  (The emulated and the defect-carrying runs take autograd over the pinned forward.)
"""
from __future__ import annotations

import importlib
import math

import torch
import torch.nn.functional as F

RZ = importlib.import_module("perceptor_amd.transforms.resize")       # (the package exports the function under the same name)

# the toy configuration at which each defect is shown, (b) unless named: the epsilon shows only behind (a)'s small embedding, and the patch
# bias moves (a)'s depth by 2.8 bf16 gates against (b)'s 2.6
DEFECT_CONFIG = {"ln_eps_1e-5": "a", "patch_bias_dropped": "a"}
DEFECTS = ("align_corners_false", "ln_eps_1e-5", "readout_ignores_cls", "patch_bias_dropped", "taps_after_norm", "hook_off_by_one",
           "tap_grad_not_injected", "skip_after_relu", "missing_negation", "rcu1_in_refinenet4")


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dtype, gs):
        ctx.dtype, ctx.gs = dtype, gs
        return x.to(dtype).double()

    @staticmethod
    def backward(ctx, g):
        return (g * ctx.gs).to(ctx.dtype).double() / ctx.gs, None, None


def resize64(x, out_shape):
    """The engine's resize (transforms/resize.py: the reference's resize_right rule with its fp32 band weights -- the reference makes them in
    fp32 for float64 images too, so its resized images are reproduced exactly) applied in float64, differentiable."""
    method, dims = RZ._plan(x.shape[2], x.shape[3], tuple(out_shape))
    for _, axis, i, o in dims:
        idx, w = RZ.band_tables(i, o, method)[:2]
        w = torch.where(idx >= 0, w, torch.zeros_like(w)).double()
        g = x.index_select(axis, idx.clamp(min=0).long().reshape(-1))
        shp = list(x.shape)
        shp[axis:axis + 1] = [o, idx.shape[1]]
        wv = w.view([1] * axis + [o, idx.shape[1]] + [1] * (3 - axis))
        x = (g.view(shp) * wv).sum(axis + 1)
    return x


def up2(x, align_corners=True):
    return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=align_corners)


class Dpt64:
    def __init__(self, sd, cfg, emulate=None, defect=None, gs=1.0):
        assert defect is None or defect in DEFECTS, defect
        self.cfg, self.emulate, self.defect, self.gs = cfg, emulate, defect, float(gs)
        self.sd = {k: v.detach().double() for k, v in sd.items()}
        if emulate is not None:                 # weights the engine packs to 16 bits: matrices and convolutions; biases, norms, cls / pos stay fp32
            for k, v in self.sd.items():
                if v.ndim >= 2 and not k.endswith(("pos_embed", "cls_token")) and k != "scratch.output_conv.4.weight":
                    self.sd[k] = v.to(emulate).double()

    def r(self, x):
        return x if self.emulate is None else _Round.apply(x, self.emulate, self.gs)

    # ---- tower -------------------------------------------------------------------------------------------------------------------------
    def tower(self, x):
        res, patch, width, layers, heads, hooks, channels, features = self.cfg
        sd, p = self.sd, "pretrained.model."
        eps = 1e-5 if self.defect == "ln_eps_1e-5" else 1e-6
        n, g = x.shape[0], res // patch
        hooks = [min(h + 1, layers - 1) for h in hooks] if self.defect == "hook_off_by_one" else list(hooks)
        x = self.r((x - 0.5) / 0.5)
        tok = F.conv2d(x, sd[p + "patch_embed.proj.weight"], None, stride=patch).flatten(2).transpose(1, 2)
        if self.defect != "patch_bias_dropped":
            tok = tok + sd[p + "patch_embed.proj.bias"]
        x = torch.cat([sd[p + "cls_token"].expand(n, -1, -1), tok], 1) + sd[p + "pos_embed"]
        d = width // heads
        taps = {}
        for i in range(layers):
            b = f"{p}blocks.{i}."
            h = self.r(F.layer_norm(x, (width,), sd[b + "norm1.weight"], sd[b + "norm1.bias"], eps))
            qkv = self.r(F.linear(h, sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"])).view(n, -1, 3, heads, d).permute(2, 0, 3, 1, 4)
            pr = self.r(torch.softmax(qkv[0] @ qkv[1].transpose(-1, -2) / math.sqrt(d), -1))
            a = self.r((pr @ qkv[2]).transpose(1, 2).reshape(n, -1, width))
            x = x + F.linear(a, sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"])
            h = self.r(F.layer_norm(x, (width,), sd[b + "norm2.weight"], sd[b + "norm2.bias"], eps))
            h = self.r(F.linear(h, sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"]))
            x = x + F.linear(self.r(F.gelu(h)), sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"])
            for j, hk in enumerate(hooks):
                if hk == i:
                    taps[j] = x
        out = [taps[k] for k in range(4)]
        if self.defect == "taps_after_norm":
            out = [F.layer_norm(t, (width,), eps=eps) for t in out]
        if self.defect == "tap_grad_not_injected":
            out[1] = out[1].detach()
        return out

    # ---- decoder -----------------------------------------------------------------------------------------------------------------------
    def relu(self, x, site, masks, seen):
        m = masks.get(site) if masks is not None else None       # (a site the engine does not have -- a defect's -- decides for itself)
        if m is None:
            m = x > 0
        seen[site] = m
        return x * m

    def conv(self, x, key, **kw):
        return F.conv2d(x, self.sd[key + ".weight"], self.sd.get(key + ".bias"), **kw)

    def unit(self, x, key, site, masks, seen):
        t = self.r(self.relu(self.conv(self.relu(x, site + ".x", masks, seen), key + ".conv1", padding=1), site + ".t", masks, seen))
        skip = x * seen[site + ".x"] if self.defect == "skip_after_relu" else x
        return self.r(self.conv(t, key + ".conv2", padding=1) + skip)

    def forward(self, images, masks=None):
        res, patch, width, layers, heads, hooks, channels, features = self.cfg
        sd = self.sd
        n, g = images.shape[0], res // patch
        x = images.double()
        if tuple(x.shape[2:]) != (res, res):
            x = resize64(x, (res, res))
        resized = x
        taps = self.tower(x)
        maps, rn = [], []
        for k, tap in enumerate(taps, start=1):
            p = f"pretrained.act_postprocess{k}."
            wp = sd[p + "0.project.0.weight"]
            tok, cls = self.r(tap[:, 1:]), self.r(tap[:, :1])
            row = F.linear(cls, wp[:, width:], sd[p + "0.project.0.bias"])
            if self.defect == "readout_ignores_cls":
                row = sd[p + "0.project.0.bias"]
            y = self.r(F.gelu(self.r(F.linear(tok, wp[:, :width]) + row)))
            y = y.transpose(1, 2).reshape(n, width, g, g)
            y = self.r(self.conv(y, p + "3"))
            if k in (1, 2):
                kk = 6 - 2 * k
                y = self.r(self.r(F.conv_transpose2d(y, sd[p + "4.weight"], None, stride=kk)) + sd[p + "4.bias"].view(1, -1, 1, 1))
            elif k == 4:
                y = self.r(self.conv(y, p + "4", stride=2, padding=1))
            maps.append(y)
            rn.append(self.r(self.conv(y, f"scratch.layer{k}_rn", padding=1)))
        seen, sums, paths = {}, [None] * 4, [None] * 4
        ac = self.defect != "align_corners_false"
        x = rn[3]
        if self.defect == "rcu1_in_refinenet4":
            x = self.unit(x, "scratch.refinenet4.resConfUnit1", "u1.3", masks, seen)
        for k in (3, 2, 1, 0):
            f = f"scratch.refinenet{k + 1}."
            sums[k] = x
            q = self.r(self.conv(self.unit(x, f + "resConfUnit2", f"u2.{k}", masks, seen), f + "out_conv"))       # out_conv before the up-sampling (exact)
            paths[k] = up2(q, ac)
            if k > 0:
                x = self.r(paths[k] + self.unit(rn[k - 1], f"scratch.refinenet{k}.resConfUnit1", f"u1.{k - 1}", masks, seen))
            else:
                x = self.r(paths[k])
        hd = self.r(up2(self.r(self.conv(x, "scratch.output_conv.0", padding=1)), ac))
        h = self.r(self.relu(self.conv(hd, "scratch.output_conv.2", padding=1), "h", masks, seen))
        z = self.conv(h, "scratch.output_conv.4")
        depth = self.relu(z, "z", masks, seen)
        out = depth if self.defect == "missing_negation" else -depth
        return dict(resized=resized, taps=taps, maps=maps, rn=rn, sums=sums, paths=paths, path1=x, h=h, z=z, depth=out, masks=seen)

    # ---- the hand-written backward ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward_backward(self, images, d_depth, masks=None):
        """-> (depth, d <depth, d_depth> / d images, the ReLU masks used): the forward above once more, without autograd, keeping what the
        adjoints need, then every adjoint written out -- LayerNorm, softmax attention, exact GELU, the readout with its class row, the
        (transposed) convolutions, the bilinear up-sampling and the resize as transposed dense matrices, the ReLU masks as given.
        float64 only (no emulation, no defect).  tests/test_midas_depth_cpu.py holds it to autograd over forward()."""
        assert self.emulate is None and self.defect is None
        res, patch, width, layers, heads, hooks, channels, features = self.cfg
        sd, pm = self.sd, "pretrained.model."
        n, g, d, eps = images.shape[0], res // patch, width // heads, 1e-6
        seen = {}

        def relu(x, site):
            m = masks.get(site) if masks is not None else None
            seen[site] = (x > 0) if m is None else m
            return x * seen[site]

        def ln(x, w, b):
            mu = x.mean(-1, keepdim=True)
            r = ((x - mu).square().mean(-1, keepdim=True) + eps).rsqrt()
            xh = (x - mu) * r
            return xh * w + b, (xh, r, w)

        def ln_bwd(dy, kept):
            xh, r, w = kept
            dh = dy * w
            return r * (dh - dh.mean(-1, keepdim=True) - xh * (dh * xh).mean(-1, keepdim=True))

        def gelu_grad(h):
            return 0.5 * (1 + torch.erf(h / math.sqrt(2))) + h * torch.exp(-0.5 * h * h) / math.sqrt(2 * math.pi)

        def up_matrix(L):
            e = torch.eye(L, dtype=torch.float64).view(L, 1, L, 1)
            return F.interpolate(e, scale_factor=2, mode="bilinear", align_corners=True)[:, 0, :, 0].t().contiguous()      # [2L, L]

        def up(x):
            return torch.einsum("ai,ncij,bj->ncab", up_matrix(x.shape[2]), x, up_matrix(x.shape[3]))

        def up_bwd(gy):
            return torch.einsum("ai,ncab,bj->ncij", up_matrix(gy.shape[2] // 2), gy, up_matrix(gy.shape[3] // 2))

        def conv_bwd(gy, key, stride=1, padding=0):
            return F.conv_transpose2d(gy, sd[key + ".weight"], None, stride=stride, padding=padding, output_padding=stride - 1 if padding else 0)

        # ---- forward
        x = images.double()
        bands = []
        if tuple(x.shape[2:]) != (res, res):
            method, dims = RZ._plan(x.shape[2], x.shape[3], (res, res))
            for _, axis, i, o in dims:
                idx, w = RZ.band_tables(i, o, method)[:2]
                A = torch.zeros(o, i, dtype=torch.float64)
                for t in range(idx.shape[1]):
                    ok = idx[:, t] >= 0
                    A[torch.arange(o)[ok], idx[ok, t].long()] += w[ok, t].double()
                bands.append((axis, A))
                x = torch.einsum("oi,ncij->ncoj", A, x) if axis == 2 else torch.einsum("oj,ncij->ncio", A, x)
        xn = (x - 0.5) / 0.5
        tok = F.conv2d(xn, sd[pm + "patch_embed.proj.weight"], sd[pm + "patch_embed.proj.bias"], stride=patch).flatten(2).transpose(1, 2)
        x = torch.cat([sd[pm + "cls_token"].expand(n, -1, -1), tok], 1) + sd[pm + "pos_embed"]
        blocks, taps = [], {}
        for i in range(layers):
            b = f"{pm}blocks.{i}."
            h1, k1 = ln(x, sd[b + "norm1.weight"], sd[b + "norm1.bias"])
            q, k, v = F.linear(h1, sd[b + "attn.qkv.weight"], sd[b + "attn.qkv.bias"]).view(n, -1, 3, heads, d).permute(2, 0, 3, 1, 4)
            P = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1)
            a = (P @ v).transpose(1, 2).reshape(n, -1, width)
            x = x + F.linear(a, sd[b + "attn.proj.weight"], sd[b + "attn.proj.bias"])
            h2, k2 = ln(x, sd[b + "norm2.weight"], sd[b + "norm2.bias"])
            hp = F.linear(h2, sd[b + "mlp.fc1.weight"], sd[b + "mlp.fc1.bias"])
            x = x + F.linear(F.gelu(hp), sd[b + "mlp.fc2.weight"], sd[b + "mlp.fc2.bias"])
            blocks.append((k1, q, k, v, P, k2, hp))
            if i in hooks:
                taps[hooks.index(i)] = x
        pres, rn = [], []
        for kk in range(1, 5):
            p = f"pretrained.act_postprocess{kk}."
            wp, tap = sd[p + "0.project.0.weight"], taps[kk - 1]
            pre = F.linear(tap[:, 1:], wp[:, :width]) + F.linear(tap[:, :1], wp[:, width:], sd[p + "0.project.0.bias"])
            pres.append(pre)
            y = self.conv(F.gelu(pre).transpose(1, 2).reshape(n, width, g, g), p + "3")
            if kk in (1, 2):
                y = F.conv_transpose2d(y, sd[p + "4.weight"], sd[p + "4.bias"], stride=6 - 2 * kk)
            elif kk == 4:
                y = self.conv(y, p + "4", stride=2, padding=1)
            rn.append(self.conv(y, f"scratch.layer{kk}_rn", padding=1))

        def unit(x, key, site):
            t = relu(self.conv(relu(x, site + ".x"), key + ".conv1", padding=1), site + ".t")
            return self.conv(t, key + ".conv2", padding=1) + x

        def unit_bwd(gy, key, site):
            gt = conv_bwd(gy, key + ".conv2", padding=1) * seen[site + ".t"]
            return conv_bwd(gt, key + ".conv1", padding=1) * seen[site + ".x"] + gy

        x = rn[3]
        for kk in (3, 2, 1, 0):
            f = f"scratch.refinenet{kk + 1}."
            x = up(self.conv(unit(x, f + "resConfUnit2", f"u2.{kk}"), f + "out_conv"))
            if kk > 0:
                x = x + unit(rn[kk - 1], f"scratch.refinenet{kk}.resConfUnit1", f"u1.{kk - 1}")
        h = relu(self.conv(up(self.conv(x, "scratch.output_conv.0", padding=1)), "scratch.output_conv.2", padding=1), "h")
        depth = -relu(self.conv(h, "scratch.output_conv.4"), "z")
        # ---- backward
        gz = -d_depth.double() * seen["z"]
        gh = conv_bwd(gz, "scratch.output_conv.4") * seen["h"]
        gx = conv_bwd(up_bwd(conv_bwd(gh, "scratch.output_conv.2", padding=1)), "scratch.output_conv.0", padding=1)
        g_rn = [None] * 4
        for kk in (0, 1, 2, 3):
            f = f"scratch.refinenet{kk + 1}."
            gs = unit_bwd(conv_bwd(up_bwd(gx), f + "out_conv"), f + "resConfUnit2", f"u2.{kk}")
            g_rn[kk] = unit_bwd(gs, f + "resConfUnit1", f"u1.{kk}") if kk < 3 else gs
            gx = gs
        g_taps = []
        for kk in range(1, 5):
            p = f"pretrained.act_postprocess{kk}."
            gy = conv_bwd(g_rn[kk - 1], f"scratch.layer{kk}_rn", padding=1)
            if kk in (1, 2):
                gy = F.conv2d(gy, sd[p + "4.weight"], None, stride=6 - 2 * kk)            # the adjoint of ConvTranspose2d(kernel = stride)
            elif kk == 4:
                gy = conv_bwd(gy, p + "4", stride=2, padding=1)
            gy = conv_bwd(gy, p + "3").reshape(n, width, g * g).transpose(1, 2)
            gpre = gy * gelu_grad(pres[kk - 1])
            wp = sd[p + "0.project.0.weight"]
            g_taps.append(torch.cat([gpre.sum(1, keepdim=True) @ wp[:, width:], gpre @ wp[:, :width]], 1))
        gx = torch.zeros_like(taps[0])
        for i in range(layers - 1, -1, -1):
            if i in hooks:
                gx = gx + g_taps[hooks.index(i)]
            b = f"{pm}blocks.{i}."
            k1, q, k, v, P, k2, hp = blocks[i]
            ghp = (gx @ sd[b + "mlp.fc2.weight"]) * gelu_grad(hp)
            gx = gx + ln_bwd(ghp @ sd[b + "mlp.fc1.weight"], k2)
            ga = (gx @ sd[b + "attn.proj.weight"]).view(n, -1, heads, d).transpose(1, 2)
            gP, gv = ga @ v.transpose(-1, -2), P.transpose(-1, -2) @ ga
            gS = P * (gP - (gP * P).sum(-1, keepdim=True)) / math.sqrt(d)
            gqkv = torch.stack([gS @ k, gS.transpose(-1, -2) @ q, gv]).permute(1, 3, 0, 2, 4).reshape(n, -1, 3 * width)
            gx = gx + ln_bwd(gqkv @ sd[b + "attn.qkv.weight"], k1)
        gtok = gx[:, 1:].transpose(1, 2).reshape(n, width, g, g)
        gi = F.conv_transpose2d(gtok, sd[pm + "patch_embed.proj.weight"], None, stride=patch) / 0.5
        for axis, A in reversed(bands):
            gi = torch.einsum("oi,ncoj->ncij", A, gi) if axis == 2 else torch.einsum("oj,ncio->ncij", A, gi)
        return depth, gi, seen

    def reference_order_out_conv(self, x, k):
        """out_conv AFTER the up-sampling, as blocks.py:385-389 runs it (float64; the commuted order above must agree to rounding)."""
        return self.conv(up2(x), f"scratch.refinenet{k + 1}.out_conv")


# ---- the two toy configurations the tests run: (res, patch, width, layers, heads, hooks, reassemble channels, features) -------------------------
CONFIGS = {"a": (64, 16, 128, 4, 2, (0, 1, 2, 3), (16, 32, 64, 64), 32),          # T = 17, heads of 64 (the LDS-resident attention route)
           "b": (96, 16, 64, 6, 2, (0, 2, 3, 5), (16, 32, 64, 64), 64)}           # T = 37, heads of 32, the layer_4 map is 3 x 3
INPUT_HW = {"a": (64, 64), "b": (80, 112)}                                        # (b) is resized: the resize and its adjoint run
_toy = {}


def quantise(w):
    """w -> k 2^e with |k| <= 127: exact in bf16, f16 and fp32"""
    a = float(w.abs().max())
    e = math.ceil(math.log2(a / 127.0)) if a > 0 else 0
    return torch.round(w.double() / 2.0 ** e).clamp(-127, 127) * 2.0 ** e


def digest(sd):
    """sha256 over the names, shapes and fp32 bytes of every weight, in name order"""
    import hashlib
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode() + str(tuple(sd[k].shape)).encode() + sd[k].detach().float().contiguous().numpy().tobytes())
    return h.hexdigest()


def fit_head(cfg, sd, images):
    """The last 1 x 1 convolution for a fixture: weights along the linear discriminant that separates the dark image's 32-channel head map
    from the bright image's (within-class covariance with a 1 % ridge), scaled to max |w| = 1 and quantised; the bias, on a grid of 1 / 16,
    at the value with the fewest pixels whose |z| lies within 8 x the bf16-emulated error of zero among those that leave 20 - 80 % of the
    pixels active.  z is then two well separated clusters, one per image: the band holds under 2 % of the pixels."""
    sd = dict(sd)
    with torch.no_grad():
        H = Dpt64(sd, cfg).forward(images.double())["h"]
        X0, X1 = H[0].reshape(32, -1).t(), H[1].reshape(32, -1).t()
        Sw = torch.cov(X0.t()) + torch.cov(X1.t())
        Sw = Sw + 1e-2 * torch.trace(Sw) / 32 * torch.eye(32, dtype=Sw.dtype)
        w = torch.linalg.solve(Sw, X1.mean(0) - X0.mean(0))
        sd["scratch.output_conv.4.weight"] = quantise((w / w.abs().max()).reshape(1, 32, 1, 1)).float()
        sd["scratch.output_conv.4.bias"] = torch.zeros(1)
        z = Dpt64(sd, cfg).forward(images.double())["z"]
        err = float((Dpt64(sd, cfg, emulate=torch.bfloat16).forward(images.double())["z"] - z).abs().max())
        best = None
        for b in torch.arange(math.floor(-float(z.max())), -float(z.min()), 1 / 16):
            share, active = float(((z + b).abs() < 8 * err).double().mean()), float(((z + b) > 0).double().mean())
            if 0.2 <= active <= 0.8 and (best is None or share < best[0]):
                best = (share, float(b))
    return sd["scratch.output_conv.4.weight"], torch.tensor([best[1]], dtype=torch.float32)


def toy(name, head=None):
    """-> (cfg, state dict (fp32, every value k 2^e), images [2, 3, h, w] of 8-bit values / 255: one dark, one bright, with a little noise).
    The weights are name-keyed synthetic values but for the last 1 x 1 convolution, which fit_head chose when the fixture was generated
    (head="fit": tools/gen_midas_golden.py) and which is read from the fixture otherwise."""
    if name not in _toy:
        import os
        import numpy as np
        from perceptor_amd.engine.dpt import dpt_state_dict_shapes
        from perceptor_amd.utils.synth import seeded_noise, synth_tensor
        cfg = CONFIGS[name]
        sd = {k: quantise(synth_tensor(k, s, 0, rounding="none")).float() for k, s in dpt_state_dict_shapes(cfg).items()}
        # (a) only: a small embedding (variance ~1e-5 at the first LayerNorm), so that the epsilon, 1e-6 against CLIP's 1e-5, shows in the
        # output.  Weights of 2^-8 also make the gradient at the embedding 2^8 times the image gradient's size; (b)'s narrower LayerNorm
        # would take that beyond f16's range at the tower's fixed gradient scale
        for k in ("patch_embed.proj.weight", "patch_embed.proj.bias", "pos_embed", "cls_token") if name == "a" else ():
            sd["pretrained.model." + k] = sd["pretrained.model." + k] * 2.0 ** -8
        images = torch.empty((2, 3) + INPUT_HW[name])
        images[0], images[1] = 0.1, 0.9
        images = (images + seeded_noise(images.shape, 7) * 0.05).clamp(0, 1).mul(255).round() / 255
        if head == "fit":
            hw, hb = fit_head(cfg, sd, images)
        else:
            with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"midas_depth_reference_{name}.npz")) as g:
                hw, hb = torch.from_numpy(g["head_w"]).float().reshape(1, 32, 1, 1), torch.from_numpy(g["head_b"]).float().reshape(1)
        sd["scratch.output_conv.4.weight"], sd["scratch.output_conv.4.bias"] = hw, hb
        _toy[name] = (cfg, sd, images.float())
    return _toy[name]


def nhwc_mask(t):
    """an engine tensor [N, H, W, C] (16-bit, on any device) -> the bool mask (> 0) in the restatement's NCHW layout, on the CPU"""
    return (t.float().cpu() > 0).permute(0, 3, 1, 2).contiguous()


def engine_masks(rec_masks):
    """record["masks"] of DptEngine.backward -> the ``masks`` argument of Dpt64.forward"""
    m = {"h": nhwc_mask(rec_masks["h"]), "z": (rec_masks["out"].cpu() < 0)}
    for u in ("u1", "u2"):
        for k, st in enumerate(rec_masks[u]):
            if st is not None:
                m[f"{u}.{k}.x"], m[f"{u}.{k}.t"] = nhwc_mask(st[0]), nhwc_mask(st[1])
    return m


# ---- what the tests measure ---------------------------------------------------------------------------------------------------------------
def rel(a, b):
    """max |a - b| / max |b| over the whole tensor (b: the float64 side)"""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def upstream(name, kind):
    """d loss / d depth [2, 1, R, R]: "mean" (the reference's own test, depths.mean()) or "rand" (seeded noise)"""
    from perceptor_amd.utils.synth import seeded_noise
    r = CONFIGS[name][0]
    if kind == "mean":
        return torch.full((2, 1, r, r), 1.0 / (2 * r * r), dtype=torch.float64)
    return seeded_noise((2, 1, r, r), 11).double()


def grad_scale(d, dtype):
    """the factor the engine's 16-bit gradients carry: 1 for bf16; f16: 65536 and the power of two of ops.f16_grad_scale"""
    if dtype in ("bf16", torch.bfloat16):
        return 1.0
    from perceptor_amd.engine.ops import f16_grad_scale
    return 65536.0 * f16_grad_scale([float((d[i] * 65536.0).abs().max()) for i in range(d.shape[0])])


_free = {}


def free_run(name):
    """the float64 forward at toy(name), its own masks: what a fixture of the reference holds"""
    if name not in _free:
        cfg, sd, images = toy(name)
        with torch.no_grad():
            _free[name] = Dpt64(sd, cfg).forward(images.double())
    return _free[name]


def image_grad(model, images, d, masks=None):
    x = images.double().clone().requires_grad_(True)
    out = model.forward(x, masks=masks)
    (g,) = torch.autograd.grad((out["depth"] * d).sum(), x)
    return g, out


def measured(name, dtype):
    """distance of the emulated restatement from the exact one: depth against the free float64 run, the image gradients against float64
    pinned to the EMULATED run's masks (what a GPU test does with the engine's masks)"""
    cfg, sd, images = toy(name)
    td = {"bf16": torch.bfloat16, "f16": torch.float16}[dtype]
    out = {}
    for kind in ("mean", "rand"):
        d = upstream(name, kind)
        ge, oe = image_grad(Dpt64(sd, cfg, emulate=td, gs=grad_scale(d, dtype)), images, d)
        gx, _ = image_grad(Dpt64(sd, cfg), images, d, masks=oe["masks"])
        out["grad_" + kind] = rel(ge, gx)
        out["depth"] = rel(oe["depth"], free_run(name)["depth"])
        out["z_err"] = float((oe["z"].detach() - free_run(name)["z"]).abs().max())
    return out
