"""float64 references and derived bounds for the precise-mode (hi + lo f16 pairs) adjoint kernels of csrc/backward.hip and the fp32
attention backward of csrc/f32gemm.hip, plus dtype-generic restatements of the oracle UNets for the engine-level yardsticks.

Bounds follow tests/_norm_ref64.py: every kernel adds hi + lo on load (exact in fp32: both are f16 and |lo| <= ulp(hi) / 2), computes in fp32
(E32 = 2^-24 relative per operation, counted per kernel below) and splits the result on store, which keeps 2^-22 |y| + 2^-25
(out_round(., "precise")).  The GroupNorm and resampling adjoints reuse the references of their 16-bit twins with dtype "precise": the
arithmetic between load and store is the same template.  C_B = 1.5 is the project's slack on a first-order bound.

Defect models (`*_defect`) are what a wrong split handling would compute, evaluated in float64: tests/test_precise_grad_cpu.py requires each
to land at least 2x outside the bound."""
import torch

from _norm_ref64 import (C_B, E32, SPLIT_FLOOR, UN, avgpool_bwd_ref, bilinear_bwd_ref, from_split16, gn1_backward_ref,  # noqa: F401
                         gn_backward_ref, nearest_bwd_ref, out_round, split_round, to_split16)
from _precise_ref64 import chain_len, coherent_hi_lo  # noqa: F401


def hi_of(x: torch.Tensor) -> torch.Tensor:
    """the high half alone (float64) of a value the precise type stores"""
    return x.float().half().double()


def lo_of(x: torch.Tensor) -> torch.Tensor:
    return split_round(x) - hi_of(x)


def coherent(shape, seed, scale=1.0):
    """split-representable float64 values whose low halves all have the sign of their high halves (a dropped low half then moves every sum
    the same way, ~1.6e-4 relative, instead of cancelling)"""
    hi, lo = coherent_hi_lo(shape, seed, scale)
    return hi.double() + lo.double()


# ---- elementwise adjoints ----------------------------------------------------------------------------------------------------------------
def add_ref(a, b):
    """pmi_split_add: one fp32 add of the two joined values"""
    y = a + b
    return y, C_B * (E32 * y.abs() + out_round(y, "precise"))


def add_defect_halves(a, b):
    """the halves added separately as 16-bit values (pmi_add16 on the physical tensor): hi = f16(a_hi + b_hi), lo = f16(a_lo + b_lo)"""
    return (hi_of(a) + hi_of(b)).half().double() + (lo_of(a) + lo_of(b)).half().double()


def relu_mask_ref(g, y):
    """pmi_split_relu_bwd: a select, no arithmetic; the store re-splits an exact split value (no error), the bound keeps the contract"""
    out = torch.where(y > 0, g, torch.zeros_like(g))
    return out, C_B * out_round(out, "precise")


def relu_mask_defect_per_half(g, y):
    """each half masked by the sign of its own half of y (pmi_act_bwd on the physical tensor)"""
    return hi_of(g) * (hi_of(y) > 0) + lo_of(g) * (lo_of(y) > 0)


# ---- attention ---------------------------------------------------------------------------------------------------------------------------
def softmax_bwd_ref(dp, p, scale):
    """pmi_softmax_bwd_f32: dS = scale P o (dP - rowsum(dP o P)); the row sum is T / 64 serial fp32 terms per lane and 6 butterfly steps"""
    T = p.shape[-1]
    depth = (T + 63) // 64 + 6
    dot = (dp * p).sum(-1, keepdim=True)
    e_dot = (depth + 1) * E32 * (dp * p).abs().sum(-1, keepdim=True)
    ds = scale * p * (dp - dot)
    e = abs(scale) * p.abs() * (e_dot + E32 * (dp.abs() + dot.abs())) + 3 * E32 * ds.abs()
    return ds, C_B * e


def softmax_bwd_defect_no_rowsum(dp, p, scale):
    return scale * p * dp


def attn_backward_ref(q, k, v, do, scale):
    """float64 autograd of softmax(q k^T scale) v for d loss / d out = do ([B, T, d] each) and elementwise bounds of the precise route
    (ops.attention_precise_train / _backward): every product is an fp32 chain over its inner dimension (d or T terms, chain_len), the
    softmax carries the score error twice (max and exponent) plus expf / division, and errors propagate first order through the five
    products; the three outputs are stored split."""
    B, T, d = q.shape
    qr, kr, vr = (t.detach().clone().requires_grad_(True) for t in (q, k, v))
    with torch.enable_grad():
        p = torch.softmax(qr @ kr.transpose(1, 2) * scale, -1)
        dq, dk, dv = torch.autograd.grad(p @ vr, (qr, kr, vr), do)
    p = p.detach()
    cd, cT = chain_len(d, 1) + 2, chain_len(T, 1) + 2
    aq, ak, av, ado = q.abs(), k.abs(), v.abs(), do.abs()
    s = q @ k.transpose(1, 2) * scale
    e_s = cd * E32 * (aq @ ak.transpose(1, 2)) * abs(scale) + E32 * s.abs()
    e_p = p * (2 * e_s + (2 * s.abs() + (T + 63) // 64 + 14) * E32)                # exponent argument, expf, row sum, reciprocal, product
    e_p = e_p + p * (p * (2 * e_s)).sum(-1, keepdim=True)                          # the normaliser moves with every score of the row
    dp = do @ v.transpose(1, 2)
    e_dp = cd * E32 * (ado @ av.transpose(1, 2))
    dot = (dp * p).sum(-1, keepdim=True)
    e_dot = (e_p * dp.abs() + p * e_dp).sum(-1, keepdim=True) + ((T + 63) // 64 + 7) * E32 * (dp * p).abs().sum(-1, keepdim=True)
    ds = scale * p * (dp - dot)
    e_ds = abs(scale) * (e_p * (dp - dot).abs() + p * (e_dp + e_dot + E32 * (dp.abs() + dot.abs()))) + 3 * E32 * ds.abs()
    t = lambda m: m.transpose(1, 2)          # noqa: E731
    e_dq = e_ds @ ak + cT * E32 * (ds.abs() @ ak)
    e_dk = t(e_ds) @ aq + cT * E32 * (t(ds.abs()) @ aq)
    e_dv = t(e_p) @ ado + cT * E32 * (t(p) @ ado)
    tol = lambda e, y: C_B * (e + out_round(y, "precise"))          # noqa: E731
    return (dq, dk, dv), (tol(e_dq, dq), tol(e_dk, dk), tol(e_dv, dv))


# ---- the oracle UNets restated without their fp32 casts -----------------------------------------------------------------------------------------
# oracle/adm_unet.py and oracle/vdiff.py call .float() on the state dict, the input, GroupNorm and softmax, so they compute in fp32 whatever they
# are given.  The functions below restate their forward passes (same layer plans, same state-dict keys, same operation order) in the dtype of
# `dtype`: at torch.float32 they must reproduce the oracle (tests/test_precise_grad_cpu.py: <= 1e-6), at torch.float64 they are the yardstick.
# The v-diffusion restatement takes `masks` (name -> 0 / 1 tensor, NCHW): every ReLU of the UNet is then x * mask, which pins the piecewise-
# linear branches to the ones the engine took (the method of tests/_rn_ref64.py); the mapping network's ReLUs are not on the tape and stay free.
import math

import torch.nn.functional as F


def _adm_gn(sd, p, x):
    return F.group_norm(x, 32, sd[p + ".weight"], sd[p + ".bias"], eps=1e-5)


def _adm_res(sd, p, x, emb, cfg, up=False, down=False):
    h = F.silu(_adm_gn(sd, p + ".in_layers.0", x))
    if up:
        h, x = F.interpolate(h, scale_factor=2, mode="nearest"), F.interpolate(x, scale_factor=2, mode="nearest")
    elif down:
        h, x = F.avg_pool2d(h, 2), F.avg_pool2d(x, 2)
    h = F.conv2d(h, sd[p + ".in_layers.2.weight"], sd[p + ".in_layers.2.bias"], padding=1)
    e = F.linear(F.silu(emb), sd[p + ".emb_layers.1.weight"], sd[p + ".emb_layers.1.bias"])[:, :, None, None]
    if cfg.use_scale_shift_norm:
        scale, shift = e.chunk(2, dim=1)
        h = F.silu(_adm_gn(sd, p + ".out_layers.0", h) * (1 + scale) + shift)
    else:
        h = F.silu(_adm_gn(sd, p + ".out_layers.0", h + e))
    h = F.conv2d(h, sd[p + ".out_layers.3.weight"], sd[p + ".out_layers.3.bias"], padding=1)
    if (p + ".skip_connection.weight") in sd:
        w = sd[p + ".skip_connection.weight"]
        x = F.conv2d(x, w, sd[p + ".skip_connection.bias"], padding=w.shape[-1] // 2)
    return x + h


def _adm_attn(sd, p, x, heads, new_order):
    b, c, hh, ww = x.shape
    xf = x.reshape(b, c, -1)
    qkv = F.conv1d(_adm_gn(sd, p + ".norm", xf), sd[p + ".qkv.weight"], sd[p + ".qkv.bias"])
    t, ch = xf.shape[-1], c // heads
    if new_order:
        q, k, v = (z.reshape(b * heads, ch, t) for z in qkv.chunk(3, dim=1))
    else:
        q, k, v = qkv.reshape(b * heads, 3 * ch, t).split(ch, dim=1)
    s = ch ** -0.25
    w = torch.softmax(torch.einsum("bct,bcs->bts", q * s, k * s), dim=-1)
    a = torch.einsum("bts,bcs->bct", w, v).reshape(b, c, t)
    return (xf + F.conv1d(a, sd[p + ".proj_out.weight"], sd[p + ".proj_out.bias"])).reshape(b, c, hh, ww)


def adm_forward(sd, cfg_kw, x, timesteps, dtype):
    """oracle.adm_unet.adm_unet_forward in `dtype` (differentiable: no no_grad, x may require grad)"""
    from oracle import adm_unet as oa
    cfg = oa.AdmConfig(**cfg_kw) if isinstance(cfg_kw, dict) else cfg_kw
    sd = {k: v.to(dtype) for k, v in sd.items()}
    inp, mid, out = oa.block_plan(cfg)
    half = cfg.model_channels // 2
    freqs = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float32) / half)       # the oracle's fp32 table
    args = timesteps[:, None].to(dtype) * freqs[None].to(dtype)
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    emb = F.linear(emb, sd["time_embed.0.weight"], sd["time_embed.0.bias"])
    emb = F.linear(F.silu(emb), sd["time_embed.2.weight"], sd["time_embed.2.bias"])

    def run(layers, h):
        for p, kind, kw in layers:
            if kind == "conv":
                h = F.conv2d(h, sd[p + ".weight"], sd[p + ".bias"], padding=1)
            elif kind == "res":
                h = _adm_res(sd, p, h, emb, cfg, **kw)
            elif kind == "attn":
                h = _adm_attn(sd, p, h, kw["heads"], cfg.use_new_attention_order)
            elif kind == "downsample":
                h = F.conv2d(h, sd[p + ".op.weight"], sd[p + ".op.bias"], stride=2, padding=1) if cfg.conv_resample else F.avg_pool2d(h, 2)
            elif kind == "upsample":
                h = F.interpolate(h, scale_factor=2, mode="nearest")
                if cfg.conv_resample:
                    h = F.conv2d(h, sd[p + ".conv.weight"], sd[p + ".conv.bias"], padding=1)
        return h

    h, hs = x.to(dtype), []
    for layers in inp:
        h = run(layers, h)
        hs.append(h)
    h = run(mid, h)
    for layers in out:
        h = run(layers, torch.cat([h, hs.pop()], dim=1))
    return F.conv2d(F.silu(_adm_gn(sd, "out.0", h)), sd["out.2.weight"], sd["out.2.bias"], padding=1)


def adm_grad(sd, cfg_kw, x, t, probe, dtype=torch.float64):
    """(output, d <output[:, :3], probe> / d x) of the restated ADM UNet in `dtype`"""
    xr = x.to(dtype).clone().requires_grad_()
    with torch.enable_grad():
        y = adm_forward(sd, cfg_kw, xr, t, dtype)
        (g,) = torch.autograd.grad((y[:, :3] * probe.to(dtype)).sum(), xr)
    return y.detach(), g


def _fourier(t, weight):
    f = 2 * math.pi * t[:, None] @ weight.T
    return torch.cat([f.cos(), f.sin()], dim=-1)


def vdiff_forward(sd, spec, x, t, clip_embed, dtype, masks=None):
    """oracle.vdiff.vdiff_forward in `dtype`; masks: see above (keys "<block prefix>.1" / ".2" for the block's first / second ReLU)"""
    sd = {k: v.to(dtype) for k, v in sd.items()}
    t = t.to(dtype)

    def relu(v, key):
        return F.relu(v) if masks is None else v * masks[key].to(dtype)

    def mod(key, v, cond):
        scales, shifts = F.linear(cond, sd[key]).chunk(2, dim=-1)
        return torch.addcmul(shifts[..., None, None], v, scales[..., None, None] + 1)

    def res(p, v, l, cond):
        _, cin, cmid, cout, last = l
        if cond is None:
            h = relu(F.conv2d(v, sd[p + ".main.0.weight"], sd[p + ".main.0.bias"], padding=1), p + ".1")
            h = F.conv2d(h, sd[p + ".main.2.weight"], sd[p + ".main.2.bias"], padding=1)
            if not last:
                h = relu(h, p + ".2")
        else:
            h = F.conv2d(v, sd[p + ".main.0.weight"], sd[p + ".main.0.bias"], padding=1)
            h = relu(mod(p + ".main.2.layer.weight", F.group_norm(h, 1, eps=1e-5), cond), p + ".1")
            h = F.conv2d(h, sd[p + ".main.4.weight"], sd[p + ".main.4.bias"], padding=1)
            if not last:
                h = relu(mod(p + ".main.6.layer.weight", F.group_norm(h, 1, eps=1e-5), cond), p + ".2")
        return h + (v if cin == cout else F.conv2d(v, sd[p + ".skip.weight"]))

    def attn(p, v, heads):
        n, c, h, w = v.shape
        vn = F.group_norm(v, 1, sd[p + ".norm.weight"], sd[p + ".norm.bias"], eps=1e-5) if (p + ".norm.weight") in sd else v
        qkv = F.conv2d(vn, sd[p + ".qkv_proj.weight"], sd[p + ".qkv_proj.bias"])
        q, k, vv = qkv.view(n, heads * 3, c // heads, h * w).transpose(2, 3).chunk(3, dim=1)
        s = k.shape[3] ** -0.25
        y = (((q * s) @ (k.transpose(2, 3) * s)).softmax(3) @ vv).transpose(2, 3).contiguous().view(n, c, h, w)
        return v + F.conv2d(y, sd[p + ".out_proj.weight"], sd[p + ".out_proj.bias"])

    head_dim, up_mode, skip_first = spec.get("head_dim", 64), spec.get("up_mode", "bilinear"), spec.get("skip_first", False)

    def walk(layers, prefix, v, cond):
        for idx, l in enumerate(layers):
            p = f"{prefix}.{idx}"
            if l[0] == "res":
                v = res(p, v, l, cond)
            elif l[0] == "attn":
                v = attn(p, v, l[1] // head_dim)
            elif l[0] == "down":
                v = F.avg_pool2d(v, 2)
            elif l[0] == "up":
                v = F.interpolate(v, scale_factor=2, mode="nearest") if up_mode == "nearest" else \
                    F.interpolate(v, scale_factor=2, mode="bilinear", align_corners=False)
            elif l[0] == "skip":
                inner = walk(l[1], p + ".main", v, cond)
                v = torch.cat([v, inner], dim=1) if skip_first else torch.cat([inner, v], dim=1)
        return v

    cond = None
    if spec["cond"]:
        ce = F.normalize(clip_embed.to(dtype), dim=-1) * clip_embed.shape[-1] ** 0.5
        z = torch.cat([ce, _fourier(t, sd["mapping_timestep_embed.weight"])], dim=1)
        h = F.relu(F.linear(z, sd["mapping.0.main.0.weight"], sd["mapping.0.main.0.bias"]))
        h = F.relu(F.linear(h, sd["mapping.0.main.2.weight"], sd["mapping.0.main.2.bias"]))
        z = h + F.linear(z, sd["mapping.0.skip.weight"])
        h = F.relu(F.linear(z, sd["mapping.1.main.0.weight"], sd["mapping.1.main.0.bias"]))
        cond = F.linear(h, sd["mapping.1.main.2.weight"], sd["mapping.1.main.2.bias"]) + z
    tf = t
    if spec.get("t_input") == "log_snr":
        tf = torch.log(torch.cos(tf * math.pi / 2) ** 2 / torch.sin(tf * math.pi / 2) ** 2)
    planes = _fourier(tf, sd["timestep_embed.weight"])[..., None, None].repeat(1, 1, x.shape[2], x.shape[3])
    return walk(spec["net"], "net", torch.cat([x.to(dtype), planes], dim=1), cond)


def vdiff_grad(sd, ospec, x, t, probe, ce=None, dtype=torch.float64, masks=None):
    """(v, d <v, probe> / d x, d / d clip_embed or None) of the restated v-diffusion UNet in `dtype`, ReLUs pinned to `masks` if given"""
    xr = x.to(dtype).clone().requires_grad_()
    cer = ce.to(dtype).clone().requires_grad_() if ce is not None else None
    with torch.enable_grad():
        v = vdiff_forward(sd, ospec, xr, t, cer, dtype, masks)
        gs = torch.autograd.grad((v * probe.to(dtype)).sum(), [xr] + ([cer] if ce is not None else []))
    return v.detach(), gs[0], (gs[1] if ce is not None else None)


def tape_masks(tape, precise: bool, out=None):
    """ReLU masks of a VDiffEngine tape as {"<block prefix>.1" / ".2": NCHW 0/1 uint8 (CPU)}: the signs of the kept post-ReLU tensors"""
    out = {} if out is None else out
    for rec in tape:
        if rec[0] == "res":
            for key, y in ((".1", rec[3]), (".2", rec[4])):
                if y is not None:
                    val = from_split16(y.cpu()) if precise else y.cpu().float()
                    out[rec[2] + key] = (val > 0).permute(0, 3, 1, 2).to(torch.uint8)
        elif rec[0] == "skip":
            tape_masks(rec[1], precise, out)
    return out


def rel_l2(a, b):
    return float((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm())
