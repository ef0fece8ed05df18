"""float64 torch restatement of the LPIPS distance (perceptor/losses/lpips.py is nothing more than
``lpips.LPIPS(net=name, lpips=linear_layers, spatial=spatial)(a, b, normalize=True)``), written from this definition
(lpips 0.1.x, version '0.1', net='vgg'):

1. Input.  Images in [0, 1] are mapped x <- 2x - 1.  Then ScalingLayer: (x - shift_c) / scale_c, with shift = (-.030, -.088, -.188) and
   scale = (.458, .448, .450).  This equals (img_c - mean_c) / std_c with mean_c = (1 + shift_c) / 2 and std_c = scale_c / 2.  The shift
   is not folded into conv1_1's bias: zero padding makes that wrong on the border.
2. VGG-16 tower.  torchvision VGG-16 ``features`` up to module 29: thirteen 3x3 pad-1 convolutions with bias, a ReLU after each, in
   groups of (2, 2, 3, 3, 3).  Convolutions are at modules 0, 2 | 5, 7 | 10, 12, 14 | 17, 19, 21 | 24, 26, 28.  MaxPool2d(2, 2) is at
   modules 4, 9, 16, 23.  Five taps come from the slices [0:4] [4:9] [9:16] [16:23] [23:30]: relu1_2, relu2_2, relu3_3, relu4_3,
   relu5_3.  Channels are (64, 128, 256, 512, 512).
3. Per level l.  u = f / (sqrt(sum_c f^2) + 1e-10) per pixel, on both sides.  d = (ua - ub)^2.  s_l[n,p] = sum_c w_{l,c} d_c, where w_l is
   the [1, C, 1, 1] weight of a bias-free 1x1 convolution.  Dropout is off in eval.  With linear_layers=False, w = 1.
4. Output.  spatial=False: sum_l mean_p s_l, shape [N, 1, 1, 1].  spatial=True: sum_l bilinear(s_l -> (H, W), align_corners=False),
   shape [N, 1, H, W].

Adjoint of a level.  Let r[n,p] = dL/ds_l[n,p], na = |fa| per pixel and q_c = 2 r w_c (ua_c - ub_c).  Then
   dfa = q / (na + eps) - fa (fa . q) / (na (na + eps)^2);
the b side is the same expression with the roles of a and b swapped (the level is symmetric: no sign flips).  At a pixel whose features
are all zero torch's autograd yields NaN (0 * inf through sqrt); the gradient is DEFINED as 0 there, here and in the engine.

Activations are keyed by the index of their CONVOLUTION.  ``emulate=torch.bfloat16 | torch.float16`` rounds every tensor where the HIP
engine stores one (the staged input, each convolution's activated output) and the weights; roundings pass gradients straight through.
``masks=`` (ReLU patterns) and ``routes=`` (pool selections) pin the discrete choices, as tests/_vgg_ref64.py.  ``defect=`` names one
seeded defect (DEFECTS).

Also here: the seeded inputs shared by tests/test_lpips_cpu.py and tests/test_gpu_lpips.py, and the per-element rounding bounds of the
kernels of csrc/lpips.hip (the |terms|-sum model of DESIGN.md section 19: fp32 accumulation over the actual number of terms, first order
with a few roundings of headroom, plus one 16-bit rounding of a 16-bit store).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from _vgg_ref64 import DTYPES, EPS32, UNIT, _gen, _rnd, first_max_route  # noqa: F401  (re-exported)

DEPTHS = (2, 2, 3, 3, 3)
WIDTHS = (64, 128, 256, 512, 512)
SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))
TAPS = (2, 7, 14, 21, 28)
TAP_NAMES = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")
LAST = 29
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
EPS = 1e-10
DEFECTS = ("no_norm", "w_before_square", "sum_pixels", "relu4_2", "fold_shift", "no_2x_minus_1", "no_projection", "negate_b")


def layer_table(widths):
    out, cin = [], 3
    for depth, w in zip(DEPTHS, widths):
        for _ in range(depth):
            out += [("conv", cin, w), ("relu",)]
            cin = w
        out.append(("pool",))
    return out[:LAST + 1]


# ---- tower ----------------------------------------------------------------------------------------------------------------------------
def stage(img, emulate=None, defect=None):
    """Images in [0, 1] -> the tower's input.  defect "no_2x_minus_1": the map x <- 2x - 1 is left out; "fold_shift": the shift is left to
    conv1_1's bias (``tower`` folds it there)."""
    x = img.double() if defect == "no_2x_minus_1" else 2 * img.double() - 1
    shift = torch.tensor(SHIFT, dtype=torch.float64).view(1, 3, 1, 1)
    scale = torch.tensor(SCALE, dtype=torch.float64).view(1, 3, 1, 1)
    x = x / scale if defect == "fold_shift" else (x - shift) / scale
    return _rnd(x, emulate)


def tower(sd, widths, img, emulate=None, masks=None, routes=None, defect=None):
    """img NCHW in [0, 1] (H, W multiples of 16) -> {conv index: post-ReLU activation}; sd: torchvision keys "{i}.weight" / "{i}.bias"."""
    dt = emulate
    x = stage(img, dt, defect)
    acts = {}
    for i, l in enumerate(layer_table(widths)):
        if l[0] == "conv":
            w, b = sd[f"{i}.weight"], sd[f"{i}.bias"].float().double()
            w = w.float().to(dt).double() if dt is not None else w.double()
            if i == 0 and defect == "fold_shift":                  # b' = b - sum_{c, ky, kx} w shift_c / scale_c: right inside, wrong at the border
                k = torch.tensor(SHIFT, dtype=torch.float64) / torch.tensor(SCALE, dtype=torch.float64)
                b = b - (w.sum(dim=(2, 3)) * k.view(1, 3)).sum(1)
            pre = F.conv2d(x, w, b, padding=1)
            x = _rnd(F.relu(pre) if masks is None else pre * masks[i].double(), dt)
            acts[i] = x
        elif l[0] == "pool":
            x = F.max_pool2d(x, 2, 2) if routes is None else F.avg_pool2d(x * routes[i].double(), 2) * 4
    return acts


def taps(acts, defect=None):
    """The five tap features.  defect "relu4_2": the fourth tap one convolution early."""
    return [acts[19 if (c == 21 and defect == "relu4_2") else c] for c in TAPS]


def engine_choices(acts, widths):
    """(masks, routes) of a tape of NCHW activations: what a float64 tower has to be pinned to."""
    masks = {i: (t > 0).double() for i, t in acts.items()}
    routes = {i: first_max_route(acts[i - 2]) for i, l in enumerate(layer_table(widths)) if l[0] == "pool"}
    return masks, routes


# ---- levels and outputs ---------------------------------------------------------------------------------------------------------------
def _norm(f):
    """sqrt(sum_c f^2) over dim 1 whose gradient is 0 (not NaN) at an all-zero pixel."""
    ss = f.square().sum(1, keepdim=True)
    pos = ss > 0
    return torch.where(pos, torch.where(pos, ss, torch.ones_like(ss)).sqrt(), torch.zeros_like(ss))


def level(fa, fb, w=None, defect=None):
    """fa, fb [N, C, ...] float64, w [C] or None -> s [N, 1, ...]."""
    shape = [1, fa.shape[1]] + [1] * (fa.dim() - 2)
    wv = torch.ones(shape, dtype=torch.float64) if w is None else w.double().reshape(shape)
    if defect == "no_norm":
        ua, ub = fa, fb
    else:
        ua, ub = fa / (_norm(fa) + EPS), fb / (_norm(fb) + EPS)
    if defect == "w_before_square":
        return (wv * (ua - ub)).square().sum(1, keepdim=True)
    return (wv * (ua - ub).square()).sum(1, keepdim=True)


def level_adjoint(fa, fb, w, r, defect=None):
    """(dfa, dfb) of sum(r * level(fa, fb, w)) by the formula in the module doc (channels on dim 1, r [N, 1, ...]); 0 at all-zero pixels.
    defects: "no_projection" drops the fa (fa . q) term, "negate_b" flips the b side's sign."""
    shape = [1, fa.shape[1]] + [1] * (fa.dim() - 2)
    wv = torch.ones(shape, dtype=torch.float64) if w is None else w.double().reshape(shape)
    na, nb = _norm(fa), _norm(fb)
    q = 2 * r * wv * (fa / (na + EPS) - fb / (nb + EPS))

    def side(f, n, qq):
        proj = f * (f * qq).sum(1, keepdim=True) / (torch.where(n > 0, n, torch.ones_like(n)) * (n + EPS).square())
        if defect == "no_projection":
            proj = torch.zeros_like(proj)
        return torch.where(n > 0, qq / (n + EPS) - proj, torch.zeros_like(f))

    dfa, dfb = side(fa, na, q), side(fb, nb, -q)
    return dfa, (-dfb if defect == "negate_b" else dfb)


def output(feats_a, feats_b, lins, hw, spatial=False, defect=None):
    """feats: the five NCHW tap features; lins: five [C] weights or None.  -> [N, 1, 1, 1] or [N, 1, H, W]."""
    total = 0.0
    for l, (fa, fb) in enumerate(zip(feats_a, feats_b)):
        s = level(fa, fb, None if lins is None else lins[l], defect)
        if spatial:
            total = total + F.interpolate(s, size=tuple(hw), mode="bilinear", align_corners=False)
        elif defect == "sum_pixels":
            total = total + s.sum(dim=(2, 3), keepdim=True)
        else:
            total = total + s.mean(dim=(2, 3), keepdim=True)
    return total


def lpips(sd, lins, widths, a, b, spatial=False, emulate=None, defect=None):
    fa = taps(tower(sd, widths, a, emulate, defect=defect), defect)
    fb = taps(tower(sd, widths, b, emulate, defect=defect), defect)
    return output(fa, fb, lins, a.shape[2:], spatial, defect)


def value_and_grads(sd, lins, widths, a, b, spatial=False, grad_out=None, emulate=None):
    """(output, d sum(grad_out * output) / da, / db) in float64 with autograd."""
    a = a.detach().double().clone().requires_grad_(True)
    b = b.detach().double().clone().requires_grad_(True)
    with torch.enable_grad():
        out = lpips(sd, lins, widths, a, b, spatial, emulate)
        go = torch.ones_like(out) if grad_out is None else grad_out.double()
        ga, gb = torch.autograd.grad((out * go).sum(), [a, b])
    return out.detach(), ga, gb


def pinned_grad(sd, lins, widths, img, acts, feats_other, side, spatial, grad_out, emulate, at_engine=True):
    """d sum(grad_out * output) / d img through the float64 emulated tower pinned to the engine's masks and routes (acts: the engine's tape
    as NCHW float64), the other side's tap features held at the engine's own.  side: "a" or "b".

    With masks and routes pinned the tower is linear in the image (the roundings pass gradients straight through), so its Jacobian does
    not depend on where it is evaluated; the level is smooth, so its adjoint does.  at_engine=True (the reference of the gradient gate)
    takes the level adjoint at the engine's own stored tap features -- the vjp the engine's backward computes, whose error is the 16-bit
    roundings of the backward path, as the gate sqrt(L) u models.  at_engine=False takes it at the emulated tower's own features: that
    adds the forward deviation between the two towers (held by the feature gates) times the level's conditioning (the gradient is the part
    of ub orthogonal to ua: 1 / sin of their angle), which no count of backward roundings models; printed for the record."""
    masks, routes = engine_choices(acts, widths)
    x = img.detach().double().clone().requires_grad_(True)
    with torch.enable_grad():
        f = taps(tower(sd, widths, x, emulate, masks=masks, routes=routes))
        at = [acts[c].detach().clone().requires_grad_(True) for c in TAPS] if at_engine else f
        out = output(at, feats_other, lins, img.shape[2:], spatial) if side == "a" else output(feats_other, at, lins, img.shape[2:], spatial)
        loss = (out * grad_out.double()).sum()
        if at_engine:
            seeds = torch.autograd.grad(loss, at)
            return torch.autograd.grad(f, x, seeds)[0]
        return torch.autograd.grad(loss, x)[0]


# ---- seeded inputs shared by the CPU and the GPU tests --------------------------------------------------------------------------------
LEVEL_SHAPES = ((1, 1, 16), (2, 37, 64), (3, 9, 48), (1, 130, 512), (2, 65, 128))       # (N, HW, C)
ENGINE_CONFIG = ((16, 16, 32, 32, 48), 2, (32, 48))                                      # widths, N, (H, W)
FEATURE_ROUNDINGS = (3, 5, 8, 11, 14)      # 16-bit stores up to each tap: the staged input + the convolutions before it
# the longest backward path stores a newly computed 16-bit value 17 times: the five level kernels and the dX convolutions of twelve of the
# thirteen convolutions (conv1_1's dX is fp32; ReLU masks and pool routes multiply by 0 / 1: exact)
GRAD_ROUNDINGS = 17


def level_inputs(shape, dt, seed=0):
    """A list of cases (fa, fb, w, r, g_in_a, g_in_b), all [N, HW, C] / [C] / [N, HW] on the CPU: post-ReLU-like features relu(randn)
    (about half zeros), non-negative w with mean 1 / C, r of both signs, g_in of both signs.  Every shape has a pixel that is all-zero on
    side a only, one on side b only and one on both: in one case when the shape has at least four pixels, else (a shape with a single
    pixel cannot hold the three at once) one case per pattern after an untouched first case."""
    n, hw, c = shape
    out = []
    patterns = [None] if n * hw >= 4 else [None, "a", "b", "ab"]
    for k, pat in enumerate(patterns):
        g = _gen(4000 + seed + 7 * n + 11 * hw + 13 * c + 101 * k)
        mk = lambda s=shape: torch.from_numpy(g.standard_normal(s, dtype=np.float32))
        fa, fb = mk().clamp_min(0), mk().clamp_min(0)
        w = mk((c,)).abs()
        w = (w / w.mean() / c).float()
        r = mk((n, hw)) / hw
        gia, gib = mk() * 0.01, mk() * 0.01
        if pat is None and n * hw >= 4:
            fa.view(-1, c)[0] = 0                                  # a only
            fb.view(-1, c)[1] = 0                                  # b only
            fa.view(-1, c)[n * hw - 1] = 0                         # both (the last pixel: a tail position of its wave)
            fb.view(-1, c)[n * hw - 1] = 0
        elif pat is not None:
            if "a" in pat:
                fa.view(-1, c)[0] = 0
            if "b" in pat:
                fb.view(-1, c)[0] = 0
        out.append((fa.to(dt), fb.to(dt), w, r.float(), gia.to(dt), gib.to(dt)))
    return out


def zero_pixel_patterns(cases):
    """The set of all-zero patterns ("a", "b", "ab") the cases of one shape contain."""
    found = set()
    for fa, fb, *_ in cases:
        za, zb = (fa.float().abs().sum(-1) == 0), (fb.float().abs().sum(-1) == 0)
        found |= ({"a"} if bool((za & ~zb).any()) else set()) | ({"b"} if bool((zb & ~za).any()) else set()) | \
                 ({"ab"} if bool((za & zb).any()) else set())
    return found


def engine_inputs():
    widths, n, (h, w) = ENGINE_CONFIG
    g = _gen(5000 + h + w)
    mk = lambda: torch.from_numpy(g.random((n, 3, h, w), dtype=np.float32))
    return mk(), mk()


def engine_weights(widths=ENGINE_CONFIG[0], seed=0):
    """(torchvision-keyed convolution weights, the five lin weight vectors) as losses.LPIPS's synthetic weights."""
    from perceptor_amd.losses.lpips import conv_key, synthetic_state_dict
    sd = synthetic_state_dict(widths, seed)
    convs = {}
    for i, l in enumerate(layer_table(widths)):
        if l[0] == "conv":
            convs[f"{i}.weight"], convs[f"{i}.bias"] = sd[f"{conv_key(i)}.weight"], sd[f"{conv_key(i)}.bias"]
    return convs, [sd[f"lin{k}.model.1.weight"].flatten() for k in range(5)]


def cl(f):
    """[N, HW, C] -> channels on dim 1: [N, C, HW] float64."""
    return f.double().permute(0, 2, 1)


# ---- per-element rounding bounds of csrc/lpips.hip ------------------------------------------------------------------------------------
# fp32 accumulation of K products in any order: |error| <= (K + 4) 2^-24 sum|terms| (tests/_vgg_ref64.py).  The chain of a level:
#   ss = sum_c f^2 (C terms, all positive)            relative error (C + 4) eps
#   n = sqrt(ss); i = 1 / (n + 1e-10)                 relative error of i: (C + 4) eps / 2 + 4 eps   (sqrt, add, divide, the absorbed 1e-10)
#   u_c = f_c i                                       relative error d_u = (C + 4) eps / 2 + 5 eps
#   d_c = ua_c - ub_c                                 e_c = d_u (|ua_c| + |ub_c|) + eps |d_c|
#   s = sum_c w_c d_c^2 (C terms, all positive)       sum_c w_c (2 |d_c| e_c + e_c^2) + (C + 4) eps s
def _du(c):
    return ((c + 4) / 2 + 5) * EPS32


def _level_parts(fa, fb, w):
    """fa, fb [N, HW, C] -> float64 pieces with channels last."""
    a, b = fa.double(), fb.double()
    c = a.shape[-1]
    wv = torch.ones(c, dtype=torch.float64) if w is None else w.double()
    na, nb = a.square().sum(-1, keepdim=True).sqrt(), b.square().sum(-1, keepdim=True).sqrt()
    ua, ub = a / (na + EPS), b / (nb + EPS)
    d = ua - ub
    e = _du(c) * (ua.abs() + ub.abs()) + EPS32 * d.abs()
    return a, b, wv, na, nb, ua, ub, d, e


def mean_chain(hw, c):
    """Longest chain of fp32 additions of pmi_lpips_level's mean: a lane's grid-stride tiles, the workgroup tree (6 + 2), the final
    kernel's pair of slots and tree (1 + 6 + 2), the scale."""
    tile = 4 * (64 // max(1, c // 8))                      # (c < 16: the hand case, which no kernel runs)
    tiles = -(-hw // tile)
    return -(-tiles // 512) + 6 + 2 + 1 + 6 + 2 + 1


def level_ref(fa, fb, w):
    """((s, na, nb, mean) in float64, their per-element bounds) of pmi_lpips_level; s, na, nb [N, HW], mean [N]."""
    a, b, wv, na, nb, ua, ub, d, e = _level_parts(fa, fb, w)
    c, hw = a.shape[-1], a.shape[1]
    s = (wv * d.square()).sum(-1)
    b_s = (wv * (2 * d.abs() * e + e.square())).sum(-1) + (c + 4) * EPS32 * s
    b_n = ((c + 4) / 2 + 2) * EPS32
    mean = s.mean(-1)
    b_mean = b_s.mean(-1) + (mean_chain(hw, c) + 4) * EPS32 * mean
    return (s, na[..., 0], nb[..., 0], mean), (b_s, b_n * na[..., 0], b_n * nb[..., 0], b_mean)


def level_bwd_ref(fa, fb, w, r, gia, gib, gscale, dt, defect=None):
    """((dFa, dFb) float64 before the 16-bit store, (bound_a, bound_b)) of pmi_lpips_level_bwd; all [N, HW, C], r [N, HW].
    The chain after d_c (above):  q_c = 2 r w_c d_c: 2 |r| w_c e_c + 3 eps |q_c|;  f . q (C terms): (C + 4) eps sum|f_c q_c| +
    sum |f_c| err(q_c);  p = (f . q) i^2 / n: relative (C + 4) eps * 1.5 + 16 eps on top;  t1 = q_c i, t2 = f_c p, t1 - t2, the scale,
    the sum with g_in: one rounding each; then the 16-bit store."""
    a, b, wv, na, nb, ua, ub, d, e = _level_parts(fa, fb, w)
    c = a.shape[-1]
    rr = r.double().unsqueeze(-1)
    q = 2 * rr * wv * d
    e_q = 2 * rr.abs() * wv * e + 3 * EPS32 * q.abs()
    u16 = UNIT[dt]
    outs, bounds = [], []
    for f, n, qq, gin, flip in ((a, na, q, gia, False), (b, nb, -q, gib, True)):
        i = 1.0 / (n + EPS)
        safe_n = torch.where(n > 0, n, torch.ones_like(n))
        dot = (f * qq).sum(-1, keepdim=True)
        e_dot = (c + 4) * EPS32 * (f * qq).abs().sum(-1, keepdim=True) + (f * e_q).sum(-1, keepdim=True)
        p = dot * i * i / safe_n
        e_p = (e_dot * i * i / safe_n) + (1.5 * (c + 4) + 16) * EPS32 * p.abs()
        t1, t2 = qq * i, f * p
        if defect == "no_projection":
            t2 = torch.zeros_like(t2)
        e_t = e_q * i + (_du(c) + EPS32) * t1.abs() + f * e_p + EPS32 * t2.abs()
        df = t1 - t2
        if defect == "negate_b" and flip:
            df = -df
        g = gin.double() if gin is not None else torch.zeros_like(f)
        v = gscale * df + g
        fp32 = gscale * (e_t + 2 * EPS32 * df.abs()) + 2 * EPS32 * (v.abs() + g.abs())
        live = f > 0
        v = torch.where(live, v, torch.zeros_like(v))
        bound = fp32 + u16 * v.abs() + (EPS32 if dt == torch.float16 else 0.0)
        outs.append(v)
        bounds.append(torch.where(live, bound, torch.zeros_like(bound)))
    return tuple(outs), tuple(bounds)


def value_bound(feats_a, feats_b, lins, hw, spatial):
    """Bound of |engine output - float64 output of the SAME 16-bit NCHW features|: the level bounds under the mean (or under the bilinear
    band: two 2-tap fp32 passes, 4 roundings), and the sum of the five levels (4 additions)."""
    total_b, total_v = 0.0, 0.0
    for l, (fa, fb) in enumerate(zip(feats_a, feats_b)):
        n, c, h, w = fa.shape
        flat = lambda f: f.flatten(2).permute(0, 2, 1)
        (s, _, _, mean), (b_s, _, _, b_mean) = level_ref(flat(fa), flat(fb), None if lins is None else lins[l])
        if spatial:
            up = lambda t: F.interpolate(t.reshape(n, 1, h, w), size=tuple(hw), mode="bilinear", align_corners=False)
            total_b = total_b + up(b_s) + 4 * EPS32 * up(s)
            total_v = total_v + up(s)
        else:
            total_b = total_b + b_mean.view(n, 1, 1, 1)
            total_v = total_v + mean.view(n, 1, 1, 1)
    return total_b + 4 * EPS32 * total_v
