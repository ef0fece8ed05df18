"""float64 torch restatement of torchvision's VGG-19 ``features`` tower and of the style-transfer loss on it
(perceptor/losses/style_transfer.py), written from the architecture:

  features  sixteen 3x3 pad-1 convolutions with bias, a ReLU after each, in groups of (2, 2, 4, 4, 4), MaxPool2d(2, 2) after each group:
            convolutions at module 0, 2 | 5, 7 | 10, 12, 14, 16 | 19, 21, 23, 25 | 28, 30, 32, 34, pools at 4, 9, 18, 27, 36
  encode    [images, features[0:4], [4:9], [9:16], [16:23], [23:30]] chained: the ReLUs at 3, 8, 15, 22, 29
  loss      0.001 * ( sum_l w_l mean|Fa_l - Fb_l| + sum_l 5e3 w_l^2 mean|G(Fa_l) - G(Fb_l)| ) over list entries 2, 3, 4, w = (5, 15, 2),
            G(F) = M M^T / (N C H W) with M = F viewed as [N C, H W]

Activations are keyed by the index of their CONVOLUTION (the ReLU is the next module).  ``emulate=torch.bfloat16 | torch.float16``
rounds every tensor where the HIP engine stores one (the staged input, each convolution's activated output; a max pool of rounded values
is exact) and the weights (through fp32, as the engine packs them); roundings pass gradients straight through.  Arithmetic is float64.

The input gradient is piecewise constant in three kinds of discrete choices, which ``masks=`` (ReLU patterns), ``routes=`` (which
element of each 2x2 window the pool selects) and ``signs=`` / ``fsigns=`` (sign(Ga - Gb) and sign(fa - fb) per level) pin to given
values: the pinned tower and loss are the smooth function whose gradient a forward with those choices has.

Also here: the seeded inputs shared by tests/test_style_transfer_cpu.py and tests/test_gpu_style_transfer.py, and the per-element
rounding bounds of the kernels of csrc/vgg.hip.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

DEPTHS = (2, 2, 4, 4, 4)
SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))
LEVELS = ((7, 5.0), (14, 15.0), (21, 2.0))               # (convolution index of relu2_2 / relu3_3 / relu4_2, w_l)
EPS32 = 2.0 ** -24
UNIT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}


def layer_table(widths):
    out, cin = [], 3
    for depth, w in zip(DEPTHS, widths):
        for _ in range(depth):
            out += [("conv", cin, w), ("relu",)]
            cin = w
        out.append(("pool",))
    return out


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dt):
        return x.to(dt).double()

    @staticmethod
    def backward(ctx, g):
        return g, None


def _rnd(x, dt):
    return _Round.apply(x, dt) if dt is not None else x


def first_max_route(x):
    """x NCHW -> 0/1 tensor of x's shape: 1 at the first maximum of each 2x2 window in the order (0,0), (0,1), (1,0), (1,1)."""
    n, c, h, w = x.shape
    win = x.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    mx = win.max(dim=-1, keepdim=True).values
    first = (win == mx).to(torch.int8).argmax(dim=-1)              # argmax of a 0/1 tensor: the first 1
    return _scatter_route(first, (n, c, h, w), x.dtype)


def last_max_route(x):
    """The seeded defect: the LAST maximum of each window."""
    n, c, h, w = x.shape
    win = x.reshape(n, c, h // 2, 2, w // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h // 2, w // 2, 4)
    mx = win.max(dim=-1, keepdim=True).values
    last = 3 - (win == mx).to(torch.int8).flip(-1).argmax(dim=-1)
    return _scatter_route(last, (n, c, h, w), x.dtype)


def _scatter_route(idx, shape, dtype):
    n, c, h, w = shape
    one = F.one_hot(idx, 4).to(dtype)                               # [n, c, h/2, w/2, 4]
    return one.reshape(n, c, h // 2, w // 2, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(n, c, h, w)


def pool_adjoint(dy, x, route_fn=first_max_route, mask=True):
    """The adjoint of MaxPool2d(2, 2) at x applied to dy, times (x > 0) when ``mask``: what pmi_maxpool2_bwd computes."""
    up = dy.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
    out = torch.where(route_fn(x) > 0, up, torch.zeros_like(up))
    return torch.where(x > 0, out, torch.zeros_like(out)) if mask else out


def tower(sd, widths, x, last=22, emulate=None, masks=None, routes=None):
    """x NCHW float64 (even maps at every pool) -> {conv index: post-ReLU activation}, through module ``last``.
    masks: {conv index: 0/1 NCHW}; routes: {pool index: 0/1 NCHW at the pool's input}."""
    dt = emulate
    x = _rnd(x.double(), dt)
    acts = {}
    for i, l in enumerate(layer_table(widths)[:last + 1]):
        if l[0] == "conv":
            w, b = sd[f"{i}.weight"], sd[f"{i}.bias"]
            w = w.float().to(dt).double() if dt is not None else w.double()
            pre = F.conv2d(x, w, b.float().double(), padding=1)
            x = _rnd(F.relu(pre) if masks is None else pre * masks[i].double(), dt)
            acts[i] = x
        elif l[0] == "pool":
            x = F.max_pool2d(x, 2, 2) if routes is None else F.avg_pool2d(x * routes[i].double(), 2) * 4
    return acts


def encode(sd, widths, images, emulate=None):
    """The reference's six-entry list for images already at the tower's size."""
    acts = tower(sd, widths, images, last=SLICES[-1][1] - 1, emulate=emulate)
    return [_rnd(images.double(), emulate)] + [acts[end - 2] for _, end in SLICES]


def gram(f, per_sample=False, drop_cross=False):
    """f NCHW -> [N C, N C].  per_sample / drop_cross: seeded defects (normalised by C H W only; cross-sample blocks zeroed)."""
    n, c, h, w = f.shape
    m = f.reshape(n * c, h * w)
    g = m @ m.t() / (c * h * w if per_sample else n * c * h * w)
    if drop_cross:
        blk = torch.block_diag(*[torch.ones(c, c, dtype=g.dtype) for _ in range(n)])
        g = g * blk
    return g


def loss(fa, fb, signs=None, fsigns=None, scale=0.001, gram_pow=2, **gram_kw):
    """fa / fb: the three level features [relu2_2, relu3_3, relu4_2] NCHW float64.  signs / fsigns pin sign(Ga - Gb) / sign(fa - fb).
    scale / gram_pow / gram_kw: seeded defects."""
    total = 0.0
    for l, (_, w) in enumerate(LEVELS):
        d = fa[l] - fb[l]
        total = total + w * ((d * fsigns[l].double()).mean() if fsigns is not None else d.abs().mean())
        dg = gram(fa[l], **gram_kw) - gram(fb[l], **gram_kw)
        total = total + 5e3 * w ** gram_pow * ((dg * signs[l].double()).mean() if signs is not None else dg.abs().mean())
    return total * scale


def level_features(acts, convs=None):
    return [acts[c] for c in (convs or [c for c, _ in LEVELS])]


def _nhwc_flat(f):
    return f.flatten(2).permute(0, 2, 1)                          # NCHW -> [N, HW, C]


def loss_kernel_bound(fa, fb):
    """Bound of |loss(engine) - float64 loss of the SAME 16-bit features|: the per-element Gram bounds of both sides under the mean, the
    fp32 subtraction Ga - Gb, the two-stage sums of pmi_style_level, and the six-term combination (a handful of fp32 roundings)."""
    total, terms = 0.0, 0.0
    for l, (_, w) in enumerate(LEVELS):
        n, c, h, wd = fa[l].shape
        r, hw = n * c, h * wd
        d = fa[l].double() - fb[l].double()
        dg = gram(fa[l].double()) - gram(fb[l].double())
        scale = 1.0 / (float(r) * hw)
        g_err = float((gram_bound(_nhwc_flat(fa[l]), scale) + gram_bound(_nhwc_flat(fb[l]), scale)).mean())
        total += w * l1_bound(d, d.numel() // 8, 8)
        total += 5e3 * w * w * (g_err + EPS32 * float(dg.abs().mean()) + l1_bound(dg, dg.numel() // 4, 4))
        terms += w * float(d.abs().mean()) + 5e3 * w * w * float(dg.abs().mean())
    return 0.001 * (total + 16 * EPS32 * terms)


def loss_feature_bound(ea, eb, u):
    """How far feature errors at the gates eps_l = sqrt(FEATURE_ROUNDINGS[l]) u can move the loss, as a quadrature model: every feature
    element carries an independent relative error of rms eps_l, propagated to first order.  d mean|fa - fb| = mean(sign (da - db)) has
    standard deviation eps sqrt(|fa|^2 + |fb|^2) / count.  With S = sign(Ga - Gb) (symmetric) and V = S M, d mean|Ga - Gb| =
    2 sum_ip dM_ip V_ip / (R^2 count) per side, standard deviation 2 eps |M o V| / (R^2 count).  The bound is four standard deviations
    of the sum (the terms in quadrature)."""
    var = 0.0
    for l, ((_, w), depth) in enumerate(zip(LEVELS, FEATURE_ROUNDINGS)):
        eps = depth ** 0.5 * u
        a, b = ea[l].double(), eb[l].double()
        n, c, h, wd = a.shape
        r, count = n * c, a.numel()
        S = torch.sign(gram(a) - gram(b))
        var += (w * eps / count) ** 2 * float(a.square().sum() + b.square().sum())
        for f in (a, b):
            m = f.reshape(r, h * wd)
            var += (5e3 * w * w * 2 * eps / (float(r) ** 2 * count)) ** 2 * float((m * (S @ m)).square().sum())
    return 0.001 * 4 * var ** 0.5


def resize64(x, size):
    """perceptor_amd.transforms.resize in float64 on the CPU, from its own host-side band tables (differentiable)."""
    from perceptor_amd.transforms.resize import _plan, band_tables
    method, dims = _plan(x.shape[2], x.shape[3], tuple(size))
    for _, axis, i, o in dims:
        idx, w, _, _ = band_tables(i, o, method)
        g = x.index_select(axis, idx.clamp(min=0).long().flatten()).unflatten(axis, tuple(idx.shape))
        wt = torch.where(idx >= 0, w.double(), torch.zeros_like(w, dtype=torch.float64))
        shape = [1] * g.dim()
        shape[axis], shape[axis + 1] = idx.shape
        x = (g * wt.view(shape)).sum(dim=axis + 1)
    return x


def loss_and_grads(sd, widths, size, a, b, emulate=None):
    """(loss, dloss/da, dloss/db, the six encodings of a, the three Grams of a) in float64 with autograd, resizing like ``encode``."""
    a = a.detach().double().clone().requires_grad_(True)
    b = b.detach().double().clone().requires_grad_(True)
    with torch.enable_grad():
        ra = a if tuple(a.shape[2:]) == (size, size) else resize64(a, (size, size))
        rb = b if tuple(b.shape[2:]) == (size, size) else resize64(b, (size, size))
        ea, eb = encode(sd, widths, ra, emulate), encode(sd, widths, rb, emulate)
        val = loss(ea[2:5], eb[2:5])
        ga, gb = torch.autograd.grad(val, [a, b])
    return val.detach(), ga, gb, [e.detach() for e in ea], [gram(e.detach()) for e in ea[2:5]]


# ---- seeded inputs shared by the CPU and the GPU tests ----------------------------------------------------------------------------------
POOL_SHAPES = ((1, 2, 2, 16), (2, 6, 10, 24), (1, 34, 18, 64), (2, 16, 16, 136))          # (N, H, W, C)
GRAM_SHAPES = ((1, 16, 16), (2, 64, 48), (3, 1032, 64), (2, 4096, 128), (4, 1024, 128))   # (N, HW, C)
ENGINE_CONFIGS = {"tiny": ((16, 16, 32, 32, 32), 32, 2), "mid": ((32, 64, 64, 128, 128), 64, 2)}   # widths, size, N
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16}


def _gen(seed):
    return np.random.Generator(np.random.Philox(key=seed))


def pool_inputs(shape, dt, seed=0):
    """(x, dy) NHWC 16-bit: x from a handful of values (zero among them: all-zero windows and non-zero ties both occur)."""
    n, h, w, c = shape
    g = _gen(1000 + seed + 7 * n + 11 * h + 13 * w + 17 * c)
    vals = np.array([0.0, 0.0, 0.5, 1.0, 1.0, 2.5], dtype=np.float32)
    x = torch.from_numpy(vals[g.integers(0, len(vals), size=shape)])
    x[0, :2, :2, 0] = 0.0                                          # the smallest case has 16 windows: place the three patterns
    x[0, :2, :2, 1] = torch.tensor([[0.5, 1.0], [1.0, 0.5]])       # a tie between (0,1) and (1,0)
    x[0, :2, :2, 2] = 2.5                                          # a four-way tie
    x = x.to(dt)
    dy =torch.from_numpy(g.standard_normal((n, h // 2, w // 2, c), dtype=np.float32)).to(dt)
    return x, dy


def gram_inputs(shape, dt, seed=0):
    """(fa, fb) [N, HW, C] 16-bit: independent relu(randn + 0.3), the features of the sign-band condition."""
    n, hw, c = shape
    g = _gen(2000 + seed + 7 * n + 11 * hw + 13 * c)
    mk = lambda: torch.from_numpy(np.maximum(g.standard_normal(shape, dtype=np.float32) + 0.3, 0)).to(dt)
    return mk(), mk()


def engine_inputs(name):
    widths, size, n = ENGINE_CONFIGS[name]
    g = _gen(3000 + size)
    mk = lambda: torch.from_numpy(g.random((n, 3, size, size), dtype=np.float32))
    return mk(), mk()


def nchw(f_nhwc_flat, n, hw, c):
    """[N, HW, C] -> [N, C, HW, 1] float64 (a one-column map: the Gram and the loss only see H W as one axis)."""
    return f_nhwc_flat.double().permute(0, 2, 1).reshape(n, c, hw, 1)


# ---- per-element rounding bounds of csrc/vgg.hip ----------------------------------------------------------------------------------------
# fp32 accumulation of K products in any order: |error| <= (K + 4) 2^-24 sum|terms| (K - 1 additions + the product roundings + the
# scale, first order, with headroom of a few roundings for the split-K adds); storing in 16 bits adds u |result|, and for f16 half of
# the subnormal spacing 2^-24.
def gram_bound(f, scale):
    """f [N, HW, C] -> per-element bound [N C, N C] of pmi_gram."""
    n, hw, c = f.shape
    m = f.double().permute(0, 2, 1).reshape(n * c, hw).abs()
    return (hw + 4) * EPS32 * scale * (m @ m.t())


def sum_chain(units, per_unit):
    """Longest chain of fp32 additions in the two-stage sums of csrc/vgg.hip: a thread's grid-stride units, the wave and workgroup
    trees (6 + 3), then the final kernel's trees over at most 1024 slots (6 + 16)."""
    nblk = min(1024, max(1, -(-units // 256)))
    return -(-units // (256 * nblk)) * per_unit + 6 + 3 + 6 + 16


def l1_bound(d, units, per_unit):
    """Bound of a mean|d| computed by those sums from exact fp32 differences."""
    return (sum_chain(units, per_unit) + 4) * EPS32 * float(d.double().abs().mean())


def gram_bwd_ref(fa, fb, S, g_in, c_feat, c_gram, gscale, dt, transpose=True):
    """(dF float64 before the 16-bit store, per-element bound) of pmi_gram_bwd; fa, fb, g_in [N, HW, C], S [N C, N C].
    transpose=False: the seeded defect that uses S without S^T."""
    n, hw, c = fa.shape
    a, b = fa.double(), fb.double()
    T = S.double() + S.double().t() if transpose else S.double()
    m = a.permute(0, 2, 1).reshape(n * c, hw)                              # [(m, d), p]
    acc = (T @ m).reshape(n, c, hw).permute(0, 2, 1)                        # [n, p, c]
    acc_abs = (T.abs() @ m.abs()).reshape(n, c, hw).permute(0, 2, 1)
    t_feat = gscale * c_feat * torch.sign(a - b)
    t_gram = gscale * c_gram * acc
    t_in = g_in.double() if g_in is not None else torch.zeros_like(a)
    v = (t_feat + t_gram + t_in) * (a > 0)
    k = n * c
    fp32 = EPS32 * ((k + 4) * gscale * abs(c_gram) * acc_abs + 4 * (t_feat.abs() + t_gram.abs() + t_in.abs()))
    bound = fp32 + UNIT[dt] * v.abs() + (EPS32 if dt == torch.float16 else 0.0)
    return v, bound


def level_coefs(n, hw, c, w):
    count = float(n * c) * hw
    return 0.001 * w / count, 0.001 * 5e3 * w * w / (float(n * c) ** 2 * count)


# the longest backward path of VggEngine.loss_and_grad stores a newly computed 16-bit value 12 times: pmi_gram_bwd at relu4_2, the dX
# convolutions of conv4_2, conv4_1, conv3_4, pmi_gram_bwd at relu3_3, dX of conv3_3, conv3_2, conv3_1, pmi_gram_bwd at relu2_2, dX of
# conv2_2, conv2_1, conv1_2 (masks and pool routes multiply by 0 / 1: exact; conv1_1's dX is stored in fp32)
GRAD_ROUNDINGS = 12
# convolutions (16-bit stores of the forward) up to relu2_2 / relu3_3 / relu4_2, plus the staged input
FEATURE_ROUNDINGS = (5, 8, 11)
