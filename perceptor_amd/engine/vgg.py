"""HIP engine for torchvision's VGG-19 ``features`` tower and the style-transfer loss on it: forward, the loss of
perceptor/losses/style_transfer.py and its gradient w.r.t. the input image.

``features`` has 37 modules: sixteen 3x3 pad-1 convolutions with bias, each followed by a ReLU, in groups of (2, 2, 4, 4, 4) with a
MaxPool2d(2, 2) after every group:
  convolutions at 0, 2 | 5, 7 | 10, 12, 14, 16 | 19, 21, 23, 25 | 28, 30, 32, 34;  pools at 4, 9, 18, 27, 36.
The reference's ``encode`` returns the input and the outputs of the slices [0:4], [4:9], [9:16], [16:23], [23:30]: the ReLUs at
3, 8, 15, 22, 29 = relu1_2, relu2_2, relu3_3, relu4_2, relu5_1.  Its loss uses relu2_2, relu3_3 and relu4_2 with weights (5, 15, 2):
  0.001 * sum_l ( w_l mean|Fa - Fb| + 5e3 w_l^2 mean|G(Fa) - G(Fb)| ),  G(F) = M M^T / (N C H W) with M = F viewed as [N C, H W]:
the Gram couples the samples of a batch, so there is no ``n_total`` here and both sides need the same batch size.

Each convolution + bias + ReLU is one ops.igemm launch; its input gradient is the same launch on transposed, flipped weights.  The
pools, the Gram, the level sums and the level gradient are csrc/vgg.hip.  The tape holds every post-ReLU activation: it is the ReLU
mask of pmi_act_bwd, the route of pmi_maxpool2_bwd and the feature of pmi_gram_bwd.  relu2_2 is followed directly by a pool: its
adjoint arrives as pmi_gram_bwd's ``g_in``, so pmi_maxpool2_bwd needs no additive input.  Activations and gradients are 16-bit NHWC;
f16 (the default: the loss is a difference of features) scales the gradient by 65536 and undoes it at the image, as engine/resnet.py.
"""
from __future__ import annotations

from typing import Dict, Tuple

import torch

from .. import _hip
from .._hip import ACT_RELU, call, ptr
from ..transforms.resize import resize as _resize, resize_backward as _resize_backward
from . import ops
from .ops import PackedLinear

DEPTHS = (2, 2, 4, 4, 4)
VGG19_CONFIG = ((64, 128, 256, 512, 512), 256)
SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))          # the reference's get_vgg_activations
LEVEL_WEIGHTS = {7: 5.0, 14: 15.0, 21: 2.0}                     # convolution whose ReLU is relu2_2 / relu3_3 / relu4_2 -> w_l
LOSS_LAST = 22                                                  # the loss path stops at relu4_2
GRAM_WEIGHT, LOSS_SCALE = 5e3, 0.001


def layer_table(widths=VGG19_CONFIG[0], depths=DEPTHS):
    """The modules of ``features`` (37 for VGG-19's depths): ("conv", cin, cout) | ("relu",) | ("pool",), at torchvision's indices.
    depths: convolutions per group; (2, 2, 3, 3, 3) is VGG-16 (engine/lpips.py)."""
    out, cin = [], 3
    for depth, w in zip(depths, widths):
        for _ in range(depth):
            out += [("conv", cin, w), ("relu",)]
            cin = w
        out.append(("pool",))
    return out


def conv_indices(widths=VGG19_CONFIG[0], depths=DEPTHS):
    return [i for i, l in enumerate(layer_table(widths, depths)) if l[0] == "conv"]


def vgg_state_dict_shapes(widths=VGG19_CONFIG[0], depths=DEPTHS) -> Dict[str, Tuple[int, ...]]:
    S: Dict[str, Tuple[int, ...]] = {}
    for i, l in enumerate(layer_table(widths, depths)):
        if l[0] == "conv":
            S[f"{i}.weight"] = (l[2], l[1], 3, 3)
            S[f"{i}.bias"] = (l[2],)
    return S


def map_state_dict(sd, widths=VGG19_CONFIG[0], depths=DEPTHS):
    """torchvision's keys "{i}.weight" / "{i}.bias", with or without a "features." prefix; "classifier.*" is ignored."""
    out = {}
    for k, v in sd.items():
        if k.startswith("classifier."):
            continue
        out[k[len("features."):] if k.startswith("features.") else k] = v
    want = vgg_state_dict_shapes(widths, depths)
    name = "VGG-19" if tuple(depths) == DEPTHS else f"VGG{tuple(depths)}"
    missing = [k for k in want if k not in out]
    extra = [k for k in out if k not in want]
    if missing or extra:
        raise ValueError(f"{name} state dict: missing {missing[:4]}, unexpected {extra[:4]}")
    for k, shp in want.items():
        if tuple(out[k].shape) != shp:
            raise ValueError(f"{name} state dict: {k} has shape {tuple(out[k].shape)}, expected {shp}")
    return out


class _Conv:
    """Forward weights + bias, and the transposed, flipped weights of the input gradient."""

    def __init__(self, w, b, dt, dev):
        self.fwd = PackedLinear(w, b, dt, dev)
        self.bwd = PackedLinear(w.permute(1, 0, 2, 3).flip(2, 3).contiguous(), None, dt, dev)


class VggEngine:
    def __init__(self, cfg, state_dict, device, dtype="f16", depths=DEPTHS):
        """depths: convolutions per group (VGG-19's by default).  size None: no style-transfer size; images run at their own size only
        (engine/lpips.py)."""
        widths, size = cfg
        widths = tuple(int(w) for w in widths)
        if len(widths) != 5 or any(w <= 0 or w % 16 for w in widths) or (size is not None and (size <= 0 or size % 32)):
            raise ValueError(f"unsupported VGG config {cfg}: five widths, each a multiple of 16, and size % 32 == 0 are required "
                             "(even maps at every pool)")
        size = None if size is None else int(size)
        self.cfg, self.widths, self.size, self.device, self.depths = (widths, size), widths, size, torch.device(device), tuple(depths)
        if dtype not in ("f16", "bf16"):
            raise ValueError("the VGG tower runs in 'f16' or 'bf16'")
        self.dt = _hip.dtype_code(dtype)
        self.gscale = 1.0 if self.dt == _hip.DT_BF16 else 65536.0
        _hip.lib()
        sd = map_state_dict(state_dict, widths, self.depths)
        self.layers = layer_table(widths, self.depths)
        self.convs = {i: _Conv(sd[f"{i}.weight"].detach().float().cpu(), sd[f"{i}.bias"].detach().float().cpu(), self.dt, self.device)
                      for i in conv_indices(widths, self.depths)}
        self.saved = None

    # ---- pieces ---------------------------------------------------------------------------------------
    def _pool(self, x):
        n, h, w, c = x.shape
        y = torch.empty((n, h // 2, w // 2, c), dtype=x.dtype, device=x.device)
        call("pmi_maxpool2", ptr(x), ptr(y), n, h, w, c, self.dt)
        return y

    def _pool_bwd(self, g, x):
        n, h, w, c = x.shape
        dx = torch.empty_like(x)
        call("pmi_maxpool2_bwd", ptr(g), ptr(x), ptr(dx), n, h, w, c, self.dt)
        return dx

    def gram(self, f):
        """f [N, H, W, C] 16-bit -> G fp32 [N C, N C] = M M^T / (N C H W)."""
        n, h, w, c = f.shape
        r = n * c
        nws = _hip.lib().pmi_gram_workspace(n, h * w, c)
        if nws < 0:
            raise ValueError(f"pmi_gram does not take N={n}, HW={h * w}, C={c}")
        ws = torch.empty(nws, dtype=torch.float32, device=f.device)
        G = torch.empty((r, r), dtype=torch.float32, device=f.device)
        call("pmi_gram", ptr(f), ptr(G), ptr(ws), n, h * w, c, 1.0 / (float(r) * h * w), self.dt)
        return G

    def _check(self, images):
        if not images.is_cuda:
            raise RuntimeError("VggEngine runs on a HIP device only (no CPU fallback)")
        if images.dim() != 4 or images.shape[1] != 3:
            raise ValueError(f"VggEngine expects NCHW images with 3 channels, got {tuple(images.shape)}")

    def _tower(self, x_nchw, last):
        """x NCHW fp32 with even maps at every pool up to module ``last`` -> (output NHWC, {conv index: post-ReLU activation})."""
        n, _, h, w = x_nchw.shape
        x_nchw = x_nchw.float().contiguous()
        x = torch.empty((n, h, w, 8), dtype=_hip.TORCH_DTYPE[self.dt], device=x_nchw.device)
        call("pmi_nchw_to_nhwc", ptr(x_nchw), ptr(x), n, 3, h, w, 8, 1.0, 0.0, self.dt)
        acts = {}
        for i, l in enumerate(self.layers[:last + 1]):
            if l[0] == "conv":
                x = ops.igemm(x, self.convs[i].fwd, act=ACT_RELU)
                acts[i] = x
            elif l[0] == "pool":
                x = self._pool(x)
        return x, acts

    def _sized(self, images):
        self._check(images)
        if tuple(images.shape[2:]) != (self.size, self.size):
            return _resize(images, (self.size, self.size))
        return images.float().contiguous()

    # ---- forward --------------------------------------------------------------------------------------
    @torch.no_grad()
    def encode(self, images):
        """The reference's ``encode``: [resized images, relu1_2, relu2_2, relu3_3, relu4_2, relu5_1] as fp32 NCHW."""
        x = self._sized(images)
        _, acts = self._tower(x, SLICES[-1][1] - 1)
        return [x] + [acts[end - 2].permute(0, 3, 1, 2).float().contiguous() for _, end in SLICES]

    @torch.no_grad()
    def features(self, images, save=False):
        """All of ``features`` at the images' own size (models.VGG19): [N, C5, H/32, W/32] fp32."""
        self._check(images)
        y, acts = self._tower(images, len(self.layers) - 1)
        if save:
            self.saved = dict(acts=acts, in_hw=tuple(images.shape[2:]), resized=False)
        return y.permute(0, 3, 1, 2).float().contiguous()

    def _levels(self, acts):
        return [(acts[i], self.gram(acts[i])) for i in LEVEL_WEIGHTS]

    @torch.no_grad()
    def targets(self, images, keep_tape=False):
        """One tower pass over the style / init images: per used level the 16-bit features and the fp32 Gram."""
        x = self._sized(images)
        _, acts = self._tower(x, LOSS_LAST)
        t = dict(n=x.shape[0], levels=self._levels(acts))
        if keep_tape:
            t.update(acts=acts, in_hw=tuple(images.shape[2:]))
        return t

    @torch.no_grad()
    def targets_from_encodings(self, encodings):
        """The same from the six fp32 NCHW tensors of ``encode`` (their values are 16-bit values: the conversion back is exact)."""
        tdt = _hip.TORCH_DTYPE[self.dt]
        feats = {}
        for conv, e in zip(LEVEL_WEIGHTS, (encodings[2], encodings[3], encodings[4])):
            if not e.is_cuda:
                raise RuntimeError("VggEngine runs on a HIP device only (no CPU fallback)")
            feats[conv] = e.detach().permute(0, 2, 3, 1).to(tdt).contiguous()
        return dict(n=int(encodings[2].shape[0]), levels=self._levels(feats))

    def _level_terms(self, la, lb):
        """Per level (loss2 [2] fp32, S); la / lb: [(features, Gram)] of the two sides."""
        out = []
        for (fa, Ga), (fb, Gb) in zip(la, lb):
            if fa.shape != fb.shape:
                raise ValueError(f"style transfer: feature shapes differ, {tuple(fa.shape)} vs {tuple(fb.shape)}")
            n, h, w, c = fa.shape
            S = torch.empty((n * c, n * c), dtype=fa.dtype, device=fa.device)
            loss2 = torch.empty(2, dtype=torch.float32, device=fa.device)
            partial = torch.empty(2048, dtype=torch.float32, device=fa.device)
            call("pmi_style_level", ptr(fa), ptr(fb), ptr(Ga), ptr(Gb), ptr(S), ptr(loss2), ptr(partial), n, h * w, c, self.dt)
            out.append((loss2, S))
        return out

    def _loss(self, terms):
        coef = torch.tensor([[w, GRAM_WEIGHT * w * w] for w in LEVEL_WEIGHTS.values()], dtype=torch.float32, device=self.device)
        return (torch.stack([t[0] for t in terms]) * coef).sum() * LOSS_SCALE

    @torch.no_grad()
    def loss_value(self, ta, tb):
        """The loss from two ``targets`` records."""
        if ta["n"] != tb["n"]:
            raise ValueError(f"style transfer needs equal batch sizes (the Gram matrix mixes the batch): {ta['n']} vs {tb['n']}")
        return self._loss(self._level_terms(ta["levels"], tb["levels"]))

    # ---- gradient -------------------------------------------------------------------------------------
    def _walk(self, acts, last, g, levels=None):
        """Backward from module ``last``.  g: gradient at its output (16-bit NHWC, times gscale), or None when the level gradients are
        the only sources.  levels: {conv index: (f_self, f_other, S, c_feat, c_gram)}.  Returns fp32 [N, H, W, 4] at the tower's input."""
        levels = levels or {}
        masked = False                                # g already carries the ReLU mask of the activation it belongs to
        for i in range(last, -1, -1):
            kind = self.layers[i][0]
            if kind == "pool":
                x = acts[i - 2]                       # the convolution two modules back: its post-ReLU output is what was pooled
                g = self._pool_bwd(g, x)
                masked = True
            elif kind == "conv":
                y = acts[i]
                if i in levels:
                    f_self, f_other, S, c_feat, c_gram = levels[i]
                    n, h, w, c = f_self.shape
                    out, T = torch.empty_like(f_self), torch.empty_like(S)          # T: workspace that receives S + S^T
                    call("pmi_gram_bwd", ptr(f_self), ptr(f_other), ptr(S), ptr(T), ptr(g), ptr(out), n, h * w, c, c_feat, c_gram,
                         self.gscale, self.dt)
                    g = out
                elif g is None:
                    continue
                elif not masked:
                    out = torch.empty_like(g)
                    call("pmi_act_bwd", ptr(g), ptr(y), ptr(out), g.numel(), ACT_RELU, self.dt)
                    g = out
                g = ops.igemm(g, self.convs[i].bwd, out_f32=(i == 0))
                masked = False
        return g

    def _image_grad(self, dx, in_hw):
        d = ops.grad_to_nchw(dx, 3, 1.0 / self.gscale)
        return _resize_backward(d, in_hw) if tuple(d.shape[2:]) != tuple(in_hw) else d

    def _level_args(self, ta_levels, tb_levels, terms, negate):
        """pmi_gram_bwd arguments of every level for side a (negate=False) or side b (the roles swapped and the Gram sign negated)."""
        out = {}
        for conv, (fa, _), (fb, _), (_, S) in zip(LEVEL_WEIGHTS, ta_levels, tb_levels, terms):
            w = LEVEL_WEIGHTS[conv]
            n, h, wd, c = fa.shape
            count = float(n * c) * h * wd
            c_feat = LOSS_SCALE * w / count
            c_gram = LOSS_SCALE * GRAM_WEIGHT * w * w / (float(n * c) ** 2 * count)
            out[conv] = (fb, fa, S, c_feat, -c_gram) if negate else (fa, fb, S, c_feat, c_gram)
        return out

    @torch.no_grad()
    def loss_and_grad(self, images_a, targets, grad_b=False, record=None):
        """(loss fp32 scalar, dL/dimages_a fp32 NCHW at the input size[, dL/dimages_b when grad_b: ``targets`` must hold b's tape]).
        record: a dict that receives a's tape ("acts"), its level features and Grams ("levels") and the per-level (loss2, S) ("terms"):
        the discrete choices (ReLU masks, pool routes, signs) a test pins its float64 tower to."""
        ta = self.targets(images_a, keep_tape=True)
        if ta["n"] != targets["n"]:
            raise ValueError(f"style transfer needs equal batch sizes (the Gram matrix mixes the batch): {ta['n']} vs {targets['n']}")
        terms = self._level_terms(ta["levels"], targets["levels"])
        loss = self._loss(terms)
        if record is not None:
            record.update(acts=ta["acts"], levels=ta["levels"], terms=terms)
        dx = self._walk(ta["acts"], LOSS_LAST, None, self._level_args(ta["levels"], targets["levels"], terms, False))
        ga = self._image_grad(dx, ta["in_hw"])
        if not grad_b:
            return loss, ga
        if "acts" not in targets:
            raise RuntimeError("the gradient to images_b needs targets(images_b, keep_tape=True)")
        dxb = self._walk(targets["acts"], LOSS_LAST, None, self._level_args(ta["levels"], targets["levels"], terms, True))
        return loss, ga, self._image_grad(dxb, targets["in_hw"])

    @torch.no_grad()
    def backward_from(self, d_out):
        """d_out: dL/d(features output), fp32 NCHW [N, C5, H/32, W/32] -> dL/dimages fp32 NCHW (after features(images, save=True))."""
        sv = self.saved
        if sv is None:
            raise RuntimeError("call features(images, save=True) before backward_from()")
        if not d_out.is_cuda:
            raise RuntimeError("VggEngine runs on a HIP device only (no CPU fallback)")
        g, scale = ops.grad_to_nhwc(d_out, self.dt, self.device, cpad=d_out.shape[1])
        dx = self._walk(sv["acts"], len(self.layers) - 1, g)
        self.saved = None
        return ops.grad_to_nchw(dx, 3, 1.0 / scale)
