"""HIP engine for the LPIPS perceptual distance (perceptor/losses/lpips.py -> the lpips package 0.1.x, version '0.1', net='vgg') and its
gradient to both images.

  input   images in [0, 1]: x = 2 img - 1, then ScalingLayer (x - shift_c) / scale_c with shift = (-.030, -.088, -.188) and
          scale = (.458, .448, .450) = (img_c - mean_c) / std_c with mean = (1 + shift) / 2, std = scale / 2: pmi_rn_stage_input.  The
          shift is NOT folded into conv1_1's bias (zero padding lives in the normalised space).
  tower   torchvision VGG-16 ``features`` through module 29: thirteen 3x3 pad-1 convolutions + bias + ReLU in groups of (2, 2, 3, 3, 3),
          convolutions at 0, 2 | 5, 7 | 10, 12, 14 | 17, 19, 21 | 24, 26, 28, MaxPool2d(2, 2) at 4, 9, 16, 23.  Five taps, the outputs of
          the slices [0:4] [4:9] [9:16] [16:23] [23:30]: relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 (the convolutions 2, 7, 14, 21, 28).
  level   u = f / (sqrt(sum_c f^2) + 1e-10) per pixel on both sides, s_l[n, p] = sum_c w_lc (ua_c - ub_c)^2 (w = 1 without linear layers)
  output  spatial=False: sum_l mean_p s_l, [N, 1, 1, 1];  spatial=True: sum_l bilinear(s_l -> (H, W), align_corners=False), [N, 1, H, W]

The tower is engine/vgg.py's VggEngine with VGG-16's depths (one ops.igemm launch per convolution + bias + ReLU, pmi_maxpool2,
pmi_maxpool2_bwd, pmi_act_bwd); the level and its adjoint are csrc/lpips.hip.  Every tap but relu5_3 is followed directly by a pool, so
the pool adjoint (already masked by the tap's ReLU) arrives as the level kernel's ``g_in`` and the level kernel's output is the gradient
at the tap's convolution output.  Images run at their own size (H % 16 == 0 and W % 16 == 0: even maps at the four pools).  A live
``images_b`` runs with ``a`` as ONE 2N batch (``pair``; measured 0.62 ms against 2 x 0.46 ms at batch 4, 256 x 256: DESIGN.md section 29),
and when both gradients are wanted the backward walks that 2N batch too; cached ``targets`` run a's tower alone, which is another
batch route: the same features up to the convolutions' rounding, not necessarily the same bits.  f16 (default) scales the gradient by
65536 and undoes it at the image.

At a pixel whose features are all zero autograd yields NaN (0 * inf through sqrt); this engine's gradient is 0 there.
"""
from __future__ import annotations

from functools import lru_cache
from typing import Optional, Sequence

import torch

from .. import _hip
from .._hip import ACT_RELU, call, ptr
from ..transforms.resize import _apply as _band_apply, bilinear_tables
from . import ops
from .vgg import VggEngine, layer_table

VGG16_DEPTHS = (2, 2, 3, 3, 3)
VGG16_WIDTHS = (64, 128, 256, 512, 512)
SLICES = ((0, 4), (4, 9), (9, 16), (16, 23), (23, 30))          # lpips' vgg16 slices over torchvision's ``features``
TAP_NAMES = ("relu1_2", "relu2_2", "relu3_3", "relu4_3", "relu5_3")
TAPS = tuple(end - 2 for _, end in SLICES)                      # the convolution whose ReLU closes each slice: 2, 7, 14, 21, 28
LAST = SLICES[-1][1] - 1                                        # module 29
SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
PARTIAL_SLOTS = 512                                             # pmi_lpips_level's workspace: 512 floats per sample


def lpips_layer_table(widths=VGG16_WIDTHS):
    """Modules 0 .. 29 of VGG-16's ``features`` (engine/vgg.py's layer_table with VGG-16's depths, without the last pool)."""
    return layer_table(widths, VGG16_DEPTHS)[:LAST + 1]


def tap_names():
    """{convolution index: name of the ReLU it feeds} for the five taps."""
    return dict(zip(TAPS, TAP_NAMES))


@lru_cache(maxsize=64)
def bilinear_tables_t(in_sz: int, out_sz: int):
    """The transpose of transforms.resize.bilinear_tables(in_sz, out_sz) as a band over the OUTPUT rows: (idx [in, taps] int32 (-1: unused),
    w [in, taps] f32) on the CPU.  Taps of one output row that hit the same input row (the clamped last row) stay separate entries."""
    idx, w = bilinear_tables(in_sz, out_sz)
    rows = [[] for _ in range(in_sz)]
    for j in range(out_sz):
        for t in range(2):
            rows[int(idx[j, t])].append((j, float(w[j, t])))
    taps = max(len(r) for r in rows)
    idx_t = torch.full((in_sz, taps), -1, dtype=torch.int32)
    w_t = torch.zeros((in_sz, taps), dtype=torch.float32)
    for r, lst in enumerate(rows):
        for k, (j, wv) in enumerate(lst):
            idx_t[r, k], w_t[r, k] = j, wv
    return idx_t.contiguous(), w_t.contiguous()


class LpipsEngine(VggEngine):
    """VggEngine's tower pieces (the packed convolutions, _pool, _pool_bwd, _check) with VGG-16's depths and LPIPS' own staging, levels and
    walk; VggEngine's style-transfer entry points (encode, features, loss_value, backward_from) have no meaning here and are not used."""

    def __init__(self, widths, state_dict, lins: Optional[Sequence[torch.Tensor]], device, dtype="f16", shift=SHIFT, scale=SCALE):
        """state_dict: torchvision vgg16 ``features`` keys ("{i}.weight" / "{i}.bias", i = 0 .. 28); lins: five non-negative weight vectors
        [C_l] (any shape with C_l elements), or None for ``linear_layers=False`` (w = 1)."""
        super().__init__((widths, None), state_dict, device, dtype, depths=VGG16_DEPTHS)
        self.layers = self.layers[:LAST + 1]
        shift = torch.as_tensor(shift, dtype=torch.float64).flatten()
        scale = torch.as_tensor(scale, dtype=torch.float64).flatten()
        self.mean = ((1.0 + shift) / 2).float().to(self.device)
        self.std = (scale / 2).float().to(self.device)
        if lins is None:
            self.lins = [None] * 5
        else:
            if len(lins) != 5 or any(l.numel() != c for l, c in zip(lins, self.widths)):
                raise ValueError(f"LPIPS: five lin weights with {self.widths} elements are required")
            self.lins = [l.detach().float().flatten().contiguous().to(self.device) for l in lins]
        self._tables = {}

    # ---- tower ----------------------------------------------------------------------------------------
    def _tower(self, images):
        """images NCHW in [0, 1] -> {conv index: post-ReLU activation NHWC 16-bit} through module 29."""
        self._check(images)
        n, _, h, w = images.shape
        if h % 16 or w % 16 or h <= 0 or w <= 0:
            raise ValueError(f"LPIPS on this engine needs height and width divisible by 16 (an even map at each of the four pools), got {h} x {w}")
        img = images.float().contiguous()
        x = torch.empty((n, h, w, 8), dtype=_hip.TORCH_DTYPE[self.dt], device=img.device)
        call("pmi_rn_stage_input", ptr(img), ptr(self.mean), ptr(self.std), ptr(x), n, h, w, self.dt)
        acts = {}
        for i, l in enumerate(self.layers):
            if l[0] == "conv":
                x = ops.igemm(x, self.convs[i].fwd, act=ACT_RELU)
                acts[i] = x
            elif l[0] == "pool":
                x = self._pool(x)
        return acts

    @torch.no_grad()
    def targets(self, images_b, keep_tape=False):
        """One tower pass: the five 16-bit tap features of ``images_b`` (and its tape when the gradient to it is wanted)."""
        acts = self._tower(images_b)
        t = dict(n=int(images_b.shape[0]), hw=tuple(images_b.shape[2:]), feats=[acts[c] for c in TAPS])
        if keep_tape:
            t["acts"] = acts
        return t

    # ---- levels ---------------------------------------------------------------------------------------
    def _levels(self, ta, tb, means):
        """Per level (s [N, h, w], na, nb fp32, mean [N] or None)."""
        if ta["n"] != tb["n"] or ta["hw"] != tb["hw"]:
            raise ValueError(f"LPIPS needs images of equal shape, got {(ta['n'], 3) + ta['hw']} and {(tb['n'], 3) + tb['hw']}")
        out = []
        for fa, fb, w in zip(ta["feats"], tb["feats"], self.lins):
            n, h, wd, c = fa.shape
            s, na, nb = (torch.empty((n, h, wd), dtype=torch.float32, device=fa.device) for _ in range(3))
            mean = torch.empty(n, dtype=torch.float32, device=fa.device) if means else None
            partial = torch.empty(n * PARTIAL_SLOTS, dtype=torch.float32, device=fa.device) if means else None
            call("pmi_lpips_level", ptr(fa), ptr(fb), ptr(w), ptr(s), ptr(na), ptr(nb), ptr(mean), ptr(partial), n, h * wd, c, self.dt)
            out.append((s, na, nb, mean))
        return out

    def _band(self, in_sz, out_sz, transposed):
        key = (in_sz, out_sz, transposed)
        if key not in self._tables:
            idx, w = bilinear_tables_t(in_sz, out_sz) if transposed else bilinear_tables(in_sz, out_sz)
            self._tables[key] = (idx.to(self.device), w.to(self.device))
        return self._tables[key]

    def _upsample(self, s, hw):
        """s [N, h, w] fp32 -> F.interpolate(s, hw, mode="bilinear", align_corners=False) as [N, 1, H, W]."""
        x = s.unsqueeze(1)
        for axis, o in ((2, hw[0]), (3, hw[1])):
            if x.shape[axis] != o:
                idx, w = self._band(x.shape[axis], o, False)
                x = _band_apply(x, idx, w, axis, o)
        return x

    def _upsample_adjoint(self, g, hw_l):
        """g [N, 1, H, W] fp32 -> the transposed bilinear band applied to it, [N, h, w]."""
        x = g
        for axis, i in ((3, hw_l[1]), (2, hw_l[0])):
            if x.shape[axis] != i:
                idx, w = self._band(i, x.shape[axis], True)
                x = _band_apply(x, idx, w, axis, i)
        return x[:, 0]

    def _output(self, levels, hw, spatial):
        if spatial:
            out = None
            for s, _, _, _ in levels:
                up = self._upsample(s, hw)
                out = up if out is None else out + up
            return out.contiguous()
        out = levels[0][3]
        for lv in levels[1:]:
            out = out + lv[3]
        return out.view(-1, 1, 1, 1)

    @torch.no_grad()
    def value(self, images_a, b, spatial=False):
        """b: ``targets``' record or a live image batch (then one 2N pass)."""
        ta, tb = (self.targets(images_a), b) if isinstance(b, dict) else self.pair(images_a, b)
        return self._output(self._levels(ta, tb, not spatial), ta["hw"], spatial)

    # ---- gradient -------------------------------------------------------------------------------------
    @torch.no_grad()
    def pair(self, images_a, images_b, keep_tape_b=False):
        """A live ``images_b``: ONE tower pass over the 2N batch [a; b] (measured faster than two N passes).  Returns
        the records of both sides as views of the joint tape; "joint" is that tape (the backward then walks both sides as one 2N batch)."""
        self._check(images_b)
        if tuple(images_a.shape) != tuple(images_b.shape):
            raise ValueError(f"LPIPS needs images of equal shape, got {tuple(images_a.shape)} and {tuple(images_b.shape)}")
        n = int(images_a.shape[0])
        acts = self._tower(torch.cat([images_a.float(), images_b.float()]))
        ta = dict(n=n, hw=tuple(images_a.shape[2:]), feats=[acts[c][:n] for c in TAPS], acts={i: t[:n] for i, t in acts.items()})
        tb = dict(n=n, hw=ta["hw"], feats=[acts[c][n:] for c in TAPS])
        if keep_tape_b:
            tb["acts"] = {i: t[n:] for i, t in acts.items()}
            ta["joint"] = tb["joint"] = acts
        return ta, tb

    def _walk(self, ta, tb, levels, rs, grad_a, grad_b):
        """Backward from module 29; levels: _levels' records; rs: per level dL/ds [N, h, w] fp32.  Returns the fp32 [N, H, W, 4] gradients at the
        tower's input (a's, b's; None where not asked for).  Each side is a stream of its own over its N-sample tape, or -- both sides asked
        for and taped by one ``pair`` pass -- both are the halves of ONE 2N stream over the joint tape."""
        n = ta["n"]
        joint = grad_a and grad_b and ta.get("joint") is not None and ta.get("joint") is tb.get("joint")
        tapes = [ta["joint"]] if joint else [ta["acts"] if grad_a else None, tb["acts"] if grad_b else None]
        live = [k for k, t in enumerate(tapes) if t is not None]
        g = [None] * len(tapes)
        masked = False                                # g already carries the ReLU mask of the activation it belongs to
        for i in range(LAST, -1, -1):
            kind = self.layers[i][0]
            if kind == "pool":
                for k in live:
                    g[k] = self._pool_bwd(g[k], tapes[k][i - 2])
                masked = True
            elif kind == "conv":
                if i in TAPS:
                    l = TAPS.index(i)
                    fa, fb = ta["feats"][l], tb["feats"][l]
                    _, h, w, c = fa.shape
                    _, na, nb, _ = levels[l]
                    if joint:
                        out = torch.empty_like(tapes[0][i])
                        gin = (None, None) if g[0] is None else (g[0][:n], g[0][n:])
                        dst, g = (out[:n], out[n:]), [out]
                    else:
                        gin = (g[0], g[1])
                        dst = g = [torch.empty_like(fa) if grad_a else None, torch.empty_like(fb) if grad_b else None]
                    call("pmi_lpips_level_bwd", ptr(fa), ptr(fb), ptr(self.lins[l]), ptr(na), ptr(nb), ptr(rs[l]), ptr(gin[0]), ptr(gin[1]),
                         ptr(dst[0]), ptr(dst[1]), n, h * w, c, self.gscale, self.dt)
                elif not masked:
                    for k in live:
                        o = torch.empty_like(g[k])
                        call("pmi_act_bwd", ptr(g[k]), ptr(tapes[k][i]), ptr(o), g[k].numel(), ACT_RELU, self.dt)
                        g[k] = o
                for k in live:
                    g[k] = ops.igemm(g[k], self.convs[i].bwd, out_f32=(i == 0))
                masked = False
        return (g[0][:n], g[0][n:]) if joint else tuple(g)

    def _image_grad(self, dx):
        n, h, w, _ = dx.shape
        d = torch.empty((n, 3, h, w), dtype=torch.float32, device=dx.device)
        call("pmi_rn_stage_input_bwd", ptr(dx), dx.shape[-1], ptr(self.std), ptr(d), n, h, w, 1.0 / self.gscale)
        return d

    @torch.no_grad()
    def forward_levels(self, images_a, b, spatial=False, keep_tape_b=False):
        """(output, state): the value and what ``backward`` needs (the tapes, the level records).  b: what ``targets`` returned (a's tower
        runs alone) or a live image batch (one 2N pass, ``pair``; keep_tape_b: the gradient to it is wanted)."""
        if isinstance(b, dict):
            ta, tb = self.targets(images_a, keep_tape=True), b
        else:
            ta, tb = self.pair(images_a, b, keep_tape_b)
        levels = self._levels(ta, tb, not spatial)
        return self._output(levels, ta["hw"], spatial), dict(ta=ta, tb=tb, levels=levels, spatial=spatial)

    @torch.no_grad()
    def backward(self, state, grad_out=None, grad_a=True, grad_b=False):
        """(dL/dimages_a or None, dL/dimages_b or None) for L = sum(grad_out * output); grad_out has the output's shape (default: ones)."""
        ta, tb, levels, spatial = state["ta"], state["tb"], state["levels"], state["spatial"]
        n, hw = ta["n"], ta["hw"]
        if grad_b and "acts" not in tb:
            raise RuntimeError("the gradient to images_b needs targets(images_b, keep_tape=True)")
        shape = (n, 1) + (hw if spatial else (1, 1))
        if grad_out is None:
            grad_out = torch.ones(shape, dtype=torch.float32, device=self.device)
        if not grad_out.is_cuda:
            raise RuntimeError("LpipsEngine runs on a HIP device only (no CPU fallback)")
        if tuple(grad_out.shape) != shape:
            raise ValueError(f"LPIPS: grad_out has shape {tuple(grad_out.shape)}, the output has {shape}")
        grad_out = grad_out.float().contiguous()
        rs = []
        for s, _, _, _ in levels:
            _, h, w = s.shape
            if spatial:
                rs.append(self._upsample_adjoint(grad_out, (h, w)).contiguous())
            else:
                rs.append((grad_out.view(n, 1, 1) / float(h * w)).expand(n, h, w).contiguous())
        g = self._walk(ta, tb, levels, rs, grad_a, grad_b)
        return tuple(self._image_grad(x) if x is not None else None for x in g)

    @torch.no_grad()
    def loss_and_grad(self, images_a, b, grad_out=None, grad_b=False, spatial=False, record=None):
        """(output, dL/dimages_a[, dL/dimages_b when grad_b]) with L = sum(grad_out * output).  b: ``targets``' record (with its tape when
        grad_b) or a live image batch.  record: a dict that receives the tapes ("acts", "acts_b"), the tap features of both sides and the
        level records: the discrete choices a test pins its float64 tower to."""
        out, state = self.forward_levels(images_a, b, spatial, keep_tape_b=grad_b)
        if record is not None:
            record.update(acts=state["ta"]["acts"], acts_b=state["tb"].get("acts"), feats_a=state["ta"]["feats"], feats_b=state["tb"]["feats"],
                          levels=state["levels"])
        ga, gb = self.backward(state, grad_out, True, grad_b)
        return (out, ga, gb) if grad_b else (out, ga)
