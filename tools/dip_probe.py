"""Times models.DeepImagePrior forward + backward (N = 1, 64 latent channels, 2 scales, bf16) at 256 x 256 and 512 x 512 on one GPU, and the
same network as stock torch modules under bf16 autocast on the same GPU (PyTorch-ROCm / MIOpen, forward + backward) as a yardstick.

Method (measuring-on-mi355x): device events around whole steps, a warm-up, `--rounds` alternating rounds of `--inner` steps per contender,
the latents rotating over `--buffers` distinct tensors so no step re-reads a cache-resident input; medians with their ranges.  The weight
gradient's achieved rate is set against its FLOP count 2 Cout taps Cin N H W per layer from a second pass that times pmi_dip_wgrad alone on
the largest layer's shapes; the BatchNorm statistics and the resamplers are set against the bytes they must move.  One JSON line per size.

    python tools/dip_probe.py [--sizes 256 512] [--rounds 5] [--inner 10] [--out profiles/dip_probe.txt]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from perceptor_amd import _hip, models                               # noqa: E402
from perceptor_amd._hip import call, ptr                             # noqa: E402
from perceptor_amd.engine import dip as E                            # noqa: E402

DEV = "cuda:0"


class _Down(nn.Module):
    def forward(self, x):
        c = x.shape[1]
        k = E.cubic_kernels()[0].to(x)[None, None].expand(c, 1, 8, 8)
        return nn.functional.conv2d(nn.functional.pad(x, (3,) * 4, "reflect"), k, stride=2, groups=c)


class _Up(nn.Module):
    def forward(self, x):
        c = x.shape[1]
        k = E.cubic_kernels()[1].to(x)[None, None].expand(c, 1, 8, 8)
        return nn.functional.conv_transpose2d(nn.functional.pad(x, (2,) * 4, "reflect"), k, stride=2, padding=7, groups=c)


class _Scale(nn.Module):
    """the network of engine/dip.py in stock torch modules (depthwise resamplers: the cheapest stock form)"""

    def __init__(self, i, n_scales, cin):
        super().__init__()
        w, s = E.WIDTH, E.SKIP
        act = lambda: nn.LeakyReLU(0.2)
        conv3 = lambda a, b: nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(a, b, 3))
        self.skip = nn.Sequential(nn.Conv2d(cin, s, 1), nn.BatchNorm2d(s), act())
        deeper = [conv3(cin, w), _Down(), nn.BatchNorm2d(w), act(), conv3(w, w), nn.BatchNorm2d(w), act()]
        if i < n_scales - 1:
            deeper.append(_Scale(i + 1, n_scales, w))
        self.deeper = nn.Sequential(*deeper, _Up())
        self.tail = nn.Sequential(nn.BatchNorm2d(s + w), conv3(s + w, w), nn.BatchNorm2d(w), act(), nn.Conv2d(w, w, 1), nn.BatchNorm2d(w), act())

    def forward(self, x):
        return self.tail(torch.cat([self.skip(x), self.deeper(x)], 1))


class _Torch(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.body, self.head = _Scale(0, 2, cin), nn.Conv2d(E.WIDTH, 3, 1)
        self.register_buffer("cm", E.colcorr_t())

    def forward(self, x):
        return torch.sigmoid(torch.einsum("nchw,cd->ndhw", self.head(self.body(x)), self.cm))


def _time(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(inner):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def _summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}


def probe(size, rounds, inner, buffers):
    torch.manual_seed(0)
    m = models.DeepImagePrior(shape=(64, size, size)).to(DEV)
    t = _Torch(64).to(DEV)
    lats = [m.random_latents() for _ in range(buffers)]
    cot = torch.randn(1, 3, size, size, device=DEV)

    def step_hip(i):
        for p in m.parameters():
            p.grad = None
        (m(lats[i % buffers]) * cot).sum().backward()

    def step_torch(i):
        for p in t.parameters():
            p.grad = None
        with torch.autocast("cuda", dtype=torch.bfloat16):
            out = t(lats[i % buffers])
        (out.float() * cot).sum().backward()

    def fwd_hip(i):
        with torch.no_grad():
            m(lats[i % buffers])

    for f in (step_hip, step_torch, fwd_hip):
        _time(f, 3)
    res = {"hip_step": [], "torch_bf16_autocast_step": [], "hip_forward": []}
    for _ in range(rounds):
        res["hip_step"].append(_time(step_hip, inner))
        res["torch_bf16_autocast_step"].append(_time(step_torch, inner))
        res["hip_forward"].append(_time(fwd_hip, inner))
    out = {"size": size, "N": 1, "latent_channels": 64, "rounds": rounds, "inner": inner, **{k: _summary(v) for k, v in res.items()}}
    # the largest weight gradient alone: 196 -> 192, 3x3 at full resolution
    eng, n, h, w = m.engine, 1, size, size
    dy = torch.randn((n, h + 2, w + 2, 192), device=DEV).to(torch.bfloat16)
    xs = [torch.randn((n, h + 2, w + 2, 200), device=DEV).to(torch.bfloat16) for _ in range(buffers)]
    wg = [_time(lambda i: eng._wgrad({}, "w", dy, 1, xs[i % buffers], 1, (n, h, w), 192, 196, 9, 1.0), inner) for _ in range(rounds + 1)][1:]
    flop = 2.0 * 192 * 9 * 196 * n * h * w
    out["wgrad_196_192_3x3"] = {**_summary(wg), "tflops_at_median": round(flop / statistics.median(wg) / 1e9, 2)}
    # BatchNorm statistics (reads x twice) and the up-sampler (reads 1/4, writes 1) against their bytes
    x = [torch.randn((n, h, w, 192), device=DEV).to(torch.bfloat16) for _ in range(buffers)]
    P = {"b.weight": torch.ones(192, device=DEV), "b.bias": torch.zeros(192, device=DEV), "b.running_mean": torch.zeros(192, device=DEV),
         "b.running_var": torch.ones(192, device=DEV), "b.num_batches_tracked": torch.tensor(0, device=DEV)}
    bn = [_time(lambda i: eng._bn(x[i % buffers], 0, (n, h, w), P, "b", 0, 192, 1, True, None), inner) for _ in range(rounds + 1)][1:]
    nbytes = 4.0 * x[0].numel() * 2                                   # statistics read x twice, apply reads and writes it once
    out["bn_stats_apply_192"] = {**_summary(bn), "gbytes_per_s_at_median": round(nbytes / statistics.median(bn) / 1e6, 1)}
    half = [torch.randn((n, h // 2, w // 2, 192), device=DEV).to(torch.bfloat16) for _ in range(buffers)]
    y = torch.empty((n, h, w, 192), dtype=torch.bfloat16, device=DEV)
    up = [_time(lambda i: call("pmi_fir8_up2", ptr(half[i % buffers]), ptr(y), n, h // 2, w // 2, 192, _hip.DT_BF16), inner) for _ in range(rounds + 1)][1:]
    out["fir8_up2_192"] = {**_summary(up), "gbytes_per_s_at_median": round(1.25 * y.numel() * 2 / statistics.median(up) / 1e6, 1)}
    out["peak_memory_mib"] = round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--buffers", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = [json.dumps(probe(s, a.rounds, a.inner, a.buffers)) for s in a.sizes]
    print("\n".join(lines))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
