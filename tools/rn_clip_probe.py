#!/usr/bin/env python3
"""CLIP ResNet towers (engine/resnet.py): forward and loss_and_grad time per architecture, with device events after warm-up, and the achieved
TFLOP/s from FLOPs computed from the layer shapes (every convolution, the attention pool's projections and its attention; the input gradient
counts each convolution's dX at its own input grid -- the stride-2 stem convolution on the zero-inserted grid -- and the attention backward).

  python tools/rn_clip_probe.py [--arch RN50 RN101 ...] [--batch 8] [--iters 20] [--dtype bf16] [--aten] [--gemm-trace]

--aten: the torch (aten) GPU kernels launched inside one loss_and_grad call, with the Python line that issued them (as tools/aten_trace.py
does for a bench step): the engine's only torch compute is the zero-insert of the stem convolution's input gradient.
--gemm-trace: every pmi_igemm launch of one loss_and_grad (ops.GEMM_TRACE) grouped by shape, with the kernel that took it -- the
convolutions left on the generic implicit-GEMM kernel are the rows with halo=-1 wd=0."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def flops(cfg, n):
    """(forward, input-gradient) FLOPs of one call on n images at the tower's resolution."""
    from perceptor_amd.engine import resnet
    res, layers, width, heads, out = cfg
    fwd = bwd = 0.0
    conv = lambda hw, cin, cout, k: 2.0 * n * hw * cin * cout * k * k
    h = width // 2
    s = res // 2
    fwd += conv(s * s, 3, h, 3) + conv(s * s, h, h, 3) + conv(s * s, h, width, 3)
    bwd += conv(res * res, h, 8, 3) + conv(s * s, h, h, 3) + conv(s * s, width, h, 3)      # stem dX: conv1's on the zero-inserted full grid
    r = res // 4
    for p, inplanes, planes, stride, ds in resnet.blocks(cfg):
        ro = r // stride
        f = conv(r * r, inplanes, planes, 1) + conv(r * r, planes, planes, 3) + conv(ro * ro, planes, 4 * planes, 1)
        if ds:
            f += conv(ro * ro, inplanes, 4 * planes, 1)
        fwd += f
        bwd += f
        r = ro
    c, t = width * 32, r * r + 1
    attn = 2.0 * n * (t * c * 2 * c + c * c + c * out) + 4.0 * n * t * c
    return fwd + attn, bwd + attn + 4.0 * n * t * c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", nargs="*", default=["RN50", "RN101", "RN50x4", "RN50x16", "RN50x64"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--aten", action="store_true")
    ap.add_argument("--gemm-trace", action="store_true")
    a = ap.parse_args()
    from perceptor_amd import losses
    from perceptor_amd.engine import resnet
    from perceptor_amd.utils.synth import seeded_noise
    if not torch.cuda.is_available():
        raise SystemExit("rn_clip_probe needs a HIP device")
    dev = torch.device("cuda:0")
    for arch in a.arch:
        cfg = resnet.RN_CONFIGS[arch]
        loss = losses.OpenCLIP(arch, "synthetic", dtype=a.dtype).to(dev)
        loss.add_encodings_(torch.nn.functional.normalize(seeded_noise((2, cfg[4]), 7)).to(dev))
        img = (seeded_noise((a.batch, 3, cfg[0], cfg[0]), 1234) * 0.25 + 0.5).to(dev)
        eng = loss.model.engine
        timings = {}
        for what, fn in (("forward", lambda: eng.forward(img)), ("loss_and_grad", lambda: loss.loss_and_grad(img))):
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.iters):
                fn()
            e1.record()
            torch.cuda.synchronize()
            timings[what] = e0.elapsed_time(e1) / a.iters
        ff, fb = flops(cfg, a.batch)
        row = dict(arch=arch, batch=a.batch, dtype=a.dtype, image=cfg[0], forward_ms=round(timings["forward"], 3),
                   loss_and_grad_ms=round(timings["loss_and_grad"], 3), forward_tflop=round(ff / 1e12, 4), fwd_grad_tflop=round((ff + fb) / 1e12, 4),
                   forward_tflops=round(ff / timings["forward"] / 1e9, 1), loss_and_grad_tflops=round((ff + fb) / timings["loss_and_grad"] / 1e9, 1))
        print(json.dumps(row), flush=True)
        if a.aten:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA], with_stack=True) as prof:
                loss.loss_and_grad(img)
                torch.cuda.synchronize()
            rows = {}
            for ev in prof.events():
                if not ev.name.startswith("aten::") or ev.self_device_time_total <= 0:
                    continue
                src = next((s for s in ev.stack if "perceptor_amd" in s), ev.stack[0] if ev.stack else "?")
                r = rows.setdefault((ev.name, src.strip()[:110]), [0, 0.0])
                r[0] += 1
                r[1] += ev.self_device_time_total
            print(f"{arch}: aten ops with device time in one loss_and_grad: {sum(r[0] for r in rows.values())} launches")
            for k, r in sorted(rows.items(), key=lambda kv: -kv[1][1]):
                print(f"  {r[1]:9.1f} us {r[0]:4d} x  {k[0]:28s} {k[1]}")
        if a.gemm_trace:
            from perceptor_amd.engine import ops
            ops.GEMM_TRACE = []
            loss.loss_and_grad(img)
            torch.cuda.synchronize()
            rows = {}
            for desc, fl, e0, e1 in ops.GEMM_TRACE:
                r = rows.setdefault(desc, [0, 0.0, 0.0])
                r[0] += 1
                r[1] += e0.elapsed_time(e1)
                r[2] += fl
            ops.GEMM_TRACE = None
            tot = sum(r[1] for r in rows.values())
            print(f"{arch}: pmi_igemm launches of one loss_and_grad: {sum(r[0] for r in rows.values())}, {tot:.3f} ms (events per launch)")
            for desc, (k, ms, fl) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
                print(f"  {ms:8.3f} ms {k:4d} x {fl / ms / 1e9 if ms > 0 else 0:7.1f} TFLOP/s  {desc}")
        del loss, eng, img
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
