#!/usr/bin/env python3
"""losses.StyleTransfer on the VGG-19 tower (engine/vgg.py) at the product shape: batch 4 at 256 x 256, f16 and bf16, medians of
device-event timings after warm-up, one process:
  targets        one tower pass to relu4_2 + the three Gram matrices (what a cached style image costs once)
  cached         loss_and_grad(images) against stored encodings: one tower pass, level sums, the backward walk
  live           loss_and_grad(images_a, images_b): the same plus b's tower pass
and the achieved TFLOP/s from FLOPs computed from the layer shapes: the forward to relu4_2 (every convolution, 36.5 GFLOP per image at
256 x 256) and the backward's dX convolutions (each convolution's input gradient at its own grid; conv1_1's on the 8-channel padded
output) -- the Gram GEMMs and the level-gradient GEMMs are listed on their own.

  python tools/vgg_probe.py [--batch 4] [--iters 20] [--dtype f16 bf16] [--out profiles/vgg_probe.txt]
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/vgg_probe.py --dtype f16 --iters 5 --warmup 2 --cached-only
  python tools/vgg_probe.py --kernel-stats DIR [--out profiles/vgg_kernel_stats.txt]      (summary of that run's kernel_stats.csv)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def flops(widths, size, n):
    """(forward to relu4_2, dX convolutions of the backward, the three Grams, the three level-gradient GEMMs) FLOPs on n images."""
    from perceptor_amd.engine import vgg
    table = vgg.layer_table(widths)
    fwd = bwd = gram = gbw = 0.0
    s = size
    for i, l in enumerate(table[:vgg.LOSS_LAST + 1]):
        if l[0] == "conv":
            fwd += 2.0 * n * s * s * l[1] * l[2] * 9
            bwd += 2.0 * n * s * s * l[2] * (8 if i == 0 else l[1]) * 9
            if i in vgg.LEVEL_WEIGHTS:
                r = n * l[2]
                gram += 2.0 * r * r * s * s
                gbw += 2.0 * n * s * s * l[2] * r
        elif l[0] == "pool":
            s //= 2
    return fwd, bwd, gram, gbw


def _median_ms(fn, iters, warmup):
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def kernel_stats(d, out):
    path = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)[0]
    rows = list(csv.DictReader(open(path)))
    tot = sum(float(r["TotalDurationNs"]) for r in rows)
    lines = ["    total us  calls  share  kernel"]
    for r in rows[:30]:
        name = r["Name"].replace("void (anonymous namespace)::", "").replace("(anonymous namespace)::", "")
        lines.append(f"{float(r['TotalDurationNs']) / 1e3:12.1f} {int(r['Calls']):6d} {float(r['TotalDurationNs']) / tot:6.1%}  {name[:150]}")
    text = "\n".join(lines)
    print(text)
    if out:
        with open(out, "a") as f:
            f.write(text + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", nargs="*", default=["f16", "bf16"])
    ap.add_argument("--cached-only", action="store_true")
    ap.add_argument("--kernel-stats")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a.kernel_stats, a.out)
    import torch
    from perceptor_amd import losses
    from perceptor_amd.engine import vgg
    from perceptor_amd.utils.synth import seeded_noise
    if not torch.cuda.is_available():
        raise SystemExit("vgg_probe needs a HIP device")
    dev = torch.device("cuda:0")
    widths, size = vgg.VGG19_CONFIG
    img = lambda seed: (seeded_noise((a.batch, 3, size, size), seed) * 0.25 + 0.5).clamp(0, 1).to(dev)
    xa, xb = img(21), img(22)
    ff, fb, fg, fl = flops(widths, size, a.batch)
    for dtype in a.dtype:
        st = losses.StyleTransfer(xb, dtype=dtype)
        eng = st.model._need_engine()
        cases = [("cached", lambda: st.loss_and_grad(xa))]
        if not a.cached_only:
            cases = [("targets", lambda: eng.targets(xb))] + cases + [("live", lambda: st.loss_and_grad(xa, xb))]
        ms = {k: _median_ms(fn, a.iters, a.warmup) for k, fn in cases}
        row = dict(tool="vgg_probe", dtype=dtype, batch=a.batch, size=size, device=torch.cuda.get_device_name(0),
                   forward_gflop_per_image=round(ff / a.batch / 1e9, 2), dx_gflop_per_image=round(fb / a.batch / 1e9, 2),
                   gram_gflop=round(fg / 1e9, 2), level_grad_gflop=round(fl / 1e9, 2), **{k + "_ms": round(v, 3) for k, v in ms.items()})
        if "targets" in ms:
            row["targets_tflops"] = round((ff + fg) / ms["targets"] / 1e9, 1)
            row["live_tflops"] = round((2 * ff + 2 * fg + fb + fl) / ms["live"] / 1e9, 1)
        row["cached_tflops"] = round((ff + fg + fb + fl) / ms["cached"] / 1e9, 1)
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")
        del st, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
