#!/usr/bin/env python3
"""losses.LPIPS on the VGG-16 tower (engine/lpips.py) at the product shape: batch 4 at 256 x 256, f16 and bf16, medians of device-event
timings after warm-up, one process:
  targets        one tower pass over images_b (what a cached init image costs once)
  tower_2n       one tower pass over a 2N batch (a and b together): against 2 x targets it decides one batch or two passes
  value          value(images_a, cached targets): one tower pass + the five level kernels
  cached         loss_and_grad(images_a, cached targets): the same plus the backward walk
  live           loss_and_grad(images_a, images_b): a and b as one 2N tower pass, a's backward walk
  live_both      the same with the gradient to images_b too (one 2N backward walk, both sides from one level launch per tap)
  live_2pass, live_both_2pass   the same two with b as its own N-sample pass (targets(images_b) inside the timed call), for the record
  spatial        loss_and_grad of the [N, 1, H, W] map with cached targets (bilinear bands and their adjoints)
and, per tap, pmi_lpips_level and pmi_lpips_level_bwd (one side, both sides) on their own: time and bytes moved / time against the HBM
ceiling (about 6.3 TB/s; ten back-to-back launches per timing).  Bytes: forward 2 x 2C read + 12 written per pixel; backward 2 x 2C + 12 read, the pool adjoint(s) 2C each where a
tap has one, 2C written per side.

  python tools/lpips_probe.py [--batch 4] [--iters 20] [--dtype f16 bf16] [--out profiles/lpips_probe.txt]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.3
REPS = 10


def flops(widths, h, w, n):
    """(forward through module 29, the backward's dX convolutions) FLOPs on n images."""
    from perceptor_amd.engine import lpips
    fwd = bwd = 0.0
    for i, l in enumerate(lpips.lpips_layer_table(widths)):
        if l[0] == "conv":
            fwd += 2.0 * n * h * w * l[1] * l[2] * 9
            bwd += 2.0 * n * h * w * l[2] * (8 if i == 0 else l[1]) * 9
        elif l[0] == "pool":
            h, w = h // 2, w // 2
    return fwd, bwd


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dtype", nargs="*", default=["f16", "bf16"])
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from perceptor_amd import losses
    from perceptor_amd._hip import call, ptr
    from perceptor_amd.utils.synth import seeded_noise
    if not torch.cuda.is_available():
        raise SystemExit("lpips_probe needs a HIP device")
    dev = torch.device("cuda:0")
    n, size = a.batch, a.size
    img = lambda seed, k=n: (seeded_noise((k, 3, size, size), seed) * 0.25 + 0.5).clamp(0, 1).to(dev)
    xa, xb = img(21), img(22)
    x2 = torch.cat([xa, xb])

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    for dtype in a.dtype:
        lp = losses.LPIPS(dtype=dtype).to(dev)
        sp = losses.LPIPS(dtype=dtype, spatial=True).to(dev)
        eng = lp._need_engine()
        ff, fb = flops(lp.widths, size, size, n)
        tb = eng.targets(xb)
        tsp = sp.targets(xb)
        go = torch.ones((n, 1, size, size), device=dev)
        cases = [("targets", lambda: eng.targets(xb)), ("tower_2n", lambda: eng.targets(x2)), ("value", lambda: eng.value(xa, tb)),
                 ("cached", lambda: lp.loss_and_grad(xa, tb)), ("live", lambda: lp.loss_and_grad(xa, xb)),
                 ("live_both", lambda: lp.loss_and_grad(xa, xb, grad_b=True)),
                 ("live_2pass", lambda: lp.loss_and_grad(xa, eng.targets(xb))),
                 ("live_both_2pass", lambda: lp.loss_and_grad(xa, eng.targets(xb, keep_tape=True), grad_b=True)),
                 ("spatial", lambda: sp.loss_and_grad(xa, tsp, grad_out=go))]
        ms = {k: _median_ms(fn, a.iters, a.warmup) for k, fn in cases}
        row = dict(tool="lpips_probe", dtype=dtype, batch=n, size=size, device=torch.cuda.get_device_name(0),
                   forward_gflop_per_image=round(ff / n / 1e9, 2), dx_gflop_per_image=round(fb / n / 1e9, 2),
                   **{k + "_ms": round(v, 3) for k, v in ms.items()})
        row["targets_tflops"] = round(ff / ms["targets"] / 1e9, 1)
        row["tower_2n_tflops"] = round(2 * ff / ms["tower_2n"] / 1e9, 1)
        row["cached_tflops"] = round((ff + fb) / ms["cached"] / 1e9, 1)
        row["live_both_tflops"] = round((2 * ff + 2 * fb) / ms["live_both"] / 1e9, 1)
        emit(row)
        # ---- the level kernels on their own, at the tower's real tap features
        ta = eng.targets(xa)
        for l, (fa, fbt, w) in enumerate(zip(ta["feats"], tb["feats"], eng.lins)):
            nn, h, wd, c = fa.shape
            hw = h * wd
            s, na, nb = (torch.empty((nn, hw), dtype=torch.float32, device=dev) for _ in range(3))
            mean, partial = torch.empty(nn, device=dev), torch.empty(512 * nn, device=dev)
            r = torch.full((nn, hw), 1.0 / hw, device=dev)
            gin = torch.zeros_like(fa) if l < 4 else None
            da, db = torch.empty_like(fa), torch.empty_like(fa)
            fwd = lambda: call("pmi_lpips_level", ptr(fa), ptr(fbt), ptr(w), ptr(s), ptr(na), ptr(nb), ptr(mean), ptr(partial), nn, hw, c, eng.dt)
            one = lambda: call("pmi_lpips_level_bwd", ptr(fa), ptr(fbt), ptr(w), ptr(na), ptr(nb), ptr(r), ptr(gin), None, ptr(da), None, nn, hw, c,
                               eng.gscale, eng.dt)
            two = lambda: call("pmi_lpips_level_bwd", ptr(fa), ptr(fbt), ptr(w), ptr(na), ptr(nb), ptr(r), ptr(gin), ptr(gin), ptr(da), ptr(db), nn, hw,
                               c, eng.gscale, eng.dt)
            px = nn * hw
            nbytes = dict(level=px * (4 * c + 12), bwd_one=px * (4 * c + 12 + 2 * c + (2 * c if gin is not None else 0)),
                          bwd_both=px * (4 * c + 12 + 4 * c + (4 * c if gin is not None else 0)))
            rep = lambda fn: (lambda: [fn() for _ in range(REPS)])            # back-to-back launches: the host's launch cost overlaps
            t = {k: _median_ms(rep(fn), a.iters, a.warmup) / REPS for k, fn in (("level", fwd), ("bwd_one", one), ("bwd_both", two))}
            emit(dict(tool="lpips_probe", kind="level_kernels", dtype=dtype, tap=l, N=nn, HW=hw, C=c,
                      **{k + "_us": round(v * 1e3, 1) for k, v in t.items()}, **{k + "_mb": round(v / 1e6, 2) for k, v in nbytes.items()},
                      **{k + "_tbs": round(nbytes[k] / t[k] / 1e9, 3) for k in t},
                      **{k + "_of_hbm": round(nbytes[k] / t[k] / 1e9 / HBM_TBS, 3) for k in t}))
        del lp, sp, eng, tb, tsp, ta
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
