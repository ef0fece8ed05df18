#!/usr/bin/env python3
"""drawers.JPEG.synthesize() and its backward pass (csrc/jpeg.hip: one launch each) at N = 8, 512 x 512, against the SAME arithmetic as the
reference's sequence of stock torch ops on the same GPU (tests/_jpeg_ref64.TorchDecoder in fp32: dequantise, alpha, 64 x 64 tensordot per
block, merge, two repeats, cat, colour tensordot, permute, two-sided clamp, / 255; its backward is torch autograd).

One process; the paths alternate round by round (device events around `--inner` back-to-back calls, after warm-up of all of them); medians and
minima over the rounds.  Traffic floor: forward 4.5 floats per pixel (1.5 coefficients read, 3 samples written), backward 6 (1.5 + 3 read,
1.5 written); achieved bytes/s = floor bytes / time, and its share of the HBM peak.  The two decoders' outputs are compared first.

  python tools/jpeg_probe.py [--n 8] [--size 512] [--rounds 7] [--inner 50] [--out profiles/jpeg_probe.txt]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK = 8.0e12       # bytes/s, MI355X


def _timed(fn, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--factor", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import _jpeg_ref64 as J
    from perceptor_amd import drawers
    from perceptor_amd.engine import jpeg as E
    if not torch.cuda.is_available():
        raise SystemExit("jpeg_probe needs a HIP device")
    dev = torch.device("cuda:0")
    n, h, w = a.n, a.size, a.size
    gen = torch.Generator().manual_seed(0)
    drawer = drawers.JPEG(torch.rand((n, 3, h, w), generator=gen).to(dev), factor=a.factor)
    with torch.no_grad():
        for p in drawer.ycbcr:          # noise on the coefficients so that both clamp edges are live, as in the tests
            p.add_(J.SIGMA * torch.randn(p.shape, generator=gen).to(dev))
    g = torch.randn((n, 3, h, w), generator=gen).to(dev)
    ref = J.TorchDecoder(h, w, a.factor, device=dev, dtype=torch.float32)
    leaves = [p.detach().clone().requires_grad_(True) for p in drawer.ycbcr]
    coef = [p.detach() for p in drawer.ycbcr]

    def hip_fwd():
        with torch.no_grad():
            return drawer.synthesize()

    def hip_fwd_bwd():
        for p in drawer.ycbcr:
            p.grad = None
        drawer.synthesize().backward(g)

    def hip_bwd_kernel():
        return E.jpeg_decode_backward(*coef, g, a.factor)

    def torch_fwd():
        with torch.no_grad():
            return ref(*coef)

    def torch_fwd_bwd():
        for p in leaves:
            p.grad = None
        ref(*leaves).backward(g)

    # same results first: forward to fp32 rounding of a 0 .. 1 image, gradients relative to their size (a clamp decision may differ on
    # a value within rounding of an edge; counted, not hidden)
    out_h, out_t = hip_fwd(), torch_fwd()
    hip_fwd_bwd(), torch_fwd_bwd()
    torch.cuda.synchronize()
    fwd_diff = float((out_h - out_t).abs().max())
    grad_rel = [float((p.grad - q.grad).abs().max() / q.grad.abs().max()) for p, q in zip(drawer.ycbcr, leaves)]
    paths = dict(hip_fwd=hip_fwd, hip_fwd_bwd=hip_fwd_bwd, hip_bwd_kernel=hip_bwd_kernel, torch_fwd=torch_fwd, torch_fwd_bwd=torch_fwd_bwd)
    for _ in range(a.warmup):
        for fn in paths.values():
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in paths}
    for _ in range(a.rounds):
        for k, fn in paths.items():
            times[k].append(_timed(fn, a.inner))
    med = {k: statistics.median(v) for k, v in times.items()}
    px = n * h * w
    fwd_bytes, bwd_bytes = 4.5 * 4 * px, 6.0 * 4 * px
    row = dict(tool="jpeg_probe", n=n, size=a.size, factor=a.factor, rounds=a.rounds, inner=a.inner,
               **{k + "_ms": round(v, 4) for k, v in med.items()}, **{k + "_min_ms": round(min(v), 4) for k, v in times.items()},
               torch_over_hip_fwd=round(med["torch_fwd"] / med["hip_fwd"], 2),
               torch_over_hip_fwd_bwd=round(med["torch_fwd_bwd"] / med["hip_fwd_bwd"], 2),
               hip_fwd_GBps=round(fwd_bytes / med["hip_fwd"] / 1e6, 1), hip_fwd_hbm_share=round(fwd_bytes / (med["hip_fwd"] * 1e-3) / HBM_PEAK, 4),
               hip_bwd_kernel_GBps=round(bwd_bytes / med["hip_bwd_kernel"] / 1e6, 1),
               hip_bwd_kernel_hbm_share=round(bwd_bytes / (med["hip_bwd_kernel"] * 1e-3) / HBM_PEAK, 4),
               fwd_floor_bytes=int(fwd_bytes), bwd_floor_bytes=int(bwd_bytes), fwd_max_abs_diff=fwd_diff, grad_max_rel_diff=grad_rel)
    print(json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(json.dumps(row) + "\n")


if __name__ == "__main__":
    main()
