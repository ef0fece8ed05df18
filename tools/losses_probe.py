#!/usr/bin/env python3
"""Guidance losses: what one shared tower pass saves, and what the smoothness kernel moves.

  python tools/losses_probe.py [--arch ViT-L-14] [--batch 8] [--size 512] [--dtype bf16] [--runs 20] [--warmup 3] [--out FILE]

1. losses.CLIP.loss_and_grad + losses.SimulacraAesthetic.loss_and_grad on one tower as two calls (two tower passes, as the reference runs
   them) against one losses.tower_loss_and_grad([clip, simulacra]) (one forward, one backward): median of --runs device-event timings each,
   after warm-up, in one process.  Synthetic weights.
2. pmi_smoothness on batch x 3 x size x size fp32: median time and the bytes it has to move (one read of x, one write of the gradient;
   neighbour reads are cache hits), with the bandwidth that implies -- once rotating over more buffers than the last-level cache
   holds (the HBM figure) and once on one buffer pair (cache resident).
Lines are printed and, with --out, written to a file.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, runs, warmup):
    """median / min / max milliseconds of fn() by device events, one pair per run"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="ViT-L-14")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("losses_probe needs a HIP device")
    from perceptor_amd import losses
    from perceptor_amd._hip import call, ptr
    from perceptor_amd.utils.synth import seeded_noise
    dev = torch.device("cuda:0")
    lines = []

    clip = losses.CLIP(a.arch, a.dtype, weights="synthetic").to(dev)
    clip.add_encodings_(torch.nn.functional.normalize(seeded_noise((2, clip.model.output_dim), 7)))
    sim = losses.SimulacraAesthetic(a.arch, 10, model=clip.model).to(dev)
    img = (seeded_noise((a.batch, 3, a.size, a.size), 1234) * 0.25 + 0.5).to(dev)

    def two_calls():
        la, ga = clip.loss_and_grad(img)
        ls, gs = sim.loss_and_grad(img)
        return la + ls, ga + gs

    def one_call():
        return losses.tower_loss_and_grad(img, [clip, sim])[:2]

    (l2, g2), (l1, g1) = two_calls(), one_call()
    rel = float((g1.double() - g2.double()).norm() / g2.double().norm())
    t2, t1 = timed(two_calls, a.runs, a.warmup), timed(one_call, a.runs, a.warmup)
    tag = f"{a.arch} batch {a.batch} {a.size}x{a.size} {a.dtype}, median of {a.runs} (min .. max) ms"
    lines.append(f"CLIP.loss_and_grad + SimulacraAesthetic.loss_and_grad, two calls, {tag}: {t2[0]:.3f} ({t2[1]:.3f} .. {t2[2]:.3f})")
    lines.append(f"tower_loss_and_grad([CLIP, SimulacraAesthetic]), one call, {tag}: {t1[0]:.3f} ({t1[1]:.3f} .. {t1[2]:.3f})")
    lines.append(f"one call / two calls = {t1[0] / t2[0]:.3f}; total loss {float(l1):.6f} vs {float(l2):.6f}; "
                 f"gradient of the one call against the sum of the two: rel-L2 {rel:.2e} (the 16-bit tower backward rounds a sum differently from two terms)")
    del clip, sim
    torch.cuda.empty_cache()

    # enough (x, gradient) pairs that a pair is out of the 256 MB last-level cache again when its turn comes: an HBM figure;
    # and one pair over and over: what a sampler step sees when the image was just written
    n, c, h, w = img.shape
    pair = 2 * img.numel() * 4
    sets = max(2, -(-3 * 256 * 2 ** 20 // pair))
    xs = [img.clone() for _ in range(sets)]
    grads = [torch.empty_like(img) for _ in range(sets)]
    loss, partial = torch.empty(1, device=dev), torch.empty(2048, device=dev)
    turn = [0]

    def smooth(rotate):
        i = turn[0] % sets if rotate else 0
        turn[0] += 1
        call("pmi_smoothness", ptr(xs[i]), ptr(loss), ptr(grads[i]), ptr(partial), n, c, h, w, n, 1.0)

    for rotate, what in ((True, f"rotating over {sets} buffer pairs ({sets * pair / 2 ** 20:.0f} MiB: each pair comes from HBM)"),
                         (False, "one buffer pair over and over (it stays in the last-level cache: not an HBM figure)")):
        ts = timed(lambda: smooth(rotate), a.runs, a.warmup)
        lines.append(f"pmi_smoothness {n}x{c}x{h}x{w} fp32, {what}, median of {a.runs} (min .. max) ms: {ts[0]:.4f} ({ts[1]:.4f} .. {ts[2]:.4f}); "
                     f"{pair / 1e6:.1f} MB moved (x read once, gradient written once) = {pair / ts[0] / 1e9:.2f} TB/s")
    lines.append(f"pmi_smoothness loss {float(loss):.6f}")
    print("\n".join(lines), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
