#!/usr/bin/env python3
"""MonsterDiffusion timings: one evaluation (engine/monster.py, product config, 48 x 48) at batch 1, 16 and 64 in f16 and bf16, eager and
replayed through engine/graph.GraphedStep; a 50-evaluation sample(); and the two FIR resamplers (csrc/fir.hip) as achieved GB/s next to a
device-to-device copy of the same bytes measured in the same run.

One process.  Per item the variants alternate round by round (device events around `--inner` back-to-back calls, after warm-up of all of
them); medians and minima over the rounds are reported.  An evaluation is 36.27 GFLOP per sample (2 * MAC, the reference module under
torch.utils.flop_counter); the share of peak is against 2.5 PFLOP/s dense 16-bit.  FIR bytes are input + output, each touched once.

  python tools/monster_probe.py [--dtype f16 bf16] [--batch 1 16 64] [--rounds 7] [--inner 5] [--sample 50] [--out profiles/monster_probe.txt]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 2.5e15
GFLOP_PER_SAMPLE = 36.27
FIR_SHAPES = [("down", (64, 48, 48, 128)), ("down", (64, 24, 24, 256)), ("up", (64, 48, 48, 128)), ("up", (64, 24, 24, 256))]


def _timed(fn, inner):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(inner):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / inner


def _alternate(variants, rounds, inner, warmup):
    """{name: fn} -> {name: (median ms, min ms)}, the variants taking turns inside every round"""
    for fn in variants.values():
        for _ in range(warmup):
            fn()
    ms = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            ms[k].append(_timed(fn, inner))
    return {k: (statistics.median(v), min(v)) for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", nargs="*", default=["f16", "bf16"])
    ap.add_argument("--batch", nargs="*", type=int, default=[1, 16, 64])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", type=int, default=50, help="evaluations of the whole sample() run (0: skip)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from perceptor_amd import _hip, models
    from perceptor_amd.engine import ops
    from perceptor_amd.engine.graph import GraphedStep
    if not torch.cuda.is_available():
        raise SystemExit("monster_probe needs a HIP device")
    dev = torch.device("cuda:0")

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    for dtype in a.dtype:
        dt = _hip.dtype_code(dtype)
        td = _hip.TORCH_DTYPE[dt]
        # ---- the resamplers against a copy of the same bytes ----
        for which, shape in FIR_SHAPES:
            n, h, w, c = shape
            x = torch.randn(shape, device=dev).to(td)
            fn = ops.fir_down2 if which == "down" else ops.fir_up2
            y = fn(x, dt)
            nbytes = (x.numel() + y.numel()) * 2
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            r = _alternate({"fir": lambda: fn(x, dt), "copy": lambda: dst.copy_(src)}, a.rounds, max(a.inner, 20), a.warmup)
            emit(dict(item=f"fir_{which}", dtype=dtype, shape=list(shape), bytes=nbytes, fir_ms=r["fir"][0], fir_min_ms=r["fir"][1],
                      fir_gbs=nbytes / r["fir"][0] / 1e6, copy_ms=r["copy"][0], copy_gbs=nbytes / r["copy"][0] / 1e6,
                      fir_over_copy=r["fir"][0] / r["copy"][0]))
        # ---- one evaluation, eager and graphed ----
        model = models.MonsterDiffusion(dtype=dtype).to(dev)
        for batch in a.batch:
            images = torch.rand((batch, 3, 48, 48), device=dev)
            sigma = torch.linspace(0.05, 60.0, batch, device=dev)
            variants = {"eager": lambda: model.denoised_(images, sigma)}
            graph_note = "captured"
            try:
                step = GraphedStep(lambda im, ts: model.denoised_(im, ts), images, sigma)
                variants["graph"] = lambda: step(images, sigma)
            except Exception as e:             # recorded, not worked around: how graphs are replayed is not this tool's to change
                graph_note = f"capture failed: {type(e).__name__}: {e}"
            r = _alternate(variants, a.rounds, a.inner, a.warmup)
            t0 = time.perf_counter()
            model.denoised_(images, sigma)
            host_ms = (time.perf_counter() - t0) * 1e3              # host time to ISSUE one eager evaluation (no synchronisation inside)
            torch.cuda.synchronize()
            row = dict(item="evaluation", dtype=dtype, batch=batch, eager_ms=r["eager"][0], eager_min_ms=r["eager"][1], host_issue_ms=host_ms,
                       eager_tflops=GFLOP_PER_SAMPLE * batch / r["eager"][0], graph=graph_note)
            if "graph" in r:
                row.update(graph_ms=r["graph"][0], graph_min_ms=r["graph"][1], graph_tflops=GFLOP_PER_SAMPLE * batch / r["graph"][0],
                           graph_of_peak=GFLOP_PER_SAMPLE * 1e9 * batch / (r["graph"][0] * 1e-3) / PEAK)
            emit(row)
        if a.sample:
            for batch in (1, a.batch[-1]):
                torch.manual_seed(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in model.sample(batch, n_evaluations=a.sample):
                    pass
                torch.cuda.synchronize()
                emit(dict(item="sample", dtype=dtype, batch=batch, evaluations=a.sample, wall_s=time.perf_counter() - t0))
        del model


if __name__ == "__main__":
    main()
