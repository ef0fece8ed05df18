#!/usr/bin/env python3
"""MonsterDiffusion input-gradient timings: forward, forward_train and forward_train + backward of engine/monster.py (product config,
48 x 48) at batch 1, 16 and 64 in f16 and bf16; the two FIR adjoints (csrc/fir.hip) as achieved GB/s next to a device-to-device copy of the
same bytes measured in the same run; and the tape's device bytes.

Method of tools/monster_probe.py: one process, per item the variants alternate round by round (device events around `--inner` back-to-back
calls, after warm-up of all of them), medians and minima over the rounds.  host_issue_ms is the host time to ISSUE one call (bf16 never
synchronises inside; f16's backward reads the per-sample maxima once): where it is close to the device-event time the row is bound by the
host's launch rate, not by the kernels.  FIR bytes are input + output, each touched once.  tape_bytes counts every distinct device buffer
the tape references; peak_alloc_bytes is torch's peak over one forward_train + backward.

  python tools/monster_grad_probe.py [--dtype f16 bf16] [--batch 1 16 64] [--rounds 7] [--inner 3] [--out profiles/monster_grad_probe.txt]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from monster_probe import FIR_SHAPES, _alternate      # noqa: E402


def tape_bytes(tape):
    import torch
    seen = {}

    def walk(v):
        if torch.is_tensor(v):
            if v.is_cuda:
                seen[v.untyped_storage().data_ptr()] = v.untyped_storage().nbytes()
        elif isinstance(v, dict):
            for t in v.values():
                walk(t)
        elif isinstance(v, (list, tuple)):
            for t in v:
                walk(t)

    walk(tape)
    return sum(seen.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dtype", nargs="*", default=["f16", "bf16"])
    ap.add_argument("--batch", nargs="*", type=int, default=[1, 16, 64])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from perceptor_amd import _hip
    from perceptor_amd.engine import monster, ops
    if not torch.cuda.is_available():
        raise SystemExit("monster_grad_probe needs a HIP device")
    dev = torch.device("cuda:0")

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    def host_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return ms

    config = monster.product_config()
    sd = monster.synthetic_state_dict(config, 0)
    for dtype in a.dtype:
        dt = _hip.dtype_code(dtype)
        td = _hip.TORCH_DTYPE[dt]
        # ---- the adjoints against a copy of the same bytes: `shape` is the forward's input, so dx has it ----
        for which, shape in FIR_SHAPES:
            n, h, w, c = shape
            g = torch.randn((n, h // 2, w // 2, c) if which == "down" else (n, 2 * h, 2 * w, c), device=dev).to(td)
            fn = ops.fir_down2_bwd if which == "down" else ops.fir_up2_bwd
            dx = fn(g, dt)
            nbytes = (g.numel() + dx.numel()) * 2
            src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            dst = torch.empty_like(src)
            r = _alternate({"fir": lambda: fn(g, dt), "copy": lambda: dst.copy_(src)}, a.rounds, max(a.inner, 20), a.warmup)
            emit(dict(item=f"fir_{which}_bwd", dtype=dtype, dx_shape=list(shape), bytes=nbytes, fir_ms=r["fir"][0], fir_min_ms=r["fir"][1],
                      fir_gbs=nbytes / r["fir"][0] / 1e6, copy_ms=r["copy"][0], copy_gbs=nbytes / r["copy"][0] / 1e6,
                      fir_over_copy=r["fir"][0] / r["copy"][0]))
        # ---- forward, forward_train, forward_train + backward ----
        eng = monster.MonsterEngine(config, sd, dev, dtype)
        for batch in a.batch:
            images = torch.rand((batch, 3, 48, 48), device=dev)
            sigma = torch.linspace(0.05, 60.0, batch, device=dev)
            cot = torch.randn((batch, 3, 48, 48), device=dev)

            def both():
                _, tape = eng.forward_train(images, sigma)
                return eng.backward(tape, cot, sd)

            variants = {"forward": lambda: eng.forward(images, sigma), "forward_train": lambda: eng.forward_train(images, sigma), "train_backward": both}
            r = _alternate(variants, a.rounds, a.inner, a.warmup)
            host = {k: host_ms(fn) for k, fn in variants.items()}
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            _, tape = eng.forward_train(images, sigma)
            tb = tape_bytes(tape)
            eng.backward(tape, cot, sd)
            torch.cuda.synchronize()
            peak = torch.cuda.max_memory_allocated() - base
            del tape
            emit(dict(item="gradient", dtype=dtype, batch=batch, forward_ms=r["forward"][0], forward_min_ms=r["forward"][1],
                      forward_train_ms=r["forward_train"][0], train_backward_ms=r["train_backward"][0], train_backward_min_ms=r["train_backward"][1],
                      ratio_train_backward_over_forward=r["train_backward"][0] / r["forward"][0],
                      ratio_forward_train_over_forward=r["forward_train"][0] / r["forward"][0],
                      host_issue_forward_ms=host["forward"], host_issue_forward_train_ms=host["forward_train"],
                      host_issue_train_backward_ms=host["train_backward"], tape_bytes=tb, peak_alloc_bytes=peak))
        del eng


if __name__ == "__main__":
    main()
