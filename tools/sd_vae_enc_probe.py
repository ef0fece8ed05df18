#!/usr/bin/env python3
"""GPU probe of the VAE encoder's image gradient.

    python tools/sd_vae_enc_probe.py [--reps 10] [--json out.json] [--aten] [--no-engine]

1. A/B of the Downsample2D adjoint at the three SD-v1 encoder down-samplers of 512 x 512 images, batch 4, bf16: the phased pmi_igemm
   launch (ops.downsample_adjoint) against the composed form of engine/adm.py (zero-inserted [N, 2h, 2w, C] buffer by two torch ops, then
   the stride-1 3x3 dX).  Same process, alternating, median of `reps` x 3; the two results are compared to each other.
2. SD-v1 encoder at 512 x 512 x 4, bf16: forward, forward_train and backward times, tape bytes and peak memory.
--aten lists the torch kernels launched inside backward (torch.profiler; there should be none)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from perceptor_amd import _hip  # noqa: E402
from perceptor_amd.engine import ops, sd  # noqa: E402
from perceptor_amd.utils.synth import seeded_noise, synth_state_dict  # noqa: E402


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def tape_bytes(tape):
    seen, total = set(), 0

    def walk(o):
        nonlocal total
        if torch.is_tensor(o):
            if o.data_ptr() not in seen:
                seen.add(o.data_ptr())
                total += o.numel() * o.element_size()
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v)
        elif isinstance(o, dict):
            for v in o.values():
                walk(v)
    walk(tape)
    return total


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--json", default=None)
    p.add_argument("--aten", action="store_true")
    p.add_argument("--no-engine", action="store_true")
    a = p.parse_args()
    dev, dt = torch.device("cuda"), _hip.DT_BF16
    res = {"adjoint_ab": []}

    for hw, c in ((256, 128), (128, 256), (64, 512)):              # gradient grid -> twice that, channels
        gen = torch.Generator().manual_seed(c)
        wt = torch.randn((c, c, 3, 3), generator=gen) / (9 * c) ** 0.5
        phased = ops.PackedLinear(sd.pack_downsample_adjoint_weights(wt).float(), None, dt, dev)
        cache = {}
        flipped = ops.packed_dx(cache, "T", wt, dt, dev)
        g = torch.randn((4, hw, hw, c), generator=gen).to(torch.bfloat16).to(dev)

        def run_phased():
            return ops.downsample_adjoint(g, phased)

        def run_composed():
            # engine/adm.py: the stride-1 dX of the zero-inserted gradient.  Downsample2D pads right / bottom only: its adjoint is the
            # pad-1 dX shifted by one pixel, i.e. the same pass over a buffer whose samples sit at the odd positions
            z = torch.zeros((4, 2 * hw + 1, 2 * hw + 1, c), dtype=g.dtype, device=dev)
            z[:, 1::2, 1::2] = g
            return ops.igemm(z, flipped)[:, :2 * hw, :2 * hw]

        def run_composed_adm():
            # exactly ADM's two ops + one pass (the symmetric-pad geometry: same cost, one pixel off for this operator)
            z = torch.zeros((4, 2 * hw, 2 * hw, c), dtype=g.dtype, device=dev)
            z[:, ::2, ::2] = g
            return ops.igemm(z, flipped)

        y0, y1 = run_phased().float(), run_composed().float()
        diff = float((y0 - y1).abs().max() / y1.abs().max())
        tp, tc = [], []
        for _ in range(3):
            tp.append(timed(run_phased, a.reps))
            tc.append(timed(run_composed_adm, a.reps))
        row = {"grid": f"{hw}->{2 * hw}", "C": c, "phased_ms": statistics.median(tp), "composed_ms": statistics.median(tc),
               "phased_all": tp, "composed_all": tc, "max_diff_rel": diff,
               "phased_tflops": 2.0 * 4 * hw * hw * c * c * 9 / statistics.median(tp) / 1e9}
        res["adjoint_ab"].append(row)
        print("[ab]", json.dumps(row), flush=True)
        del g, y0, y1

    if not a.no_engine:
        w = synth_state_dict(sd.vae_encoder_state_dict_shapes(sd.VAE_V1), 0)
        eng = sd.VaeEncoderEngine(sd.VAE_V1, w, dev, "bf16")
        img = (seeded_noise((4, 3, 512, 512), 74) * 0.25 + 0.5).to(dev)
        dm, dl = (seeded_noise((4, 4, 64, 64), 93) * 1e-6).to(dev), (seeded_noise((4, 4, 64, 64), 94) * 1e-6).to(dev)
        eng.forward(img)
        _, tape = eng.forward_train(img)
        eng.backward(tape, dm, dl, w)                                # packs the transposed / phase-packed weights
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res["forward_ms"] = statistics.median(timed(lambda: eng.forward(img), a.reps) for _ in range(3))
        res["forward_peak_mib"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        torch.cuda.reset_peak_memory_stats()
        res["forward_train_ms"] = statistics.median(timed(lambda: eng.forward_train(img), a.reps) for _ in range(3))
        res["backward_ms"] = statistics.median(timed(lambda: eng.backward(tape, dm, dl, w), a.reps) for _ in range(3))
        res["train_peak_mib"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
        res["tape_mib"] = tape_bytes(tape) / 2 ** 20
        print("[c4 encoder]", json.dumps({k: v for k, v in res.items() if k != "adjoint_ab"}), flush=True)
        if a.aten:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                eng.backward(tape, dm, dl, w)
                torch.cuda.synchronize()
            aten = [(ev.name, ev.self_device_time_total) for ev in prof.events() if ev.name.startswith("aten::") and ev.self_device_time_total > 0]
            res["aten_kernels_in_backward"] = aten
            print("[aten]", len(aten), aten[:20], flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
