"""Precise-mode input gradient: per-stage gradient range, tape size and timing.

    python tools/precise_backward_probe.py range      # max |g| entering every tape record, 558 M ADM net and yfcc_2 at 128 x 128
    python tools/precise_backward_probe.py time NAME  # forward_train + backward, 20 calls after 3 warm-up, device events, f16 next to precise
                                                      # NAME: standard (512 x 512 x 8), yfcc_2 (512 x 512 x 8), cc12m_1 (256 x 256 x 1)

A split value keeps its ~22 bits only while lo = f16(x - hi) is a normal f16 (|x| >~ 2^-3 ... 2^-12 with a shrinking share of bits); the
range run reports every stage whose max |g| (after the input's power-of-two scale) falls below 2^-12.
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"


def _engines(name, dtype):
    from perceptor_amd.engine import adm, vdiff
    from perceptor_amd import models
    from perceptor_amd.utils.synth import synth_state_dict
    if name == "standard":
        cfg = adm.openimages_config()
        sd = synth_state_dict(adm.state_dict_shapes(cfg), 0)
        eng = adm.AdmEngine(cfg, sd, DEV, dtype)
        return eng, sd, (lambda img, n: eng.forward_train(img, torch.full((n,), 333.0, device=DEV), sd, out_channels=3)), \
            (lambda tape, d: eng.backward(tape, d, sd))
    m = models.VelocityDiffusion("cc12m_1_cfg" if name == "cc12m_1" else name, dtype=dtype).to(DEV)
    eng, sd = m.engine, m.model.state_dict()
    ce = torch.randn(1, 512, generator=torch.Generator().manual_seed(4)).to(DEV) if name == "cc12m_1" else None
    return eng, sd, (lambda img, n: eng.forward_train(img, torch.full((n,), 0.5, device=DEV), ce.expand(n, -1) if ce is not None else None)), \
        (lambda tape, d: eng.backward(tape, d, sd))


def _inputs(n, size):
    g = torch.Generator().manual_seed(3)
    return torch.rand(n, 3, size, size, generator=g).to(DEV), torch.randn(n, 3, size, size, generator=g).to(DEV)


def run_range():
    out = {}
    for name in ("standard", "yfcc_2"):
        eng, sd, fwd, bwd = _engines(name, "precise")
        stages = []

        def wrap(fn, label):
            def inner(rec, g, *a, **k):
                stages.append((f"{label}:{getattr(rec[1], 'p', None) or rec[2] if len(rec) > 2 and isinstance(rec[2], str) else getattr(rec[1], 'p', label)}",
                               float(g.float().abs().max())))
                return fn(rec, g, *a, **k)
            return inner
        eng._res_back, eng._attn_back = wrap(eng._res_back, "res"), wrap(eng._attn_back, "attn")
        img, probe = _inputs(1, 128)
        _, tape = fwd(img, 1)
        bwd(tape, probe)
        vals = [v for _, v in stages]
        low = [(s, v) for s, v in stages if v < 2.0 ** -12]
        out[name] = dict(stages=len(stages), max=max(vals), min=min(vals), below_2m12=low, first=stages[:3], last=stages[-3:])
        print(f"[range] {name}: {len(stages)} stages, max |g| per stage in [{min(vals):.3e}, {max(vals):.3e}] "
              f"(2^{torch.tensor(min(vals)).log2():.1f} .. 2^{torch.tensor(max(vals)).log2():.1f}); below 2^-12: {len(low)}", flush=True)
        del eng, tape
        torch.cuda.empty_cache()
    return out


def run_time(name):
    n, size = dict(standard=(8, 512), yfcc_2=(8, 512), cc12m_1=(1, 256))[name]
    res = {}
    for dtype in ("f16", "precise"):
        eng, sd, fwd, bwd = _engines(name, dtype)
        img, probe = _inputs(n, size)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        _, tape = fwd(img, n)
        torch.cuda.synchronize()
        tape_gb = (torch.cuda.memory_allocated() - base) / 1e9
        bwd(tape, probe)
        del tape
        ms = []
        for i in range(23):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, tape = fwd(img, n)
            bwd(tape, probe)
            e1.record()
            del tape
            torch.cuda.synchronize()
            if i >= 3:
                ms.append(e0.elapsed_time(e1))
        res[dtype] = dict(ms=sum(ms) / len(ms), tape_gb=tape_gb, peak_gb=torch.cuda.max_memory_allocated() / 1e9)
        print(f"[time] {name} {size}x{size} x {n} {dtype}: forward_train + backward {res[dtype]['ms']:.1f} ms, tape {tape_gb:.1f} GB, "
              f"peak {res[dtype]['peak_gb']:.1f} GB", flush=True)
        del eng
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
    print(f"[time] {name}: precise / f16 = {res['precise']['ms'] / res['f16']['ms']:.2f}")
    return res


if __name__ == "__main__":
    with torch.no_grad():
        r = run_range() if sys.argv[1] == "range" else run_time(sys.argv[2])
    print(json.dumps(r))
