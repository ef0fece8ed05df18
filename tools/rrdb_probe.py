#!/usr/bin/env python3
"""pmi_rdb_conv3x3 (csrc/rrdb.hip) against ops.igemm on the same arithmetic, per shape of the Real-ESRGAN RRDBNet, and one whole "x4"
forward.  One process; per shape the two paths alternate round by round (device events around `--inner` back-to-back launches, after
warm-up of both), and the medians and minima over the rounds are reported.

  trunk shapes at 512 x 512, N = 1:  64 / 96 / 128 / 160 -> 32 and 192 -> 64 (LeakyReLU; conv5 with alpha = 0.2 and R1), 64 -> 64 (conv_body, R1)
  tail shapes:                       64 -> 64 with the nearest-x2 read at 1024^2 (conv_up1) and 2048^2 (conv_up2), 64 -> 64 at 2048^2 (conv_hr)
Baseline: what the engine would run without the kernel -- ops.igemm on a CONTIGUOUS input of exactly Cin channels (the concatenation
already made, its cost not counted), bias in the launch, 16-bit output; ops.igemm has no LeakyReLU and no scaled second residual, so the
baseline does LESS work than the kernel it is compared with (no activation, at most one unscaled residual).  Outputs of the two paths
are compared on the same seeded inputs (slope 1, no residual) before timing.
FLOPs are 2 * 9 * Cin * N per output pixel; the share of peak is against 2.5 PFLOP/s dense 16-bit.

  python tools/rrdb_probe.py [--dtype f16 bf16] [--rounds 7] [--inner 10] [--forward 512] [--out profiles/rrdb_probe.txt]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 2.5e15
SHAPES = [  # (tag, cin, n, output size, up, residual)
    ("rdb.conv1", 64, 32, 512, False, False), ("rdb.conv2", 96, 32, 512, False, False), ("rdb.conv3", 128, 32, 512, False, False),
    ("rdb.conv4", 160, 32, 512, False, False), ("rdb.conv5", 192, 64, 512, False, True), ("conv_body", 64, 64, 512, False, True),
    ("conv_up1", 64, 64, 1024, True, False), ("conv_up2", 64, 64, 2048, True, False), ("conv_hr", 64, 64, 2048, False, False),
]


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
    ap.add_argument("--dtype", nargs="*", default=["f16", "bf16"])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--forward", type=int, default=512, help="input size of the whole x4 forward (0: skip)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from perceptor_amd import _hip, models
    from perceptor_amd.engine import ops
    from perceptor_amd.engine.ops import PackedLinear
    from perceptor_amd.engine.rrdb import RrdbEngine, _RdbConv
    from perceptor_amd.utils.synth import synth_tensor
    if not torch.cuda.is_available():
        raise SystemExit("rrdb_probe needs a HIP device")
    dev = torch.device("cuda:0")

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    for dtype in a.dtype:
        dt = _hip.dtype_code(dtype)
        td = _hip.TORCH_DTYPE[dt]
        eng = RrdbEngine.__new__(RrdbEngine)            # only .conv (one launch) is used
        eng.dt = dt
        for tag, cin, n, size, up, res in SHAPES:
            w, b = synth_tensor(f"{tag}.weight", (n, cin, 3, 3), 0), synth_tensor(f"{tag}.bias", (n,), 0)
            cv, lin = _RdbConv(w, b, dt, dev), PackedLinear(w, b, dt, dev)
            hin = size // 2 if up else size
            g = torch.Generator().manual_seed(cin + n)
            x = (torch.rand((1, hin, hin, cin), generator=g) - 0.5).to(td).to(dev)
            r = (torch.rand((1, size, size, n), generator=g) - 0.5).to(td).to(dev) if res else None
            out_k = torch.empty((1, size, size, n), dtype=td, device=dev)
            out_i = torch.empty((1, size, size, n), dtype=td, device=dev)
            # same arithmetic first: slope 1, no residual
            eng.conv(cv, x, out_k, up=up)
            ops.igemm(x, lin, up=up, out=out_i)
            torch.cuda.synchronize()
            diff = float((out_k.float() - out_i.float()).abs().max())
            scale = float(out_i.float().abs().max())
            kern = lambda: eng.conv(cv, x, out_k, r1=r, alpha=0.2 if res else 1.0, slope=1.0 if res else 0.2, up=up)
            base = lambda: ops.igemm(x, lin, up=up, residual=r, out=out_i)
            for _ in range(a.warmup):
                kern(), base()
            torch.cuda.synchronize()
            tk, tb = [], []
            for _ in range(a.rounds):
                tk.append(_timed(kern, a.inner))
                tb.append(_timed(base, a.inner))
            fl = 2.0 * 9 * cin * n * size * size
            mk, mb = statistics.median(tk), statistics.median(tb)
            emit(dict(tool="rrdb_probe", dtype=dtype, shape=tag, cin=cin, n=n, size=size, up=int(up), residual=int(res),
                      rdb_ms=round(mk, 4), rdb_min_ms=round(min(tk), 4), igemm_ms=round(mb, 4), igemm_min_ms=round(min(tb), 4),
                      igemm_over_rdb=round(mb / mk, 3), rdb_tflops=round(fl / mk / 1e9, 1), igemm_tflops=round(fl / mb / 1e9, 1),
                      rdb_peak_share=round(fl / mk / 1e-3 / PEAK, 4), igemm_peak_share=round(fl / mb / 1e-3 / PEAK, 4),
                      max_abs_diff=diff, out_abs_max=scale))
            del x, r, out_k, out_i, cv, lin
            torch.cuda.empty_cache()
        if a.forward:
            m = models.SuperResolution("x4", dtype=dtype).to(dev)
            img = torch.rand((1, 3, a.forward, a.forward), generator=torch.Generator().manual_seed(1)).to(dev)
            fn = lambda: m(img)
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            ts = [_timed(fn, 1) for _ in range(max(3, a.rounds // 2))]
            px = a.forward * a.forward
            fl = px * (23 * 3 * 2.0 * 9 * (64 * 32 + 96 * 32 + 128 * 32 + 160 * 32 + 192 * 64) + 2.0 * 9 * (8 * 64 + 64 * 64)) \
                + 2.0 * 9 * 64 * 64 * (4 * px + 16 * px + 16 * px) + 2.0 * 9 * 64 * 4 * 16 * px
            ms = statistics.median(ts)
            emit(dict(tool="rrdb_probe", dtype=dtype, shape="x4 forward", size=a.forward, ms=round(ms, 2), min_ms=round(min(ts), 2),
                      tflop=round(fl / 1e12, 3), tflops=round(fl / ms / 1e9, 1), peak_share=round(fl / ms / 1e-3 / PEAK, 4)))
            del m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
