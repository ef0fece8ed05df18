#!/usr/bin/env python3
"""pmi_convt4x4s2 (csrc/disc.hip) per layer of the Real-ESRGAN discriminator at the grids of one 1024 x 1024 image, against pmi_igemm's
taps = 16 / stride 2 FORWARD of the same layer, and one whole loss_and_grad.  One process; per shape the two paths alternate round by round
(device events around `--inner` back-to-back launches, after warm-up of both), and the medians and minima over the rounds are reported.

No older kernel does the adjoint's arithmetic; the yardstick is the forward convolution of the same layer: the same FLOP count (low-resolution
pixels x 2 x 16 Cin Cout) and the mirrored memory traffic (it reads the large tensor the adjoint writes).  The adjoint is timed as the engine
calls it (R and Y present: two more reads of the large tensor), and bare.

  conv1^T  g 512^2 x 128 -> 1024^2 x 64      conv2^T  g 256^2 x 256 -> 512^2 x 128      conv3^T  g 128^2 x 512 -> 256^2 x 256

  python tools/disc_probe.py [--dtype f16 bf16] [--rounds 7] [--inner 10] [--size 1024] [--out profiles/disc_probe.txt]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 2.5e15


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
    ap.add_argument("--size", type=int, default=1024, help="image size (the layers' grids follow); 0 skips the whole loss_and_grad")
    ap.add_argument("--feat", type=int, default=64)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from perceptor_amd import _hip
    from perceptor_amd._hip import call, ptr
    from perceptor_amd.engine import ops
    from perceptor_amd.engine.disc import pack_convt_weights
    from perceptor_amd.engine.ops import PackedLinear
    from perceptor_amd.losses.super_resolution_discriminator import SuperResolutionDiscriminator
    from perceptor_amd.utils.synth import synth_tensor
    if not torch.cuda.is_available():
        raise SystemExit("disc_probe needs a HIP device")
    dev = torch.device("cuda:0")
    size, f = a.size or 1024, a.feat

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "a") as fh:
                fh.write(json.dumps(row) + "\n")

    for dtype in a.dtype:
        dt = _hip.dtype_code(dtype)
        td = _hip.TORCH_DTYPE[dt]
        for k in (1, 2, 3):
            cin, cout, low = f << (k - 1), f << k, size >> k
            w = synth_tensor(f"conv{k}.weight_orig", (cout, cin, 4, 4), 0)
            lin, wp = PackedLinear(w, None, dt, dev), pack_convt_weights(w).to(device=dev, dtype=td)
            gen = torch.Generator().manual_seed(k)
            x = (torch.rand((1, 2 * low, 2 * low, cin), generator=gen) - 0.5).to(td).to(dev)       # forward input; the adjoint's Y
            r = (torch.rand((1, 2 * low, 2 * low, cin), generator=gen) - 0.5).to(td).to(dev)
            g = (torch.rand((1, low, low, cout), generator=gen) - 0.5).to(td).to(dev)
            z = torch.empty((1, low, low, cout), dtype=td, device=dev)
            d = torch.empty((1, 2 * low, 2 * low, cin), dtype=td, device=dev)
            fwd = lambda: ops.igemm(x, lin, stride=2, out=z)
            adj = lambda: call("pmi_convt4x4s2", ptr(g), cout, cout, ptr(wp), cin, ptr(d), cin, ptr(r), cin, ptr(x), cin, 0.2, 0, 1, low, low, dt)
            bare = lambda: call("pmi_convt4x4s2", ptr(g), cout, cout, ptr(wp), cin, ptr(d), cin, None, 0, None, 0, 0.2, 0, 1, low, low, dt)
            # <adjoint g, x> = <g, forward x> on the same operands (fp32 sums of 16-bit results)
            fwd(), bare()
            torch.cuda.synchronize()
            lhs, rhs = float((d.float() * x.float()).sum()), float((g.float() * z.float()).sum())
            for _ in range(a.warmup):
                fwd(), adj(), bare()
            torch.cuda.synchronize()
            tf, ta, tb = [], [], []
            for _ in range(a.rounds):
                tf.append(_timed(fwd, a.inner))
                ta.append(_timed(adj, a.inner))
                tb.append(_timed(bare, a.inner))
            fl = 2.0 * 16 * cin * cout * low * low
            mf, ma, mb = statistics.median(tf), statistics.median(ta), statistics.median(tb)
            emit(dict(tool="disc_probe", dtype=dtype, layer=f"conv{k}^T", cout=cout, cin=cin, low=low, convt_ms=round(ma, 4),
                      convt_min_ms=round(min(ta), 4), convt_bare_ms=round(mb, 4), igemm_fwd_ms=round(mf, 4), igemm_fwd_min_ms=round(min(tf), 4),
                      convt_over_fwd=round(ma / mf, 3), bare_over_fwd=round(mb / mf, 3), convt_tflops=round(fl / ma / 1e9, 1),
                      fwd_tflops=round(fl / mf / 1e9, 1), convt_peak_share=round(fl / ma / 1e-3 / PEAK, 4), adjoint_dot=lhs, forward_dot=rhs))
            del x, r, g, z, d, lin, wp
            torch.cuda.empty_cache()
        if a.size:
            m = SuperResolutionDiscriminator(num_feat=f, dtype=dtype).to(dev)
            img = torch.rand((1, 3, a.size, a.size), generator=torch.Generator().manual_seed(1)).to(dev)
            fn = lambda: m.loss_and_grad(img)
            for _ in range(2):
                fn()
            torch.cuda.synchronize()
            ts = [_timed(fn, 1) for _ in range(max(3, a.rounds // 2))]
            ms = statistics.median(ts)
            emit(dict(tool="disc_probe", dtype=dtype, shape="loss_and_grad", size=a.size, num_feat=f, ms=round(ms, 2), min_ms=round(min(ts), 2)))
            del m
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
