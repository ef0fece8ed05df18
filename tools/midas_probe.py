"""Times the kernels of csrc/dpt.hip against the torch device-op sequence each replaces, models.MidasDepth forward and forward + backward at
N = 1 and 8 (dpt_large, synthetic weights, bf16), and prints the route every pmi_igemm of one forward + backward takes at product shape.

Method (measuring-on-mi355x): device events around `--inner` calls, a warm-up, `--rounds` alternating rounds per contender, medians with
their ranges.  These are reports, not gates: where a kernel loses to torch the table says so.

    python tools/midas_probe.py [--rounds 5] [--inner 20] [--batches 1 8] [--out profiles/midas_probe.txt]
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from perceptor_amd import models                                     # noqa: E402
from perceptor_amd._hip import call, ptr                             # noqa: E402
from perceptor_amd.engine import ops                                 # noqa: E402

DEV, DT, TD = "cuda:0", 1, torch.bfloat16


def _time(fn, inner):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / inner


def compare(name, ours, theirs, rounds, inner, nbytes=None):
    ours(), theirs()
    torch.cuda.synchronize()
    t = {"hip": [], "torch": []}
    for _ in range(rounds):                                          # alternating rounds
        t["hip"].append(_time(ours, inner))
        t["torch"].append(_time(theirs, inner))
    mh, mt = statistics.median(t["hip"]), statistics.median(t["torch"])
    bw = f"  {nbytes / mh / 1e6:7.0f} GB/s" if nbytes else ""
    verdict = "" if mh <= mt else "   LOSES to torch"
    return (f"{name:34s} hip {mh * 1e3:8.1f} us [{min(t['hip']) * 1e3:.1f} .. {max(t['hip']) * 1e3:.1f}]   torch {mt * 1e3:8.1f} us "
            f"[{min(t['torch']) * 1e3:.1f} .. {max(t['torch']) * 1e3:.1f}]   x{mt / mh:5.2f}{bw}{verdict}")


def kernels(n, rounds, inner):
    rows = []
    g = lambda *s: torch.randn(s, device=DEV).to(TD)
    e = lambda *s: torch.empty(s, device=DEV, dtype=TD)
    for (h, c) in ((24, 256), (96, 256), (192, 128)):                # fusion blocks and the head's up-sampling
        x, r, y = g(n, h, h, c), g(n, 2 * h, 2 * h, c), e(n, 2 * h, 2 * h, c)
        xc = x.permute(0, 3, 1, 2)                                     # channels-last view: torch's fast layout for this op
        rc = r.permute(0, 3, 1, 2)
        rows.append(compare(f"bilinear2_ac_fwd+add {h}^2 x {c}", lambda: call("pmi_bilinear2_ac_fwd", ptr(x), ptr(r), ptr(y), n, h, h, c, DT),
                            lambda: F.interpolate(xc, scale_factor=2, mode="bilinear", align_corners=True) + rc, rounds, inner,
                            nbytes=2 * (x.numel() + 2 * y.numel())))
        dx = e(n, h, h, c)
        xg = xc.detach().clone().requires_grad_(True)
        up = F.interpolate(xg, scale_factor=2, mode="bilinear", align_corners=True)
        rows.append(compare(f"bilinear2_ac_bwd {h}^2 x {c}", lambda: call("pmi_bilinear2_ac_bwd", ptr(r), ptr(dx), n, h, h, c, DT),
                            lambda: torch.autograd.grad(up, xg, rc, retain_graph=True), rounds, inner, nbytes=2 * (x.numel() + y.numel())))
    for k, c in ((4, 256), (2, 512)):
        x, y, b = g(n, 24, 24, k * k * c), e(n, 24 * k, 24 * k, c), torch.randn(c, device=DEV)
        rows.append(compare(f"depth_to_space k={k} C={c}", lambda: call("pmi_depth_to_space", ptr(x), ptr(b), ptr(y), n, 24, 24, c, k, DT),
                            lambda: (x.view(n, 24, 24, k, k, c).permute(0, 1, 3, 2, 4, 5).reshape(n, 24 * k, 24 * k, c) + b.to(TD)), rounds, inner,
                            nbytes=4 * x.numel()))
        rows.append(compare(f"space_to_depth k={k} C={c}", lambda: call("pmi_space_to_depth", ptr(y), ptr(x), n, 24, 24, c, k, DT),
                            lambda: y.view(n, 24, k, 24, k, c).permute(0, 1, 3, 2, 4, 5).reshape(n, 24, 24, k * k * c).contiguous(), rounds, inner,
                            nbytes=4 * x.numel()))
    t, w = 577, 1024
    tap = torch.randn(n, t, w, device=DEV)
    tok, cls = e(n * (t - 1), w), e(n, w)
    rows.append(compare("tap_split 577 x 1024", lambda: call("pmi_dpt_tap_split", ptr(tap), ptr(tok), ptr(cls), n, t, w, DT),
                        lambda: (tap[:, 1:].to(TD).contiguous(), tap[:, 0].to(TD).contiguous()), rounds, inner, nbytes=6 * tap.numel()))
    s = torch.empty(n, w, device=DEV)
    t3 = tok.view(n, t - 1, w)
    rows.append(compare("colsum 576 x 1024", lambda: call("pmi_dpt_colsum", ptr(tok), ptr(s), n, t - 1, w, DT), lambda: t3.float().sum(1), rounds, inner,
                        nbytes=2 * tok.numel()))
    dtok, dcls, out = torch.randn(n * (t - 1), w, device=DEV), torch.randn(n, w, device=DEV), torch.empty(n, t, w, device=DEV)
    rows.append(compare("tap_join 577 x 1024", lambda: call("pmi_dpt_tap_join", ptr(dtok), ptr(dcls), ptr(out), n, t, w),
                        lambda: torch.cat([dcls[:, None], dtok.view(n, t - 1, w)], 1), rounds, inner, nbytes=8 * out.numel()))
    o16 = e(n, t, w)
    rows.append(compare("tap_add 577 x 1024", lambda: call("pmi_dpt_tap_add", ptr(tap), ptr(out), ptr(tap), ptr(o16), tap.numel(), DT),
                        lambda: ((tap + out), (tap + out).to(TD)), rounds, inner, nbytes=14 * out.numel()))
    a, b, r, d = g(n, 96, 96, 256), g(n, 96, 96, 256).relu(), g(n, 96, 96, 256), e(n, 96, 96, 256)
    rows.append(compare("relu_bwd+add 96^2 x 256", lambda: call("pmi_dpt_relu_bwd", ptr(a), ptr(b), ptr(r), ptr(d), a.numel(), DT),
                        lambda: a * (b > 0) + r, rounds, inner, nbytes=8 * a.numel()))
    h, wv, bv, o = g(n * 384 * 384, 32).relu(), torch.randn(32, device=DEV), torch.randn(1, device=DEV), torch.empty(n * 384 * 384, device=DEV)
    rows.append(compare("head_fwd 384^2", lambda: call("pmi_dpt_head_fwd", ptr(h), ptr(wv), ptr(bv), ptr(o), o.numel(), DT),
                        lambda: -F.relu(h.float() @ wv + bv), rounds, inner, nbytes=2 * h.numel() + 4 * o.numel()))
    do, dh = torch.randn_like(o), torch.empty_like(h)
    rows.append(compare("head_bwd 384^2", lambda: call("pmi_dpt_head_bwd", ptr(do), ptr(o), ptr(h), ptr(wv), ptr(dh), o.numel(), 1.0, DT),
                        lambda: ((-do * (o < 0))[:, None] * wv[None] * (h > 0)).to(TD), rounds, inner, nbytes=4 * h.numel() + 8 * o.numel()))
    return rows


def model_times(batches, rounds, inner):
    rows = []
    m = models.MidasDepth().to(DEV)
    for n in batches:
        x = torch.rand(n, 3, 384, 384, device=DEV)
        xg = x.clone().requires_grad_(True)

        def fb():
            xg.grad = None
            m(xg).mean().backward()

        m(x), fb()
        torch.cuda.synchronize()
        tf = [_time(lambda: m(x), inner) for _ in range(rounds)]
        tb = [_time(fb, inner) for _ in range(rounds)]
        rows.append(f"MidasDepth dpt_large bf16 N={n}: forward {statistics.median(tf):8.2f} ms [{min(tf):.2f} .. {max(tf):.2f}]   "
                    f"forward + backward {statistics.median(tb):8.2f} ms [{min(tb):.2f} .. {max(tb):.2f}]")
    # route census at product shape (N = 1): every pmi_igemm of one forward + backward, the tower's GEMMs and the decoder's convolutions
    ops.GEMM_TRACE = []
    x = torch.rand(1, 3, 384, 384, device=DEV, requires_grad=True)
    m(x).mean().backward()
    torch.cuda.synchronize()
    trace, ops.GEMM_TRACE = ops.GEMM_TRACE, None
    seen = {}
    for desc, flops, e0, e1 in trace:
        ms = e0.elapsed_time(e1)
        k = seen.setdefault(desc, [0, 0.0, flops])
        k[0] += 1
        k[1] += ms
    rows.append("route census (forward + backward, N = 1; calls, total ms, TFLOP/s):")
    for desc, (cnt, ms, flops) in sorted(seen.items(), key=lambda kv: -kv[1][1]):
        rows.append(f"  {cnt:3d} x  {ms:8.3f} ms  {flops * cnt / ms / 1e9:7.1f}  {desc}")
    return rows


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "midas_probe.txt"))
    args = ap.parse_args()
    lines = [f"tools/midas_probe.py  rounds={args.rounds} inner={args.inner}  {torch.cuda.get_device_name(0)}", "kernels at N = 1:"]
    lines += kernels(1, args.rounds, args.inner)
    lines += model_times(args.batches, args.rounds, max(2, args.inner // 4))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))
