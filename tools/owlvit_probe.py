#!/usr/bin/env python3
"""losses.OWLViT at the product config (768 / 32 / 768 / 12 / 12 / 512, text 16 / 49408 / 512 / 12 / 8 / 512), synthetic weights, Q = 3
queries, N = 1 and 8: device-event timings after warm-up, the variants alternating in one process, medians and minima over --rounds rounds
of --reps back-to-back calls.

  merge_fwd        pmi_owl_merge_ln_fwd (1 launch)            vs merge_fwd_torch: layer_norm, slice * slice, layer_norm, cast (torch device ops)
  merge_bwd        pmi_owl_merge_ln_bwd (2 launches)          vs merge_bwd_torch: torch.autograd.grad through merge_fwd_torch's graph
  class_fwd        pmi_owl_class_logits_fwd                   vs class_fwd_torch: norm, divide, matmul with q^T, elu + 1, add, multiply
  class_bwd        pmi_owl_class_logits_bwd                   vs class_bwd_torch: torch.autograd.grad through class_fwd_torch's graph + cast
  topk             pmi_owl_topk_loss (loss partials + dlogits) vs topk_torch: log_softmax, topk, mean, weighted sum and its autograd.grad
  box_out          pmi_owl_box_out                            vs box_out_torch: matmul with w2^T, + bias, sigmoid
  loss_and_grad    the whole fused path; tower = VitEngine.forward(save=True, features=True) + backward_tokens alone
Bytes moved / time against the HBM ceiling (about 6.3 TB/s) for the kernels: inputs read once and outputs written once (weights, gains and
the query block are re-read from L2 and not counted).

  python tools/owlvit_probe.py [--batch 1 8] [--dtype bf16] [--rounds 20] [--reps 10] [--out profiles/owlvit_probe.txt]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_TBS = 6.3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="*", default=[1, 8])
    ap.add_argument("--dtype", nargs="*", default=["bf16"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    import torch.nn.functional as F
    from perceptor_amd import _hip, losses
    if not torch.cuda.is_available():
        raise SystemExit("owlvit_probe needs a HIP device")
    dev = torch.device("cuda:0")

    def emit(row):
        print(json.dumps(row), flush=True)
        if a.out:
            with open(a.out, "a") as f:
                f.write(json.dumps(row) + "\n")

    def timed(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps                 # microseconds per call

    def alternate(cases, reps):
        for _ in range(a.warmup):
            for fn in cases.values():
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in cases}
        for _ in range(a.rounds):
            for k, fn in cases.items():
                ts[k].append(timed(fn, reps))
        return {k: (statistics.median(v), min(v)) for k, v in ts.items()}

    ids = torch.zeros(3, 16, dtype=torch.int64)
    for i, body in enumerate(([320, 1125], [320, 1929, 539, 320, 2368], list(range(1000, 1014)))):
        row = [49406] + body + [49407]
        ids[i, :len(row)] = torch.tensor(row)
    for dtype in a.dtype:
        loss = losses.OWLViT(dtype=dtype).to(dev)
        loss.add_encodings_(loss.model.encode_texts(ids), weights=[1.0, 0.5, 2.0])
        eng = loss.model.engine
        tdt = _hip.TORCH_DTYPE[eng.dt]
        q = loss.encodings.queries
        nq, d = q.shape
        g1, b1 = eng.vit.ln_post
        g2, b2 = eng.ln
        w2, bb2 = eng.box2
        for n in a.batch:
            img = torch.rand(n, 3, 768, 768, generator=torch.Generator().manual_seed(1)).to(dev)
            with torch.no_grad():
                _, hidden, _ = eng.vit.forward(img, features=True)
                hidden = hidden.contiguous().clone()
                _, t, w = hidden.shape
                p, m = t - 1, n * (t - 1)
                f32o, f16o, mr1, mr2 = eng.merge(hidden)
                logits, ce, g = eng.class_logits(f16o, q)
                h1 = torch.randn(m, w, device=dev).to(tdt)
                bias = eng.box_bias(24)
                dfe = torch.randn(m, w, device=dev)
                dl = torch.randn(m, nq, device=dev) * 0.01
                wts = loss.weights.data
                lg3 = logits.view(n, p, nq).contiguous()
            boxes = torch.empty(m, 4, device=dev)

            def merge_torch(x):
                y = F.layer_norm(x, (w,), g1, b1, 1e-5)
                f = F.layer_norm(y[:, 1:] * y[:, :1], (w,), g2, b2, 1e-5)
                return f, f.to(tdt)

            hg = hidden.clone().requires_grad_(True)
            with torch.enable_grad():
                fg, _ = merge_torch(hg)

            def class_torch(gg):
                e = gg[:, :d]
                eh = e / (torch.linalg.norm(e, dim=-1, keepdim=True) + 1e-6)
                return (eh @ q.t() + gg[:, d:d + 1]) * (F.elu(gg[:, d + 1:d + 2]) + 1), eh

            gg = g.clone().requires_grad_(True)
            with torch.enable_grad():
                lgg, _ = class_torch(gg)

            def topk_torch():
                x = lg3.clone().requires_grad_(True)
                with torch.enable_grad():
                    v = -(x.log_softmax(dim=1).topk(5, dim=1).values.mean(dim=(0, 1)) * wts).sum() * 0.01
                return v, torch.autograd.grad(v, x)[0]

            with torch.no_grad():
                cases = {
                    "merge_fwd": lambda: eng.merge(hidden), "merge_fwd_torch": lambda: merge_torch(hidden),
                    "merge_bwd": lambda: eng.merge_backward(dfe, hidden, mr1, mr2),
                    "merge_bwd_torch": lambda: torch.autograd.grad(fg, hg, dfe.view_as(fg), retain_graph=True),
                    "class_fwd": lambda: _hip.call("pmi_owl_class_logits_fwd", _hip.ptr(g), g.shape[1], _hip.ptr(q), _hip.ptr(logits), _hip.ptr(ce), m, d, nq),
                    "class_fwd_torch": lambda: class_torch(g),
                    "class_bwd": lambda: _hip.call("pmi_owl_class_logits_bwd", _hip.ptr(dl), _hip.ptr(g), g.shape[1], _hip.ptr(q), _hip.ptr(gg16), m, d, nq, eng.dt),
                    "class_bwd_torch": lambda: torch.autograd.grad(lgg, gg, dl, retain_graph=True)[0].to(tdt),
                    "topk": lambda: eng.topk_loss(lg3, wts, 5), "topk_torch": topk_torch,
                    "box_out": lambda: _hip.call("pmi_owl_box_out", _hip.ptr(h1), w, _hip.ptr(w2), _hip.ptr(bb2), _hip.ptr(bias), _hip.ptr(boxes), m, p, w, eng.dt),
                    "box_out_torch": lambda: torch.sigmoid(h1.float() @ w2.t() + bb2 + bias.repeat(n, 1)),
                }
                gg16 = torch.empty(g.shape, dtype=tdt, device=dev)
            kern = alternate(cases, a.reps)

            def tower():
                eng.vit.forward(img, save=True, features=True)
                eng.vit.backward_tokens(dfe_h)

            dfe_h = torch.randn(n, t, w, device=dev) * 1e-3
            whole = alternate({"loss_and_grad": lambda: loss.loss_and_grad(img), "tower": tower}, 1)
            nbytes = dict(merge_fwd=4 * n * t * w + 6 * m * w, merge_bwd=4 * (m * w + 2 * n * t * w), class_fwd=4 * (m * g.shape[1] + m * d + m * nq),
                          class_bwd=4 * m * g.shape[1] + 2 * m * g.shape[1], topk=4 * 3 * m * nq, box_out=2 * m * w + 16 * m)
            row = dict(tool="owlvit_probe", dtype=dtype, N=n, Q=nq, rounds=a.rounds, reps=a.reps, device=torch.cuda.get_device_name(0))
            for k, (med, lo) in {**kern, **whole}.items():
                row[k + "_us_median"], row[k + "_us_min"] = round(med, 2), round(lo, 2)
            for k, b in nbytes.items():
                row[k + "_mb"] = round(b / 1e6, 3)
                row[k + "_of_hbm"] = round(b / kern[k][0] / 1e6 / HBM_TBS, 4)
                row[k + "_no_slower_than_torch"] = kern[k][0] <= kern[k + "_torch"][0]
            row["tower_share_of_loss_and_grad"] = round(whole["tower"][0] / whole["loss_and_grad"][0], 3)
            emit(row)
        del loss, eng
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
