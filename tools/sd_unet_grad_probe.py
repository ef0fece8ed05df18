#!/usr/bin/env python3
"""The SD UNet's latent gradient on the HIP path: per attention shape of SD-v1 at 64 x 64 latents the flash backward (pmi_attn_flash_bwd, P
recomputed from lse) against the kept-P backward (ops.attention_backward / cross_attention_backward), same process, alternating, median of
reps x 3 device-event times, with the bytes each route keeps between forward and backward; then the c4 shape end to end (SD-v1, 64 x 64
latents, 8 samples, f16): forward, forward_train, backward, tape bytes, peak memory above the weights, algorithmic TFLOP/s.

    python tools/sd_unet_grad_probe.py [--reps 10] [--batch 8] [--json out.json] [--no-e2e]
    python tools/sd_unet_grad_probe.py --ctx [--json profiles/sd_unet_ctx_grad_probe.json]

--ctx: the gradient to the prompt encodings instead.  Per cross-attention shape the joint launch of pmi_attn_flash_bwd_kv (dQ + the key
role split into S query chunks + the reduce launch) against the same entry point with S forced to 1 (the unsplit key role,
pmi_set_option 14) and against the dq_only launch, alternating, three rounds, medians and the spread of the rounds; then the c4 shape end
to end: backward with cond_grad=False and cond_grad=True, alternating, and the peak memory of each.

Backward FLOP count: every convolution / linear dX costs its forward's multiply-adds; an attention's backward forms four T x Tk x C products
(dP, dQ, dK, dV) plus the recomputed S where the forward formed two (cross-attention: dP, dQ and S); the up-samplers' folded adjoints cost
16 / 36 of their forward.  Stated as 1.0 x unet_gflop + one more pair of attention products: a lower bound used for the TFLOP/s figure."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.sd_guided_probe import tape_bytes, timed          # noqa: E402


def nbytes(*ts):
    return sum(t.untyped_storage().nbytes() for t in ts)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--batch", type=int, default=8)
    p.add_argument("--json", default=None)
    p.add_argument("--no-e2e", action="store_true")
    p.add_argument("--ctx", action="store_true")
    a = p.parse_args()
    if a.ctx:
        return ctx_main(a)
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops, sd
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    dev = torch.device("cuda:0")
    dt, tdt, heads, n = _hip.DT_F16, torch.float16, 8, a.batch
    res = {"attention": []}
    med3 = lambda f: sorted(timed(f, a.reps) for _ in range(3))[1]
    for t, d in ((4096, 40), (1024, 80), (256, 160), (64, 160)):
        c = heads * d
        qkv = seeded_noise((n, t, 3 * c), 3).to(tdt).to(dev)
        q = seeded_noise((n, t, c), 4).to(tdt).to(dev)
        kv = seeded_noise((n, 77, 2 * c), 5).to(tdt).to(dev)
        do = seeded_noise((n, t, c), 6).to(tdt).to(dev)
        for kind in ("self", "cross"):
            if kind == "self":
                _, sf = ops.flash_attention_train(qkv, qkv[..., c:], qkv[..., 2 * c:], heads, d, dt)
                _, pm = ops.attention_train(qkv, heads, dt)
                ff = lambda: ops.flash_attention_backward(sf, do, heads, d, dt)
                fp = lambda: ops.attention_backward(qkv, pm, do, heads, dt)
            else:
                _, sf = ops.flash_attention_train(q, kv, kv[..., c:], heads, d, dt)
                _, pm = ops.cross_attention_train(q, kv, heads, dt)
                ff = lambda: ops.flash_attention_backward(sf, do, heads, d, dt, dq_only=True)
                fp = lambda: ops.cross_attention_backward(kv, pm, do, heads, dt)
            ff(); fp()
            tf, tp = [], []
            for _ in range(3):                                   # alternating
                tf.append(timed(ff, a.reps)); tp.append(timed(fp, a.reps))
            row = {"kind": kind, "T": t, "Tk": t if kind == "self" else 77, "d": d, "batch": n, "flash_ms": sorted(tf)[1], "kept_p_ms": sorted(tp)[1],
                   "flash_kept_MB": nbytes(sf[3], sf[4], sf[5]) / 2 ** 20, "kept_p_kept_MB": nbytes(pm) / 2 ** 20}
            print(json.dumps(row), flush=True)
            res["attention"].append(row)
            del sf, pm
        torch.cuda.empty_cache()
    if not a.no_e2e:
        w = synth_state_dict(sd.unet_state_dict_shapes(sd.SD_V1), 0)
        eng = sd.SdUnetEngine(sd.SD_V1, w, dev, "f16")
        x = seeded_noise((n, 4, 64, 64), 71).to(dev)
        ts = torch.full((n,), 500.0, device=dev)
        ctx = seeded_noise((n, 77, 768), 72).to(dev)
        cot = seeded_noise((n, 4, 64, 64), 93).to(dev)
        eng.forward(x, ts, ctx)
        _, tape = eng.forward_train(x, ts, ctx)
        eng.backward(tape, cot, w)                               # packs the transposed weights
        del tape
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        _, tape = eng.forward_train(x, ts, ctx)
        eng.backward(tape, cot, w)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        tb = tape_bytes(tape)
        gf = sd.unet_gflop(sd.SD_V1, 64, 64) * n
        e2e = {"batch": n, "forward_ms": med3(lambda: eng.forward(x, ts, ctx)), "forward_train_ms": med3(lambda: eng.forward_train(x, ts, ctx)),
               "backward_ms": med3(lambda: eng.backward(tape, cot, w)), "tape_MB": tb / 2 ** 20, "peak_above_weights_MB": peak / 2 ** 20, "fwd_gflop": gf}
        e2e["forward_tflops"] = gf / e2e["forward_ms"]
        e2e["backward_tflops_lower_bound"] = gf / e2e["backward_ms"]
        eng.flash_backward = False
        del tape
        _, tape = eng.forward_train(x, ts, ctx)
        e2e["kept_p_tape_MB"] = tape_bytes(tape) / 2 ** 20
        e2e["kept_p_backward_ms"] = med3(lambda: eng.backward(tape, cot, w))
        print(json.dumps(e2e), flush=True)
        res["c4"] = e2e
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


def ctx_main(a):
    from perceptor_amd import _hip
    from perceptor_amd.engine import ops, sd
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    dev = torch.device("cuda:0")
    dt, tdt, heads, n = _hip.DT_F16, torch.float16, 8, a.batch
    lib = _hip.lib()
    res = {"cross_attention": []}
    for t, d in ((4096, 40), (1024, 80), (256, 160), (64, 160)):
        c = heads * d
        q = seeded_noise((n, t, c), 4).to(tdt).to(dev)
        kv = seeded_noise((n, 77, 2 * c), 5).to(tdt).to(dev)
        do = seeded_noise((n, t, c), 6).to(tdt).to(dev)
        _, sf = ops.flash_attention_train(q, kv, kv[..., c:], heads, d, dt)
        s_auto = lib.pmi_attn_flash_bwd_kv_chunks(n, t, 77, heads, d)
        f_dq = lambda: ops.flash_attention_backward(sf, do, heads, d, dt, dq_only=True)
        f_kv = lambda: ops.flash_attention_backward(sf, do, heads, d, dt)
        f_dq(); f_kv()
        rounds = {"dq_only": [], "split": [], "unsplit": []}
        for _ in range(3):                                       # alternating
            rounds["dq_only"].append(timed(f_dq, a.reps))
            rounds["split"].append(timed(f_kv, a.reps))
            lib.pmi_set_option(14, 1)
            f_kv()
            rounds["unsplit"].append(timed(f_kv, a.reps))
            lib.pmi_set_option(14, 0)
        row = {"T": t, "Tk": 77, "d": d, "batch": n, "S": s_auto, "workspace_MB": lib.pmi_attn_flash_bwd_kv_workspace(n, t, 77, heads, d) / 1024,
               "dq_only_workspace_MB": lib.pmi_attn_flash_bwd_workspace(n, t, 77, heads, d, 1) / 1024}
        for k, v in rounds.items():
            row[k + "_ms"] = sorted(v)[1]
            row[k + "_rounds_ms"] = v
        print(json.dumps(row), flush=True)
        res["cross_attention"].append(row)
        del sf
        torch.cuda.empty_cache()
    if not a.no_e2e:
        w = synth_state_dict(sd.unet_state_dict_shapes(sd.SD_V1), 0)
        eng = sd.SdUnetEngine(sd.SD_V1, w, dev, "f16")
        x = seeded_noise((n, 4, 64, 64), 71).to(dev)
        ts = torch.full((n,), 500.0, device=dev)
        ctx = seeded_noise((n, 77, 768), 72).to(dev)
        cot = seeded_noise((n, 4, 64, 64), 93).to(dev)
        _, tape = eng.forward_train(x, ts, ctx)
        eng.backward(tape, cot, w, cond_grad=True)               # packs the transposed weights
        del tape
        e2e = {"batch": n}
        for tag, cg in (("latents", False), ("latents_and_context", True)):
            torch.cuda.synchronize(); torch.cuda.empty_cache()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            _, tape = eng.forward_train(x, ts, ctx)
            eng.backward(tape, cot, w, cond_grad=cg)
            torch.cuda.synchronize()
            e2e[tag + "_peak_above_weights_MB"] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            del tape
        e2e["context_weights_MB"] = sum(v.numel() * 4 for k, v in eng.w.items() if k.endswith(".kv2T")) / 2 ** 20
        _, tape = eng.forward_train(x, ts, ctx)
        r0, r1 = [], []
        for _ in range(3):                                       # alternating
            r0.append(timed(lambda: eng.backward(tape, cot, w), a.reps))
            r1.append(timed(lambda: eng.backward(tape, cot, w, cond_grad=True), a.reps))
        e2e.update({"backward_ms": sorted(r0)[1], "backward_rounds_ms": r0, "backward_cond_grad_ms": sorted(r1)[1], "backward_cond_grad_rounds_ms": r1,
                    "forward_train_ms": timed(lambda: eng.forward_train(x, ts, ctx), a.reps)})
        print(json.dumps(e2e), flush=True)
        res["c4"] = e2e
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
