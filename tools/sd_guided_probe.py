#!/usr/bin/env python3
"""CLIP-guided StableDiffusion on the HIP path at the c4 shape (SD-v1, 512 x 512, batch 4, bf16 VAE): device-event times of the VAE decoder's
no-grad decode, training-mode forward and input-gradient backward, the tape's bytes and the peak memory, the backward's FLOP/s, one full
guided step, and the A/B of the Upsample2D adjoint (one-pass folded 4x4 stride-2 kernel vs 3x3 dX at the high resolution + 2x2 sum).

    python tools/sd_guided_probe.py [--reps 10] [--json out.json] [--no-step] [--aten]

--aten lists the torch kernels launched inside forward_train + backward (torch.profiler; there should be none)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def tape_bytes(tape):
    seen, tot = set(), 0

    def walk(o):
        nonlocal tot
        if torch.is_tensor(o):
            key = o.untyped_storage().data_ptr()
            if key not in seen:
                seen.add(key)
                tot += o.untyped_storage().nbytes()
        elif isinstance(o, (list, tuple)):
            for x in o:
                walk(x)
        elif isinstance(o, dict):
            for x in o.values():
                walk(x)
    walk(tape)
    return tot


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--reps", type=int, default=10)
    p.add_argument("--json", default=None)
    p.add_argument("--no-step", action="store_true")
    p.add_argument("--aten", action="store_true")
    a = p.parse_args()
    from perceptor_amd.engine import ops, sd
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    dev = torch.device("cuda:0")
    res = {}
    n, hw = 4, 64
    w = synth_state_dict(sd.vae_decoder_state_dict_shapes(sd.VAE_V1), 0)
    w = {k: v.to(dev) for k, v in w.items()}
    eng = sd.VaeDecoderEngine(sd.VAE_V1, w, dev, "bf16")
    z = seeded_noise((n, 4, hw, hw), 73).to(dev)
    d = (seeded_noise((n, 3, 8 * hw, 8 * hw), 91) * 1e-6).to(dev)

    # ---- A/B of the up-sampler adjoint: alternate the two, same process, same inputs -------------------------------------------------
    ab = []
    h = hw
    chans = list(reversed(sd.VAE_V1.block_out))
    for i in range(len(chans) - 1):
        k = f"decoder.up_blocks.{i}.upsamplers.0.conv"
        c = chans[i]
        g = torch.randn((n, 2 * h, 2 * h, c), generator=torch.Generator(dev).manual_seed(100 + i), device=dev).to(torch.bfloat16)
        f1 = lambda: eng._up_back(k, g, w)
        f0 = lambda: ops.upsample_nearest2_bwd(ops.igemm(g, ops.packed_dx(eng.w, k + "T", w[k + ".weight"], eng.dt, dev)), eng.dt)
        r1, r0 = f1(), f0()                                        # (packs both weight sets)
        diff = float((r1.float() - r0.float()).norm() / r0.float().norm())
        t1, t0 = [], []
        for _ in range(a.reps):
            t1.append(timed(f1, 3)); t0.append(timed(f0, 3))
        t1.sort(); t0.sort()
        fl_f = 2.0 * n * h * h * c * c * 16 / 1e9
        fl_c = 2.0 * n * 4 * h * h * c * c * 9 / 1e9
        row = dict(low_res=h, high_res=2 * h, channels=c, fused_ms=t1[len(t1) // 2], composed_ms=t0[len(t0) // 2],
                   fused_tflops=fl_f / t1[len(t1) // 2], composed_dx_tflops_alg=fl_c / t0[len(t0) // 2], rel_l2_between=diff)
        print("[ab]", json.dumps(row), flush=True)
        ab.append(row)
        h *= 2
    res["up_adjoint_ab"] = ab

    # ---- decoder phases ---------------------------------------------------------------------------------------------------------------
    for _ in range(2):
        eng.forward(z)
        _, tape = eng.forward_train(z)
        eng.backward(tape, d, w)
        del tape
    torch.cuda.synchronize()
    res["decode_ms"] = timed(lambda: eng.forward(z), a.reps)
    holder = {}

    def ft():
        holder["t"] = None
        holder["t"] = eng.forward_train(z)[1]
    res["forward_train_ms"] = timed(ft, a.reps)
    tape = holder["t"]
    res["backward_ms"] = timed(lambda: eng.backward(tape, d, w), a.reps)
    res["tape_bytes"] = tape_bytes(tape)
    del tape, holder["t"]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    _, tape = eng.forward_train(z)
    eng.backward(tape, d, w)
    torch.cuda.synchronize()
    res["peak_bytes_above_weights"] = torch.cuda.max_memory_allocated() - base
    del tape
    fwd_g, bwd_g = sd.vae_decoder_gflop(sd.VAE_V1, hw, hw)
    res["decoder_gflop_per_image"] = (fwd_g, bwd_g)
    res["backward_tflops"] = n * bwd_g / res["backward_ms"]
    res["forward_train_tflops"] = n * fwd_g / res["forward_train_ms"]
    print("[decoder]", json.dumps({k: v for k, v in res.items() if k != "up_adjoint_ab"}), flush=True)

    if a.aten:
        from torch.profiler import ProfilerActivity, profile
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            _, tape = eng.forward_train(z)
            eng.backward(tape, d, w)
            torch.cuda.synchronize()
        aten = [(ev.name, ev.self_device_time_total) for ev in prof.events() if ev.name.startswith("aten::") and ev.self_device_time_total > 0]
        res["aten_kernels_in_forward_train_backward"] = aten
        print("[aten]", len(aten), aten[:20], flush=True)
        del tape

    # ---- one CLIP-guided SD step: CFG UNet pair, decode forward_train, ViT-L/14 loss_and_grad, backward, guided, DDIM step -----------------
    if not a.no_step:
        from perceptor_amd import losses, models
        model = models.StableDiffusion(fp16=True).to(dev)
        clip = losses.OpenCLIP("ViT-L-14", "synthetic", dtype="bf16").to(dev)
        clip.add_encodings_(torch.nn.functional.normalize(seeded_noise((2, clip.model.output_dim), 7)).to(dev))
        ids = torch.full((2, 77), 49407, dtype=torch.int64)
        ids[:, 0] = 49406
        ids[1, 1:9] = torch.tensor([1125, 539, 320, 2368, 525, 320, 4558, 267])
        neutral, positive = model.conditioning(token_ids=ids[:1]), model.conditioning(token_ids=ids[1:])
        lat = seeded_noise((n, 4, hw, hw), 1234).to(dev)
        sched = model.schedule_indices(n_steps=50)
        deng = model._engine("decoder")
        vsd = model.vae.state_dict()
        ph = {}

        def ev():
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e

        def step(lat, i):
            fi, ti = sched[i]
            e = [ev()]
            un, pos = model.predictions_pair(lat, fi, neutral, positive)
            pred = un.classifier_free_guidance(pos, guidance_scale=7.0)
            e.append(ev())
            img, tape = deng.forward_train(pred.denoised_latents)
            e.append(ev())
            _, g_img = clip.loss_and_grad(img)
            e.append(ev())
            g_lat = deng.backward(tape, g_img, vsd)
            e.append(ev())
            out = pred.guided(g_lat).step(ti)
            e.append(ev())
            e[-1].synchronize()
            for nm, e0, e1 in zip(("unet_pair_cfg", "decode_forward_train", "clip_loss_and_grad", "decode_backward", "guided_step"), e[:-1], e[1:]):
                ph.setdefault(nm, []).append(e0.elapsed_time(e1))
            ph.setdefault("total", []).append(e[0].elapsed_time(e[-1]))
            return out
        for i in range(2):
            lat = step(lat, i)
        ph.clear()
        for i in range(2, 2 + a.reps):
            lat = step(lat, i)
        res["guided_step_ms"] = {k: sorted(v)[len(v) // 2] for k, v in ph.items()}
        res["guided_step_finite"] = bool(torch.isfinite(lat).all())
        print("[step]", json.dumps(res["guided_step_ms"]), res["guided_step_finite"], flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
