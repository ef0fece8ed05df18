#!/usr/bin/env python3
"""models.GlideCLIP at the product config (64 / 4 / 768 / 12 / 12 / 512, 1000 timesteps), N = 8 and N = 64, bf16 and f16: device-event
timings after warm-up, the variants alternating in one process, medians and minima over --rounds rounds of --reps back-to-back calls.

  stem_fwd_fused   pmi_glide_embed_fwd                                            (1 launch)
  stem_fwd_seq     the sequence it replaces, from entry points that exist without it: a torch row lookup (index_select of the timestep
                   table) + pmi_patchify + ops.igemm + pmi_vit_assemble + pmi_layernorm_fwd                                   (5 launches)
                   -- VitEngine._embed itself, on a ViT engine that holds the same stem weights.  Its token 0 is the shared class
                   embedding, so it does NOT compute the GLIDE stem: placing the looked-up rows costs one more launch
  stem_fwd_seq6    the same + the in-place add that puts the rows into token 0                                                (6 launches)
  stem_bwd_fused   pmi_glide_embed_bwd                                            (1 launch)
  stem_bwd_seq     pmi_layernorm_bwd + ops.bgemm + pmi_unpatchify: VitEngine._embed_backward itself                           (3 launches)
  encode_fwd       GlideCLIP.encode_images, no gradient
  encode_fwd_bwd   encode_images on a leaf that requires grad + backward of <unit embedding, probe>
Bytes moved / time for the two fused kernels against the HBM ceiling (about 6.3 TB/s): forward reads the image and writes x0, x and
mean / rstd (the weight panel, positions and table rows are re-read from L2 and not counted); backward reads g and x0 and writes the
image gradient.

  python tools/glide_clip_probe.py [--batch 8 64] [--dtype bf16 f16] [--rounds 20] [--reps 10] [--out profiles/glide_clip_probe.txt]
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
    ap.add_argument("--batch", type=int, nargs="*", default=[8, 64])
    ap.add_argument("--dtype", nargs="*", default=["bf16", "f16"])
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--layers", type=int, default=None, help="blocks of the tower (default: the product's 12)")
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from perceptor_amd import models
    from perceptor_amd.engine import glide
    from perceptor_amd.engine.vit import VitEngine
    from perceptor_amd.utils.synth import seeded_noise
    if not torch.cuda.is_available():
        raise SystemExit("glide_clip_probe needs a HIP device")
    dev = torch.device("cuda:0")
    cfg = list(glide.GLIDE_IMAGE_CONFIG)
    if a.layers is not None:
        cfg[3] = a.layers
    cfg = tuple(cfg)
    res, patch, width, layers, heads, out, nt = cfg
    t = (res // patch) ** 2 + 1

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
        """{name: (median, min)} microseconds; one round times every variant once, in turn"""
        for _ in range(a.warmup):
            for fn in cases.values():
                fn()
        torch.cuda.synchronize()
        ts = {k: [] for k in cases}
        for _ in range(a.rounds):
            for k, fn in cases.items():
                ts[k].append(timed(fn, reps))
        return {k: (statistics.median(v), min(v)) for k, v in ts.items()}

    for dtype in a.dtype:
        model = models.GlideCLIP("synthetic", config=cfg, precision="fp16" if dtype == "f16" else "bf16").to(dev)
        eng = model.engine
        # the parent's stem: a ViT engine over the same stem weights (one block: only its stem runs here)
        vsd = glide.image_state_dict_to_vit({k[len("model.image_encoder."):]: v.cpu() for k, v in model.state_dict().items()
                                             if k.startswith("model.image_encoder.")})
        vcfg = (res, patch, width, 1, heads, out)
        vsd = {k: v for k, v in vsd.items() if not k.startswith("transformer.resblocks.") or k.startswith("transformer.resblocks.0.")}
        vsd["class_embedding"] = torch.zeros(width)
        vit = VitEngine(vcfg, vsd, dev, dtype, quick_gelu=False)
        vit.mean, vit.std = eng.mean / 255, eng.std / 255        # pmi_patchify normalises on the 0..1 scale: the same values
        for n in a.batch:
            img = (seeded_noise((n, 3, res, res), 31) * 0.25 + 0.5).clamp(0, 1).to(dev)
            ts = (torch.arange(n) * 37 % nt).to(dev)
            probe = torch.nn.functional.normalize(seeded_noise((n, out), 7)).to(dev)
            g32 = (seeded_noise((n * t, width), 8) * eng.gscale).to(dev)
            eng._ts = ts
            x0, x, mr = eng._embed(img)
            sv = dict(n=n, x0=x0, mr_pre=mr, in_hw=(res, res))
            x0v, _, mrv = vit._embed(img)
            svv = dict(n=n, x0=x0v, mr_pre=mrv, in_hw=(res, res))

            def seq5():
                rows = eng.w_t.index_select(0, ts)
                vit._embed(img)
                return rows

            def seq6():
                rows = eng.w_t.index_select(0, ts)
                x0_, _, _ = vit._embed(img)
                x0_[:, 0].add_(rows)

            stem = alternate({"stem_fwd_fused": lambda: eng._embed(img), "stem_fwd_seq": seq5, "stem_fwd_seq6": seq6,
                              "stem_bwd_fused": lambda: eng._embed_backward(g32, sv), "stem_bwd_seq": lambda: vit._embed_backward(g32, svv)}, a.reps)
            eng._ts = None

            def fwd_bwd():
                xi = img.clone().requires_grad_(True)
                (model.encode_images(xi, ts) * probe).sum().backward()

            with torch.no_grad():
                whole = alternate({"encode_fwd": lambda: model.encode_images(img, ts)}, 1)
            whole.update(alternate({"encode_fwd_bwd": fwd_bwd}, 1))
            m = n * t
            nbytes = dict(stem_fwd_fused=4 * (n * 3 * res * res + 2 * m * width + 2 * m), stem_bwd_fused=4 * (2 * m * width + 2 * m + n * 3 * res * res))
            row = dict(tool="glide_clip_probe", dtype=dtype, N=n, layers=layers, rounds=a.rounds, reps=a.reps, device=torch.cuda.get_device_name(0))
            for k, (med, lo) in {**stem, **whole}.items():
                row[k + "_us_median"], row[k + "_us_min"] = round(med, 2), round(lo, 2)
            for k, b in nbytes.items():
                row[k + "_mb"] = round(b / 1e6, 2)
                row[k + "_tbs"] = round(b / stem[k][0] / 1e6, 3)
                row[k + "_of_hbm"] = round(b / stem[k][0] / 1e6 / HBM_TBS, 3)
            row["fwd_fused_no_slower_than_seq"] = stem["stem_fwd_fused"][0] <= stem["stem_fwd_seq"][0]
            row["bwd_fused_no_slower_than_seq"] = stem["stem_bwd_fused"][0] <= stem["stem_bwd_seq"][0]
            emit(row)
        del model, eng, vit
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
