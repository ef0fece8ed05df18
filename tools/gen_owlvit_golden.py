"""Writes tests/golden/owlvit_weights.npz, owlvit_reference_a.npz and owlvit_reference_b.npz: inputs and outputs of the reference's own
OWL-ViT (perceptor/models/owlvit/modeling_owlvit.py, OwlViTForObjectDetection, the vendored file with its quirks) and of its own loss
(perceptor/losses/owlvit.py, OWLViT.forward), run unmodified on the CPU in float64 with eager attention.

The checkpoint is unreachable and the product model would make a large fixture, so two tiny models carry name-keyed synthetic weights
(perceptor_amd.utils.synth) quantised to k * 2^e, |k| <= 127: exact in bf16, f16 and fp32, and one byte per weight in the file.
  (a) vision (96, 32, 128, 2 layers, 2 heads of 64): P = 9, T = 10;   text (16, 64, 32, 1 layer, 1 head), projection 32
  (b) vision (128, 32, 128, 2, 2):                   P = 16, T = 17;  text (16, 64, 48, 1, 1),           projection 48
The class head maps to the TEXT width and is compared with the PROJECTED queries (modeling_owlvit.py:1249-1277), so the reference runs
only where the two agree (512 = 512 in the product): the toy text width is the projection.  Tensors whose name and shape agree in (a) and
(b) are the same tensor and are stored once (``w:``); (b)'s own are ``wb:``.
Inputs: N = 2 images (8-bit values / 255), Q = 3 hand-made queries of lengths 3, 6 and 16 (= the context) over a 64-id toy vocabulary
(start 62, end 63 = the largest id, zero padded), loss weights (1, 0.5, 2), top_k = 5.
Stored per configuration: the inputs, logits / pred_boxes / class_embeds / image_feats, the raw text embeddings, the last hidden state of
the vision tower, the loss and its gradient at that hidden state, d loss / d images and d scores.mean() / d images (scores =
sigmoid(max_q logits), the reference's own test).  (b)'s two image gradients are stored as float32 (one rounding; as float64 they would
not fit a file of 1 MiB).
Stand-ins cover imports only:
  * package shells for perceptor.models.owlvit / perceptor.losses and perceptor.transforms.resize.resize (the reference's own function);
  * ``perceptor.models.OWLViT`` is bound to a shell over the tiny model: forward(images, encodings) normalises with the CLIP mean / std as
    models/owlvit/owlvit.py:84-88 does (torchvision is absent), repeats the encodings per image (:93) and returns the model's logits.  The
    loss is the reference's own OWLViT.forward on it.
  * the vendored post_process needs transformers mixins that are gone: boxes, scores and labels past pred_boxes are pinned by the
    restatement only (tests/_owlvit_ref64.py).
No arithmetic of the reference is replaced.  Only numbers are written.  Deterministic.

    python tools/gen_owlvit_golden.py [--check | --search]
"""
from __future__ import annotations

import importlib
import io
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

import transformers                                                          # noqa: E402  (before the torchvision shell below exists)
from transformers.models.owlvit.configuration_owlvit import OwlViTConfig     # noqa: E402

from oracle import _refimport as R                                           # noqa: E402
from perceptor_amd.engine import owlvit as E                                 # noqa: E402
from perceptor_amd.utils.synth import seeded_noise, synth_tensor             # noqa: E402

SEED = 0
# the top-k set is discontinuous in the logits, so the images are chosen: ``--search`` walks the seeds 1..59 for (a) and 1..3999 for (b) and
# prints, per configuration, the five seeds with the largest ratio of the gap between the 5th and 6th largest logit of any (image, query)
# column to the bf16-emulated restatement's worst logit error (tests/_owlvit_ref64.py).  Of those five the seed with the widest gap is used
# (gap 0.49 = 18 x and 0.27 = 9.6 x).  tests/test_owlvit_cpu.py asserts gap > 8 x error in both dtypes
IMAGE_SEED = {"a": 29, "b": 3878}
CONFIGS = {"a": ((96, 32, 128, 2, 2, 32), (16, 64, 32, 1, 1, 32)), "b": ((128, 32, 128, 2, 2, 48), (16, 64, 48, 1, 1, 48))}
SOT, EOT = 62, 63
QUERIES = [[5], [17, 23, 41, 9], [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7]]
WEIGHTS = (1.0, 0.5, 2.0)
TOP_K = 5
MEAN = (0.48145466, 0.4578275, 0.40821073)
STD = (0.26862954, 0.26130258, 0.27577711)


def quantise(w: torch.Tensor):
    """-> (k int8, e int8) with w ~ k * 2^e, |k| <= 127"""
    a = float(w.abs().max())
    e = int(np.ceil(np.log2(a / 127.0))) if a > 0 else 0
    k = torch.round(w.double() / 2.0 ** e).clamp(-127, 127)
    return k.to(torch.int8).numpy(), np.int8(e)


def weights(shapes):
    out = {}
    for name, shp in shapes.items():
        k, e = quantise(synth_tensor(name, shp, SEED, rounding="none"))
        out[name] = (k.reshape(tuple(shp)), e)
    return out


def dequantise(k, e) -> torch.Tensor:
    return torch.as_tensor(np.asarray(k, dtype=np.float64) * 2.0 ** int(e), dtype=torch.float64)


def token_ids() -> torch.Tensor:
    ids = torch.zeros(len(QUERIES), 16, dtype=torch.int64)
    for i, q in enumerate(QUERIES):
        row = [SOT] + q + [EOT]
        ids[i, :len(row)] = torch.tensor(row)
    return ids


def _modules():
    R.install()
    base = os.path.join(R.REF_ROOT, "perceptor")
    R._shell("perceptor.models.owlvit", os.path.join(base, "models", "owlvit"))
    R._shell("perceptor.losses", os.path.join(base, "losses"))
    sys.modules["perceptor.transforms.resize"].resize = R.ref("transforms.resize.resize_right").resize
    return importlib.import_module("perceptor.models.owlvit.modeling_owlvit")


def build(mod, cfg, text_cfg, w):
    res, patch, width, layers, heads, proj = cfg
    ctx, vocab, tw, tl, th, tout = text_cfg
    config = OwlViTConfig(
        text_config=dict(vocab_size=vocab, hidden_size=tw, intermediate_size=4 * tw, num_hidden_layers=tl, num_attention_heads=th,
                         max_position_embeddings=ctx, hidden_act="quick_gelu", pad_token_id=0, bos_token_id=SOT, eos_token_id=EOT),
        vision_config=dict(hidden_size=width, intermediate_size=4 * width, num_hidden_layers=layers, num_attention_heads=heads,
                           image_size=res, patch_size=patch, hidden_act="quick_gelu"),
        projection_dim=proj)
    config._attn_implementation = "eager"
    model = mod.OwlViTForObjectDetection(config).double().eval().requires_grad_(False)
    have = {k for k in model.state_dict() if not k.endswith("position_ids")}
    assert have == set(w), sorted(have ^ set(w))
    missing = model.load_state_dict({k: dequantise(*v).reshape(model.state_dict()[k].shape) for k, v in w.items()}, strict=False)
    assert all(k.endswith("position_ids") for k in missing.missing_keys) and not missing.unexpected_keys, missing
    return model


def run(mod, name, w):
    cfg, text_cfg = CONFIGS[name]
    model = build(mod, cfg, text_cfg, w)
    res = cfg[0]
    ids = token_ids()
    img8 = images8(name, IMAGE_SEED[name])
    kept = {}
    model.owlvit.vision_model.encoder.register_forward_hook(lambda m, a, out: kept.__setitem__("hidden", out[0]))

    class Shell(torch.nn.Module):                                            # stands where models.OWLViT() stands (module doc)
        def __init__(self):
            super().__init__()
            self.model = model

        def forward(self, images, encodings):
            x = (images - torch.tensor(MEAN, dtype=images.dtype).view(1, 3, 1, 1)) / torch.tensor(STD, dtype=images.dtype).view(1, 3, 1, 1)
            rep = encodings.repeat(images.shape[0]).batch_encoding
            kept["out"] = self.model(pixel_values=x, input_ids=rep["input_ids"], attention_mask=rep["attention_mask"], return_dict=True)
            return types.SimpleNamespace(logits=kept["out"].logits)

    sys.modules["perceptor.models"].OWLViT = Shell
    losses = importlib.import_module("perceptor.losses.owlvit")
    enc_mod = importlib.import_module("perceptor.models.owlvit.owlvit")
    from transformers.tokenization_utils_base import BatchEncoding
    enc = enc_mod.OWLViTEncodings(texts=[["q0", "q1", "q2"]], batch_encoding=BatchEncoding({"input_ids": ids, "attention_mask": (ids != 0).long()}))
    loss_mod = losses.OWLViT()
    loss_mod.add_encodings_(enc, weights=list(WEIGHTS))
    # add_encodings_ sizes default weights by len(texts) = the number of inner lists; given explicitly they are per query
    images = (img8.double() / 255.0).requires_grad_(True)
    loss = loss_mod(images, top_k=TOP_K)
    out, hidden = kept["out"], kept["hidden"]
    g_img, g_hidden = torch.autograd.grad(loss, (images, hidden), retain_graph=True)
    scores = torch.sigmoid(out.logits.max(dim=-1).values)
    (g_scores,) = torch.autograd.grad(scores.mean(), images)
    A = {"cfg": np.array(cfg), "text_cfg": np.array(text_cfg), "images8": img8.numpy(), "ids": ids.numpy(), "weights": np.array(WEIGHTS),
         "top_k": np.array(TOP_K), "logits": out.logits.detach().numpy(), "pred_boxes": out.pred_boxes.detach().numpy(),
         "class_embeds": out.class_embeds.detach().numpy(), "image_feats": out.image_embeds.detach().numpy(),
         "text_embeds": out.text_embeds.detach().numpy()[0], "hidden": hidden.detach().numpy(), "loss": loss.detach().numpy(),
         "grad_hidden": g_hidden.numpy()}
    if name == "a":
        A["grad_images"], A["grad_scores_images"] = g_img.numpy(), g_scores.numpy()
    else:                                    # 2 x 786 KB as float64: stored as float32 (one rounding, 2^-24 relative per element)
        A["grad_images"], A["grad_scores_images"] = g_img.numpy().astype(np.float32), g_scores.numpy().astype(np.float32)
    return A


def generate():
    mod = _modules()
    wa, wb = (weights(E.owlvit_state_dict_shapes(*CONFIGS[n])) for n in "ab")
    W = {}
    for k, (q, e) in wa.items():
        W["w:" + k], W["e:" + k] = q, e
    for k, (q, e) in wb.items():
        if k not in wa or wa[k][0].shape != q.shape:
            W["wb:" + k], W["eb:" + k] = q, e
        else:
            assert np.array_equal(wa[k][0], q) and wa[k][1] == e
    return {"owlvit_weights.npz": W, "owlvit_reference_a.npz": run(mod, "a", wa), "owlvit_reference_b.npz": run(mod, "b", wb)}


def images8(name, seed):
    res = CONFIGS[name][0][0]
    return (seeded_noise((2, 3, res, res), seed) * 0.25 + 0.5).clamp(0, 1).mul(255).round().to(torch.uint8)


def search():
    """the seed choice above, reproduced: float64 and bf16-emulated restatement logits per seed (no reference needed)"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _owlvit_ref64 as O
    ids = token_ids()
    for name, seeds in (("a", range(1, 60)), ("b", range(1, 4000))):
        cfg, tcfg = CONFIGS[name]
        sd = {k: dequantise(*v) for k, v in weights(E.owlvit_state_dict_shapes(cfg, tcfg)).items()}
        exact, emu = O.OwlVit(sd, cfg, tcfg), O.OwlVit(sd, cfg, tcfg, emulate=torch.bfloat16)
        q, qe = exact.queries(ids), emu.queries(ids)
        best = []
        for seed in seeds:
            img = images8(name, seed).double() / 255
            lg = exact.class_head(exact.merge(exact.tower.forward(img)[1]["x_final"]), q)[0]
            gap = float(O.topk_gap(lg, TOP_K).min())
            if gap > 0.2:                                                    # (the emulated run only for candidates)
                err = float((emu.class_head(emu.merge(emu.tower.forward(img)[1]["x_final"]), qe)[0] - lg).abs().max())
                best.append((round(gap / err, 2), round(gap, 4), seed))
        print(name, "(gap / error, gap, seed):", sorted(best, reverse=True)[:5])


def to_bytes(arrays) -> bytes:
    buf = io.BytesIO()
    np.savez(buf, **arrays)
    return buf.getvalue()


if __name__ == "__main__":
    if "--search" in sys.argv:
        search()
        sys.exit(0)
    ok = True
    for fname, arrays in generate().items():
        path, data = os.path.join(GOLDEN, fname), to_bytes(arrays)
        assert len(data) <= 1 << 20, (path, len(data))
        if "--check" in sys.argv:
            same = os.path.exists(path) and open(path, "rb").read() == data
            print(f"{path}: {'reproduced bit for bit' if same else 'DIFFERS'}")
            ok &= same
        else:
            with open(path, "wb") as f:
                f.write(data)
            print(f"wrote {path} ({len(data)} bytes)")
    sys.exit(0 if ok else 1)
