"""Writes tests/golden/glide_clip_image_reference.npz and tests/golden/glide_clip_text_reference.npz: inputs and outputs of the reference's
own GLIDE CLIP (perceptor/models/glide_clip/: encoders.ImageEncoder, encoders.TextEncoder, model_creation.CLIPModel and
simple_tokenizer.SimpleTokenizer), run unmodified on the CPU in float64.

The checkpoints are unreachable and the product towers would make large fixtures, so two tiny networks carry name-keyed synthetic weights
(perceptor_amd.engine.glide.glide_synth_state_dict, full-precision draws) rounded to fp16-representable values and stored as float16:
  image  (16, 4, 128, 2 blocks, 2 heads of 64, 32, 8 timesteps): 3 images, ts = [0, 3, 7]; the encoder's output, the unit embedding as
         GlideCLIP.encode_images forms it (glide_clip.py:46-57: image_embeddings(2 x - 1, ts), then F.normalize), the gradient of
         <unit embedding, probe> w.r.t. the images, and CLIPModel.cond_fn's gradient for the three prompts of the text fixture
  text   (context 12, vocab 64, width 64, 2 blocks, 2 heads of 32, 32): hand-made prompts of lengths 2, 7 and 12 (= context, cut from a
         longer one); ids and lengths as CLIPModel.encode_prompts gives them, the encoder's output and text_embeddings
  tokens SimpleTokenizer.padded_tokens_and_len at context 77 for the ASCII prompts the clip_tokenizer_merges fixture covers
Stand-ins cover imports, dtype names and the toy vocabulary only:
  * a package shell for perceptor.models.glide_clip and an identity ftfy.fix_text (what it returns for well-formed ASCII text);
  * the reference's LayerNorm casts its input with ``x.type(torch.float32)``: inside glide_clip/utils.py alone the name ``torch.float32``
    resolves to float64, so that the float64 run stays float64 (every other attribute of torch is passed through);
  * the toy text tower has 64 token ids, CLIP's BPE has 49408: a tokenizer whose encode() looks the hand-made prompts up and whose start /
    end ids are 62 / 63 stands in for the vocabulary; padded_tokens_and_len is the reference's own function.
No arithmetic of the reference is replaced.  Only numbers are written.  Deterministic.

    python tools/gen_glide_clip_golden.py [--check]
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
OUT_IMAGE = os.path.join(GOLDEN, "glide_clip_image_reference.npz")
OUT_TEXT = os.path.join(GOLDEN, "glide_clip_text_reference.npz")

from oracle import _refimport as R                                           # noqa: E402
from perceptor_amd.engine import glide                                       # noqa: E402
from perceptor_amd.utils.synth import seeded_noise                           # noqa: E402

SEED = 0
IMAGE_CFG = (16, 4, 128, 2, 2, 32, 8)
TEXT_CFG = (12, 64, 64, 2, 2, 32)
TS = [0, 3, 7]
LOGIT_SCALE, GRAD_SCALE = 100.0, 3.0
SOT, EOT = 62, 63
PROMPTS = {"": [], "five toy words here ok": [5, 17, 23, 41, 9], "a prompt longer than the context": [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7]}


def weights(shapes):
    """fp16-representable synthetic weights (float16 tensors)"""
    return {k: v.half() for k, v in glide.glide_synth_state_dict(shapes, SEED, rounding="none").items()}


def _modules():
    R.install()
    sys.modules.setdefault("ftfy", types.SimpleNamespace(fix_text=lambda t: t))
    base = os.path.join(R.REF_ROOT, "perceptor", "models", "glide_clip")
    R._shell("perceptor.models.glide_clip", base)
    utils = importlib.import_module("perceptor.models.glide_clip.utils")

    class _Torch64:                                                          # the dtype-name stand-in (module doc)
        float32 = torch.float64

        def __getattr__(self, name):
            return getattr(torch, name)

    utils.torch = _Torch64()
    enc = importlib.import_module("perceptor.models.glide_clip.encoders")
    mc = importlib.import_module("perceptor.models.glide_clip.model_creation")
    tok = importlib.import_module("perceptor.models.glide_clip.simple_tokenizer")
    return enc, mc, tok


def generate():
    enc, mc, tok = _modules()
    cpu = torch.device("cpu")
    res, patch, width, layers, heads, out, n_t = IMAGE_CFG
    image = enc.ImageEncoder(image_size=res, patch_size=patch, n_embd=out, n_head=heads, n_xf_blocks=layers, n_head_state=width // heads,
                             n_timestep=n_t, device=cpu)
    ctx, vocab, twidth, tlayers, theads, tout = TEXT_CFG
    text = enc.TextEncoder(n_bpe_vocab=vocab, max_text_len=ctx, n_embd=tout, n_head=theads, n_xf_blocks=tlayers, n_head_state=twidth // theads,
                           device=cpu)
    wi, wt = weights(glide.glide_image_state_dict_shapes(IMAGE_CFG)), weights(glide.glide_text_state_dict_shapes(TEXT_CFG))
    assert list(wi) == list(image.state_dict()) and list(wt) == list(text.state_dict()), "state-dict names or their order differ from the reference's"
    image.double().load_state_dict({k: v.double() for k, v in wi.items()})
    text.double().load_state_dict({k: v.double() for k, v in wt.items()})

    class ToyTokenizer:                                                      # the vocabulary stand-in (module doc)
        start_token, end_token = SOT, EOT
        encode = staticmethod(lambda prompt: list(PROMPTS[prompt]))
        padded_tokens_and_len = tok.SimpleTokenizer.padded_tokens_and_len

    clip = mc.CLIPModel(config={}, text_encoder=text, image_encoder=image, logit_scale=torch.tensor(np.log(LOGIT_SCALE), dtype=torch.float64),
                        device=cpu, tokenizer=ToyTokenizer()).eval().requires_grad_(False)
    prompts = list(PROMPTS)
    # ---- text
    ids, lens = clip.encode_prompts(prompts)
    with torch.no_grad():
        z_text, z_t = text(ids, lens), clip.text_embeddings(prompts)
    T = {"cfg": np.array(TEXT_CFG), "ids": ids.numpy(), "lengths": lens.numpy(), "z": z_text.numpy(), "unit": z_t.numpy()}
    T.update({"w:" + k: v.numpy() for k, v in wt.items()})
    # ---- the real tokenizer at the product context
    from oracle.gen_golden import TOKENIZER_PROMPTS
    tk = tok.SimpleTokenizer()
    pairs = [tk.padded_tokens_and_len(tk.encode(p), 77) for p in TOKENIZER_PROMPTS]
    T["bpe_ids"], T["bpe_lengths"] = np.array([p[0] for p in pairs], dtype=np.int64), np.array([p[1] for p in pairs], dtype=np.int64)
    # ---- image
    x = (seeded_noise((len(TS), 3, res, res), 4321) * 0.25 + 0.5).clamp(0, 1)
    ts = torch.tensor(TS)
    probe = torch.nn.functional.normalize(seeded_noise((len(TS), out), 99)).double()
    xv = x.double().requires_grad_(True)
    z = image((xv.mul(2).sub(1) + 1) * 127.5, ts)                             # what image_embeddings hands the encoder
    unit = torch.nn.functional.normalize(clip.image_embeddings(xv.mul(2).sub(1), ts))
    (grad,) = torch.autograd.grad((unit * probe).sum(), xv)
    cond = clip.cond_fn(prompts, GRAD_SCALE)(x.double().mul(2).sub(1), ts)
    I = {"cfg": np.array(IMAGE_CFG), "images": x.numpy(), "ts": ts.numpy(), "probe": probe.numpy(), "z": z.detach().numpy(), "unit": unit.detach().numpy(),
         "grad": grad.numpy(), "cond_grad": cond.numpy(), "z_t": z_t.numpy(), "logit_scale": np.array(LOGIT_SCALE), "grad_scale": np.array(GRAD_SCALE)}
    I.update({"w:" + k: v.numpy() for k, v in wi.items()})
    return I, T


def to_bytes(arrays) -> bytes:
    buf = io.BytesIO()
    np.savez(buf, **arrays)
    return buf.getvalue()


if __name__ == "__main__":
    ok = True
    for path, arrays in zip((OUT_IMAGE, OUT_TEXT), generate()):
        data = to_bytes(arrays)
        assert len(data) <= 1_000_000, (path, len(data))
        if "--check" in sys.argv:
            same = open(path, "rb").read() == data
            print(f"{path}: {'reproduced bit for bit' if same else 'DIFFERS'}")
            ok &= same
        else:
            with open(path, "wb") as f:
                f.write(data)
            print(f"wrote {path} ({len(data)} bytes)")
    sys.exit(0 if ok else 1)
