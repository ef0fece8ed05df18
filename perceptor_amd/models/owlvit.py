"""OWL-ViT -- drop-in for perceptor.models.OWLViT (perceptor/models/owlvit/owlvit.py:15-117): open-vocabulary detection, the class logits
of every 32 x 32 patch of a 768 x 768 image against a list of text queries, with the predicted box of every patch.

Call surface of the reference: ``encode_texts([[query, ...]]) -> OWLViTEncodings`` and ``forward(images, encodings) -> OWLViTPredictions``
(logits, boxes, scores, labels, texts).  Both towers and the heads run in perceptor_amd.engine.owlvit.OwlVitEngine.  ``logits`` is the
output of an autograd.Function over the engine, so a loss on it reaches the images; ``scores = sigmoid(max_q logits)`` and ``labels`` are
torch ops on that small tensor (``predictions.scores.mean().backward()`` works as in the reference's own test).  ``boxes`` carry NO
gradient: the reference's loss reads the logits only, and the box head runs forward only.

The texts go through ClipTokenizer at context 16, zero padded (what OwlViTProcessor's CLIPTokenizer gives: pad id 0 behind the end token).
A prompt longer than 16 tokens is a ValueError, as the reference raises; more than one inner list (a list of queries per image) is a
NotImplementedError: the reference's loss never makes one.  A tensor of token ids [Q, T <= 16] is accepted in place of the texts.

Not available here: the pretrained weights (no network).  ``weights="synthetic"`` gives deterministic offline weights; ``checkpoint=``
takes the state dict of transformers' OwlViTForObjectDetection (google/owlvit-base-patch32).
"""
from __future__ import annotations

from typing import List, Optional

import torch

from ..engine import owlvit as E
from ..utils.param_tree import ParamTree
from ..utils.record import FrozenRecord
from ..utils.synth import synth_state_dict


class OWLViTEncodings(torch.nn.Module):
    """texts: List[List[str]]; input_ids int64 [B Q, T] and attention_mask, the reference's ``batch_encoding``; queries [Q, D]: the
    prepared query vectors of the first image's list (the engine's operand; forward() repeats them over the batch as the reference
    repeats the ids)."""

    def __init__(self, texts, input_ids, queries=None):
        super().__init__()
        self.texts = texts
        self.batch_encoding = {"input_ids": input_ids, "attention_mask": (input_ids != 0).long()}
        self.queries = queries

    def to(self, device):
        self.batch_encoding = {k: v.to(device) for k, v in self.batch_encoding.items()}
        if self.queries is not None:
            self.queries = self.queries.to(device)
        return super().to(device)

    def repeat(self, repetitions):
        enc = OWLViTEncodings(self.texts, torch.cat([self.batch_encoding["input_ids"] for _ in range(repetitions)], dim=0), self.queries)
        return enc


class OWLViTPredictions(FrozenRecord):
    """logits [N, P, Q]; boxes [N, P, 4] (left, top, right, bottom) in pixels of the 768 x 768 input, no gradient; scores [N, P];
    labels [N, P] int64; texts."""
    _fields = ("logits", "boxes", "scores", "labels", "texts")

    def __repr__(self):
        return f"OWLViTPredictions(logits=<{tuple(self.logits.shape)}>, boxes=<{tuple(self.boxes.shape)}>, texts={self.texts!r})"


class _Logits(torch.autograd.Function):
    """forward / backward are the HIP engine's (cf. glide_clip._EncodeImages); returns (logits, pred_boxes), the boxes not differentiable"""

    @staticmethod
    def forward(ctx, images, queries, model):
        eng = model.engine
        out = eng.forward(images, queries, save=True)
        ctx.model, ctx.saved_state = model, eng.saved
        ctx.mark_non_differentiable(out["boxes"])
        return out["logits"], out["boxes"]

    @staticmethod
    def backward(ctx, grad_logits, _grad_boxes):
        eng = ctx.model.engine
        eng.saved = ctx.saved_state
        return eng.backward(grad_logits.float().contiguous() * eng.gscale), None, None


class OWLViT(torch.nn.Module):
    def __init__(self, *, weights="synthetic", checkpoint: Optional[str] = None, dtype="bf16", seed: int = 0, config: Optional[tuple] = None,
                 text_config: Optional[tuple] = None):
        """
        OWL-ViT zero-shot text-conditioned bounding box model

        Args:
            weights (str): "synthetic" for deterministic offline weights, or "google/owlvit-base-patch32" with checkpoint=
            checkpoint (str): a file holding the state dict of transformers' OwlViTForObjectDetection
            dtype (str): "bf16" (default) or "f16", the type the towers multiply in
            config / text_config: (image, patch, width, layers, heads, projection) and (context, vocab, width, layers, heads, projection)
        """
        super().__init__()
        if dtype not in ("bf16", "f16", "fp16"):
            raise ValueError(f"Invalid dtype: {dtype} (the HIP towers multiply in 'bf16' or 'f16')")
        self.cfg = tuple(config) if config is not None else E.OWLVIT_VISION_CONFIG
        self.text_cfg = tuple(text_config) if text_config is not None else E.OWLVIT_TEXT_CONFIG
        self.precision = "bf16" if dtype == "bf16" else "f16"
        shapes = E.owlvit_state_dict_shapes(self.cfg, self.text_cfg)
        if checkpoint is not None:
            sd = {k: v.float() for k, v in torch.load(checkpoint, map_location="cpu", weights_only=True).items() if not k.endswith("position_ids")}
            E.check_state_dict(sd, self.cfg, self.text_cfg)
        elif weights == "synthetic":
            sd = {k: v.reshape(shapes[k]) for k, v in synth_state_dict(shapes, seed).items()}      # (logit_scale is a scalar)
        else:
            raise RuntimeError(f"pretrained weights OWLViT/{weights} cannot be downloaded (no network): pass checkpoint= (a state-dict file) "
                               "or weights='synthetic'")
        self.weights = weights
        self.model = ParamTree(sd)             # the reference holds OwlViTForObjectDetection as self.model (owlvit.py:57-59)
        self.size = (self.cfg[0], self.cfg[0])
        self._engine: Optional[E.OwlVitEngine] = None
        self._tokenizer = None
        self.register_load_state_dict_post_hook(lambda module, incompatible: setattr(module, "_engine", None))

    @property
    def device(self):
        return next(iter(self.parameters())).device

    @property
    def engine(self) -> E.OwlVitEngine:
        if self.device.type != "cuda":
            raise RuntimeError("OWLViT needs a HIP device: call .to('cuda') first (perceptor_amd has no CPU fallback)")
        if self._engine is None:
            self._engine = E.OwlVitEngine(self.cfg, self.text_cfg, self.model.state_dict(), self.device, self.precision)
        return self._engine

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)

    def tokenize(self, texts: List[str], tokenizer=None) -> torch.Tensor:
        """-> int64 [Q, context], zero padded.  A prompt of more than ``context`` tokens (start and end included) is a ValueError."""
        if tokenizer is not None:
            self._tokenizer = tokenizer
        if self._tokenizer is None:
            from ..utils.tokenizer import ClipTokenizer
            self._tokenizer = ClipTokenizer()                 # (the BPE file: PERCEPTOR_AMD_BPE)
        ctx = self.text_cfg[0]
        for t in texts:
            if len(self._tokenizer.encode(t)) + 2 > ctx:
                raise ValueError("Failed to encode texts, they are probably too long")
        return self._tokenizer(list(texts), context_length=ctx, pad="zero")

    def encode_texts(self, texts) -> OWLViTEncodings:
        """texts: [[query, ...]] (one list: the same queries for every image), or a tensor of token ids [Q, T]."""
        if isinstance(texts, torch.Tensor):
            ids, texts = texts, [[f"query {i}" for i in range(texts.shape[0])]]
            if ids.ndim != 2 or ids.dtype != torch.int64 or ids.shape[1] > self.text_cfg[0]:
                raise ValueError(f"token ids must be int64 [Q, T <= {self.text_cfg[0]}]")
        else:
            if len(texts) == 0 or isinstance(texts[0], str):
                raise ValueError("texts must be a list of lists of queries: [[query, ...]]")
            if len(texts) != 1:
                raise NotImplementedError("one list of queries per image (ragged queries, query_mask) is not supported")
            ids = self.tokenize(texts[0])
        ids = ids.to(self.device)
        return OWLViTEncodings(texts, ids, self.engine.prepare_queries(ids))

    def forward(self, images, encodings: OWLViTEncodings) -> OWLViTPredictions:
        """images NCHW in [0, 1]; resized to ``size`` and normalised with the CLIP mean / std inside the engine."""
        if not images.is_cuda:
            raise RuntimeError("OWLViT runs on a HIP device only (no CPU fallback)")
        if encodings.queries is None:
            raise ValueError("encodings hold no prepared queries: make them with encode_texts")
        eng = self.engine
        queries = encodings.queries.to(self.device)
        if images.requires_grad and torch.is_grad_enabled():
            logits, pred = _Logits.apply(images, queries, self)
        else:
            out = eng.forward(images, queries)
            logits, pred = out["logits"], out["boxes"]
        mx = logits.max(dim=-1)
        cx, cy, w, h = pred.detach().unbind(-1)
        boxes = torch.stack([cx - 0.5 * w, cy - 0.5 * h, cx + 0.5 * w, cy + 0.5 * h], dim=-1)
        boxes = boxes * torch.tensor([self.size[1], self.size[0], self.size[1], self.size[0]], dtype=boxes.dtype, device=boxes.device)
        return OWLViTPredictions(logits=logits, boxes=boxes, scores=torch.sigmoid(mx.values), labels=mx.indices, texts=encodings.texts)
