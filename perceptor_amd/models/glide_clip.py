"""GLIDE CLIP -- drop-in for perceptor.models.GlideCLIP (perceptor/models/glide_clip/glide_clip.py:15-60): OpenAI's CLIP trained on
DIFFUSED 64x64 images and their timestep, so a guided sampler can score x_t directly instead of a denoised prediction.

Call surface of the reference: ``encode_texts(prompts)``, ``encode_images(diffused, ts)`` (unit rows), ``forward`` raising
NotImplementedError; plus ``cond_fn(prompts, grad_scale)`` of the model it wraps (glide_clip/model_creation.py:60-74).  The image tower
runs in perceptor_amd.engine.glide.GlideImageEngine (the ViT engine behind the fused GLIDE stem kernels), the text tower in
GlideTextEngine behind perceptor_amd.utils.tokenizer.ClipTokenizer (CLIP's BPE, ``[sot] + ids[:context - 2] + [eot]``, zero padded,
pooled at the prompt's own length: simple_tokenizer.py:105-112).

Not available here: the pretrained weights (no network).  ``weights="synthetic"`` gives deterministic offline weights; ``"openai"``
needs ``checkpoint_image=`` and ``checkpoint_text=``, the state dicts of OpenAI's clip_image_enc.pt / clip_text_enc.pt.
"""
from __future__ import annotations

from typing import Optional

import torch

from .._hip import call, ptr
from ..engine import glide
from ..utils.param_tree import ParamTree


def _unit_rows(emb):
    # the reference normalises twice, x / (|x| + 1e-12) then F.normalize (model_creation.py:58, glide_clip.py:52): the second divides a
    # row of norm |x| / (|x| + 1e-12) = 1 - 1e-12 / |x| by it, so one pmi_l2norm_rows gives the same row to 1e-12 relative
    out = torch.empty_like(emb)
    emb = emb.contiguous()
    call("pmi_l2norm_rows", ptr(emb), ptr(out), emb.shape[0], emb.shape[1], 1.0)
    return out


class _EncodeImages(torch.autograd.Function):
    """``loss(encode_images(x, ts)).backward()`` as in the reference: forward / backward are the HIP engine's (cf. open_clip._EncodeImages)."""

    @staticmethod
    def forward(ctx, images, ts, model):
        emb = model.engine.forward(images, ts, save=True)
        ctx.model = model
        ctx.saved_state = model.engine.saved
        ctx.save_for_backward(emb)
        return _unit_rows(emb)

    @staticmethod
    def backward(ctx, grad_out):
        (emb,) = ctx.saved_tensors
        eng = ctx.model.engine
        g = grad_out.float()
        nrm = emb.norm(dim=1, keepdim=True).clamp(min=1e-12)      # d/d emb of emb / |emb|  (tiny [N, D] tensors)
        e = emb / nrm
        g = (g - e * (e * g).sum(dim=1, keepdim=True)) / nrm
        eng.saved = ctx.saved_state
        return eng.backward(g * eng.gscale), None, None


class GlideCLIP(torch.nn.Module):
    def __init__(self, weights="openai", *, checkpoint_image: Optional[str] = None, checkpoint_text: Optional[str] = None,
                 precision: Optional[str] = None, config: Optional[tuple] = None, text_config: Optional[tuple] = None,
                 bpe_path: Optional[str] = None, seed: int = 0):
        """
        Args:
            weights (str): "openai", with checkpoint_image= / checkpoint_text=, or "synthetic" for deterministic offline weights
            precision (str): "bf16" (default) or "fp16"
            config: the image tower (image, patch, width, layers, heads, out_dim, n_timestep)
            text_config: the text tower (context, vocab, width, layers, heads, out_dim)
        """
        super().__init__()
        if weights not in ("openai", "synthetic"):
            raise ValueError(f"Invalid weights: {weights}")
        if precision not in (None, "bf16", "fp16", "f16"):
            raise ValueError(f"Invalid precision: {precision} (the HIP towers multiply in 'bf16' or 'fp16')")
        self.weights = weights
        self.cfg = tuple(config) if config is not None else glide.GLIDE_IMAGE_CONFIG
        self.text_cfg = tuple(text_config) if text_config is not None else glide.GLIDE_TEXT_CONFIG
        self.precision = {None: "bf16", "bf16": "bf16", "fp16": "f16", "f16": "f16"}[precision]
        self.logit_scale = glide.GLIDE_LOGIT_SCALE
        shapes, tshapes = glide.glide_image_state_dict_shapes(self.cfg), glide.glide_text_state_dict_shapes(self.text_cfg)
        if weights == "synthetic":
            sd, tsd = glide.glide_synth_state_dict(shapes, seed), glide.glide_synth_state_dict(tshapes, seed)
        else:
            if checkpoint_image is None or checkpoint_text is None:
                raise RuntimeError("pretrained weights GlideCLIP/openai cannot be downloaded (no network): "
                                   "pass checkpoint_image= and checkpoint_text= (state dicts) or weights='synthetic'")
            sd = {k: v.float() for k, v in torch.load(checkpoint_image, map_location="cpu", weights_only=True).items() if k in shapes}
            tsd = {k: v.float() for k, v in torch.load(checkpoint_text, map_location="cpu", weights_only=True).items() if k in tshapes}
            for have, want, what in ((sd, shapes, "image"), (tsd, tshapes, "text")):
                if set(have) != set(want) or any(tuple(have[k].shape) != tuple(want[k]) for k in want):
                    raise RuntimeError(f"checkpoint_{what} does not hold the {what} encoder's tensors")
        # the reference holds both encoders under self.model (glide_clip.py:25-37)
        self.model = ParamTree({**{"image_encoder." + k: v for k, v in sd.items()}, **{"text_encoder." + k: v for k, v in tsd.items()}})
        self._engine: Optional[glide.GlideImageEngine] = None
        self._text_engine: Optional[glide.GlideTextEngine] = None
        self._tokenizer, self._bpe_path = None, bpe_path
        self.register_load_state_dict_post_hook(lambda module, incompatible: (setattr(module, "_engine", None), setattr(module, "_text_engine", None)))
        self.output_dim = self.cfg[5]

    def _sub_state_dict(self, prefix):
        return {k[len(prefix):]: v for k, v in self.model.state_dict().items() if k.startswith(prefix)}

    @property
    def device(self):
        return next(self.model.parameters()).device

    @property
    def image_size(self):
        return (self.cfg[0], self.cfg[0])

    def _need_device(self):
        if self.device.type != "cuda":
            raise RuntimeError("GlideCLIP needs a HIP device: call .to('cuda') first (perceptor_amd has no CPU fallback)")

    @property
    def engine(self) -> glide.GlideImageEngine:
        self._need_device()
        if self._engine is None:
            self._engine = glide.GlideImageEngine(self.cfg, self._sub_state_dict("image_encoder."), self.device, self.precision)
        return self._engine

    @property
    def text(self) -> glide.GlideTextEngine:
        """The text tower's engine, packed on first use (prompts are encoded once per run)."""
        self._need_device()
        if self._text_engine is None:
            self._text_engine = glide.GlideTextEngine(self.text_cfg, self._sub_state_dict("text_encoder."), self.device, self.precision)
        return self._text_engine

    def _apply(self, fn, *a, **k):
        self._engine = None
        self._text_engine = None
        return super()._apply(fn, *a, **k)

    def tokenize(self, text_prompts, tokenizer=None):
        """simple_tokenizer.py:105-112: -> (ids int64 [N, context], zero padded; lengths int64 [N])."""
        if tokenizer is not None:
            self._tokenizer = tokenizer
        if self._tokenizer is None:
            from ..utils.tokenizer import ClipTokenizer
            self._tokenizer = ClipTokenizer(self._bpe_path)
        if isinstance(text_prompts, str):
            text_prompts = [text_prompts]
        ctx = self.text_cfg[0]
        ids = self._tokenizer(text_prompts, context_length=ctx, pad="zero")
        lengths = torch.tensor([min(len(self._tokenizer.encode(p)) + 2, ctx) for p in text_prompts], dtype=torch.int64)
        return ids, lengths

    def encode_tokens(self, token_ids: torch.Tensor, lengths: torch.Tensor):
        _, pooled = self.text.forward(token_ids, lengths=lengths)
        return _unit_rows(pooled)

    def encode_texts(self, text_prompts):
        return self.encode_tokens(*self.tokenize(text_prompts))

    def _check_ts(self, ts):
        if not ts.is_cuda and ts.numel() and (int(ts.min()) < 0 or int(ts.max()) >= self.cfg[6]):      # a device ts is not synchronised on:
            raise ValueError(f"ts out of range [0, {self.cfg[6]})")                                     # the stem kernel clamps it
        return ts.to(self.device)

    def encode_images(self, diffused, ts):
        """
        Args:
            diffused: [batch_size, 3, 64, 64] diffused images between 0 and 1
            ts: [batch_size] int64 timestep between 0 and 999 where 0 is without noise.
        """
        eng = self.engine
        ts = self._check_ts(ts)
        diffused = diffused.to(self.device)
        if diffused.requires_grad and torch.is_grad_enabled():
            return _EncodeImages.apply(diffused, ts, self)
        return _unit_rows(eng.forward(diffused, ts))

    def cond_fn(self, prompts, grad_scale: float):
        """model_creation.py:60-74: f(x, t), x in [-1, 1] -> grad_scale * d/dx [logit_scale * sum(z_t * z_i)].  One forward and one
        backward of the engine; the images enter the tower as (x + 1) / 2, whose adjoint is the factor 0.5."""
        z_t = self.encode_texts(prompts)

        def cond_fn(x, t, grad_scale=grad_scale, **kwargs):
            eng = self.engine
            x01 = (x.detach().to(self.device).float() + 1) * 0.5
            emb = eng.forward(x01, self._check_ts(t), save=True)
            nrm = emb.norm(dim=1, keepdim=True).clamp(min=1e-12)
            e = emb / nrm
            g = z_t.expand_as(e)
            d_emb = (g - e * (e * g).sum(dim=1, keepdim=True)) / nrm
            # the backward is linear in d_emb: logit_scale multiplies its result, not the 16-bit tensors inside it (times gscale = 65536 an
            # f16 backward would overflow)
            return eng.backward(d_emb * eng.gscale) * (0.5 * grad_scale * self.logit_scale)

        return cond_fn

    def forward(self, _):
        raise NotImplementedError
