"""CPU: models.GlideCLIP's float64 restatement (tests/_glide_ref64.py) against the reference's own GLIDE CLIP, its host logic, and
seeded defects against the gates of tests/test_gpu_glide_clip.py.

1. The restatement reproduces tests/golden/glide_clip_image_reference.npz and glide_clip_text_reference.npz
   (tools/gen_glide_clip_golden.py: the reference's ImageEncoder / TextEncoder / CLIPModel in float64 over tiny networks): encoder
   outputs, unit embeddings, the image gradient of the fixed probe and CLIPModel.cond_fn's gradient, at 1e-9 relative (float64
   round-off; measured: the [bound] lines this module prints, all below 1e-13).
2. The key maps of engine/glide.py round-trip through the restatement's inverses; shapes and defaults are the reference config's.
3. The tokenizer's zero-padded ids and lengths equal the reference's padded_tokens_and_len.
4. Header, _hip.py and the built library agree on the two stem entry points.
5. Constructor and shape errors.
6. Seeded defects (_glide_ref64.DEFECTS) each exceed twice a gate the GPU test uses.
"""
import ctypes as C
import os
import re

import pytest
import torch

import _glide_ref64 as G
import _vit_ref64 as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TD = {"bf16": torch.bfloat16, "f16": torch.float16}
GSCALE = {"bf16": 1.0, "f16": 65536.0}


def _weights(g):
    return {k[2:]: v.float() for k, v in g.items() if k.startswith("w:")}


def _rel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


# ---- 1. the restatement against the reference's own numbers ---------------------------------------------------------------------------
def test_image_tower_reproduces_the_reference(load_golden):
    g = load_golden("glide_clip_image_reference")
    cfg = tuple(int(v) for v in g["cfg"])
    tower = G.GlideTower(_weights(g), cfg).at(g["ts"])
    run = tower.run(g["images"], g["probe"])
    unit = torch.nn.functional.normalize(run["emb"])
    cond = G.cond_fn_grad(tower, g["images"].double() * 2 - 1, g["z_t"], float(g["logit_scale"]), float(g["grad_scale"]))
    figs = dict(z=_rel(run["emb"], g["z"]), unit=_rel(unit, g["unit"]), grad=_rel(run["grad"], g["grad"]), cond_grad=_rel(cond, g["cond_grad"]))
    print("[bound] glide ref64 vs reference, image tower (max-abs / max-abs): " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    assert all(v <= 1e-9 for v in figs.values()), figs
    assert float(g["grad"].abs().max()) > 0 and float(g["cond_grad"].abs().max()) > 0


def test_text_tower_reproduces_the_reference(load_golden):
    g = load_golden("glide_clip_text_reference")
    cfg = tuple(int(v) for v in g["cfg"])
    assert g["lengths"].tolist() == [2, 7, 12] and cfg[0] == 12
    z, _ = G.GlideText(_weights(g), cfg).forward(g["ids"], g["lengths"])
    figs = dict(z=_rel(z, g["z"]), unit=_rel(torch.nn.functional.normalize(z), g["unit"]))
    print("[bound] glide ref64 vs reference, text tower (max-abs / max-abs): " + ", ".join(f"{k} {v:.2e}" for k, v in figs.items()))
    assert all(v <= 1e-9 for v in figs.values()), figs
    # pooled where the reference pools: another row gives another embedding
    z_off, _ = G.GlideText(_weights(g), cfg).forward(g["ids"], (g["lengths"] - 1).clamp(min=1))
    assert _rel(z_off[1:], g["z"][1:]) > 1e-3


def test_written_out_gradient_is_the_towers_vjp(load_golden):
    g = load_golden("glide_clip_image_reference")
    tower = G.GlideTower(_weights(g), tuple(int(v) for v in g["cfg"])).at(g["ts"])
    x = g["images"].double().requires_grad_(True)
    with torch.enable_grad():
        emb, _ = tower.forward(x)
        (torch.nn.functional.normalize(emb) * g["probe"]).sum().backward()
    assert V.rel_l2(tower.run(g["images"], g["probe"])["grad"], x.grad) <= 1e-12


# ---- 2. key maps, shapes, defaults ----------------------------------------------------------------------------------------------------
def test_key_maps_round_trip(load_golden):
    from perceptor_amd.engine import glide
    for name, fwd, inv, ref_fwd, shapes in (
            ("glide_clip_image_reference", glide.image_state_dict_to_vit, G.image_from_vit_names, G.image_to_vit_names, glide.glide_image_state_dict_shapes),
            ("glide_clip_text_reference", glide.text_state_dict_to_clip, G.text_from_clip_names, G.text_to_clip_names, glide.glide_text_state_dict_shapes)):
        g = load_golden(name)
        sd = _weights(g)
        assert {k: tuple(v.shape) for k, v in sd.items()} == shapes(tuple(int(v) for v in g["cfg"]))
        mapped = fwd(sd)
        want = ref_fwd(sd)
        assert set(mapped) == set(want) and all(torch.equal(mapped[k], want[k]) for k in want)
        back = inv(mapped)
        assert set(back) == set(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
        width = mapped["transformer.resblocks.0.attn.in_proj_weight"].shape[1]
        assert not mapped["transformer.resblocks.0.attn.in_proj_bias"][width:2 * width].any()          # no key bias
        assert mapped["transformer.resblocks.0.attn.in_proj_bias"][:width].any()


def test_default_configs_are_the_reference_config():
    from perceptor_amd import models
    from perceptor_amd.engine import glide
    assert glide.GLIDE_IMAGE_CONFIG == (64, 4, 768, 12, 12, 512, 1000) and glide.GLIDE_TEXT_CONFIG == (77, 65536, 512, 12, 8, 512)
    assert glide.GLIDE_LOGIT_SCALE == 100.0
    S = glide.glide_image_state_dict_shapes(glide.GLIDE_IMAGE_CONFIG)
    assert S["blocks.input.w_t"] == (1000, 768) and S["blocks.input.w_pos"] == (257, 768) and S["blocks.input.patch_proj"] == (768, 3, 4, 4)
    assert "blocks.block_11.f_attn.f_k.w" in S and "blocks.block_11.f_attn.f_k.b" not in S and S["blocks.output.f.w"] == (512, 768)
    m = models.GlideCLIP("synthetic", config=(16, 4, 128, 1, 2, 32, 8), text_config=(12, 64, 64, 1, 2, 32))
    assert set(m.state_dict()) == ({"model.image_encoder." + k for k in glide.glide_image_state_dict_shapes(m.cfg)}
                                   | {"model.text_encoder." + k for k in glide.glide_text_state_dict_shapes(m.text_cfg)})
    gains = m.state_dict()["model.image_encoder.blocks.input.ln.g"]
    assert abs(float(gains.mean()) - 1) < 0.1                                       # LayerNorm gains are drawn around 1, not around 0
    assert m.image_size == (16, 16) and m.output_dim == 32 and m.device.type == "cpu"


# ---- 3. tokenizer ---------------------------------------------------------------------------------------------------------------------
def test_tokenizer_ids_and_lengths_match_reference(load_golden):
    from oracle.gen_golden import TOKENIZER_PROMPTS
    from perceptor_amd import models
    from perceptor_amd.utils.tokenizer import ClipTokenizer
    g, gm = load_golden("glide_clip_text_reference"), load_golden("clip_tokenizer_merges")
    merges = [(f"\0{r}", "\0") for r in range(int(gm["n_merges"]))]     # "\0" is no symbol of the byte alphabet (tests/test_host_logic.py)
    for m, r in zip(gm["merges"].tolist(), gm["ranks"].tolist()):
        merges[r] = tuple(m)
    model = models.GlideCLIP("synthetic", config=(16, 4, 128, 1, 2, 32, 8), text_config=(77, 49408, 64, 1, 2, 32))
    ids, lengths = model.tokenize(TOKENIZER_PROMPTS, tokenizer=ClipTokenizer(merges=merges))
    assert torch.equal(ids, g["bpe_ids"]) and torch.equal(lengths, g["bpe_lengths"])
    assert int(lengths.min()) == 2 and int(lengths.max()) == 77          # the empty prompt and an over-long one are among them


# ---- 4. the two entry points ------------------------------------------------------------------------------------------------------------
def test_header_binding_and_library_agree_on_the_stem_entry_points():
    from perceptor_amd import _hip
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "perceptor_hip.h")).read(), flags=re.S)
    if not os.path.exists(_hip.LIB_PATH):
        from perceptor_amd.csrc import build
        build.build()
    lib = C.CDLL(_hip.LIB_PATH)
    for name, n_ptr in (("pmi_glide_embed_fwd", 12), ("pmi_glide_embed_bwd", 7)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;{]*?)\)\s*;", src, flags=re.S)
        assert m, f"{name} is not declared in include/perceptor_hip.h"
        params = [p.strip() for p in m.group(1).split(",")]
        (args,) = _hip._PROTOS[name]
        assert len(args) == len(params) and hasattr(lib, name)
        assert all("*" in p for p in params[:n_ptr]) and all(a is C.c_void_p for a in args[:n_ptr]) and "pmi_stream_t" in params[-1]
        for a, p in zip(args[n_ptr:-1], params[n_ptr:-1]):
            assert a is (C.c_float if re.search(r"\bfloat\b", p) else C.c_int), (name, p)
    from perceptor_amd.csrc import build
    assert "glide.hip" in build.SOURCES


# ---- 5. errors --------------------------------------------------------------------------------------------------------------------------
def test_constructor_and_shape_errors(tmp_path):
    from perceptor_amd import models
    from perceptor_amd.engine import glide
    with pytest.raises(RuntimeError, match=r"cannot be downloaded \(no network\): pass checkpoint_"):
        models.GlideCLIP()
    with pytest.raises(RuntimeError, match="cannot be downloaded"):
        models.GlideCLIP("openai", checkpoint_image="only-one.pt")
    with pytest.raises(ValueError):
        models.GlideCLIP("laion")
    with pytest.raises(ValueError):
        models.GlideCLIP("synthetic", precision="fp32")
    icfg, tcfg = (16, 4, 128, 1, 2, 32, 8), (12, 64, 64, 1, 2, 32)
    m = models.GlideCLIP("synthetic", config=icfg, text_config=tcfg)
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="HIP device"):
        m.encode_images(torch.zeros(1, 3, 16, 16), torch.zeros(1, dtype=torch.int64))
    for bad in (torch.tensor([8]), torch.tensor([-1])):
        with pytest.raises(ValueError, match="out of range"):
            m._check_ts(bad)
    # checkpoints: the two files' state dicts, loaded with weights_only=True; a file without the encoder's tensors is refused
    isd = {k[len("model.image_encoder."):]: v for k, v in m.state_dict().items() if k.startswith("model.image_encoder.")}
    tsd = {k[len("model.text_encoder."):]: v for k, v in m.state_dict().items() if k.startswith("model.text_encoder.")}
    torch.save(isd, tmp_path / "image.pt"); torch.save(tsd, tmp_path / "text.pt")
    m2 = models.GlideCLIP("openai", checkpoint_image=str(tmp_path / "image.pt"), checkpoint_text=str(tmp_path / "text.pt"), config=icfg, text_config=tcfg)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), m2.state_dict().values()))
    with pytest.raises(RuntimeError, match="does not hold"):
        models.GlideCLIP("openai", checkpoint_image=str(tmp_path / "text.pt"), checkpoint_text=str(tmp_path / "text.pt"), config=icfg, text_config=tcfg)
    # engines: shapes refused on the host
    for cfg in ((16, 8, 128, 1, 2, 32, 8), (16, 4, 96, 1, 2, 32, 8), (18, 4, 128, 1, 2, 32, 8)):
        with pytest.raises((ValueError, KeyError)):
            glide.GlideImageEngine(cfg, glide.glide_synth_state_dict(glide.glide_image_state_dict_shapes(cfg)), "cpu")


# ---- 6. seeded defects ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_seeded_defects_exceed_twice_a_gate(dtype, load_golden):
    g = load_golden("glide_clip_image_reference")
    cfg, sd = tuple(int(v) for v in g["cfg"]), _weights(g)
    u, gs, dt = V.U[TD[dtype]], GSCALE[dtype], TD[dtype]
    img, probe, ts = g["images"], g["probe"], g["ts"]
    ref = G.GlideTower(sd, cfg, emulate=dt).at(ts)
    whole = ref.run(img, probe)

    def ratios(got):
        out = [(st / (u * k ** 0.5), name) for name, st, k in G.tower_checks(ref, img, probe, got, whole)]
        return out + [(r, name) for name, r in G.stem_ratios(ref, img, got)]

    clean = max(ratios(ref.run(img, probe, bwd=dt, gscale=gs)))
    print(f"[bound] glide defect {dtype} none: {clean[0]:.2f}x the gate of '{clean[1]}'")
    assert clean[0] <= 1.0, clean
    for defect in G.DEFECTS:
        tower = G.GlideTower(sd, cfg, emulate=dt, defect=defect).at(ts) if defect in ("key bias", "quick gelu") else ref
        best = max(ratios(tower.run(img, probe, bwd=dt, gscale=gs, defect=defect)))
        print(f"[bound] glide defect {dtype} '{defect}': {best[0]:.1f}x the gate of '{best[1]}'")
        assert best[0] > 2.0, (dtype, defect, best)
