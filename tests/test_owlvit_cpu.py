"""CPU: models.OWLViT / losses.OWLViT -- the float64 restatement against the reference's own numbers, key tables, refusals, the loss gradient.

1. tests/_owlvit_ref64.py reproduces tests/golden/owlvit_reference_{a,b}.npz (tools/gen_owlvit_golden.py: the reference's vendored
   OwlViTForObjectDetection and its own losses.OWLViT.forward in float64).  Achieved, max |err| / max |ref| unless noted:
     hidden state 7e-16, image_feats 9e-16, text embeddings 1e-15, class_embeds 2e-15, pred_boxes 4e-16     gate 1e-13
     logits     per element 5.0e-8 / 5.9e-8 relative: the vendored head casts them to float32              gate 2^-24 relative, exactly
   The reference's loss runs on those float32 logits, so its log-softmax, sort and mean are float32 arithmetic and the gradient enters the
   float64 model through a float32 tensor.  That leg is mirrored, not given a wider gate: the reference's expression is evaluated in float32
   on the fixture's logits (loss: the fixture's to 2^-24, in fact the same bits) and its dloss/dlogits goes through the restatement's float64
   adjoints: d/d hidden and both image gradients then agree to 1e-13 ((b)'s image gradients, stored as float32, to that one rounding).  The
   closed-form float64 loss and dlogits are held to the float32 leg by running-error bounds n u A with counted n (in the test).
2. The top-k set is discontinuous in the logits: for every (image, query) column of both fixtures the gap between the 5th and 6th largest
   logit exceeds 8 x the emulated restatement's worst logit error, in bf16 and f16 (the seeds were chosen for that), and the emulated
   selection equals the exact one.
3. The closed-form loss gradient equals float64 autograd on the reference's expression at P = 9, 16, 576 and at P < k, P = k.
4. Key tables and mappers round-trip; missing, extra and mis-shaped keys are ValueErrors.
5. Refusals: a CPU tensor, a prompt of more than 16 tokens, ragged queries, a second add_encodings_, add_images_; the exports exist.
6. Each seeded defect of _owlvit_ref64.DEFECTS, at the engine test's inputs, exceeds 2 x its gate (multiples printed); the engine itself is
   held away from each defective restatement in tests/test_gpu_owlvit.py.
"""
import functools

import numpy as np
import pytest
import torch

import _owlvit_ref64 as O

CFG_A, TEXT_A = (96, 32, 128, 2, 2, 32), (16, 64, 32, 1, 1, 32)
TD = {"bf16": torch.bfloat16, "f16": torch.float16}


@functools.lru_cache(maxsize=None)
def _fixture(name):
    sd, R = O.load_fixture(name)
    return sd, R, torch.from_numpy(R["images8"]).double() / 255, torch.from_numpy(R["ids"]), torch.from_numpy(R["weights"]), int(R["top_k"])


@functools.lru_cache(maxsize=None)
def _run(name, emulate=None):
    sd, R, img, ids, w, k = _fixture(name)
    m = O.OwlVit(sd, R["cfg"], R["text_cfg"], emulate=emulate)
    return m, m.loss_and_grad(img, ids, w, k, bwd=emulate)


def _rel(got, want):
    want = torch.as_tensor(np.asarray(want)).double()
    return float((got.double() - want).abs().max() / want.abs().max())


# ---- 1 ------------------------------------------------------------------------------------------------------------------------------------
def _reference_loss_f32(logits32, w, k):
    """the reference's expression (losses/owlvit.py:66-79) on its float32 logits, in float32 as it runs there -> (loss, dloss / dlogits)"""
    x = logits32.clone().requires_grad_(True)
    loss = torch.tensor(0.0)
    for i, wi in enumerate(w.float()):
        loss = loss - x[:, :, i].flatten(start_dim=1).log_softmax(dim=1).sort(dim=1)[0][:, -k:].mean() * wi
    loss = loss * 0.01
    return loss.detach(), torch.autograd.grad(loss, x)[0]


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_reproduces_the_reference(name):
    _, R, img, ids, w, k = _fixture(name)
    m, out = _run(name)
    U = 2.0 ** -24
    figs = dict(hidden=_rel(out["hidden"], R["hidden"]), image_feats=_rel(out["image_feats"].reshape(R["image_feats"].shape), R["image_feats"]),
                text_embeds=_rel(m.text.forward(ids), R["text_embeds"]), class_embeds=_rel(out["class_embeds"], R["class_embeds"]),
                pred_boxes=_rel(out["pred_boxes"], R["pred_boxes"]))
    ref32 = torch.from_numpy(R["logits"])
    logit_rel = float(((out["logits"] - ref32.double()).abs() / ref32.double().abs()).max())
    assert R["logits"].dtype == np.float32 and logit_rel <= U
    # ---- the float32 leg, mirrored: the reference's loss and its gradient at the float32 logits, then the float64 adjoints of the restatement
    same_bits = torch.equal(out["logits"].float(), ref32)
    loss32, dl32 = _reference_loss_f32(ref32, w, k)
    _, d_hidden = m.backward(dl32.double(), out)
    figs["grad_hidden"] = _rel(d_hidden, R["grad_hidden"])
    grad, _ = m.backward(dl32.double(), out)
    s32 = ref32.clone().requires_grad_(True)
    (ds32,) = torch.autograd.grad(torch.sigmoid(s32.max(dim=-1).values).mean(), s32)
    g_scores, _ = m.backward(ds32.double(), out)
    if name == "a":
        figs["grad_images"], figs["grad_scores_images"] = _rel(grad, R["grad_images"]), _rel(g_scores, R["grad_scores_images"])
    else:                                                                    # stored as float32: one rounding per element
        assert R["grad_images"].dtype == np.float32
        for key, g in (("grad_images", grad), ("grad_scores_images", g_scores)):
            ref = torch.from_numpy(R[key]).double()
            figs[key + " (f32, in roundings)"] = float(((g - ref).abs() / (U * g.abs() + 1e-13 * g.abs().max())).max())
    loss_rel = abs(float(loss32) - float(R["loss"])) / abs(float(R["loss"]))
    # ---- the closed form in float64 against that float32 leg: running-error bounds n u A, A on absolute values.  log-softmax: max, subtract,
    # exp, a P-term sum, log, subtract = P + 5 roundings on |x| + |lse|; the mean over N k values N k + 1, weight, sum over Q and 0.01: Q + 2
    x = ref32.double()
    n_, p, q = x.shape
    ke = min(k, p)
    lse = torch.logsumexp(x, dim=1, keepdim=True)
    sel = O.topk_sets(x, k).double()
    coef = 0.01 * w / (n_ * ke)
    loss64, dl64 = O.topk_loss(x, w, k)
    A_loss = float((coef * ((x.abs() + lse.abs()) * sel).sum(dim=(0, 1))).sum())
    n_loss = (p + 5) + (n_ * ke + 1) + (q + 2)
    loss_ratio = abs(float(loss64) - float(R["loss"])) / (n_loss * U * A_loss)
    sm = torch.exp(x - lse)
    tol_dl = coef * (ke * sm * (p + 5) * U * (1 + x.abs() + lse.abs()) + (n_ * ke + q + 4) * U * (sel + ke * sm))
    dl_ratio = float(((dl64 - dl32.double()).abs() / tol_dl).max())
    print(f"[restatement] owlvit {name}: {figs}; logits {logit_rel:.3e} relative per element (same float32 bits: {same_bits}); float32 loss mirrored "
          f"{loss_rel:.3e}; closed-form float64 loss {loss_ratio:.3f} and dlogits {dl_ratio:.3f} of their float32 running-error bounds")
    assert all(v <= 1e-13 for key, v in figs.items() if "f32" not in key), figs
    assert all(v <= 1.0 for key, v in figs.items() if "f32" in key), figs
    assert loss_rel <= U and loss_ratio <= 1.0 and dl_ratio <= 1.0


def test_post_processing_on_the_reference_outputs():
    _, R, *_ = _fixture("a")
    logits, pred = torch.from_numpy(R["logits"]).double(), torch.from_numpy(R["pred_boxes"])
    boxes, scores, labels = O.post_process(logits, pred, (96, 96))
    assert boxes.shape == (2, 9, 4) and scores.shape == (2, 9) and labels.dtype == torch.int64
    assert torch.allclose((boxes[..., 0] + boxes[..., 2]) / 2, pred[..., 0] * 96) and torch.allclose(boxes[..., 3] - boxes[..., 1], pred[..., 3] * 96)
    assert torch.equal(labels, logits.argmax(-1)) and torch.allclose(scores, torch.sigmoid(logits.amax(-1)))


# ---- 2 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("name", ["a", "b"])
def test_topk_gap_exceeds_eight_logit_errors(name, dtype):
    _, R, *_, k = _fixture(name)
    exact = torch.from_numpy(R["logits"]).double()
    _, emu = _run(name, TD[dtype])
    err = float((emu["logits"] - exact).abs().max())
    gap = float(O.topk_gap(exact, k).min())
    print(f"[condition] owlvit {name} {dtype}: worst emulated logit error {err:.3e}, smallest gap {gap:.3e} = {gap / err:.1f} x")
    assert gap > 8 * err
    assert torch.equal(O.topk_sets(emu["logits"], k), O.topk_sets(exact, k))


# ---- 3 ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [4, 5, 9, 16, 576])
def test_loss_gradient_closed_form_equals_autograd(p):
    g = torch.Generator().manual_seed(p)
    logits = (torch.randn(2, p, 3, generator=g, dtype=torch.float64) * 2).requires_grad_(True)
    w = torch.tensor([1.0, 0.5, 2.0], dtype=torch.float64)
    loss = torch.tensor(0.0, dtype=torch.float64)
    for i, wi in enumerate(w):                                               # the reference's expression (losses/owlvit.py:66-79)
        loss = loss - logits[:, :, i].flatten(start_dim=1).log_softmax(dim=1).sort(dim=1)[0][:, -5:].mean() * wi
    loss = loss * 0.01
    (auto,) = torch.autograd.grad(loss, logits)
    got_loss, got = O.topk_loss(logits.detach(), w, 5)
    assert abs(float(got_loss) - float(loss.detach())) <= 1e-15 and float((got - auto).abs().max()) <= 1e-16
    assert float(got.sum(dim=1).abs().max()) <= 1e-16                        # a log-softmax gradient sums to zero over the tokens
    auto_s, = torch.autograd.grad(torch.sigmoid(logits.max(dim=-1).values).mean(), logits)
    assert float((O.scores_mean_grad(logits.detach()) - auto_s).abs().max()) <= 1e-16


# ---- 4 ------------------------------------------------------------------------------------------------------------------------------------
def test_key_tables_and_mappers_round_trip():
    from perceptor_amd.engine import owlvit as E
    from perceptor_amd.engine.text import from_owlvit_text_state_dict, text_state_dict_shapes
    from perceptor_amd.engine.vit import from_owlvit_vision_state_dict, vit_state_dict_shapes
    sd, R, *_ = _fixture("a")
    shapes = E.owlvit_state_dict_shapes(CFG_A, TEXT_A)
    assert set(shapes) == set(sd) and all(tuple(sd[k].shape) == tuple(shapes[k]) for k in shapes)
    E.check_state_dict(sd, CFG_A, TEXT_A)
    v, t = from_owlvit_vision_state_dict(sd), from_owlvit_text_state_dict(sd)
    assert {k: tuple(x.shape) for k, x in v.items()} == vit_state_dict_shapes(CFG_A)
    assert {k: tuple(x.shape) for k, x in t.items()} == text_state_dict_shapes(TEXT_A)
    rv, rt = O.vision_to_clip(sd), O.text_to_clip(sd)                        # the restatement's own mapping: the same tensors
    assert all(torch.equal(v[k].double(), rv[k]) for k in rv) and all(torch.equal(t[k].double(), rt[k]) for k in rt)
    prod = E.owlvit_state_dict_shapes(E.OWLVIT_VISION_CONFIG, E.OWLVIT_TEXT_CONFIG)
    assert prod["owlvit.vision_model.embeddings.position_embedding.weight"] == (577, 768) and prod["class_head.dense0.weight"] == (512, 768)
    assert prod["owlvit.text_model.embeddings.position_embedding.weight"] == (16, 512) and prod["box_head.dense2.weight"] == (4, 768)
    assert torch.equal(E.box_bias(3).double(), O.box_bias(3)) and torch.equal(E.box_bias(24).double(), O.box_bias(24))
    for bad in (dict(drop="layer_norm.weight"), dict(add="class_head.extra"), dict(reshape="box_head.dense2.weight")):
        s = dict(sd)
        if "drop" in bad:
            del s[bad["drop"]]
        if "add" in bad:
            s[bad["add"]] = torch.zeros(1)
        if "reshape" in bad:
            s[bad["reshape"]] = torch.zeros(8, 128)
        with pytest.raises(ValueError):
            E.check_state_dict(s, CFG_A, TEXT_A)
    with pytest.raises(ValueError):                                          # the class head needs text width == projection
        E.OwlVitEngine(CFG_A, (16, 64, 64, 1, 1, 32), sd, "cpu")


# ---- 5 ------------------------------------------------------------------------------------------------------------------------------------
class _Words:
    """one token per word"""
    sot, eot = 62, 63

    def encode(self, text):
        return [1 + len(w) % 60 for w in text.split()]

    def __call__(self, texts, context_length=77, pad="zero"):
        out = torch.zeros(len(texts), context_length, dtype=torch.int64)
        for i, t in enumerate(texts):
            ids = [self.sot] + self.encode(t) + [self.eot]
            out[i, :len(ids)] = torch.tensor(ids)
        return out


def test_exports_and_refusals():
    from perceptor_amd import losses, models
    from perceptor_amd.models.owlvit import OWLViTEncodings, OWLViTPredictions
    assert models.OWLViT.__name__ == "OWLViT" and losses.OWLViT.__name__ == "OWLViT" and models.OWLViTEncodings is OWLViTEncodings
    model = models.OWLViT(config=CFG_A, text_config=TEXT_A)
    assert model.size == (96, 96) and models.OWLViT.__init__.__kwdefaults__["weights"] == "synthetic"
    ids = model.tokenize(["a photo of a cat", "dog"], tokenizer=_Words())
    assert ids.shape == (2, 16) and ids[1].tolist()[:4] == [62, 4, 63, 0]
    with pytest.raises(ValueError):
        model.tokenize(["photo of a warrior trending on artstation photorealistic artstation and six more words here too"])      # 15 + 2 tokens
    assert model.tokenize(["photo of a warrior trending on artstation photorealistic artstation and six more words here"])[0, 15] == 63   # 14 + 2 fit
    with pytest.raises(NotImplementedError):
        model.encode_texts([["a cat"], ["a dog", "a bird"]])
    with pytest.raises(ValueError):
        model.encode_texts(torch.zeros(2, 17, dtype=torch.int64))
    enc = OWLViTEncodings([["x", "y"]], ids, torch.zeros(2, 32))
    rep = enc.repeat(3)
    assert rep.batch_encoding["input_ids"].shape == (6, 16) and rep.batch_encoding["attention_mask"].sum() == 3 * (7 + 3) and rep.texts == enc.texts
    assert enc.to("cpu") is enc
    with pytest.raises(RuntimeError):
        model(torch.zeros(1, 3, 96, 96), enc)
    with pytest.raises(RuntimeError):
        model.encode_texts(ids)                                              # the text tower has no CPU path either
    loss = losses.OWLViT(config=CFG_A, text_config=TEXT_A)
    with pytest.raises(NotImplementedError):
        loss.add_images_(torch.zeros(1, 3, 96, 96))
    loss.add_encodings_(enc, weights=[1.0, 0.5])
    with pytest.raises(ValueError):
        loss.add_encodings_(enc)
    with pytest.raises(ValueError):
        losses.OWLViT(config=CFG_A, text_config=TEXT_A).add_encodings_(enc, weights=[1.0, 1.0, 1.0])
    # the reference's default is one weight per inner list and its loss walks the weights: only the first query is scored
    assert losses.OWLViT(config=CFG_A, text_config=TEXT_A).add_encodings_(enc).weights.tolist() == [1.0, 0.0]
    with pytest.raises(RuntimeError):
        loss(torch.zeros(1, 3, 96, 96))
    rec = OWLViTPredictions(logits=torch.zeros(1, 9, 2), boxes=torch.zeros(1, 9, 4), scores=torch.zeros(1, 9), labels=torch.zeros(1, 9), texts=[["x", "y"]])
    with pytest.raises(AttributeError):
        rec.logits = None
    with pytest.raises(RuntimeError):
        models.OWLViT(weights="google/owlvit-base-patch32")


# ---- 6 ------------------------------------------------------------------------------------------------------------------------------------
DEFECT_METRIC = {"merge row 1": "logits", "query eps inside": "logits", "elu no +1": "logits", "shift after scale": "logits", "mean over k": "loss",
                 "box xy swapped": "boxes", "eos last": "logits"}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
@pytest.mark.parametrize("defect", O.DEFECTS)
def test_seeded_defects_exceed_twice_their_gate(defect, dtype):
    """At the engine test's inputs (fixture a), the float64 restatement with one defect against the fixture, in the metric of
    tests/test_gpu_owlvit.py section C: more than 2 x that test's gate (which is itself 2 x the measured distance).
    One defect cannot: ``query eps inside`` moves the logits by 2.4e-6, far inside any 16-bit gate.  What holds that quirk is the
    float64 restatement's logit check at 2^-24 relative (section 1), and that is the gate it is held to here: 361 x twice that gate."""
    from test_gpu_owlvit import MEASURED
    sd, R, img, ids, w, k = _fixture("a")
    m, _ = _run("a")
    bad = m.loss_and_grad(img, ids, w, k, defect=defect)
    T = lambda a: torch.as_tensor(np.asarray(a)).double()
    dist = dict(logits=float((bad["logits"] - T(R["logits"])).abs().max()), boxes=float((bad["pred_boxes"] - T(R["pred_boxes"])).abs().max()),
                loss=abs(float(bad["loss"]) - float(R["loss"])))[DEFECT_METRIC[defect]]
    gate = 2 * MEASURED[("a", dtype)][DEFECT_METRIC[defect]]
    print(f"[defect] owlvit {dtype} {defect}: {DEFECT_METRIC[defect]} moved {dist:.3e} = {dist / gate:.1f} x the engine gate {gate:.3e}")
    if defect == "query eps inside":
        ref = T(R["logits"])
        rel = float(((bad["logits"] - ref).abs() / ref.abs()).max())
        print(f"[defect] owlvit {defect}: {rel:.3e} relative = {rel / 2.0 ** -24:.1f} x the restatement's 2^-24 gate")
        assert rel > 2 * 2.0 ** -24
    else:
        assert dist > 2 * gate, (defect, dist, gate)
