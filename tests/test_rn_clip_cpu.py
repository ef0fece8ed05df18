"""CLIP ResNet image towers (RN50 .. RN50x64) without a GPU: state-dict layout, checkpoint loading, BatchNorm folding, the model / loss
surface and the synthetic BatchNorm statistics."""
import pytest
import torch
import torch.nn.functional as F

from perceptor_amd.engine import resnet

NAMES = ["RN50", "RN101", "RN50x4", "RN50x16", "RN50x64"]
# written out from open_clip's model configs, independently of resnet.RN_CONFIGS
POS = {"RN50": (50, 2048), "RN101": (50, 2048), "RN50x4": (82, 2560), "RN50x16": (145, 3072), "RN50x64": (197, 4096)}
CPROJ = {"RN50": (1024, 2048), "RN101": (512, 2048), "RN50x4": (640, 2560), "RN50x16": (768, 3072), "RN50x64": (1024, 4096)}
LAYERS = {"RN50": (3, 4, 6, 3), "RN101": (3, 4, 23, 3), "RN50x4": (4, 6, 10, 6), "RN50x16": (6, 8, 18, 8), "RN50x64": (3, 15, 36, 10)}
WIDTH = {"RN50": 64, "RN101": 64, "RN50x4": 80, "RN50x16": 96, "RN50x64": 128}


@pytest.mark.parametrize("name", NAMES)
def test_state_dict_shapes(name):
    S = resnet.rn_state_dict_shapes(resnet.RN_CONFIGS[name])
    assert S["attnpool.positional_embedding"] == POS[name]
    assert S["attnpool.c_proj.weight"] == CPROJ[name]
    w = WIDTH[name]
    assert S["conv1.weight"] == (w // 2, 3, 3, 3) and S["conv3.weight"] == (w, w // 2, 3, 3)
    for n in "qkv":
        assert S[f"attnpool.{n}_proj.weight"] == (32 * w, 32 * w)
    inplanes = w
    for li, nb in enumerate(LAYERS[name]):
        blocks = {k.split(".")[1] for k in S if k.startswith(f"layer{li + 1}.")}
        assert blocks == {str(b) for b in range(nb)}, (li, blocks)
        planes = w * 2 ** li
        for b in range(nb):
            p = f"layer{li + 1}.{b}."
            stride = 2 if li > 0 and b == 0 else 1
            assert S[p + "conv1.weight"] == (planes, inplanes, 1, 1)
            assert S[p + "conv2.weight"] == (planes, planes, 3, 3)
            assert S[p + "conv3.weight"] == (4 * planes, planes, 1, 1)
            want = stride > 1 or inplanes != 4 * planes
            assert (p + "downsample.0.weight" in S) == want
            assert all((p + f"downsample.1.{leaf}" in S) == want for leaf in ("weight", "bias", "running_mean", "running_var"))
            if want:
                assert S[p + "downsample.0.weight"] == (4 * planes, inplanes, 1, 1)
            inplanes = 4 * planes
    assert not any(k.endswith("num_batches_tracked") for k in S)


def test_checkpoint_with_num_batches_tracked_loads(tmp_path):
    from perceptor_amd import models
    from perceptor_amd.utils.synth import synth_state_dict
    S = resnet.rn_state_dict_shapes(resnet.RN_CONFIGS["RN50"])
    sd = {"visual." + k: v for k, v in synth_state_dict(S, 3).items()}
    for k in list(sd):
        if k.endswith(".running_var"):
            sd[k[:-len("running_var")] + "num_batches_tracked"] = torch.tensor(7, dtype=torch.int64)
    sd["logit_scale"] = torch.tensor(4.6)                  # a full open_clip checkpoint's non-visual entry (no text tower here)
    path = tmp_path / "rn50.pt"
    torch.save(sd, path)
    m = models.OpenCLIP("RN50", "cc12m", checkpoint=str(path))
    vsd = m.visual_state_dict()
    assert set(vsd) == set(S)
    assert torch.equal(vsd["layer2.0.downsample.1.running_var"], sd["visual.layer2.0.downsample.1.running_var"])
    assert m.output_dim == 1024 and m.image_size == (224, 224) and m.text_cfg is None


@pytest.mark.parametrize("k,stride", [(3, 1), (3, 2), (1, 1)])
def test_bn_folding_is_exact(k, stride):
    g = torch.Generator().manual_seed(k * 10 + stride)
    x = torch.randn(2, 6, 9, 10, generator=g, dtype=torch.float64)
    w = torch.randn(5, 6, k, k, generator=g, dtype=torch.float64)
    bn = {"weight": 1 + 0.1 * torch.randn(5, generator=g, dtype=torch.float64), "bias": 0.05 * torch.randn(5, generator=g, dtype=torch.float64),
          "running_mean": 0.1 * torch.randn(5, generator=g, dtype=torch.float64),
          "running_var": 0.5 + torch.randn(5, generator=g, dtype=torch.float64).abs()}
    ref = F.batch_norm(F.conv2d(x, w, stride=stride, padding=k // 2), bn["running_mean"], bn["running_var"], bn["weight"], bn["bias"],
                       training=False, eps=1e-5)
    wf, bf = resnet.fold_bn(w, bn)
    got = F.conv2d(x, wf, bf, stride=stride, padding=k // 2)
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_model_and_loss_surface():
    from perceptor_amd import losses, models
    m = models.OpenCLIP("RN50x4", "synthetic")
    assert m.output_dim == 640 and m.image_size == (288, 288)
    assert m.text_cfg == (77, 49408, 640, 12, 10, 640)
    c = models.CLIP("RN50", weights="synthetic")
    assert c.architecture == "RN50-quickgelu" and c.output_dim == 1024
    lo = losses.CLIP("RN101", weights="synthetic")
    assert lo.model.architecture == "RN101-quickgelu" and lo.model.output_dim == 512
    with pytest.raises(RuntimeError, match="no network"):
        models.OpenCLIP("RN50x16", "openai")
    with pytest.raises(RuntimeError, match="no network"):
        models.CLIP("RN50")


def test_synthetic_batchnorm_statistics():
    from perceptor_amd.utils.synth import synth_state_dict
    sd = synth_state_dict(resnet.rn_state_dict_shapes(resnet.RN_CONFIGS["RN50"]), 0)
    vars_ = [v for k, v in sd.items() if k.endswith("running_var")]
    assert len(vars_) == 3 + 16 * 3 + 4
    assert all(float(v.min()) >= 0.5 for v in vars_)
    means = torch.cat([v for k, v in sd.items() if k.endswith("running_mean")])
    assert 0.05 < float(means.std()) < 0.2


def _checksum(shapes):
    from perceptor_amd.utils.synth import synth_state_dict
    sd = synth_state_dict(shapes, 0)
    return (sum(float(sd[k].double().abs().sum()) for k in sorted(sd)), sum(float(sd[k].double().sum()) for k in sorted(sd)))


def test_synthetic_weights_of_existing_models_unchanged():
    """Checksums taken before the BatchNorm branches were added to synth_tensor: no ViT / text / UNet weight may change."""
    from perceptor_amd.engine import adm, text, vit
    kw = dict(image_size=64, model_channels=64, num_res_blocks=1, channel_mult=(1, 2), attention_ds=(1, 2), num_head_channels=64,
              use_scale_shift_norm=True, resblock_updown=True)
    for shapes, want in ((vit.vit_state_dict_shapes(vit.VIT_CONFIGS["ViT-B-32"]), (2108427.507007943, 20074.859766655416)),
                         (adm.state_dict_shapes(adm.AdmConfig(**kw)), (117591.30246242425, 3253.0675311440027)),
                         (text.text_state_dict_shapes(text.TEXT_CONFIGS["ViT-B-32"]), (2027670.251403433, 12564.587325034336))):
        got = _checksum(shapes)
        assert got[0] == pytest.approx(want[0], rel=1e-12) and got[1] == pytest.approx(want[1], rel=1e-9, abs=1e-6), (got, want)


def test_unsupported_configs_rejected_before_any_launch():
    """An image size that is not a multiple of 32 would floor a 2x2 pool (the backward's maps would no longer match the saved masks)."""
    cfg = resnet.RN_CONFIGS["RN50"]
    with pytest.raises(ValueError, match="image % 32"):
        resnet.ResNetEngine((112,) + cfg[1:], {}, "cpu")
    with pytest.raises(ValueError):
        resnet.ResNetEngine((224, cfg[1], 64, 16, 1024), {}, "cpu")          # heads != width / 2


def test_synthetic_residual_stream_stays_bounded():
    """Synthetic Bottleneck bn3 gains ~0.5: the residual stream of the deep towers stays O(1), so the attention pool is not an argmax."""
    import _rn_ref64 as RN
    from perceptor_amd.utils.synth import seeded_noise, synth_state_dict
    cfg = resnet.RN_CONFIGS["RN101"]
    sd = synth_state_dict(resnet.rn_state_dict_shapes(cfg), 0)
    g3 = torch.stack([v.mean() for k, v in sd.items() if k.startswith("layer") and k.endswith("bn3.weight")])
    assert float((g3 - 0.5).abs().max()) < 0.05 and float(sd["bn3.weight"].mean()) > 0.9     # the stem's bn3 keeps the ordinary gains
    stages = []
    with torch.no_grad():
        RN.tower(sd, cfg, RN.normalize(seeded_noise((1, 3, 224, 224), 31) * 0.25 + 0.5), stages=stages)
    rms = [float(t.pow(2).mean().sqrt()) for t in stages]
    assert max(rms) < 1.0, rms
