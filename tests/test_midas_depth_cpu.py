"""CPU: models.MidasDepth without a device -- the float64 restatement (tests/_dpt_ref64.py) against plain torch modules and autograd, the
commuted out_conv, the state-dict key table and the mappers, refusals, the MEASURED table of tests/test_gpu_midas_depth.py, the seeded
defects against its gates, and the argument refusals of the kernels of csrc/dpt.hip (PMI_ERR_ARG without a launch).

The fixtures' images are one dark and one bright image and their last 1 x 1 convolution is a fitted discriminant (D.fit_head), so that z
is two separated clusters: the share of output pixels with |z| within 8 x the emulated error of zero is asserted <= 2 % in bf16 and f16
on both, the active share 20 - 80 %.  The figures are the [bound] lines; DESIGN.md section 33 keeps them.
"""
import ctypes as C
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _dpt_ref64 as D                      # noqa: E402
from perceptor_amd.engine import dpt as E   # noqa: E402
from perceptor_amd.engine import vit as V   # noqa: E402


def test_midas_depth_is_exported():
    from perceptor_amd import models
    assert hasattr(models, "MidasDepth")
    m = models.MidasDepth(config=D.CONFIGS["a"])
    assert m.image_size == (64, 64) and m.name == "dpt_large"
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 64, 64))                                  # a CPU tensor
    with pytest.raises(RuntimeError):
        m.engine                                                      # no HIP device behind the parameters


@pytest.mark.parametrize("name", ["dpt_hybrid", "dpt_hybrid_nyu", "dpt_hybrid_kitti", "midas_v21", "midas_v21_small"])
def test_other_names_say_why(name):
    from perceptor_amd import models
    with pytest.raises(NotImplementedError, match="timm|torch.hub"):
        models.MidasDepth(name)
    with pytest.raises(ValueError):
        models.MidasDepth("nope")


def test_key_table_and_mappers(tmp_path):
    from perceptor_amd import models
    cfg = E.DPT_CONFIGS["dpt_large"]
    S = E.dpt_state_dict_shapes(cfg)
    R = E.reference_state_dict_shapes(cfg)
    assert len(S) == 364 and set(R) - set(S) == {"pretrained.model.norm.weight", "pretrained.model.norm.bias", "pretrained.model.head.weight",
                                                 "pretrained.model.head.bias"}
    assert S["pretrained.model.pos_embed"] == (1, 577, 1024) and S["pretrained.act_postprocess1.4.weight"] == (256, 256, 4, 4)
    assert S["pretrained.act_postprocess2.4.weight"] == (512, 512, 2, 2) and S["pretrained.act_postprocess4.4.weight"] == (1024, 1024, 3, 3)
    assert "pretrained.act_postprocess3.4.weight" not in S and S["scratch.output_conv.4.weight"] == (1, 32, 1, 1)
    assert S["scratch.refinenet4.resConfUnit1.conv1.weight"] == (256, 256, 3, 3)              # in the checkpoint, never run
    # the timm mapper: names, the folded patch bias, and a round trip through the shapes table
    cfg_a, sd, _ = D.toy("a")
    assert {k: tuple(v.shape) for k, v in sd.items()} == E.dpt_state_dict_shapes(cfg_a)
    m = V.from_timm_vit_state_dict(sd, "pretrained.model.")
    assert set(m) == set(V.vit_state_dict_shapes(cfg_a[:5] + (0,))) - {"ln_pre.weight", "ln_pre.bias", "ln_post.weight", "ln_post.bias", "proj"}
    pos, bias = sd["pretrained.model.pos_embed"][0], sd["pretrained.model.patch_embed.proj.bias"]
    assert torch.equal(m["positional_embedding"][0], pos[0]) and torch.equal(m["positional_embedding"][1:], pos[1:] + bias)
    assert torch.equal(m["transformer.resblocks.3.mlp.c_proj.weight"], sd["pretrained.model.blocks.3.mlp.fc2.weight"])
    # the checkpoint formats of base_model.py, the ignored keys, and the refusals
    full = dict(sd)
    full.update({"pretrained.model.norm.weight": torch.ones(128), "pretrained.model.norm.bias": torch.zeros(128),
                 "pretrained.model.head.weight": torch.zeros(1000, 128), "pretrained.model.head.bias": torch.zeros(1000)})
    for i, payload in enumerate((full, {"model": full, "optimizer": {}})):
        path = str(tmp_path / f"ckpt{i}.pt")
        torch.save(payload, path)
        mm = models.MidasDepth(config=cfg_a, checkpoint=path)
        got = mm.model.state_dict()
        assert set(got) == set(sd) and all(torch.equal(got[k], sd[k]) for k in sd)
    for bad in ({k: v for k, v in sd.items() if k != "scratch.layer1_rn.weight"}, dict(sd, extra=torch.zeros(1)),
                dict(sd, **{"scratch.layer1_rn.weight": torch.zeros(32, 16, 1, 1)})):
        with pytest.raises(ValueError):
            E.check_state_dict(bad, cfg_a)
    with pytest.raises(ValueError):
        E.check_config((64, 32, 128, 4, 2, (0, 1, 2, 3), (16, 32, 64, 64), 32))              # patch 32
    with pytest.raises(ValueError):
        E.check_config((64, 16, 128, 4, 2, (0, 1, 2, 4), (16, 32, 64, 64), 32))              # a hook past the last block


def test_position_grid_must_match():
    """the reference resamples the positional embedding to the input grid; at res / patch that is the identity, anything else is refused"""
    cfg, sd, _ = D.toy("a")
    m = V.from_timm_vit_state_dict(sd, "pretrained.model.")
    m["positional_embedding"] = torch.zeros(26, 128)                  # a 5 x 5 grid
    with pytest.raises(ValueError, match="position grid"):
        V.VitEngine(cfg[:5] + (0,), m, "cpu", "bf16", quick_gelu=False, ln_eps=1e-6, pre_ln=False, pooled_head=False)


class _Unit(torch.nn.Module):
    def __init__(self, f):
        super().__init__()
        self.conv1, self.conv2 = torch.nn.Conv2d(f, f, 3, padding=1), torch.nn.Conv2d(f, f, 3, padding=1)

    def forward(self, x):
        return self.conv2(F.relu(self.conv1(F.relu(x)))) + x


def test_restatement_pieces_against_torch_modules():
    """the decoder of the restatement against an independent assembly from nn modules in the reference's order (out_conv AFTER the
    up-sampling, ConvTranspose2d, ProjectReadout by concatenation), float64, same weights"""
    cfg, sd, images = D.toy("b")
    res, patch, width, layers, heads, hooks, channels, features = cfg
    ref = D.Dpt64(sd, cfg)
    with torch.no_grad():
        out = ref.forward(images.double())
        n, g = 2, res // patch
        maps = []
        for k, tap in enumerate(out["taps"], start=1):
            p = f"pretrained.act_postprocess{k}."
            cat = torch.cat([tap[:, 1:], tap[:, :1].expand(-1, g * g, -1)], -1)                    # vit.py:39-40
            y = F.gelu(F.linear(cat, ref.sd[p + "0.project.0.weight"], ref.sd[p + "0.project.0.bias"]))
            y = F.conv2d(y.transpose(1, 2).reshape(n, width, g, g), ref.sd[p + "3.weight"], ref.sd[p + "3.bias"])
            if k in (1, 2):
                y = F.conv_transpose2d(y, ref.sd[p + "4.weight"], ref.sd[p + "4.bias"], stride=6 - 2 * k)
            elif k == 4:
                y = F.conv2d(y, ref.sd[p + "4.weight"], ref.sd[p + "4.bias"], stride=2, padding=1)
            maps.append(y)
            assert D.rel(out["maps"][k - 1], y) <= 1e-12

        def unit(key):
            u = _Unit(features).double()
            u.load_state_dict({f"conv{i}.{wb}": ref.sd[f"{key}.conv{i}.{wb}"] for i in (1, 2) for wb in ("weight", "bias")})
            return u

        rn = [F.conv2d(m, ref.sd[f"scratch.layer{k + 1}_rn.weight"], None, padding=1) for k, m in enumerate(maps)]
        path = None
        for k in (3, 2, 1, 0):
            f = f"scratch.refinenet{k + 1}."
            x = rn[k] if path is None else path + unit(f + "resConfUnit1")(rn[k])
            path = F.conv2d(D.up2(unit(f + "resConfUnit2")(x)), ref.sd[f + "out_conv.weight"], ref.sd[f + "out_conv.bias"])
            r = D.rel(out["paths"][k], path)
            print(f"[bound] path_{k + 1} (commuted out_conv) against the reference order: {r:.2e}")
            assert r <= 1e-13
        y = D.up2(F.conv2d(path, ref.sd["scratch.output_conv.0.weight"], ref.sd["scratch.output_conv.0.bias"], padding=1))
        y = F.relu(F.conv2d(y, ref.sd["scratch.output_conv.2.weight"], ref.sd["scratch.output_conv.2.bias"], padding=1))
        y = -F.relu(F.conv2d(y, ref.sd["scratch.output_conv.4.weight"], ref.sd["scratch.output_conv.4.bias"]))
        assert D.rel(out["depth"], y) <= 1e-12


def _tool():
    import importlib
    import transformers                      # noqa: F401  (before the tool's package shells could exist)
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    return importlib.import_module("gen_midas_golden")


@pytest.mark.parametrize("name", ["a", "b"])
def test_vit_standin_and_restatement_tower_against_transformers(name):
    """the VisionTransformer stand-in of tools/gen_midas_golden.py (the one piece of the fixtures' arithmetic not taken from the reference)
    and the restatement's tower against the installed transformers.ViTModel configured as timm's ViT (gelu, eps 1e-6, qkv bias, eager
    attention with its softmax taken in float64: the tool's hf_vit), on every block output / tap, to 1e-12"""
    T = _tool()
    w = T.check_standin(name)
    print(f"[bound] {name}: ViT stand-in against transformers.ViTModel, worst block output {w:.2e}")
    assert w <= 1e-12
    cfg, sd, images = D.toy(name)
    with torch.no_grad():
        x = D.resize64(images.double(), (cfg[0], cfg[0])) if tuple(images.shape[2:]) != (cfg[0], cfg[0]) else images.double()
        hidden = T.hf_vit(cfg, sd)(pixel_values=(x - 0.5) / 0.5, output_hidden_states=True).hidden_states
        taps = D.Dpt64(sd, cfg).tower(x)
    for k, hk in enumerate(cfg[5]):
        r = D.rel(taps[k], hidden[hk + 1])
        print(f"[bound] {name}: tap {k} of the restatement against transformers.ViTModel: {r:.2e}")
        assert r <= 1e-12


@pytest.mark.parametrize("name", ["a", "b"])
def test_hand_written_backward_equals_autograd(name):
    """Dpt64.forward_backward (no autograd; takes the masks and the upstream gradient) against float64 autograd over Dpt64.forward, with
    its own masks and with masks pinned to another run's (the bf16-emulated run's, as the GPU tests pin the engine's)"""
    cfg, sd, images = D.toy(name)
    with torch.no_grad():
        other = D.Dpt64(sd, cfg, emulate=torch.bfloat16).forward(images.double())["masks"]
    assert any(not torch.equal(other[k], D.free_run(name)["masks"][k]) for k in other), "the pinned masks should differ from the free run's"
    for kind in ("mean", "rand"):
        d = D.upstream(name, kind)
        for masks in (None, other):
            g0, o0 = D.image_grad(D.Dpt64(sd, cfg), images, d, masks=masks)
            depth, g1, seen = D.Dpt64(sd, cfg).forward_backward(images, d, masks=masks)
            rd, rg = D.rel(depth, o0["depth"]), D.rel(g1, g0)
            print(f"[bound] {name} {kind} {'pinned' if masks else 'free'}: depth {rd:.2e}, image gradient {rg:.2e}")
            assert rd <= 1e-12 and rg <= 1e-12 and all(torch.equal(seen[k], o0["masks"][k]) for k in seen)


def test_pinned_masks_reproduce_the_free_run_and_its_gradient():
    cfg, sd, images = D.toy("a")
    free = D.free_run("a")
    d = D.upstream("a", "rand")
    g0, o0 = D.image_grad(D.Dpt64(sd, cfg), images, d)
    g1, o1 = D.image_grad(D.Dpt64(sd, cfg), images, d, masks=o0["masks"])
    assert torch.equal(o0["depth"], free["depth"]) and torch.equal(o1["depth"], o0["depth"]) and torch.equal(g0, g1)
    # the gradient is autograd's of float64: a central difference along one random direction agrees
    v = torch.randn(images.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    eps = 1e-6
    with torch.no_grad():
        hi = (D.Dpt64(sd, cfg).forward(images.double() + eps * v, masks=o0["masks"])["depth"] * d).sum()
        lo = (D.Dpt64(sd, cfg).forward(images.double() - eps * v, masks=o0["masks"])["depth"] * d).sum()
    fd, an = float(hi - lo) / (2 * eps), float((g0 * v).sum())
    assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-12), (fd, an)


@pytest.mark.parametrize("name", ["a", "b"])
def test_measured_table_and_defects(name):
    from test_gpu_midas_depth import MEASURED
    cfg, sd, images = D.toy(name)
    free = D.free_run(name)
    active = float((free["z"] > 0).double().mean())
    assert 0.2 <= active <= 0.8
    for dtype in ("bf16", "f16"):
        m, M = D.measured(name, dtype), MEASURED[(name, dtype)]
        band = float((free["z"].abs() < 8 * m["z_err"]).double().mean())
        print(f"[bound] {name} {dtype}: measured {({k: float(f'{v:.3g}') for k, v in m.items()})}; active share {active:.3f}, z-band share {band:.3f}")
        assert band <= 0.02, f"{band:.3f} of the output pixels lie within 8 x the {dtype}-emulated error of zero"
        for k, v in m.items():
            assert 0.8 * M[k] <= v <= M[k], f"MEASURED[{name}, {dtype}][{k}] = {M[k]} but the emulated restatement is {v:.3g} away"
    M = MEASURED[(name, "bf16")]
    d = D.upstream(name, "rand")
    g0, o0 = D.image_grad(D.Dpt64(sd, cfg), images, d)
    for defect in [x for x in D.DEFECTS if D.DEFECT_CONFIG.get(x, "b") == name]:          # at the inputs the GPU test shows it at
        if defect == "tap_grad_not_injected":
            g1, _ = D.image_grad(D.Dpt64(sd, cfg, defect=defect), images, d, masks=o0["masks"])
            moved, gate = D.rel(g1, g0), 2 * M["grad_rand"]
        else:
            with torch.no_grad():
                moved, gate = D.rel(D.Dpt64(sd, cfg, defect=defect).forward(images.double())["depth"], free["depth"]), 2 * M["depth"]
        print(f"[bound] {name} defect {defect}: moves the output by {moved / gate:.1f} bf16 gates")
        assert moved > 2 * gate


def test_kernel_argument_refusals():
    from perceptor_amd import _hip
    L = _hip.lib()
    x = C.create_string_buffer(4096)
    a = (C.addressof(x) + 15) // 16 * 16
    ERR = -1
    assert L.pmi_bilinear2_ac_fwd(a, None, a, 1, 1, 1, 4, 1, None) == ERR            # C % 8
    assert L.pmi_bilinear2_ac_fwd(a + 2, None, a, 1, 1, 1, 8, 1, None) == ERR        # alignment
    assert L.pmi_bilinear2_ac_fwd(a, None, a, 1, 0, 1, 8, 1, None) == ERR            # H = 0
    assert L.pmi_bilinear2_ac_fwd(a, None, a, 1, 1, 1, 8, 2, None) == ERR            # dtype
    assert L.pmi_bilinear2_ac_fwd(None, None, a, 1, 1, 1, 8, 1, None) == ERR
    assert L.pmi_bilinear2_ac_bwd(a, a, 1, 20000, 1, 8, 1, None) == ERR              # beyond the 32-bit index arithmetic
    assert L.pmi_bilinear2_ac_bwd(a, None, 1, 1, 1, 8, 1, None) == ERR
    assert L.pmi_depth_to_space(a, None, a, 1, 1, 1, 8, 3, 1, None) == ERR           # k
    assert L.pmi_depth_to_space(a, None, a, 1, 1, 1, 12, 2, 1, None) == ERR
    assert L.pmi_space_to_depth(a, a, 1, 1, 1, 8, 8, 0, None) == ERR
    assert L.pmi_space_to_depth(a, None, 1, 1, 1, 8, 2, 0, None) == ERR
    assert L.pmi_dpt_tap_split(a, a, a, 1, 1, 64, 1, None) == ERR                    # T = 1: no patch rows
    assert L.pmi_dpt_tap_split(a, a, a, 1, 2, 6, 1, None) == ERR                     # W % 4
    assert L.pmi_dpt_tap_join(a, a, None, 1, 2, 64, None) == ERR
    assert L.pmi_dpt_tap_join(a, a, a, 0, 2, 64, None) == ERR
    assert L.pmi_dpt_tap_add(a, a, a, a, 6, 1, None) == ERR                          # n % 4
    assert L.pmi_dpt_tap_add(a, a, a, None, 8, 1, None) == ERR
    assert L.pmi_dpt_colsum(a, a, 1, 0, 64, 1, None) == ERR
    assert L.pmi_dpt_colsum(a, a, 1, 4, 63, 1, None) == ERR                          # W odd
    assert L.pmi_dpt_colsum(a, a, 70000, 4, 64, 1, None) == ERR                      # grid.y
    assert L.pmi_dpt_relu_bwd(a, a, None, a, 12, 1, None) == ERR                     # n % 8
    assert L.pmi_dpt_relu_bwd(a, None, None, a, 8, 1, None) == ERR
    assert L.pmi_dpt_head_fwd(a, a, None, a, 8, 1, None) == ERR
    assert L.pmi_dpt_head_fwd(a, a, a, a, 0, 1, None) == ERR
    assert L.pmi_dpt_head_bwd(a, a, a, a, a, 8, float("nan"), 1, None) == ERR
    assert L.pmi_dpt_head_bwd(a, a, a, a, None, 8, 1.0, 1, None) == ERR


def _sample(t, step):
    return t.detach().double().reshape(-1)[::int(step)] if int(step) > 1 else t.detach().double()


@pytest.mark.parametrize("name", ["a", "b"])
def test_restatement_reproduces_the_reference_fixture(name, load_golden):
    """tests/golden/midas_depth_reference_{a,b}.npz: the reference's own DPT modules in float64 (tools/gen_midas_golden.py).  Tensors of more
    than 8192 elements are stored as every step-th element.  (b) is resized by the reference's resize_right, whose band weights are fp32
    as the engine's tables are: the resized images are reproduced exactly."""
    g = load_golden(f"midas_depth_reference_{name}")
    cfg, sd, images = D.toy(name)
    assert [int(v) for v in g["cfg"]] == [cfg[0], cfg[1], cfg[2], cfg[3], cfg[4], cfg[7]] and tuple(int(v) for v in g["hooks"]) == cfg[5]
    assert D.digest(sd) == str(g["weight_sha256"]), "the synthetic weights differ from the ones the fixture was generated with"
    assert torch.equal(_sample(images, g["step:images"]), g["images"])
    x = images.double().requires_grad_(True)
    model = D.Dpt64(sd, cfg)
    out = model.forward(x)
    got = dict(resized=out["resized"], depth=out["depth"], z=out["z"])
    for k in range(4):
        got[f"tap{k + 1}"], got[f"map{k + 1}"], got[f"path{k + 1}"] = out["taps"][k], out["maps"][k], out["paths"][k]
    for kind in ("mean", "rand"):
        got["grad_" + kind], got["grad_resized_" + kind] = torch.autograd.grad((out["depth"] * D.upstream(name, kind)).sum(), [x, out["resized"]],
                                                                                retain_graph=True)
    worst = 0.0
    for k, v in got.items():
        r = D.rel(_sample(v, g["step:" + k]).reshape(g[k].shape), g[k])
        worst = max(worst, r)
        assert r <= 1e-12, f"{name} {k}: {r:.2e}"
    for kind in ("mean", "rand"):
        _, gi, _ = D.Dpt64(sd, cfg).forward_backward(images, D.upstream(name, kind))
        r = D.rel(_sample(gi, g["step:grad_" + kind]).reshape(g["grad_" + kind].shape), g["grad_" + kind])
        worst = max(worst, r)
        assert r <= 1e-12, f"{name} hand-written backward, {kind}: {r:.2e}"
    print(f"[bound] fixture {name}: worst relative distance of {len(got)} quantities and the hand-written backward {worst:.2e}")


def test_key_table_equals_the_references():
    """tests/golden/midas_dpt_large_keys.json: state_dict() names and shapes of the reference's DPTDepthModel(backbone="vitl16_384") on the
    meta device over a full-size timm stand-in (tools/gen_midas_golden.py)"""
    import json
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "midas_dpt_large_keys.json")) as f:
        table = {k: tuple(v) for k, v in json.load(f).items()}
    assert table == E.reference_state_dict_shapes(E.DPT_CONFIGS["dpt_large"])
