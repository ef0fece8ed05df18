"""CPU: the float64 restatements of tests/_losses_ref64.py equal the reference's own values (tests/golden/losses_reference.npz, written
by tools/gen_losses_golden.py); each bound of tests/test_gpu_losses.py accepts an fp32 CPU evaluation of the same formula with 4x room and
rejects seeded defects, at that test's inputs; the loss classes exist with the reference's signatures; the argument guards return before
any launch; the product refuses CPU tensors.
"""
import ctypes as C
import inspect

import pytest
import torch

import _losses_ref64 as R
import test_gpu_losses as T
from conftest import golden

ROOM = 0.25          # an fp32 CPU evaluation must sit at or below a quarter of every bound


def _rejected(tag, ok):
    print(f"[defect] {tag}: {'accepted' if ok else 'rejected'}")
    assert not ok, f"{tag}: the bound accepts this defect"


def _close(a, b, rel=1e-12):
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    return bool(((a - b).abs() <= rel * b.abs().max()).all())


# ---- the restatements are the reference's arithmetic -----------------------------------------------------------------------------------
def test_head_restatements_equal_the_reference_values():
    g = golden("losses_reference")
    emb, n = g["head_emb"], g["head_emb"].shape[0]
    out, loss, demb = R.head_eval(emb, g["sim_w"], g["sim_b"], 0, float(g["sim_target"]), n, float(g["sim_multiplier"]), 1.0)
    assert _close(out, g["sim_ratings"]) and _close(loss, g["sim_loss"]) and _close(demb, g["sim_demb"])
    la, da = R.head_loss_autograd64(emb, g["sim_w"], g["sim_b"], 0, float(g["sim_target"]), n, float(g["sim_multiplier"]))
    assert _close(la, g["sim_loss"]) and _close(da, g["sim_demb"])
    for mode, name in ((1, "logit"), (2, "expected"), (3, "probability")):
        out, loss, demb = R.head_eval(emb, g["ava_w"], g["ava_b"], mode, int(g["ava_target"]), n, 1.0, 1.0)
        assert _close(out, g["ava_logits"]), name
        assert _close(loss, g[f"ava_{name}_loss"]) and _close(demb, g[f"ava_{name}_demb"]), name
        la, da = R.head_loss_autograd64(emb, g["ava_w"], g["ava_b"], mode, int(g["ava_target"]), n, 1.0)
        assert _close(la, g[f"ava_{name}_loss"]) and _close(da, g[f"ava_{name}_demb"]), name
    # n_total and gscale scale as documented
    _, l2, d2 = R.head_eval(emb, g["ava_w"], g["ava_b"], 2, int(g["ava_target"]), 2 * n + 1, 1.7, 65536.0)
    assert _close(l2, g["ava_expected_loss"] * 1.7 * n / (2 * n + 1)) and _close(d2, g["ava_expected_demb"] * 1.7 * 65536.0 * n / (2 * n + 1))


def test_smoothness_and_sqdiff_restatements_equal_the_reference_values():
    g = golden("losses_reference")
    x = g["smooth_x"]
    loss, grad, _ = R.smoothness_eval(x, x.shape[0], 1.0)
    assert _close(loss, g["smooth_loss"]) and _close(grad, g["smooth_grad"])
    a, b = g["sq_a"], g["sq_b"]
    loss, ga, gb = R.sqdiff_eval(a, b, a.numel())
    assert _close(loss, g["sq_loss"]) and _close(ga, g["sq_grad_a"]) and _close(gb, g["sq_grad_b"])
    # losses.Resize through the product's fp32 band tables: the tables are fp32, so this holds to the tables' precision only
    size = tuple(int(v) for v in g["resize_size"])
    ra, rb = R.resize64(g["resize_a"], size), R.resize64(g["resize_b"], size)
    loss, _, _ = R.sqdiff_eval(ra, rb, ra.numel())
    assert abs(float(loss) - float(g["resize_loss"])) <= R.resize_loss_tol(g["resize_a"], g["resize_b"], size)[0]


# ---- the bounds accept fp32, with room, and reject defects ------------------------------------------------------------------------------
@pytest.mark.parametrize("D", T.HEAD_D)
@pytest.mark.parametrize("N", T.HEAD_N)
@pytest.mark.parametrize("mode", [0, 1, 2, 3])
def test_head_bounds_accept_fp32_and_reject_defects(mode, N, D):
    (emb, W, b), combos = T.head_cases(mode, N, D)
    mult = T.HEAD_MULT[mode]
    K = W.shape[0]
    worst = [0.0, 0.0, 0.0]
    for target, n_total, gscale in combos:
        args = (emb, W, b, mode, target, n_total, mult, gscale)
        ref = R.head_eval(*args)
        tol = R.head_tol(*args)
        f32 = R.head_eval(*args, dtype=torch.float32)
        for i in range(3):
            worst[i] = max(worst[i], R.worst(f32[i], ref[i], tol[i]))
        ok = lambda got: [R.within(got[i], ref[i], tol[i]) for i in range(3)]
        tag = f"{R.MODE_NAMES[mode]} N={N} D={D} target={target} n_total={n_total} gscale={gscale:g}"
        if mode == 0:
            bad = ok(R.head_eval(*args, defect="no_sqrt_d"))
            _rejected(f"mode 0 without sqrt(D), {tag}", bad[0] or bad[2])
        if mode == 2:
            _rejected(f"mode 2 sums the K terms before squaring, {tag}", ok(R.head_eval(*args, defect="sum_before_square"))[1])
        if mode in (1, 3) and target < K:
            bad = ok(R.head_eval(*args, defect="index_without_minus_1"))
            _rejected(f"target used as an index without the -1, {tag}", bad[1] or bad[2])
        if n_total != N:
            bad = ok(R.head_eval(*args, defect="n_for_n_total"))
            _rejected(f"n in place of n_total, {tag}", bad[1] or bad[2])
    print(f"[fp32-cpu] head {R.MODE_NAMES[mode]} N={N} D={D}: out {worst[0]:.3e} loss {worst[1]:.3e} demb {worst[2]:.3e} of the bound")
    assert max(worst) <= ROOM


@pytest.mark.parametrize("case", T.SMOOTH_CASES, ids=str)
def test_smoothness_bounds_accept_fp32_and_reject_defects(case):
    shape, n_total = case
    x = R.smoothness_input(shape, sum(shape))
    for gscale in (1.0, 65536.0):
        l64, g64, _ = R.smoothness_eval(x, n_total, gscale)
        l_tol, g_tol = R.smoothness_tol(x, n_total, gscale)
        l32, g32, _ = R.smoothness_eval(x, n_total, gscale, dtype=torch.float32)
        wl, wg = R.worst(l32.reshape(1), l64.reshape(1), l_tol), R.worst(g32, g64, g_tol)
        print(f"[fp32-cpu] smoothness {shape} gscale={gscale:g}: loss {wl:.3e} grad {wg:.3e} of the bound")
        assert wl <= ROOM and wg <= ROOM
        bad = R.smoothness_eval(x, n_total, gscale, defect="both_over_hw")
        _rejected(f"smoothness divides both sums by H W, {shape}", R.within(bad[0].reshape(1), l64.reshape(1), l_tol))
        for d in ("grad_misses_last_row", "grad_misses_last_col"):
            _rejected(f"smoothness {d}, {shape}", R.within(R.smoothness_eval(x, n_total, gscale, defect=d)[1], g64, g_tol))


@pytest.mark.parametrize("count", T.SQDIFF_COUNTS)
def test_sqdiff_bounds_accept_fp32_and_reject_defects(count):
    a, b = R.sqdiff_inputs(count, count)
    for n_total_count in (count, 3 * count):
        l64, ga64, gb64 = R.sqdiff_eval(a, b, n_total_count)
        l_tol, g_tol = R.sqdiff_tol(a, b, n_total_count)
        l32, ga32, gb32 = R.sqdiff_eval(a, b, n_total_count, dtype=torch.float32)
        wl, wg = R.worst(l32.reshape(1), l64.reshape(1), l_tol), max(R.worst(ga32, ga64, g_tol), R.worst(gb32, gb64, g_tol))
        print(f"[fp32-cpu] sqdiff count={count} n_total_count={n_total_count}: loss {wl:.3e} g {wg:.3e} of the bound")
        assert wl <= ROOM and wg <= ROOM
        _rejected(f"sqdiff b-gradient sign flipped, count={count}", R.within(R.sqdiff_eval(a, b, n_total_count, defect="b_gradient_sign")[2], gb64, g_tol))
        if n_total_count != count:
            _rejected(f"sqdiff count in place of n_total_count, count={count}", R.within(R.sqdiff_eval(a, b, count)[0].reshape(1), l64.reshape(1), l_tol))


# ---- the public surface ------------------------------------------------------------------------------------------------------------------
def _params(fn):
    return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()
            if p.kind is p.POSITIONAL_OR_KEYWORD and p.name != "self"]


def test_classes_exist_with_the_reference_signatures():
    from perceptor_amd import losses, models
    E = inspect.Parameter.empty
    assert _params(losses.SimulacraAesthetic.__init__) == [("model_name", "ViT-L-14"), ("aesthetic_target", 10)]
    assert _params(losses.AestheticVisualAssessment.__init__) == [("aesthetic_target", 10), ("mode", "expected")]
    assert _params(losses.Resize.__init__) == [("size", None)]
    assert _params(losses.SphericalDistance.__init__) == [("model", E)]
    assert _params(models.SimulacraAesthetic.__init__) == [("model_name", "ViT-B-32")]
    assert _params(losses.Smoothness.forward) == [("images", E)] and _params(losses.SimulacraAesthetic.forward) == [("images", E)]
    assert _params(losses.AestheticVisualAssessment.forward) == [("images", E)] and _params(models.SimulacraAesthetic.forward) == [("images", E)]
    assert _params(losses.Resize.forward) == [("images_a", E), ("images_b", E), ("size", None)]
    assert _params(losses.SphericalDistance.forward) == [("images_a", E), ("images_b", E)]
    for cls in (losses.SimulacraAesthetic, losses.AestheticVisualAssessment):
        kwonly = [p.name for p in inspect.signature(cls.__init__).parameters.values() if p.kind is p.KEYWORD_ONLY]
        assert kwonly == ["model", "checkpoint", "seed"]
    for cls in (losses.SimulacraAesthetic, losses.AestheticVisualAssessment, losses.Smoothness, losses.Resize, losses.SphericalDistance):
        assert issubclass(cls, losses.LossInterface) and callable(getattr(cls, "loss_and_grad"))
    assert callable(losses.tower_loss_and_grad)


def test_vit_l_14_336_is_configured():
    from perceptor_amd.engine import text, vit
    assert vit.VIT_CONFIGS["ViT-L-14-336"] == (336, 14, 1024, 24, 16, 768)
    assert text.TEXT_CONFIGS["ViT-L-14-336"] == text.TEXT_CONFIGS["ViT-L-14"]
    assert vit.vit_state_dict_shapes(vit.VIT_CONFIGS["ViT-L-14-336"])["positional_embedding"] == (577, 1024)


def _tiny_tower(name):
    from perceptor_amd import models
    return models.OpenCLIP(name, "synthetic", quick_gelu=True, config=T.VIT_TINY)


def test_multipliers_heads_and_checkpoints(tmp_path):
    from perceptor_amd import losses
    tower = _tiny_tower("losses-cpu-tiny")
    dim = T.VIT_TINY[5]
    assert losses.SimulacraAesthetic("ViT-L-14", model=tower).multiplier == 1e-5
    assert losses.SimulacraAesthetic("ViT-L-14-336", model=tower).multiplier == 1e-5
    sim = losses.SimulacraAesthetic("ViT-B-32", 7, model=tower)
    assert sim.multiplier == 1e-3 and sim.model is tower and float(sim.aesthetic_target) == 7.0
    assert sim.aesthetic_model.linear.weight.shape == (1, dim)
    again = losses.SimulacraAesthetic("ViT-B-32", 7, model=tower)
    assert torch.equal(again.aesthetic_model.linear.weight, sim.aesthetic_model.linear.weight)          # the synthetic head is deterministic
    assert not torch.equal(losses.SimulacraAesthetic("ViT-B-32", model=tower, seed=1).aesthetic_model.linear.weight, sim.aesthetic_model.linear.weight)
    w1, b1 = torch.randn(1, dim), torch.randn(1)
    torch.save({"linear.weight": w1, "linear.bias": b1}, tmp_path / "sim.pth")
    sim = losses.SimulacraAesthetic("ViT-B-32", model=tower, checkpoint=str(tmp_path / "sim.pth"))
    assert torch.equal(sim.aesthetic_model.linear.weight, w1) and torch.equal(sim.aesthetic_model.linear.bias, b1)
    w10, b10 = torch.randn(10, dim), torch.randn(10)
    torch.save({"weight": w10, "bias": b10}, tmp_path / "ava.pth")
    ava = losses.AestheticVisualAssessment(3, "logit", model=tower, checkpoint=str(tmp_path / "ava.pth"))
    assert torch.equal(ava.aesthetic_head.weight, w10) and torch.equal(ava.aesthetic_head.bias, b10) and ava.model is tower
    with pytest.raises(RuntimeError):
        losses.AestheticVisualAssessment(model=tower, checkpoint=str(tmp_path / "sim.pth"))                # the other head's keys
    with pytest.raises(ValueError):
        losses.AestheticVisualAssessment(mode="median", model=tower)._head()


def test_tower_loss_and_grad_refuses_different_towers():
    from perceptor_amd import losses
    a, b = _tiny_tower("losses-cpu-a"), _tiny_tower("losses-cpu-b")
    t1, t2 = losses.SimulacraAesthetic("x", model=a), losses.AestheticVisualAssessment(model=b)
    with pytest.raises(ValueError):
        losses.tower_loss_and_grad(torch.zeros(1, 3, 32, 32), [t1, t2])
    with pytest.raises(TypeError):
        losses.tower_loss_and_grad(torch.zeros(1, 3, 32, 32), [t1, losses.Smoothness()])


def test_losses_refuse_cpu_tensors():
    from perceptor_amd import losses
    img = torch.rand(1, 3, 32, 32)
    tower = _tiny_tower("losses-cpu-tiny")
    with pytest.raises(RuntimeError):
        losses.Smoothness()(img)
    with pytest.raises(RuntimeError):
        losses.Smoothness().loss_and_grad(img)
    with pytest.raises(RuntimeError):
        losses.Resize((16, 16))(img, img)
    with pytest.raises(RuntimeError):
        losses.SimulacraAesthetic("x", model=tower).loss_and_grad(img)
    with pytest.raises(RuntimeError):
        losses.AestheticVisualAssessment(model=tower)(img)
    with pytest.raises(RuntimeError):
        losses.SphericalDistance(tower).loss_and_grad(img, img)
    with pytest.raises(RuntimeError):
        losses.tower_loss_and_grad(img, [losses.SimulacraAesthetic("x", model=tower)])


def test_argument_guards_return_before_any_launch():
    """no GPU here: a guard that let one of these through would reach a launch and fail differently"""
    import os
    from perceptor_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):           # a fresh tree: build as tests/test_abi.py does
        from perceptor_amd.csrc import build
        build.build()
    lib = _hip.lib()
    buf = (C.c_float * 4096)()
    p = C.cast(buf, C.c_void_p)
    assert lib.pmi_smoothness(p, p, p, p, 1, 3, 1, 8, 1, 1.0, None) == -1          # H < 2: the reference yields NaN
    assert lib.pmi_smoothness(p, p, p, p, 1, 3, 8, 1, 1, 1.0, None) == -1          # W < 2
    assert lib.pmi_smoothness(p, p, p, p, 2, 3, 8, 8, 1, 1.0, None) == -1          # n_total < N
    assert lib.pmi_smoothness(p, None, p, p, 1, 3, 8, 8, 1, 1.0, None) == -1
    assert lib.pmi_sqdiff_loss(p, p, p, p, p, 0, 0, None) == -1
    assert lib.pmi_sqdiff_loss(p, p, p, p, p, 8, 7, None) == -1                    # n_total_count < count
    assert lib.pmi_sqdiff_loss(p, p, p, p, None, 8, 8, None) == -1
    assert lib.pmi_head_loss(p, p, p, p, p, p, p, 1, 17, 64, 1, 1.0, 1, 1.0, 1.0, None) == -1      # K > 16
    assert lib.pmi_head_loss(p, p, p, p, p, p, p, 1, 10, 4097, 1, 1.0, 1, 1.0, 1.0, None) == -1    # D > 4096
    assert lib.pmi_head_loss(p, p, p, p, p, p, p, 1, 10, 64, 4, 1.0, 1, 1.0, 1.0, None) == -1      # mode out of range
    assert lib.pmi_head_loss(p, p, p, p, p, p, p, 1, 10, 64, 3, 0.0, 1, 1.0, 1.0, None) == -1      # class 0
    assert lib.pmi_head_loss(p, p, p, p, p, p, p, 1, 10, 64, 1, 2.5, 1, 1.0, 1.0, None) == -1      # a class is an integer
    assert lib.pmi_head_loss(p, p, p, p, p, p, p, 1, 2, 64, 0, 5.0, 1, 1.0, 1.0, None) == -1       # mode 0 is a K = 1 probe
    assert lib.pmi_head_loss(p, p, p, p, p, p, p, 3, 1, 64, 0, 5.0, 2, 1.0, 1.0, None) == -1       # n_total < N
    assert not any(buf)
