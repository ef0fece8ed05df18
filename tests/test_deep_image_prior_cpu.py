"""CPU: tests/_dip_ref64.py against the reference module's own values (tests/golden/deep_image_prior_reference.npz, written by
tools/gen_deep_image_prior_golden.py), the planted faults against the tolerances the GPU tests use, state-dict parity, the host-side
argument checks and parameter_dicts.  No GPU: nothing here launches a kernel."""
import functools

import numpy as np
import pytest
import torch

import _dip_ref64 as D
from conftest import golden
from perceptor_amd.engine import dip as E


@functools.lru_cache(maxsize=None)
def _gold():
    return golden("deep_image_prior_reference")


@functools.lru_cache(maxsize=None)
def _ref(case):
    return D.run_case64(case)


def _close(a, b):
    b = b.double()
    return bool(((a.double() - b).abs() <= 1e-12 * (1 + b.abs())).all())


@pytest.mark.parametrize("case", D.CASES, ids=D.case_name)
def test_restatement_equals_the_reference(case):
    g, c = _gold(), D.case_name(case)
    out, dl, grads, stats = _ref(case)
    assert _close(out, g[c + "/out"])
    assert _close(dl[:, ::4], g[c + "/dlatents4"]) and _close(D.contraction("latents", dl)[0], g[c + "/dlatents_dot"])
    assert {k for k in g if k.startswith(c + "/stat/") and not k.endswith("num_batches_tracked")} == {c + "/stat/" + k for k in stats}
    for k, v in stats.items():
        assert _close(v, g[c + "/stat/" + k]), k
    for k in g:
        if k.startswith(c + "/stat/") and k.endswith("num_batches_tracked"):
            assert int(g[k]) == 4                                    # the synthetic 3, one training forward
    seen = 0
    for k, v in grads.items():
        if c + "/grad/" + k in g:
            assert v.numel() <= D.SMALL and _close(v, g[c + "/grad/" + k]), k
        else:
            s, smp = D.contraction(k, v)
            assert _close(s, g[c + "/dot/" + k]) and _close(smp, g[c + "/sample/" + k]), k
        seen += 1
    assert seen == sum(1 for k in g if k.startswith(c + "/grad/") or k.startswith(c + "/dot/"))
    for k in D.zero_gradient_names(grads):
        assert float(grads[k].abs().max()) < 1e-12, k               # analytically zero: the reference gives ~1e-15


@pytest.mark.parametrize("ns", [1, 2, 3])
def test_state_dict_parity(ns):
    from perceptor_amd import models
    g = _gold()
    size = {1: 8, 2: 16, 3: 24}[ns]
    m = models.DeepImagePrior(shape=(D.CIN, size, size), n_scales=ns)
    sd = m.state_dict()
    assert list(sd) == g["keys_s%d" % ns].tolist()
    assert [",".join(map(str, v.shape)) for v in sd.values()] == g["shapes_s%d" % ns].tolist()
    assert [str(v.dtype) for v in sd.values()] == g["dtypes_s%d" % ns].tolist()
    assert list(sd) == list(E.state_dict_shapes(ns, D.CIN))
    m.load_state_dict(E.synthetic_state_dict(ns, D.CIN), strict=True)
    assert all(isinstance(p, torch.nn.Parameter) and p.dtype == torch.float32 for p in m.parameters())
    # torch's own initialisation rules: BatchNorm gains 1, biases 0, running (0, 1); Conv2d's bound 1 / sqrt(fan_in)
    fresh = models.DeepImagePrior(shape=(D.CIN, size, size), n_scales=ns).state_dict()
    assert bool((fresh["network.2.weight"] == 1).all()) and not bool(fresh["network.2.bias"].any()) and bool((fresh["network.2.running_var"] == 1).all())
    w = fresh["network.3.1.weight"]
    assert float(w.abs().max()) <= (196 * 9) ** -0.5 and float(w.std()) > 0.4 * (196 * 9) ** -0.5
    assert torch.equal(fresh["network.10.colcorr_t"], E.colcorr_t()) and torch.equal(fresh["network.1.1.1.2.kernel"], E.cubic_kernels()[0])


def test_variants_build():
    from perceptor_amd import models
    m = models.DeepImagePrior(shape=(8, 16, 16), sigmoid=False, decorrelate_rgb=False, output_channels=4)
    assert "network.10.colcorr_t" not in m.state_dict() and m.state_dict()["network.9.1.weight"].shape == (4, 192, 1, 1)
    assert (m.input_channels, m.height, m.width) == (8, 16, 16) and m.device.type == "cpu"
    assert m.random_latents(2).shape == (2, 8, 16, 16) and m.fourier_latents(1).shape == (1, 8, 16, 16)
    assert m.noisy_image_latents(torch.rand(1, 3, 16, 16)).shape == (1, 8, 16, 16)


def test_argument_checks():
    from perceptor_amd import drawers, models
    for ot in ("1x1", "full"):
        with pytest.raises(NotImplementedError, match="torchvision.ops"):
            models.DeepImagePrior(shape=(8, 16, 16), offset_type=ot)
    with pytest.raises(ValueError):
        models.DeepImagePrior(shape=(8, 8, 8), n_scales=2)            # upstream's reflect padding fails here
    with pytest.raises(ValueError):
        models.DeepImagePrior(shape=(8, 16, 16), n_scales=3)          # and here
    with pytest.raises(AssertionError):
        models.DeepImagePrior(shape=(8, 16, 24))
    with pytest.raises(AssertionError):
        models.DeepImagePrior(shape=(8, 12, 12))
    with pytest.raises(ValueError):
        models.DeepImagePrior(shape=(8, 16, 16), n_scales=0)
    with pytest.raises(ValueError):
        models.DeepImagePrior(shape=(8, 16, 16), output_channels=5, decorrelate_rgb=False)
    with pytest.raises(ValueError):
        models.DeepImagePrior(shape=(8, 16, 16), output_channels=4)   # the colour matrix is 3 x 3
    with pytest.raises(ValueError):
        models.DeepImagePrior(shape=(8, 16, 16), dtype="precise")
    m = models.DeepImagePrior(shape=(8, 16, 16))
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 8, 16, 16))                                 # no CPU fallback
    with pytest.raises(ValueError):
        m(torch.zeros(1, 8, 32, 32))
    d = drawers.DeepImagePrior((16, 16), n_feature_channels=8)
    assert not d.latents.requires_grad and d.images.requires_grad and d.images.shape == (1, 3, 16, 16) and float(d.loss().detach()) == 0.0
    with torch.no_grad():
        d.images.fill_(-2.0)
    assert abs(float(d.loss().detach()) - 2e-4) < 1e-10


def test_library_refuses_bad_arguments():
    """the entry points check their arguments before any launch: each call below returns PMI_ERR_ARG (-1)"""
    from perceptor_amd import _hip
    L = _hip.lib()
    a = 4096                                                          # a non-null, aligned address that is never dereferenced
    assert L.pmi_dip_wgrad_splits(0, 4, 4, 1) == -1 and L.pmi_dip_wgrad_splits(16, 192, 64, 4) == -1
    assert L.pmi_dip_wgrad_splits(16, 192, 64, 9) == 1 and L.pmi_dip_wgrad_splits(16, 4, 192, 1) == 1
    assert 1 <= L.pmi_dip_wgrad_splits(65536, 192, 192, 9) <= 64
    assert L.pmi_dip_bn_blocks(16) == 1 and L.pmi_dip_bn_blocks(1 << 20) == 256 and L.pmi_dip_bn_blocks(0) == -1
    assert L.pmi_dip_wgrad(a, 192, 0, a, 64, 0, a, a, a, 1, 4, 4, 192, 64, 9, 1, 1.0, 1, None) == -1        # 9 taps need the ringed input
    assert L.pmi_dip_wgrad(a, 192, 1, a, 196, 1, a, a, a, 1, 4, 4, 192, 196, 9, 1, 1.0, 1, None) == -1      # pitch below the channels rounded to 8
    assert L.pmi_dip_wgrad(a, 192, 1, a, 64, 1, a, a, a, 1, 4, 4, 192, 64, 9, 7, 1.0, 1, None) == -1        # not the library's split count
    assert L.pmi_dip_bn_stats(a, 6, 0, a, a, a, None, None, 1, 4, 4, 6, 0.1, 1e-5, 1, None) == -1           # C % 4
    assert L.pmi_dip_bn_stats(a, 4, 0, a, a, a, None, None, 1, 1, 1, 4, 0.1, 1e-5, 1, None) == -1           # one sample has no unbiased variance
    assert L.pmi_dip_bn_apply(a, 4, 0, a, a, a, a, a, 4, 1, 1, 1, 4, 4, 0, 1, None) == -1                   # a ring needs two samples per axis
    assert L.pmi_dip_bn_apply(a, 4, 0, a, a, a, a, a, 4, 0, 1, 4, 4, 4, 2, 1, None) == -1                   # activation code
    assert L.pmi_fir8_down2(a, 0, a, 1, 6, 5, 8, 1, None) == -1 and L.pmi_fir8_down2(a, 0, a, 1, 2, 2, 8, 1, None) == -1
    assert L.pmi_fir8_up2(a, a, 1, 2, 2, 8, 1, None) == -1                                                  # reflect pad 2 needs 3 samples
    assert L.pmi_dip_head_fwd(a, a, a, a, a, 1, 16, 192, 4, 1, 1, None) == -1                               # the colour matrix with 4 channels
    assert L.pmi_dip_head_fwd(a, a, a, None, a, 1, 16, 190, 3, 1, 1, None) == -1
    assert L.pmi_dip_pack_w(a, a, None, 4, 8, 4, 4, 8, 8, 8, 1, None) == -1                                 # taps


def test_parameter_dicts():
    from perceptor_amd import models
    m = models.DeepImagePrior(shape=(8, 16, 16))
    groups = m.parameter_dicts(0.01)
    assert [g["lr"] for g in groups] == [0.001, 0.01] and groups[0]["params"] == [] and m.offset_parameters() == []
    assert len(groups[1]["params"]) == len(list(m.parameters())) == len(m.non_offset_parameters())
    torch.optim.Adam(groups[1:])                                      # (an empty group is what upstream hands over too; Adam takes the rest)


@functools.lru_cache(maxsize=None)
def _floors(case, dt):
    out, dl, grads, stats = _ref(case)
    eo, edl, eg, es = D.run_case64(case, emulate=dt)
    zero = set(D.zero_gradient_names(grads))
    fl = {"out": D.rel_l2(eo, out), "dlatents": D.rel_l2(edl, dl)}
    fl.update({k: D.rel_l2(es[k], stats[k]) for k in stats})
    fl.update({k: D.rel_l2(eg[k], grads[k]) for k in grads if k not in zero})
    return fl


@pytest.mark.parametrize("case", D.CASES, ids=D.case_name)
def test_planted_faults_fail_the_network_tolerance(case):
    """every fault that is visible in the whole network's values leaves at least one tensor outside floor x MARGIN, in both types"""
    out, dl, grads, stats = _ref(case)
    ns = case[0]
    prev = D.to64(E.synthetic_state_dict(ns, D.CIN, seed=1), grad=False)
    for defect in D.NETWORK_DEFECTS:
        bo, bdl, bg, bs = D.run_case64(case, defect=defect, conv_sd=prev)
        dev = {"out": D.rel_l2(bo, out), "dlatents": D.rel_l2(bdl, dl)}
        dev.update({k: D.rel_l2(bs[k], stats[k]) for k in stats})
        for dt in ("bf16", "f16"):
            fl = _floors(case, dt)
            dev.update({k: D.rel_l2(bg[k], grads[k]) for k in fl if k in grads})
            worst = max(dev[k] / (fl[k] * D.MARGIN[D.tensor_class(k)]) for k in fl)
            assert worst > 1.0, f"{defect} stays inside the {dt} tolerance at {D.case_name(case)} (worst {worst:.2f})"


def test_kernel_faults_are_switches():
    """the per-kernel faults change the operator they name (the GPU tests hold each against its kernel's bound) and nothing else"""
    torch.manual_seed(0)
    x, dy = torch.randn(2, 8, 8, 8, dtype=torch.float64), torch.randn(2, 8, 8, 8, dtype=torch.float64)
    gamma, beta = 1 + 0.1 * torch.randn(8, dtype=torch.float64), 0.1 * torch.randn(8, dtype=torch.float64)
    base = D.bn_bwd64(x, dy, gamma, beta, 1)
    y, _, _ = D.bn_train64(x.clone().requires_grad_(True), gamma, beta, True)
    xg = x.clone().requires_grad_(True)
    yg = D.bn_train64(xg, gamma, beta, True)[0]
    assert torch.allclose(torch.autograd.grad(yg, xg, dy)[0], base[0], rtol=1e-12, atol=1e-14)      # the explicit backward is autograd's
    for defect in ("bn_bwd_no_mean", "bn_bwd_no_xhat", "lrelu_bwd_slope_1", "lrelu_bwd_slope_0"):
        assert not torch.allclose(D.bn_bwd64(x, dy, gamma, beta, 1, defect)[0], base[0])
    for defect in ("lrelu_bwd_slope_1", "lrelu_bwd_slope_0"):                                        # not observable without the activation
        assert torch.equal(D.bn_bwd64(x, dy, gamma, beta, 0, defect)[0], D.bn_bwd64(x, dy, gamma, beta, 0)[0])
    w9 = D.wgrad64(dy, x, 9)
    xg = x.clone()
    wt = torch.zeros(8, 8, 3, 3, dtype=torch.float64, requires_grad=True)
    torch.autograd.grad(torch.nn.functional.conv2d(D.pad1(xg), wt), wt, dy)
    assert torch.allclose(torch.autograd.grad(torch.nn.functional.conv2d(D.pad1(xg), wt), wt, dy)[0], w9[0], rtol=1e-12, atol=1e-12)
    for defect in ("wgrad_kykx_swapped", "wgrad_no_ring"):
        assert not torch.allclose(D.wgrad64(dy, x, 9, defect)[0], w9[0])
        assert torch.equal(D.wgrad64(dy, x, 1, defect)[0], D.wgrad64(dy, x, 1)[0])                   # a 1x1 has neither taps nor a ring
    yu = torch.randn(2, 8, 16, 16, dtype=torch.float64)
    assert not torch.allclose(D.adjoint64(D.up64, x.shape, yu, "adjoint_no_folds"), D.adjoint64(D.up64, x.shape, yu))
    inner = (slice(None), slice(None), slice(3, 5), slice(3, 5))                                     # away from the border the folds add nothing
    assert torch.allclose(D.adjoint64(D.up64, x.shape, yu, "adjoint_no_folds")[inner], D.adjoint64(D.up64, x.shape, yu)[inner])
    assert set(D.NETWORK_DEFECTS) <= set(D.DEFECTS) and len(D.DEFECTS) == 14
