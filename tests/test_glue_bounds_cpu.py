"""CPU: the restatements of tests/_glue_ref64.py can fail -- each seeded defect is rejected by the very bound function the GPU test of
tests/test_gpu_glue_kernels.py asserts, at that test's inputs; the host tables of the resize against the reference's own outputs; the
argument guards that return before any launch; and every entry point of include/perceptor_hip.h is tested by name.
"""
import ctypes as C
import glob
import inspect
import os
import re

import numpy as np
import pytest
import torch

import _glue_ref64 as R
import test_gpu_glue_kernels as T
from test_abi import _header_decls

HERE = os.path.dirname(os.path.abspath(__file__))


def _rejected(tag, ok):
    print(f"[defect] {tag}: {'accepted' if ok else 'rejected'}")
    assert not ok, f"{tag}: the bound accepts this defect"


# ---- the references can fail -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("case", T.PATCH_CASES, ids=str)
def test_defect_patchify_py_px_swapped(case, dtype):
    N, Rr, P, Kp = case
    img, mean, std = T.patchify_inputs(case)
    ref = R.patchify64(img, mean, std, P, Kp)
    good = ref.to(R.TORCH16[dtype])                                      # a correctly rounded result passes
    assert R.within(good, ref, R.patchify_tol(ref, dtype))
    _rejected(f"patchify py/px swapped {case} {dtype}",
              R.within(R.patchify64(img, mean, std, P, Kp, swap_pypx=True).to(R.TORCH16[dtype]), ref, R.patchify_tol(ref, dtype)))


@pytest.mark.parametrize("case", T.PATCH_CASES, ids=str)
def test_defect_unpatchify_std0(case):
    N, Rr, P, Kp = case
    dcol, std, mul = T.unpatchify_inputs(case)
    ref = R.unpatchify64(dcol, std, N, Rr, P, mul)
    assert R.within(ref.float(), ref, R.unpatchify_tol(ref))
    _rejected(f"unpatchify divides by std[0] {case}",
              R.within(R.unpatchify64(dcol, std, N, Rr, P, mul, std0_everywhere=True).float(), ref, R.unpatchify_tol(ref)))


@pytest.mark.parametrize("chw", [c for c in T.CHW])
def test_defect_lincomb_sample_index(chw):
    a, b, ca, cb, cc = T.lincomb_inputs(chw)
    for with_b in (False, True):
        for with_cc in (False, True):
            args = (a, b if with_b else None, ca, cb, cc if with_cc else None, chw)
            ref, mag = R.lincomb64(*args)
            assert R.within(ref.float(), ref, R.lincomb_tol(mag))
            _rejected(f"lincomb n = i // (chw + 1), chw {chw} b {with_b} cc {with_cc}",
                      R.within(R.lincomb64(*args, bad_sample_index=True)[0].float(), ref, R.lincomb_tol(mag)))


@pytest.mark.parametrize("n", [n for n in T.QUANT_N if n > 1])
def test_defect_quantile_ceil_for_lower(n):
    x = R.quantile_rows(n, 40 + n)
    hit = 0
    for q in (0.5, 0.95):
        a, b, w, ref = R.quantile_parts(x, q)
        assert R.quantile_ok(torch.lerp(a, b, float(np.float32(w))), a, b, w, ref)
        if w == 0:
            continue                                                     # an integer rank: floor = ceil
        bad = R.quantile_parts(x, q, ceil_for_lower=True)[3].float()
        _rejected(f"quantile lower statistic at ceil, n {n} q {q}", R.quantile_ok(bad, a, b, w, ref))
        hit += 1
    assert hit


@pytest.mark.parametrize("heads", [1, 3])
def test_defect_qkv_order_ignored(heads):
    qkv = R.counter16((2, 33, 3 * heads * 64))
    want = R.qkv_split_ref(qkv, heads, 1)
    bad = R.qkv_split_ref(qkv, heads, 0)
    if heads == 1:                                                       # one head: (head, which, d) and (which, head, d) coincide
        assert all(torch.equal(a, b) for a, b in zip(want, bad))
        return
    _rejected("qkv layout with order ignored", all(torch.equal(a, b) for a, b in zip(want, bad)))
    for buf in want:                                                     # and the pad rows t >= T are zero in the restatement itself
        assert int((buf != 0).sum()) == 2 * heads * 33 * 64


@pytest.mark.parametrize("dtype", T.DTYPES)
def test_defect_cast_truncates(dtype):
    x = R.cast_specials(dtype)
    keep = ~x.isnan()
    good, bad = R.cast16_bits(x, dtype), R.cast16_bits(x, dtype, truncate=True)
    ties_up = (good != bad) & keep
    assert int(ties_up.sum()) >= 3, "the inputs hold no tie that rounds to the even neighbour above"
    _rejected(f"cast truncates {dtype}", torch.equal(good[keep], bad[keep]))


@pytest.mark.parametrize("case", T.BAND_CASES, ids=str)
def test_defect_resize_border_tap_dropped(case):
    from perceptor_amd.transforms.resize import band_tables
    in_sz, out_sz, method = case
    idx, w, _, _ = band_tables(in_sz, out_sz, method)
    x = T.band_input((6, in_sz, 5), in_sz + 2)
    ref, absum = R.band_apply(x, idx, w)
    tol = R.band_tol(absum, idx.shape[1])
    assert R.within(ref.float(), ref, tol)
    _rejected(f"resize with a border tap dropped {case}", R.within(R.band_apply(x, idx, w, drop_border_tap=True)[0].float(), ref, tol))


def test_defect_resize_hand_table_tap_dropped():
    (outer, in_sz, inner, out_sz, taps), idx, w = T.hand_tables(0)
    x = T.band_input((outer, in_sz, inner), 72) * 2 - 1
    ref, absum = R.band_apply(x, idx, w)
    _rejected("hand table with a border tap dropped",
              R.within(R.band_apply(x, idx, w, drop_border_tap=True)[0].float(), ref, R.band_tol(absum, taps)))


@pytest.mark.parametrize("power", [1, 2])
@pytest.mark.parametrize("n", [n for n in T.WASS_N if n > 1])
def test_defect_wasserstein_unit_linspace(n, power):
    srt = R.wasserstein_rows(n, 60 + n).sort(1)[0]
    tol, err = R.wasserstein_tol(srt, power)
    ref = float(R.wasserstein64(srt, power))
    print(f"[reference] wasserstein n {n} power {power}: |ref32 - ref64| = {err:.3e}, ref64 = {ref:.6g}, bound = {tol:.3e}")
    assert err <= tol
    bad = float(R.wasserstein64(srt, power, unit_linspace=True))
    _rejected(f"wasserstein against linspace(0, 1, n), n {n} power {power}", abs(bad - ref) <= tol)


def test_wasserstein_reference_error_is_recorded():
    """the figures in test_wasserstein's docstring and DESIGN.md are the reference's fp32 expression against float64 at the test's rows"""
    for n in T.WASS_N:
        for power in (1, 2):
            srt = R.wasserstein_rows(n, 60 + n).sort(1)[0]
            tol, err = R.wasserstein_tol(srt, power)
            print(f"[reference] wasserstein n {n} power {power}: |ref32 - ref64| = {err:.3e} (ref64 {float(R.wasserstein64(srt, power)):.6g})")
            assert err <= 1e-6


# ---- resize: the host tables against the reference's own outputs ----------------------------------------------------------------------
def _dense_resize(img, target):
    """perceptor_amd.transforms.resize.resize with band_tables applied as dense float64 operators"""
    from perceptor_amd.transforms.resize import _plan, band_tables
    x = img.double()
    method, dims = _plan(x.shape[2], x.shape[3], target)
    for _, axis, i, o in dims:
        idx, w, _, _ = band_tables(i, o, method)
        A = R.dense_band(idx, w, i)[0]
        x = torch.einsum("jr,ncrw->ncjw", A, x) if axis == 2 else torch.einsum("jr,nchr->nchj", A, x)
    return x


@pytest.mark.parametrize("tag,shape,target", T.RESIZE2, ids=[c[0] for c in T.RESIZE2])
def test_dense_tables_match_reference_fixture(load_golden, tag, shape, target):
    from perceptor_amd.utils.synth import seeded_noise
    want = load_golden("clip_resize2")["rz_" + tag]
    got = _dense_resize(seeded_noise(shape, 51) * 0.25 + 0.5, target)
    assert got.shape == want.shape
    err = float((got - want.double()).abs().max())
    print(f"[resize] {tag}: dense float64 tables vs the reference, max abs {err:.3e}")
    assert err <= 1e-6


@pytest.mark.parametrize("case", T.BAND_CASES + [(75, 32, "cubic"), (64, 63, "cubic"), (64, 65, "cubic"), (225, 224, "lanczos3")], ids=str)
def test_transposed_tables_are_the_exact_transpose(case):
    from perceptor_amd.transforms.resize import band_tables
    in_sz, out_sz, method = case
    idx, w, idx_t, w_t = band_tables(in_sz, out_sz, method)
    A, At = R.dense_band(idx, w, in_sz)[0], R.dense_band(idx_t, w_t, out_sz)[0]
    assert torch.equal(At, A.t())


# ---- argument guards: refused before any launch -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from perceptor_amd import _hip
    if not os.path.exists(_hip.LIB_PATH):
        from perceptor_amd.csrc import build
        build.build()
    L = C.CDLL(_hip.LIB_PATH)
    for name, (args,) in _hip._PROTOS.items():
        getattr(L, name).argtypes = args
        getattr(L, name).restype = C.c_int
    return L


def test_argument_guards(lib):
    """only calls that must be refused: every one returns PMI_ERR_ARG (-1) from the host guard; the pointers are never dereferenced"""
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    assert lib.pmi_vit_assemble(p, p, p, p, 2, 1, 4, 0, None) == -1
    assert lib.pmi_vit_assemble(p, p, p, p, 2, 0, 4, 0, None) == -1
    assert lib.pmi_patchify(p, p, p, p, 2, 28, 14, 590, 0, 0, None) == -1             # Kp % 8
    assert lib.pmi_patchify(p, p, p, p, 2, 28, 8, 192, 0, 0, None) == -1              # R % P
    assert lib.pmi_patchify(p, p, p, p, 2, 28, 14, 584, 0, 0, None) == -1             # Kp < 3 P^2
    for R_, P_, Kp in ((28, 0, 592), (0, 14, 592), (-28, 14, 592), (28, -14, 592), (28, 14, 587), (28, 14, 0), (28, 8, 192)):
        assert lib.pmi_unpatchify(p, p, p, 2, R_, P_, Kp, 1.0, None) == -1, (R_, P_, Kp)
    assert lib.pmi_unpatchify(p, p, p, 0, 28, 14, 592, 1.0, None) == -1
    for c in (4, 40):
        for to_split in (0, 1):
            assert lib.pmi_split_convert(p, p, 1, c, to_split, None) == -1
    for q in (-0.1, 1.5, float("nan")):
        assert lib.pmi_quantile_abs(p, p, 3, 8, q, None) == -1
    assert lib.pmi_quantile_abs(p, p, 3, 0, 0.5, None) == -1
    for n in (0, -1, 2 ** 30 + 1):
        assert lib.pmi_sort_rows_padded(n) == -1
        assert lib.pmi_sort_rows(p, p, 3, n, None) == -1
    for n in (1, 2, 4095, 4096, 4097, 8193):
        assert lib.pmi_sort_rows_padded(n) == max(4096, 1 << (n - 1).bit_length())
    assert lib.pmi_wasserstein(p, 3, 8, 3, p, p, None) == -1
    assert lib.pmi_qkv_split(p, p, p, p, 1, 0, 1, 0, 0, None) == -1
    assert lib.pmi_qkv_split(p, p, p, p, 1, 8, 1, 2, 0, None) == -1
    assert lib.pmi_gather_rows(p, p, p, 3, 20, 19, 9, None) == -1                      # ld < D
    assert lib.pmi_embed_tokens(p, p, None, p, 1, 7, 8, 0, None) == -1


# ---- every entry point is tested by name ------------------------------------------------------------------------------------------
# Entry points that no GPU test calls by name: the wrapper that calls them and the GPU test file that uses the wrapper.
VIA_WRAPPER = {
    "pmi_gemm_f32": ("ops.gemm_f32", "test_gpu_precise_kernels.py"),
    "pmi_geglu_bwd": ("ops.geglu_backward", "test_gpu_sd_unet_grad.py"),
}
# Queries answered on the host without a launch: a CPU test file may name them instead.
HOST_ONLY = re.compile(r"^pmi_(abi_version|\w+_workspace|\w+_chunks|\w+_eligible|igemm_splitk|igemm_stats_rows|sort_rows_padded|"
                       r"gn1_bwd_partials|conv3x3_halo_config)$")


def _read(paths):
    return "".join(open(p).read() for p in paths)


def uncovered(names, gpu_src, cpu_src, via_wrapper):
    return [n for n in names
            if not re.search(rf"\b{n}\b", gpu_src) and n not in via_wrapper
            and not (HOST_ONLY.match(n) and re.search(rf"\b{n}\b", cpu_src))]


def test_every_entry_point_is_tested_by_name():
    names = list(_header_decls())
    assert len(names) >= 90
    gpu_files = sorted(glob.glob(os.path.join(HERE, "test_gpu_*.py")))
    cpu_files = [p for p in sorted(glob.glob(os.path.join(HERE, "test_*.py"))) if p not in gpu_files]
    gpu_src, cpu_src = _read(gpu_files), _read(cpu_files)
    missing = uncovered(names, gpu_src, cpu_src, VIA_WRAPPER)
    assert not missing, f"entry points no test calls by name: {missing}"
    # a prototype added later without a test makes this fail
    assert uncovered(names + ["pmi_not_yet_tested"], gpu_src, cpu_src, VIA_WRAPPER) == ["pmi_not_yet_tested"]
    # the table holds only what it must, and each entry is what it says
    from perceptor_amd.engine import ops
    for name, (wrapper, test_file) in VIA_WRAPPER.items():
        assert name in names, f"{name} is no entry point any more"
        assert not re.search(rf"\b{name}\b", gpu_src), f"{name} is named by a GPU test now: drop it from VIA_WRAPPER"
        mod, fn = wrapper.split(".")
        assert mod == "ops"
        assert re.search(rf'"{name}"', inspect.getsource(getattr(ops, fn))), f"{wrapper} does not call {name}"
        assert re.search(rf"\bops\.{fn}\(", open(os.path.join(HERE, test_file)).read()), f"{test_file} does not use {wrapper}"
