"""Shared by oracle/gen_golden.py (gen_fullsize), tools/gen_fullsize_floor64.py and the full-size reference tests: which positions of a
full-size UNet output the fixtures keep, how a test rebuilds the (unstored) input, and the comparison the GPU test applies.

Sampling.  A fault confined to a tile edge (the last column of a 32-wide tile, a halo row) is invisible to a lattice whose stride divides the
tile size: y[:, :, ::32, ::32] only ever reads positions = 0 mod 32.  The fixtures keep, for every output channel,

  * a lattice from offset 0 with a stride coprime to every power-of-two tile size (3 at 256 px, 7 at 512 px): its positions run through
    every residue mod 64 on both axes (test_fullsize_golden_cpu.py asserts that);
  * the full first and last two rows and columns (image borders: padding, halo loads);
  * moments and float64 per-channel sums of the WHOLE output (gross faults off the sampled positions: see compare).
"""
import torch

STRIDE = {256: 3, 512: 7}
BORDER = 2


def border_index(n):
    return list(range(BORDER)) + list(range(n - BORDER, n))


def sample(y, stride):
    """y [N, C, H, W] -> {"lat", "rows", "cols"}: lattice, first / last two rows, first / last two columns"""
    h, w = y.shape[-2:]
    return {"lat": y[..., ::stride, ::stride].contiguous(), "rows": y[..., border_index(h), :].contiguous(),
            "cols": y[..., :, border_index(w)].contiguous()}


def sampled_vector(y, stride):
    """the sampled positions of y [N, C, H, W] as one [N, C, K] tensor (lattice, rows, columns in this order)"""
    s = sample(y, stride)
    return torch.cat([s[k].flatten(2) for k in ("lat", "rows", "cols")], dim=2)


def fixture_vector(g, prefix="y_"):
    return torch.cat([g[prefix + k].flatten(2) for k in ("lat", "rows", "cols")], dim=2)


def sampled_positions(n, stride):
    """sorted positions along an axis of length n that the fixture reads on at least one full line of the other axis"""
    return sorted(set(range(0, n, stride)) | set(border_index(n)))


def moments(y):
    f = y.flatten(1).double()
    return torch.stack([f.mean(1), f.std(1), f.norm(dim=1)], dim=1).float()


def channel_sums(y):
    return y.double().sum((2, 3))


def checksum(x):
    d = x.double()
    return torch.stack([d.sum(), d.abs().sum()])


def rebuild(shape, seed, want):
    """seeded_noise(shape, seed), asserted to be the tensor the fixture was generated from (float64 sum and abs-sum)"""
    from perceptor_amd.utils.synth import seeded_noise
    x = seeded_noise(tuple(int(v) for v in shape), int(seed))
    got = checksum(x)
    assert torch.allclose(got, want.double(), rtol=1e-12, atol=1e-9), ("rebuilt input differs from the fixture's", got, want)
    return x


def compare(got, g, stride, tag, bound_abs, ref_prefix="y_"):
    """The full-size comparison: `got` [1, C, H, W] (the fixture chain's output) against fixture `g` at the sampled positions, and its
    float64 channel sums against the fixture's.  bound_abs is the absolute bound on a sampled element.

    Whole-output figures (a second line behind the sampled positions, which carry the element-wise contract): std and norm of the output
    against the fixture's moments at rtol 5e-2, as test_gpu_clip.py compares moments, and the channel sums at n * bound_abs, n the
    element count -- what the element bound implies for a sum with no assumption on how errors combine.  A sqrt(n) bound (independent
    errors) does not hold for a correct implementation: rounding errors of a UNet forward are spatially coherent (an error in a deep
    low-resolution layer is up-sampled into a smooth field, a GroupNorm statistic shifts a channel), and the fp32 reference's own channel
    sums differ from the float64 ones by 50-160 x what independent errors of size F would give (F_sum in tests/golden/*_floor64.npz).
    The measured sum error is printed for the record.
    Returns (max|err|, scale, rel-L2) and prints the [parity] line before asserting."""
    got = got.detach().float().cpu()
    ref = fixture_vector(g, ref_prefix).double()
    vec = sampled_vector(got, stride).double()
    err, scale = float((vec - ref).abs().max()), float(ref.abs().max())
    l2 = float((vec - ref).norm() / ref.norm())
    n = got.shape[2] * got.shape[3]
    serr = float((channel_sums(got) - g["ch_sum"].double()).abs().max())
    sbound = bound_abs * n
    mom, want = moments(got)[:, 1:].double(), g["y_mom"][:, 1:].double()
    print(f"[parity] {tag}: max|err|={err:.3e} (scale {scale:.3f}), rel-L2={l2:.3e}, max|channel-sum err|={serr:.3e} (bound {sbound:.3e}, n={n})")
    assert bool(torch.isfinite(got).all()), tag
    assert err < bound_abs, (tag, err, bound_abs, scale)
    assert serr < sbound, (tag, serr, sbound)
    assert torch.allclose(mom, want, rtol=5e-2, atol=0), (tag, mom, want)
    return err, scale, l2
