"""GPU: the LDS-resident route of pmi_vit_attn_fwd / pmi_vit_attn_bwd (csrc/attn.hip: head dim 64, Tp <= 288, one workgroup per image and
head, pmi_set_option key 17) against float64 torch on the same pre-rounded 16-bit operands.

References and bounds are those tests/test_gpu_attention.py part A holds the fragment-order route to (tests/_ref64.py: attn_ref, attn_tol,
the lse bound), unchanged.  Every buffer a call may write -- workspaces, lse, out, delta, dqkv -- is filled with NaN first, so a padded row
t >= T that contributed anything, or an element nobody wrote, shows as a NaN.

Which route a call took is read off the workspace: only the fragment-order route writes the transposed parts 3..5 of the forward workspace,
the backward workspace and delta; the LDS route leaves them as they were (NaN here).
"""
import contextlib

import pytest
import torch

import _ref64 as R

pytestmark = pytest.mark.gpu

DTYPES = ["f16", "bf16"]
REGIMES = ["flat", "peaked", "last", "first"]
LDS_T = [1, 31, 32, 33, 50, 197, 257, 288]      # tile edges, one row, ViT-B/32, ViT-B/16, ViT-L/14, the LDS limit
SHAPES = [(1, 1), (3, 3)]                        # (N, heads)
OPT_LDS = 17


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _heads_to_tokens(x, N, H):
    B, T, d = x.shape
    return x.view(N, H, T, d).permute(0, 2, 1, 3).reshape(N, T, H * d)


def _tokens_to_heads(x, N, H):
    N_, T, C = x.shape
    return x.reshape(N, T, H, C // H).permute(0, 2, 1, 3).reshape(N * H, T, C // H)


def _unfrag(part, T):
    """one rfrag-ordered workspace part [B, Tp, 64] (stored [B][Tp/32][k-step 4][half 2][row 32][8]) -> [B, Tp, 64] row-major"""
    B, tp = part.shape[:2]
    return part.reshape(B, tp // 32, 4, 2, 32, 8).permute(0, 1, 4, 2, 3, 5).reshape(B, tp, 64)


@contextlib.contextmanager
def _route(lds: bool):
    from perceptor_amd import _hip
    _hip.lib().pmi_set_option(OPT_LDS, int(lds))
    try:
        yield
    finally:
        _hip.lib().pmi_set_option(OPT_LDS, 1)


def _run(qkv, dout, N, T, H, dtype):
    """forward + backward as engine/ops.py issues them -> dict of every buffer the calls may write"""
    from perceptor_amd._hip import call, dtype_code, ptr
    dev, td = qkv.device, R.TD[dtype]
    tp32 = (T + 31) // 32 * 32
    scale = 64 ** -0.5
    b = dict(aws=_nan((6, N * H, tp32, 64), td, dev), lse=_nan((N * H, tp32), torch.float32, dev), out=_nan((N, T, H * 64), td, dev),
             bws=_nan((2, N * H, tp32, 64), td, dev), delta=_nan((N * H, tp32), torch.float32, dev), dqkv=_nan((N, T, 3 * H * 64), td, dev))
    call("pmi_vit_attn_fwd", ptr(qkv), ptr(b["aws"]), ptr(b["lse"]), ptr(b["out"]), N, T, H, scale, dtype_code(dtype))
    call("pmi_vit_attn_bwd", ptr(b["aws"]), ptr(b["lse"]), ptr(b["out"]), ptr(dout), ptr(b["bws"]), ptr(b["delta"]), ptr(b["dqkv"]), N, T, H,
         scale, dtype_code(dtype))
    torch.cuda.synchronize()
    return b


def _took_lds(b) -> bool:
    """the route of a _run: the transposed workspace parts, the backward workspace and delta are written by the fragment-order route only"""
    untouched = [bool(torch.isnan(z).all()) for z in (b["aws"][3:], b["bws"], b["delta"])]
    written = [bool(torch.isfinite(z).all()) for z in (b["aws"][3:], b["bws"], b["delta"])]
    assert all(untouched) or all(written), "forward and backward took different routes"
    return all(untouched)


_CACHE = {}


def _case(T, N, H, regime, dtype):
    """operands (float64 on the 16-bit grid, heads-major), device tensors and the float64 reference of one case, computed once"""
    key = (T, N, H, regime, dtype)
    if key not in _CACHE:
        td = R.TD[dtype]
        q, k, v = R.attn_inputs(N * H, T, 64, regime, dtype, seed=T * 7 + N * H)
        g = torch.Generator().manual_seed(T + 1)
        dO = R.rnd(torch.randn(N * H, T, 64, generator=g, dtype=torch.float64), dtype)
        qkv = torch.cat([_heads_to_tokens(z, N, H) for z in (q, k, v)], -1).to(td)
        dout = _heads_to_tokens(dO, N, H).to(td)
        _CACHE[key] = dict(q=q, k=k, v=v, dO=dO, qkv=qkv, dout=dout, ref=R.attn_ref(q, k, v, dO, 64 ** -0.5))
    return _CACHE[key]


def _check_values(tag, b, c, T, N, H, dtype):
    """out, lse, dqkv against float64 inside the bounds of test_gpu_attention.py part A"""
    out, lse, dqkv, r, q, k = b["out"], b["lse"], b["dqkv"], c["ref"], c["q"], c["k"]
    assert torch.isfinite(out).all() and torch.isfinite(dqkv).all() and torch.isfinite(lse).all(), f"{tag}: NaN / inf in an output"
    assert (lse[:, T:] == 0).all(), "lse rows t >= T must be written as 0"
    R.check(f"{tag} out", _tokens_to_heads(out.cpu(), N, H), r["O"], R.attn_tol(r, "O", dtype))
    dq, dk, dv = (_tokens_to_heads(z, N, H) for z in dqkv.cpu().split(H * 64, -1))
    R.check(f"{tag} dQ", dq, r["dQ"], R.attn_tol(r, "dQ", dtype))
    R.check(f"{tag} dK", dk, r["dK"], R.attn_tol(r, "dK", dtype))
    R.check(f"{tag} dV", dv, r["dV"], R.attn_tol(r, "dV", dtype))
    smax = float((q.abs() @ k.abs().transpose(-1, -2)).max()) * 64 ** -0.5
    R.check(f"{tag} lse", lse[:, :T].cpu(), r["lse"], 2.0 ** -19 * (1.0 + smax + float(r["lse"].abs().max())))


def _check_workspace(tag, b, c, T, N, H):
    """parts 0..2 of the forward workspace, un-fragmented, are the q, k, v slices of qkv bit for bit, with zero rows from T on"""
    for part, name in enumerate("qkv"):
        got = _unfrag(b["aws"][part], T).cpu()
        want = _tokens_to_heads(c["qkv"].split(H * 64, -1)[part], N, H)
        assert torch.equal(got[:, :T], want), f"{tag}: workspace part {name} differs from its qkv slice"
        assert (got[:, T:] == 0).all(), f"{tag}: workspace part {name} has non-zero padded rows"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H", SHAPES)
@pytest.mark.parametrize("T", LDS_T)
def test_lds_route_values_workspace_and_bits(T, N, H, dtype):
    dev = _dev()
    regime = REGIMES[(LDS_T.index(T) + N) % 4]
    c = _case(T, N, H, regime, dtype)
    qkv, dout = c["qkv"].to(dev), c["dout"].to(dev)
    tag = f"vit_attn_lds T={T} {N}x{H} {regime} {dtype}"
    b = _run(qkv, dout, N, T, H, dtype)
    assert _took_lds(b), f"{tag}: expected the LDS route"
    _check_values(tag, b, c, T, N, H, dtype)
    _check_workspace(tag, b, c, T, N, H)
    b2 = _run(qkv, dout, N, T, H, dtype)
    for n in ("out", "lse", "dqkv"):
        assert torch.equal(b[n], b2[n]), f"{tag}: two identical launches differ in {n}"
    if N == 3:      # nothing reduces across (image, head), and the route does not depend on N: image 0 alone gives the same bits
        b1 = _run(qkv[:1].contiguous(), dout[:1].contiguous(), 1, T, H, dtype)
        assert _took_lds(b1)
        assert torch.equal(b1["out"][0], b["out"][0]) and torch.equal(b1["dqkv"][0], b["dqkv"][0])
        assert torch.equal(b1["lse"], b["lse"][:H])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("regime", REGIMES)
def test_lds_route_score_regimes(regime, dtype):
    """T = 257 (9 key tiles, one live row in the last) in each score regime: flat, near one-hot, the maximum rising over every key tile (each
    tile rescales the running sums) and the maximum in the first tile"""
    dev = _dev()
    T, N, H = 257, 1, 3
    c = _case(T, N, H, regime, dtype)
    b = _run(c["qkv"].to(dev), c["dout"].to(dev), N, T, H, dtype)
    assert _took_lds(b)
    _check_values(f"vit_attn_lds regimes T={T} {regime} {dtype}", b, c, T, N, H, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_route_boundary(dtype):
    """T = 289 (Tp = 320) is past the LDS limit: the fragment-order route takes it, and passes"""
    dev = _dev()
    T, N, H = 289, 1, 3
    c = _case(T, N, H, "last", dtype)
    b = _run(c["qkv"].to(dev), c["dout"].to(dev), N, T, H, dtype)
    assert not _took_lds(b), "T = 289 must stay on the fragment-order route"
    tag = f"vit_attn T={T} {dtype} (fragment-order route)"
    _check_values(tag, b, c, T, N, H, dtype)
    _check_workspace(tag, b, c, T, N, H)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", LDS_T)
def test_option_off_takes_the_old_route(T, dtype):
    dev = _dev()
    N, H = 3, 3
    c = _case(T, N, H, REGIMES[(LDS_T.index(T) + N) % 4], dtype)
    with _route(False):
        b = _run(c["qkv"].to(dev), c["dout"].to(dev), N, T, H, dtype)
    assert not _took_lds(b), "option 17 = 0 must keep every shape on the fragment-order route"
    _check_values(f"vit_attn T={T} {dtype} (option off)", b, c, T, N, H, dtype)
