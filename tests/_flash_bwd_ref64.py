"""float64 model, per-element bounds, fp32 emulation, defect models and the case lists of the flash attention backward
(csrc/attn_flash.hip: pmi_attn_flash_bwd, pmi_attn_flash_bwd_kv), shared by tests/test_gpu_flash_backward.py and
tests/test_flash_backward_bounds_cpu.py.

For 16-bit operands q, k, v, dO and scale = d^-0.5, in float64 (tests/_ref64.py derives the error scale):
  P = softmax(scale q k^T), O = P v, dP = dO v^T, delta = rowsum(dO * O), dS = scale P (dP - delta), dQ = dS k, dK = dS^T q, dV = P^T dO
  E_dS = |dS| + scale P (|dP - delta| + sum_s P|dP| + sum_c |dO||O|)        the last term: delta is formed from the 16-bit O
Bounds per output element, u the unit roundoff of the type, C = 1.5 (R.C_ATTN), no fitted constant:
  dQ: C (u (|dQ| + E_dS |k|)   + sub (sum_s |k[s, c]| + 1))
  dK: C (u (|dK| + E_dS^T |q|) + sub (sum_t |q[t, c]| + 1))
  dV: C (u (|dV| + P^T |dO|)   + sub (sum_t |dO[t, c]| + 1))
sub = 2^-25 for f16 (half the f16 subnormal spacing: once per rounded P or dS term of the sum, once for the output), 0 for bf16.
The fp32 dK / dV of pmi_attn_flash_bwd_kv have no output rounding: the u |dK|, u |dV| terms and the + 1 go, and the fp32 chain (one
accumulator update per query tile, S - 1 additions in the reduce, the MFMA's own sums) adds C (T / 32 + S + 3) 2^-24 times the same
magnitude sums E_dS^T |q| and P^T |dO|.
  lse (natural log): 2^-19 (1 + max |scale |q| |k|^T| + max |lse|); pad rows exactly 0.
  delta: against float64 sum_c dO * O16 on the kernel's own 16-bit output, C d 2^-24 sum_c |dO * O16| per row (products of two 16-bit
  values are exact in fp32); pad rows exactly 0.
"""
from __future__ import annotations

import math

import torch

import _ref64 as R

LOG2E = 1.4426950408889634
SUB = {"f16": 2.0 ** -25, "bf16": 0.0}
TILE = 32

FLASH_D = [8, 16, 24, 40, 64, 72, 80, 96, 104, 128, 136, 160]      # (KQ, DB) = (ceil(d/16), ceil(d/32)): all ten instantiations
DTYPES = ["f16", "bf16"]

# ---- the cases: (d, T, Tk, N, H, regime) ----------------------------------------------------------------------------------------------
# self-attention (dq_only = 0): every head dim on two tiles with one live row in the second; then the single row, a partial single tile,
# three and four tiles and the whole-tile shape, with workgroup counts (T tiles + Tk tiles) x N x H that are no multiple of 8
SELF_CASES = [(d, 33, 33, 2, 3, "last") for d in FLASH_D] + \
    [(d, T, T, N, H, reg) for d in (40, 64, 160)
     for T, N, H, reg in ((1, 1, 1, "flat"), (31, 1, 5, "peaked"), (65, 1, 1, "first"), (97, 2, 3, "peaked"), (64, 1, 1, "last"))]
# cross-attention (dq_only = 1, and the kv form with one chunk)
CROSS_CASES = [(d, 33, 77, 2, 3, "last") for d in FLASH_D] + \
    [(d, T, Tk, N, H, reg) for d in (40, 160) for T, Tk, N, H in ((64, 7, 1, 5), (100, 33, 2, 2)) for reg in ("peaked", "first")]
# the kv form split over query chunks: (d, T, Tk, N, H, regime) -> the S of flash_kv_chunks
KV_SPLIT_CASES = [(d, T, Tk, N, H, reg) for d in (24, 64, 160)
                  for T, Tk, N, H, reg in ((257, 77, 1, 2, "last"), (385, 33, 1, 1, "peaked"), (417, 7, 2, 1, "first"))]
KV_SPLIT_S = {(257, 77): 2, (385, 33): 3, (417, 7): 3}      # chunks of 5 + 4, 5 + 5 + 3 and 5 + 5 + 4 query tiles
# f16 with dO scaled by 2^-14: dS and every output are subnormal.  family -> case
SUBNORMAL_CASES = {"self": (64, 97, 97, 2, 3, "peaked"), "cross": (40, 100, 33, 2, 2, "first"), "kv": (64, 257, 77, 1, 2, "last")}
# the training forward's lse through each forward kernel: (d, T, N, H, regime, pmi_set_option(9, .))
LSE_CASES = [(d, T, 2, 3, reg, qt) for d in (40, 64) for T, reg in ((33, "last"), (65, "first")) for qt in (0, 1, 2)] + \
    [(40, 2049, 1, 1, "last", 0)]      # 65 query tiles: the automatic rule takes the LDS kernel from 64


def kv_chunks(N, T, Tk, H, cap=0):
    """flash_kv_chunks of csrc/attn_flash.hip: (S, L); cap = pmi_set_option(14, .)"""
    ntq, ntk = (T + 31) // 32, (Tk + 31) // 32
    waves = ntk * N * H
    want = min((2048 + waves - 1) // waves, ntq // 4)
    if cap > 0:
        want = min(want, cap)
    want = max(want, 1)
    L = (ntq + want - 1) // want
    return (ntq + L - 1) // L, L


def last_channel_heavy(q, k):
    """channel d-1 of q and k scaled up (its product alone moves a score by ~1): a dropped last channel of a partial k-step shows"""
    q, k = q.clone(), k.clone()
    q[..., -1] = q[..., -1].sign() * 2.0 + q[..., -1]
    k[..., -1] = k[..., -1] * 4.0
    return q, k


def operands(case, dtype, do_scale=1.0):
    """q [B, T, d], k, v [B, Tk, d], dO [B, T, d] float64 on the 16-bit grid, B = N * H (sample-major)"""
    d, T, Tk, N, H, regime = case
    q, k, v = R.attn_inputs(N * H, T, d, regime, dtype, seed=1000 * d + 10 * T + Tk, Tk=Tk)
    q, k = last_channel_heavy(q, k)
    q, k = R.rnd(q, dtype), R.rnd(k, dtype)
    g = torch.Generator().manual_seed(d + T + 1)
    dO = R.rnd(torch.randn(N * H, T, d, generator=g, dtype=torch.float64) * do_scale, dtype)
    return q, k, v, dO


def model(q, k, v, dO, dtype, fp32_kv=False, S=1):
    """The float64 outputs and the per-element bounds of the module docstring: dict with P, O, dP, delta, dS, dQ, dK, dV, lse (natural
    log), bQ, bK, bV (tensors shaped like dQ, dK, dV) and blse (a number)."""
    T, d = q.shape[-2:]
    scale = d ** -0.5
    u, sub, C = R.U[dtype], SUB[dtype], R.C_ATTN
    s = scale * q @ k.transpose(-1, -2)
    P = torch.softmax(s, -1)
    O = P @ v
    dP = dO @ v.transpose(-1, -2)
    delta = (dO * O).sum(-1, keepdim=True)
    dS = scale * P * (dP - delta)
    e_ds = dS.abs() + scale * P * ((dP - delta).abs() + (P * dP.abs()).sum(-1, keepdim=True) + (dO.abs() * O.abs()).sum(-1, keepdim=True))
    r = dict(P=P, O=O, dP=dP, delta=delta.squeeze(-1), dS=dS, E_dS=e_ds, dQ=dS @ k, dK=dS.transpose(-1, -2) @ q, dV=P.transpose(-1, -2) @ dO,
             lse=torch.logsumexp(s, -1))
    mk, mv = e_ds.transpose(-1, -2) @ q.abs(), P.transpose(-1, -2) @ dO.abs()
    r["bQ"] = C * (u * (r["dQ"].abs() + e_ds @ k.abs()) + sub * (k.abs().sum(-2, keepdim=True) + 1))
    if fp32_kv:
        chain = C * (T / 32 + S + 3) * 2.0 ** -24
        r["bK"] = C * (u * mk + sub * q.abs().sum(-2, keepdim=True)) + chain * mk
        r["bV"] = C * (u * mv + sub * dO.abs().sum(-2, keepdim=True)) + chain * mv
    else:
        r["bK"] = C * (u * (r["dK"].abs() + mk) + sub * (q.abs().sum(-2, keepdim=True) + 1))
        r["bV"] = C * (u * (r["dV"].abs() + mv) + sub * (dO.abs().sum(-2, keepdim=True) + 1))
    smax = float((q.abs() @ k.abs().transpose(-1, -2)).max()) * scale
    r["blse"] = 2.0 ** -19 * (1.0 + smax + float(r["lse"].abs().max()))
    return r


def ratio(got, ref, bound) -> float:
    """max over the elements of |got - ref| / bound (inf where an element with bound 0 differs)"""
    err = (got.double() - ref).abs()
    bound = bound.expand_as(err) if torch.is_tensor(bound) else torch.full_like(err, bound)
    rt = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, math.inf, 0.0))
    return float(rt.max()) if rt.numel() else 0.0


def check(tag, got, ref, bound) -> float:
    rt = ratio(got, ref, bound)
    print(f"[parity] {tag}: max err {R.max_err(got, ref):.3e} err/bound {rt:.3f}")
    assert rt <= 1.0, f"{tag}: err/bound {rt:.3f}"
    return rt


def delta_bound(dO, o16, d):
    """(float64 delta of the kernel's own 16-bit output [B, T], its bound [B, T])"""
    pr = dO * o16.double()
    return pr.sum(-1), R.C_ATTN * d * 2.0 ** -24 * pr.abs().sum(-1)


# ---- fp32 emulation of the kernels' arithmetic ----------------------------------------------------------------------------------------------
def emulate(q, k, v, dO, dtype, fp32_kv=False):
    """fp32 throughout, with the kernels' roundings: the forward's P rounded before P v and O rounded once; delta from that O; the
    backward's P = exp2(S scale log2e - lse) rounded before P^T dO, dS rounded before its two products, the outputs rounded once (the
    kv form's dK / dV not at all)."""
    td = R.TD[dtype]
    r16 = lambda x: x.to(td).float()
    d = q.shape[-1]
    scale = torch.tensor(d ** -0.5, dtype=torch.float32)
    sl2 = scale * torch.tensor(LOG2E, dtype=torch.float32)
    q, k, v, dO = (z.float() for z in (q, k, v, dO))
    z = (q @ k.transpose(-1, -2)) * sl2
    m = z.amax(-1, keepdim=True)
    pu = torch.exp2(z - m)
    l = pu.sum(-1, keepdim=True)
    lse = m + torch.log2(l)
    o16 = r16((r16(pu) @ v) / l)
    delta = (dO * o16).sum(-1, keepdim=True)
    P = torch.exp2(z - lse)
    dS16 = r16(P * (dO @ v.transpose(-1, -2) - delta) * scale)
    dQ, dK, dV = dS16 @ k, dS16.transpose(-1, -2) @ q, r16(P).transpose(-1, -2) @ dO
    if not fp32_kv:
        dK, dV = r16(dK), r16(dV)
    return dict(dQ=r16(dQ), dK=dK, dV=dV, lse=lse.squeeze(-1) / LOG2E, delta=delta.squeeze(-1), O16=o16)


# ---- defect models ------------------------------------------------------------------------------------------------------------------
def trunc16(x, dtype):
    """x moved towards zero onto the 16-bit grid"""
    y = R.rnd(x, dtype)
    td = R.TD[dtype]
    over = y.abs() > x.abs()
    return torch.where(over, torch.nextafter(y.to(td), torch.zeros_like(y).to(td)).double(), y)


def defects(q, k, v, dO, N, H, S=1, L=0):
    """float64 outputs of plausible defects of the backward kernels: name -> {output name: defect value}.  A defect that cannot occur at
    the shape (or leaves every output as it is there) is not listed."""
    B, T, d = q.shape
    Tk = k.shape[1]
    scale = d ** -0.5
    r = model(q, k, v, dO, "bf16")
    P, dP, dS, delta = r["P"], r["dP"], r["dS"], r["delta"].unsqueeze(-1)
    grads = lambda ds, p=P: dict(dQ=ds @ k, dK=ds.transpose(-1, -2) @ q, dV=p.transpose(-1, -2) @ dO)
    out = {}
    if Tk > 1:      # one key: dP = delta and dS = 0 whatever delta is
        out["delta taken as 0"] = {n: g for n, g in grads(scale * P * dP).items() if n != "dV"}
        out["scale missing from dS"] = {n: g for n, g in grads(dS / scale).items() if n != "dV"}
        k0 = (Tk - 1) // TILE * TILE
        out["last key tile dropped from dQ"] = dict(dQ=dS[..., :k0] @ k[:, :k0])
    out["dK and dV swapped"] = dict(dK=r["dV"], dV=r["dK"])
    t0 = (T - 1) // TILE * TILE
    out["last query tile dropped from dK and dV"] = dict(dV=P[:, :t0].transpose(-1, -2) @ dO[:, :t0])
    if Tk > 1:
        out["last query tile dropped from dK and dV"]["dK"] = dS[:, :t0].transpose(-1, -2) @ q[:, :t0]
    if S > 1:
        t1 = (S - 1) * L * TILE
        out["last chunk's partial dropped by the reduce"] = dict(dK=dS[:, :t1].transpose(-1, -2) @ q[:, :t1], dV=P[:, :t1].transpose(-1, -2) @ dO[:, :t1])
    if B > 1:      # P = exp(S - lse) with the lse of the next (sample, head)
        s = scale * q @ k.transpose(-1, -2)
        Pn = torch.exp(s - r["lse"].roll(-1, 0).unsqueeze(-1))
        out["lse of the neighbouring (sample, head)"] = grads(scale * Pn * (dP - delta), Pn)
    if d % 16:     # the scores without channel d - 1; lse is the forward's
        Pc = torch.exp(scale * q[..., :d - 1] @ k[..., :d - 1].transpose(-1, -2) - r["lse"].unsqueeze(-1))
        out["last channel of the partial k-step dropped from the scores"] = grads(scale * Pc * (dP - delta), Pc)
    if N > 1 and Tk > 1:
        out["delta of the other sample"] = {n: g for n, g in grads(scale * P * (dP - delta.roll(H, 0))).items() if n != "dV"}
    return r, out


def margins(case, defect_fn=defects, **kw):
    """{defect: {output: deviation / bf16 bound}} at one case"""
    d, T, Tk, N, H, regime = case
    q, k, v, dO = operands(case, "bf16")
    r, out = defect_fn(q, k, v, dO, N, H, **kw)
    return {name: {o: ratio(val, r[o], r["b" + o[1]]) for o, val in outs.items()} for name, outs in out.items()}
