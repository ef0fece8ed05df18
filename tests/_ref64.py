"""float64 references, error scales and defect models shared by the kernel-level attention / transformer tests.

Every reference here is float64 torch (autograd for gradients) on operands already rounded to the 16-bit compute type.
`u` is the unit roundoff of that type (half an ulp at 1): rounding a value x to it moves x by at most u * |x|.

The attention bounds are worst-case sums of the roundings the kernels perform, each written out elementwise in float64:
  out = P V          P is rounded to 16 bit before P.V:                    |err| <= u (|O| + P |V|)
  dV  = P^T dO       P rounded to 16 bit:                                  |err| <= u (|dV| + P^T |dO|)
  dS  = P (dP - delta) scale, rounded to 16 bit before the dQ / dK products; delta = rowsum(dO * O) comes from the 16-bit O
                     (flash backward) or from the 16-bit P (split backward):  |err dS| <= u E_dS,
                     E_dS = |dS| + scale P (|dP - delta| + P|dP| + |dO|.|O|)
  dQ  = dS K, dK = dS^T Q:                                                 |err| <= u (|dQ| + E_dS |K|), u (|dK| + E_dS^T |Q|)
A test asserts max|got - ref| <= c u max(scale term) with c = 1.5: the extra half covers the fp32 accumulation, the hardware exp and the
second-order products of the roundings above, none of which reaches u.
"""
from __future__ import annotations

import math

import torch

U = {"f16": 2.0 ** -11, "bf16": 2.0 ** -8}
TD = {"f16": torch.float16, "bf16": torch.bfloat16}
C_ATTN = 1.5


def rnd(x: torch.Tensor, dtype: str) -> torch.Tensor:
    """x rounded to the 16-bit type, returned as float64."""
    return x.to(TD[dtype]).double()


def max_err(got, ref) -> float:
    return float((got.double().cpu() - ref.double().cpu()).abs().max()) if ref.numel() else 0.0


def parity(tag: str, err: float, tol: float) -> None:
    print(f"[parity] {tag}: err {err:.3e} tol {tol:.3e} ratio {err / tol if tol > 0 else 0.0:.3f}")


def check(tag: str, got, ref, tol: float) -> float:
    err = max_err(got, ref)
    parity(tag, err, tol)
    assert err <= tol, f"{tag}: max err {err:.4e} > tol {tol:.4e}"
    return err


# ---- attention ------------------------------------------------------------------------------------------------------
def attn_ref(q, k, v, dout=None, scale=None, causal=False):
    """softmax(scale q k^T) v on [B, T, d] / [B, Tk, d] float64 tensors; gradients by float64 autograd when dout is given.
    Returns the outputs and the elementwise error scales of the module docstring."""
    scale = scale if scale is not None else q.shape[-1] ** -0.5
    q, k, v = (z.detach().double().clone().requires_grad_(dout is not None) for z in (q, k, v))
    with torch.enable_grad():
        s = scale * q @ k.transpose(-1, -2)
        if causal:
            t, tk = s.shape[-2:]
            s = s.masked_fill(torch.ones(t, tk, dtype=torch.bool).triu(1), float("-inf"))
        s.retain_grad() if dout is not None else None
        p = torch.softmax(s, dim=-1)
        p.retain_grad() if dout is not None else None
        o = p @ v
        r = dict(O=o.detach(), P=p.detach(), lse=torch.logsumexp(s.detach(), dim=-1))
        r["sO"] = float((o.detach().abs() + p.detach() @ v.detach().abs()).max())
        if dout is None:
            return r
        o.backward(dout.double())
    P, dP, dS = p.detach(), p.grad, s.grad
    dO = dout.double()
    delta = (P * dP).sum(-1, keepdim=True)
    absdot = (dO.abs() * o.detach().abs()).sum(-1, keepdim=True)
    e_ds = dS.abs() + scale * P * ((dP - delta).abs() + (P * dP.abs()).sum(-1, keepdim=True) + absdot)
    Q, K, V = q.detach(), k.detach(), v.detach()
    r.update(dQ=q.grad, dK=k.grad, dV=v.grad, dS=dS, dP=dP)
    r["sdQ"] = float((q.grad.abs() + e_ds @ K.abs()).max())
    r["sdK"] = float((k.grad.abs() + e_ds.transpose(-1, -2) @ Q.abs()).max())
    r["sdV"] = float((v.grad.abs() + P.transpose(-1, -2) @ dO.abs()).max())
    return r


def attn_tol(r, key: str, dtype: str) -> float:
    return C_ATTN * U[dtype] * r["s" + key]


def score_bias(T: int, regime: str) -> torch.Tensor:
    """Target score offset per key for the structured regimes: 'last' puts each query's largest score on the last key and rises over
    every key (so each key tile raises the running maximum), steeply over the last ~16 keys; 'first' is its mirror (the maximum in the
    first key tile, every later tile below it).  Scores span [-16, 0]: a padded key with score 0 would compete with the top keys."""
    s = torch.arange(T, dtype=torch.float64)
    dist = (T - 1 - s) if regime == "last" else s
    return -torch.minimum(0.75 * dist, 8.0 + 8.0 * dist / max(T, 1))


def attn_inputs(B: int, T: int, d: int, regime: str, dtype: str, seed: int, Tk: int = None, scale: float = None):
    """q [B, T, d], k / v [B, Tk, d] float64, rounded to the 16-bit type, in one of four score regimes:
    flat (|scale q.k| ~ 0.3), peaked (|scale q.k| ~ 3: near one-hot rows), last / first (score_bias)."""
    Tk = Tk or T
    scale = scale if scale is not None else d ** -0.5
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(B, Tk, d, generator=g, dtype=torch.float64)
    if regime in ("flat", "peaked"):
        sig = (0.3 if regime == "flat" else 3.0) ** 0.5 / (scale * d ** 0.5) ** 0.5
        q = sig * torch.randn(B, T, d, generator=g, dtype=torch.float64)
        k = sig * torch.randn(B, Tk, d, generator=g, dtype=torch.float64)
    else:
        u = torch.randn(B, 1, d, generator=g, dtype=torch.float64)
        u = u / u.norm(dim=-1, keepdim=True)
        a = 8.0
        q = a * u + 0.1 * torch.randn(B, T, d, generator=g, dtype=torch.float64)
        k = (score_bias(Tk, regime)[None, :, None] / (a * scale)) * u + 0.1 * torch.randn(B, Tk, d, generator=g, dtype=torch.float64)
    return rnd(q, dtype), rnd(k, dtype), rnd(v, dtype)


def _softmax_out(s, v):
    return torch.softmax(s, -1) @ v


def defect_outputs(q, k, v, dout, scale, tile=32):
    """float64 outputs of plausible kernel defects (B, T, d tensors).  Each entry: (output name, defect value)."""
    T, Tk = q.shape[1], k.shape[1]
    s = scale * q @ k.transpose(-1, -2)
    r = attn_ref(q, k, v, dout, scale)
    out = {}
    # the last key dropped from the softmax
    out["last key dropped"] = ("O", _softmax_out(s[..., :Tk - 1], v[:, :Tk - 1]) if Tk > 1 else torch.zeros_like(r["O"]))
    # one zero-padded key (score 0, value 0) included -- only where T is not a whole number of tiles
    if Tk % tile:
        sp = torch.cat([s, torch.zeros_like(s[..., :1])], -1)
        vp = torch.cat([v, torch.zeros_like(v[:, :1])], 1)
        out["padded key included"] = ("O", _softmax_out(sp, vp))
    # the online rescale alpha skipped: each key tile weighted against the running maximum of its own step
    num = torch.zeros_like(r["O"])
    den = torch.zeros_like(r["O"][..., :1])
    m = torch.full_like(den, -math.inf)
    for j in range(0, Tk, tile):
        sj = s[..., j:j + tile]
        m = torch.maximum(m, sj.max(-1, keepdim=True).values)
        e = torch.exp(sj - m)
        num = num + e @ v[:, j:j + tile]
        den = den + e.sum(-1, keepdim=True)
    out["alpha rescale skipped"] = ("O", num / den)
    if dout is not None:
        P, dP = r["P"], r["dP"]
        out["delta taken as 0 in dQ"] = ("dQ", (P * dP * scale) @ k)
        out["dK and dV swapped"] = ("dK", r["dV"])
        dq = r["dQ"].clone()
        dq[:, T - 1] = 0
        out["last query row's gradients zeroed"] = ("dQ", dq)
    return r, out


# ---- transformer pieces ---------------------------------------------------------------------------------------------
def act_ref(x: torch.Tensor, act: int) -> torch.Tensor:
    import torch.nn.functional as F
    from perceptor_amd._hip import ACT_GELU, ACT_QUICKGELU, ACT_RELU, ACT_SILU
    if act == ACT_RELU:
        return F.relu(x)
    if act == ACT_SILU:
        return F.silu(x)
    if act == ACT_GELU:
        return F.gelu(x)
    if act == ACT_QUICKGELU:
        return x * torch.sigmoid(1.702 * x)
    raise ValueError(act)


def act_grad_ref(x: torch.Tensor, act: int) -> torch.Tensor:
    x = x.double().detach().clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(act_ref(x, act).sum(), x)
    return g
