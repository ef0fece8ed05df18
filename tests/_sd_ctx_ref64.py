"""TEST INFRASTRUCTURE -- the SD UNet's gradient with respect to the prompt encodings (the `context`) by torch autograd of
tests/_sd_unet_ref64.py's unet_forward, and a torch restatement of the split key role of csrc/attn_flash.hip (pmi_attn_flash_bwd_kv).
Pinned by tests/test_sd_ctx_grad_cpu.py."""
import torch

import _sd_unet_ref64 as R


def joint_grad(sd32, cfg, x, timesteps, context, cot, dtype=torch.float64):
    """(eps, d <eps, cot> / d x, d <eps, cot> / d context) in `dtype` on the fp32 master weights.  A context of batch 1 is broadcast over
    the samples inside the graph, as upstream's call does: its gradient is the sum over the samples, shape [1, Tk, D]."""
    w = {k: v.to(dtype) for k, v in sd32.items()}
    xx = x.to(dtype).clone().requires_grad_()
    cc = context.to(dtype).clone().requires_grad_()
    eps = R.unet_forward(w, cfg, xx, timesteps, cc.expand(x.shape[0], -1, -1))
    eps.backward(cot.to(dtype))
    return eps.detach(), xx.grad.detach(), cc.grad.detach()


def kv_chunks(n, t, tk, heads):
    """(S, L) of csrc/attn_flash.hip's flash_kv_chunks: chunks per key tile and query tiles per chunk, from the shape alone."""
    ntq, ntk = (t + 31) // 32, (tk + 31) // 32
    waves = ntk * n * heads
    want = max(1, min((2048 + waves - 1) // waves, ntq // 4))
    L = (ntq + want - 1) // want
    return (ntq + L - 1) // L, L


def kv_split_backward(q, k, v, d_out, scale, chunks, tile=32):
    """Restatement of the split key role for one head: q [T, d], k / v [Tk, d], d_out [T, d] -> (dk, dv, S used).  32-key tiles, the
    query tiles cut into `chunks` chunks of L tiles (S = ceil(ntq / L) of them are non-empty), P from the exp2-domain log-sum-exp, padded
    keys and padded queries given weight 0, one partial tile per (key tile, chunk), the partials added in chunk order."""
    t, tk, d = q.shape[0], k.shape[0], q.shape[1]
    sl2 = scale * 1.4426950408889634
    s2 = (q @ k.T) * sl2
    lse = torch.log2(torch.exp2(s2 - s2.max(1, keepdim=True).values).sum(1)) + s2.max(1).values
    out = torch.exp2(s2 - lse[:, None]) @ v
    delta = (d_out * out).sum(1)
    ntq, ntk = (t + tile - 1) // tile, (tk + tile - 1) // tile
    pad = lambda a, rows: torch.cat([a, a.new_zeros((rows - a.shape[0],) + tuple(a.shape[1:]))], 0)
    qp, dop, lsep, dlp = pad(q, ntq * tile), pad(d_out, ntq * tile), pad(lse, ntq * tile), pad(delta, ntq * tile)
    kp, vp = pad(k, ntk * tile), pad(v, ntk * tile)
    L = (ntq + chunks - 1) // chunks
    S = (ntq + L - 1) // L
    dk, dv = q.new_zeros((ntk * tile, d)), q.new_zeros((ntk * tile, d))
    for kt in range(ntk):
        ks, vs = kp[kt * tile:(kt + 1) * tile], vp[kt * tile:(kt + 1) * tile]
        key_ok = (torch.arange(tile) + kt * tile) < tk
        parts = []
        for ch in range(S):
            gk, gv = q.new_zeros((tile, d)), q.new_zeros((tile, d))
            for tb in range(ch * L, min(ntq, (ch + 1) * L)):
                r = slice(tb * tile, (tb + 1) * tile)
                p = torch.exp2((qp[r] @ ks.T) * sl2 - lsep[r, None])
                p = p * key_ok[None, :] * ((torch.arange(tile) + tb * tile) < t)[:, None]
                ds = p * (dop[r] @ vs.T - dlp[r, None]) * scale
                gv += p.T @ dop[r]
                gk += ds.T @ qp[r]
            parts.append((gk, gv))
        ak, av = parts[0]
        for gk, gv in parts[1:]:
            ak, av = ak + gk, av + gv
        dk[kt * tile:(kt + 1) * tile], dv[kt * tile:(kt + 1) * tile] = ak, av
    return dk[:tk], dv[:tk], S
