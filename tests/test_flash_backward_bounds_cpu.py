"""CPU side of tests/test_gpu_flash_backward.py: the bounds of tests/_flash_bwd_ref64.py hold an fp32 emulation of the flash backward's
arithmetic at every GPU case, the listed defects fall outside them, the case lists claim every (KQ, DB) instantiation, and the chunk
rule of the library (host-only queries) is the one the kv cases name."""
import pytest
import torch

import _flash_bwd_ref64 as FB
import _ref64 as R

REGIMES = ["flat", "peaked", "last", "first"]
FAMILIES = {"self": (FB.SELF_CASES, False), "cross dq_only": (FB.CROSS_CASES, False), "cross kv": (FB.CROSS_CASES + FB.KV_SPLIT_CASES, True)}
SHAPES = sorted({c[:5] for c in FB.SELF_CASES + FB.CROSS_CASES + FB.KV_SPLIT_CASES})


def _chunks(case):
    d, T, Tk, N, H = case[:5]
    return FB.kv_chunks(N, T, Tk, H) if T != Tk else (1, 0)


def _ratios(case, dtype, kv, do_scale=1.0):
    d, T, Tk, N, H, _ = case
    q, k, v, dO = FB.operands(case, dtype, do_scale)
    r = FB.model(q, k, v, dO, dtype, fp32_kv=kv, S=_chunks(case)[0] if kv else 1)
    e = FB.emulate(q, k, v, dO, dtype, fp32_kv=kv)
    out = {n: FB.ratio(e[n], r[n], r["b" + n[1]]) for n in ("dQ", "dK", "dV")}
    out["lse"] = FB.ratio(e["lse"], r["lse"], r["blse"])
    out["delta"] = FB.ratio(e["delta"], *FB.delta_bound(dO, e["O16"], d))
    return out


@pytest.mark.parametrize("dtype", FB.DTYPES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_fp32_emulation_stays_inside_every_bound(family, dtype):
    """The kernels' arithmetic in fp32 -- P rounded before P^T dO, dS rounded before its products, delta from the rounded O, outputs
    rounded once (the kv form's dK / dV not at all) -- at every GPU case of the family: shape, regime and dtype."""
    cases, kv = FAMILIES[family]
    worst = {}
    for case in cases:
        for n, rt in _ratios(case, dtype, kv).items():
            if rt > worst.get(n, (-1.0, None))[0]:
                worst[n] = (rt, case)
    for n, (rt, case) in worst.items():
        print(f"[emulation] {family} {dtype} {n}: largest err/bound {rt:.3f} at {case}")
        assert rt <= 1.0, (family, dtype, n, rt, case)


@pytest.mark.parametrize("family", list(FB.SUBNORMAL_CASES))
def test_fp32_emulation_stays_inside_the_f16_bound_with_subnormal_gradients(family):
    """dO scaled by 2^-14: every dS is an f16 subnormal and the sub term is what holds the emulation."""
    case = FB.SUBNORMAL_CASES[family]
    q, k, v, dO = FB.operands(case, "f16", 2.0 ** -14)
    assert float(FB.model(q, k, v, dO, "f16")["dS"].abs().max()) < 2.0 ** -14
    for n, rt in _ratios(case, "f16", family == "kv", 2.0 ** -14).items():
        print(f"[emulation] {family} f16 dO*2^-14 {n}: err/bound {rt:.3f}")
        assert rt <= 1.0, (family, n, rt)


def test_case_lists_claim_every_instantiation():
    """Each family's case list holds all ten (KQ, DB) = (ceil(d / 16), ceil(d / 32)) pairs the dispatchers compile, on a ragged shape."""
    pairs = {(k, (k + 1) // 2) for k in range(1, 11)}
    for family, (cases, _) in FAMILIES.items():
        got = {((c[0] + 15) // 16, (c[0] + 31) // 32) for c in cases if c[1] % 32 and c[2] % 32}
        assert got == pairs, (family, sorted(pairs - got))
    assert {((d + 15) // 16, (d + 31) // 32) for d in FB.FLASH_D} == pairs


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "-".join(str(x) for x in s))
def test_bounds_reject_defects(shape):
    """Each defect of FB.defects moves an output by >= 2x its bf16 bound (the looser type) at this shape, in at least one of the four
    regimes.  A defect that cannot occur at a shape is not listed there (FB.defects).  A defect of one piece of code that moves several
    outputs -- the key role's loop ending one query tile early moves dK and dV -- is caught when one of them leaves its bound; every
    output's figure is printed.  (dK alone does not see the one live row of the last query tile at T = 417: 0.6x.)"""
    d, T, Tk, N, H = shape
    S, L = _chunks(shape)
    best = {}
    for reg in REGIMES:
        for name, outs in FB.margins(shape + (reg,), S=S, L=L).items():
            for o, m in outs.items():
                if m > best.setdefault(name, {}).get(o, (-1.0, ""))[0]:
                    best[name][o] = (m, reg)
    want = {"dK and dV swapped", "last query tile dropped from dK and dV"}
    if Tk > 1:
        want |= {"delta taken as 0", "scale missing from dS", "last key tile dropped from dQ"}
    if S > 1:
        want.add("last chunk's partial dropped by the reduce")
    if N * H > 1:
        want.add("lse of the neighbouring (sample, head)")
    if d % 16:
        want.add("last channel of the partial k-step dropped from the scores")
    if N > 1 and Tk > 1:
        want.add("delta of the other sample")
    assert set(best) == want
    for name, outs in best.items():
        print(f"[sensitivity] flash_bwd {shape}: {name}: " + ", ".join(f"{o} {m:.1f}x ({reg})" for o, (m, reg) in outs.items()))
        assert max(m for m, _ in outs.values()) >= 2.0, f"{shape}: the bounds let '{name}' through"


def test_truncated_ds_is_not_separated_from_rounded_ds():
    """dS truncated instead of rounded to nearest moves each dS by up to 2 u |dS| where rounding moves it by u |dS|; the bound carries
    C u (|dQ| + E_dS |K|) with E_dS >= 2 |dS|, so truncation can reach 2 / (3 C) ... 2 / C of it and never 2x.  What it reaches on the
    coherent 'last' regime is asserted instead: >= 0.1 of the dQ bound at every shape with more than one key (measured 0.13 .. 0.26)."""
    lo = hi = None
    for shape in SHAPES:
        if shape[2] == 1:
            continue
        q, k, v, dO = FB.operands(shape + ("last",), "bf16")
        r = FB.model(q, k, v, dO, "bf16")
        m = FB.ratio(FB.trunc16(r["dS"], "bf16") @ k, r["dQ"], r["bQ"])
        lo, hi = min(m, lo or m), max(m, hi or m)
        assert 0.1 <= m < 2.0 / R.C_ATTN, (shape, m)
    print(f"[sensitivity] flash_bwd: dS truncated: {lo:.3f} .. {hi:.3f} of the dQ bound ('last' regime)")


def test_chunk_rule_of_the_kv_cases():
    """pmi_attn_flash_bwd_kv_chunks / _workspace are host-only.  S at every kv case is the value the case names; the workspace is the
    fragments plus N heads ntk S DB x 8 KiB of partial tiles (none with S = 1: the accumulators go straight out); under
    pmi_set_option(14, n) S never exceeds n."""
    from perceptor_amd import _hip
    lib = _hip.lib()
    cases = [(c, 1) for c in FB.CROSS_CASES] + [(c, FB.KV_SPLIT_S[c[1:3]]) for c in FB.KV_SPLIT_CASES] + \
        [(FB.SUBNORMAL_CASES["kv"], 2)]
    try:
        for opt in (0, 1, 2):
            lib.pmi_set_option(14, opt)
            for (d, T, Tk, N, H, _), s_named in cases:
                S = lib.pmi_attn_flash_bwd_kv_chunks(N, T, Tk, H, d)
                assert S == (s_named if opt == 0 else min(opt, s_named)) == FB.kv_chunks(N, T, Tk, H, opt)[0], (d, T, Tk, N, H, opt, S)
                assert opt == 0 or S <= opt
                frag = lib.pmi_attn_flash_bwd_workspace(N, T, Tk, H, d, 0)
                part = N * H * ((Tk + 31) // 32) * S * ((d + 31) // 32) * 8 if S > 1 else 0
                assert frag > 0 and lib.pmi_attn_flash_bwd_kv_workspace(N, T, Tk, H, d) == frag + part
    finally:
        lib.pmi_set_option(14, 0)
    # the chunk lengths the split cases name: 5 + 4, 5 + 5 + 3 and 5 + 5 + 4 query tiles
    assert [FB.kv_chunks(N, T, Tk, H) for _, T, Tk, N, H, _ in FB.KV_SPLIT_CASES[:3]] == [(2, 5), (3, 5), (3, 5)]
