"""GPU: the DeepImagePrior kernels (csrc/dip.hip, the 8-tap resamplers of csrc/fir.hip) per element against tests/_dip_ref64.py with the
bound K 2^-24 sum|terms| (+ the output's 16-bit rounding), the whole network (output, every parameter gradient, the latent gradient, the
running statistics) against the float64 restatement with tolerances set from its 16-bit emulation floor, the training / eval behaviour,
the stale-pack test and drawers.DeepImagePrior under Adam.

Shapes.  Weight gradient: (Cout, Cin, taps) in {(192, 64, 9), (192, 196, 9), (192, 192, 1), (4, 192, 1), (3, 192, 1)} on (N, H, W) in
{(1, 4, 4), (1, 8, 8), (2, 16, 16), (1, 24, 40)}: 16 pixels (less than one 32-pixel step), a Cin tail (196 = 3 tiles + 4, not a multiple
of 8), the plain route (Cout 4 and 3), a batch, and 960 pixels = 30 steps that do not divide among the splits.  BN and resamplers: C in
{4, 192, 196} on the same grids (the down-sampler from 8 -> 4 up, the up-sampler from 4 -> 8 up).  Kernel inputs are exactly representable
in the 16-bit type, so the only 16-bit rounding in a per-kernel bound is the output's.

Whole network: tolerance = FLOOR x MARGIN per tensor class; FLOOR = relative L2 deviation of the restatement's 16-bit emulation from pure
float64, computed here on the CPU; MARGIN (below) = twice the largest GPU / floor ratio measured on an MI355X.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import _dip_ref64 as D
from perceptor_amd.engine import dip as E

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24
DTS = ("bf16", "f16")
GRIDS = [(1, 4, 4), (1, 8, 8), (2, 16, 16), (1, 24, 40)]
WG_SHAPES = [(192, 64, 9), (192, 196, 9), (192, 192, 1), (4, 192, 1), (3, 192, 1)]
MARGIN, DRAWER_MARGIN = D.MARGIN, D.DRAWER_MARGIN


def _hip():
    from perceptor_amd import _hip
    _hip.lib()
    return _hip


def _rand(shape, seed, dt, scale=1.0):
    from perceptor_amd.utils.synth import seeded_noise
    return D.rnd(seeded_noise(shape, seed).double() * scale, dt)


def _nhwc(x64, dt, ld=None, ring=0, mode="constant"):
    """float64 NCHW -> 16-bit NHWC on the device, channels zero-padded to ld, with a ring filled by `mode`"""
    if ring:
        x64 = F.pad(x64, (ring,) * 4, mode)
    x = x64.permute(0, 2, 3, 1)
    if ld is not None and ld > x.shape[-1]:
        x = F.pad(x, (0, ld - x.shape[-1]))
    return x.contiguous().to(D.TDT[dt]).to(DEV)


def _nchw64(y, c=None, ring=0):
    y = y.detach().cpu().double()
    if ring:
        y = y[:, ring:-ring, ring:-ring]
    return y[..., :c].permute(0, 3, 1, 2).contiguous()


def _check(name, got, want, tol):
    err = (got - want).abs()
    worst = float((err / tol.clamp_min(1e-300)).max())
    print(f"{name}: max err {float(err.max()):.3e}, worst err / bound {worst:.3f}")
    assert worst <= 1.0, f"{name}: error is {worst:.2f} x the bound"


# ---- weight gradient ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("shape", WG_SHAPES)
def test_wgrad(shape, grid, dt):
    H_ = _hip()
    cout, cin, taps = shape
    n, h, w = grid
    dy = _rand((n, cout, h, w), 11, dt)
    x = _rand((n, cin, h, w), 12, dt)
    dW, db, aW, ab = D.wgrad64(dy, x, taps)
    ring = 1 if taps == 9 else 0
    dyd = _nhwc(dy, dt, ld=(cout + 7) // 8 * 8, ring=ring)
    xd = _nhwc(x, dt, ld=(cin + 7) // 8 * 8, ring=ring, mode="reflect")
    from perceptor_amd._hip import call, ptr, dtype_code
    splits = H_.lib().pmi_dip_wgrad_splits(n * h * w, cout, cin, taps)
    assert 1 <= splits <= 64
    outs = []
    for _ in range(2):
        slabs = torch.full((splits * (cout * cin * taps + cout),), float("nan"), dtype=torch.float32, device=DEV)    # every slab entry must be written
        gw = torch.empty((cout, cin, 3, 3) if taps == 9 else (cout, cin, 1, 1), dtype=torch.float32, device=DEV)
        gb = torch.empty((cout,), dtype=torch.float32, device=DEV)
        call("pmi_dip_wgrad", ptr(dyd), dyd.shape[-1], ring, ptr(xd), xd.shape[-1], ring, ptr(slabs), ptr(gw), ptr(gb), n, h, w, cout, cin, taps,
             splits, 1.0, dtype_code(dt))
        outs.append((gw.cpu(), gb.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "two runs differ: the reduction is not in a fixed order"
    k = D.kernel_k("wgrad", n * h * w)
    _check("dW", outs[0][0].double(), dW, k * U24 * aW)
    _check("db", outs[0][1].double(), db, k * U24 * ab)
    for defect in ("wgrad_kykx_swapped", "wgrad_no_ring"):
        bad = D.wgrad64(dy, x, taps, defect)[0]
        if taps == 9:
            assert bool(((bad - dW).abs() > k * U24 * aW).any()), f"{defect} passes the bound"
        else:
            assert torch.equal(bad, dW)


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("shape", WG_SHAPES)
def test_pack_w(shape, dt):
    """pmi_dip_pack_w: the forward order [n_p][tap][cin_p] and the transposed, tap-reversed order [cin_p][tap][cout_p], zero padded, each value
    the parameter rounded once to the 16-bit type (torch's own cast is the yardstick: round to nearest even)"""
    from perceptor_amd._hip import call, ptr, dtype_code
    _hip()
    cout, cin, taps = shape
    k = 3 if taps == 9 else 1
    wt = (_rand((cout, cin, k, k), 61, None) * 0.1).float()
    n_p, cin_p, cout_p = (cout + 3) // 4 * 4, (cin + 7) // 8 * 8, (cout + 7) // 8 * 8
    wd = wt.to(DEV)
    fwd = torch.full((n_p, taps, cin_p), 7.0, dtype=D.TDT[dt], device=DEV)
    dxp = torch.full((cin_p, taps, cout_p), 7.0, dtype=D.TDT[dt], device=DEV)
    call("pmi_dip_pack_w", ptr(wd), ptr(fwd), ptr(dxp), cout, cin, taps, n_p, cin_p, cin_p, cout_p, dtype_code(dt))
    w16 = wt.to(D.TDT[dt])
    want_f = torch.zeros((n_p, taps, cin_p), dtype=D.TDT[dt])
    want_f[:cout, :, :cin] = w16.permute(0, 2, 3, 1).reshape(cout, taps, cin)
    want_d = torch.zeros((cin_p, taps, cout_p), dtype=D.TDT[dt])
    want_d[:cin, :, :cout] = w16.flip(2, 3).permute(1, 2, 3, 0).reshape(cin, taps, cout)
    assert torch.equal(fwd.cpu(), want_f) and torch.equal(dxp.cpu(), want_d)
    wd.mul_(2.0)                                       # packed again after the weights moved: nothing is cached
    call("pmi_dip_pack_w", ptr(wd), ptr(fwd), None, cout, cin, taps, n_p, cin_p, cin_p, cout_p, dtype_code(dt))
    want_2 = torch.zeros((n_p, taps, cin_p), dtype=D.TDT[dt])
    want_2[:cout, :, :cin] = (2.0 * wt).to(D.TDT[dt]).permute(0, 2, 3, 1).reshape(cout, taps, cin)   # (rounded from the doubled fp32 value: a subnormal f16 does not double exactly)
    assert torch.equal(fwd.cpu(), want_2) and torch.equal(dxp.cpu(), want_d)                           # dxp = NULL: left alone


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------------------
def _bn_case(c, grid, dt):
    n, h, w = grid
    x = _rand((n, c, h, w), 21, dt, 1.5) + D.rnd(torch.linspace(-2, 2, c, dtype=torch.float64), dt).view(1, c, 1, 1)
    x = D.rnd(x, dt)
    gamma = (1.0 + 0.3 * _rand((c,), 22, None)).float().double()
    beta = (0.2 * _rand((c,), 23, None)).float().double()
    return x, gamma, beta


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("c", [4, 192, 196])
def test_bn_forward(c, grid, dt):
    H_ = _hip()
    n, h, w = grid
    p = n * h * w
    x, gamma, beta = _bn_case(c, grid, dt)
    rm0, rv0 = (0.1 * _rand((c,), 24, None)).float(), (0.5 + _rand((c,), 25, None).abs()).float()
    from perceptor_amd._hip import call, ptr, dtype_code
    P = {"b.running_mean": rm0.clone().to(DEV), "b.running_var": rv0.clone().to(DEV)}
    gd, bd = gamma.float().to(DEV), beta.float().to(DEV)
    ld = (c + 7) // 8 * 8
    xd = _nhwc(x, dt, ld=ld)
    dst = torch.zeros((n, h + 2, w + 2, ld + 8), dtype=D.TDT[dt], device=DEV)       # a wider ringed destination, written at channel offset 4
    blocks = H_.lib().pmi_dip_bn_blocks(p)
    assert blocks == max(1, min(256, (p + 63) // 64))
    part = torch.full((blocks * c,), float("nan"), dtype=torch.float32, device=DEV)
    md, rd = torch.empty(c, dtype=torch.float32, device=DEV), torch.empty(c, dtype=torch.float32, device=DEV)
    call("pmi_dip_bn_stats", ptr(xd), ld, 0, ptr(part), ptr(md), ptr(rd), ptr(P["b.running_mean"]), ptr(P["b.running_var"]), n, h, w, c,
         E.BN_MOMENTUM, E.BN_EPS, dtype_code(dt))
    call("pmi_dip_bn_apply", ptr(xd), ld, 0, ptr(md), ptr(rd), ptr(gd), ptr(bd), dst.data_ptr() + 2 * 4, dst.shape[-1], 1, n, h, w, c, 1, dtype_code(dt))
    mean_g, rstd_g = md.cpu().double(), rd.cpu().double()
    y64, mean, var = D.bn_train64(x, gamma, beta, True)
    amean = x.abs().mean(dim=(0, 2, 3))
    _check("mean", mean_g, mean, D.kernel_k("bn_mean", p) * U24 * amean)
    rstd = torch.rsqrt(var + E.BN_EPS)
    krs = D.kernel_k("bn_rstd", p) + 2 * D.kernel_k("bn_mean", p)                     # the mean's own error enters the centred squares twice
    _check("rstd", rstd_g, rstd, krs * U24 * rstd * (1 + amean * rstd) ** 2)
    unb = p / (p - 1)
    _check("running_mean", P["b.running_mean"].cpu().double(), 0.9 * rm0.double() + 0.1 * mean,
           U24 * (4 * (0.9 * rm0.double().abs() + 0.1 * mean.abs()) + 0.1 * D.kernel_k("bn_mean", p) * amean))
    _check("running_var", P["b.running_var"].cpu().double(), 0.9 * rv0.double() + 0.1 * var * unb,
           U24 * (6 + krs) * (0.9 * rv0.double() + 0.1 * (var + amean ** 2) * unb))
    biased = 0.9 * rv0.double() + 0.1 * var
    assert bool(((biased - (0.9 * rv0.double() + 0.1 * var * unb)).abs() > U24 * (6 + krs) * (0.9 * rv0.double() + 0.1 * (var + amean ** 2) * unb)).any())
    a = (gamma * rstd).view(1, c, 1, 1)
    xc = (x - mean.view(1, c, 1, 1)).abs()
    tol = D.out_rounding(dt, y64) + U24 * a.abs() * ((krs + 4) * (xc + amean.view(1, c, 1, 1)) + 4 * (x.abs() + mean.abs().view(1, c, 1, 1))) \
        + 4 * U24 * beta.abs().view(1, c, 1, 1)
    got = dst.cpu().double()
    want = F.pad(y64, (1,) * 4, "reflect")
    _check("y", got[..., 4:4 + c].permute(0, 3, 1, 2), want, F.pad(tol, (1,) * 4, "reflect"))
    assert not bool(got[..., :4].any()) and not bool(got[..., 4 + c:].any()), "bn_apply wrote outside its channel slice"
    for defect in ("border_clamp", "border_zero"):
        bad = F.pad(y64, (1,) * 4, D.pad_mode(defect))
        assert bool(((bad - want).abs() > F.pad(tol, (1,) * 4, "reflect")).any()), f"{defect} passes the bound"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("c", [4, 192, 196])
@pytest.mark.parametrize("act", [0, 1])
def test_bn_backward(c, grid, dt, act):
    H_ = _hip()
    n, h, w = grid
    p = n * h * w
    x, gamma, beta = _bn_case(c, grid, dt)
    dy = _rand((n, c, h, w), 26, dt)
    for _ in range(20):        # move the few values whose pre-activation sits on LeakyReLU's kink (fp32 and float64 could take different sides)
        mean = x.mean(dim=(0, 2, 3))
        var = ((x - mean.view(1, c, 1, 1)) ** 2).mean(dim=(0, 2, 3))
        rstd = torch.rsqrt(var + E.BN_EPS)
        pre = (x - mean.view(1, c, 1, 1)) * (rstd * gamma).view(1, c, 1, 1) + beta.view(1, c, 1, 1)
        near = pre.abs() < 1e-3
        if not bool(near.any()):
            break
        x = D.rnd(torch.where(near, x + 0.25, x), dt)
    assert float(pre.abs().min()) >= 1e-3, "a pre-activation still sits on LeakyReLU's kink"
    dx, dg, db, ag, ab = D.bn_bwd64(x, dy, gamma, beta, act)
    from perceptor_amd._hip import call, ptr, dtype_code
    ld = (c + 7) // 8 * 8
    xd, dyd, md, rd = _nhwc(x, dt, ld=ld), _nhwc(dy, dt, ld=ld), mean.float().to(DEV), rstd.float().to(DEV)
    gd, bd = gamma.float().to(DEV), beta.float().to(DEV)
    part = torch.full((2 * H_.lib().pmi_dip_bn_blocks(p) * c,), float("nan"), dtype=torch.float32, device=DEV)
    sums = torch.empty(2 * c, dtype=torch.float32, device=DEV)
    grads = {"b.weight": torch.empty(c, dtype=torch.float32, device=DEV), "b.bias": torch.empty(c, dtype=torch.float32, device=DEV)}
    dxg = torch.zeros((n, h + 2, w + 2, ld), dtype=D.TDT[dt], device=DEV)
    call("pmi_dip_bn_bwd", ptr(xd), ld, 0, ptr(dyd), ld, ptr(md), ptr(rd), ptr(gd), ptr(bd), ptr(part), ptr(sums), ptr(grads["b.weight"]),
         ptr(grads["b.bias"]), ptr(dxg), ld, 1, n, h, w, c, act, 1.0, dtype_code(dt))
    ks = D.kernel_k("bn_bwd_sums", p)
    xh = ((x - mean.view(1, c, 1, 1)) * rstd.view(1, c, 1, 1)).abs()
    _check("dgamma", grads["b.weight"].cpu().double(), dg, (ks + 4) * U24 * ag)
    _check("dbeta", grads["b.bias"].cpu().double(), db, ks * U24 * ab)
    a = (gamma * rstd).abs().view(1, c, 1, 1)
    tol = D.out_rounding(dt, dx) + (ks + 14) * U24 * a * (dy.abs() + (ab / p).view(1, c, 1, 1) + xh * (ag / p).view(1, c, 1, 1))
    got = dxg.cpu().double()
    _check("dx", _nchw64(got, c, ring=1), dx, tol)
    assert not bool(got[:, 0].any()) and not bool(got[:, :, 0].any()), "bn_bwd wrote into the ring"
    for defect in ("bn_bwd_no_mean", "bn_bwd_no_xhat") + (("lrelu_bwd_slope_1", "lrelu_bwd_slope_0") if act else ()):
        bad = D.bn_bwd64(x, dy, gamma, beta, act, defect)[0]
        assert bool(((bad - dx).abs() > tol).any()), f"{defect} passes the bound"


# ---- resamplers, the pad fold ---------------------------------------------------------------------------------------------------------------
def _fir(name, x16, out_shape, *dims, ring_in=None, ring_out=None, dt="bf16"):
    from perceptor_amd._hip import call, ptr, dtype_code
    y = torch.zeros(out_shape, dtype=x16.dtype, device=DEV)
    args = [ptr(x16)] + ([ring_in] if ring_in is not None else []) + [ptr(y)] + ([ring_out] if ring_out is not None else []) + list(dims)
    call(name, *args, dtype_code(dt))
    return y


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("c", [4, 192, 196])
def test_resamplers(c, grid, dt):
    H_ = _hip()
    n, h, w = grid
    x = _rand((n, c, h, w), 31, dt)
    ka = D.K1.abs()

    def absmap(t, up):                                # the operator with |taps| (linear: give it |x|): sum |terms| per output element
        cc = t.shape[1]
        if up:
            k = torch.outer(2 * ka, 2 * ka)[None, None].expand(cc, 1, 8, 8)
            return F.conv_transpose2d(F.pad(t, (2,) * 4, "reflect"), k, stride=2, padding=7, groups=cc)
        k = torch.outer(ka, ka)[None, None].expand(cc, 1, 8, 8)
        return F.conv2d(F.pad(t, (3,) * 4, "reflect"), k, stride=2, groups=cc)

    # up: h -> 2h (h >= 4 here), and its adjoint
    up = D.up64(x)
    got = _fir("pmi_fir8_up2", _nhwc(x, dt), (n, 2 * h, 2 * w, c), n, h, w, c, dt=dt)
    tol_up = D.out_rounding(dt, up) + D.kernel_k("up") * U24 * absmap(x.abs(), True)
    _check("up", _nchw64(got), up, tol_up)
    for defect in ("border_clamp", "border_zero", "up_kernel_not_doubled"):
        assert bool(((D.up64(x, defect) - up).abs() > tol_up).any()), f"{defect} passes the up-sampler's bound"
    yy = _rand((n, c, 2 * h, 2 * w), 32, dt)
    adj = D.adjoint64(D.up64, x.shape, yy)
    aadj = D.adjoint64(lambda t, d: absmap(t, True), x.shape, yy.abs())
    got = _fir("pmi_fir8_up2_bwd", _nhwc(yy, dt), (n, h, w, c), n, h, w, c, dt=dt)
    tol = D.out_rounding(dt, adj) + D.kernel_k("up_bwd") * U24 * aadj
    _check("up_bwd", _nchw64(got), adj, tol)
    assert bool(((D.adjoint64(D.up64, x.shape, yy, "adjoint_no_folds") - adj).abs() > tol).any()), "the fold-less adjoint passes"
    if h >= 8:                                        # down: h -> h / 2 needs h >= 4 ... the issue's smallest is 8 -> 4
        down = D.down64(x)
        got = _fir("pmi_fir8_down2", _nhwc(x, dt, ring=1), (n, h // 2, w // 2, c), n, h, w, c, ring_in=1, dt=dt)
        tol_d = D.out_rounding(dt, down) + D.kernel_k("down") * U24 * absmap(x.abs(), False)
        _check("down", _nchw64(got), down, tol_d)
        for defect in ("border_clamp", "border_zero"):
            assert bool(((D.down64(x, defect) - down).abs() > tol_d).any()), f"{defect} passes the down-sampler's bound"
        yd = _rand((n, c, h // 2, w // 2), 33, dt)
        adj = D.adjoint64(D.down64, x.shape, yd)
        aadj = D.adjoint64(lambda t, d: absmap(t, False), x.shape, yd.abs())
        got = _fir("pmi_fir8_down2_bwd", _nhwc(yd, dt), (n, h + 2, w + 2, c), n, h, w, c, ring_out=1, dt=dt)
        tol = D.out_rounding(dt, adj) + D.kernel_k("down_bwd") * U24 * aadj
        _check("down_bwd", _nchw64(got, ring=1), adj, tol)
        assert not bool(got[:, 0].any()), "down2_bwd wrote into the ring"
        assert bool(((D.adjoint64(D.down64, x.shape, yd, "adjoint_no_folds") - adj).abs() > tol).any()), "the fold-less adjoint passes"


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("grid", GRIDS)
def test_pad_fold_and_adjointness(grid, dt):
    """<A x, y> = <x, A^T y> for the pad, the down- and the up-sampler: both sides from the kernels' own 16-bit outputs, summed in float64; the
    bound is the outputs' rounding, u16 (sum |A x| |y| + sum |x| |A^T y|)."""
    from perceptor_amd._hip import call, ptr, dtype_code
    n, h, w = grid
    c = 8
    x = _rand((n, c, h, w), 41, dt)
    yp = _rand((n, c, h + 2, w + 2), 42, dt)
    xd, ypd = _nhwc(x, dt), _nhwc(yp, dt)
    ax = torch.empty((n, h + 2, w + 2, c), dtype=xd.dtype, device=DEV)
    call("pmi_dip_reflect_pad", ptr(xd), ptr(ax), n, h, w, c, dtype_code(dt))
    assert torch.equal(_nchw64(ax), F.pad(x, (1,) * 4, "reflect")), "reflect_pad is a copy: it must be exact"
    aty = torch.empty((n, h, w, c), dtype=xd.dtype, device=DEV)
    call("pmi_dip_pad_fold", ptr(ypd), None, ptr(aty), n, h, w, c, dtype_code(dt))
    fold = D.adjoint64(lambda t, d: D.pad1(t, d), x.shape, yp)
    afold = D.adjoint64(lambda t, d: D.pad1(t, d), x.shape, yp.abs())
    _check("fold", _nchw64(aty), fold, D.out_rounding(dt, fold) + D.kernel_k("fold") * U24 * afold)
    pairs = [("pad", _nchw64(ax), yp, x, _nchw64(aty))]
    yu = _rand((n, c, 2 * h, 2 * w), 43, dt)
    pairs.append(("up", _nchw64(_fir("pmi_fir8_up2", xd, (n, 2 * h, 2 * w, c), n, h, w, c, dt=dt)), yu, x,
                  _nchw64(_fir("pmi_fir8_up2_bwd", _nhwc(yu, dt), (n, h, w, c), n, h, w, c, dt=dt))))
    if h >= 8:
        yd = _rand((n, c, h // 2, w // 2), 44, dt)
        pairs.append(("down", _nchw64(_fir("pmi_fir8_down2", xd, (n, h // 2, w // 2, c), n, h, w, c, ring_in=0, dt=dt)), yd, x,
                      _nchw64(_fir("pmi_fir8_down2_bwd", _nhwc(yd, dt), (n, h, w, c), n, h, w, c, ring_out=0, dt=dt))))
    for name, a_x, y, x_, at_y in pairs:
        lhs, rhs = float((a_x * y).sum()), float((x_ * at_y).sum())
        bound = D.U16[dt] * float((a_x * y).abs().sum() + (x_ * at_y).abs().sum()) \
            + (2.0 ** -25 * float(y.abs().sum() + x_.abs().sum()) if dt == "f16" else 0.0)            # f16's subnormal outputs
        print(f"adjointness {name}: <Ax, y> = {lhs:.6e}, <x, A^T y> = {rhs:.6e}, bound {bound:.3e}")
        assert abs(lhs - rhs) <= bound


# ---- head -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("variant", [(3, True, True), (3, False, False), (4, True, False)])
def test_head(variant, grid, dt):
    from perceptor_amd._hip import call, ptr, dtype_code
    cout, sig, dec = variant
    n, h, w = grid
    x = _rand((n, 192, h, w), 51, dt)
    wt = (_rand((cout, 192, 1, 1), 52, None) * 0.1).float().double()
    b = (_rand((cout,), 53, None) * 0.1).float().double()
    cm = E.colcorr_t().double() if dec else None
    want = D.head64(x, wt, b, cm, sig)
    z = F.conv2d(x.abs(), wt.abs(), b.abs())
    if dec:
        z = torch.einsum("nchw,cd->ndhw", z, cm.abs())
    out = torch.empty((n, cout, h, w), dtype=torch.float32, device=DEV)
    cmd = cm.float().contiguous().to(DEV) if dec else None
    xd, wd, bd = _nhwc(x, dt), wt.float().contiguous().to(DEV), b.float().to(DEV)          # (named: they must outlive the launch)
    call("pmi_dip_head_fwd", ptr(xd), ptr(wd), ptr(bd), ptr(cmd), ptr(out), n, h * w, 192, cout, int(sig), dtype_code(dt))
    tol = D.kernel_k("head", cin=192) * U24 * (z * (0.25 if sig else 1.0) + want.abs())          # sigmoid' <= 1/4 carries the logit's error
    _check("head", out.cpu().double(), want, tol)
    if dec:
        assert bool(((D.head64(x, wt, b, cm, sig, "colour_transposed") - want).abs() > tol).any()), "the transposed colour matrix passes"
    # backward: dz = scale cm (dout sigmoid'), 16-bit, channels cout..7 zero
    dout = _rand((n, cout, h, w), 54, None).float()
    o = out.cpu().double()
    dr = dout.double() * (o * (1 - o) if sig else 1.0)
    dz = torch.einsum("ndhw,cd->nchw", dr, cm) if dec else dr
    adz = torch.einsum("ndhw,cd->nchw", dr.abs(), cm.abs()) if dec else dr.abs()
    dzg = torch.empty((n, h, w, 8), dtype=D.TDT[dt], device=DEV)
    doutd = dout.to(DEV)
    call("pmi_dip_head_bwd", ptr(doutd), ptr(out), ptr(cmd), ptr(dzg), n, h * w, cout, int(sig), 0.5, dtype_code(dt))
    got = dzg.cpu().double()
    _check("head_bwd", _nchw64(got, cout), 0.5 * dz, D.out_rounding(dt, 0.5 * dz) + 8 * U24 * 0.5 * adz)
    assert not bool(got[..., cout:].any())


# ---- whole network ------------------------------------------------------------------------------------------------------------------------------
_classes, zero_gradient_names = D.tensor_class, D.zero_gradient_names


@functools.lru_cache(maxsize=None)
def _ref(case):
    return D.run_case64(case)


@functools.lru_cache(maxsize=None)
def _floor(case, dt):
    """per tensor: relative L2 deviation of the 16-bit emulation from pure float64 (CPU only)"""
    out, dl, grads, stats = _ref(case)
    eo, edl, eg, es = D.run_case64(case, emulate=dt)
    fl = {"out": D.rel_l2(eo, out), "dlatents": D.rel_l2(edl, dl)}
    for k in stats:
        fl[k] = D.rel_l2(es[k], stats[k])
    for k in grads:
        fl[k] = D.rel_l2(eg[k], grads[k])
    return fl


def _model(case, dt, sd=None, train=True):
    from perceptor_amd import models
    ns, size, n = case
    m = models.DeepImagePrior(shape=(D.CIN, size, size), n_scales=ns, dtype=dt)
    m.load_state_dict(E.synthetic_state_dict(ns, D.CIN) if sd is None else sd, strict=True)
    m = m.to(DEV)
    return m.train() if train else m.eval()


def _run_gpu(case, dt, m=None):
    m = _model(case, dt) if m is None else m
    lat32, cot32 = D.case_inputs(case)
    lat = lat32.to(DEV).requires_grad_(True)
    out = m(lat)
    (out * cot32.to(DEV)).sum().backward()
    grads = {k: p.grad.detach().cpu().double() for k, p in m.named_parameters()}
    stats = {k: v.detach().cpu().double() for k, v in m.named_buffers() if k.endswith(("running_mean", "running_var"))}
    return out.detach().cpu().double(), lat.grad.cpu().double(), grads, stats, m


@functools.lru_cache(maxsize=None)
def _abs_terms(case):
    """sum |cotangent| per channel of every convolution output and every BN(196) output: sum |terms| of the analytically-zero bias gradients"""
    ns, size, n = case
    sd = D.to64(E.synthetic_state_dict(ns, D.CIN))
    lat32, cot32 = D.case_inputs(case)
    terms = {}
    out, _ = D.network64(sd, lat32.double(), ns, abs_terms=terms)
    (out * cot32.double()).sum().backward()
    return terms


@pytest.mark.parametrize("dt", DTS)
@pytest.mark.parametrize("case", D.GPU_CASES, ids=D.case_name)
def test_network(case, dt):
    out, dl, grads, stats = _ref(case)
    fl = _floor(case, dt)
    go, gdl, gg, gs, m = _run_gpu(case, dt)
    zero = set(zero_gradient_names(grads))
    terms = _abs_terms(case)
    worst, fails = {}, []

    def hold(cls, name, got, want):                # every figure is taken (and printed below) before anything is asserted
        r = D.rel_l2(got, want) / fl[name]
        worst[cls] = max(worst.get(cls, 0.0), r)
        if not r <= MARGIN[cls]:
            fails.append(f"{name}: rel L2 {D.rel_l2(got, want):.3e} is {r:.2f} x the floor {fl[name]:.3e} (margin {MARGIN[cls]})")

    hold("out", "out", go, out)
    hold("dlatents", "dlatents", gdl, dl)
    for k in stats:
        hold("stats", k, gs[k], stats[k])
    for k in grads:
        if k in zero:
            # the terms are 16-bit values that cancel: each carries one rounding of its type, so the sum is off by at most u16 sum|terms|
            bound = D.U16[dt] * terms[k]
            zr = float((gg[k].abs() / bound).max())
            worst["zero"] = max(worst.get("zero", 0.0), zr)
            if not zr <= 1.0:
                fails.append(f"{k}: |gradient| {float(gg[k].abs().max()):.3e} is {zr:.2f} x u16 sum|terms|")
            continue
        hold(_classes(k), k, gg[k], grads[k])
    print(f"{D.case_name(case)} {dt}: GPU / floor per class " + ", ".join(f"{k} {v:.2f}" for k, v in sorted(worst.items())))
    assert not fails, "; ".join(fails)
    # the ky / kx fault at this level, as a sanity check that the comparison reads PyTorch's layout
    k3 = [k for k in grads if k.endswith(".1.1.4.1.weight")][0]
    assert D.rel_l2(grads[k3].transpose(2, 3), grads[k3]) > MARGIN["conv_w"] * fl[k3]


# ---- behaviour ----------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_bit_identical():
    case = (2, 16, 2)
    a, b = _run_gpu(case, "bf16"), _run_gpu(case, "bf16")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for k in a[2]:
        assert torch.equal(a[2][k], b[2][k]), k
    for k in a[3]:
        assert torch.equal(a[3][k], b[3][k]), k


def test_batch_statistics_and_eval():
    case = (2, 16, 2)
    lat = D.case_inputs(case)[0].to(DEV)
    m = _model(case, "bf16")
    with torch.no_grad():
        both, first = m(lat), m(lat[:1])
    assert not torch.equal(both[:1], first), "training mode must use the batch's statistics"
    m = _model(case, "bf16", train=False)
    before = {k: v.clone() for k, v in m.named_buffers()}
    with torch.no_grad():
        both, first = m(lat), m(lat[:1])
    assert torch.equal(both[:1], first), "eval mode normalises with the running statistics: a sample cannot see its batch"
    for k, v in m.named_buffers():
        assert torch.equal(v, before[k]), f"eval mode changed {k}"
    sd = D.to64(E.synthetic_state_dict(2, D.CIN), grad=False)
    want = D.network64(sd, lat.cpu().double(), 2, train=False)[0]
    assert D.rel_l2(both.cpu(), want) < 0.05
    out = m(lat.clone().requires_grad_(True))
    with pytest.raises(NotImplementedError):
        out.sum().backward()


def test_no_stale_weight_pack():
    """forward, one optimiser step on every weight, forward again: the second picture is the restatement's on the NEW weights, and the
    restatement on the old convolution weights (the planted stale pack) is far outside the tolerance"""
    case, dt = (2, 16, 1), "bf16"
    m = _model(case, dt)
    lat32, cot32 = D.case_inputs(case)
    opt = torch.optim.SGD(m.parameters(), lr=0.05)
    old = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    (m(lat32.to(DEV)) * cot32.to(DEV)).sum().backward()
    opt.step()
    new = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    assert all(not torch.equal(old[k], new[k]) for k, _ in m.named_parameters() if k not in zero_gradient_names(old)), "a weight did not move"
    with torch.no_grad():
        got = m(lat32.to(DEV)).cpu().double()
    want = D.network64(D.to64(new, grad=False), lat32.double(), 2)[0]
    stale = D.network64(D.to64(new, grad=False), lat32.double(), 2, defect="stale_weight_pack", conv_sd=D.to64(old, grad=False))[0]
    floor = D.rel_l2(D.network64(D.to64(new, grad=False), lat32.double(), 2, emulate=dt)[0], want)
    r = D.rel_l2(got, want) / floor
    print(f"second forward: rel L2 {D.rel_l2(got, want):.3e} = {r:.2f} x floor; stale restatement at {D.rel_l2(stale, want) / floor:.1f} x floor")
    assert r <= MARGIN["out"]
    assert D.rel_l2(stale, want) > MARGIN["out"] * floor


def test_state_dict_round_trip():
    m = _model((2, 16, 1), "bf16")
    sd = {k: v.cpu() for k, v in m.state_dict().items()}
    ref = E.synthetic_state_dict(2, D.CIN)
    assert list(sd) == list(ref)
    for k in ref:
        assert sd[k].dtype == ref[k].dtype and torch.equal(sd[k], ref[k]), k


# ---- drawer ---------------------------------------------------------------------------------------------------------------------------------------
def _fit64(seed, steps=30):
    """the float64 restatement of drawers.DeepImagePrior((16, 16)) under Adam on the CPU, default initialisation from torch's own modules"""
    from perceptor_amd import drawers
    torch.manual_seed(seed)
    d = drawers.DeepImagePrior((16, 16))
    sd = D.to64(d.deep_image_prior.state_dict())
    lat = d.latents.detach().double()
    images = torch.zeros(1, 3, 16, 16, dtype=torch.float64, requires_grad=True)
    params = [v for v in sd.values() if torch.is_floating_point(v) and v.requires_grad] + [images]
    opt = torch.optim.Adam(params, lr=2e-3)
    target = _target()
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        out, stats = D.network64(sd, lat, 2)
        loss = ((out + images - target) ** 2).mean() + images.abs().mean() * 1e-4
        loss.backward()
        opt.step()
        with torch.no_grad():
            for k, v in stats.items():
                sd[k].copy_(v)
        losses.append(float(loss))
    return d, losses


def _target():
    from perceptor_amd.utils.synth import seeded_noise
    return torch.sigmoid(seeded_noise((1, 3, 16, 16), 77).double())


def test_drawer_fits_target_under_adam():
    from perceptor_amd import drawers
    d, ref_losses = _fit64(0)
    d = d.to(DEV)
    assert not d.latents.requires_grad and d.images.requires_grad and not bool(d.images.any())
    target = _target().float().to(DEV)
    opt = torch.optim.Adam([p for p in d.parameters() if p.requires_grad], lr=2e-3)
    losses = []
    for step in range(30):
        opt.zero_grad()
        pic = d.synthesize()
        reg = d.loss()
        loss = ((pic - target) ** 2).mean() + reg
        loss.backward()
        if step == 0:
            assert float(reg) == 0.0
            want = 2 * (pic.detach() - target) / pic.numel()            # images = 0: |.|'s subgradient is sign(0) = 0
            assert torch.allclose(d.images.grad, want, rtol=1e-6, atol=1e-9)
        opt.step()
        losses.append(float(loss))
    assert abs(float(d.loss()) - float(d.images.detach().abs().mean()) * 1e-4) <= 1e-9
    print(f"drawer: loss {losses[0]:.5f} -> {losses[-1]:.5f}; restatement {ref_losses[0]:.5f} -> {ref_losses[-1]:.5f}")
    assert losses[-1] < losses[0]
    assert losses[-1] <= DRAWER_MARGIN * ref_losses[-1]
