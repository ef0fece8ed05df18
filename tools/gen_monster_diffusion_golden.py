"""Writes tests/golden/monster_diffusion_reference.npz: inputs and outputs of the reference's own base.Model
(perceptor/models/monster_diffusion/base/model.py), MonsterDiffusion (monster_diffusion.py) and PredictionBatch (prediction.py), run
unmodified on the CPU in float64 (torch's default dtype is float64 while the reference runs, so its schedules are float64 too).

The checkpoints are unreachable and the product network would make a large fixture, so two tiny networks carry this package's synthetic
weights (utils.synth; the resamplers' `kernel` buffers keep the reference's own values):
  A  feats 64, depths [1, 2, 2], channels [32, 64, 128], attention [F, T, T], batch 2 at 8 x 12, per-sample sigma (0.3, 40)
  B  feats 64, depths [2, 1, 1], channels [64, 64, 128], attention [F, F, T], batch 3 at 16 x 16, scalar sigma 2.5
Stand-ins cover imports and the constructor only:
  * shells for perceptor.models.monster_diffusion and .base, lantern.module_device, and a lantern.Tensor whose dims / shape / float return
    the class itself and which accepts any torch.Tensor (the stock stand-in of oracle/_refimport.py has no .shape(...));
  * the constructor downloads a checkpoint: the stand-in builds base.Model with the tiny config and loads the synthetic state dict instead;
  * the samplers build their zero augmentations in float32 whatever the module's dtype: a forward pre-hook on mapping_cond casts its input
    to the weights' dtype (zeros: exact);
  * torch.randn_like is wrapped by a recorder that returns what the original returns and keeps a copy of every draw.
No arithmetic of the reference is replaced.  Only numbers and key names with shapes are written.  Block outputs larger than 2048 values
are stored as every s-th value of the flattened tensor (s odd, `<name>_stride`) next to the full tensor's L2 norm.  Deterministic.

    python tools/gen_monster_diffusion_golden.py [--check]
"""
from __future__ import annotations

import importlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "monster_diffusion_reference.npz")

from oracle import _refimport as R                                           # noqa: E402
from perceptor_amd.engine.monster import monster_state_dict_shapes, product_config, synthetic_state_dict    # noqa: E402

SEED = 0
NETS = {"A": ((64, [1, 2, 2], [32, 64, 128], [False, True, True], 9), (2, 3, 8, 12), (0.3, 40.0)),
        "B": ((64, [2, 1, 1], [64, 64, 128], [False, False, True], 9), (3, 3, 16, 16), 2.5)}
CAP = 2048


def synthetic(config):
    return synthetic_state_dict(config, SEED)


def _modules():
    R.install()
    import lantern

    class _Any(type):
        def __instancecheck__(cls, obj):
            return isinstance(obj, torch.Tensor)

    class Tensor(metaclass=_Any):
        dims = shape = float = classmethod(lambda cls, *a, **k: cls)

    lantern.Tensor = Tensor
    lantern.module_device = lambda module: next(module.parameters()).device
    base = os.path.join(R.REF_ROOT, "perceptor", "models", "monster_diffusion")
    R._shell("perceptor.models.monster_diffusion", base)
    R._shell("perceptor.models.monster_diffusion.base", os.path.join(base, "base"))
    model = importlib.import_module("perceptor.models.monster_diffusion.base.model")
    sys.modules["perceptor.models.monster_diffusion.base"].Model = model.Model
    md = importlib.import_module("perceptor.models.monster_diffusion.monster_diffusion")
    return model, md


def _wrapper(model_mod, md_mod, config):
    feats, depths, channels, attn, mcd = config

    class Tiny(md_mod.MonsterDiffusion):                 # the constructor stand-in (module doc)
        def __init__(self):
            torch.nn.Module.__init__(self)
            self.network = model_mod.Model(feats_in=feats, depths=depths, channels=channels, self_attn_depths=attn, mapping_cond_dim=mcd)
            sd = synthetic(config)
            assert list(sd) == list(self.network.state_dict()), "state-dict names or their order differ from the reference's"
            self.network.load_state_dict({k: v.double() for k, v in sd.items()})
            self.network.mapping_cond.register_forward_pre_hook(lambda m, a: (a[0].to(m.weight.dtype),))
            self.eval().requires_grad_(False)

    return Tiny().double()


class _Recorder:
    def __init__(self):
        self.draws, self._orig = [], torch.randn_like

    def __call__(self, *a, **k):
        z = self._orig(*a, **k)
        self.draws.append(z.clone())
        return z

    def __enter__(self):
        torch.randn_like = self
        return self

    def __exit__(self, *exc):
        torch.randn_like = self._orig


def _keep(out, name, t):
    t = t.detach().double().contiguous()
    if t.numel() > CAP:
        s = -(-t.numel() // CAP)
        s += 1 - s % 2
        out[name + "_stride"] = torch.tensor(s)
        out[name + "_norm"] = t.norm()
        out[name + "_shape"] = torch.tensor(t.shape)
        t = t.reshape(-1)[::s].contiguous()
    out[name] = t


def generate():
    torch.set_default_dtype(torch.float64)
    try:
        model_mod, md_mod = _modules()
        g = np.random.Generator(np.random.Philox(key=4242))
        rand = lambda shape: torch.from_numpy(g.random(shape, dtype=np.float32)).double()
        randn = lambda shape: torch.from_numpy(g.standard_normal(shape, dtype=np.float32)).double()
        out = {"seed": torch.tensor(SEED)}
        for name, (config, shape, sigma) in NETS.items():
            m = _wrapper(model_mod, md_mod, config)
            net = m.network
            # images around mid-grey plus noise of the sample's own sigma would leave [0, 1] by far; the network only sees c_in * x, so plain
            # uniform images are as good an input at every sigma
            x = rand(shape)
            ts = torch.tensor(sigma)                                              # a tuple: one sigma per sample; a float: a 0-dim tensor
            taps = {}
            hooks = [net.proj_in.register_forward_hook(lambda mod, a, y: taps.__setitem__("proj_in", y)),
                     net.proj_out.register_forward_hook(lambda mod, a, y: taps.__setitem__("proj_out", y)),
                     net.mapping.register_forward_hook(lambda mod, a, y: taps.__setitem__("cond", y))]
            for i, blk in enumerate(net.u_net.d_blocks):
                hooks.append(blk.register_forward_hook(lambda mod, a, y, i=i: taps.__setitem__(f"d{i}", y)))
            for i, blk in enumerate(net.u_net.u_blocks):
                hooks.append(blk.register_forward_hook(lambda mod, a, y, i=i: taps.__setitem__(f"u{i}", y)))
            pred = m.predictions(x, ts)
            for h in hooks:
                h.remove()
            out[f"{name}_in"] = x.float()
            out[f"{name}_sigma"] = torch.as_tensor(sigma, dtype=torch.float64).reshape(-1)
            for k, v in taps.items():
                _keep(out, f"{name}_{k}", v)
            out[f"{name}_denoised_xs"], out[f"{name}_eps"] = pred.denoised_xs, pred.eps
            to_ts = ts * 0.5
            out[f"{name}_to_sigma"] = to_ts.reshape(-1)
            out[f"{name}_step"] = pred.step(to_ts)
            prev_images, prev_eps = rand(shape), randn(shape)
            prev_ts = ts * 1.25
            out[f"{name}_prev_in"], out[f"{name}_prev_eps"], out[f"{name}_prev_sigma"] = prev_images.float(), prev_eps.float(), prev_ts.reshape(-1)
            out[f"{name}_correction"] = pred.correction(prev_images, prev_ts, prev_eps)
            torch.manual_seed(99)
            with _Recorder() as rec:
                out[f"{name}_inject"] = m.inject_noise(x, ts, ts * 1.3)
            out[f"{name}_inject_noise"] = rec.draws[0]
            if name == "A":
                x0 = (randn(shape) * 80 + 1) / 2                                  # random_noise at this size: decode(randn * sigma_max)
                out["A_x0"] = x0.float()
                x0 = x0.float().double()
                torch.manual_seed(1234)
                with _Recorder() as rec:
                    ys = list(m.elucidated_sample(shape[0], n_evaluations=6, diffused_images=x0))
                assert len(ys) == 3 and len(rec.draws) == 3
                out["A_heun"], out["A_heun_noise"] = torch.stack(ys), torch.stack(rec.draws)
                ys = list(m.linear_multistep_sample(shape[0], n_evaluations=6, diffused_images=x0))
                assert len(ys) == 6
                out["A_lms"] = torch.stack(ys)
                sig = m.sigmas(m._schedule_ts(6)).flatten()
                coeffs = torch.zeros(5, 4)
                for i in range(5):
                    for j in range(min(i + 1, 4)):
                        coeffs[i, j] = m.linear_multistep_coeff(min(i + 1, 4), sig, i, j)
                out["A_lms_coeffs"] = coeffs
        # host tables
        probe = torch.tensor([0.01, 0.05, 0.3, 2.0, 50.0, 50.5, 80.0])
        out["schedule_5"] = m._schedule_ts(5)
        out["gamma_ts"], out["gamma_10"], out["gamma_400"] = probe, m.gamma(probe, 10), m.gamma(probe, 400)
        out["reversed_10"] = m.reversed_ts(probe, 10)
        out["sigmas_float_shape"] = torch.tensor(m.sigmas(0.5).shape)
        out["sigmas_0dim_shape"] = torch.tensor(m.sigmas(torch.tensor(0.5)).shape)
        out["sigmas_1dim_shape"] = torch.tensor(m.sigmas(torch.tensor([0.5, 0.7])).shape)
        out["alphas_1dim"] = m.alphas(torch.tensor([0.5, 0.7]))
        for fn in ("c_skip", "c_out", "c_in", "c_noise"):
            out[fn] = getattr(m, fn)(probe)
        # the product config's state dict: names and shapes from the reference's own module
        ref_sd = model_mod.Model(mapping_cond_dim=9).state_dict()
        assert list(ref_sd) == list(monster_state_dict_shapes(product_config()))
        arrays = {k: np.ascontiguousarray(v.detach().numpy()) for k, v in out.items()}
        arrays["product_names"] = np.array(list(ref_sd))
        arrays["product_shapes"] = np.array([",".join(str(s) for s in v.shape) for v in ref_sd.values()])
        arrays["product_numel"] = np.array(sum(v.numel() for v in ref_sd.values()))
        return arrays
    finally:
        torch.set_default_dtype(torch.float32)


def to_bytes(arrays) -> bytes:
    buf = io.BytesIO()
    np.savez(buf, **arrays)
    return buf.getvalue()


if __name__ == "__main__":
    data = to_bytes(generate())
    if "--check" in sys.argv:
        same = open(OUT, "rb").read() == data
        print(f"{OUT}: {'reproduced bit for bit' if same else 'DIFFERS'}")
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as f:
        f.write(data)
    print(f"wrote {OUT} ({len(data)} bytes)")
