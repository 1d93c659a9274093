#!/usr/bin/env python
"""Golden numbers of the reference's OWN denoiser classes (sgm/modules/diffusionmodules/denoiser.py, denoiser_scaling.py,
discretizer.py) under its own samplers, for panacea_amd.sampling's Denoiser / DiscreteDenoiser / VScaling / EDMScaling /
EDMDiscretization mirrors and the general-skip exit kernels (needs the reference tree next to the checkout; CPU only):

  tests/golden/denoisers.npz           * EDMDiscretization sigmas and the four coefficients of every scaling on a sigma vector;
                                       * every case of tests/denoiser_cases.py (v + discrete quantised, v + discrete with a float
                                         c_noise, EDM scaling + continuous Denoiser + EDMDiscretization, eps + continuous Denoiser)
                                         under Euler, Heun, DPM++ 2M and ancestral Euler around the closed-form `fake_network` of
                                         oracle/gen_golden.py, 3 and 25 steps: the c_noise the network saw, the final latent and
                                         the noise drawn
  tests/golden/denoisers_tiny_net.npz  every case for 4 steps of Euler and DPM++ 2M around the reference's tiny Panacea network:
                                       the latent after every step.  Before writing, the classes `panacea_amd.dropin.install()`
                                       puts in the network's place, on the emulated kernels (tests/emu.py),
                                       must stay within tol_rel of max|x| at every step; tol_rel is the bound
                                       tests/golden/samplers_tiny_net.npz carries for this network, copied.

    python tools/gen_golden_denoisers.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
from oracle import ref_import                                  # noqa: E402
from oracle.gen_golden import GOLDEN, fake_network             # noqa: E402
from oracle.gen_golden_sampler_net import sampler_inputs       # noqa: E402
from gen_golden_samplers import Recorder                      # noqa: E402
from denoiser_cases import CASES, EDM_SCHEDULES, SAMPLERS, SCALINGS, TINY_SAMPLERS, CFG_SCALE, sampler_config   # noqa: E402
from panacea_amd import configs, synth                         # noqa: E402

TINY_STEPS = 4
SIGMAS = [0.0292, 0.1, 0.5, 1.0, 2.5, 14.6146, 80.0]           # the scalings are evaluated on these


def build(ns, cfg):
    return ns.util.instantiate_from_config(cfg)


def table(ns):
    """the reference's discretization and scalings as numbers"""
    out = {"scaling.sigma": np.asarray(SIGMAS, dtype=np.float32)}
    sig = torch.tensor(SIGMAS, dtype=torch.float32)
    for name, (cls, kw) in SCALINGS.items():
        coeffs = build(ns, {"target": "sgm.modules.diffusionmodules.denoiser_scaling." + cls, "params": kw})(sig)
        for k, v in zip(("c_skip", "c_out", "c_in", "c_noise"), coeffs):
            out[f"scaling.{name}.{k}"] = v.numpy()
    for name, (kw, n) in EDM_SCHEDULES.items():
        disc = build(ns, {"target": "sgm.modules.diffusionmodules.discretizer.EDMDiscretization", "params": kw})
        out[f"edm_sigmas.{name}"] = disc(n).numpy()
        out[f"edm_sigmas.{name}.flipped_no_zero"] = disc(n, do_append_zero=False, flip=True).numpy()
    return out


def fake_trajectories(ns):
    g = torch.Generator().manual_seed(5)                        # the inputs of tests/sampler_cases.py: fake_inputs()
    x0 = torch.randn(2, 4, 4, 12, generator=g)
    c = {"crossattn": torch.randn(1, 77, 8, generator=g), "concat": torch.randn(2, 4, 4, 12, generator=g),
         "cond_feat": torch.rand(2, 19, 8, 8, generator=g)}
    uc = {"crossattn": torch.randn(1, 77, 8, generator=g), "concat": c["concat"].clone(), "cond_feat": c["cond_feat"].clone()}
    out = {"x0": x0.numpy(), "cfg_scale": np.float32(CFG_SCALE)}
    for case, (den_cfg, *_rest) in CASES.items():
        den = build(ns, den_cfg)
        for smp_name in SAMPLERS:
            for n in (3, 25):
                smp = build(ns, _cpu(sampler_config(case, smp_name, n)))
                xs, seen, noise = Recorder(ns).run(smp, den, fake_network, x0, dict(c), dict(uc))
                key = f"{case}.{smp_name}.{n}"
                out[key + ".c_noise"], out[key + ".x_final"], out[key + ".noise"] = seen.numpy(), xs[-1].numpy(), noise.numpy()
                print(f"{key:32s}: {len(seen)} network calls, c_noise {seen.dtype} {seen[0].item():.6g} .. {seen[-1].item():.6g}, "
                      f"{len(noise)} noise draws, |x| {float(xs[-1].abs().max()):.3f}")
    return out


def _cpu(cfg):
    cfg = dict(cfg, params=dict(cfg["params"], device="cpu"))
    return cfg


def tiny_trajectories(ns):
    import emu
    from panacea_amd import dropin, engine as E
    kw = configs.get("tiny")
    net, wrapper = ref_import.build_reference_network(ns, kw)
    sd = synth.synth_state_dict({k: list(v.shape) for k, v in net.state_dict().items()})
    net.load_state_dict(sd, strict=True)
    x0, c, uc = sampler_inputs(kw)
    runs = [(case, s) for case in CASES for s in TINY_SAMPLERS]
    ref = {}
    for case, s in runs:
        ref[case, s] = Recorder(ns).run(build(ns, _cpu(sampler_config(case, s, TINY_STEPS))), build(ns, CASES[case][0]), wrapper, x0,
                                        dict(c), dict(uc))
    # the dropped-in classes, built by the reference's own instantiate_from_config, on the emulated kernels
    dropin.install()
    wr = sys.modules["sgm.modules.diffusionmodules.wrappers"]
    cn_cfg = {"target": "sgm.modules.diffusionmodules.controlmodel.ControlNet3D", "params": dict(kw, hint_channels=19, control_scales=1.0)}
    mirror = ns.util.instantiate_from_config({"target": "sgm.modules.diffusionmodules.controlmodel.ControlledUNetModel3D",
                                              "params": dict(kw, controlnet_config=cn_cfg, out_channels=4)}).eval()
    assert type(mirror).__module__.startswith("panacea_amd"), "the drop-in did not take"
    mirror.load_state_dict(sd, strict=True)
    mwrap = wr.OpenAIWrapperControlLDM3D(mirror)
    tol = np.load(GOLDEN / "samplers_tiny_net.npz")["tol_rel"]          # the bound this network already carries under `precise`
    out = {"x0": x0.numpy(), "steps": np.int32(TINY_STEPS), "cfg_scale": np.float32(CFG_SCALE), "tol_rel": np.float32(tol)}
    for case, s in runs:
        xs_ref, t_ref, noise = ref[case, s]
        with E.use_backend(emu):
            xs_mir, t_mir, _ = Recorder(ns).run(build(ns, _cpu(sampler_config(case, s, TINY_STEPS))), build(ns, CASES[case][0]), mwrap,
                                                x0, dict(c), dict(uc))
        assert torch.equal(t_ref, t_mir), (case, s)
        errs = [(a - b).abs().max().item() / a.abs().max().item() for a, b in zip(xs_ref, xs_mir)]
        print(f"{case + '.' + s:28s} c_noise {[round(v, 5) for v in t_ref.tolist()]}  drop-in (emulated) vs reference per step:",
              [f"{e:.2e}" for e in errs])
        assert max(errs) <= float(tol), (case, s, errs)
        key = f"{case}.{s}"
        out.update({key + ".x_steps": xs_ref.numpy(), key + ".c_noise": t_ref.numpy(), key + ".noise": noise.numpy(),
                    key + ".dropin_emu_err_rel": np.asarray(errs, dtype=np.float32)})
    return out


def main():
    import importlib
    ns = ref_import.import_reference()
    for m in ("guiders", "discretizer", "denoiser_scaling", "denoiser_weighting", "sampling_utils"):
        importlib.import_module("sgm.modules.diffusionmodules." + m)
    out = table(ns)
    out.update(fake_trajectories(ns))
    np.savez_compressed(GOLDEN / "denoisers.npz", **out)
    print("written tests/golden/denoisers.npz")
    np.savez_compressed(GOLDEN / "denoisers_tiny_net.npz", **tiny_trajectories(ns))
    print("written tests/golden/denoisers_tiny_net.npz")


if __name__ == "__main__":
    main()
