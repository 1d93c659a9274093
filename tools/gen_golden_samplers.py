#!/usr/bin/env python
"""Golden trajectories of the reference's OWN sampler classes (sgm/modules/diffusionmodules/sampling.py) for
panacea_amd.sampling's mirrors and pnc_cfg_sampler_step (needs the reference tree next to the checkout; CPU only):

  tests/golden/samplers.npz           every sampler of the table below around the closed-form `fake_network` of
                                      oracle/gen_golden.py, 3 and 25 steps: timesteps the network saw, final latent, and the
                                      noise the ancestral / churn samplers drew (torch.randn_like is patched for the run)
  tests/golden/samplers_tiny_net.npz  every sampler for 4 steps around the reference's tiny Panacea network: the latent after
                                      every step (LMS reaches order 4 on the last one).  Before writing, the classes
                                      `panacea_amd.dropin.install()` puts in the network's place, on the emulated kernels
                                      (tests/emu.py), must stay within TOL of max|x| at every step.

Every run uses DiscreteDenoiser(EpsScaling) + LegacyDDPMDiscretization + VanillaCFG(5).

    python tools/gen_golden_samplers.py
"""
from __future__ import annotations

import importlib
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
from oracle import ref_import                                  # noqa: E402
from oracle.gen_golden import GOLDEN, fake_network             # noqa: E402
from oracle.gen_golden_sampler_net import reference_stack, sampler_inputs   # noqa: E402
from panacea_amd import configs, synth                         # noqa: E402

P = "sgm.modules.diffusionmodules."
CFG_SCALE = 5.0
TINY_STEPS = 4
TOL = 1e-3          # |x_dropin - x_reference| per step, relative to max|x| (Euler measured 3.4e-4 on 3 steps)
CHURN = dict(s_churn=1.0, s_tmin=0.5, s_tmax=10.0)     # churn on the steps with 0.5 <= sigma <= 10 only
# name -> (reference class, its kwargs)
SAMPLERS = {
    "euler_churn": ("EulerEDMSampler", CHURN),
    "heun": ("HeunEDMSampler", {}),
    "heun_churn": ("HeunEDMSampler", CHURN),
    "euler_a": ("EulerAncestralSampler", {}),
    "dpmpp2s_a": ("DPMPP2SAncestralSampler", {}),
    "dpmpp2m": ("DPMPP2MSampler", {}),
    "lms": ("LinearMultistepSampler", {"order": 4}),
}


def make_sampler(ns, name, n):
    cls, kw = SAMPLERS[name]
    disc = {"target": P + "discretizer.LegacyDDPMDiscretization"}
    return getattr(ns.sp, cls)(num_steps=n, discretization_config=disc, device="cpu",
                               guider_config={"target": P + "guiders.VanillaCFG", "params": {"scale": CFG_SCALE}}, **kw)


class Recorder:
    """runs a reference sampler's own __call__ and records, without changing a bit of its arithmetic,
      * the timestep indices handed to the network,
      * every torch.randn_like draw (made from a seeded generator),
      * the latent after every step: the return value of `sampler_step` (its first element for DPM++ 2M, which returns
        (x, denoised)), or for LMS, which has no sampler_step, x at the step's network call + the `sum(...)` of its update
        (the module's `sum` is wrapped for the run: x_next = x + that sum, the same fp32 addition)."""

    def __init__(self, ns, seed=11):
        self.ns, self.g = ns, torch.Generator().manual_seed(seed)

    def run(self, smp, den, network, x0, c, uc):
        xs, seen, noise, x_in, sums = [], [], [], [], []
        real_randn = torch.randn_like

        def randn_like(x, *a, **k):
            z = torch.randn(x.shape, generator=self.g, dtype=x.dtype)
            noise.append(z.clone())
            return z
        patched = []
        if hasattr(smp, "sampler_step"):
            step = smp.sampler_step

            def recording_step(*a, **k):
                r = step(*a, **k)
                xs.append((r[0] if isinstance(r, tuple) else r).detach().clone())
                return r
            smp.sampler_step = recording_step
            patched.append(lambda: setattr(smp, "sampler_step", step))
        else:
            prep = smp.guider.prepare_inputs

            def recording_prep(x, s, cc, uu):
                x_in.append(x.detach().clone())
                return prep(x, s, cc, uu)
            smp.guider.prepare_inputs = recording_prep
            patched.append(lambda: delattr(smp.guider, "prepare_inputs"))

            def recording_sum(it, start=0):
                r = sum(it, start)
                sums.append(r.detach().clone())
                return r
            self.ns.sp.sum = recording_sum
            patched.append(lambda: delattr(self.ns.sp, "sum"))

        def net(x, t, cc):
            seen.append(t.clone())
            return network(x, t, cc)
        torch.randn_like = randn_like
        try:
            with torch.no_grad():
                out = smp(lambda inp, sigma, cc: den(net, inp, sigma, cc), x0.clone(), c, uc)
        finally:
            torch.randn_like = real_randn
            for undo in patched:
                undo()
        if not xs:
            xs = [a + b for a, b in zip(x_in, sums)]
        assert torch.equal(out, xs[-1])
        return torch.stack(xs), torch.stack(seen)[:, 0], (torch.stack(noise) if noise else torch.zeros(0))


def fake_vectors(ns, den):
    g = torch.Generator().manual_seed(5)                        # the inputs of tests/golden/sampler.npz
    x0 = torch.randn(2, 4, 4, 12, generator=g)
    c = {"crossattn": torch.randn(1, 77, 8, generator=g), "concat": torch.randn(2, 4, 4, 12, generator=g),
         "cond_feat": torch.rand(2, 19, 8, 8, generator=g)}
    uc = {"crossattn": torch.randn(1, 77, 8, generator=g), "concat": c["concat"].clone(), "cond_feat": c["cond_feat"].clone()}
    out = {"x0": x0.numpy(), "cfg_scale": np.float32(CFG_SCALE)}
    for name in SAMPLERS:
        for n in (3, 25):
            xs, ts, noise = Recorder(ns).run(make_sampler(ns, name, n), den, fake_network, x0, dict(c), dict(uc))
            out[f"{name}.{n}.timesteps"] = ts.numpy()
            out[f"{name}.{n}.x_final"] = xs[-1].numpy()
            out[f"{name}.{n}.noise"] = noise.numpy()
            print(f"{name:12s} {n:2d} steps: {len(ts)} network calls, {len(noise)} noise draws, |x| {float(xs[-1].abs().max()):.3f}")
    return out


def main():
    ns = ref_import.import_reference()
    for m in ("guiders", "discretizer", "denoiser_scaling", "denoiser_weighting", "sampling_utils"):
        importlib.import_module(P + m)
    den, _ = reference_stack(ns)
    np.savez_compressed(GOLDEN / "samplers.npz", **fake_vectors(ns, den))
    print("written tests/golden/samplers.npz")

    kw = configs.get("tiny")
    net, wrapper = ref_import.build_reference_network(ns, kw)
    sd = synth.synth_state_dict({k: list(v.shape) for k, v in net.state_dict().items()})
    net.load_state_dict(sd, strict=True)
    x0, c, uc = sampler_inputs(kw)
    ref = {name: Recorder(ns).run(make_sampler(ns, name, TINY_STEPS), den, wrapper, x0, dict(c), dict(uc)) for name in SAMPLERS}
    # the dropped-in classes, built by the reference's own instantiate_from_config, on the emulated kernels
    import emu
    from panacea_amd import dropin, engine as E
    dropin.install()
    wr = sys.modules["sgm.modules.diffusionmodules.wrappers"]
    cn_cfg = {"target": "sgm.modules.diffusionmodules.controlmodel.ControlNet3D", "params": dict(kw, hint_channels=19, control_scales=1.0)}
    mirror = ns.util.instantiate_from_config({"target": "sgm.modules.diffusionmodules.controlmodel.ControlledUNetModel3D",
                                              "params": dict(kw, controlnet_config=cn_cfg, out_channels=4)}).eval()
    assert type(mirror).__module__.startswith("panacea_amd"), "the drop-in did not take"
    mirror.load_state_dict(sd, strict=True)
    mwrap = wr.OpenAIWrapperControlLDM3D(mirror)
    out = {"x0": x0.numpy(), "steps": np.int32(TINY_STEPS), "cfg_scale": np.float32(CFG_SCALE), "tol_rel": np.float32(TOL)}
    for name, (xs_ref, t_ref, noise) in ref.items():
        with E.use_backend(emu):
            xs_mir, t_mir, _ = Recorder(ns).run(make_sampler(ns, name, TINY_STEPS), den, mwrap, x0, dict(c), dict(uc))
        assert torch.equal(t_ref, t_mir), name
        errs = [(a - b).abs().max().item() / a.abs().max().item() for a, b in zip(xs_ref, xs_mir)]
        print(f"{name:12s} timesteps {t_ref.tolist()}  drop-in (emulated) vs reference per step:", [f"{e:.2e}" for e in errs])
        assert max(errs) <= TOL, (name, errs)
        out.update({f"{name}.x_steps": xs_ref.numpy(), f"{name}.timesteps": t_ref.numpy(), f"{name}.noise": noise.numpy(),
                    f"{name}.dropin_emu_err_rel": np.asarray(errs, dtype=np.float32)})
    np.savez_compressed(GOLDEN / "samplers_tiny_net.npz", **out)
    print("written tests/golden/samplers_tiny_net.npz")


if __name__ == "__main__":
    main()
