"""What tests/test_denoisers.py, tests/test_denoisers_gpu.py and tools/gen_golden_denoisers.py share: the denoiser
parameterisations of tests/golden/denoisers*.npz as reference-style config dicts (the YAML's `denoiser_config` and the
`discretization_config` of its `sampler_config`), and the samplers each runs under."""
from panacea_amd import sampling as S

P = "sgm.modules.diffusionmodules."
CFG_SCALE = 5.0
_DDPM = {"target": P + "discretizer.LegacyDDPMDiscretization"}
_EDM = {"target": P + "discretizer.EDMDiscretization", "params": {"sigma_min": 0.02, "sigma_max": 80.0, "rho": 7.0}}


def _discrete(scaling, weighting, **kw):
    return {"target": P + "denoiser.DiscreteDenoiser",
            "params": dict(weighting_config={"target": P + "denoiser_weighting." + weighting},
                           scaling_config={"target": P + "denoiser_scaling." + scaling}, num_idx=1000,
                           discretization_config=_DDPM, **kw)}


def _continuous(scaling, weighting, **scaling_params):
    sc = {"target": P + "denoiser_scaling." + scaling}
    if scaling_params:
        sc["params"] = scaling_params
    return {"target": P + "denoiser.Denoiser",
            "params": dict(weighting_config={"target": P + "denoiser_weighting." + weighting}, scaling_config=sc)}


# name -> (denoiser_config, the sampler's discretization_config, mirror denoiser class, mirror scaling class, float c_noise?)
CASES = {
    "v_quantised": (_discrete("VScaling", "VWeighting"), _DDPM, S.DiscreteDenoiser, S.VScaling, False),
    "v_float": (_discrete("VScaling", "VWeighting", quantize_c_noise=False), _DDPM, S.DiscreteDenoiser, S.VScaling, True),
    "edm_continuous": (_continuous("EDMScaling", "EDMWeighting", sigma_data=0.5), _EDM, S.Denoiser, S.EDMScaling, True),
    "eps_continuous": (_continuous("EpsScaling", "EpsWeighting"), _DDPM, S.Denoiser, S.EpsScaling, True),
}
# name -> (sampler class name, kwargs); the tiny-network fixture runs TINY_SAMPLERS only
SAMPLERS = {
    "euler": ("EulerEDMSampler", {}),
    "heun": ("HeunEDMSampler", {}),
    "dpmpp2m": ("DPMPP2MSampler", {}),
    "euler_a": ("EulerAncestralSampler", {}),
}
TINY_SAMPLERS = ("euler", "dpmpp2m")
SCALINGS = {"eps": ("EpsScaling", {}), "v": ("VScaling", {}), "edm": ("EDMScaling", {"sigma_data": 0.5}),
            "edm_sd1": ("EDMScaling", {"sigma_data": 1.0})}
EDM_SCHEDULES = {"default3": ({}, 3), "default25": ({}, 25), "custom10": ({"sigma_min": 0.002, "sigma_max": 120.0, "rho": 5.0}, 10)}


def sampler_config(case, sampler, n, scale=CFG_SCALE):
    cls, kw = SAMPLERS[sampler]
    return {"target": P + "sampling." + cls,
            "params": dict(num_steps=n, discretization_config=CASES[case][1],
                           guider_config={"target": P + "guiders.VanillaCFG", "params": {"scale": scale}}, **kw)}


def make(case, sampler, n, device="cpu", scale=CFG_SCALE):
    """(denoiser mirror, sampler mirror) of a case, built from the reference-style dicts"""
    return S.denoiser_from_config(CASES[case][0]).to(device), S.from_config(sampler_config(case, sampler, n, scale), device=device)
