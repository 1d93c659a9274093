"""Latents-in, frames-out composition of the pieces this package owns (hot path + f1 + f2 + f4):

    cond / uc  ->  EulerEDMSampler (or any sampler mirror) + VanillaCFG + DiscreteDenoiser (or any denoiser mirror) around the ControlNet-UNet (step invariants hoisted)
               ->  z / scale_factor  ->  FirstStageDecoder  ->  frames in [-1, 1]  (-> checkpoint.save_view_frames / save_gif)

which is what `DiffusionEngine3D.sample` + `decode_first_stage` do around the network (diffusion.py:138-151, 242-249;
`scale_factor` 0.18215, inference_nuscenes.yaml:5).  The text / image conditioners are not part of it:
`cond` and `uc` arrive as tensors.
"""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import engine, image, sampling

SCALE_FACTOR = 0.18215


def sample_frames(network, first_stage, cond: Dict[str, torch.Tensor], uc: Dict[str, torch.Tensor],
                  noise: torch.Tensor, num_steps: int = 25, cfg_scale: float = 5.0, hoist: bool = True,
                  scale_factor: float = SCALE_FACTOR, sampler=None, denoiser=None, output: str = "float") -> torch.Tensor:
    """noise: (T, 4, h, w) unit-variance latents of ONE sample; returns (T, 3, 8h, 8w) frames.  T is taken from `noise` and has
    to be the `num_frames` the network was built with (configs.with_frames), 1 <= T <= 16: the temporal kernels hold at most 16
    frames of a pixel, and a network for a longer clip is refused when it is built.
    `sampler`: None = the YAML's 25-step Euler / CFG `cfg_scale` (num_steps, cfg_scale apply); a sampler mirror of
    panacea_amd.sampling; or a reference `sampler_config` dict (sampling.from_config; its num_steps, else `num_steps`).
    `denoiser`: None = the YAML's DiscreteDenoiser with EpsScaling; a denoiser mirror of panacea_amd.sampling (Denoiser or
    DiscreteDenoiser with EpsScaling / VScaling / EDMScaling); or a reference `denoiser_config` dict
    (sampling.denoiser_from_config).
    `output`: "float" = (T, 3, 8h, 8w) frames in [-1, 1]; "uint8" = (T, 8h, 8w, 3) uint8 frames on the device, quantised from the
    decoder's token matrix (FirstStageDecoder.decode_u8) — what checkpoint.save_view_frames / save_gif write for the float frames.
    `cond["cond_feat"]` / `uc["cond_feat"]` may be the dataset's uint8 channels-last BEV layout (T, 8h, 8w, C)."""
    if output not in ("float", "uint8"):
        raise ValueError(f"output: 'float' or 'uint8', got {output!r}")
    if output == "uint8":               # refused before the first step, not after the last
        if not hasattr(first_stage, "decode_u8"):
            raise TypeError(f"output='uint8' needs a first stage with decode_u8; {type(first_stage).__name__} has none")
        image.capability(engine.backend(), "tokens_to_u8")
    dev = noise.device
    if denoiser is None:
        den = sampling.DiscreteDenoiser()
    else:
        den = sampling.denoiser_from_config(denoiser) if isinstance(denoiser, dict) else denoiser
        if not isinstance(den, sampling.Denoiser):
            raise TypeError(f"denoiser: a panacea_amd.sampling denoiser mirror or a denoiser_config dict (got {type(den).__name__})")
    den = den.to(dev)
    if sampler is None:
        smp = sampling.EulerEDMSampler(num_steps, guider=sampling.VanillaCFG(cfg_scale), device=dev)
    else:
        smp = sampling.from_config(sampler, device=dev) if isinstance(sampler, dict) else sampler
        if smp.num_steps is None:
            smp.num_steps = num_steps
    with torch.no_grad():
        z = smp(sampling.BoundDenoiser(den, network), noise, cond, uc, network=network if hoist else None)
        return first_stage.decode_u8(z / scale_factor) if output == "uint8" else first_stage.decode(z / scale_factor)
