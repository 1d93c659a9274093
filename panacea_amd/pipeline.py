"""Latents-in, frames-out composition of the pieces this package owns (hot path + f1 + f2 + f4):

    cond / uc  ->  EulerEDMSampler (or any sampler mirror) + VanillaCFG + DiscreteDenoiser (or any denoiser mirror) around the ControlNet-UNet (step invariants hoisted)
               ->  z / scale_factor  ->  FirstStageDecoder  ->  frames in [-1, 1]  (-> checkpoint.save_view_frames / save_gif)

which is what `DiffusionEngine3D.sample` + `decode_first_stage` do around the network (diffusion.py:138-151, 242-249;
`scale_factor` 0.18215, inference_nuscenes.yaml:5).  The text / image conditioners are not part of it:
`cond` and `uc` arrive as tensors.

`rollout_frames` chains such windows into a video of any length by conditioning, on one device: the `concat` of window k is the
first-stage encoding of a `final_cond_zero` clip (image.SparseClip) around an anchor frame, and the anchor of window k + 1 is a frame
window k decoded.

The first stages arrive as objects and carry their own operand policy (`FirstStageDecoder / FirstStageEncoder(..., precision=)`):
"fast" runs them on plain fp16 operands and fp16 weights; "precise-wide" / "precise-full" on fp16 pairs (and split weights), which
is what an fp32 checkpoint wants — the reference runs its first stage in fp32, and in a rollout the encoder's moments enter every
evaluation of the next window.  Nothing here changes with the policy.
"""
from __future__ import annotations

import math
import operator
from typing import Dict, Optional, Sequence, Tuple

import torch

from . import engine, image, sampling

SCALE_FACTOR = 0.18215


def _sampler_stack(dev, num_steps: int, cfg_scale: float, sampler, denoiser):
    """(sampler, denoiser) on `dev` from the `sampler` / `denoiser` arguments of sample_frames and rollout_frames"""
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
    return smp, den


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
    smp, den = _sampler_stack(noise.device, num_steps, cfg_scale, sampler, denoiser)
    with torch.no_grad():
        z = smp(sampling.BoundDenoiser(den, network), noise, cond, uc, network=network if hoist else None)
        return first_stage.decode_u8(z / scale_factor) if output == "uint8" else first_stage.decode(z / scale_factor)


def rollout_frames(network, first_stage_dec, first_stage_enc, anchor_u8: torch.Tensor, windows: Sequence[Tuple[Dict, Dict]],
                   noise: torch.Tensor, *, anchor: str = "last", share_noise_level: float = 0.07, sample_posterior: bool = True,
                   generator=None, num_steps: int = 25, cfg_scale: float = 5.0, hoist: bool = True,
                   scale_factor: float = SCALE_FACTOR, sampler=None, denoiser=None) -> torch.Tensor:
    """A video of W windows of T frames chained on one device by conditioning, the way the model reaches past one clip: window k
    is sampled with `concat` = the first-stage latents of a `final_cond_zero` clip (nuscenes_datasets_video.py:559-566) whose one
    given frame, the anchor, is `anchor_u8` for window 0 and a frame window k-1 generated for every later one.  Returns
    (N, H, W, 3) uint8 frames on the device in temporal order, N = T + (W - 1)(T - 1).

    anchor_u8: (H, W, 3) uint8.  windows: W pairs (cond, uc) as sample_frames takes them but WITHOUT `concat` (`cond_feat` float
    NCHW or the uint8 layout).  noise: (W, T, 4, h, w) unit-variance latents; T has to be the network's `num_frames`.
    anchor: "last" puts the anchor in slot T-1 (inference.py --use_last_frame, the reference's default), "first" in slot 0.

    Window k: c["concat"] and uc["concat"] each come from their own pass of image.SparseClip(anchor_k[None], [slot], T) through
    `scale_factor * first_stage_enc.encode_sparse_u8` — what VAEEmbedder does, twice, as get_unconditional_conditioning runs the
    conditioner twice: with `sample_posterior` two posterior draws from `generator`, c before uc; without, twice the posterior mean.
    The start latent is sampling.share_noise_init(noise[k], c["concat"], share_noise_level) (diffusion.py:242-249: `concat[-1]`
    whatever the anchor's slot).  The window is sampled and decoded by `first_stage_dec.decode_u8`, and the frame at the far end
    from the anchor — slot 0 for "last", slot T-1 for "first" — is anchor k+1, a slice of the decoded frames on the device.

    From window 1 on the anchor's slot depicts a frame that was already emitted and is dropped.  With "last" window k+1 lies BEFORE
    window k in time, so the result is [w_{W-1}[:-1], ..., w_1[:-1], w_0]; with "first" it is [w_0, w_1[1:], ...].  The layouts
    and text of the windows have to overlap by one frame in the same way: that is the caller's to arrange.

    Refused before the first launch: first stages without decode_u8 / encode_sparse_u8 (TypeError), a backend without the
    image-boundary kernels (NotImplementedError), a network carrying a frame or view shard (NotImplementedError: one device),
    T != num_frames and a malformed anchor, `noise` or window (ValueError).  Other arguments: see sample_frames."""
    if anchor not in ("last", "first"):
        raise ValueError(f"anchor: 'last' or 'first', got {anchor!r}")
    if not hasattr(first_stage_dec, "decode_u8"):
        raise TypeError(f"rollout_frames needs a first stage with decode_u8; {type(first_stage_dec).__name__} has none")
    if not hasattr(first_stage_enc, "encode_sparse_u8"):
        raise TypeError(f"rollout_frames needs a first stage with encode_sparse_u8; {type(first_stage_enc).__name__} has none")
    for name in ("tokens_to_u8", "u8_to_tokens_f16"):
        image.capability(engine.backend(), name)
    model = network.diffusion_model
    for m in (model, getattr(model, "controlnet", None)):
        if getattr(m, "frame_shard", None) is not None or getattr(m, "view_shard", None) is not None:
            raise NotImplementedError("rollout_frames runs on one device: the network carries a frame or view shard")
    windows = list(windows)
    if not isinstance(noise, torch.Tensor) or noise.dim() != 5 or noise.shape[0] != len(windows) or not windows:
        raise ValueError(f"noise: (W, T, 4, h, w) with one entry per window ({len(windows)}), got "
                         f"{tuple(noise.shape) if isinstance(noise, torch.Tensor) else type(noise).__name__}")
    T, (h, w) = noise.shape[1], noise.shape[3:]
    if T != model.num_frames:
        raise ValueError(f"noise carries {T} frames per window, the network was built for num_frames = {model.num_frames}")
    if (not isinstance(anchor_u8, torch.Tensor) or anchor_u8.dtype != torch.uint8 or anchor_u8.dim() != 3 or anchor_u8.shape[2] != 3
            or anchor_u8.shape[0] % h or anchor_u8.shape[1] % w or anchor_u8.shape[0] // h != anchor_u8.shape[1] // w):
        raise ValueError(f"anchor_u8: one (H, W, 3) uint8 frame at a multiple of the {h} x {w} latent, got "
                         f"{tuple(anchor_u8.shape) if isinstance(anchor_u8, torch.Tensor) else type(anchor_u8).__name__}"
                         f"{' ' + str(anchor_u8.dtype) if isinstance(anchor_u8, torch.Tensor) else ''}")
    for k, pair in enumerate(windows):
        if len(pair) != 2 or not all(isinstance(d, dict) for d in pair):
            raise ValueError(f"windows[{k}]: a (cond, uc) pair of dicts expected")
        if any("concat" in d for d in pair):
            raise ValueError(f"windows[{k}] carries `concat`: rollout_frames builds it from the window's anchor")
    smp, den = _sampler_stack(noise.device, num_steps, cfg_scale, sampler, denoiser)
    slot, far = (T - 1, 0) if anchor == "last" else (0, T - 1)
    frame, out = anchor_u8.to(noise.device), []
    with torch.no_grad():
        for k, (cond, uc) in enumerate(windows):
            clip = image.SparseClip(frame[None], (slot,), T)
            c, u = (dict(d, concat=scale_factor * first_stage_enc.encode_sparse_u8(clip, generator=generator, sample=sample_posterior))
                    for d in (cond, uc))
            x0 = sampling.share_noise_init(noise[k], c["concat"], share_noise_level)
            z = smp(sampling.BoundDenoiser(den, network), x0, c, u, network=network if hoist else None)
            frames = first_stage_dec.decode_u8(z / scale_factor)
            frame = frames[far]
            out.append(frames if k == 0 else frames[:-1] if anchor == "last" else frames[1:])
    return torch.cat(out[::-1] if anchor == "last" else out)


def edit_start_step(strength: float, num_steps: int) -> int:
    """the schedule index an edit of `strength` in (0, 1] starts at: min(num_steps - 1, floor((1 - strength) * num_steps)).  1.0
    starts at the first sigma (the clip only seeds the noise's mean), a small strength runs the last steps only."""
    if isinstance(strength, bool) or not isinstance(strength, (int, float)) or not 0.0 < strength <= 1.0:
        raise ValueError(f"strength: a number in (0, 1], got {strength!r}")
    return min(num_steps - 1, int(math.floor((1.0 - strength) * num_steps)))


def edit_frames(network, first_stage_dec, first_stage_enc, frames_u8: torch.Tensor, cond: Dict[str, torch.Tensor],
                uc: Dict[str, torch.Tensor], noise: torch.Tensor, *, strength: float = 0.6, keep: Sequence[int] = (),
                num_steps: int = 25, cfg_scale: float = 5.0, sampler=None, denoiser=None, generator=None,
                sample_posterior: bool = True, scale_factor: float = SCALE_FACTOR, hoist: bool = True, callback=None,
                keep_mask_u8: Optional[torch.Tensor] = None) -> torch.Tensor:
    """A recorded clip re-rendered under `cond` / `uc` (another prompt, another layout), on one device: frames_u8 (T, H, W, 3) uint8
    -> (T, H, W, 3) uint8.  The clip is encoded (z = scale_factor * first_stage_enc.encode_u8(frames_u8): a posterior draw from
    `generator`, or the mean without `sample_posterior`), noised to the level the schedule has at
    start_step = edit_start_step(strength, num_steps) with the ONE draw `noise` (T, 4, h, w), sampled from there on, and decoded by
    first_stage_dec.decode_u8(z_out / scale_factor).  The frame slots in `keep` come out as the clip's own latents (what the first
    stage makes of the recorded frames): they are put back at every noise level (sampling.ClipSource), so the frames between them
    are generated next to them — keep=(0, T - 1) fills in between two given frames.

    cond, uc: as sample_frames takes them, `concat` included.  T has to be the network's `num_frames`.  sampler, denoiser, num_steps,
    cfg_scale, hoist: see sample_frames; kept frames need a sampler that serves them (sampling.ClipSource).  `callback(i, x)` sees the
    latent after every step.

    `keep_mask_u8` (region editing): a (T, H, W) uint8 mask of the clip's size, nonzero = this pixel is kept — a camera view
    (image.view_mask), everything outside a rectangle (image.rect_mask), any region.  The clip is encoded as without it; the mask
    is pooled to the latent (image.pool_keep_mask at f = H / h: a latent cell counts as known only where all of its f x f pixels
    are kept), the sampler runs on ClipSource(z, noise, keep, mask=pooled), which puts the kept cells back at every noise level, and
    the result is image.select_u8(frames_u8, decoded, keep_mask_u8): every kept pixel is the recorded byte itself, not the first
    stage's reconstruction of it.  Frames in `keep` that the mask does not cover stay that reconstruction.  Generated pixels right
    at the seam see kept latents through the decoder's receptive field; the kept region is not eroded for it.  None: the path above,
    launch for launch.

    Refused before the first launch: a malformed `keep_mask_u8` (ValueError), a backend without the region-editing kernels it needs
    (NotImplementedError), a sampler that does not keep frames given a mask (NotImplementedError), first stages without encode_u8 / decode_u8 (TypeError), a backend without pnc_frames_renoise or
    the image-boundary kernels (NotImplementedError), a network carrying a frame or view shard (NotImplementedError: one device), a
    malformed clip or `noise`, T != num_frames, `strength` outside (0, 1] and `keep` slots outside 0 .. T-1 (ValueError)."""
    if not hasattr(first_stage_dec, "decode_u8"):
        raise TypeError(f"edit_frames needs a first stage with decode_u8; {type(first_stage_dec).__name__} has none")
    if not hasattr(first_stage_enc, "encode_u8"):
        raise TypeError(f"edit_frames needs a first stage with encode_u8; {type(first_stage_enc).__name__} has none")
    for name in ("tokens_to_u8", "u8_to_tokens_f16"):
        image.capability(engine.backend(), name)
    sampling._renoise_capability()
    model = network.diffusion_model
    for m in (model, getattr(model, "controlnet", None)):
        if getattr(m, "frame_shard", None) is not None or getattr(m, "view_shard", None) is not None:
            raise NotImplementedError("edit_frames runs on one device: the network carries a frame or view shard")
    if not isinstance(noise, torch.Tensor) or noise.dim() != 4 or 0 in noise.shape:
        raise ValueError(f"noise: one (T, 4, h, w) draw, got "
                         f"{tuple(noise.shape) if isinstance(noise, torch.Tensor) else type(noise).__name__}")
    T, (h, w) = noise.shape[0], noise.shape[2:]
    if T != model.num_frames:
        raise ValueError(f"noise carries {T} frames, the network was built for num_frames = {model.num_frames}")
    f = frames_u8
    if (not isinstance(f, torch.Tensor) or f.dtype != torch.uint8 or f.dim() != 4 or f.shape[0] != T or f.shape[3] != 3
            or f.shape[1] % h or f.shape[2] % w or f.shape[1] // h != f.shape[2] // w):
        raise ValueError(f"frames_u8: a ({T}, H, W, 3) uint8 clip at a multiple of the {h} x {w} latent, got "
                         f"{tuple(f.shape) if isinstance(f, torch.Tensor) else type(f).__name__}"
                         f"{' ' + str(f.dtype) if isinstance(f, torch.Tensor) else ''}")
    try:
        keep = tuple(operator.index(s) for s in keep)
    except TypeError:
        raise ValueError(f"keep: frame slots (integers) expected, got {keep!r}") from None
    if any(not 0 <= s < T for s in keep) or len(set(keep)) != len(keep):
        raise ValueError(f"keep: distinct frame slots in 0 .. {T - 1} expected, got {keep}")
    if keep_mask_u8 is not None:
        keep_mask_u8 = image.keep_mask_u8(keep_mask_u8, T, f.shape[1], f.shape[2])
        if f.shape[1] // h > 16:
            raise ValueError(f"keep_mask_u8: the mask pools by at most 16, the clip is {f.shape[1] // h} times the latent")
        for name in ("mask_pool_u8", "u8_select"):
            image.region_capability(engine.backend(), name)
        sampling._masked_capability()
    smp, den = _sampler_stack(noise.device, num_steps, cfg_scale, sampler, denoiser)
    start_step = edit_start_step(strength, smp.num_steps)
    why = smp._keep_refusal() if keep or keep_mask_u8 is not None else None
    if why is not None:
        raise NotImplementedError(f"{type(smp).__name__} does not keep frames {why}")
    with torch.no_grad():
        z = scale_factor * first_stage_enc.encode_u8(f.to(noise.device), generator=generator, sample=sample_posterior)
        if z.shape != noise.shape:
            raise ValueError(f"the first stage encodes the clip to {tuple(z.shape)}, noise is {tuple(noise.shape)}")
        pooled = None
        if keep_mask_u8 is not None:
            keep_mask_u8 = keep_mask_u8.to(noise.device)
            pooled = image.pool_keep_mask(keep_mask_u8, h, w)
        source = sampling.ClipSource(z.to(torch.float32), noise.to(torch.float32), keep, mask=pooled)
        z_out = smp(sampling.BoundDenoiser(den, network), None, cond, uc, network=network if hoist else None, callback=callback,
                    start_step=start_step, source=source)
        decoded = first_stage_dec.decode_u8(z_out / scale_factor)
        return decoded if keep_mask_u8 is None else image.select_u8(f.to(noise.device), decoded, keep_mask_u8)
