"""The callers either side of the hot path: discretisation, discrete denoiser with
eps-scaling, classifier-free guidance and the Euler sampler of `configs/inference_nuscenes.yaml`.

Host-side mirrors with the reference's names and call signatures
  LegacyDDPMDiscretization   sgm/modules/diffusionmodules/discretizer.py:42-69
  EDMDiscretization          .../discretizer.py:28-39
  EpsScaling, VScaling, EDMScaling   .../denoiser_scaling.py:4-31
  Denoiser, DiscreteDenoiser .../denoiser.py:6-63 (`denoiser_from_config` builds either from the YAML's denoiser_config)
  VanillaCFG                 .../guiders.py:8-40 (+ sampling_utils.py:7-9)
  EulerEDMSampler            .../sampling.py:27-133,214-218 (+ churn)
  HeunEDMSampler, EulerAncestralSampler, DPMPP2SAncestralSampler, DPMPP2MSampler, LinearMultistepSampler
                             .../sampling.py:135-365 (+ sampling_utils.py:12-43); `from_config` builds any of them from the
                             YAML's sampler_config
written for a device-resident loop: the sigma schedule is a Python list of floats plus one device tensor
(no `.item()` sync per step — the reference compares Python floats with a device element at
sampling.py:118-122), and every per-step quantity (c_in, c_out, timestep index) is a host scalar.
These are a handful of elementwise torch ops per step; the arithmetic that matters is in the network.
"""
from __future__ import annotations

import operator
from typing import Callable, Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn


def append_dims(x: torch.Tensor, target_dims: int) -> torch.Tensor:
    return x[(...,) + (None,) * (target_dims - x.ndim)]


class LegacyDDPMDiscretization:
    """discretizer.py:42-69 — sigma_i = sqrt((1 - abar_i) / abar_i) of the 1000-step linear-beta DDPM schedule."""

    def __init__(self, linear_start=0.00085, linear_end=0.0120, num_timesteps=1000):
        self.num_timesteps = num_timesteps
        betas = np.linspace(linear_start ** 0.5, linear_end ** 0.5, num_timesteps, dtype=np.float64) ** 2
        self.alphas_cumprod = np.cumprod(1.0 - betas, axis=0)

    def get_sigmas(self, n, device="cpu"):
        if n < self.num_timesteps:
            ts = np.linspace(self.num_timesteps - 1, 0, n, endpoint=False).astype(int)[::-1]
            ac = self.alphas_cumprod[ts]
        elif n == self.num_timesteps:
            ac = self.alphas_cumprod
        else:
            raise ValueError("more sampling steps than training timesteps")
        sig = torch.tensor((1 - ac) / ac, dtype=torch.float32, device=device) ** 0.5
        return torch.flip(sig, (0,))

    def __call__(self, n, do_append_zero=True, device="cpu", flip=False):
        s = self.get_sigmas(n, device=device)
        if do_append_zero:
            s = torch.cat([s, s.new_zeros([1])])
        return s if not flip else torch.flip(s, (0,))


class EDMDiscretization:
    """discretizer.py:28-39 — Karras et al.'s rho-schedule: sigma_i = (smax^(1/rho) + i/(n-1) (smin^(1/rho) - smax^(1/rho)))^rho,
    the ramp and the power in fp32 torch ops, the two roots Python floats.  The n values are computed on the HOST and moved to
    `device`: a device's linspace and powf are not the host's to the bit, and the samplers decide their branches from the host copy
    of the schedule (`_Sampler.host_sigmas`) — so the device holds exactly the sigmas the host reasons about, on any device.  At
    sigma_max = 80 the initial latent is ~250, where one ulp of sigma moves a 3-step Heun trajectory by several 1e-5."""

    def __init__(self, sigma_min=0.02, sigma_max=80.0, rho=7.0):
        self.sigma_min, self.sigma_max, self.rho = sigma_min, sigma_max, rho

    def get_sigmas(self, n, device="cpu"):
        ramp = torch.linspace(0, 1, n)
        lo, hi = self.sigma_min ** (1 / self.rho), self.sigma_max ** (1 / self.rho)
        return ((hi + ramp * (lo - hi)) ** self.rho).to(device)

    def __call__(self, n, do_append_zero=True, device="cpu", flip=False):
        s = self.get_sigmas(n, device=device)
        if do_append_zero:
            s = torch.cat([s, s.new_zeros([1])])
        return s if not flip else torch.flip(s, (0,))


# The scalings return (c_skip, c_out, c_in, c_noise).  Each coefficient is the reference's torch expression with its operations in
# the reference's order: a fused step computes its [T] vectors with these very calls, so they are the plain step's bits.
class EpsScaling:
    """denoiser_scaling.py:16-22"""

    def __call__(self, sigma):
        return torch.ones_like(sigma), -sigma, 1 / (sigma ** 2 + 1.0) ** 0.5, sigma.clone()


class VScaling:
    """denoiser_scaling.py:25-31 — v-prediction: c_skip = 1 / (sigma^2 + 1), c_out = -sigma / sqrt(sigma^2 + 1)"""

    def __call__(self, sigma):
        return 1.0 / (sigma ** 2 + 1.0), -sigma / (sigma ** 2 + 1.0) ** 0.5, 1.0 / (sigma ** 2 + 1.0) ** 0.5, sigma.clone()


class EDMScaling:
    """denoiser_scaling.py:4-13 — Karras et al.'s preconditioning; c_noise = log(sigma) / 4 is a float"""

    def __init__(self, sigma_data=0.5):
        self.sigma_data = sigma_data

    def __call__(self, sigma):
        sd = self.sigma_data
        return (sd ** 2 / (sigma ** 2 + sd ** 2), sigma * sd / (sigma ** 2 + sd ** 2) ** 0.5, 1 / (sigma ** 2 + sd ** 2) ** 0.5,
                0.25 * sigma.log())


class Denoiser(nn.Module):
    """denoiser.py:6-28 — the continuous denoiser: sigma is used as it comes, and the network is handed the scaling's c_noise as
    a FLOAT (nn.util.timestep_embedding evaluates it in fp32)."""

    def __init__(self, scaling=None):
        super().__init__()
        self.scaling = scaling or EpsScaling()

    def possibly_quantize_sigma(self, sigma):
        return sigma

    def possibly_quantize_c_noise(self, c_noise):
        return c_noise

    def coefficients(self, sigma):
        """(c_skip, c_out, c_in, c_noise) for a [T] sigma, as __call__ forms them (the fused step's per-frame vectors)"""
        c_skip, c_out, c_in, c_noise = self.scaling(self.possibly_quantize_sigma(sigma))
        return c_skip, c_out, c_in, self.possibly_quantize_c_noise(c_noise)

    def __call__(self, network: Callable, input: torch.Tensor, sigma: torch.Tensor, cond: Dict) -> torch.Tensor:
        sigma = self.possibly_quantize_sigma(sigma)
        shape = sigma.shape
        sigma = append_dims(sigma, input.ndim)
        c_skip, c_out, c_in, c_noise = self.scaling(sigma)
        c_noise = self.possibly_quantize_c_noise(c_noise.reshape(shape))
        return network(input * c_in, c_noise, cond) * c_out + input * c_skip


class DiscreteDenoiser(Denoiser):
    """denoiser.py:31-63: snaps sigma to the `num_idx`-entry table of the discretization; with quantize_c_noise (the default) the
    network is handed the table INDEX of c_noise, else the float c_noise of the snapped sigma.  `scaling`: EpsScaling (default),
    VScaling or EDMScaling."""

    def __init__(self, num_idx=1000, discretization=None, do_append_zero=False, quantize_c_noise=True, flip=True, scaling=None):
        super().__init__(scaling)
        disc = discretization or LegacyDDPMDiscretization()
        self.register_buffer("sigmas", disc(num_idx, do_append_zero=do_append_zero, flip=flip))
        self.quantize_c_noise = quantize_c_noise

    def sigma_to_idx(self, sigma):
        return (sigma - self.sigmas[:, None]).abs().argmin(dim=0).view(sigma.shape)

    def idx_to_sigma(self, idx):
        return self.sigmas[idx]

    def possibly_quantize_sigma(self, sigma):
        return self.idx_to_sigma(self.sigma_to_idx(sigma))

    def possibly_quantize_c_noise(self, c_noise):
        return self.sigma_to_idx(c_noise) if self.quantize_c_noise else c_noise


class VanillaCFG:
    """guiders.py:8-40: batch-doubling (uncond half first) and x_u + s (x_c - x_u)."""
    KEYS = ("vector", "crossattn", "concat", "cond_feat", "cond_bev_feat")

    def __init__(self, scale, dyn_thresh_config=None):
        self.scale = scale

    def __call__(self, x, sigma):
        x_u, x_c = x.chunk(2)
        return x_u + self.scale * (x_c - x_u)

    def prepare_inputs(self, x, s, c, uc):
        c_out = {}
        pre = c.get("_cat")                       # hoist_invariants(): uc|c already concatenated once per schedule
        for k in c:
            if k == "_cat":
                continue
            if k in self.KEYS:
                c_out[k] = pre[k] if pre is not None else torch.cat((uc[k], c[k]), 0)
            else:
                assert c[k] is uc[k] or c[k] == uc[k]
                c_out[k] = c[k]
        return torch.cat([x] * 2), torch.cat([s] * 2), c_out


def _same_tensor(a: torch.Tensor, b: torch.Tensor) -> bool:
    """the two names refer to the same values in the same memory (identity of content without reading it)"""
    return a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride() and a.dtype == b.dtype
                      and a.device == b.device)


class BoundDenoiser:
    """`lambda input, sigma, c: denoiser(model, input, sigma, c)` of DiffusionEngine3D.sample (diffusion.py:251-253) as an
    object: the sampler can see which denoiser and which network it drives and run the whole step on the device — the
    c_in scaling and the CFG batch doubling folded into the network's entry kernel, c_out / c_skip + CFG combine + Euler
    update in ONE exit kernel on the network's channels-last output.  Calling it is exactly the lambda."""

    def __init__(self, denoiser: "Denoiser", network):
        self.denoiser, self.network = denoiser, network

    def __call__(self, x, sigma, cond):
        return self.denoiser(self.network, x, sigma, cond)


def _renoise_capability():
    """the backend's `frames_renoise` wrapper (pnc_frames_renoise), an optional capability looked up by name the way image.py looks up
    the image-boundary kernels; NotImplementedError when the backend has none (nothing has been launched then)"""
    from . import engine as E
    fn = getattr(E.backend(), "frames_renoise", None)
    if fn is None:
        raise NotImplementedError("this backend has no `frames_renoise`: a clip source needs pnc_frames_renoise of "
                                  "include/panacea_hip.h")
    return fn


def _masked_capability():
    """the backend's `latent_renoise_masked` wrapper (pnc_latent_renoise_masked), looked up by name like `frames_renoise` and only
    for a source that carries a mask"""
    from . import engine as E
    fn = getattr(E.backend(), "latent_renoise_masked", None)
    if fn is None:
        raise NotImplementedError("this backend has no `latent_renoise_masked`: a clip source with a mask needs "
                                  "pnc_latent_renoise_masked of include/panacea_hip.h")
    return fn


class ClipSource:
    """A recorded clip to start a schedule from (clip editing): `z` (T, C, h, w) fp32, the clip's latents already multiplied by
    scale_factor; `noise`, ONE fixed draw of that shape; `keep`, the frame slots (0 .. T-1, each once, possibly none) that come out
    as they went in.  The schedule starts at z + sigmas[start_step] * noise, and after every step the kept frames are rewritten as
    z + sigma_next * noise: with a fixed noise that is where a deterministic Euler step itself lands when the denoised frame is z
    (x + (sigma_next - sigma) * (x - z) / sigma at x = z + sigma * noise), so the other frames are denoised next to frames that sit
    at their own noise level, and the kept frames are z exactly once sigma_next is 0.  Both are one pnc_frames_renoise launch.

    `mask` (region editing): a (T, h, w) tensor on z's device that keeps latent PIXELS — bool, uint8 (nonzero keeps) or fp32 (> 0
    keeps; 0.0, -0.0, negatives and NaN do not).  The fact above holds element by element, so it holds for any subset of elements:
    what is kept is the union of the mask with the whole frames in `keep`, held as `selector`, contiguous fp32 0 / 1 made once
    here, and the put-back is one pnc_latent_renoise_masked launch in place instead of the pnc_frames_renoise one.  A source with a
    mask counts as keeping something even where the mask is empty (the selector lives on the device)."""

    def __init__(self, z: torch.Tensor, noise: torch.Tensor, keep=(), mask: Optional[torch.Tensor] = None):
        for name, t in (("z", z), ("noise", noise)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
                raise TypeError(f"ClipSource: {name} is an fp32 tensor, got "
                                f"{t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
        if z.dim() != 4 or 0 in z.shape:
            raise ValueError(f"ClipSource: z is (T, C, h, w), got {tuple(z.shape)}")
        if noise.shape != z.shape or noise.device != z.device:
            raise ValueError(f"ClipSource: noise is one draw of z's shape {tuple(z.shape)} on its device, got {tuple(noise.shape)} "
                             f"on {noise.device}")
        try:
            keep = tuple(operator.index(s) for s in keep)
        except TypeError:
            raise TypeError(f"ClipSource: keep holds frame slots (integers), got {keep!r}") from None
        T = z.shape[0]
        if any(not 0 <= s < T for s in keep):
            raise ValueError(f"ClipSource: keep slots {keep} outside 0 .. {T - 1}")
        if len(set(keep)) != len(keep):
            raise ValueError(f"ClipSource: keep slots {keep} name a frame twice")
        if mask is not None:
            if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.bool, torch.uint8, torch.float32):
                raise TypeError(f"ClipSource: mask is a bool, uint8 or fp32 tensor, got "
                                f"{mask.dtype if isinstance(mask, torch.Tensor) else type(mask).__name__}")
            if mask.shape != (T,) + tuple(z.shape[2:]) or mask.device != z.device:
                raise ValueError(f"ClipSource: mask is {(T,) + tuple(z.shape[2:])} on z's device {z.device}, got {tuple(mask.shape)} "
                                 f"on {mask.device}")
        self.z, self.noise, self.keep = z.detach().contiguous(), noise.detach().contiguous(), tuple(sorted(keep))
        self._keep_vec = None
        self.selector = None
        if mask is not None:
            kept = mask.detach() if mask.dtype == torch.bool else mask.detach() > 0
            if self.keep:
                kept = kept.clone()
                kept[list(self.keep)] = True
            self.selector = kept.to(torch.float32).contiguous()

    @property
    def keeps(self) -> bool:
        """whether the put-back after a step launches anything: kept frames, or a mask"""
        return bool(self.keep) or self.selector is not None

    def keep_vector(self) -> torch.Tensor:
        """[T] fp32 on z's device: 1 for a kept frame, 0 elsewhere (made once)"""
        if self._keep_vec is None:
            self._keep_vec = torch.tensor([1.0 if t in self.keep else 0.0 for t in range(self.z.shape[0])], dtype=torch.float32,
                                          device=self.z.device)
        return self._keep_vec

    def renoise(self, sigma: torch.Tensor) -> torch.Tensor:
        """z + sigma * noise of every frame, a new latent; `sigma`: [T] fp32 on the device"""
        out = torch.empty_like(self.z)
        _renoise_capability()(self.z, self.noise, sigma.contiguous(), out)
        return out

    def put_back(self, x: torch.Tensor, sigma: torch.Tensor) -> torch.Tensor:
        """the kept frames of `x` rewritten IN PLACE as z + sigma * noise (the others are not touched; no launch when nothing is
        kept); with a mask, the kept elements, in one pnc_latent_renoise_masked launch; returns `x`"""
        if self.selector is not None:
            _masked_capability()(self.z, self.noise, sigma.contiguous(), self.selector, x, x)
        elif self.keep:
            _renoise_capability()(self.z, self.noise, sigma.contiguous(), x, keep=self.keep_vector(), x=x)
        return x


class _Edit:
    """A ClipSource bound to one schedule: the [T] sigma vector of every schedule index as rows of ONE device tensor made up front
    (frame-wise copies of the schedule's own fp32 sigmas), so the loop launches without a host sync."""

    def __init__(self, source: ClipSource, sig: torch.Tensor, start_step: int):
        self.source, self.start_step = source, start_step
        self.rows = sig.to(torch.float32)[:, None].expand(-1, source.z.shape[0]).contiguous()

    def start(self) -> torch.Tensor:
        return self.source.renoise(self.rows[self.start_step])

    def after(self, callback):
        """`callback` behind the put-back of the step's output (the loops hand every step's latent to their callback)"""
        if not self.source.keeps:
            return callback

        def hook(i, x):
            self.source.put_back(x, self.rows[i + 1])
            if callback is not None:
                callback(i, x)
        return hook


class _Sampler:
    """What every sampler mirror shares: BaseDiffusionSampler (sampling.py:24-76) and the device half of a fused step — the
    network's eps tokens of the CFG batch for one sigma, handed to an exit kernel."""
    fuse = True          # use the fused device step when the denoiser is a BoundDenoiser around the HIP network
    keeps_frames = False  # ClipSource.keep: served where ONE network evaluation per step feeds the next and no noise is drawn

    def __init__(self, num_steps: int, guider: Optional[VanillaCFG] = None, discretization=None, device="cuda"):
        self.num_steps = num_steps
        self.discretization = discretization or LegacyDDPMDiscretization()
        self.guider = guider
        self.device = device

    def _keep_refusal(self) -> Optional[str]:
        """why this sampler as configured does not serve kept frames, or None"""
        if hasattr(self.guider, "half"):
            return "under parallel.ShardedCFG (one CFG half per rank)"
        return None if self.keeps_frames else "(it evaluates the network twice per step or draws fresh noise)"

    def _begin(self, sig: torch.Tensor, x, start_step: int, source: Optional[ClipSource], callback):
        """The start of a schedule, checked before anything is launched -> (start_step, the hook that stands in for `callback`,
        a function that makes the start latent).  Without a source the start latent is `x`, scaled by sqrt(1 + sigmas[0]^2) when the
        schedule starts at its first sigma; with one it is z + sigmas[start_step] * noise and `x` is ignored."""
        start_step = operator.index(start_step)
        n = len(sig) - 1
        if not 0 <= start_step < n:
            raise ValueError(f"start_step {start_step} outside 0 .. {n - 1} (a schedule of {n} steps)")
        if source is None:
            return start_step, callback, (lambda: x * torch.sqrt(1.0 + sig[0] ** 2.0) if start_step == 0 else x)
        if not isinstance(source, ClipSource):
            raise TypeError(f"source: a sampling.ClipSource, got {type(source).__name__}")
        why = self._keep_refusal() if source.keeps else None
        if why is not None:
            raise NotImplementedError(f"{type(self).__name__} does not keep frames {why}: kept frames are served by EulerEDMSampler "
                                      "without churn, DPMPP2MSampler and LinearMultistepSampler under VanillaCFG or no guider")
        _renoise_capability()
        if source.selector is not None:
            _masked_capability()
        edit = _Edit(source, sig, start_step)
        return start_step, edit.after(callback), edit.start

    def sigmas(self, num_steps=None) -> torch.Tensor:
        return self.discretization(self.num_steps if num_steps is None else num_steps, device=self.device)

    def host_sigmas(self, num_steps=None) -> List[float]:
        """the same fp32 schedule as Python floats (computed on the host: the branches the reference takes on device values are
        decided from these, without a sync)"""
        return self.discretization(self.num_steps if num_steps is None else num_steps, device="cpu").tolist()

    def _check_cfg_half(self, denoiser):
        """parallel.ShardedCFG evaluates one CFG half per rank: each rank would escalate on its own half's count, so the pair could end
        up on two policies.  The sharded guider refuses 'precise-wide' and 'escalate' wherever it meets the network, and any
        denoiser but EpsScaling with a quantised c_noise."""
        if getattr(self.guider, "half", None) is None:
            return
        from .parallel import _refuse_denoiser, _refuse_wide
        _refuse_denoiser(getattr(denoiser, "denoiser", None))
        net = getattr(denoiser, "network", None)
        if net is not None:
            _refuse_wide(getattr(net, "diffusion_model", net))

    def denoise(self, x, denoiser, sigma, cond, uc):
        self._check_cfg_half(denoiser)
        if self.guider is None:
            return denoiser(x, sigma, cond)
        return self.guider(denoiser(*self.guider.prepare_inputs(x, sigma, cond, uc)), sigma)

    def _fusable(self, denoiser, x, cond) -> bool:
        if not (self.fuse and isinstance(denoiser, BoundDenoiser) and x.is_cuda):
            return False
        return self._fusable_network(denoiser, cond)

    def _fusable_network(self, denoiser, cond) -> bool:
        model = getattr(denoiser.network, "diffusion_model", None)
        den = denoiser.denoiser
        # frame- / view-sharded networks fuse as well (round 4): the entry and exit kernels are elementwise over whatever frames /
        # band the rank holds; a CFG pair (parallel.ShardedCFG: `half`, `group`) all-gathers its eps halves in front of the
        # exit kernel instead of the denoised halves behind it
        guider_ok = type(self.guider) in (VanillaCFG, type(None)) or (isinstance(self.guider, VanillaCFG) and hasattr(self.guider, "half"))
        # any denoiser mirror with any scaling mirror, quantised or float c_noise: the exit kernels take c_skip as a [T] vector
        # (pnc_cfg_*_step_skip) and the network embeds a float timestep as given
        return (hasattr(model, "denoise_tokens") and guider_ok and isinstance(den, Denoiser)
                and type(den.scaling) in (EpsScaling, VScaling, EDMScaling)
                and "concat" in cond and cond.get("vector") is None)

    def _fused_eps(self, sigma, denoiser, x, cond, uc) -> "_Eps":
        """The network half of a fused step: a few tiny torch ops on T sigmas (the denoiser's own snap and scaling) + the network
        with c_in and the CFG batch doubling in its entry kernel.  Returns the channels-last fp32 eps tokens with what an exit
        kernel needs."""
        den, model = denoiser.denoiser, denoiser.network.diffusion_model
        T = x.shape[0]
        # denoiser.py:23-27 on the [T] vector: sigma snapped where the denoiser snaps, the scaling's four coefficients, c_noise the
        # table index (int64) or the float the scaling gives
        c_skip, c_out, c_in, c_noise = den.coefficients(sigma)
        c_skip = None if isinstance(den.scaling, EpsScaling) else c_skip.contiguous()     # eps: c_skip = 1, the kernels without it
        half = getattr(self.guider, "half", None)
        self._check_cfg_half(denoiser)
        if self.guider is None:
            cat, inv, nh = cond, cond.get("_invariants"), 1
        elif half is not None:
            # one CFG half per rank: this rank evaluates its half; the pair's eps tokens are gathered for the exit kernel
            cat, inv, nh = (uc if half == 0 else cond), cond.get("_invariants"), 1
        else:
            pre = cond.get("_cat")
            if pre is not None:
                cat = pre
            else:
                cat = {k: torch.cat((uc[k], cond[k]), 0) for k in ("crossattn", "concat")}
                # the BEV-layout hint: uc and c normally hold the SAME tensor (IdentityEncoder returns its input for both
                # conditioner passes, modules.py:242-247).  Then it is handed over once — no 2 x 0.5 GB concatenation per step
                # and the network runs its hint stem on T frames instead of 2 T
                hu, hc = uc["cond_feat"], cond["cond_feat"]
                cat["cond_feat"] = hc if _same_tensor(hu, hc) else torch.cat((hu, hc), 0)
            inv, nh = cond.get("_invariants"), 2
        ctx = cat["crossattn"].to(model.controlnet.input_hint_block[0].weight.dtype)
        eps = model.denoise_tokens(x, c_in.repeat(nh).contiguous(), c_noise.repeat(nh).contiguous(), ctx, cat["concat"],
                                   cat["cond_feat"], invariants=inv)
        x32 = x.detach().to(torch.float32).contiguous()
        eps32, cfg = eps.f32, nh == 2
        if half is not None:
            import torch.distributed as dist
            mine = eps32.contiguous()
            stage = dist.get_backend(self.guider.group) == "gloo" and mine.is_cuda       # two processes on one GPU (tests)
            send = mine.cpu() if stage else mine
            both = torch.empty((2 * send.shape[0], send.shape[1]), dtype=send.dtype, device=send.device)   # [uncond half; cond half]
            dist.all_gather_into_tensor(both, send, group=self.guider.group)
            eps32, cfg = both.to(mine.device), True
        return _Eps(eps32, eps.C, T, eps.N, x.shape[1], cfg, float(self.guider.scale) if cfg else 0.0, x32, c_out.contiguous(), c_skip)


class _Eps:
    """eps tokens of one network evaluation: tok [(cfg ? 2 : 1) * T * Npix][ld] fp32, x = the fp32 NCHW latent the network saw,
    c_out [T] = the scaling's c_out of the (snapped) sigma (EpsScaling: -sigma), c_skip [T] = its c_skip, or None for EpsScaling
    (c_skip = 1: the exit kernels without a skip vector)"""
    __slots__ = ("tok", "ld", "T", "Npix", "C", "cfg", "scale", "x", "c_out", "c_skip")

    def __init__(self, tok, ld, T, Npix, C, cfg, scale, x, c_out, c_skip=None):
        self.tok, self.ld, self.T, self.Npix, self.C, self.cfg, self.scale, self.x, self.c_out = tok, ld, T, Npix, C, cfg, scale, x, c_out
        self.c_skip = c_skip

    def skip_kw(self) -> Dict:
        """`c_skip=` for the backend's exit kernels, passed exactly when the scaling is not EpsScaling"""
        return {} if self.c_skip is None else {"c_skip": self.c_skip}

    def step(self, mode, v, out_aux=None, **kw) -> torch.Tensor:
        """pnc_cfg_sampler_step on these tokens; returns `out` (a new fp32 latent)"""
        from . import engine as E
        out = torch.empty_like(self.x)
        E.backend().cfg_sampler_step(mode, self.tok, self.ld, self.T, self.Npix, self.C, self.cfg, self.scale, self.x, self.c_out,
                                     [t.contiguous() for t in v], out, out_aux=out_aux, **kw, **self.skip_kw())
        return out

    def euler(self, sigma, next_sigma) -> torch.Tensor:
        """pnc_cfg_euler_step on these tokens (HEUN1's `out` with no d kept); returns the new fp32 latent"""
        from . import engine as E
        out = torch.empty_like(self.x)
        E.backend().cfg_euler_step(self.tok, self.ld, self.T, self.Npix, self.C, self.cfg, self.scale, self.x, self.c_out,
                                   sigma.contiguous(), next_sigma.contiguous(), out, **self.skip_kw())
        return out


def _churn_gamma(s_churn, s_tmin, s_tmax, sigma_i: float, num_sigmas: int) -> float:
    """EDMSampler.__call__ (sampling.py:118-122) on the host: the device comparison is fp32 against the fp32-rounded bounds"""
    lo, hi = float(np.float32(s_tmin)), float(np.float32(s_tmax))
    return min(s_churn / (num_sigmas - 1), 2 ** 0.5 - 1) if lo <= sigma_i <= hi else 0.0


class _EDM(_Sampler):
    """EDMSampler (sampling.py:85-133): optional churn noise before the network.  The churn stays three torch ops in the
    reference's order (x + eps * sqrt(sigma_hat^2 - sigma^2)) in front of the fused step; its noise comes from `noise_sampler`."""

    def __init__(self, num_steps: int, guider: Optional[VanillaCFG] = None, discretization=None, device="cuda",
                 s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0):
        super().__init__(num_steps, guider, discretization, device)
        self.s_churn, self.s_tmin, self.s_tmax, self.s_noise = s_churn, s_tmin, s_tmax, s_noise
        self.noise_sampler = lambda x: torch.randn_like(x)

    def _churn(self, sigma, x, gamma, noise=None):
        sigma_hat = sigma * (gamma + 1.0)
        if gamma > 0:
            eps = (self.noise_sampler(x) if noise is None else noise) * self.s_noise
            x = x + eps * append_dims(sigma_hat ** 2 - sigma ** 2, x.ndim) ** 0.5
        return sigma_hat, x


class EulerEDMSampler(_EDM):
    """sampling.py:27-133,214-218.  s_churn = 0 (default) is deterministic (== DDIM for eps-prediction)."""

    def _fused_step(self, sigma, next_sigma, denoiser, x, cond, uc):
        """One step with three tiny torch ops (table snap of T sigmas) + the network + one exit kernel; same arithmetic, in
        the reference's rounding order, as denoise() + the Euler update below."""
        return self._fused_eps(sigma, denoiser, x, cond, uc).euler(sigma, next_sigma).to(x.dtype)

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None, gamma=0.0):
        if gamma > 0:
            sigma, x = self._churn(sigma, x, gamma)                   # sigma_hat from here on
        if self._fusable(denoiser, x, cond):
            return self._fused_step(sigma, next_sigma, denoiser, x, cond, uc)
        denoised = self.denoise(x, denoiser, sigma, cond, uc)
        d = (x - denoised) / append_dims(sigma, x.ndim)
        return x + append_dims(next_sigma - sigma, x.ndim) * d

    keeps_frames = True

    def _keep_refusal(self):
        return "with churn (it draws fresh noise)" if self.s_churn > 0 else super()._keep_refusal()

    def __call__(self, denoiser, x, cond, uc=None, num_steps=None, network=None, callback=None, start_step: int = 0,
                 source: Optional[ClipSource] = None):
        """`network`: optional OpenAIWrapperControlLDM3D.  When given, the step invariants of the conditioning (text
        K/V of every cross-attention site, ControlNet hint stem) are computed once for the whole schedule instead of
        once per step; the trajectory is bit-identical to the plain loop.  `callback(i, x)` sees the
        latent after every step.
        `start_step`: the schedule index the loop begins at (`x` is then the latent at sigmas[start_step], taken as it is).
        `source`: a ClipSource — the loop starts from the clip at sigmas[start_step] (`x` is ignored and may be None) and puts the
        kept frames back after every step."""
        sig = self.sigmas(num_steps)
        start_step, callback, start = self._begin(sig, x, start_step, source, callback)
        uc = cond if uc is None else uc
        if network is not None:
            cond, uc = hoist_invariants(network, self.guider, cond, uc)
        x = start()
        s_in = x.new_ones([x.shape[0]])
        sig_f = self.host_sigmas(num_steps) if self.s_churn > 0 else None
        for i in range(start_step, len(sig) - 1):
            gamma = _churn_gamma(self.s_churn, self.s_tmin, self.s_tmax, sig_f[i], len(sig)) if sig_f else 0.0
            if gamma > 0:
                x = self.sampler_step(s_in * sig[i], s_in * sig[i + 1], denoiser, x, cond, uc, gamma)
            else:
                x = self.sampler_step(s_in * sig[i], s_in * sig[i + 1], denoiser, x, cond, uc)
            if callback is not None:
                callback(i, x)
        return x

    # the step forms of a schedule (graph.GraphedSchedule): one per churn gamma
    def _steps(self, sig, sig_f, s_in):
        for i in range(len(sig_f) - 1):
            gamma = _churn_gamma(self.s_churn, self.s_tmin, self.s_tmax, sig_f[i], len(sig_f))
            yield gamma, {"sigma": s_in * sig[i], "next_sigma": s_in * sig[i + 1]}, gamma > 0

    def _state(self, x):
        return {}

    def _device_step(self, form, sv, x, denoiser, cond, uc, state):
        sigma, x = self._churn(sv["sigma"], x, form, sv.get("noise"))
        return self._fused_step(sigma, sv["next_sigma"], denoiser, x, cond, uc)


# ------------------------------------------------------------------------------------------------------------------------------
# the other samplers of sampling.py.  Each has the reference's `sampler_step` (torch ops in the reference's order, used whenever the
# step does not fuse) and a device step: the network's eps tokens + ONE pnc_cfg_sampler_step per network evaluation, with every
# per-frame scalar (sigma_hat, sigma_down / sigma_up, the exp / expm1 multipliers, the LMS coefficients) a [T] device vector made by
# the same torch ops as the plain step, so a fused step gives the plain step's bits.  Branches the reference takes on device sums
# (`torch.sum(next_sigma) < 1e-14`, the first step) are decided from the host copy of the schedule.
# ------------------------------------------------------------------------------------------------------------------------------
def to_d(x, sigma, denoised):
    return (x - denoised) / append_dims(sigma, x.ndim)


def to_neg_log_sigma(sigma):
    return sigma.log().neg()


def to_sigma(neg_log_sigma):
    return neg_log_sigma.neg().exp()


def get_ancestral_step(sigma_from, sigma_to, eta=1.0):
    """sampling_utils.py: (sigma_down, sigma_up); sigma_up is the float 0.0 when eta is 0"""
    if not eta:
        return sigma_to, 0.0
    sigma_up = torch.minimum(sigma_to, eta * (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5)
    sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
    return sigma_down, sigma_up


def _vec(v, like):
    """a per-frame scalar as a [T] fp32 vector (sigma_up is a Python 0.0 when eta = 0)"""
    return v if torch.is_tensor(v) else torch.full_like(like, float(v))


def _all_zero(v: List[float]) -> bool:
    """`torch.sum(v) < 1e-14` of a [T] vector whose frames hold the same value"""
    return len(v) * v[0] < 1e-14 if v else True


class _Scheduled(_Sampler):
    """The schedule loop of the samplers below: the reference's own loop on plain steps, or the device loop over
    `_steps()` / `_device_step()` (the forms graph.GraphedSchedule captures)."""

    def _check_guider(self):
        if hasattr(self.guider, "half"):
            raise NotImplementedError(f"{type(self).__name__} does not run under parallel.ShardedCFG (one CFG half per rank); "
                                      "use VanillaCFG, or EulerEDMSampler for CFG-half sharding")

    def __call__(self, denoiser, x, cond, uc=None, num_steps=None, network=None, callback=None, start_step: int = 0,
                 source: Optional[ClipSource] = None):
        """`network`: hoist the step invariants once per schedule (they serve every evaluation of a step); `callback(i, x)`
        sees the latent after every step.  `start_step`, `source`: as EulerEDMSampler.__call__ takes them; a sampler that carries
        a history (DPM++ 2M, LMS) starts at `start_step` with an empty one, as it does at step 0."""
        self._check_guider()
        sig, sig_f = self.sigmas(num_steps), self.host_sigmas(num_steps)
        start_step, callback, start = self._begin(sig, x, start_step, source, callback)
        uc = cond if uc is None else uc
        if network is not None:
            cond, uc = hoist_invariants(network, self.guider, cond, uc)
        x = start()
        s_in = x.new_ones([x.shape[0]])
        loop = self._fused_loop if self._fusable(denoiser, x, cond) else self._plain_loop
        return loop(sig, sig_f, s_in, denoiser, x, cond, uc, callback, start_step)

    def _fused_loop(self, sig, sig_f, s_in, denoiser, x, cond, uc, callback=None, start=0):
        state = self._state(x)
        for i, (form, sv, draw) in enumerate(self._steps(sig, sig_f, s_in, start), start):
            if draw:
                sv["noise"] = self.noise_sampler(x).to(torch.float32).contiguous()
            x = self._device_step(form, sv, x, denoiser, cond, uc, state).to(x.dtype)
            if callback is not None:
                callback(i, x)
        return x

    def _state(self, x):
        return {}


class HeunEDMSampler(_EDM, _Scheduled):
    """sampling.py:85-133,221-237: Euler to next_sigma, then (unless every next_sigma is 0) a second evaluation there and the
    trapezoidal correction."""

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None, gamma=0.0, last=None):
        sigma_hat, x = self._churn(sigma, x, gamma)
        denoised = self.denoise(x, denoiser, sigma_hat, cond, uc)
        d = to_d(x, sigma_hat, denoised)
        dt = append_dims(next_sigma - sigma_hat, x.ndim)
        euler_step = x + dt * d
        if last is None:
            last = bool(torch.sum(next_sigma) < 1e-14)
        if last:
            return euler_step
        denoised = self.denoise(euler_step, denoiser, next_sigma, cond, uc)
        d_new = to_d(euler_step, next_sigma, denoised)
        d_prime = (d + d_new) / 2.0
        return torch.where(append_dims(next_sigma, x.ndim) > 0.0, x + d_prime * dt, euler_step)

    def _plain_loop(self, sig, sig_f, s_in, denoiser, x, cond, uc, callback=None, start=0):
        for i, ((gamma, last), _, _) in enumerate(self._steps(sig, sig_f, s_in, start), start):
            x = self.sampler_step(s_in * sig[i], s_in * sig[i + 1], denoiser, x, cond, uc, gamma, last=last)
            if callback is not None:
                callback(i, x)
        return x

    def _steps(self, sig, sig_f, s_in, start=0):
        T = s_in.shape[0]
        for i in range(start, len(sig_f) - 1):
            gamma = _churn_gamma(self.s_churn, self.s_tmin, self.s_tmax, sig_f[i], len(sig_f))
            yield (gamma, _all_zero([sig_f[i + 1]] * T)), {"sigma": s_in * sig[i], "next_sigma": s_in * sig[i + 1]}, gamma > 0

    def _device_step(self, form, sv, x, denoiser, cond, uc, state):
        from . import hip
        gamma, last = form
        nxt = sv["next_sigma"]
        sigma_hat, x = self._churn(sv["sigma"], x, gamma, sv.get("noise"))
        e = self._fused_eps(sigma_hat, denoiser, x, cond, uc)
        d = torch.empty_like(e.x)
        x_euler = e.step(hip.SAMPLER_HEUN1, [sigma_hat, nxt], out_aux=d)
        if last:
            return x_euler
        e2 = self._fused_eps(nxt, denoiser, x_euler, cond, uc)
        return e2.step(hip.SAMPLER_HEUN2, [sigma_hat, nxt], x0=e.x, aux=d)


class _Ancestral(_Scheduled):
    """AncestralSampler (sampling.py:135-172)"""

    def __init__(self, num_steps: int, guider: Optional[VanillaCFG] = None, discretization=None, device="cuda",
                 eta=1.0, s_noise=1.0):
        super().__init__(num_steps, guider, discretization, device)
        self.eta, self.s_noise = eta, s_noise
        self.noise_sampler = lambda x: torch.randn_like(x)

    def ancestral_euler_step(self, x, denoised, sigma, sigma_down):
        d = to_d(x, sigma, denoised)
        dt = append_dims(sigma_down - sigma, x.ndim)
        return x + dt * d

    def ancestral_step(self, x, sigma, next_sigma, sigma_up):
        return torch.where(append_dims(next_sigma, x.ndim) > 0.0,
                           x + self.noise_sampler(x) * self.s_noise * append_dims(sigma_up, x.ndim), x)

    def _plain_loop(self, sig, sig_f, s_in, denoiser, x, cond, uc, callback=None, start=0):
        for i in range(start, len(sig_f) - 1):
            x = self.sampler_step(s_in * sig[i], s_in * sig[i + 1], denoiser, x, cond, uc)
            if callback is not None:
                callback(i, x)
        return x

    def _noise_v(self, sigma, nxt):
        sd, su = get_ancestral_step(sigma, nxt, eta=self.eta)
        return sd, _vec(su, sigma)


class EulerAncestralSampler(_Ancestral):
    """sampling.py:240-247"""

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None):
        sigma_down, sigma_up = get_ancestral_step(sigma, next_sigma, eta=self.eta)
        denoised = self.denoise(x, denoiser, sigma, cond, uc)
        x = self.ancestral_euler_step(x, denoised, sigma, sigma_down)
        return self.ancestral_step(x, sigma, next_sigma, sigma_up)

    def _steps(self, sig, sig_f, s_in, start=0):
        for i in range(start, len(sig_f) - 1):
            yield None, {"sigma": s_in * sig[i], "next_sigma": s_in * sig[i + 1]}, True

    def _device_step(self, form, sv, x, denoiser, cond, uc, state):
        from . import hip
        sigma, nxt = sv["sigma"], sv["next_sigma"]
        sd, su = self._noise_v(sigma, nxt)
        e = self._fused_eps(sigma, denoiser, x, cond, uc)
        return e.step(hip.SAMPLER_EULER_A, [sigma, sd, su, nxt], noise=sv["noise"], s_noise=self.s_noise)


class DPMPP2SAncestralSampler(_Ancestral):
    """sampling.py:250-287: DPM-Solver++(2S) with ancestral noise; the midpoint evaluation is skipped where sigma_down is 0."""

    def get_variables(self, sigma, sigma_down):
        t, t_next = [to_neg_log_sigma(s) for s in (sigma, sigma_down)]
        h = t_next - t
        s = t + 0.5 * h
        return h, s, t, t_next

    def get_mult(self, h, s, t, t_next):
        return to_sigma(s) / to_sigma(t), (-0.5 * h).expm1(), to_sigma(t_next) / to_sigma(t), (-h).expm1()

    def sampler_step(self, sigma, next_sigma, denoiser, x, cond, uc=None, last=None):
        sigma_down, sigma_up = get_ancestral_step(sigma, next_sigma, eta=self.eta)
        denoised = self.denoise(x, denoiser, sigma, cond, uc)
        x_euler = self.ancestral_euler_step(x, denoised, sigma, sigma_down)
        if last is None:
            last = bool(torch.sum(sigma_down) < 1e-14)
        if last:
            x = x_euler
        else:
            h, s, t, t_next = self.get_variables(sigma, sigma_down)
            mult = [append_dims(m, x.ndim) for m in self.get_mult(h, s, t, t_next)]
            x2 = mult[0] * x - mult[1] * denoised
            denoised2 = self.denoise(x2, denoiser, to_sigma(s), cond, uc)
            x_dpmpp2s = mult[2] * x - mult[3] * denoised2
            x = torch.where(append_dims(sigma_down, x.ndim) > 0.0, x_dpmpp2s, x_euler)
        return self.ancestral_step(x, sigma, next_sigma, sigma_up)

    def _plain_loop(self, sig, sig_f, s_in, denoiser, x, cond, uc, callback=None, start=0):
        for i, (last, _, _) in enumerate(self._steps(sig, sig_f, s_in, start), start):
            x = self.sampler_step(s_in * sig[i], s_in * sig[i + 1], denoiser, x, cond, uc, last=last)
            if callback is not None:
                callback(i, x)
        return x

    def _steps(self, sig, sig_f, s_in, start=0):
        T = s_in.shape[0]
        for i in range(start, len(sig_f) - 1):
            # sigma_down of the fp32 schedule, on the host (the reference sums it on the device)
            sd, _ = get_ancestral_step(torch.tensor([sig_f[i]]), torch.tensor([sig_f[i + 1]]), eta=self.eta)
            yield _all_zero([float(sd[0])] * T), {"sigma": s_in * sig[i], "next_sigma": s_in * sig[i + 1]}, True

    def _device_step(self, form, sv, x, denoiser, cond, uc, state):
        from . import hip
        sigma, nxt = sv["sigma"], sv["next_sigma"]
        sd, su = self._noise_v(sigma, nxt)
        e = self._fused_eps(sigma, denoiser, x, cond, uc)
        if form:                                                      # every sigma_down is 0: the ancestral Euler step
            return e.step(hip.SAMPLER_EULER_A, [sigma, sd, su, nxt], noise=sv["noise"], s_noise=self.s_noise)
        h, s, t, t_next = self.get_variables(sigma, sd)
        m1, m2, m3, m4 = self.get_mult(h, s, t, t_next)
        x_euler = torch.empty_like(e.x)
        x2 = e.step(hip.SAMPLER_DPM2S_1, [sigma, sd, m1, m2], out_aux=x_euler)
        e2 = self._fused_eps(to_sigma(s), denoiser, x2, cond, uc)
        return e2.step(hip.SAMPLER_DPM2S_2, [m3, m4, sd, su, nxt], x0=e.x, aux=x_euler, noise=sv["noise"], s_noise=self.s_noise)


class DPMPP2MSampler(_Scheduled):
    """sampling.py:290-365: DPM-Solver++(2M); carries the previous step's denoised (a device plane)."""
    keeps_frames = True

    def get_variables(self, sigma, next_sigma, previous_sigma=None):
        t, t_next = [to_neg_log_sigma(s) for s in (sigma, next_sigma)]
        h = t_next - t
        if previous_sigma is not None:
            h_last = t - to_neg_log_sigma(previous_sigma)
            return h, h_last / h, t, t_next
        return h, None, t, t_next

    def get_mult(self, h, r, t, t_next, previous_sigma):
        mult1 = to_sigma(t_next) / to_sigma(t)
        mult2 = (-h).expm1()
        if previous_sigma is not None:
            return mult1, mult2, 1 + 1 / (2 * r), 1 / (2 * r)
        return mult1, mult2

    def sampler_step(self, old_denoised, previous_sigma, sigma, next_sigma, denoiser, x, cond, uc=None, last=None):
        denoised = self.denoise(x, denoiser, sigma, cond, uc)
        h, r, t, t_next = self.get_variables(sigma, next_sigma, previous_sigma)
        mult = [append_dims(m, x.ndim) for m in self.get_mult(h, r, t, t_next, previous_sigma)]
        x_standard = mult[0] * x - mult[1] * denoised
        if last is None:
            last = bool(torch.sum(next_sigma) < 1e-14)
        if old_denoised is None or last:
            return x_standard, denoised
        denoised_d = mult[2] * denoised - mult[3] * old_denoised
        x_advanced = mult[0] * x - mult[1] * denoised_d
        return torch.where(append_dims(next_sigma, x.ndim) > 0.0, x_advanced, x_standard), denoised

    def _plain_loop(self, sig, sig_f, s_in, denoiser, x, cond, uc, callback=None, start=0):
        old = None
        T = s_in.shape[0]
        for i in range(start, len(sig_f) - 1):
            x, old = self.sampler_step(old, None if i == start else s_in * sig[i - 1], s_in * sig[i], s_in * sig[i + 1], denoiser, x,
                                       cond, uc, last=_all_zero([sig_f[i + 1]] * T))
            if callback is not None:
                callback(i, x)
        return x

    def _steps(self, sig, sig_f, s_in, start=0):
        T = s_in.shape[0]
        for i in range(start, len(sig_f) - 1):
            sv = {"sigma": s_in * sig[i], "next_sigma": s_in * sig[i + 1]}
            if i > start:
                sv["previous_sigma"] = s_in * sig[i - 1]
            # forms: "first" (no previous denoised: the step the loop begins at), "last" (every next_sigma 0), "middle"
            yield ("first" if i == start else "last" if _all_zero([sig_f[i + 1]] * T) else "middle"), sv, False

    def _state(self, x):
        return {"old": torch.empty(x.shape, dtype=torch.float32, device=x.device)}

    def _device_step(self, form, sv, x, denoiser, cond, uc, state):
        from . import hip
        sigma, nxt, prev = sv["sigma"], sv["next_sigma"], sv.get("previous_sigma")
        e = self._fused_eps(sigma, denoiser, x, cond, uc)
        h, r, t, t_next = self.get_variables(sigma, nxt, prev)
        mult = self.get_mult(h, r, t, t_next, prev)
        old = state["old"]
        if form == "middle":
            # the kernel reads the previous denoised of an element before it writes this step's there
            return e.step(hip.SAMPLER_DPM2M, [*mult, nxt], out_aux=old, aux=old)
        return e.step(hip.SAMPLER_DPM2M, list(mult[:2]), out_aux=old)


def linear_multistep_coeff(order: int, t, i: int, j: int, epsrel=1e-4) -> float:
    """sampling_utils.py:12-24 in float64: the integral over [t_i, t_(i+1)] of the j-th Lagrange basis polynomial through
    t_i, t_(i-1), ...  scipy's `quad` when scipy is present, else Gauss-Legendre with 4 nodes (exact: degree <= 3)."""
    if order - 1 > i:
        raise ValueError(f"Order {order} too high for step {i}")
    t = [float(v) for v in t]

    def fn(tau):
        prod = 1.0
        for k in range(order):
            if j != k:
                prod *= (tau - t[i - k]) / (t[i - j] - t[i - k])
        return prod
    try:
        from scipy import integrate
    except ImportError:
        a, b = t[i], t[i + 1]
        nodes, weights = np.polynomial.legendre.leggauss(4)
        return float(sum(w * fn(0.5 * (b - a) * u + 0.5 * (a + b)) for u, w in zip(nodes, weights)) * 0.5 * (b - a))
    return integrate.quad(fn, t[i], t[i + 1], epsrel=epsrel)[0]


class LinearMultistepSampler(_Scheduled):
    """sampling.py:176-211: linear multistep of `order` on the last `order` d = (x - denoised) / sigma.  The coefficients are
    computed once per schedule (float64) and enter the update as fp32 scalars, the way torch rounds a Python float."""
    MAX_FUSED_ORDER = 4          # pnc_cfg_sampler_step keeps up to 3 previous d
    keeps_frames = True

    def __init__(self, num_steps: int, guider: Optional[VanillaCFG] = None, discretization=None, device="cuda", order=4):
        super().__init__(num_steps, guider, discretization, device)
        self.order = order

    def coefficients(self, sig_f: List[float], start: int = 0) -> List[List[float]]:
        """the coefficients of steps start, start + 1, ...: the order grows from 1 at the step the loop begins at"""
        out = []
        for i in range(start, len(sig_f) - 1):
            cur = min(i - start + 1, self.order)
            out.append([linear_multistep_coeff(cur, sig_f, i, j) for j in range(cur)])
        return out

    def sampler_step(self, sigma, denoiser, x, cond, uc, ds: list, coeffs: List[float]):
        """one step of the reference's loop: appends this step's d to `ds` (kept at `order` entries)"""
        denoised = self.denoise(x, denoiser, sigma, cond, uc)
        d = to_d(x, sigma, denoised)
        ds.append(d)
        if len(ds) > self.order:
            ds.pop(0)
        return x + sum(coeff * d for coeff, d in zip(coeffs, reversed(ds)))

    def _plain_loop(self, sig, sig_f, s_in, denoiser, x, cond, uc, callback=None, start=0):
        ds = []
        for i, cs in enumerate(self.coefficients(sig_f, start), start):
            x = self.sampler_step(s_in * sig[i], denoiser, x, cond, uc, ds, cs)
            if callback is not None:
                callback(i, x)
        return x

    def _steps(self, sig, sig_f, s_in, start=0):
        if self.order > self.MAX_FUSED_ORDER:
            raise NotImplementedError(f"the fused LMS step keeps at most {self.MAX_FUSED_ORDER - 1} previous d (order {self.order})")
        co = self.coefficients(sig_f, start)
        table = torch.tensor([c + [0.0] * (self.order - len(c)) for c in co], dtype=torch.float32)      # fp32 rounding of each
        table = table[:, :, None].expand(-1, -1, s_in.shape[0]).contiguous().to(s_in.device)
        for k, cs in enumerate(co):
            yield len(cs) - 1, {"sigma": s_in * sig[start + k], "coeffs": table[k, :len(cs)]}, False

    def _state(self, x):
        return {"hist": [torch.empty(x.shape, dtype=torch.float32, device=x.device) for _ in range(self.order - 1)]}

    def _device_step(self, form, sv, x, denoiser, cond, uc, state):
        from . import hip
        e = self._fused_eps(sv["sigma"], denoiser, x, cond, uc)
        hist = state["hist"]
        d = torch.empty_like(e.x)
        out = e.step(hip.SAMPLER_LMS, [sv["sigma"], *sv["coeffs"].unbind(0)], out_aux=d, hist=hist[:form])
        for k in range(len(hist) - 1, 0, -1):                         # newest first: shift the history, d enters in front
            hist[k].copy_(hist[k - 1])
        if hist:
            hist[0].copy_(d)
        return out


SAMPLERS = {"EulerEDMSampler": EulerEDMSampler, "HeunEDMSampler": HeunEDMSampler, "EulerAncestralSampler": EulerAncestralSampler,
            "DPMPP2SAncestralSampler": DPMPP2SAncestralSampler, "DPMPP2MSampler": DPMPP2MSampler,
            "LinearMultistepSampler": LinearMultistepSampler}
_REF_SAMPLING = "sgm.modules.diffusionmodules.sampling."


DISCRETIZATIONS = {"LegacyDDPMDiscretization": LegacyDDPMDiscretization, "EDMDiscretization": EDMDiscretization}
SCALINGS = {"EpsScaling": EpsScaling, "VScaling": VScaling, "EDMScaling": EDMScaling}
_REF = "sgm.modules.diffusionmodules."


def _mirror_of(cfg: Optional[Dict], module: str, table: Dict, default: str, what: str):
    """the mirror class a reference `{target, params}` block names, with its params"""
    cfg = cfg or {"target": _REF + module + "." + default}
    target = str(cfg.get("target", ""))
    prefix = _REF + module + "."
    name = target[len(prefix):] if target.startswith(prefix) else None
    if name not in table:
        raise NotImplementedError(f"{what} {target!r} has no mirror in panacea_amd.sampling "
                                  f"(supported: {', '.join(prefix + n for n in table)})")
    return table[name], dict(cfg.get("params") or {})


def _discretization_from_config(disc_cfg: Optional[Dict]):
    cls, kw = _mirror_of(disc_cfg, "discretizer", DISCRETIZATIONS, "LegacyDDPMDiscretization", "discretization")
    return cls(**kw)


def denoiser_from_config(denoiser_config: Optional[Dict]) -> Denoiser:
    """The mirror of the reference's YAML `denoiser_config` (configs/inference_nuscenes.yaml:12-22): `target` Denoiser or
    DiscreteDenoiser of sgm.modules.diffusionmodules.denoiser, `params` with scaling_config (EpsScaling / VScaling / EDMScaling)
    and, for the discrete one, num_idx, discretization_config, do_append_zero, quantize_c_noise, flip.  `weighting_config` is the
    training loss weight: accepted and ignored.  None = the shipped YAML's DiscreteDenoiser()."""
    if denoiser_config is None:
        return DiscreteDenoiser()
    cls, params = _mirror_of(denoiser_config, "denoiser", {"Denoiser": Denoiser, "DiscreteDenoiser": DiscreteDenoiser},
                             "DiscreteDenoiser", "denoiser")
    params.pop("weighting_config", None)
    s_cls, s_kw = _mirror_of(params.pop("scaling_config", None), "denoiser_scaling", SCALINGS, "EpsScaling", "scaling")
    scaling = s_cls(**s_kw)
    if cls is Denoiser:
        if params:
            raise TypeError(f"Denoiser takes weighting_config and scaling_config only (got {sorted(params)})")
        return Denoiser(scaling)
    disc = _discretization_from_config(params.pop("discretization_config", None))
    return DiscreteDenoiser(discretization=disc, scaling=scaling, **params)


def from_config(sampler_config: Dict, device="cuda") -> _Sampler:
    """The mirror of the reference's YAML `sampler_config` (configs/inference_nuscenes.yaml:115-126): `target` one of the six
    samplers of sgm.modules.diffusionmodules.sampling, `params` with num_steps, discretization_config (LegacyDDPMDiscretization
    or EDMDiscretization),
    guider_config (VanillaCFG or IdentityGuider) and the sampler's own kwargs (s_churn, eta, s_noise, order, ...)."""
    target = sampler_config.get("target", "")
    name = target[len(_REF_SAMPLING):] if target.startswith(_REF_SAMPLING) else None
    if name not in SAMPLERS:
        raise NotImplementedError(f"sampler target {target!r} has no mirror in panacea_amd.sampling "
                                  f"(supported: {', '.join(_REF_SAMPLING + n for n in SAMPLERS)})")
    params = dict(sampler_config.get("params") or {})
    params.pop("verbose", None)
    disc = _discretization_from_config(params.pop("discretization_config", None))
    g_cfg = params.pop("guider_config", None)
    g_target = str((g_cfg or {}).get("target", "IdentityGuider"))
    if g_target.endswith("VanillaCFG"):
        g_params = dict(g_cfg.get("params") or {})
        if g_params.get("dyn_thresh_config") is not None:
            raise NotImplementedError("dynamic thresholding is not mirrored")
        guider = VanillaCFG(g_params["scale"])
    elif g_target.endswith("IdentityGuider"):
        guider = None
    else:
        raise NotImplementedError(f"guider {g_target!r} has no mirror (VanillaCFG / IdentityGuider)")
    num_steps = params.pop("num_steps", None)
    return SAMPLERS[name](num_steps, guider=guider, discretization=disc, device=device, **params)


def share_noise_init(randn: torch.Tensor, concat: torch.Tensor, share_noise_level: float) -> torch.Tensor:
    """DiffusionEngine3D.sample (sgm/models/diffusion.py:242-249): the initial latent of every frame of a clip carries
    `share_noise_level` x the conditioning latent of the LAST frame (`concat[-1]` tiled over the frames)."""
    if share_noise_level <= 0.0:
        return randn
    return randn + concat[-1].unsqueeze(0).expand(randn.shape[0], *concat.shape[1:]) * share_noise_level


def hoist_invariants(network, guider, cond: Dict, uc: Dict):
    """Returns copies of (cond, uc) that carry the network's StepInvariants for the batch the guider will build from
    them.  The concatenated conditioning tensors are built ONCE here and shared by every step (prepare_inputs would
    otherwise re-concatenate them per step, which also changes their identity)."""
    model = network.diffusion_model
    half = getattr(guider, "half", None)
    if half is not None:
        # parallel.ShardedCFG: this rank evaluates ONE CFG half with that half's own tensors (same objects every step)
        from .parallel import _refuse_wide
        _refuse_wide(model)
        src = dict(uc if half == 0 else cond)
        src["crossattn"] = src["crossattn"].to(model.controlnet.input_hint_block[0].weight.dtype)
        inv = model.prepare(src["crossattn"], src["cond_feat"])
        c2, u2 = dict(cond), dict(uc)
        (u2 if half == 0 else c2).update(crossattn=src["crossattn"])
        c2["_invariants"] = u2["_invariants"] = inv
        return c2, u2
    if guider is None:
        c2 = dict(cond)
        c2["crossattn"] = cond["crossattn"].to(model.controlnet.input_hint_block[0].weight.dtype)
        c2["_invariants"] = model.prepare(c2["crossattn"], c2["cond_feat"])
        return c2, c2
    cat = {k: torch.cat((uc[k], cond[k]), 0) for k in cond if k in guider.KEYS}
    cat["crossattn"] = cat["crossattn"].to(model.controlnet.input_hint_block[0].weight.dtype)
    inv = model.prepare(cat["crossattn"], cat["cond_feat"])
    c2, u2 = dict(cond), dict(uc)
    c2["_invariants"] = u2["_invariants"] = inv
    c2["_cat"] = u2["_cat"] = cat
    return c2, u2


def timestep_indices(num_steps: int) -> List[int]:
    """The int64 timestep indices the network sees over a `num_steps` schedule (999, 959, ... for 25)."""
    den = DiscreteDenoiser()
    sig = LegacyDDPMDiscretization()(num_steps)[:-1]
    return den.sigma_to_idx(sig).tolist()
