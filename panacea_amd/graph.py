"""hipGraph replay of one denoising step.

Every kernel of the path is enqueued on the current torch stream with no allocation or synchronisation of
its own (include/panacea_hip.h), so a whole `EulerEDMSampler.sampler_step` — guidance batch doubling,
sigma -> timestep-index lookup, ControlNet + UNet (~1 800 launches), CFG combine, Euler update — captures into
ONE hipGraph.  Replaying it removes the per-launch host cost (Python + ctypes + hipLaunch, ~5-8 us each)
from the step, which is what `torch.compile` was for in the reference's IdentityWrapper (wrappers.py:10-22).

Step inputs that change between replays (latent, sigma, next sigma) live in static device buffers that are
overwritten before each replay; the conditioning tensors are captured by reference (update them in place).
"""
from __future__ import annotations

from typing import Callable

import torch


def refuse_unescalated(network):
    """A captured step replays kernels only: the range monitor of on_range_exceeded = "escalate" never runs inside it.  A network
    in that mode may be captured once it has escalated (its policy no longer changes), not before."""
    if network is None:
        return
    model = getattr(network, "diffusion_model", network)
    if getattr(model, "on_range_exceeded", None) == "escalate" and not model.escalated:
        raise ValueError("on_range_exceeded='escalate' is not monitored during graph replay: capture the network after it has "
                         "escalated, or use 'warn' / 'raise'")


class GraphedStep:
    def __init__(self, step_fn: Callable[[torch.Tensor, torch.Tensor, torch.Tensor], torch.Tensor],
                 x: torch.Tensor, sigma: torch.Tensor, next_sigma: torch.Tensor, warmup: int = 2, network=None):
        """`network`: the network `step_fn` evaluates (refused while in an un-escalated "escalate" mode)"""
        refuse_unescalated(network)
        self.x, self.sigma, self.next_sigma = x.clone(), sigma.clone(), next_sigma.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side), torch.no_grad():
            for _ in range(warmup):                      # packs weights, primes every lazily built table
                step_fn(self.x, self.sigma, self.next_sigma)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.out = step_fn(self.x, self.sigma, self.next_sigma)

    def __call__(self, x: torch.Tensor, sigma: torch.Tensor, next_sigma: torch.Tensor) -> torch.Tensor:
        self.x.copy_(x)
        self.sigma.copy_(sigma)
        self.next_sigma.copy_(next_sigma)
        self.graph.replay()
        return self.out


class GraphedSchedule:
    """hipGraph replay of a whole schedule of any sampler of panacea_amd.sampling (fused steps only).

    A schedule has a few distinct step FORMS — Heun's last step skips the second evaluation, DPM++ 2M's first and last steps
    skip the multistep correction, LMS grows its order over the first steps, churn applies on some sigmas only — and every
    step of one form launches the same kernels on the same buffers.  One graph is captured per form (all sharing one memory
    pool; they replay one after another on one stream).  Per-step inputs live in static device buffers that are overwritten
    before each replay: the latent, the sigma vectors, the LMS coefficients and the noise the sampler's `noise_sampler`
    draws for the step.  The state carried between steps (DPM++ 2M's previous denoised, LMS's previous d) is the sampler's
    own device planes, written by one replay and read by the next.  The conditioning is captured by reference.

        g = GraphedSchedule(sampler, BoundDenoiser(den, network), x_like, cond, uc, network=network)
        x = g(noise)                      # == sampler(BoundDenoiser(den, network), noise, cond, uc, network=network)
    """

    def __init__(self, sampler, denoiser, x_like: torch.Tensor, cond, uc=None, num_steps=None, network=None, warmup: int = 1):
        from . import sampling
        refuse_unescalated(network if network is not None else getattr(denoiser, "network", None))
        if hasattr(sampler, "_check_guider"):
            sampler._check_guider()
        if not sampler._fusable(denoiser, x_like, cond):
            raise ValueError("GraphedSchedule replays fused device steps: needs a BoundDenoiser around the HIP network and "
                             "device tensors")
        self.sampler, self.denoiser = sampler, denoiser
        uc = cond if uc is None else uc
        if network is not None:
            cond, uc = sampling.hoist_invariants(network, sampler.guider, cond, uc)
        self.cond, self.uc = cond, uc
        self.sig, sig_f = sampler.sigmas(num_steps), sampler.host_sigmas(num_steps)
        s_in = x_like.new_ones([x_like.shape[0]])
        self.plan = list(sampler._steps(self.sig, sig_f, s_in))         # (form, per-step device vectors, draws noise)
        self.state = sampler._state(x_like)
        self.static, self.graphs, self.out = {}, {}, {}
        pool = None
        for form, sv, draw in self.plan:
            if form in self.graphs:
                continue
            st = {k: v.clone() for k, v in sv.items()}
            if draw:
                st["noise"] = torch.zeros(x_like.shape, dtype=torch.float32, device=x_like.device)
            x = torch.zeros_like(x_like)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():
                for _ in range(warmup):                  # packs weights, primes every lazily built table
                    sampler._device_step(form, st, x, denoiser, cond, uc, self.state)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=pool), torch.no_grad():
                self.out[form] = sampler._device_step(form, st, x, denoiser, cond, uc, self.state)
            pool = g.pool() if pool is None else pool
            self.static[form], self.graphs[form] = (x, st), g

    def __call__(self, x: torch.Tensor, callback=None) -> torch.Tensor:
        """x: the unit-variance initial latent (scaled by sqrt(1 + sigma_0^2) here, as the sampler does)"""
        dtype = x.dtype
        x = x * torch.sqrt(1.0 + self.sig[0] ** 2.0)
        for i, (form, sv, draw) in enumerate(self.plan):
            xs, st = self.static[form]
            for k, v in sv.items():
                st[k].copy_(v)
            if draw:
                st["noise"].copy_(self.sampler.noise_sampler(x))
            xs.copy_(x)
            self.graphs[form].replay()
            x = self.out[form]
            if callback is not None:
                callback(i, x)
        return x.to(dtype, copy=True)
