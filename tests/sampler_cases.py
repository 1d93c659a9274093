"""What tests/test_samplers.py and tests/test_samplers_gpu.py share: the sampler cases of tests/golden/samplers*.npz
(tools/gen_golden_samplers.py), noise injection, and a stand-in network with the product's `denoise_tokens` interface around the
closed-form `fake_network`, so that the fused device loop (pnc_cfg_sampler_step) can replay the fake-network trajectories."""
from types import SimpleNamespace

import numpy as np
import torch

from helpers import GOLDEN
from panacea_amd import sampling as S

CHURN = dict(s_churn=1.0, s_tmin=0.5, s_tmax=10.0)
CASES = {
    "euler_churn": ("EulerEDMSampler", CHURN),
    "heun": ("HeunEDMSampler", {}),
    "heun_churn": ("HeunEDMSampler", CHURN),
    "euler_a": ("EulerAncestralSampler", {}),
    "dpmpp2s_a": ("DPMPP2SAncestralSampler", {}),
    "dpmpp2m": ("DPMPP2MSampler", {}),
    "lms": ("LinearMultistepSampler", {"order": 4}),
}


def golden(name):
    return np.load(GOLDEN / name)


def make(name, n, device="cpu", scale=5.0):
    cls, kw = CASES[name]
    return getattr(S, cls)(n, guider=S.VanillaCFG(scale), device=device, **kw)


def inject_noise(smp, noise: np.ndarray):
    """the sampler draws the noise the reference drew, in order; returns a function telling how many were used"""
    draws = [torch.from_numpy(z) for z in noise]
    used = [0]

    def sampler(x):
        z = draws[used[0]]
        used[0] += 1
        return z.to(device=x.device, dtype=x.dtype)
    smp.noise_sampler = sampler
    return lambda: used[0]


def fake_network(x, t, c):
    return torch.tanh(0.3 * x) * 0.5 + 1e-4 * t.float()[:, None, None, None] + 0.01 * c["crossattn"].mean() \
        + 0.05 * c["concat"]


def fake_inputs(device="cpu"):
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(2, 4, 4, 12, generator=g)
    c = {"crossattn": torch.randn(1, 77, 8, generator=g), "concat": torch.randn(2, 4, 4, 12, generator=g),
         "cond_feat": torch.rand(2, 19, 8, 8, generator=g)}
    uc = {"crossattn": torch.randn(1, 77, 8, generator=g), "concat": c["concat"].clone(), "cond_feat": c["cond_feat"].clone()}
    mv = lambda d: {k: v.to(device) for k, v in d.items()}     # noqa: E731
    return x0.to(device), mv(c), mv(uc)


class FakeTokenNetwork:
    """`network.diffusion_model.denoise_tokens` around fake_network: eps of the CFG batch as channels-last fp32 tokens, the
    timesteps it saw recorded in `seen`"""

    def __init__(self):
        self.seen = []
        w = torch.zeros(1)
        self.diffusion_model = SimpleNamespace(denoise_tokens=self.denoise_tokens,
                                               controlnet=SimpleNamespace(input_hint_block=[SimpleNamespace(weight=w)]))

    def denoise_tokens(self, x, c_in, c_noise, ctx, concat, cond_feat, invariants=None):
        nh = c_in.shape[0] // x.shape[0]
        self.seen.append(c_noise.clone())
        eps = fake_network(torch.cat([x] * nh) * c_in[:, None, None, None], c_noise, {"crossattn": ctx, "concat": concat})
        T, C, H, W = eps.shape
        return SimpleNamespace(f32=eps.permute(0, 2, 3, 1).reshape(-1, C).contiguous(), C=C, N=H * W)
