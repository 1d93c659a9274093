"""What tests/test_clip_edit.py (emulated backend) and tests/test_clip_edit_gpu.py (MI355X) share: the tiny network (T = 2 frames,
latent 8 x 96) with the tiny first stage, the six samplers with step-indexed noise, and the `start_step` composition check."""
import torch

import rollout_cases as rc
import test_vae as tv
from helpers import product_network
from panacea_amd import configs, sampling as S, synth
from panacea_amd.nn import model

_, T, LH, LW = configs.SHAPES["tiny"]
H, W = 2 * LH, 2 * LW                            # frames of the tiny first stage (one Downsample)
STEPS = 4
SAMPLERS = {
    "euler": lambda n, dev: S.EulerEDMSampler(n, guider=S.VanillaCFG(5.0), device=dev),
    "heun": lambda n, dev: S.HeunEDMSampler(n, guider=S.VanillaCFG(5.0), device=dev),
    "euler_a": lambda n, dev: S.EulerAncestralSampler(n, guider=S.VanillaCFG(5.0), device=dev),
    "dpmpp2s_a": lambda n, dev: S.DPMPP2SAncestralSampler(n, guider=S.VanillaCFG(5.0), device=dev),
    "dpmpp2m": lambda n, dev: S.DPMPP2MSampler(n, guider=S.VanillaCFG(5.0), device=dev),
    "lms": lambda n, dev: S.LinearMultistepSampler(n, guider=S.VanillaCFG(5.0), device=dev, order=4),
    "lms1": lambda n, dev: S.LinearMultistepSampler(n, guider=S.VanillaCFG(5.0), device=dev, order=1),
}
KEEPERS = ("euler", "dpmpp2m", "lms")            # one network evaluation per step feeds the next, no fresh noise
REFUSERS = ("heun", "euler_a", "dpmpp2s_a")


def composes_exactly(name: str, start_step: int, n: int = STEPS) -> bool:
    """Whether a run begun at `start_step` from the ordinary run's latent ends on the ordinary run's bits.  The one-step samplers
    carry nothing from step to step.  DPM++ 2M's step uses the previous denoised unless it is the first step or the last (every
    next_sigma 0: the standard update), so a restart — which has no previous denoised — agrees exactly when it begins at the last
    step.  LMS of order 4 uses the previous d from its second step on, so a restart (order 1 at its first step) never agrees;
    order 1 has no history to lose."""
    if name == "dpmpp2m":
        return start_step == n - 1
    return name != "lms"


def tiny_stack(device="cpu"):
    net, _, kw = product_network("tiny", device)
    _, sd, _ = tv._tiny()
    dec = model.FirstStageDecoder(4, tv.TINY)
    dec.load_state_dict(sd, strict=True)
    return dict(net=net, dec=dec.to(device), enc=rc.tiny_encoder(device), kw=kw)


def tiny_inputs(kw, device="cpu"):
    """(x0, cond, uc) of one sample: the conditional half of the synthetic step inputs, the unconditional half as uc"""
    inp = synth.synth_inputs(2, T, LH, LW, context_dim=kw["context_dim"])
    c = {"crossattn": inp["crossattn"][1:2].clone(), "concat": inp["concat"][T:].clone(), "cond_feat": inp["cond_feat"][T:].clone()}
    uc = {"crossattn": inp["crossattn"][0:1].clone(), "concat": inp["concat"][:T].clone(), "cond_feat": inp["cond_feat"][:T].clone()}
    mv = lambda d: {k: v.to(device) for k, v in d.items()}      # noqa: E731
    return inp["x"][T:].clone().to(device), mv(c), mv(uc)


def clip_u8(device="cpu", seed=21):
    return rc.frames_u8(T, seed=seed).to(device)


def make(name, n=STEPS, device="cpu"):
    """the sampler with noise that depends on the step index alone, so that a restarted run draws what the ordinary run drew"""
    smp = SAMPLERS[name](n, device)
    smp.step_index = 0

    def draw(x):
        g = torch.Generator().manual_seed(77 + smp.step_index)
        return torch.randn(x.shape, generator=g).to(device=x.device, dtype=x.dtype)
    smp.noise_sampler = draw
    return smp


def run(smp, bd, x, c, uc, **kw):
    """smp(...) -> (result, the latent after every step by index)"""
    seen = {}
    smp.step_index = kw.get("start_step", 0)

    def rec(i, x):
        seen[i] = x.detach().clone()
        smp.step_index = i + 1
    with torch.no_grad():
        out = smp(bd, x, c, uc, callback=rec, **kw)
    return out, seen


def check_composition(name, bd, x0, c, uc, n=STEPS, device="cpu", ks=None):
    """an ordinary run records x after step k; a second run with start_step = k + 1 from that x ends on the same bits where
    `composes_exactly` says so, and differs (finitely) elsewhere"""
    full, seen = run(make(name, n, device), bd, x0.clone(), c, uc)
    assert sorted(seen) == list(range(n)) and torch.equal(seen[n - 1], full)
    for k in (range(n - 1) if ks is None else ks):
        tail, seen_k = run(make(name, n, device), bd, seen[k].clone(), c, uc, start_step=k + 1)
        assert sorted(seen_k) == list(range(k + 1, n)), (name, k)
        if composes_exactly(name, k + 1, n):
            assert torch.equal(tail, full), (name, k, (tail - full).abs().max().item())
        else:
            assert torch.isfinite(tail).all() and not torch.equal(tail, full), (name, k)
    return full
