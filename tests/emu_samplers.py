"""CPU emulation of pnc_cfg_sampler_step (include/panacea_hip.h) for the emu backend of tests/emu.py: the reference's torch ops
in the reference's order (sampling.py:85-365) on channels-last eps tokens.  tests/test_samplers.py attaches it to `emu` with
monkeypatch; the HIP kernel is held to the same trajectories on the MI355X (tests/test_samplers_gpu.py)."""
import torch

import emu
from panacea_amd import hip


def cfg_sampler_step(mode, eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, v, out, out_aux=None, x0=None, aux=None, hist=(),
                     noise=None, s_noise=1.0):
    E = emu._mat(eps_tok, (2 if cfg else 1) * T * Npix, Cch, ld).view(-1, T, Npix, Cch).permute(0, 1, 3, 2)   # [halves, T, C, Npix]
    X = x.reshape(T, Cch, Npix)
    D = E * c_out.reshape(T, 1, 1) + X
    D = D[0] + scale * (D[1] - D[0]) if cfg else D[0]
    v = [t.reshape(T, 1, 1) for t in v]
    plane = lambda t: t.reshape(T, Cch, Npix)                       # noqa: E731
    if mode == hip.SAMPLER_HEUN1:
        d = (X - D) / v[0]
        y = X + (v[1] - v[0]) * d
        plane(out_aux).copy_(d)
    elif mode == hip.SAMPLER_HEUN2:
        d_new = (X - D) / v[1]
        d_prime = (plane(aux) + d_new) / 2.0
        y = torch.where(v[1] > 0.0, plane(x0) + d_prime * (v[1] - v[0]), X)
    elif mode in (hip.SAMPLER_EULER_A, hip.SAMPLER_DPM2S_1):
        xe = X + (v[1] - v[0]) * ((X - D) / v[0])
        if mode == hip.SAMPLER_DPM2S_1:
            y = v[2] * X - v[3] * D
            plane(out_aux).copy_(xe)
        else:
            y = torch.where(v[3] > 0.0, xe + plane(noise) * s_noise * v[2], xe)
    elif mode == hip.SAMPLER_DPM2S_2:
        xs = torch.where(v[2] > 0.0, v[0] * plane(x0) - v[1] * D, plane(aux))
        y = torch.where(v[4] > 0.0, xs + plane(noise) * s_noise * v[3], xs)
    elif mode == hip.SAMPLER_DPM2M:
        y = v[0] * X - v[1] * D
        if aux is not None:
            y = torch.where(v[4] > 0.0, v[0] * X - v[1] * (v[2] * D - v[3] * plane(aux)), y)
        plane(out_aux).copy_(D)
    elif mode == hip.SAMPLER_LMS:
        d = (X - D) / v[0]
        acc = 0 + v[1] * d
        for k, h in enumerate(hist):
            acc = acc + v[2 + k] * plane(h)
        y = X + acc
        plane(out_aux).copy_(d)
    else:
        raise ValueError(f"mode {mode}")
    plane(out).copy_(y)
