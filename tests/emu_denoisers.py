"""CPU emulation of the denoiser-parameterisation entry points (include/panacea_hip.h: pnc_timestep_embedding_f32,
pnc_cfg_euler_step_skip, pnc_cfg_sampler_step_skip) for the emu backend of tests/emu.py, layered on it the way
tests/emu_samplers.py is: the reference's torch ops in the reference's order (denoiser.py:28: eps * c_out + x * c_skip), then the
update of the eps-path emulation.  `attach(monkeypatch)` puts them on `emu`; without a `c_skip` the eps-path emulations run
untouched.  The HIP kernels are held to the same trajectories on the MI355X (tests/test_denoisers_gpu.py)."""
import torch

import emu
import emu_samplers

_eps_euler_step = emu.cfg_euler_step          # the eps-path emulation (attach() puts this module's function in its place)


def timestep_embedding_f32(t_f32, F, dim, freqs, out32):
    """float timesteps as given: the int64 emulation's arithmetic after its `.float()`"""
    assert t_f32.dtype == torch.float32
    emu.timestep_embedding(t_f32, F, dim, freqs, out32)


def _denoised(eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, c_skip):
    """(X [T, C, Npix], guided D): D_h = E_h * c_out + X * c_skip with both products and the sum rounded on their own, then CFG"""
    E = emu._mat(eps_tok, (2 if cfg else 1) * T * Npix, Cch, ld).view(-1, T, Npix, Cch).permute(0, 1, 3, 2)   # [halves, T, C, Npix]
    X = x.reshape(T, Cch, Npix)
    D = E * c_out.reshape(T, 1, 1) + X * c_skip.reshape(T, 1, 1)
    return X, (D[0] + scale * (D[1] - D[0]) if cfg else D[0])


def cfg_euler_step(eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, sigma, sigma_next, x_next, c_skip=None):
    if c_skip is None:
        return _eps_euler_step(eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, sigma, sigma_next, x_next)
    X, D = _denoised(eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, c_skip)
    sg = sigma.reshape(T, 1, 1)
    d = (X - D) / sg
    x_next.reshape(T, Cch, Npix).copy_(X + (sigma_next.reshape(T, 1, 1) - sg) * d)


def cfg_sampler_step(mode, eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, v, out, out_aux=None, x0=None, aux=None, hist=(),
                     noise=None, s_noise=1.0, c_skip=None):
    if c_skip is None:
        return emu_samplers.cfg_sampler_step(mode, eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, v, out, out_aux=out_aux, x0=x0,
                                             aux=aux, hist=hist, noise=noise, s_noise=s_noise)
    # the mode's update is emu_samplers' own, written out again because that function forms its D (c_skip = 1) inside
    from panacea_amd import hip
    X, D = _denoised(eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, c_skip)
    v = [t.reshape(T, 1, 1) for t in v]
    plane = lambda t: t.reshape(T, Cch, Npix)                       # noqa: E731
    if mode == hip.SAMPLER_HEUN1:
        d = (X - D) / v[0]
        y = X + (v[1] - v[0]) * d
        plane(out_aux).copy_(d)
    elif mode == hip.SAMPLER_HEUN2:
        d_new = (X - D) / v[1]
        y = torch.where(v[1] > 0.0, plane(x0) + ((plane(aux) + d_new) / 2.0) * (v[1] - v[0]), X)
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


def attach(monkeypatch):
    """put the emulations on tests/emu.py's module for one test (monkeypatch undoes it)"""
    monkeypatch.setattr(emu, "timestep_embedding_f32", timestep_embedding_f32, raising=False)
    monkeypatch.setattr(emu, "cfg_euler_step", cfg_euler_step)
    monkeypatch.setattr(emu, "cfg_sampler_step", cfg_sampler_step, raising=False)
