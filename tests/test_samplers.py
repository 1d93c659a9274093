"""Heun / ancestral / DPM++ / LMS sampler mirrors and their exit kernel pnc_cfg_sampler_step (CPU: the emulation of
tests/emu.py) against the reference's own sampler classes (tests/golden/samplers*.npz, tools/gen_golden_samplers.py)."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import emu
from sampler_cases import CASES, FakeTokenNetwork, fake_inputs, fake_network, golden, inject_noise, make
from panacea_amd import engine as E, hip, sampling as S

G = golden("samplers.npz")
GT = golden("samplers_tiny_net.npz")
TOL = float(GT["tol_rel"])


@pytest.fixture
def emu_backend():
    with E.use_backend(emu):
        yield


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("n", [3, 25])
def test_mirror_reproduces_the_reference_sampler(name, n):
    x0, c, uc = fake_inputs()
    den = S.DiscreteDenoiser()
    seen = []

    def net(x, t, cc):
        seen.append(t.clone())
        return fake_network(x, t, cc)
    smp = make(name, n)
    used = inject_noise(smp, G[f"{name}.{n}.noise"])
    with torch.no_grad():
        xs = smp(lambda inp, sigma, cc: den(net, inp, sigma, cc), x0.clone(), c, uc)
    assert np.array_equal(torch.stack(seen)[:, 0].numpy(), G[f"{name}.{n}.timesteps"])
    assert used() == len(G[f"{name}.{n}.noise"])
    assert np.allclose(xs.numpy(), G[f"{name}.{n}.x_final"], atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("n", [3, 25])
def test_exit_kernel_replays_the_reference_sampler_on_the_emulation(name, n, emu_backend):
    """the fused device loop: eps tokens of the stand-in network + one exit kernel per network evaluation"""
    x0, c, uc = fake_inputs()
    net = FakeTokenNetwork()
    bd = S.BoundDenoiser(S.DiscreteDenoiser(), net)
    smp = make(name, n)
    assert smp._fusable_network(bd, c)
    inject_noise(smp, G[f"{name}.{n}.noise"])
    sig, sig_f = smp.sigmas(), smp.host_sigmas()
    x = x0 * torch.sqrt(1.0 + sig[0] ** 2.0)
    s_in = x.new_ones([x.shape[0]])
    with torch.no_grad():
        if isinstance(smp, S.EulerEDMSampler):
            state = smp._state(x)
            for form, sv, draw in smp._steps(sig, sig_f, s_in):
                if draw:
                    sv["noise"] = smp.noise_sampler(x)
                x = smp._device_step(form, sv, x, bd, c, uc, state)
        else:
            x = smp._fused_loop(sig, sig_f, s_in, bd, x, c, uc)
    assert np.array_equal(torch.stack(net.seen)[:, 0].numpy(), G[f"{name}.{n}.timesteps"])
    assert np.allclose(x.numpy(), G[f"{name}.{n}.x_final"], atol=2e-5, rtol=1e-5)


def _tiny(kw):
    from helpers import step_inputs
    inp = step_inputs("tiny", kw)
    T = kw["num_frames"]
    c = {"crossattn": inp["crossattn"][1:2], "concat": inp["concat"][T:], "cond_feat": inp["cond_feat"][T:]}
    uc = {"crossattn": inp["crossattn"][0:1], "concat": inp["concat"][:T], "cond_feat": inp["cond_feat"][:T]}
    x0 = inp["x"][T:].clone()
    assert np.array_equal(x0.numpy(), GT["x0"])
    return x0, c, uc


def _run(smp, bd, x0, c, uc, fused, network=None):
    """the sampler's schedule, plain (reference torch ops) or fused (device loop), with the latent after every step"""
    xs = []
    rec = lambda i, x: xs.append(x.clone())              # noqa: E731
    with torch.no_grad():
        if not fused:
            smp(bd, x0.clone(), c, uc, network=network, callback=rec)
        else:
            if network is not None:
                c, uc = S.hoist_invariants(network, smp.guider, c, uc)
            sig, sig_f = smp.sigmas(), smp.host_sigmas()
            x = x0 * torch.sqrt(1.0 + sig[0] ** 2.0)
            smp._fused_loop(sig, sig_f, x.new_ones([x.shape[0]]), bd, x, c, uc, callback=rec)
    return torch.stack(xs)


@pytest.mark.parametrize("name", ["heun", "heun_churn", "euler_a", "dpmpp2s_a", "dpmpp2m", "lms"])
def test_fused_steps_are_the_plain_steps_and_replay_the_tiny_net_reference(name, emu_backend):
    """on the tiny product network (emulated kernels): fused == plain bit for bit, also with hoisted invariants, and both
    within the stated tolerance of the reference's sampler around the reference network (samplers_tiny_net.npz)"""
    from helpers import product_network
    w, _, kw = product_network("tiny")
    x0, c, uc = _tiny(kw)
    bd = S.BoundDenoiser(S.DiscreteDenoiser(), w)
    runs = {}
    for mode in ("plain", "fused", "fused+hoisted"):
        smp = make(name, int(GT["steps"]), scale=float(GT["cfg_scale"]))
        inject_noise(smp, GT[f"{name}.noise"])
        runs[mode] = _run(smp, bd, x0, c, uc, mode != "plain", w if mode == "fused+hoisted" else None)
    assert torch.equal(runs["plain"], runs["fused"]) and torch.equal(runs["fused"], runs["fused+hoisted"])
    ref = torch.from_numpy(GT[f"{name}.x_steps"])
    errs = [((a - b).abs().max() / b.abs().max()).item() for a, b in zip(runs["fused"], ref)]
    assert max(errs) <= TOL, errs


def test_lms_coefficients_quadrature_fallback(monkeypatch):
    """Gauss-Legendre (no scipy) gives the same fp32 coefficients as scipy's quad"""
    import builtins
    sig_f = S.LegacyDDPMDiscretization()(25).tolist()
    smp = S.LinearMultistepSampler(25, device="cpu")
    with_quad = smp.coefficients(sig_f)
    real_import = builtins.__import__

    def no_scipy(name, *a, **k):
        if name.startswith("scipy"):
            raise ImportError(name)
        return real_import(name, *a, **k)
    monkeypatch.setattr(builtins, "__import__", no_scipy)
    gauss = smp.coefficients(sig_f)
    assert [len(c) for c in gauss] == [1, 2, 3] + [4] * 22
    for a, b in zip(with_quad, gauss):
        np.testing.assert_allclose(a, b, rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("name", sorted(S.SAMPLERS))
def test_from_config_builds_every_yaml_target(name):
    P = "sgm.modules.diffusionmodules."
    cfg = {"target": P + "sampling." + name,
           "params": {"num_steps": 15, "discretization_config": {"target": P + "discretizer.LegacyDDPMDiscretization"},
                      "guider_config": {"target": P + "guiders.VanillaCFG", "params": {"scale": 5.0}}}}
    extra = {"HeunEDMSampler": {"s_churn": 0.5}, "EulerAncestralSampler": {"eta": 0.5, "s_noise": 0.9},
             "LinearMultistepSampler": {"order": 3}}.get(name, {})
    cfg["params"].update(extra)
    smp = S.from_config(cfg, device="cpu")
    assert type(smp) is S.SAMPLERS[name] and smp.num_steps == 15 and smp.guider.scale == 5.0
    assert isinstance(smp.discretization, S.LegacyDDPMDiscretization)
    for k, v in extra.items():
        assert getattr(smp, k) == v
    assert S.from_config({"target": P + "sampling." + name}, device="cpu").guider is None      # IdentityGuider default
    with pytest.raises(NotImplementedError, match="NoSuchSampler"):
        S.from_config({"target": P + "sampling.NoSuchSampler"})


def test_new_samplers_refuse_sharded_cfg():
    class Half(S.VanillaCFG):
        half, group = 0, None
    for name in ("heun", "euler_a", "dpmpp2s_a", "dpmpp2m", "lms"):
        smp = make(name, 3)
        smp.guider = Half(5.0)
        with pytest.raises(NotImplementedError, match="ShardedCFG"):
            smp(lambda *a: None, torch.zeros(2, 4, 4, 12), {}, {})


def test_sampler_struct_matches_the_header_as_gcc_lays_it_out(tmp_path):
    fields = [f[0] for f in hip.SamplerStepParams._fields_]
    modes = ["HEUN1", "HEUN2", "EULER_A", "DPM2S_1", "DPM2S_2", "DPM2M", "LMS"]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hip.HEADER}"', 'int main(void) {',
           'printf("size %zu\\n", sizeof(PncSamplerStepParams));']
    src += [f'printf("{f} %zu\\n", offsetof(PncSamplerStepParams, {f}));' for f in fields]
    src += [f'printf("PNC_SAMPLER_{m} %d\\n", (int)PNC_SAMPLER_{m});' for m in modes]
    src.append('printf("abi %d\\n", PNC_ABI_VERSION); return 0; }')
    c = tmp_path / "sampler_layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "sampler_layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(c), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert int(got["size"]) == ctypes.sizeof(hip.SamplerStepParams)
    for f in fields:
        assert int(got[f]) == getattr(hip.SamplerStepParams, f).offset, f
    for m in modes:
        assert int(got[f"PNC_SAMPLER_{m}"]) == getattr(hip, f"SAMPLER_{m}"), m
    assert int(got["abi"]) == hip.ABI_VERSION == 8


def test_sampler_step_validates_its_arguments_without_gpu():
    lib = hip.load()
    p = hip.SamplerStepParams()
    assert lib.pnc_cfg_sampler_step(ctypes.byref(p), None) == -3            # PNC_EABI: struct_bytes not set
    p.struct_bytes = ctypes.sizeof(hip.SamplerStepParams) - 8
    assert lib.pnc_cfg_sampler_step(ctypes.byref(p), None) == -3            # a shorter struct of another header
    p.struct_bytes = ctypes.sizeof(hip.SamplerStepParams)
    assert lib.pnc_cfg_sampler_step(ctypes.byref(p), None) == -1            # PNC_EINVAL: null operands
    p.eps_tok = p.x = p.c_out = p.out = 16
    p.ld, p.T, p.Npix, p.C, p.mode = 4, 1, 1, 4, hip.SAMPLER_HEUN1
    assert lib.pnc_cfg_sampler_step(ctypes.byref(p), None) == -1            # HEUN1 without out_aux / sigma vectors
    p.mode = 7
    assert lib.pnc_cfg_sampler_step(ctypes.byref(p), None) == -1            # unknown mode
