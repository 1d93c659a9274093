"""pnc_cfg_sampler_step and the Heun / ancestral / DPM++ / LMS sampler mirrors on the MI355X (-m gpu): the reference's own
trajectories (tests/golden/samplers*.npz, tools/gen_golden_samplers.py) replayed through the HIP exit kernel, plain vs fused vs
fused + hoisted vs graphed on the tiny network, and short fused schedules at the config-3 shape."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

from helpers import product_network, step_inputs
from sampler_cases import CASES, FakeTokenNetwork, fake_inputs, golden, inject_noise, make
from panacea_amd import hip, sampling as S
from panacea_amd.graph import GraphedSchedule

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = golden("samplers.npz")
GT = golden("samplers_tiny_net.npz")
TOL = float(GT["tol_rel"])


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


@pytest.mark.parametrize("name", sorted(CASES))
def test_exit_kernel_replays_the_reference_samplers(name):
    """the fused loop around the closed-form stand-in network: eps tokens -> pnc_cfg_sampler_step (Euler churn: churn +
    pnc_cfg_euler_step) against the reference's 3- and 25-step trajectories"""
    for n in (3, 25):
        x0, c, uc = fake_inputs(DEV)
        net = FakeTokenNetwork()
        bd = S.BoundDenoiser(S.DiscreteDenoiser().to(DEV), net)
        smp = make(name, n, DEV)
        assert smp._fusable(bd, x0, c)
        inject_noise(smp, G[f"{name}.{n}.noise"])
        with torch.no_grad():
            xs = smp(bd, x0.clone(), c, uc)
        torch.cuda.synchronize()
        assert np.array_equal(torch.stack(net.seen)[:, 0].cpu().numpy(), G[f"{name}.{n}.timesteps"])
        assert np.allclose(xs.cpu().numpy(), G[f"{name}.{n}.x_final"], atol=2e-5, rtol=1e-5), (name, n)
    assert "libpanacea_hip.so" in Path("/proc/self/maps").read_text()


def _tiny_inputs(kw):
    inp = step_inputs("tiny", kw, DEV)
    T = kw["num_frames"]
    c = {"crossattn": inp["crossattn"][1:2], "concat": inp["concat"][T:], "cond_feat": inp["cond_feat"][T:]}
    uc = {"crossattn": inp["crossattn"][0:1], "concat": inp["concat"][:T], "cond_feat": inp["cond_feat"][:T]}
    x0 = inp["x"][T:].clone()
    assert np.array_equal(x0.cpu().numpy(), GT["x0"])
    return x0, c, uc


@pytest.mark.parametrize("name", ["euler_churn", "heun", "heun_churn", "euler_a", "dpmpp2s_a", "dpmpp2m", "lms"])
def test_tiny_net_plain_fused_hoisted_graphed(name):
    w, _, kw = product_network("tiny", DEV)
    x0, c, uc = _tiny_inputs(kw)
    bd = S.BoundDenoiser(S.DiscreteDenoiser().to(DEV), w)
    steps, scale = int(GT["steps"]), float(GT["cfg_scale"])
    runs = {}
    for mode in ("plain", "fused", "fused+hoisted", "graphed"):
        smp = make(name, steps, DEV, scale)
        smp.fuse = mode != "plain"
        xs = []
        rec = lambda i, x: xs.append(x.detach().clone())      # noqa: E731
        with torch.no_grad():
            if mode == "graphed":
                g = GraphedSchedule(smp, bd, x0, c, uc, network=w)
                inject_noise(smp, GT[f"{name}.noise"])
                g(x0.clone(), callback=rec)
            else:
                used = inject_noise(smp, GT[f"{name}.noise"])
                smp(bd, x0.clone(), c, uc, network=w if mode == "fused+hoisted" else None, callback=rec)
                assert used() == len(GT[f"{name}.noise"])
        torch.cuda.synchronize()
        runs[mode] = torch.stack(xs).cpu()
    ref = torch.from_numpy(GT[f"{name}.x_steps"])
    for mode, xs in runs.items():
        errs = [((a - b).abs().max() / b.abs().max()).item() for a, b in zip(xs, ref)]
        print(f"{name} {mode}: per-step error / max|x| {['%.2e' % e for e in errs]}")
        assert max(errs) <= TOL, (name, mode, errs)
    d = (runs["fused"] - runs["plain"]).abs().max().item()
    print(f"{name}: fused vs plain max {d:.3e}, fused == plain bitwise {torch.equal(runs['fused'], runs['plain'])}")
    assert d <= 2e-5
    assert torch.equal(runs["fused"], runs["fused+hoisted"])
    assert torch.equal(runs["graphed"], runs["fused+hoisted"])


@pytest.mark.parametrize("cls", [S.DPMPP2MSampler, S.HeunEDMSampler])
def test_two_step_schedule_at_the_config3_shape(cls):
    w, _, kw = product_network("full", DEV)
    inp = step_inputs("full", kw, DEV)
    T = kw["num_frames"]
    c = {"crossattn": inp["crossattn"][1:2], "concat": inp["concat"][T:], "cond_feat": inp["cond_feat"][T:]}
    uc = {"crossattn": inp["crossattn"][0:1], "concat": inp["concat"][:T], "cond_feat": inp["cond_feat"][:T]}
    x0 = inp["x"][T:].clone()
    bd = S.BoundDenoiser(S.DiscreteDenoiser().to(DEV), w)
    out = {}
    for fused in (False, True):
        smp = cls(2, guider=S.VanillaCFG(5.0), device=DEV)
        smp.fuse = fused
        with torch.no_grad():
            out[fused] = smp(bd, x0.clone(), c, uc, network=w if fused else None)
        torch.cuda.synchronize()
    d = (out[True] - out[False]).abs().max().item()
    print(f"{cls.__name__} 2 steps at {tuple(x0.shape)}: fused + hoisted vs plain max {d:.3e}")
    assert torch.isfinite(out[True]).all() and d <= 2e-5


def test_sampler_step_refuses_a_short_struct():
    T, Npix, C = 1, 64, 4
    eps, x, out, d = (torch.zeros(T * C * Npix, device=DEV) for _ in range(4))
    sig = torch.ones(T, device=DEV)
    p = hip.SamplerStepParams()
    p.struct_bytes = ctypes.sizeof(hip.SamplerStepParams) - 8
    p.mode, p.ld, p.T, p.Npix, p.C = hip.SAMPLER_LMS, C, T, Npix, C
    p.eps_tok, p.x, p.c_out, p.out, p.out_aux = eps.data_ptr(), x.data_ptr(), sig.data_ptr(), out.data_ptr(), d.data_ptr()
    p.v[0] = p.v[1] = sig.data_ptr()
    lib = hip.load()
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.pnc_cfg_sampler_step(ctypes.byref(p), stream) == -3             # PNC_EABI
    p.struct_bytes = ctypes.sizeof(hip.SamplerStepParams)
    assert lib.pnc_cfg_sampler_step(ctypes.byref(p), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, x) and torch.equal(d, x)                             # eps 0: denoised = x, d = 0, x + 0
