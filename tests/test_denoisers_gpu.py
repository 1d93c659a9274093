"""pnc_timestep_embedding_f32, the general-skip exit kernels and the denoiser parameterisations (v-prediction, EDM, continuous
c_noise) on the MI355X (-m gpu): the reference's own trajectories (tests/golden/denoisers*.npz, tools/gen_golden_denoisers.py)
replayed through the HIP kernels; plain vs fused vs fused + hoisted vs graphed on the tiny network; the general-skip entries
against the eps entries with c_skip = 1; and a short v-prediction schedule at the config-3 shape."""
import ctypes
import hashlib
from pathlib import Path

import numpy as np
import pytest
import torch

from denoiser_cases import CASES, SAMPLERS, TINY_SAMPLERS, make
from helpers import product_network, step_inputs
from sampler_cases import FakeTokenNetwork, fake_inputs, golden, inject_noise
from panacea_amd import engine as E, hip, sampling as S
from panacea_amd.graph import GraphedSchedule

pytestmark = pytest.mark.gpu
DEV = "cuda"
G = golden("denoisers.npz")
GT = golden("denoisers_tiny_net.npz")
TOL = float(GT["tol_rel"])


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def test_timestep_embedding_f32_against_the_int64_kernel_and_torch():
    dim = 320
    freqs = E.timestep_freqs(dim, torch.device(DEV))
    ti = torch.cat([torch.arange(0, 1000, 7), torch.tensor([999])]).to(DEV)
    a, b = (torch.zeros(ti.numel(), dim, device=DEV) for _ in range(2))
    hip.timestep_embedding(ti, ti.numel(), dim, freqs, a)
    hip.timestep_embedding_f32(ti.float(), ti.numel(), dim, freqs, b)
    torch.cuda.synchronize()
    assert torch.equal(a, b)                                             # integer-valued floats: the int64 kernel's bits
    g = torch.Generator().manual_seed(3)
    t = torch.cat([torch.rand(64, generator=g) * 2.2 - 1.1,              # EDMScaling's 0.25 log sigma
                   torch.rand(64, generator=g) * 14.6,                   # a float sigma as c_noise
                   torch.rand(16, generator=g) * 999.0]).to(DEV)
    out = torch.zeros(t.numel(), dim, device=DEV)
    hip.timestep_embedding_f32(t, t.numel(), dim, freqs, out)
    torch.cuda.synchronize()
    args = t.cpu()[:, None] * freqs.cpu()[None]
    ref = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    d = (out.cpu() - ref).abs().max().item()
    print(f"pnc_timestep_embedding_f32 vs torch fp32 on non-integer timesteps: max abs {d:.3e}")
    assert d <= 2e-4                  # the bound of the timestep_embedding case of tests/test_kernels_vs_oracle_gpu.py
    # through nn.util: the float route is taken, nothing truncates
    from panacea_amd.nn.util import timestep_embedding
    assert torch.equal(timestep_embedding(t, dim), out)
    assert not torch.equal(timestep_embedding(t.to(torch.int64), dim), out)


def _c_noise_matches(seen, want):
    got = torch.stack(seen)[:, 0].cpu().numpy()
    assert got.dtype == want.dtype
    if want.dtype == np.int64:
        return np.array_equal(got, want)
    # a float c_noise passes through the device's own pow / log (the schedule, 0.25 log sigma), which are not specified to
    # the bit: a few ulps, where truncation would be off by O(1)
    return np.allclose(got, want, rtol=1e-6, atol=1e-6)


@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("case", sorted(CASES))
def test_fused_loop_replays_the_reference_trajectories(case, sampler):
    """the fused loop around the closed-form stand-in network: eps tokens -> pnc_cfg_euler_step[_skip] / pnc_cfg_sampler_step[_skip]
    against the reference's 3- and 25-step trajectories"""
    for n in (3, 25):
        key = f"{case}.{sampler}.{n}"
        x0, c, uc = fake_inputs(DEV)
        net = FakeTokenNetwork()
        den, smp = make(case, sampler, n, DEV)
        bd = S.BoundDenoiser(den, net)
        assert smp._fusable(bd, x0, c)
        used = inject_noise(smp, G[key + ".noise"])
        with torch.no_grad():
            xs = smp(bd, x0.clone(), c, uc)
        torch.cuda.synchronize()
        assert used() == len(G[key + ".noise"])
        assert _c_noise_matches(net.seen, G[key + ".c_noise"]), key
        err = np.abs(xs.cpu().numpy() - G[key + ".x_final"]).max()
        print(f"{key}: max abs vs reference {err:.3e}")
        assert np.allclose(xs.cpu().numpy(), G[key + ".x_final"], atol=2e-5, rtol=1e-5), key
    assert "libpanacea_hip.so" in Path("/proc/self/maps").read_text()


def _tiny_inputs(kw):
    inp = step_inputs("tiny", kw, DEV)
    T = kw["num_frames"]
    c = {"crossattn": inp["crossattn"][1:2], "concat": inp["concat"][T:], "cond_feat": inp["cond_feat"][T:]}
    uc = {"crossattn": inp["crossattn"][0:1], "concat": inp["concat"][:T], "cond_feat": inp["cond_feat"][:T]}
    x0 = inp["x"][T:].clone()
    assert np.array_equal(x0.cpu().numpy(), GT["x0"])
    return x0, c, uc


@pytest.mark.parametrize("sampler", TINY_SAMPLERS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_tiny_net_plain_fused_hoisted_graphed(case, sampler):
    """Measured on the MI355X, per-step error / max|x| against the reference (worst of the four run modes): see DESIGN.md §6,
    row "denoiser parameterisations"."""
    w, _, kw = product_network("tiny", DEV)
    x0, c, uc = _tiny_inputs(kw)
    steps, scale = int(GT["steps"]), float(GT["cfg_scale"])
    key = f"{case}.{sampler}"
    runs = {}
    for mode in ("plain", "fused", "fused+hoisted", "graphed"):
        den, smp = make(case, sampler, steps, DEV, scale)
        bd = S.BoundDenoiser(den, w)
        smp.fuse = mode != "plain"
        xs = []
        rec = lambda i, x: xs.append(x.detach().clone())      # noqa: E731
        with torch.no_grad():
            if mode == "graphed":
                GraphedSchedule(smp, bd, x0, c, uc, network=w)(x0.clone(), callback=rec)
            else:
                smp(bd, x0.clone(), c, uc, network=w if mode == "fused+hoisted" else None, callback=rec)
        torch.cuda.synchronize()
        runs[mode] = torch.stack(xs).cpu()
    ref = torch.from_numpy(GT[key + ".x_steps"])
    for mode, xs in runs.items():
        errs = [((a - b).abs().max() / b.abs().max()).item() for a, b in zip(xs, ref)]
        print(f"{key} {mode}: per-step error / max|x| {['%.2e' % e for e in errs]}")
    for mode, xs in runs.items():
        errs = [((a - b).abs().max() / b.abs().max()).item() for a, b in zip(xs, ref)]
        assert max(errs) <= TOL, (key, mode, errs)
    d = (runs["fused"] - runs["plain"]).abs().max().item()
    print(f"{key}: fused vs plain max {d:.3e}, fused == plain bitwise {torch.equal(runs['fused'], runs['plain'])}")
    assert d <= 2e-5
    assert torch.equal(runs["fused"], runs["fused+hoisted"])
    assert torch.equal(runs["graphed"], runs["fused+hoisted"])


def _exit_operands(T=2, C=4, Npix=96, ld=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).to(DEV)        # noqa: E731
    pos = lambda: (torch.rand(T, generator=g) + 0.5).to(DEV)   # noqa: E731
    return dict(tok=r(2 * T * Npix, ld), x=r(T, C, Npix), x0=r(T, C, Npix), aux=r(T, C, Npix), noise=r(T, C, Npix),
                hist=[r(T, C, Npix) for _ in range(3)], c_out=-pos(), v=[pos() for _ in range(6)])


MODES = {  # mode -> (number of per-frame vectors, operands)
    hip.SAMPLER_HEUN1: (2, ("out_aux",)), hip.SAMPLER_HEUN2: (2, ("x0", "aux")), hip.SAMPLER_EULER_A: (4, ("noise",)),
    hip.SAMPLER_DPM2S_1: (4, ("out_aux",)), hip.SAMPLER_DPM2S_2: (5, ("x0", "aux", "noise")),
    hip.SAMPLER_DPM2M: (5, ("out_aux", "aux")), hip.SAMPLER_LMS: (5, ("out_aux", "hist")),
}


def _struct_entry(mode, o, shape, cfg, c_skip):
    """(out, out_aux) of hip.cfg_sampler_step in `mode` on the operands `o`, with the operands MODES names (out_aux stays 0 where the
    mode writes none)"""
    T, C, Npix, ld = shape
    nv, ops = MODES[mode]
    out, out_aux = torch.zeros(T, C, Npix, device=DEV), torch.zeros(T, C, Npix, device=DEV)
    kw = {k: o[k] for k in ops if k in ("x0", "aux", "noise")}
    if "hist" in ops:
        kw["hist"] = o["hist"]
    if "out_aux" in ops:
        kw["out_aux"] = out_aux
    hip.cfg_sampler_step(mode, o["tok"], ld, T, Npix, C, cfg, 5.0, o["x"], o["c_out"], o["v"][:nv], out, s_noise=0.9, c_skip=c_skip, **kw)
    torch.cuda.synchronize()
    return out, out_aux


def _sha(t):
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


# (T, C, Npix, ld): the operands of the tests below; two workgroups with frame boundaries inside one, a partial last one and padded
# token rows; one live thread
EXIT_SHAPES = [(2, 4, 96, 8), (3, 4, 100, 8), (1, 1, 1, 1)]


@pytest.mark.parametrize("shape", EXIT_SHAPES, ids=lambda s: "T%dC%dN%dld%d" % s)
@pytest.mark.parametrize("skip", [False, True], ids=["eps", "skip"])
@pytest.mark.parametrize("cfg", [True, False], ids=["cfg", "nocfg"])
def test_euler_entries_are_heun1_of_the_struct_entries(cfg, skip, shape):
    """pnc_cfg_euler_step[_skip] against `out` of pnc_cfg_sampler_step[_skip] in mode HEUN1 with v = {sigma, sigma_next} on the same
    operands: the same bits, so the two kinds of entry cannot drift apart.  Prints the SHA-256 of every output plane of the Euler
    entry and of all seven modes of the struct entry: the lines a run on another build of the same ABI (PANACEA_HIP_LIB) must
    repeat one for one (profiles/sampler_exits.md)."""
    T, C, Npix, ld = shape
    o = _exit_operands(T, C, Npix, ld)
    cs = (torch.arange(T, dtype=torch.float32) * 0.17 + 0.3).to(DEV) if skip else None
    tag = f"cfg={int(cfg)} skip={int(skip)} T{T}C{C}N{Npix}ld{ld}"
    x_next = torch.zeros(T, C, Npix, device=DEV)
    hip.cfg_euler_step(o["tok"], ld, T, Npix, C, cfg, 5.0, o["x"], o["c_out"], o["v"][0], o["v"][1], x_next, c_skip=cs)
    torch.cuda.synchronize()
    print(f"exit-sha euler {tag} out={_sha(x_next)}")
    for mode in MODES:
        out, out_aux = _struct_entry(mode, o, shape, cfg, cs)
        print(f"exit-sha mode{mode} {tag} out={_sha(out)} out_aux={_sha(out_aux)}")
        if mode == hip.SAMPLER_HEUN1:
            assert torch.isfinite(out).all() and torch.equal(x_next, out)


@pytest.mark.parametrize("cfg", [True, False])
def test_skip_entries_with_c_skip_one_are_the_eps_entries(cfg):
    """x * 1 is exact, so the general-skip instantiation with c_skip = 1 must give the eps entries' bits: the shared device code
    has not drifted.  A c_skip other than 1 gives D = eps * c_out + x * c_skip in the reference's rounding order."""
    T, C, Npix, ld = 2, 4, 96, 8
    o = _exit_operands(T, C, Npix, ld)
    ones = torch.ones(T, device=DEV)
    skip = torch.tensor([0.25, 0.0625], device=DEV)
    for mode in MODES:
        res = {name: _struct_entry(mode, o, (T, C, Npix, ld), cfg, cs) for name, cs in (("eps", None), ("one", ones), ("skip", skip))}
        assert torch.equal(res["eps"][0], res["one"][0]) and torch.equal(res["eps"][1], res["one"][1]), mode
        assert torch.isfinite(res["skip"][0]).all() and not torch.equal(res["skip"][0], res["eps"][0]), mode
    res = {}
    for name, cs in (("eps", None), ("one", ones), ("skip", skip)):
        out = torch.zeros(T, C, Npix, device=DEV)
        hip.cfg_euler_step(o["tok"], ld, T, Npix, C, cfg, 5.0, o["x"], o["c_out"], o["v"][0], o["v"][1], out, c_skip=cs)
        torch.cuda.synchronize()
        res[name] = out
    assert torch.equal(res["eps"], res["one"])
    # the general form against the reference's torch ops on the device (each op rounded on its own)
    E_ = o["tok"][:, :C].view(2, T, Npix, C).permute(0, 1, 3, 2)
    D = E_ * o["c_out"].view(T, 1, 1) + o["x"] * skip.view(T, 1, 1)
    D = D[0] + 5.0 * (D[1] - D[0]) if cfg else D[0]
    sg, nx = o["v"][0].view(T, 1, 1), o["v"][1].view(T, 1, 1)
    want = o["x"] + (nx - sg) * ((o["x"] - D) / sg)
    print(f"euler skip entry vs torch ops on the device: max abs {(res['skip'] - want).abs().max().item():.3e}, "
          f"bitwise {torch.equal(res['skip'], want)}")
    assert torch.allclose(res["skip"], want, atol=2e-5, rtol=1e-5)       # the project's bound for these updates


def test_skip_entries_refuse_null_c_skip_and_a_short_struct():
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
    assert lib.pnc_cfg_sampler_step_skip(ctypes.byref(p), sig.data_ptr(), stream) == -3        # PNC_EABI
    p.struct_bytes = ctypes.sizeof(hip.SamplerStepParams)
    assert lib.pnc_cfg_sampler_step_skip(ctypes.byref(p), None, stream) == -1                  # PNC_EINVAL: NULL is not "1"
    assert lib.pnc_cfg_euler_step_skip(eps.data_ptr(), C, T, Npix, C, 0, 0.0, x.data_ptr(), None, sig.data_ptr(), sig.data_ptr(),
                                       sig.data_ptr(), out.data_ptr(), stream) == -1
    assert lib.pnc_cfg_sampler_step_skip(ctypes.byref(p), sig.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, x) and torch.equal(d, x)                             # eps 0, x 0: denoised = 0, d = 0, x + 0


def test_two_step_v_schedule_at_the_config3_shape():
    w, _, kw = product_network("full", DEV)
    inp = step_inputs("full", kw, DEV)
    T = kw["num_frames"]
    c = {"crossattn": inp["crossattn"][1:2], "concat": inp["concat"][T:], "cond_feat": inp["cond_feat"][T:]}
    uc = {"crossattn": inp["crossattn"][0:1], "concat": inp["concat"][:T], "cond_feat": inp["cond_feat"][:T]}
    x0 = inp["x"][T:].clone()
    out = {}
    for fused in (False, True):
        den, smp = make("v_quantised", "euler", 2, DEV)
        smp.fuse = fused
        with torch.no_grad():
            out[fused] = smp(S.BoundDenoiser(den, w), x0.clone(), c, uc, network=w if fused else None)
        torch.cuda.synchronize()
    d = (out[True] - out[False]).abs().max().item()
    print(f"VScaling, Euler, 2 steps at {tuple(x0.shape)}: fused + hoisted vs plain max {d:.3e}")
    assert torch.isfinite(out[True]).all() and d <= 2e-5
