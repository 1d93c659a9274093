"""Denoiser parameterisations (v-prediction, EDM, continuous c_noise) on the CPU: the mirrors of panacea_amd.sampling against
the reference's own Denoiser / DiscreteDenoiser / VScaling / EDMScaling / EDMDiscretization (tests/golden/denoisers*.npz,
tools/gen_golden_denoisers.py), plain on torch and fused on the emulation of the general-skip exit kernels
(tests/emu.py)."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import emu
from denoiser_cases import CASES, EDM_SCHEDULES, P, SAMPLERS, SCALINGS, TINY_SAMPLERS, make, sampler_config
from sampler_cases import FakeTokenNetwork, fake_inputs, fake_network, golden, inject_noise
from panacea_amd import engine as E, hip, sampling as S

G = golden("denoisers.npz")
GT = golden("denoisers_tiny_net.npz")
TOL = float(GT["tol_rel"])
NEW_SYMBOLS = ("pnc_timestep_embedding_f32", "pnc_cfg_euler_step_skip", "pnc_cfg_sampler_step_skip")


@pytest.fixture
def emu_backend():
    with E.use_backend(emu):
        yield


# ---- mirrors against the reference's numbers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EDM_SCHEDULES))
def test_edm_discretization_gives_the_reference_sigmas(name):
    kw, n = EDM_SCHEDULES[name]
    disc = S.EDMDiscretization(**kw)
    assert np.array_equal(disc(n).numpy(), G[f"edm_sigmas.{name}"])
    assert np.array_equal(disc(n, do_append_zero=False, flip=True).numpy(), G[f"edm_sigmas.{name}.flipped_no_zero"])
    assert disc(n)[-1] == 0.0 and len(disc(n)) == n + 1


@pytest.mark.parametrize("name", sorted(SCALINGS))
def test_scaling_coefficients_are_the_reference_bits(name):
    cls, kw = SCALINGS[name]
    sigma = torch.from_numpy(G["scaling.sigma"])
    coeffs = getattr(S, cls)(**kw)(sigma)
    for k, v in zip(("c_skip", "c_out", "c_in", "c_noise"), coeffs):
        assert v.dtype == torch.float32 and np.array_equal(v.numpy(), G[f"scaling.{name}.{k}"]), (name, k)


def test_the_table_of_a_discrete_denoiser_follows_its_options():
    """do_append_zero / flip of DiscreteDenoiser (denoiser.py:38-45) are real options of the mirror"""
    base = S.DiscreteDenoiser()
    up = S.DiscreteDenoiser(flip=False)
    assert torch.equal(up.sigmas, torch.flip(base.sigmas, (0,)))
    z = S.DiscreteDenoiser(do_append_zero=True, flip=False)
    assert len(z.sigmas) == 1001 and z.sigmas[-1] == 0 and torch.equal(z.sigmas[:-1], up.sigmas)
    # the index the network is handed follows the table's order
    s = base.sigmas[[10, 500]]
    assert base.sigma_to_idx(s).tolist() == [10, 500] and up.sigma_to_idx(s).tolist() == [989, 499]


# ---- config builders ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_denoiser_from_config_builds_every_case(case):
    cfg, _, den_cls, scaling_cls, float_c_noise = CASES[case]
    den = S.denoiser_from_config(cfg)
    assert type(den) is den_cls and type(den.scaling) is scaling_cls
    c_noise = den.coefficients(torch.tensor([1.0, 3.0]))[3]
    assert c_noise.is_floating_point() == float_c_noise
    if den_cls is S.DiscreteDenoiser:
        assert den.quantize_c_noise == (not float_c_noise) and den.sigmas.shape == (1000,)


def test_denoiser_from_config_defaults_and_options():
    assert type(S.denoiser_from_config(None)) is S.DiscreteDenoiser
    d = S.denoiser_from_config({"target": P + "denoiser.DiscreteDenoiser",
                                "params": {"num_idx": 50, "do_append_zero": True, "flip": False,
                                           "weighting_config": {"target": P + "denoiser_weighting.NoSuchWeightingIsFine"},
                                           "scaling_config": {"target": P + "denoiser_scaling.EDMScaling", "params": {"sigma_data": 1.0}},
                                           "discretization_config": {"target": P + "discretizer.EDMDiscretization",
                                                                     "params": {"sigma_max": 20.0}}}})
    assert d.scaling.sigma_data == 1.0 and d.sigmas.shape == (51,) and d.sigmas[-1] == 0 and d.sigmas[0] == d.sigmas[:-1].max()
    assert isinstance(d.scaling, S.EDMScaling) and d.quantize_c_noise


def test_unknown_targets_raise_and_name_what_is_supported():
    with pytest.raises(NotImplementedError, match="DiscreteDenoiser"):
        S.denoiser_from_config({"target": P + "denoiser.NoSuchDenoiser"})
    with pytest.raises(NotImplementedError, match="VScaling"):
        S.denoiser_from_config({"target": P + "denoiser.Denoiser", "params": {"scaling_config": {"target": P + "denoiser_scaling.Nope"}}})
    with pytest.raises(NotImplementedError, match="EDMDiscretization"):
        S.denoiser_from_config({"target": P + "denoiser.DiscreteDenoiser",
                                "params": {"num_idx": 10, "discretization_config": {"target": P + "discretizer.Nope"}}})
    with pytest.raises(NotImplementedError, match="EDMDiscretization"):
        S.from_config({"target": P + "sampling.EulerEDMSampler", "params": {"discretization_config": {"target": "other.Discretization"}}})


@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
def test_from_config_accepts_the_edm_discretization(sampler):
    smp = S.from_config(sampler_config("edm_continuous", sampler, 7), device="cpu")
    assert type(smp).__name__ == SAMPLERS[sampler][0] and isinstance(smp.discretization, S.EDMDiscretization)
    assert np.array_equal(smp.sigmas().numpy(), S.EDMDiscretization()(7).numpy()) and abs(smp.host_sigmas()[0] - 80.0) < 1e-3
    custom = sampler_config("edm_continuous", sampler, 7)
    custom["params"]["discretization_config"] = {"target": P + "discretizer.EDMDiscretization", "params": {"sigma_max": 20.0, "rho": 5.0}}
    d = S.from_config(custom, device="cpu").discretization
    assert (d.sigma_min, d.sigma_max, d.rho) == (0.02, 20.0, 5.0)


# ---- fake-network trajectories ------------------------------------------------------------------------------------------------
def _check_c_noise(seen, key):
    want = G[key + ".c_noise"]
    got = torch.stack(seen)[:, 0].numpy()
    assert got.dtype == want.dtype, (got.dtype, want.dtype)            # int64 where the reference quantises, float32 where not
    assert np.array_equal(got, want)                                    # exact: nothing snaps or truncates a float c_noise


@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("n", [3, 25])
def test_mirrors_reproduce_the_reference_plain(case, sampler, n):
    key = f"{case}.{sampler}.{n}"
    x0, c, uc = fake_inputs()
    assert np.array_equal(x0.numpy(), G["x0"])
    den, smp = make(case, sampler, n)
    seen = []

    def net(x, t, cc):
        seen.append(t.clone())
        return fake_network(x, t, cc)
    used = inject_noise(smp, G[key + ".noise"])
    with torch.no_grad():
        xs = smp(lambda inp, sigma, cc: den(net, inp, sigma, cc), x0.clone(), c, uc)
    _check_c_noise(seen, key)
    assert used() == len(G[key + ".noise"])
    assert np.allclose(xs.numpy(), G[key + ".x_final"], atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize("sampler", sorted(SAMPLERS))
@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("n", [3, 25])
def test_fused_loop_replays_the_reference_on_the_emulation(case, sampler, n, emu_backend, monkeypatch):
    """the fused device loop: eps tokens of the stand-in network + one exit kernel per network evaluation, c_skip handed over
    exactly when the scaling is not EpsScaling"""
    key = f"{case}.{sampler}.{n}"
    x0, c, uc = fake_inputs()
    den, smp = make(case, sampler, n)
    net = FakeTokenNetwork()
    bd = S.BoundDenoiser(den, net)
    assert smp._fusable_network(bd, c)
    skips = []
    for fn in ("cfg_euler_step", "cfg_sampler_step"):
        def spy(*a, _fn=getattr(emu, fn), **k):
            skips.append(k.get("c_skip") is not None)
            return _fn(*a, **k)
        monkeypatch.setattr(emu, fn, spy)
    inject_noise(smp, G[key + ".noise"])
    sig, sig_f = smp.sigmas(), smp.host_sigmas()
    x = x0 * torch.sqrt(1.0 + sig[0] ** 2.0)
    s_in = x.new_ones([x.shape[0]])
    with torch.no_grad():
        state = smp._state(x)
        for form, sv, draw in smp._steps(sig, sig_f, s_in):
            if draw:
                sv["noise"] = smp.noise_sampler(x)
            x = smp._device_step(form, sv, x, bd, c, uc, state)
    _check_c_noise(net.seen, key)
    assert len(skips) == len(net.seen) and all(s == (not isinstance(den.scaling, S.EpsScaling)) for s in skips)
    assert np.allclose(x.numpy(), G[key + ".x_final"], atol=2e-5, rtol=1e-5)


# ---- tiny network on the emulation --------------------------------------------------------------------------------------------
def _tiny(kw):
    from helpers import step_inputs
    inp = step_inputs("tiny", kw)
    T = kw["num_frames"]
    c = {"crossattn": inp["crossattn"][1:2], "concat": inp["concat"][T:], "cond_feat": inp["cond_feat"][T:]}
    uc = {"crossattn": inp["crossattn"][0:1], "concat": inp["concat"][:T], "cond_feat": inp["cond_feat"][:T]}
    x0 = inp["x"][T:].clone()
    assert np.array_equal(x0.numpy(), GT["x0"])
    return x0, c, uc


@pytest.mark.parametrize("sampler", TINY_SAMPLERS)
@pytest.mark.parametrize("case", sorted(CASES))
def test_tiny_net_plain_fused_hoisted_on_the_emulation(case, sampler, emu_backend):
    """on the tiny product network (emulated kernels): plain, fused and fused + hoisted are each within tol_rel of the reference's
    denoiser + sampler around the reference network at every step, and fused == plain bit for bit"""
    from helpers import product_network
    w, _, kw = product_network("tiny")
    x0, c, uc = _tiny(kw)
    key = f"{case}.{sampler}"
    ref = torch.from_numpy(GT[key + ".x_steps"])
    runs = {}
    for mode in ("plain", "fused", "fused+hoisted"):
        den, smp = make(case, sampler, int(GT["steps"]), scale=float(GT["cfg_scale"]))
        bd = S.BoundDenoiser(den, w)
        xs = []
        rec = lambda i, x: xs.append(x.clone())              # noqa: E731
        with torch.no_grad():
            if mode == "plain":
                smp.fuse = False
                smp(bd, x0.clone(), c, uc, callback=rec)
            else:
                cc, uu = S.hoist_invariants(w, smp.guider, c, uc) if mode == "fused+hoisted" else (c, uc)
                sig, sig_f = smp.sigmas(), smp.host_sigmas()
                x = x0 * torch.sqrt(1.0 + sig[0] ** 2.0)
                s_in = x.new_ones([x.shape[0]])
                state = smp._state(x)
                for i, (form, sv, _) in enumerate(smp._steps(sig, sig_f, s_in)):
                    x = smp._device_step(form, sv, x, bd, cc, uu, state)
                    rec(i, x)
        runs[mode] = torch.stack(xs)
        errs = [((a - b).abs().max() / b.abs().max()).item() for a, b in zip(runs[mode], ref)]
        print(f"{key} {mode}: per-step error / max|x| {['%.2e' % e for e in errs]}")
        assert max(errs) <= TOL, (key, mode, errs)
    assert torch.equal(runs["plain"], runs["fused"]) and torch.equal(runs["fused"], runs["fused+hoisted"])


# ---- the emulated embedding ---------------------------------------------------------------------------------------------------
def test_timestep_embedding_of_floats_is_not_truncated(emu_backend):
    from panacea_amd.nn.util import timestep_embedding
    dim = 320
    freqs = E.timestep_freqs(dim, torch.device("cpu"))
    t = torch.tensor([1.09551, 0.63492, 0.00806, -0.97801, 14.6146, 0.25, 999.5], dtype=torch.float32)
    emb = timestep_embedding(t, dim)
    args = t[:, None] * freqs[None]
    assert torch.equal(emb, torch.cat([torch.cos(args), torch.sin(args)], dim=-1))
    assert not torch.equal(emb, timestep_embedding(t.to(torch.int64), dim))          # what truncation would give
    ti = torch.tensor([0, 1, 39, 249, 999], dtype=torch.int64)
    for ft in (torch.float32, torch.float64, torch.float16):
        assert torch.equal(timestep_embedding(ti.to(ft), dim), timestep_embedding(ti, dim))
    assert torch.equal(timestep_embedding(ti.to(torch.int32), dim), timestep_embedding(ti, dim))


def test_the_network_embeds_the_float_timestep_it_is_given(emu_backend):
    """through UNetModel3D._time_embedding / ControlNet3D / denoise: a float c_noise changes eps, and differs from its truncation"""
    from helpers import product_network, step_inputs
    w, _, kw = product_network("tiny")
    inp = step_inputs("tiny", kw)
    F = inp["x"].shape[0]
    cond = {"crossattn": inp["crossattn"], "concat": inp["concat"], "cond_feat": inp["cond_feat"]}
    with torch.no_grad():
        out = {name: w(inp["x"], t, cond) for name, t in
               (("0.8", torch.full((F,), 0.8)), ("0.0", torch.full((F,), 0.0)), ("0", torch.zeros(F, dtype=torch.int64)),
                ("1.0", torch.full((F,), 1.0)), ("1", torch.ones(F, dtype=torch.int64)))}
    assert torch.equal(out["0.0"], out["0"]) and torch.equal(out["1.0"], out["1"])
    assert not torch.equal(out["0.8"], out["0"]) and not torch.equal(out["0.8"], out["1"])


# ---- header and binding -------------------------------------------------------------------------------------------------------
def test_header_and_binding_agree_on_the_new_entries(tmp_path):
    syms = hip.header_symbols()
    for s in NEW_SYMBOLS:
        assert s in syms and s in hip._SIGNATURES, s
    assert sorted(hip._SIGNATURES) == syms
    lib = hip.load()
    for s in NEW_SYMBOLS:
        assert hasattr(lib, s)
    # existing structs keep their size (ABI 8): the sizes of the parent commit as gcc lays the header out
    want = {"PncGemmParams": ctypes.sizeof(hip.GemmParams), "PncAttnParams": ctypes.sizeof(hip.AttnParams),
            "PncAttnSplitParams": ctypes.sizeof(hip.AttnSplitParams), "PncSamplerStepParams": ctypes.sizeof(hip.SamplerStepParams)}
    assert want["PncSamplerStepParams"] == 184
    src = ['#include <stdio.h>', f'#include "{hip.HEADER}"', 'int main(void) {']
    src += [f'printf("{n} %zu\\n", sizeof({n}));' for n in want]
    pointers = ['int (*e)(const float*, int, int, const float*, float*, void*) = pnc_timestep_embedding_f32; (void)e;',
            'int (*s)(const PncSamplerStepParams*, const float*, void*) = pnc_cfg_sampler_step_skip; (void)s;',
            'int (*u)(const float*, int, int, int, int, int, float, const float*, const float*, const float*, const float*, '
            'const float*, float*, void*) = pnc_cfg_euler_step_skip; (void)u;']
    end = ['printf("abi %d\\n", PNC_ABI_VERSION); return 0; }']
    c = tmp_path / "denoiser_abi.c"
    c.write_text("\n".join(src + pointers + end))
    obj = tmp_path / "denoiser_abi.o"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-c", str(c), "-o", str(obj)])     # the header compiles as C
    # sizes: an executable that does not link the library (no function pointers)
    c2 = tmp_path / "denoiser_sizes.c"
    c2.write_text("\n".join(src + end))
    exe = tmp_path / "denoiser_sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(c2), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    for n, sz in want.items():
        assert int(got[n]) == sz, n
    assert int(got["abi"]) == hip.ABI_VERSION == 8


def test_skip_entries_validate_their_arguments_without_gpu():
    lib = hip.load()
    p = hip.SamplerStepParams()
    assert lib.pnc_cfg_sampler_step_skip(ctypes.byref(p), 16, None) == -3       # PNC_EABI: struct_bytes not set
    p.struct_bytes = ctypes.sizeof(hip.SamplerStepParams) - 8
    assert lib.pnc_cfg_sampler_step_skip(ctypes.byref(p), 16, None) == -3       # a shorter struct of another header
    p.struct_bytes = ctypes.sizeof(hip.SamplerStepParams)
    p.eps_tok = p.x = p.c_out = p.out = p.out_aux = 16
    p.v[0] = p.v[1] = 16
    p.ld, p.T, p.Npix, p.C, p.mode = 4, 1, 1, 4, hip.SAMPLER_HEUN1
    assert lib.pnc_cfg_sampler_step_skip(ctypes.byref(p), None, None) == -1     # PNC_EINVAL: a NULL c_skip is not "1"
    p.mode = 7
    assert lib.pnc_cfg_sampler_step_skip(ctypes.byref(p), 16, None) == -1       # unknown mode
    assert lib.pnc_cfg_euler_step_skip(16, 4, 1, 1, 4, 1, 5.0, 16, None, 16, 16, 16, 16, None) == -1     # NULL c_skip
    assert lib.pnc_cfg_euler_step_skip(16, 2, 1, 1, 4, 1, 5.0, 16, 16, 16, 16, 16, 16, None) == -1       # ld < C
    assert lib.pnc_timestep_embedding_f32(None, 1, 320, 16, 16, None) == -1
    assert lib.pnc_timestep_embedding_f32(16, 1, 1, 16, 16, None) == -1


# ---- ShardedCFG ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(CASES))
def test_sharded_cfg_refuses_the_new_parameterisations(case):
    class Half(S.VanillaCFG):
        half, group = 0, None
    x0, c, uc = fake_inputs()
    den, smp = make(case, "euler", 3)
    smp.guider = Half(5.0)
    bd = S.BoundDenoiser(den, FakeTokenNetwork())
    with pytest.raises(NotImplementedError, match="ShardedCFG"):
        smp(bd, x0, c, uc)
    with pytest.raises(NotImplementedError, match="ShardedCFG"):
        smp._fused_eps(torch.ones(2), bd, x0, c, uc)
    # the shipped parameterisation passes the check
    from panacea_amd.parallel import _refuse_denoiser
    _refuse_denoiser(S.DiscreteDenoiser())
    _refuse_denoiser(None)
    with pytest.raises(NotImplementedError):
        _refuse_denoiser(S.DiscreteDenoiser(quantize_c_noise=False))


# ---- public entry point -------------------------------------------------------------------------------------------------------
def test_sample_frames_selects_the_denoiser(monkeypatch):
    from panacea_amd import pipeline
    got = []

    class Sampler(S.EulerEDMSampler):
        def __call__(self, denoiser, x, cond, uc=None, num_steps=None, network=None, callback=None):
            got.append(denoiser.denoiser)
            return x

    class Decoder:
        def decode(self, z):
            return z
    noise = torch.zeros(2, 4, 4, 12)
    for arg in (None, S.Denoiser(S.EDMScaling()), CASES["v_float"][0]):
        pipeline.sample_frames(object(), Decoder(), {}, {}, noise, sampler=Sampler(3, device="cpu"), denoiser=arg)
    assert type(got[0]) is S.DiscreteDenoiser and isinstance(got[0].scaling, S.EpsScaling) and got[0].quantize_c_noise
    assert type(got[1]) is S.Denoiser and isinstance(got[1].scaling, S.EDMScaling)
    assert type(got[2]) is S.DiscreteDenoiser and isinstance(got[2].scaling, S.VScaling) and not got[2].quantize_c_noise
    with pytest.raises(TypeError):
        pipeline.sample_frames(object(), Decoder(), {}, {}, noise, sampler=Sampler(3, device="cpu"), denoiser=lambda *a: None)
