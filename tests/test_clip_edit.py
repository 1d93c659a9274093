"""Clip editing without a GPU: the per-op reference of pnc_frames_renoise and its two wrong-kernel models (tests/clip_edit_ref.py),
and — on the emulated backend with that reference as its `frames_renoise` (tests/emu_edit.py) — `start_step`, sampling.ClipSource with
kept frames, pipeline.edit_frames and every refusal, on the tiny network (T = 2 frames, latent 8 x 96)."""
import inspect
import shutil
import subprocess
import types

import pytest
import torch

import clip_edit_cases as cc
import clip_edit_ref as ref
import emu
import emu_edit
from panacea_amd import engine as E, hip, pipeline, sampling as S

T = cc.T


@pytest.fixture(scope="module")
def stack():
    return cc.tiny_stack("cpu")


@pytest.fixture(scope="module")
def inputs(stack):
    return cc.tiny_inputs(stack["kw"])


@pytest.fixture(scope="module")
def bd(stack):
    return S.BoundDenoiser(S.DiscreteDenoiser(), stack["net"])


@pytest.fixture()
def calls():
    del emu_edit.CALLS[:]
    return emu_edit.CALLS


# ---- the reference and the wrong kernels --------------------------------------------------------------------------------------------
def test_reference_follows_the_header_on_a_case_worked_by_hand():
    z = torch.tensor([[[1.0, -0.0]], [[3.0, 4.0]], [[5.0, 6.0]], [[7.0, 8.0]]])
    n = torch.tensor([[[0.5, ref.NAN]], [[ref.NAN, 1.0]], [[1.0, -1.0]], [[1.0, 1.0]]])
    x = torch.full((4, 1, 2), 9.0)
    sigma = torch.tensor([0.0, 2.0, 2.0, 2.0])
    keep = torch.tensor([1.0, -0.0, 2.0, ref.NAN])
    out = ref.frames_renoise(z, n, sigma, keep, x)
    assert torch.equal(ref.bits(out), ref.bits(torch.tensor([[[1.0, -0.0]], [[9.0, 9.0]], [[7.0, 4.0]], [[9.0, 9.0]]])))
    every = ref.frames_renoise(z, torch.nan_to_num(n), sigma)
    assert torch.equal(every[1:], torch.tensor([[[3.0, 6.0]], [[7.0, 4.0]], [[9.0, 10.0]]])) and torch.equal(ref.bits(every[0]), ref.bits(z[0]))


def test_the_product_is_rounded_before_the_sum():
    """n = 1 + 2^-23, s = 2^-24 (1 - 2^-24): n * s = 2^-24 (1 + 2^-24 - 2^-47) rounds to 2^-24, half an ulp of z = 1, and the tie goes
    to the even 1.0; the exact z + n * s lies above the tie and a single rounding gives 1 + 2^-23"""
    z, n, s = torch.tensor([[[1.0]]]), torch.tensor([[[1.0 + 2.0 ** -23]]]), torch.tensor([2.0 ** -24 * (1.0 - 2.0 ** -24)])
    assert float(n * s) == 2.0 ** -24 and float(n.double() * s.double()) > 2.0 ** -24
    assert float(ref.frames_renoise(z, n, s)) == 1.0
    assert float(ref.frames_renoise(z, n, s, mutant="fma")) == 1.0 + 2.0 ** -23


@pytest.mark.parametrize("mutant", sorted(ref.MUTANTS))
def test_every_wrong_kernel_changes_bits_on_the_case_list(mutant):
    differing = []
    for shape, variant in ref.cases():
        ops = ref.case(shape, variant)
        args = (ops["z"], ops["noise"], ops["sigma"], ops["keep"], ops["x"])
        want, got = ref.frames_renoise(*args), ref.frames_renoise(*args, mutant=mutant)
        if not torch.equal(ref.bits(want), ref.bits(got)):
            differing.append((shape, variant))
    print(f"{mutant}: differs on {len(differing)} of {len(ref.SHAPES) * len(ref.VARIANTS)} cases")
    if mutant == "fma":                # wherever a frame is renoised: every shape, every variant
        assert {s for s, _ in differing} == set(ref.SHAPES) and {v for _, v in differing} == set(ref.VARIANTS)
    else:                              # wherever the selector holds a negative or a NaN frame: T = 1 (NaN) and T = 16
        assert {(s, v) for s, v in differing} >= {((16, 4, 768), v) for v in ref.VARIANTS[1:]} | {((1, 4, 7), "selector")}
        assert all(v != "keep_null" for _, v in differing)


def test_nan_noise_is_inert_where_sigma_is_zero_or_the_frame_is_not_kept():
    for shape in ref.SHAPES:
        ops = ref.case(shape, "nan_noise")
        assert torch.isnan(ops["noise"]).any()
        out = ref.frames_renoise(ops["z"], ops["noise"], ops["sigma"], ops["keep"], ops["x"])
        assert not torch.isnan(out).any()


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------
def test_abi_stays_8_and_the_binding_is_the_header():
    assert sorted(hip._SIGNATURES) == hip.header_symbols() and "pnc_frames_renoise" in hip._SIGNATURES
    assert hip.ABI_VERSION == 8 and "#define PNC_ABI_VERSION 8" in hip.HEADER.read_text()
    assert hip.load().pnc_abi_version() == 8
    assert len(hip._SIGNATURES["pnc_frames_renoise"][1]) == 10


def test_header_compiles_as_c99():
    cc_ = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc_, "a C compiler is needed to check the header"
    r = subprocess.run([cc_, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", str(hip.HEADER)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_emu_edit_is_emu_plus_the_wrapper_with_the_products_signature():
    assert not hasattr(emu, "frames_renoise")
    names = [n for n in dir(emu) if not n.startswith("__")]
    assert all(getattr(emu_edit, n) is getattr(emu, n) for n in names)
    want = [(p.name, p.kind, p.default) for p in inspect.signature(hip.frames_renoise).parameters.values()]
    got = [(p.name, p.kind, p.default) for p in inspect.signature(emu_edit.frames_renoise).parameters.values()]
    assert got == want


# ---- start_step -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(cc.SAMPLERS))
def test_start_step_composes(name, bd, inputs):
    """cc.composes_exactly states where: every k for the one-step samplers and LMS of order 1; DPM++ 2M at the last step only; LMS of
    order 4 nowhere (a documented difference, asserted as one)"""
    x0, c, uc = inputs
    with E.use_backend(emu_edit):
        cc.check_composition(name, bd, x0, c, uc)


@pytest.mark.parametrize("name", sorted(cc.SAMPLERS))
def test_defaults_are_the_call_without_the_new_arguments(name, bd, inputs, calls):
    x0, c, uc = inputs
    with E.use_backend(emu):                    # the committed backend, which has no frames_renoise: the default path never asks
        a, _ = cc.run(cc.make(name, 2), bd, x0.clone(), c, uc)
        b, _ = cc.run(cc.make(name, 2), bd, x0.clone(), c, uc, start_step=0, source=None)
    assert torch.equal(a, b) and calls == []


def test_start_step_outside_the_schedule_is_refused(bd, inputs):
    x0, c, uc = inputs
    with E.use_backend(_counting(emu_edit)[0]):
        for name in sorted(cc.SAMPLERS):
            for bad in (-1, cc.STEPS, cc.STEPS + 3):
                with pytest.raises(ValueError, match="start_step"):
                    cc.make(name)(bd, x0, c, uc, start_step=bad)
            with pytest.raises(TypeError):
                cc.make(name)(bd, x0, c, uc, start_step=1.0)


# ---- kept frames ------------------------------------------------------------------------------------------------------------------
def _source(inputs, keep, seed=3):
    x0, _, _ = inputs
    g = torch.Generator().manual_seed(seed)
    return S.ClipSource(0.5 * torch.randn(x0.shape, generator=g), torch.randn(x0.shape, generator=g), keep)


@pytest.mark.parametrize("keep", [(0,), (0, 1)], ids=["keep0", "keep01"])
@pytest.mark.parametrize("name", cc.KEEPERS)
def test_kept_frames_arrive_at_z_exactly(name, keep, bd, inputs, calls):
    _, c, uc = inputs
    src = _source(inputs, keep)
    with E.use_backend(emu_edit):
        out, seen = cc.run(cc.make(name, 3), bd, None, c, uc, start_step=1, source=src)
    for t in range(T):
        assert torch.equal(ref.bits(out[t]), ref.bits(src.z[t])) == (t in keep), (name, keep, t)
    assert torch.isfinite(out).all() and sorted(seen) == [1, 2]
    # the start launch keeps every frame, then one launch per step on the step's output; the last one at sigma 0
    kv = tuple(int(t in keep) for t in range(T))
    assert calls == [(None, False), (kv, False), (kv, True)]
    # in between, the kept frames sit on z + sigma_next * noise
    sig = cc.make(name, 3).sigmas()
    mid = src.z + src.noise * sig[2]
    assert all(torch.equal(seen[1][t], mid[t]) for t in keep)


@pytest.mark.parametrize("name", sorted(cc.SAMPLERS))
def test_an_empty_keep_works_everywhere_and_launches_once(name, bd, inputs, calls):
    _, c, uc = inputs
    src = _source(inputs, ())
    smp = cc.make(name, 3)
    with E.use_backend(emu_edit):
        out, _ = cc.run(smp, bd, None, c, uc, start_step=1, source=src)
        assert calls == [(None, False)]
        # the same trajectory from the same start latent handed over as x
        start = src.z + src.noise * smp.sigmas()[1]
        want, _ = cc.run(cc.make(name, 3), bd, start, c, uc, start_step=1)
    assert torch.equal(out, want) and not any(torch.equal(out[t], src.z[t]) for t in range(T))


def test_clip_source_validates_at_construction():
    z, n = torch.zeros(2, 4, 3, 5), torch.zeros(2, 4, 3, 5)
    assert S.ClipSource(z, n, [1, 0]).keep == (0, 1) and S.ClipSource(z, n).keep == ()
    assert S.ClipSource(z, n, (1,)).keep_vector().tolist() == [0.0, 1.0]
    for bad, exc in [((z.half(), n), TypeError), ((z, n.double()), TypeError), ((z.numpy(), n), TypeError), ((z, n, [0.5]), TypeError),
                     ((z[0], n[0]), ValueError), ((z, n[:1]), ValueError), ((z, n, [2]), ValueError), ((z, n, [-1]), ValueError),
                     ((z, n, [0, 0]), ValueError), ((z[:0], n[:0]), ValueError)]:
        with pytest.raises(exc):
            S.ClipSource(*bad)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _counting(module):
    """`module` as a backend namespace with every call counted"""
    calls = []

    def counted(name, fn):
        def run(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return run
    names = [n for n in dir(module) if not n.startswith("_") and isinstance(getattr(module, n), types.FunctionType)]
    return types.SimpleNamespace(**{n: counted(n, getattr(module, n)) for n in names}), calls


def test_samplers_that_do_not_keep_frames_refuse_by_name(bd, inputs):
    _, c, uc = inputs
    src = _source(inputs, (0,))
    be, calls = _counting(emu_edit)
    with E.use_backend(be):
        for name in cc.REFUSERS:
            smp = cc.make(name, 3)
            with pytest.raises(NotImplementedError, match=type(smp).__name__):
                smp(bd, None, c, uc, source=src)
        churned = S.EulerEDMSampler(3, guider=S.VanillaCFG(5.0), device="cpu", s_churn=1.0)
        with pytest.raises(NotImplementedError, match="EulerEDMSampler.*churn"):
            churned(bd, None, c, uc, source=src)
        sharded = S.VanillaCFG(5.0)
        sharded.half, sharded.group = 0, None                       # what parallel.ShardedCFG carries
        with pytest.raises(NotImplementedError, match="ShardedCFG"):
            S.EulerEDMSampler(3, guider=sharded, device="cpu")(bd, None, c, uc, source=src)
        with pytest.raises(TypeError, match="ClipSource"):
            cc.make("euler", 3)(bd, None, c, uc, source=(src.z, src.noise))
    assert calls == []
    # a backend without the capability: refused by name, before anything is launched, kept frames or not
    bare, calls = _counting(emu)
    with E.use_backend(bare):
        for keep in ((), (0,)):
            with pytest.raises(NotImplementedError, match="frames_renoise"):
                cc.make("euler", 3)(bd, None, c, uc, source=_source(inputs, keep), network=bd.network)
    assert calls == []


def test_parallel_sharded_cfg_is_the_guider_the_refusal_means():
    from panacea_amd import parallel
    assert hasattr(parallel, "ShardedCFG") and issubclass(parallel.ShardedCFG, S.VanillaCFG)


# ---- edit_frames ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twins():
    import image_boundary_cases as ib
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(emu_edit, "u8_to_tokens_f16", ib.u8_to_tokens_f16, raising=False)
        mp.setattr(emu_edit, "tokens_to_u8", ib.tokens_to_u8, raising=False)
        yield


def test_edit_start_step():
    f = pipeline.edit_start_step
    assert [f(s, 25) for s in (1.0, 0.6, 0.5, 0.04, 0.01)] == [0, 10, 12, 24, 24] and f(1, 3) == 0 and f(0.2, 3) == 2
    for bad in (0.0, -0.1, 1.01, float("nan"), "0.5", None, True):
        with pytest.raises(ValueError, match="strength"):
            f(bad, 25)


def test_edit_frames_is_the_composition_and_keeps_the_first_stage_latent(stack, inputs, twins, calls):
    x0, c, uc = inputs
    clip, noise = cc.clip_u8(), torch.randn(x0.shape, generator=torch.Generator().manual_seed(9))
    seen = {}
    with E.use_backend(emu_edit):
        out = pipeline.edit_frames(stack["net"], stack["dec"], stack["enc"], clip, c, uc, noise, strength=0.7, keep=(1,), num_steps=3,
                                   sample_posterior=False, callback=lambda i, x: seen.__setitem__(i, x.clone()))
        z = pipeline.SCALE_FACTOR * stack["enc"].encode_u8(clip, sample=False)
        assert sorted(seen) == [0, 1, 2] and pipeline.edit_start_step(0.7, 3) == 0
        assert torch.equal(ref.bits(seen[2][1]), ref.bits(z[1])) and not torch.equal(seen[2][0], z[0])
        assert torch.equal(out, stack["dec"].decode_u8(seen[2] / pipeline.SCALE_FACTOR))
        assert out.shape == clip.shape and out.dtype == torch.uint8
        # by hand: the sampler on a ClipSource
        smp = S.EulerEDMSampler(3, guider=S.VanillaCFG(5.0), device="cpu")
        want = smp(S.BoundDenoiser(S.DiscreteDenoiser(), stack["net"]), None, c, uc, network=stack["net"],
                   source=S.ClipSource(z, noise, (1,)))
        assert torch.equal(want, seen[2])
        # a posterior draw from the generator, a later start
        del calls[:]
        g = torch.Generator().manual_seed(4)
        pipeline.edit_frames(stack["net"], stack["dec"], stack["enc"], clip, c, uc, noise, strength=0.4, num_steps=3, generator=g,
                             callback=lambda i, x: seen.__setitem__(10 + i, x.clone()))
        assert sorted(k for k in seen if k >= 10) == [11, 12] and calls == [(None, False)]


def test_edit_frames_refuses_before_the_first_backend_call(stack, inputs, twins):
    x0, c, uc = inputs
    net, dec, enc = stack["net"], stack["dec"], stack["enc"]
    clip, noise = cc.clip_u8(), torch.randn(x0.shape, generator=torch.Generator().manual_seed(9))
    no_dec, no_enc = types.SimpleNamespace(decode=dec.decode), types.SimpleNamespace(encode=enc.encode, encode_sparse_u8=enc.encode_sparse_u8)

    def edit(net=net, dec=dec, enc=enc, clip=clip, noise=noise, **kw):
        return pipeline.edit_frames(net, dec, enc, clip, c, uc, noise, **{"num_steps": 3, **kw})
    be, calls = _counting(emu_edit)
    assert hasattr(be, "frames_renoise") and hasattr(be, "tokens_to_u8")
    cases = [(dict(dec=no_dec), TypeError, "decode_u8"), (dict(enc=no_enc), TypeError, "encode_u8"),
             (dict(noise=noise[0]), ValueError, "noise"), (dict(noise=noise.numpy()), ValueError, "noise"),
             (dict(noise=torch.cat([noise, noise[:1]])), ValueError, "num_frames"),
             (dict(clip=clip.float()), ValueError, "frames_u8"), (dict(clip=clip[0]), ValueError, "frames_u8"),
             (dict(clip=clip[:1]), ValueError, "frames_u8"), (dict(clip=clip[:, :-1].contiguous()), ValueError, "frames_u8"),
             (dict(clip=clip[..., :2].contiguous()), ValueError, "frames_u8"), (dict(clip=clip.numpy()), ValueError, "frames_u8"),
             (dict(strength=0.0), ValueError, "strength"), (dict(strength=1.5), ValueError, "strength"), (dict(strength=-0.2), ValueError, "strength"),
             (dict(keep=(T,)), ValueError, "keep"), (dict(keep=(-1,)), ValueError, "keep"), (dict(keep=(0, 0)), ValueError, "keep"),
             (dict(keep=(0.5,)), ValueError, "keep"),
             (dict(keep=(0,), sampler=S.HeunEDMSampler(3, guider=S.VanillaCFG(5.0), device="cpu")), NotImplementedError, "HeunEDMSampler"),
             (dict(keep=(0,), sampler=S.EulerAncestralSampler(3, guider=S.VanillaCFG(5.0), device="cpu")), NotImplementedError, "EulerAncestralSampler"),
             (dict(keep=(0,), sampler=S.DPMPP2SAncestralSampler(3, guider=S.VanillaCFG(5.0), device="cpu")), NotImplementedError, "DPMPP2SAncestralSampler"),
             (dict(keep=(0,), sampler=S.EulerEDMSampler(3, guider=S.VanillaCFG(5.0), device="cpu", s_churn=1.0)), NotImplementedError, "churn")]
    with E.use_backend(be):
        for kw, exc, match in cases:
            with pytest.raises(exc, match=match):
                edit(**kw)
            assert calls == [], (kw.keys(), calls[:3])
        for where in ("diffusion_model", "controlnet"):
            for attr in ("frame_shard", "view_shard"):
                m = net.diffusion_model if where == "diffusion_model" else net.diffusion_model.controlnet
                setattr(m, attr, object())
                try:
                    with pytest.raises(NotImplementedError, match="one device"):
                        edit()
                finally:
                    delattr(m, attr)
                assert getattr(m, attr) is None and calls == []
    # backends without one of the three capabilities: each refused by name
    for missing in ("frames_renoise", "tokens_to_u8", "u8_to_tokens_f16"):
        bare, calls = _counting(emu_edit)
        delattr(bare, missing)
        with E.use_backend(bare):
            with pytest.raises(NotImplementedError, match=missing):
                edit()
        assert calls == []
