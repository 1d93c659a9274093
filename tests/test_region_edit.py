"""Region editing without a GPU: the per-op references of the three entries and their wrong-kernel models
(tests/region_edit_ref.py), and — on the emulated backend with those references as its wrappers (tests/emu_region.py) —
sampling.ClipSource with a mask, pipeline.edit_frames with `keep_mask_u8`, the mask helpers, every refusal and the tool's argument
errors, on the tiny network (T = 2 frames, latent 8 x 96, frames 16 x 192: six views of 32 columns)."""
import inspect
import shutil
import subprocess
import sys
import types
from pathlib import Path

import pytest
import torch

import clip_edit_cases as cc
import clip_edit_ref as cref
import emu
import emu_edit
import emu_region
import region_edit_ref as ref
from panacea_amd import engine as E, hip, image, pipeline, sampling as S

T, LH, LW, H, W = cc.T, cc.LH, cc.LW, cc.H, cc.W
ROOT = Path(__file__).resolve().parent.parent
MASKED = ("latent_renoise_masked", True)          # the put-back's entry in CALLS: in place on x, then whether a sigma is 0


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
    del emu_region.CALLS[:]
    return emu_region.CALLS


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


# ---- the references and the wrong kernels ------------------------------------------------------------------------------------------
def test_references_follow_the_header_on_cases_worked_by_hand():
    z = torch.tensor([[[1.0, -0.0, 3.0], [4.0, 5.0, 6.0]], [[7.0, 8.0, 9.0], [10.0, 11.0, 12.0]]])
    n = torch.tensor([[[ref.NAN, ref.NAN, ref.NAN], [1.0, 1.0, 1.0]], [[1.0, -1.0, ref.NAN], [0.5, 2.0, ref.NAN]]])
    x = torch.full((2, 2, 3), 99.0)
    x[1, :, 0] = ref.NAN
    sigma = torch.tensor([-0.0, 2.0])
    mask = torch.tensor([[1.0, 1e-45, -0.0], [0.5, float("inf"), ref.NAN]])
    out = ref.latent_renoise_masked(z, n, sigma, mask, x)
    want = torch.tensor([[[1.0, -0.0, 99.0], [4.0, 5.0, 99.0]], [[9.0, 6.0, 99.0], [11.0, 15.0, 99.0]]])
    assert torch.equal(ref.bits(out), ref.bits(want))
    m = torch.tensor([[[255, 1, 0, 7], [128, 2, 9, 9], [1, 1, 1, 1], [1, 1, 1, 0]]], dtype=torch.uint8)
    assert ref.mask_pool_u8(m, 2).tolist() == [[[1.0, 0.0], [1.0, 0.0]]] and ref.mask_pool_u8(m, 4).tolist() == [[[0.0]]]
    assert ref.mask_pool_u8(m, 1).tolist() == (m != 0).float().tolist()
    src, gen = torch.tensor([[1, 2, 3], [4, 5, 6]], dtype=torch.uint8), torch.tensor([[7, 8, 9], [10, 11, 12]], dtype=torch.uint8)
    assert ref.u8_select(src, gen, torch.tensor([0, 128], dtype=torch.uint8)).tolist() == [[7, 8, 9], [4, 5, 6]]


def _differing(mutant):
    kind = ref.MUTANTS[mutant][0]
    out = []
    if kind == "renoise":
        for shape, pattern, variant in ref.renoise_cases():
            o = ref.renoise_case(shape, pattern, variant)
            args = (o["z"], o["noise"], o["sigma"], o["mask"], o["x"])
            if not torch.equal(ref.bits(ref.latent_renoise_masked(*args)), ref.bits(ref.latent_renoise_masked(*args, mutant=mutant))):
                out.append((shape, pattern, variant))
    elif kind == "pool":
        for case in ref.POOL_CASES:
            for fill in ref.POOL_FILLS:
                m = ref.pool_mask(case, fill)
                if not torch.equal(ref.mask_pool_u8(m, case[3]), ref.mask_pool_u8(m, case[3], mutant=mutant)):
                    out.append((case, fill))
    else:
        for case in ref.SELECT_CASES:
            ops = ref.select_case(case)
            if not torch.equal(ref.u8_select(*ops), ref.u8_select(*ops, mutant=mutant)):
                out.append(case)
    return out


@pytest.mark.parametrize("mutant", sorted(ref.MUTANTS))
def test_every_wrong_kernel_changes_bits_on_the_case_list(mutant):
    differing = _differing(mutant)
    print(f"{mutant}: differs on {len(differing)} cases")
    assert differing
    if mutant == "fma":                       # wherever something is renoised: every shape
        assert {d[0] for d in differing} == set(ref.RENOISE_SHAPES) and all(d[1] != "none" for d in differing)
    if mutant == "mask_nonzero":              # only where the selector holds negative or NaN values
        assert {d[1] for d in differing} == {"selector"}
    if mutant == "mask_by_element":           # plane c reads the row of frame t + c: it shows where the frames' rows differ
        assert ((2, 3, 1025), "alternate", "plain") in differing and ((3, 4, 100), "band", "plain") in differing
        assert all(d[0][0] > 1 and d[1] not in ("all", "none", "last_pixel") for d in differing)
    if mutant == "x_blend":                   # NaN comes through the product with 0 (and -0.0 + 0.0 * x loses its sign at sigma 0)
        assert {(s, m, "nan_inert") for s in ref.RENOISE_SHAPES for m in ref.MASKS} <= set(differing)
    if mutant == "pool_skip_last_row":
        assert {d[1] for d in differing} >= {"hole_bl"} and all(d[1] != "hole_tl" or d[0][3] == 1 for d in differing)
    if mutant == "pool_skip_last_col":
        assert {d[1] for d in differing} >= {"hole_tr"}
    if mutant == "select_per_byte":           # one channel: a byte is a pixel
        assert (33, 1) not in differing and (231, 3) in differing


def test_operands_that_are_not_selected_are_inert():
    for shape in ref.RENOISE_SHAPES:
        for pattern in ref.MASKS:
            o = ref.renoise_case(shape, pattern, "nan_inert")
            assert torch.isnan(o["noise"]).any() or pattern == "all"
            out = ref.latent_renoise_masked(o["z"], o["noise"], o["sigma"], o["mask"], o["x"])
            assert not torch.isnan(out).any(), (shape, pattern)


@pytest.mark.parametrize("shape", ref.RENOISE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_a_frame_uniform_mask_is_frames_renoise(shape):
    Tn, C, Npix = shape
    for variant in ("selector", "sigma_zero", "nan_noise"):
        o = cref.case(shape, variant)
        mask = o["keep"][:, None].expand(Tn, Npix).contiguous()
        got = ref.latent_renoise_masked(o["z"], o["noise"], o["sigma"], mask, o["x"])
        want = cref.frames_renoise(o["z"], o["noise"], o["sigma"], o["keep"], o["x"])
        assert torch.equal(ref.bits(got), ref.bits(want)), (shape, variant)


# ---- the ABI and the emulated wrappers ---------------------------------------------------------------------------------------------
NEW = ("latent_renoise_masked", "mask_pool_u8", "u8_select")


def test_abi_stays_8_and_the_binding_is_the_header():
    assert sorted(hip._SIGNATURES) == hip.header_symbols() and all("pnc_" + n in hip._SIGNATURES for n in NEW)
    assert hip.ABI_VERSION == 8 and "#define PNC_ABI_VERSION 8" in hip.HEADER.read_text()
    assert hip.load().pnc_abi_version() == 8
    assert [len(hip._SIGNATURES["pnc_" + n][1]) for n in NEW] == [10, 7, 7]
    assert all(hasattr(hip.load(), "pnc_" + n) for n in NEW)


def test_header_compiles_as_c99():
    cc_ = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    assert cc_, "a C compiler is needed to check the header"
    r = subprocess.run([cc_, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", str(hip.HEADER)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_emu_region_is_emu_edit_plus_the_wrappers_with_the_products_signatures():
    assert not any(hasattr(emu_edit, n) or hasattr(emu, n) for n in NEW)
    names = [n for n in dir(emu_edit) if not n.startswith("__")]
    assert all(getattr(emu_region, n) is getattr(emu_edit, n) for n in names)
    for n in NEW:
        want = [(p.name, p.kind, p.default) for p in inspect.signature(getattr(hip, n)).parameters.values()]
        got = [(p.name, p.kind, p.default) for p in inspect.signature(getattr(emu_region, n)).parameters.values()]
        assert got == want, n


# ---- ClipSource with a mask --------------------------------------------------------------------------------------------------------
def _band_mask(view=1):
    """(T, LH, LW) bool: the latent columns of one of six views"""
    m = torch.zeros(T, LH, LW, dtype=torch.bool)
    m[:, :, view * (LW // 6):(view + 1) * (LW // 6)] = True
    return m


def _source(inputs, keep=(), mask=None, seed=3):
    x0, _, _ = inputs
    g = torch.Generator().manual_seed(seed)
    return S.ClipSource(0.5 * torch.randn(x0.shape, generator=g), torch.randn(x0.shape, generator=g), keep, mask=mask)


def test_the_selector_is_the_union_of_the_mask_and_the_kept_frames(inputs):
    band = _band_mask()
    for mask in (band, band.to(torch.uint8) * 7, torch.where(band, 0.25, -1.0), torch.where(band, float("inf"), ref.NAN)):
        src = _source(inputs, (1,), mask)
        want = band.clone()
        want[1] = True
        assert src.selector.dtype == torch.float32 and src.selector.is_contiguous() and torch.equal(src.selector, want.float())
        assert src.keep == (1,) and src.keep_vector().tolist() == [0.0, 1.0] and src.keeps
    plain = _source(inputs, ())
    assert plain.selector is None and not plain.keeps and _source(inputs, (), torch.zeros(T, LH, LW)).keeps


@pytest.mark.parametrize("name", cc.KEEPERS)
def test_kept_elements_arrive_at_z_exactly(name, bd, inputs, calls):
    """a mask that keeps one column band, and frame 1 kept whole"""
    _, c, uc = inputs
    src = _source(inputs, (1,), _band_mask())
    sel = src.selector.bool()[:, None].expand_as(src.z)
    with E.use_backend(emu_region):
        out, seen = cc.run(cc.make(name, 3), bd, None, c, uc, start_step=1, source=src)
    assert torch.isfinite(out).all() and sorted(seen) == [1, 2]
    assert torch.equal(ref.bits(out)[sel], ref.bits(src.z)[sel])
    for t in range(T):                      # every frame with elements outside the selector has moved somewhere outside it
        if not sel[t].all():
            assert (ref.bits(out[t])[~sel[t]] != ref.bits(src.z[t])[~sel[t]]).any(), (name, t)
    assert sel[1].all() and not sel[0].all()
    # one frames_renoise start that keeps every frame, then one masked launch per step, in place; the last one at sigma 0
    assert calls == [(None, False), MASKED + (False,), MASKED + (True,)]
    mid = src.z + src.noise * cc.make(name, 3).sigmas()[2]
    assert torch.equal(ref.bits(seen[1])[sel], ref.bits(mid)[sel])


@pytest.mark.parametrize("name", sorted(cc.SAMPLERS))
def test_mask_none_is_the_call_without_the_argument(name, bd, inputs, calls):
    _, c, uc = inputs
    keep = (0,) if name in cc.KEEPERS else ()
    g = torch.Generator().manual_seed(3)
    z, noise = 0.5 * torch.randn(inputs[0].shape, generator=g), torch.randn(inputs[0].shape, generator=g)
    be, looked = _counting(emu_edit)          # has frames_renoise and none of the new wrappers: they are never looked up
    assert not any(hasattr(be, n) for n in NEW)
    with E.use_backend(be):
        a, _ = cc.run(cc.make(name, 3), bd, None, c, uc, start_step=1, source=S.ClipSource(z, noise, keep))
        first = list(calls)
        del calls[:]
        b, _ = cc.run(cc.make(name, 3), bd, None, c, uc, start_step=1, source=S.ClipSource(z, noise, keep, mask=None))
    assert torch.equal(ref.bits(a), ref.bits(b)) and calls == first and len(first) == (3 if keep else 1)
    # and without a source on the committed backend, which has none of the four
    x0 = inputs[0]
    with E.use_backend(emu):
        a, _ = cc.run(cc.make(name, 2), bd, x0.clone(), c, uc)
        b, _ = cc.run(cc.make(name, 2), bd, x0.clone(), c, uc, start_step=0, source=None)
    assert torch.equal(a, b)


def test_clip_source_refuses_bad_masks_at_construction():
    z, n = torch.zeros(2, 4, 3, 5), torch.zeros(2, 4, 3, 5)
    ok = torch.ones(2, 3, 5)
    assert S.ClipSource(z, n, mask=ok).selector.shape == (2, 3, 5)
    for bad, exc in [(ok.double(), TypeError), (ok.half(), TypeError), (ok.to(torch.int32), TypeError), (ok.numpy(), TypeError),
                     ([[1.0]], TypeError), (ok[0], ValueError), (ok[:, :2], ValueError), (torch.ones(2, 4, 3, 5), ValueError),
                     (torch.ones(2, 15), ValueError), (ok.to("meta"), ValueError)]:
        with pytest.raises(exc, match="mask"):
            S.ClipSource(z, n, (), mask=bad)


def test_a_masked_source_is_refused_by_name_before_anything_is_launched(bd, inputs):
    _, c, uc = inputs
    src = _source(inputs, (), _band_mask())                            # no kept frame: the mask alone counts as keeping
    be, calls = _counting(emu_region)
    with E.use_backend(be):
        for name in cc.REFUSERS:
            smp = cc.make(name, 3)
            with pytest.raises(NotImplementedError, match=type(smp).__name__):
                smp(bd, None, c, uc, source=src)
        churned = S.EulerEDMSampler(3, guider=S.VanillaCFG(5.0), device="cpu", s_churn=1.0)
        with pytest.raises(NotImplementedError, match="EulerEDMSampler.*churn"):
            churned(bd, None, c, uc, source=src)
        sharded = S.VanillaCFG(5.0)
        sharded.half, sharded.group = 0, None                           # what parallel.ShardedCFG carries
        with pytest.raises(NotImplementedError, match="ShardedCFG"):
            S.EulerEDMSampler(3, guider=sharded, device="cpu")(bd, None, c, uc, source=src)
    assert calls == []
    for missing in ("latent_renoise_masked", "frames_renoise"):
        bare, calls = _counting(emu_region)
        delattr(bare, missing)
        with E.use_backend(bare):
            with pytest.raises(NotImplementedError, match=missing):
                cc.make("euler", 3)(bd, None, c, uc, source=src, network=bd.network)
        assert calls == []


# ---- the mask helpers --------------------------------------------------------------------------------------------------------------
def test_view_mask_and_rect_mask_against_arrays_written_by_hand():
    m = image.view_mask(2, 2, 6, 3, (0, 2))
    assert m.dtype == torch.uint8 and m.tolist() == [[[255, 255, 0, 0, 255, 255]] * 2] * 2
    assert image.view_mask(1, 1, 4, 2, ()).tolist() == [[[0, 0, 0, 0]]] and image.view_mask(1, 1, 4, 4, [3]).tolist() == [[[0, 0, 0, 255]]]
    for bad in (dict(W=7, views=3, keep=(0,)), dict(W=6, views=3, keep=(3,)), dict(W=6, views=3, keep=(-1,)), dict(W=6, views=0, keep=())):
        with pytest.raises(ValueError, match="view_mask"):
            image.view_mask(1, 2, bad["W"], bad["views"], bad["keep"])
    r = image.rect_mask(2, 3, 4, (1, 1, 3, 3))
    assert r.dtype == torch.uint8 and r.tolist() == [[[255, 255, 255, 255], [255, 0, 0, 255], [255, 0, 0, 255]]] * 2
    assert image.rect_mask(1, 2, 2, (0, 0, 2, 2)).tolist() == [[[0, 0], [0, 0]]]
    for bad in ((1, 1, 1, 3), (0, 0, 4, 2), (-1, 0, 2, 2), (0, 0, 2), (0.5, 0, 2, 2), None):
        with pytest.raises(ValueError, match="rect_mask"):
            image.rect_mask(1, 3, 4, bad)


def test_pool_and_select_helpers_are_the_references(calls):
    m = image.view_mask(T, H, W, 6, (0,))
    m[0, 5, 3] = 0                                                       # one regenerated pixel: its cell is not known
    src, gen = cc.clip_u8(), cc.clip_u8(seed=5)
    with E.use_backend(emu_region):
        pooled = image.pool_keep_mask(m, LH, LW)
        out = image.select_u8(src, gen, m)
        for bad in (m.float(), m[0], torch.zeros(T, 0, W, dtype=torch.uint8)):
            with pytest.raises(ValueError, match="pool_keep_mask"):
                image.pool_keep_mask(bad, LH, LW)
        for h, w in ((LH, LW // 2), (5, LW), (0, LW), (H, W // 2)):
            with pytest.raises(ValueError, match="pool_keep_mask"):
                image.pool_keep_mask(m, h, w)
        with pytest.raises(ValueError, match="select_u8"):
            image.select_u8(src, gen[:1], m)
        with pytest.raises(TypeError, match="select_u8"):
            image.select_u8(src.float(), gen, m)
    assert calls == [("mask_pool_u8", 2), ("u8_select", 3)]
    assert torch.equal(pooled, ref.mask_pool_u8(m, 2)) and pooled[0, 2, 1] == 0 and pooled[0, 2, 0] == 1 and pooled.shape == (T, LH, LW)
    assert torch.equal(out, torch.where((m != 0)[..., None], src, gen)) and out.data_ptr() not in (src.data_ptr(), gen.data_ptr())
    with E.use_backend(emu_edit):
        with pytest.raises(NotImplementedError, match="mask_pool_u8"):
            image.pool_keep_mask(m, LH, LW)
        with pytest.raises(NotImplementedError, match="u8_select"):
            image.select_u8(src, gen, m)


# ---- edit_frames -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def twins():
    import image_boundary_cases as ib
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(emu_region, "u8_to_tokens_f16", ib.u8_to_tokens_f16, raising=False)
        mp.setattr(emu_region, "tokens_to_u8", ib.tokens_to_u8, raising=False)
        yield


MASKS = {"view": lambda: image.view_mask(T, H, W, 6, (2,)), "rect": lambda: image.rect_mask(T, H, W, (3, 40, 11, 75))}


@pytest.mark.parametrize("kind", sorted(MASKS))
def test_edit_frames_keeps_the_recorded_bytes_and_the_known_latent_cells(kind, stack, inputs, twins, calls):
    x0, c, uc = inputs
    clip, noise, mask = cc.clip_u8(), torch.randn(x0.shape, generator=torch.Generator().manual_seed(9)), MASKS[kind]()
    seen = {}
    with E.use_backend(emu_region):
        out = pipeline.edit_frames(stack["net"], stack["dec"], stack["enc"], clip, c, uc, noise, strength=0.7, num_steps=3,
                                   sample_posterior=False, keep_mask_u8=mask, callback=lambda i, x: seen.__setitem__(i, x.clone()))
        launches = list(calls)
        z = pipeline.SCALE_FACTOR * stack["enc"].encode_u8(clip, sample=False)
        decoded = stack["dec"].decode_u8(seen[2] / pipeline.SCALE_FACTOR)
    kept = mask != 0
    assert out.shape == clip.shape and out.dtype == torch.uint8 and sorted(seen) == [0, 1, 2]
    assert torch.equal(out[kept], clip[kept]) and torch.equal(out[~kept], decoded[~kept]) and 0 < kept.sum() < kept.numel()
    assert not torch.equal(decoded[kept], clip[kept])                  # the first stage's reconstruction is not the recording
    # the pooled mask is the reference's, the start and the three put-backs are one launch each, then the select
    pooled = ref.mask_pool_u8(mask, 2)
    assert launches == [("mask_pool_u8", 2), (None, False), MASKED + (False,), MASKED + (False,), MASKED + (True,), ("u8_select", 3)]
    sel = pooled.bool()[:, None].expand_as(z)
    assert 0 < sel.sum() < sel.numel() and torch.equal(ref.bits(seen[2])[sel], ref.bits(z)[sel])
    assert (ref.bits(seen[2])[~sel] != ref.bits(z)[~sel]).any()
    if kind == "rect":      # rows 3 .. 10, columns 40 .. 74: latent rows 1 .. 5, columns 20 .. 37 hold a regenerated pixel
        inside = torch.zeros(LH, LW, dtype=torch.bool)
        inside[1:6, 20:38] = True
        assert torch.equal(pooled[0] == 0, inside) and torch.equal(pooled[1], pooled[0])


def test_edit_frames_without_a_mask_is_the_call_without_the_argument(stack, inputs, twins, calls):
    x0, c, uc = inputs
    clip, noise = cc.clip_u8(), torch.randn(x0.shape, generator=torch.Generator().manual_seed(9))
    kw = dict(strength=0.7, keep=(1,), num_steps=3, sample_posterior=False)
    be, _ = _counting(emu_edit)                                          # none of the new wrappers
    with pytest.MonkeyPatch.context() as mp:
        import image_boundary_cases as ib
        mp.setattr(be, "u8_to_tokens_f16", ib.u8_to_tokens_f16, raising=False)
        mp.setattr(be, "tokens_to_u8", ib.tokens_to_u8, raising=False)
        with E.use_backend(be):
            a = pipeline.edit_frames(stack["net"], stack["dec"], stack["enc"], clip, c, uc, noise, **kw)
            first = list(calls)
            del calls[:]
            b = pipeline.edit_frames(stack["net"], stack["dec"], stack["enc"], clip, c, uc, noise, keep_mask_u8=None, **kw)
    assert torch.equal(a, b) and calls == first and len(first) == 4


def test_edit_frames_refuses_a_mask_before_the_first_backend_call(stack, inputs, twins):
    x0, c, uc = inputs
    net, dec, enc = stack["net"], stack["dec"], stack["enc"]
    clip, noise, mask = cc.clip_u8(), torch.randn(x0.shape, generator=torch.Generator().manual_seed(9)), MASKS["view"]()

    def edit(**kw):
        return pipeline.edit_frames(net, dec, enc, clip, c, uc, noise, **{"num_steps": 3, "keep_mask_u8": mask, **kw})
    be, calls = _counting(emu_region)
    cases = [(dict(keep_mask_u8=mask.float()), ValueError, "keep_mask_u8"), (dict(keep_mask_u8=mask.bool()), ValueError, "keep_mask_u8"),
             (dict(keep_mask_u8=mask[0]), ValueError, "keep_mask_u8"), (dict(keep_mask_u8=mask[:, :-2]), ValueError, "keep_mask_u8"),
             (dict(keep_mask_u8=mask[..., None].expand(T, H, W, 3)), ValueError, "keep_mask_u8"),
             (dict(keep_mask_u8=mask.numpy()), ValueError, "keep_mask_u8"), (dict(keep_mask_u8=mask[:1]), ValueError, "keep_mask_u8"),
             (dict(strength=0.0), ValueError, "strength"), (dict(keep=(T,)), ValueError, "keep"),
             (dict(sampler=S.HeunEDMSampler(3, guider=S.VanillaCFG(5.0), device="cpu")), NotImplementedError, "HeunEDMSampler"),
             (dict(sampler=S.EulerAncestralSampler(3, guider=S.VanillaCFG(5.0), device="cpu")), NotImplementedError, "EulerAncestralSampler"),
             (dict(sampler=S.EulerEDMSampler(3, guider=S.VanillaCFG(5.0), device="cpu", s_churn=1.0)), NotImplementedError, "churn")]
    with E.use_backend(be):
        for kw, exc, match in cases:
            with pytest.raises(exc, match=match):
                edit(**kw)
            assert calls == [], (kw.keys(), calls[:3])
        net.diffusion_model.view_shard = object()
        try:
            with pytest.raises(NotImplementedError, match="one device"):
                edit()
        finally:
            del net.diffusion_model.view_shard
        assert net.diffusion_model.view_shard is None and calls == []
    for missing in NEW + ("frames_renoise",):
        bare, calls = _counting(emu_region)
        delattr(bare, missing)
        with E.use_backend(bare):
            with pytest.raises(NotImplementedError, match=missing):
                edit()
        assert calls == []


# ---- the tool ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("argv,match", [(["--keep-views", "0"], "belong to --edit"), (["--edit", "--edit-rect", "4,2,3,9"], "four integers"),
                                        (["--edit", "--keep-views", "6"], "camera views in 0 .. 5")])
def test_the_tool_refuses_its_new_options_before_it_touches_a_device(argv, match):
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "sample.py"), *argv], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 2 and match in r.stderr, r.stderr[-400:]
