"""Region editing on the MI355X: pnc_latent_renoise_masked, pnc_mask_pool_u8 and pnc_u8_select against the per-op references of
tests/region_edit_ref.py bit for bit, their argument checks, and the tiny network (T = 2 frames, latent 8 x 96) through
pipeline.edit_frames with a view mask and through a captured step.

Kernel cases: every operand and the output live in an allocation of their own filled with a pattern (a NaN for floats, 0xA5 for
bytes), the tensor MARGIN elements in; after the launch the WHOLE allocations are compared as integers — the output's margins still
hold the pattern, the operands are untouched.  Each case runs in three layouts: every tensor on a 16-byte boundary ("aligned");
every tensor one element off one ("shifted": the 16-byte body with a head); the tensors at four different offsets ("mixed": element
by element).  The kernels index in int64 from their first line and the hosts refuse what a launch cannot count, so no case needs a
size past 2^31 to reach another path."""
import ctypes as C
from pathlib import Path

import pytest
import torch

import clip_edit_cases as cc
import region_edit_ref as ref
from panacea_amd import hip, image, pipeline, sampling as S

DEV = "cuda"
T = cc.T
MARGIN = 64                     # elements either side: a multiple of 16 bytes, so a shift of 0 keeps the allocator's alignment
POISON = 0x7FC0BEEF             # a quiet NaN with a payload
POISON_U8 = 0xA5
LAYOUTS = {"aligned": dict(z=0, noise=0, x=0, out=0, mask=0), "shifted": dict(z=1, noise=1, x=1, out=1, mask=1),
           "mixed": dict(z=1, noise=2, x=3, out=0, mask=2)}
BYTE_LAYOUTS = {"aligned": dict(src=0, gen=0, out=0, mask=0), "shifted": dict(src=1, gen=1, out=1, mask=1),
                "mixed": dict(src=1, gen=2, out=0, mask=3)}


def _poisoned(t: torch.Tensor, shift=0):
    """-> (the whole allocation as integers, `t`'s values in a contiguous view MARGIN + shift elements in)"""
    n = t.numel()
    if t.dtype == torch.uint8:
        buf = torch.full((MARGIN + shift + n + MARGIN,), POISON_U8, dtype=torch.uint8, device=DEV)
        view = buf[MARGIN + shift:MARGIN + shift + n].view(t.shape)
    else:
        buf = torch.full((MARGIN + shift + n + MARGIN,), POISON, dtype=torch.int32, device=DEV)
        view = buf.view(torch.float32)[MARGIN + shift:MARGIN + shift + n].view(t.shape)
    view.copy_(t)
    return buf, view


def _like(kind, args, inner, as_bits):
    return [m for m, (k, _) in ref.MUTANTS.items()
            if k == kind and torch.equal(inner, as_bits({"renoise": ref.latent_renoise_masked, "pool": ref.mask_pool_u8,
                                                         "select": ref.u8_select}[kind](*args, mutant=m)).reshape(-1))]


def _compare(tag, kind, args, dev, before, lo, want_bits, skip=()):
    """the whole output allocation against `before` with the reference's bits laid in at `lo`; every operand untouched"""
    torch.cuda.synchronize()
    expect = before["out"].clone()
    expect[lo:lo + want_bits.numel()] = want_bits.reshape(-1).to(DEV)
    got = dev["out"][0]
    if not torch.equal(got, expect):
        inner = got[lo:lo + want_bits.numel()].cpu()
        as_bits = (lambda t: t.contiguous()) if want_bits.dtype == torch.uint8 else ref.bits
        bad = (got != expect).nonzero().flatten()
        pytest.fail(f"{tag}: {bad.numel()} elements differ, first at {bad[0].item() - lo} of the output (negative / past "
                    f"{want_bits.numel()}: a margin); the bits of wrong kernel(s) {_like(kind, args, inner, as_bits) or 'none'}")
    for k in dev:
        if k != "out" and k not in skip:
            assert torch.equal(dev[k][0], before[k]), (tag, k)


# ---- pnc_latent_renoise_masked -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,pattern", [(s, m) for s in ref.RENOISE_SHAPES for m in ref.MASKS],
                         ids=[f"{'x'.join(map(str, s))}-{m}" for s in ref.RENOISE_SHAPES for m in ref.MASKS])
def test_masked_renoise_has_the_reference_bits_in_poisoned_allocations(shape, pattern):
    for variant in ref.VARIANTS:
        ops = ref.renoise_case(shape, pattern, variant)
        args = (ops["z"], ops["noise"], ops["sigma"], ops["mask"], ops["x"])
        want = ref.latent_renoise_masked(*args)
        for layout, shift in LAYOUTS.items():
            dev = {k: _poisoned(ops[k], shift.get(k, 0)) for k in ("z", "noise", "sigma", "mask", "x")}
            if ops["out_is_x"]:
                dev["out"] = dev["x"]
            else:
                dev["out"] = _poisoned(torch.zeros(shape), shift["out"])
                dev["out"][0][:] = POISON                               # the output region too: every element has to be written
            before = {k: b.clone() for k, (b, _) in dev.items()}
            view = {k: v for k, (_, v) in dev.items()}
            out_shift = shift["x"] if ops["out_is_x"] else shift["out"]
            assert (view["out"].data_ptr() % 16 == 0) == (out_shift == 0)
            hip.latent_renoise_masked(view["z"], view["noise"], view["sigma"], view["mask"], view["x"], view["out"])
            _compare(f"{shape} {pattern} {variant} {layout}", "renoise", args, dev, before, MARGIN + out_shift, ref.bits(want),
                     skip=("x",) if ops["out_is_x"] else ())
    assert "libpanacea_hip.so" in Path("/proc/self/maps").read_text()


# ---- pnc_mask_pool_u8 --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ref.POOL_CASES, ids=lambda c: "x".join(map(str, c[:4])) + f"+{c[4]}")
def test_mask_pool_has_the_reference_bits_in_poisoned_allocations(case):
    Tn, H, W, f, off = case
    for fill in ref.POOL_FILLS:
        m = ref.pool_mask(case, fill)
        want = ref.mask_pool_u8(m, f)
        for mshift in sorted({off, 0, 1}):                             # the case's own base, and both an aligned and an odd one
            for oshift in (0, 1):
                dev = dict(mask=_poisoned(m, mshift), out=_poisoned(torch.zeros(want.shape), oshift))
                dev["out"][0][:] = POISON
                before = {k: b.clone() for k, (b, _) in dev.items()}
                assert dev["mask"][1].data_ptr() % 8 == mshift
                hip.mask_pool_u8(dev["mask"][1], f, dev["out"][1])
                _compare(f"{case} {fill} mask+{mshift} out+{oshift}", "pool", (m, f), dev, before, MARGIN + oshift, ref.bits(want))


# ---- pnc_u8_select -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ref.SELECT_CASES, ids=lambda c: f"{c[0]}x{c[1]}")
def test_u8_select_has_the_reference_bytes_in_poisoned_allocations(case):
    src, gen, mask = ref.select_case(case)
    want = ref.u8_select(src, gen, mask)
    assert not torch.equal(want, gen) or case[0] == 1
    for layout, shift in BYTE_LAYOUTS.items():
        for out_is_gen in (False, True):
            dev = dict(src=_poisoned(src, shift["src"]), gen=_poisoned(gen, shift["gen"]), mask=_poisoned(mask, shift["mask"]))
            dev["out"] = dev["gen"] if out_is_gen else _poisoned(torch.full(case, POISON_U8, dtype=torch.uint8), shift["out"])
            before = {k: b.clone() for k, (b, _) in dev.items()}
            view = {k: v for k, (_, v) in dev.items()}
            out_shift = shift["gen"] if out_is_gen else shift["out"]
            hip.u8_select(view["src"], view["gen"], view["mask"], view["out"])
            _compare(f"{case} {layout} out_is_gen={out_is_gen}", "select", (src, gen, mask), dev, before, MARGIN + out_shift, want,
                     skip=("gen",) if out_is_gen else ())


# ---- the argument checks: rejected before any launch -------------------------------------------------------------------------------
EINVAL, EALIGN = -1, -2
_BUF = (C.c_char * 256)()
A16 = (C.addressof(_BUF) + 15) & ~15
A2, A1, B16, NULL = A16 + 2, A16 + 1, A16 + 64, None
RENOISE = dict(z=A16, noise=A16, sigma=A16, mask=A16, x=A16, out=A16, T=2, C=4, Npix=5)
POOL = dict(mask_u8=A16, out=A16, T=2, H=16, W=24, f=8)
SELECT = dict(src=A16, gen=B16, mask_u8=A16, out=B16, npix=5, C=3)
ROWS = [("pnc_latent_renoise_masked", RENOISE, tag, over, want) for tag, over, want in
        [(f"{k}=NULL", {k: NULL}, EINVAL) for k in ("z", "noise", "sigma", "mask", "x", "out")] + [
            ("T=0", dict(T=0), EINVAL), ("C=0", dict(C=0), EINVAL), ("Npix=0", dict(Npix=0), EINVAL), ("T=-1", dict(T=-1), EINVAL),
            ("frame>2^40", dict(C=4, Npix=(1 << 38) + 1), EINVAL), ("grid>=2^31", dict(T=1 << 21, C=1, Npix=1 << 20), EINVAL)] + [
            (f"{k}&3", {k: A2}, EALIGN) for k in ("z", "noise", "sigma", "mask", "x", "out")] + [
            ("order:mask,out", dict(mask=NULL, out=A2), EINVAL), ("order:T,sigma", dict(T=0, sigma=A2), EINVAL),
            ("order:grid,noise", dict(T=1 << 21, C=1, Npix=1 << 20, noise=A2), EINVAL)]] + [
    ("pnc_mask_pool_u8", POOL, tag, over, want) for tag, over, want in
    [("mask=NULL", dict(mask_u8=NULL), EINVAL), ("out=NULL", dict(out=NULL), EINVAL), ("T=0", dict(T=0), EINVAL), ("H=0", dict(H=0), EINVAL),
     ("W=0", dict(W=0), EINVAL), ("f=0", dict(f=0), EINVAL), ("f=17", dict(f=17, H=34, W=34), EINVAL), ("H%f", dict(H=20), EINVAL),
     ("W%f", dict(W=28), EINVAL), ("cells>2^38", dict(T=1 << 20, H=1 << 10, W=1 << 10, f=1), EINVAL), ("out&3", dict(out=A2), EALIGN),
     ("order:f,out", dict(f=0, out=A2), EINVAL), ("order:W%f,out", dict(W=28, out=A2), EINVAL)]] + [
    ("pnc_u8_select", SELECT, tag, over, want) for tag, over, want in
    [(f"{k}=NULL", {k: NULL}, EINVAL) for k in ("src", "gen", "mask_u8", "out")] + [
        ("npix=0", dict(npix=0), EINVAL), ("npix>2^40", dict(npix=(1 << 40) + 1), EINVAL), ("C=0", dict(C=0), EINVAL), ("C=5", dict(C=5), EINVAL),
        ("out==src", dict(out=A16), EINVAL), ("out==src, odd", dict(src=A1, out=A1), EINVAL)]]


@pytest.mark.gpu
@pytest.mark.parametrize("entry,base,over,want", [pytest.param(e, b, o, w, id=f"{e[4:]}-{tag}") for e, b, tag, o, w in ROWS])
def test_rejected_before_any_launch(entry, base, over, want):
    assert want < 0 and set(over) <= set(base)
    assert len(base) + 1 == len(hip._SIGNATURES[entry][1])
    assert getattr(hip.load(), entry)(*{**base, **over}.values(), None) == want


# ---- the tiny network ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stack():
    return cc.tiny_stack(DEV)


@pytest.mark.gpu
def test_edit_frames_keeps_view_0_and_a_captured_step_replays_the_eager_bits(stack):
    from panacea_amd.graph import GraphedStep
    net, dec, enc = stack["net"], stack["dec"], stack["enc"]
    x0, c, uc = cc.tiny_inputs(stack["kw"], DEV)
    clip = cc.clip_u8(DEV)
    noise = torch.randn(x0.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    mask = image.view_mask(T, cc.H, cc.W, 6, (0,), DEV)
    seen = {}
    out = pipeline.edit_frames(net, dec, enc, clip, c, uc, noise, strength=1.0, num_steps=3, sample_posterior=False, keep_mask_u8=mask,
                               callback=lambda i, x: seen.__setitem__(i, x.clone()))
    z = pipeline.SCALE_FACTOR * enc.encode_u8(clip, sample=False)
    torch.cuda.synchronize()
    assert sorted(seen) == [0, 1, 2] and out.shape == clip.shape and out.dtype == torch.uint8 and out.device.type == "cuda"
    kept = (mask != 0).cpu()
    decoded = dec.decode_u8(seen[2] / pipeline.SCALE_FACTOR).cpu()
    assert torch.equal(out.cpu()[kept], clip.cpu()[kept]) and torch.equal(out.cpu()[~kept], decoded[~kept])
    pooled = image.pool_keep_mask(mask, cc.LH, cc.LW)
    assert torch.equal(pooled.cpu(), ref.mask_pool_u8(mask.cpu(), 2))
    sel = pooled.bool().cpu()[:, None].expand(z.shape)
    last, zc = seen[2].cpu(), z.cpu()
    assert 0 < sel.sum() < sel.numel() and torch.equal(ref.bits(last)[sel], ref.bits(zc)[sel])
    assert torch.isfinite(last).all() and all((ref.bits(last[t])[~sel[t]] != ref.bits(zc[t])[~sel[t]]).any() for t in range(T))
    # the first step of that schedule with its masked put-back, eager and replayed from a captured graph
    src = S.ClipSource(z, noise, (), mask=pooled)
    smp = S.EulerEDMSampler(3, guider=S.VanillaCFG(5.0), device=DEV)
    bd = S.BoundDenoiser(S.DiscreteDenoiser().to(DEV), net)
    sig = smp.sigmas()
    s_in = x0.new_ones([T])
    with torch.no_grad():
        hc, hu = S.hoist_invariants(net, smp.guider, c, uc)
        assert smp._fusable(bd, x0, hc)
        start = src.renoise(s_in * sig[0])

        def step(xi, s0, s1):
            return src.put_back(smp.sampler_step(s0, s1, bd, xi, hc, hu), s1)
        eager = step(start, s_in * sig[0], s_in * sig[1]).clone()
        g = GraphedStep(step, start, s_in * sig[0], s_in * sig[1], network=net)
        graphed = g(start, s_in * sig[0], s_in * sig[1]).clone()
    torch.cuda.synchronize()
    assert torch.equal(eager, seen[0]) and torch.equal(ref.bits(graphed.cpu()), ref.bits(eager.cpu()))
    want = ref.latent_renoise_masked(zc.reshape(T, 4, -1), noise.cpu().reshape(T, 4, -1), (s_in * sig[1]).cpu(), pooled.cpu().reshape(T, -1),
                                     eager.cpu().reshape(T, 4, -1))
    assert torch.equal(ref.bits(eager.cpu().reshape(T, 4, -1)), ref.bits(want))
