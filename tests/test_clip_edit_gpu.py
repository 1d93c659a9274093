"""Clip editing on the MI355X: pnc_frames_renoise against the per-op fp32 reference of tests/clip_edit_ref.py bit for bit, its
argument checks, and the tiny network (T = 2 frames, latent 8 x 96) through pipeline.edit_frames, a captured step and `start_step`.

Kernel cases: every operand and the output live in an allocation of their own filled with a NaN pattern, the tensor MARGIN floats
in; after the launch the WHOLE allocations are compared as int32 — the output's margins still hold the pattern, the operands are
untouched.  Each case runs in three layouts: every tensor on a 16-byte boundary ("aligned"); every tensor 4 bytes off one
("shifted": the 16-byte body with a three-element head); z, noise and out at three different offsets ("mixed": element by element).
The kernel indexes in int64 from its first line (the host refuses frames past 2^40 elements and grids past 2^31 workgroups), so no
case needs a size past 2^31 to reach another path; such a case would move 8 GiB per operand."""
import ctypes as C
from pathlib import Path

import pytest
import torch

import clip_edit_cases as cc
import clip_edit_ref as ref
from panacea_amd import hip, pipeline, sampling as S

DEV = "cuda"
T = cc.T
MARGIN = 64                     # floats either side: 256 bytes, so a shift of 0 keeps the allocator's alignment
POISON = 0x7FC0BEEF             # a quiet NaN with a payload
LAYOUTS = {"aligned": dict(z=0, noise=0, x=0, out=0), "shifted": dict(z=1, noise=1, x=1, out=1), "mixed": dict(z=1, noise=2, x=3, out=0)}


def _poisoned(t: torch.Tensor, shift=0):
    """-> (the whole allocation as int32, `t`'s values in a contiguous view MARGIN + shift floats in)"""
    n = t.numel()
    buf = torch.full((MARGIN + shift + n + MARGIN,), POISON, dtype=torch.int32, device=DEV)
    view = buf.view(torch.float32)[MARGIN + shift:MARGIN + shift + n].view(t.shape)
    view.copy_(t)
    return buf, view


@pytest.mark.gpu
@pytest.mark.parametrize("shape,variant", list(ref.cases()), ids=[f"{'x'.join(map(str, s))}-{v}" for s, v in ref.cases()])
def test_kernel_has_the_reference_bits_in_poisoned_allocations(shape, variant):
    ops = ref.case(shape, variant)
    want = ref.frames_renoise(ops["z"], ops["noise"], ops["sigma"], ops["keep"], ops["x"])
    for layout, shift in LAYOUTS.items():
        dev = {k: _poisoned(ops[k], shift.get(k, 0)) for k in ("z", "noise", "sigma", "keep", "x") if ops[k] is not None}
        if ops["out_is_x"]:
            dev["out"] = dev["x"]
        else:
            dev["out"] = _poisoned(torch.zeros(shape), shift["out"])
            dev["out"][0][:] = POISON                                   # the output region too: every element has to be written
        before = {k: b.clone() for k, (b, _) in dev.items()}
        view = {k: v for k, (_, v) in dev.items()}
        out_shift = shift["x"] if ops["out_is_x"] else shift["out"]
        assert (view["out"].data_ptr() % 16 == 0) == (out_shift == 0)
        hip.frames_renoise(view["z"], view["noise"], view["sigma"], view["out"], keep=view.get("keep"), x=view.get("x"))
        torch.cuda.synchronize()
        expect = before["out"].clone()
        lo = MARGIN + out_shift
        expect[lo:lo + want.numel()] = ref.bits(want).reshape(-1).to(DEV)
        got = dev["out"][0]
        if not torch.equal(got, expect):
            inner = got[lo:lo + want.numel()].cpu()
            args = (ops["z"], ops["noise"], ops["sigma"], ops["keep"], ops["x"])
            like = [m for m in ref.MUTANTS if torch.equal(inner, ref.bits(ref.frames_renoise(*args, mutant=m)).reshape(-1))]
            bad = (got != expect).nonzero().flatten()
            pytest.fail(f"{shape} {variant} {layout}: {bad.numel()} words differ, first at {bad[0].item() - lo} of the output "
                        f"(negative / past {want.numel()}: a margin); the bits of wrong kernel(s) {like or 'none'}")
        for k in dev:
            if k != "out" and not (k == "x" and ops["out_is_x"]):
                assert torch.equal(dev[k][0], before[k]), (shape, variant, layout, k)
    assert "libpanacea_hip.so" in Path("/proc/self/maps").read_text()


# ---- the argument checks: rejected before any launch -------------------------------------------------------------------------------
EINVAL, EALIGN = -1, -2
_BUF = (C.c_char * 256)()
A16 = (C.addressof(_BUF) + 15) & ~15
A2, NULL = A16 + 2, None
BASE = dict(z=A16, noise=A16, sigma=A16, keep=A16, x=A16, out=A16, T=2, C=4, Npix=5)
HOST_ROWS = [(f"{k}=NULL", {k: NULL}, EINVAL) for k in ("z", "noise", "sigma", "out")] + [
    ("keep-without-x", dict(x=NULL), EINVAL), ("T=0", dict(T=0), EINVAL), ("C=0", dict(C=0), EINVAL), ("Npix=0", dict(Npix=0), EINVAL),
    ("T=-1", dict(T=-1), EINVAL), ("frame>2^40", dict(C=4, Npix=(1 << 38) + 1), EINVAL),
    ("grid>=2^31", dict(T=1 << 21, C=1, Npix=1 << 20), EINVAL)] + [
    (f"{k}&3", {k: A2}, EALIGN) for k in ("z", "noise", "sigma", "keep", "x", "out")] + [
    # two faults at once: the EINVAL checks come before the alignment
    ("order:z,out", dict(z=NULL, out=A2), EINVAL), ("order:T,sigma", dict(T=0, sigma=A2), EINVAL),
    ("order:keep-without-x,z", dict(x=NULL, z=A2), EINVAL), ("order:grid,noise", dict(T=1 << 21, C=1, Npix=1 << 20, noise=A2), EINVAL)]


@pytest.mark.gpu
@pytest.mark.parametrize("over,want", [pytest.param(o, w, id=tag) for tag, o, w in HOST_ROWS])
def test_rejected_before_any_launch(over, want):
    assert want < 0 and set(over) <= set(BASE)
    assert len(BASE) + 1 == len(hip._SIGNATURES["pnc_frames_renoise"][1])
    assert hip.load().pnc_frames_renoise(*{**BASE, **over}.values(), None) == want


# ---- the tiny network ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def stack():
    return cc.tiny_stack(DEV)


@pytest.mark.gpu
def test_edit_frames_keeps_frame_0_and_a_captured_step_replays_the_eager_bits(stack):
    from panacea_amd.graph import GraphedStep
    net, dec, enc = stack["net"], stack["dec"], stack["enc"]
    x0, c, uc = cc.tiny_inputs(stack["kw"], DEV)
    clip = cc.clip_u8(DEV)
    noise = torch.randn(x0.shape, generator=torch.Generator().manual_seed(9)).to(DEV)
    seen = {}
    out = pipeline.edit_frames(net, dec, enc, clip, c, uc, noise, strength=1.0, keep=(0,), num_steps=3, sample_posterior=False,
                               callback=lambda i, x: seen.__setitem__(i, x.clone()))
    z = pipeline.SCALE_FACTOR * enc.encode_u8(clip, sample=False)
    torch.cuda.synchronize()
    assert sorted(seen) == [0, 1, 2] and out.shape == clip.shape and out.dtype == torch.uint8 and out.device.type == "cuda"
    assert torch.equal(ref.bits(seen[2][0].cpu()), ref.bits(z[0].cpu())) and not torch.equal(seen[2][1], z[1])
    assert torch.isfinite(seen[2]).all() and torch.equal(out, dec.decode_u8(seen[2] / pipeline.SCALE_FACTOR))
    # the first step of that schedule with its put-back, eager and replayed from a captured graph
    src = S.ClipSource(z, noise, (0,))
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
    want0 = ref.frames_renoise(z.cpu().reshape(T, 4, -1), noise.cpu().reshape(T, 4, -1), (s_in * sig[1]).cpu())[0]
    assert torch.equal(ref.bits(eager[0].cpu().reshape(4, -1)), ref.bits(want0))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["euler", "dpmpp2m"])
def test_start_step_composes_on_the_fused_path(stack, name):
    x0, c, uc = cc.tiny_inputs(stack["kw"], DEV)
    bd = S.BoundDenoiser(S.DiscreteDenoiser().to(DEV), stack["net"])
    assert cc.make(name, device=DEV)._fusable(bd, x0, c)
    with torch.no_grad():
        full = cc.check_composition(name, bd, x0, c, uc, device=DEV)
    assert torch.isfinite(full).all()
