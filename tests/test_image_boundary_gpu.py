"""The image boundary on the MI355X; every comparison is exact.

* pnc_u8_to_tokens_f16 against pnc_nchw_to_tokens_f16 on the float NCHW tensor built from the same bytes with the reference's numpy
  expression: both planes, both tables, with and without a lo plane, the source at byte offsets 0, 1, 3 and 13 inside a larger
  allocation (aligned-down vector loads stay inside memory the test owns), 0xFF-filled outputs with a guard behind them.
* pnc_tokens_to_u8 against the reference's formula in numpy float32 at every rounding threshold, the specials and random values.
* end to end on the tiny first stage and the tiny network: decode_u8, encode_u8, eps with a uint8 hint (eager and replayed).
"""
import numpy as np
import pytest
import torch

import image_boundary_cases as ib
import test_vae as tv
from helpers import product_network, step_inputs
from panacea_amd import checkpoint as ck, hip, image
from panacea_amd.nn import model

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _filled(nbytes: int) -> torch.Tensor:
    """nbytes + GUARD bytes of 0xFF on the device"""
    return torch.full((nbytes + ib.GUARD,), 0xFF, dtype=torch.uint8, device=DEV)


def _bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("C,Cpad,F,H,W", ib.U8_SHAPES, ids=[f"c{s[0]}-f{s[2]}-{s[3]}x{s[4]}" for s in ib.U8_SHAPES])
def test_u8_to_tokens_is_nchw_to_tokens_of_the_scaled_floats(C, Cpad, F, H, W):
    Npix, rows = H * W, F * H * W
    u8 = ib.frame_bytes(F, H, W, C)
    assert all(len(np.unique(u8[..., c])) == min(256, rows) for c in range(C))
    n, plane = u8.size, rows * Cpad * 2
    for kind in ("layout", "image"):
        # the reference: the old entry on the float tensor the host pipeline builds
        a32 = torch.from_numpy(ib.scaled_nchw(u8, kind)).to(DEV)
        ref_hi = torch.empty((rows, Cpad), dtype=torch.float16, device=DEV)
        ref_lo = torch.empty_like(ref_hi)
        hip.nchw_to_tokens_f16(a32, C, None, 0, F, Npix, Cpad, ref_hi, ref_lo)
        lut = torch.from_numpy(ib.TABLES[kind]).to(DEV)
        assert np.array_equal(image.device_table(kind, DEV).cpu().numpy().view(np.uint32), ib.TABLES[kind].view(np.uint32))
        for off in ib.U8_OFFSETS:
            big = torch.zeros(16 + off + n + 32, dtype=torch.uint8, device=DEV)
            src = big[16 + off: 16 + off + n]
            src.copy_(torch.from_numpy(u8.reshape(-1)))
            assert src.data_ptr() % 16 == off and src.is_contiguous()
            for with_lo in (True, False):
                bh, bl = _filled(plane), _filled(plane)
                hi, lo = bh[:plane].view(torch.float16).view(rows, Cpad), bl[:plane].view(torch.float16).view(rows, Cpad)
                hip.u8_to_tokens_f16(src.view(F, H, W, C), lut, F, Npix, C, Cpad, hi, lo if with_lo else None)
                torch.cuda.synchronize()
                tag = (kind, off, with_lo)
                assert torch.equal(_bits(hi), _bits(ref_hi)), tag
                assert (bh[plane:] == 0xFF).all() and (bl[plane:] == 0xFF).all(), tag
                if with_lo:
                    assert torch.equal(_bits(lo), _bits(ref_lo)), tag
                else:
                    assert (bl == 0xFF).all(), tag


@pytest.mark.parametrize("C,Cpad,P,off", [(19, 24, 30 * 61, 3), (19, 24, 2049 * 861 + 5, 13), (3, 8, 2 * 2048 + 77, 1)],
                         ids=["three-tiles", "more-tiles-than-workgroups", "c3-three-tiles"])
def test_u8_to_tokens_over_several_tiles(C, Cpad, P, off):
    """Beyond the five shapes above, which fit one tile: a workgroup stages (16384 - 16) // C pixels at a time (861 of 19 bytes, at
    most 2048), every tile starts at another offset of a 16-byte chunk, and past 2048 tiles the workgroups stride over them.  The
    bytes and the float tensor are built on the device here (the table lookup IS the numpy expression, elementwise:
    tests/test_image_boundary.py), the reference is again the old entry."""
    p = torch.arange(P, device=DEV).view(P, 1)
    u8 = ((7 * p + 13 * torch.arange(C, device=DEV).view(1, C) + p // 256) % 256).to(torch.uint8)
    lut = torch.from_numpy(ib.TABLES["layout"]).to(DEV)
    a32 = lut[u8.long()].t().contiguous().view(1, C, P)
    ref_hi = torch.empty((P, Cpad), dtype=torch.float16, device=DEV)
    ref_lo = torch.empty_like(ref_hi)
    hip.nchw_to_tokens_f16(a32, C, None, 0, 1, P, Cpad, ref_hi, ref_lo)
    big = torch.zeros(16 + off + P * C + 32, dtype=torch.uint8, device=DEV)
    src = big[16 + off: 16 + off + P * C]
    src.copy_(u8.view(-1))
    plane = P * Cpad * 2
    bh, bl = _filled(plane), _filled(plane)
    hi, lo = bh[:plane].view(torch.float16).view(P, Cpad), bl[:plane].view(torch.float16).view(P, Cpad)
    hip.u8_to_tokens_f16(src.view(1, P, C), lut, 1, P, C, Cpad, hi, lo)
    torch.cuda.synchronize()
    assert torch.equal(_bits(hi), _bits(ref_hi)) and torch.equal(_bits(lo), _bits(ref_lo))
    assert (bh[plane:] == 0xFF).all() and (bl[plane:] == 0xFF).all()


def test_u8_to_tokens_refusals_raise_before_any_launch():
    src = torch.zeros((1, 4, 3), dtype=torch.uint8, device=DEV)
    lut = torch.zeros(256, device=DEV)
    out = _filled(4 * 8 * 2 + 32)
    o16 = out[:64].view(torch.float16).view(4, 8)
    for kw, code in [(dict(Cpad=12), "PNC_EINVAL"), (dict(Cch=9), "PNC_EINVAL"), (dict(out16=out[8:72].view(torch.float16)), "PNC_EALIGN"),
                     (dict(out16_lo=out[66:130].view(torch.float16)), "PNC_EALIGN")]:
        args = dict(src_u8=src, lut32=lut, F=1, Npix=4, Cch=3, Cpad=8, out16=o16, out16_lo=None)
        args.update(kw)
        if "Cch" in kw:
            args["src_u8"] = torch.zeros((1, 4, 9), dtype=torch.uint8, device=DEV)
        with pytest.raises(hip.PncError, match=code):
            hip.u8_to_tokens_f16(**args)
    with pytest.raises(hip.PncError, match="PNC_EINVAL"):
        hip.tokens_to_u8(torch.zeros((4, 9), device=DEV), 9, 4, 9, torch.zeros((4, 9), dtype=torch.uint8, device=DEV))
    with pytest.raises(hip.PncError, match="PNC_EALIGN"):
        hip.tokens_to_u8(torch.zeros((4, 3), device=DEV), 3, 4, 3, out[1:13].view(4, 3))
    torch.cuda.synchronize()
    assert (out == 0xFF).all()


@pytest.mark.parametrize("M,C,ld", ib.Q_SHAPES, ids=[f"m{m}-c{c}-ld{ld}" for m, c, ld in ib.Q_SHAPES])
def test_tokens_to_u8_is_the_references_formula(M, C, ld):
    vals = ib.quantiser_inputs(M * C).reshape(M, C)
    want = ib.quantise(vals)
    if M * C >= 1024:          # the whole list is in: every output value occurs, at its threshold and just below the next one
        assert np.array_equal(np.unique(want), np.arange(256)) and np.isnan(vals).any() and np.isinf(vals).any()
    x = np.full((M, ld), np.nan, dtype=np.float32)          # row padding the kernel must not read into the output
    x[:, C:] = 7.0
    x[:, :C] = vals
    xd = torch.from_numpy(x).to(DEV)
    buf = _filled(M * C)
    out = buf[:M * C].view(M, C)
    hip.tokens_to_u8(xd, ld, M, C, out)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(vals[i, j], got[i, j], want[i, j]) for i, j in bad[:5]]
    assert (buf[M * C:] == 0xFF).all()


# ---- end to end -----------------------------------------------------------------------------------------------------------------
def test_decode_u8_is_to_uint8_of_decode():
    _, sd, g = tv._tiny()
    fs = model.FirstStageDecoder(4, tv.TINY)
    fs.load_state_dict(sd, strict=True)
    fs = fs.to(DEV)
    z = torch.from_numpy(g["z"]).to(DEV) * 1.5             # (some outputs beyond +-1: the clamp is exercised)
    img = fs.decode(z)
    got = fs.decode_u8(z)
    torch.cuda.synchronize()
    F, _, H, W = img.shape
    want = np.stack([ck._to_uint8(f) for f in img])
    assert got.dtype == torch.uint8 and got.is_cuda and got.shape == (F, H, W, 3)
    assert np.array_equal(got.cpu().numpy(), want) and 0 in want and 255 in want and len(np.unique(want)) > 100


def test_encode_u8_is_encode_of_the_scaled_floats():
    _, sd, g = tv._tiny_enc()
    fe = model.FirstStageEncoder(4, tv.TINY)
    fe.load_state_dict(sd, strict=True)
    fe = fe.to(DEV)
    F, _, H, W = g["x"].shape
    u8 = np.random.default_rng(9).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    x = torch.from_numpy(ib.scaled_nchw(u8, "image")).to(DEV)
    ud = torch.from_numpy(u8).to(DEV)
    assert torch.equal(fe.moments_u8(ud), fe.moments(x))
    want = fe.encode(x, generator=torch.Generator(DEV).manual_seed(11))
    got = fe.encode_u8(ud, generator=torch.Generator(DEV).manual_seed(11))
    torch.cuda.synchronize()
    assert got.shape == (F, 4, H // 2, W // 2) and torch.isfinite(got).all() and torch.equal(got, want)


@pytest.fixture(scope="module")
def tiny_net():
    w, _, kw = product_network("tiny", DEV)
    inp = step_inputs("tiny", kw, DEV)
    T = kw["num_frames"]
    _, C, H, W = inp["cond_feat"].shape
    u8 = np.random.default_rng(5).integers(0, 256, (T, H, W, C), dtype=np.uint8)
    return w, kw, inp, torch.from_numpy(u8).to(DEV), torch.from_numpy(ib.scaled_nchw(u8, "layout")).to(DEV)


@pytest.mark.parametrize("prec", ["precise", "fast"])
def test_eps_with_a_uint8_hint_is_eps_with_the_float_hint(tiny_net, prec):
    from panacea_amd import sampling as S
    from panacea_amd.graph import GraphedStep
    w, kw, inp, u8, f32 = tiny_net
    T = kw["num_frames"]
    net = w.diffusion_model
    net.precision = prec
    try:
        # the network as the drop-in boundary calls it: one hint frame per latent frame of the doubled batch
        cf = dict(concat=inp["concat"], crossattn=inp["crossattn"], cond_feat=f32.repeat(2, 1, 1, 1))
        cu = dict(cf, cond_feat=u8.repeat(2, 1, 1, 1))
        ef, eu = w(inp["x"], inp["t"], cf), w(inp["x"], inp["t"], cu)
        assert torch.isfinite(ef).all() and torch.equal(ef, eu)
        # one fused Euler / CFG step with hoisted invariants: eager on the float hint, replayed from a captured graph on the bytes
        den = S.DiscreteDenoiser().to(DEV)
        smp = S.EulerEDMSampler(3, guider=S.VanillaCFG(5.0), device=DEV)
        sig = smp.sigmas()
        x0 = inp["x"][T:] * 14.6
        s_in = x0.new_ones([T])
        bd = S.BoundDenoiser(den, w)

        def conds(hint):
            c = {"crossattn": inp["crossattn"][1:2], "concat": inp["concat"][T:], "cond_feat": hint}
            uc = {"crossattn": inp["crossattn"][0:1], "concat": inp["concat"][:T], "cond_feat": hint}
            return c, uc
        with torch.no_grad():
            c, uc = conds(f32)
            assert smp._fusable(bd, x0, c)
            want = smp.sampler_step(s_in * sig[0], s_in * sig[1], bd, x0, c, uc)
            c8, uc8 = conds(u8)
            eager = smp.sampler_step(s_in * sig[0], s_in * sig[1], bd, x0, c8, uc8)
            h8, hu8 = S.hoist_invariants(w, smp.guider, c8, uc8)
            hoisted = smp.sampler_step(s_in * sig[0], s_in * sig[1], bd, x0, h8, hu8)
            g = GraphedStep(lambda xi, s0, s1: smp.sampler_step(s0, s1, bd, xi, c8, uc8), x0, s_in * sig[0], s_in * sig[1])
            graphed = g(x0, s_in * sig[0], s_in * sig[1]).clone()
        torch.cuda.synchronize()
        assert torch.isfinite(want).all() and torch.equal(eager, want) and torch.equal(hoisted, want) and torch.equal(graphed, want)
    finally:
        net.precision = "precise"
