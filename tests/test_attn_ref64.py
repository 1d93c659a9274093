"""The float64 attention reference of tests/attn_ref64.py against the fp32 emulation (tests/emu.py), on the CPU.

The GPU tests of tests/test_attn_edges_gpu.py hold the kernels to attn_ref64 under the project's bounds.  Here emu.attn_views /
emu.attn_temporal — fp32 softmax, output rounded to fp16, indexed through strided views — must agree with the reference — float64,
indexed element by element from the header's formulae — within HALF of those bounds on the same shapes: the reference alone sits
well inside the bound, and two independent indexings of the same buffers agree.  The buffers hold NaN wherever the contract says
nothing is read, so either side reading a wrong element fails loudly."""
import ctypes

import pytest
import torch

import attn_edge_cases as cases
import attn_ref64
import emu
from panacea_amd import hip


def _half_bound(tag, got16, ref, bound):
    assert torch.isfinite(ref).all() and torch.isfinite(got16.float()).all(), tag
    err, over = cases.excess_error(got16, ref, (bound[0] / 2, bound[1] / 2))
    used = ((got16.double() - ref).abs() / (bound[0] + bound[1] * ref.abs())).max().item()
    print(f"{tag}: emulation vs float64 max|err| {err:.3e}, at most {used:.2f} of the GPU tests' bound (limit here: 0.50)")
    assert over <= 0, (tag, err, over)


@pytest.mark.parametrize("name,build,bound", [
    ("text-ragged-77", lambda: cases.text_case(1, 2, 4, 48, 2, 77, 77, seed=11), cases.UNIT),
    ("text-ragged-65", lambda: cases.text_case(1, 2, 4, 48, 2, 65, 65, seed=12), cases.UNIT),
    ("text-77of80-7heads", lambda: cases.text_case(1, 3, 13, 31, 7, 80, 77, seed=13), cases.UNIT),
    ("text-80of96-sharp", lambda: cases.text_case(2, 1, 8, 24, 7, 96, 80, sharp=6.0, seed=14), cases.SHARP),
    ("text-90of96-garbage", lambda: cases.text_case(2, 2, 4, 48, 5, 96, 90, pad="garbage", seed=15), cases.UNIT),
    ("causal-77of80", lambda: cases.causal_case(2, 77, 80, 3, pad="garbage"), cases.UNIT),
    ("causal-33of200", lambda: cases.causal_case(1, 33, 200, 2, pad="garbage"), cases.UNIT),
    ("cross-5x10-37", lambda: cases.cross_case(2, 5, 10, 2, 37, pad="garbage"), cases.UNIT),
])
def test_emulation_agrees_with_float64_reference_views(name, build, bound):
    buf, lds, geo = build()
    ops = cases.operands(buf, lds)
    ref = attn_ref64.attn_views(*ops, **geo)
    o = torch.full((buf["M"] + cases.EXCESS, buf["C"]), cases.NAN, dtype=torch.float16)
    emu.attn_views(*ops, o, lds["ldo"], **geo)
    assert torch.isnan(o[buf["M"]:]).all()
    _half_bound(name, o[: buf["M"]], ref, bound)


@pytest.mark.parametrize("B,T,Npix,heads", [(2, 9, 21, 2), (1, 13, 7, 5), (1, 15, 33, 1), (2, 16, 10, 2), (1, 3, 33, 2)])
def test_emulation_agrees_with_float64_reference_temporal(B, T, Npix, heads):
    C, M = heads * 64, B * T * Npix
    qkv = cases.nan_tail(cases.rnd16(M, 3 * C, seed=21 + T), cases.EXCESS)
    flat = qkv.reshape(-1)
    ref = attn_ref64.attn_temporal(flat, 3 * C, flat[C:], 3 * C, flat[2 * C:], 3 * C, B=B, T=T, Npix=Npix, heads=heads, scale=0.125)
    o = torch.full((M, C), cases.NAN, dtype=torch.float16)
    emu.attn_temporal(flat, 3 * C, flat[C:], 3 * C, flat[2 * C:], 3 * C, o, C, B=B, T=T, Npix=Npix, heads=heads, scale=0.125)
    _half_bound(f"temporal T={T}", o, ref, cases.UNIT)


def test_reference_identity_and_single_key():
    """what the reference must give without any arithmetic to trust: a causal row 0 is v[0]; one-hot q = k selects each frame's own v"""
    buf, lds, geo = cases.causal_case(2, 33, 40, 1)
    ref = attn_ref64.attn_views(*cases.operands(buf, lds), **geo)
    v0 = buf["vt"].reshape(-1)[: 2 * 64 * 40].view(2, 64, 40)[:, :, 0].double()
    assert torch.equal(ref.view(2, 40, 64)[:, 0], v0)
    T, Npix = 13, 5
    q = torch.zeros(T, Npix, 64)
    for t in range(T):
        q[t, :, (5 * t + 3) % 64] = 20.0
    q = q.reshape(T * Npix, 64).half()
    v = ((torch.arange(T * Npix * 64).view(-1, 64) * 7) % 1021).half()
    out = attn_ref64.attn_temporal(q, 64, q, 64, v, 64, B=1, T=T, Npix=Npix, heads=1, scale=0.125)
    assert (out - v.double()).abs().max().item() < 1e-15 * 1021 * T


def _params(**over):
    """a PncAttnParams of the product's text launch (80 key rows, 77 valid) with made-up, aligned, never dereferenced pointers"""
    p = hip.AttnParams()
    geo = dict(groups=2, heads=12, H=8, W=96, views=1, kvH=1, kvW=80, kv_views=1, kv_rows_per_group=80, q_per_kv=2, kv_valid=77,
               scale=0.125, causal=0, ldq=768, ldk=768, ldvt=80, vt_gstride=768 * 80, ldo=768)
    geo.update(q=0x10000, k=0x20000, vt=0x30000, o=0x40000)
    geo.update(over)
    for name, val in geo.items():
        setattr(p, name, val)
    p.nseg[0], p.seg[0][0] = 1, 0
    return p


def test_text_kernel_query_follows_the_dispatch_rules():
    """pnc_attn_uses_text_kernel needs no device: the dispatch predicate on the product's launch and on every way out of it"""
    lib = hip.load()
    uses = lambda **over: lib.pnc_attn_uses_text_kernel(ctypes.byref(_params(**over)))      # noqa: E731
    assert lib.pnc_attn_uses_text_kernel(None) == 0
    assert uses() == 1                                          # 6 query tiles x 3 head groups = 18 >= 16
    assert uses(kvW=96, kv_rows_per_group=96, ldvt=96, vt_gstride=768 * 96, kv_valid=96) == 1
    assert uses(heads=10) == 0 and uses(H=4, W=48) == 0         # 12 / 6 workgroups per group: the small grids stay
    for ragged in (65, 77, 90):                                 # a key buffer whose row count is no multiple of 8
        assert uses(kvW=ragged, kv_valid=min(ragged, 77)) == 0
    assert uses(causal=1) == 0 and uses(kv_valid=64) == 0 and uses(q=0) == 0 and uses(ldvt=84) == 0
    prev = hip.set_option(hip.OPT_ATTN_VARIANT, 43)
    try:
        assert uses(H=4, W=48) == 1 and uses(kvW=77) == 0 and uses(kv_valid=64) == 0
        hip.set_option(hip.OPT_ATTN_VARIANT, 42)
        assert uses() == 0
    finally:
        hip.set_option(hip.OPT_ATTN_VARIANT, prev)
    prev = hip.set_option(hip.OPT_ATTN_DMA, 1 | 4)
    try:
        assert uses() == 0
        hip.set_option(hip.OPT_ATTN_DMA, 0)
        assert uses() == 0
    finally:
        hip.set_option(hip.OPT_ATTN_DMA, prev)
    assert uses() == 1
