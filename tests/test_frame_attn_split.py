"""The fused first-stage attention on split operands (include/panacea_hip.h section 6b, pnc_attn_frame_split_f16) without a GPU:
header and binding, the argument checks of the entry point (nothing is launched), the float64 reference of
tests/frame_attn_split_ref64.py against torch's own attention on the recombined operands, and the proof that its derived bound
bites: five wrong kernels fall outside it on the operands the GPU test uses, at every shape it uses.

The kernel itself is held to the same reference and bound in tests/test_frame_attn_split_gpu.py."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import frame_attn_split_ref64 as ref64
from panacea_amd import build, hip

PKG = Path(hip.__file__).resolve().parent
CS = (128, 256, 512)
NS = (8, 40, 72, 136)        # below one key tile, a ragged last key tile, a ragged second query tile (64 + 8), several tiles
EINVAL, EALIGN = -1, -2


# ------------------------------------------------------------------------------------------ 1. header, binding, build
def test_header_binding_and_build_list():
    assert "pnc_attn_frame_split_f16" in hip.header_symbols()
    assert set(hip.header_symbols()) == set(hip._SIGNATURES)
    res, args = hip._SIGNATURES["pnc_attn_frame_split_f16"]
    L, P, I = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
    assert res is I and args == [P, P, L, P, P, L, P, P, L, P, P, L, I, I, I, ctypes.c_float, P]
    assert "attn_frame_split.hip" in build.SOURCES
    assert hip.ABI_VERSION == 8                                  # additive: the ABI version did not move
    assert callable(hip.attn_frame_split)
    assert hasattr(hip.load(), "pnc_attn_frame_split_f16")


# ------------------------------------------------------------------------------------------ 2. argument checks, no device
NAMES = ("q", "q_lo", "k", "k_lo", "v", "v_lo", "o", "o_lo")


def test_entry_point_refuses_before_any_launch():
    lib = hip.load()
    buf = (ctypes.c_char * 64)()
    a16 = (ctypes.addressof(buf) + 15) & ~15
    ok, odd = ctypes.c_void_p(a16), ctypes.c_void_p(a16 + 2)

    def call(F=2, N=64, C=128, ldq=None, ldk=None, ldv=None, ldo=None, **ptr):
        p = {n: ptr.get(n, ok) for n in NAMES}
        ldq, ldk, ldv, ldo = (C if x is None else x for x in (ldq, ldk, ldv, ldo))
        return lib.pnc_attn_frame_split_f16(p["q"], p["q_lo"], ldq, p["k"], p["k_lo"], ldk, p["v"], p["v_lo"], ldv, p["o"], p["o_lo"], ldo,
                                            F, N, C, 0.125, None)

    all_odd = {n: odd for n in NAMES}
    # null pointers first, whatever else is wrong
    for n in NAMES:
        assert call(**{n: None}) == EINVAL, n
        assert call(**dict(all_odd, **{n: None}), C=64, ldq=3) == EINVAL, n
    # ranges are looked at before leading dimensions and alignment
    for kw in (dict(C=64), dict(C=384), dict(C=0), dict(N=0), dict(N=12), dict(N=-8), dict(F=0)):
        assert call(**kw) == EINVAL, kw
        assert call(**all_odd, ldq=132, **kw) == EINVAL, kw
    assert call(q=odd, F=2 ** 31 - 1, N=2 ** 20) == EINVAL        # one workgroup per 32 queries of a frame: the grid must fit
    # leading dimensions: too short is PNC_EINVAL, a misaligned one PNC_EALIGN, both ahead of the pointers
    for kw in (dict(ldq=120), dict(ldk=127), dict(ldv=64), dict(ldo=0)):
        assert call(**kw) == EINVAL, kw
        assert call(**all_odd, **kw) == EINVAL, kw
    for kw in (dict(ldq=132), dict(ldk=129), dict(ldv=130), dict(ldo=140)):
        assert call(**kw) == EALIGN, kw
    # pointers, each of the eight
    for n in NAMES:
        assert call(**{n: odd}) == EALIGN, n
    # valid-looking ranges of every instantiated width stop at the alignment check
    for C in CS:
        for F, N in ((1, 8), (3, 136), (1, 49152), (8, 12288)):
            assert call(o_lo=odd, F=F, N=N, C=C) == EALIGN, (F, N, C)
            assert call(v_lo=odd, F=F, N=N, C=C, ldq=C + 8, ldk=C + 16, ldv=C + 24, ldo=C + 8) == EALIGN, (F, N, C)


# ------------------------------------------------------------------------------------------ 3. the reference against torch
def _ops(planes, C, pad):
    lds = dict(q=C + pad, k=C + 2 * pad, v=C + 3 * pad)
    return (ref64.embed(planes["q"], lds["q"]), ref64.embed(planes["q_lo"], lds["q"]), lds["q"],
            ref64.embed(planes["k"], lds["k"]), ref64.embed(planes["k_lo"], lds["k"]), lds["k"],
            ref64.embed(planes["v"], lds["v"]), ref64.embed(planes["v_lo"], lds["v"]), lds["v"])


@pytest.mark.parametrize("kind", ["unit", "spike", "large"])
def test_reference_agrees_with_torch_float64_on_the_recombined_operands(kind):
    F, N, C = 3, 40, 128
    planes, scale = ref64.case(kind, F=F, N=N, C=C)
    ref, bnd = ref64.attn_frame_split(*_ops(planes, C, 8), F=F, N=N, C=C, scale=scale)      # NaN padding, buffers end at the last element
    q, k, v = (ref64.value(planes[n], planes[n + "_lo"]) for n in ("q", "k", "v"))
    want = torch.softmax(scale * (q @ k.transpose(1, 2)), dim=-1) @ v
    assert torch.isfinite(ref).all() and torch.isfinite(bnd).all() and (bnd > 0).all()
    assert (ref - want).abs().max().item() <= 1e-13 * max(1.0, want.abs().max().item())
    dense, _ = ref64.attn_frame_split(*_ops(planes, C, 0), F=F, N=N, C=C, scale=scale)
    assert torch.equal(dense, ref)                               # the leading dimensions are honoured
    # the split of values the library would make recombines to 2^-22
    x = torch.randn(1000, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    hi, lo = ref64.split(x)
    assert (ref64.value(hi, lo) - x.float().double()).abs().max().item() <= 2.0 ** -22 * x.abs().max().item()


# ------------------------------------------------------------------------------------------ 4. the bound bites
@pytest.mark.parametrize("kind", ["unit", "spike", "large"])
@pytest.mark.parametrize("C", CS)
def test_five_wrong_kernels_fall_outside_the_bound_at_every_shape(kind, C):
    """q_lo, k_lo or v_lo ignored, Pl dropped, o_lo written as zero: each is off by more than the bound somewhere, at every N the GPU
    test runs (F does not enter: frames are independent), so a kernel that loses one of the planes cannot pass it.  Measured on the
    `unit` operands: between 2.2 (C = 512, N = 136, Pl) and 42 (C = 128, N = 8, o_lo) times the bound."""
    for N in NS:
        planes, scale = ref64.case(kind, F=1, N=N, C=C)
        ops = _ops(planes, C, 0)
        ref, bnd = ref64.attn_frame_split(*ops, F=1, N=N, C=C, scale=scale)
        for m in ref64.MUTATIONS:
            wrong, none = ref64.attn_frame_split(*ops, F=1, N=N, C=C, scale=scale, mutate=m)
            assert none is None
            err, over = ref64.excess(wrong, ref, bnd)
            assert over > 0, f"{kind} C{C} N{N}: a kernel with `{m}` lost stays inside the bound (max err {err:.3e})"
            assert ((wrong - ref).abs() / bnd).max().item() > 1.5, (kind, C, N, m)
        # and the reference rounded to an fp16 PAIR is inside it: the bound does not ask for more than the format holds
        hi, lo = ref64.split(ref)
        assert ref64.excess(ref64.value(hi, lo), ref, bnd)[1] <= 0


def test_spike_case_raises_a_row_maximum_by_more_than_the_deferral_threshold():
    """rows with h_i g_j = +1 at the spiked key: their maximum rises by more than 8 in the exp2 domain, in the LAST key tile"""
    for C in CS:
        planes, scale = ref64.case("spike", F=1, N=136, C=C)
        x = scale * 1.4426950408889634 * (planes["q"][0].double() @ planes["k"][0].double().t())
        before, after = x[:, :128].max(dim=1).values, x[:, 128:].max(dim=1).values
        assert ((after - before) > 8.0).sum().item() >= 136 // 2 - 1


# ------------------------------------------------------------------------------------------ 5. the optional capability stays optional
def test_no_direct_call_through_a_backend_handle():
    for f in sorted(PKG.rglob("*.py")):
        txt = f.read_text()
        assert ".be.attn_frame_split(" not in txt, f
        assert "attn_frame_split" not in re.findall(r"(?:\.be|backend\(\)|\bbe)\.([A-Za-z_]\w*)\s*\(", txt), f
