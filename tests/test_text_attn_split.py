"""The text tower's causal attention on split operands (include/panacea_hip.h section 6c, pnc_attn_text_split_f16) without a GPU:
header and binding, the argument checks of the entry point (nothing is launched), the float64 reference of
tests/text_attn_split_ref64.py against torch's own attention on the recombined operands, and the proof that its derived bound bites:
eight wrong kernels fall outside it, by a factor of at least 2, on the operands and at the shapes the GPU test uses; the emulated twin
of tests/emu_text_tower.py lies inside it.

The kernel itself is held to the same reference and bound in tests/test_text_attn_split_gpu.py."""
import ctypes
import re
from pathlib import Path

import pytest
import torch

import emu_text_tower as ett
import text_attn_split_ref64 as ref64
from panacea_amd import build, hip

PKG = Path(hip.__file__).resolve().parent
EINVAL, EALIGN = -1, -2


# ------------------------------------------------------------------------------------------ 1. header, binding, build
def test_header_binding_and_build_list():
    assert "pnc_attn_text_split_f16" in hip.header_symbols()
    assert set(hip.header_symbols()) == set(hip._SIGNATURES)
    res, args = hip._SIGNATURES["pnc_attn_text_split_f16"]
    L, P, I = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
    assert res is I and args == [P, P, L, P, P, L, P, P, L, P, P, L, I, I, I, I, ctypes.c_float, P]
    assert "attn_text_split.hip" in build.SOURCES
    assert hip.ABI_VERSION == 8                                  # additive: the ABI version did not move
    assert callable(hip.attn_text_split)
    assert hasattr(hip.load(), "pnc_attn_text_split_f16")
    header = (PKG.parent / "include" / "panacea_hip.h").read_text()
    doc = header[header.index("6c. Text-tower attention"):header.index("int pnc_attn_text_split_f16")]
    assert "sgm/modules/encoders/modules.py:604-616" in doc


# ------------------------------------------------------------------------------------------ 2. argument checks, no device
NAMES = ("q", "q_lo", "k", "k_lo", "v", "v_lo", "o", "o_lo")


def test_entry_point_refuses_before_any_launch():
    lib = hip.load()
    buf = (ctypes.c_char * 64)()
    a16 = (ctypes.addressof(buf) + 15) & ~15
    ok, odd = ctypes.c_void_p(a16), ctypes.c_void_p(a16 + 2)

    def call(groups=2, heads=2, Lp=80, kv_valid=77, ldq=None, ldk=None, ldv=None, ldo=None, **ptr):
        p = {n: ptr.get(n, ok) for n in NAMES}
        ldq, ldk, ldv, ldo = (64 * heads if x is None else x for x in (ldq, ldk, ldv, ldo))
        return lib.pnc_attn_text_split_f16(p["q"], p["q_lo"], ldq, p["k"], p["k_lo"], ldk, p["v"], p["v_lo"], ldv, p["o"], p["o_lo"], ldo,
                                           groups, heads, Lp, kv_valid, 0.125, None)

    all_odd = {n: odd for n in NAMES}
    # null pointers first, whatever else is wrong
    for n in NAMES:
        assert call(**{n: None}) == EINVAL, n
        assert call(**dict(all_odd, **{n: None}), Lp=4, ldq=3) == EINVAL, n
    # ranges are looked at before leading dimensions and alignment
    for kw in (dict(groups=0), dict(groups=-1), dict(heads=0), dict(Lp=0), dict(Lp=4), dict(Lp=12, kv_valid=12), dict(Lp=104), dict(Lp=-8),
               dict(kv_valid=0), dict(kv_valid=81), dict(kv_valid=-3), dict(groups=2 ** 16, heads=2 ** 15, ldq=2 ** 21, ldk=2 ** 21,
                                                                          ldv=2 ** 21, ldo=2 ** 21)):
        assert call(**kw) == EINVAL, kw
        assert call(**{**all_odd, "ldq": 132, **kw}) == EINVAL, kw
    # leading dimensions: too short is PNC_EINVAL, a misaligned one PNC_EALIGN, both ahead of the pointers
    for kw in (dict(ldq=120), dict(ldk=127), dict(ldv=64), dict(ldo=0)):
        assert call(**kw) == EINVAL, kw
        assert call(**all_odd, **kw) == EINVAL, kw
    for kw in (dict(ldq=132), dict(ldk=129), dict(ldv=130), dict(ldo=140)):
        assert call(**kw) == EALIGN, kw
    # pointers, each of the eight
    for n in NAMES:
        assert call(**{n: odd}) == EALIGN, n
    # valid-looking ranges stop at the alignment check
    for Lp, kv in ref64.SHAPES:
        for groups, heads in ((1, 1), (3, 2), (2, 16)):
            assert call(o_lo=odd, groups=groups, heads=heads, Lp=Lp, kv_valid=kv) == EALIGN, (Lp, kv, groups, heads)
            W = 64 * heads
            assert call(v_lo=odd, groups=groups, heads=heads, Lp=Lp, kv_valid=kv, ldq=3 * W, ldk=3 * W, ldv=3 * W, ldo=W + 8) == EALIGN


# ------------------------------------------------------------------------------------------ 3. the reference against torch
def _ops(planes, pad):
    W = planes["q"].shape[-1]
    lds = dict(q=W + pad, k=W + 2 * pad, v=W + 3 * pad)
    return (ref64.embed(planes["q"], lds["q"]), ref64.embed(planes["q_lo"], lds["q"]), lds["q"],
            ref64.embed(planes["k"], lds["k"]), ref64.embed(planes["k_lo"], lds["k"]), lds["k"],
            ref64.embed(planes["v"], lds["v"]), ref64.embed(planes["v_lo"], lds["v"]), lds["v"])


def _poison_invalid_rows(planes, kv_valid):
    out = {n: t.clone() for n, t in planes.items()}
    for n in ("k", "k_lo", "v", "v_lo"):
        out[n][:, kv_valid:] = float("nan")
    return out


@pytest.mark.parametrize("Lp,kv", [(24, 17), (80, 77), (8, 1)])
def test_reference_agrees_with_torch_float64_on_the_recombined_operands(Lp, kv):
    geo = dict(groups=3, heads=2, Lp=Lp)
    planes, scale = ref64.case("unit", **geo)
    ref, bnd = ref64.attn_text_split(*_ops(_poison_invalid_rows(planes, kv), 8), kv_valid=kv, scale=scale, **geo)      # NaN padding and NaN rows behind kv_valid
    q, k, v = (ref64.value(planes[n], planes[n + "_lo"]).reshape(3, Lp, 2, 64).transpose(1, 2) for n in ("q", "k", "v"))
    i, j = torch.arange(Lp)[:, None], torch.arange(Lp)[None, :]
    s = (scale * (q @ k.transpose(2, 3))).masked_fill((j > i) | (j >= kv), -float("inf"))
    want = (torch.softmax(s, dim=-1) @ v).transpose(1, 2).reshape(3, Lp, 128)
    assert torch.isfinite(ref).all() and torch.isfinite(bnd).all() and (bnd > 0).all()
    assert (ref - want).abs().max().item() <= 1e-13 * max(1.0, want.abs().max().item())
    dense, _ = ref64.attn_text_split(*_ops(planes, 0), kv_valid=kv, scale=scale, **geo)
    assert torch.equal(dense, ref)                               # the leading dimensions are honoured
    # q / k / v as column blocks of one QKV buffer
    (_, (qh, kh, vh)), (_, (ql, kl, vl)) = ref64.qkv_buffer(planes, ""), ref64.qkv_buffer(planes, "_lo")
    blocks, _ = ref64.attn_text_split(qh, ql, 384, kh, kl, 384, vh, vl, 384, kv_valid=kv, scale=scale, **geo)
    assert torch.equal(blocks, ref)


# ------------------------------------------------------------------------------------------ 4. the bound bites
@pytest.mark.parametrize("Lp,kv", ref64.SHAPES)
def test_eight_wrong_kernels_fall_outside_the_bound_at_every_shape(Lp, kv):
    """q_lo, k_lo or v_lo ignored, Pl dropped, o_lo written as zero, the diagonal off by one either way, kv_valid ignored: each is off
    by at least TWICE the bound somewhere, at every (Lp, kv_valid) the GPU test runs (prompts and heads do not enter: each (prompt,
    head) is an attention of its own), wherever it is a wrong kernel at all (ref64.applies: with one valid key the softmax is the single
    probability 1, with kv_valid = Lp there is nothing to ignore) — where it is not, it must give the reference itself."""
    geo = dict(groups=1, heads=1, Lp=Lp)
    planes, scale = ref64.case("unit", **geo)
    ops = _ops(planes, 0)
    ref, bnd = ref64.attn_text_split(*ops, kv_valid=kv, scale=scale, **geo)
    for m in ref64.MUTATIONS:
        wrong, none = ref64.attn_text_split(*ops, kv_valid=kv, scale=scale, mutate=m, **geo)
        assert none is None
        factor = ((wrong - ref).abs() / bnd).max().item()
        print(f"Lp {Lp} kv_valid {kv}: `{m}` is {factor:.1f} times the bound" + ("" if ref64.applies(m, Lp, kv) else " (not a wrong kernel here)"))
        if ref64.applies(m, Lp, kv):
            assert factor >= 2.0, f"Lp {Lp} kv_valid {kv}: a kernel with `{m}` stays within twice the bound ({factor:.2f})"
        else:
            assert torch.equal(wrong, ref), (Lp, kv, m)
    # the reference rounded to an fp16 PAIR is inside it: the bound does not ask for more than the format holds
    hi, lo = ref64.split(ref)
    assert ref64.excess(ref64.value(hi, lo), ref, bnd)[1] <= 0


@pytest.mark.parametrize("Lp,kv", ref64.SHAPES)
def test_emulated_twin_lies_inside_the_bound(Lp, kv):
    geo = dict(groups=3, heads=2, Lp=Lp)
    planes, scale = ref64.case("unit", **geo)
    ops = _ops(_poison_invalid_rows(planes, kv), 8)
    ref, bnd = ref64.attn_text_split(*ops, kv_valid=kv, scale=scale, **geo)
    ldo = 128 + 8
    o, o_lo = (torch.full(((3 * Lp - 1) * ldo + 128,), 7.0, dtype=torch.float16) for _ in range(2))
    ett.Backend().attn_text_split(*ops, o, o_lo, ldo, kv_valid=kv, scale=scale, **geo)
    named = ref64.named_mask(ldo, F=3, N=Lp, C=128)
    assert bool((o[~named] == 7.0).all()) and bool((o_lo[~named] == 7.0).all())
    got = ref64.value(o[named], o_lo[named]).reshape(3, Lp, 128)
    err, over = ref64.excess(got, ref, bnd)
    print(f"Lp {Lp} kv_valid {kv}: emulated twin max|err| {err:.3e}, {((got - ref).abs() / bnd).max().item():.3f} of the bound")
    assert over <= 0


# ------------------------------------------------------------------------------------------ 5. the optional capability stays optional
def test_no_direct_call_through_a_backend_handle():
    for f in sorted(PKG.rglob("*.py")):
        txt = f.read_text()
        assert ".be.attn_text_split(" not in txt, f
        assert "attn_text_split" not in re.findall(r"(?:\.be|backend\(\)|\bbe)\.([A-Za-z_]\w*)\s*\(", txt), f
