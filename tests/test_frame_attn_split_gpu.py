"""pnc_attn_frame_split_f16 (include/panacea_hip.h section 6b) on the MI355X against the float64 reference and the derived bound of
tests/frame_attn_split_ref64.py (tests/test_frame_attn_split.py shows on the CPU that five wrong kernels fall outside that bound on
these very operands and shapes).

The kernel works on 32-query x 32-key tiles: N = 8 (below one tile), 40 (a ragged last key tile), 72 (a ragged query tile behind two
whole ones), 136 (several tiles).  Every operand is a view inside a NaN-filled allocation that ENDS right behind its last named element;
the unnamed elements of o and o_lo hold a bit pattern of their own and are compared bit for bit before and after."""
import ctypes

import pytest
import torch

import attn_edge_cases as cases
import frame_attn_ref64 as single64
import frame_attn_split_ref64 as ref64
from helpers import measured
from panacea_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
CS = (128, 256, 512)
NS = (8, 40, 72, 136)


def _device_ops(planes, lds):
    """-> the nine arguments in front of `o`: NaN-filled buffers that end behind their last named element"""
    return (ref64.embed(planes["q"], lds["q"]).to(DEV), ref64.embed(planes["q_lo"], lds["q"]).to(DEV), lds["q"],
            ref64.embed(planes["k"], lds["k"]).to(DEV), ref64.embed(planes["k_lo"], lds["k"]).to(DEV), lds["k"],
            ref64.embed(planes["v"], lds["v"]).to(DEV), ref64.embed(planes["v_lo"], lds["v"]).to(DEV), lds["v"])


def _launch(ops, ldo, *, F, N, C, scale):
    """-> (o, o_lo) as float64 [F, N, C]; everything but the named elements of either plane must keep its bits"""
    n = (F * N - 1) * ldo + C
    seed = (torch.arange(n, dtype=torch.int64) * 40503 % 65536 - 32768).to(torch.int16)          # NaN, Inf and finite patterns alike
    o, o_lo = seed.clone().to(DEV).view(torch.float16), seed.clone().to(DEV).view(torch.float16)
    hip.attn_frame_split(*ops, o, o_lo, ldo, F=F, N=N, C=C, scale=scale)
    torch.cuda.synchronize()
    named = ref64.named_mask(ldo, F=F, N=N, C=C)
    for name, t in (("o", o), ("o_lo", o_lo)):
        assert torch.equal(t.cpu().view(torch.int16)[~named], seed[~named]), f"unnamed elements of {name} were written"
    return ref64.gather(o.cpu(), ldo, F=F, N=N, C=C), ref64.gather(o_lo.cpu(), ldo, F=F, N=N, C=C)


def _check(tag, kind, *, F, N, C, pad):
    planes, scale = ref64.case(kind, F=F, N=N, C=C)
    lds = dict(q=C + pad, k=C + pad, v=C + pad)
    ldo = C + pad
    ops = _device_ops(planes, lds)
    ref, bnd = ref64.attn_frame_split(*(t.cpu() if torch.is_tensor(t) else t for t in ops), F=F, N=N, C=C, scale=scale)
    o, o_lo = _launch(ops, ldo, F=F, N=N, C=C, scale=scale)
    got = o + ref64.LO * o_lo
    finite = bool(torch.isfinite(got).all())
    err, over = ref64.excess(got, ref, bnd) if finite else (float("nan"), float("nan"))
    frac = ((got - ref).abs() / bnd).max().item() if finite else float("nan")
    print(f"{tag}: attn_frame_split_kernel vs float64 max|err| {err:.3e}, {frac:.3f} of the bound (|ref| max {ref.abs().max().item():.2f})")
    measured("frame_attn_split " + tag.replace(" ", "_"), kernel="attn_frame_split_kernel", max_err=err, of_bound=frac)
    assert finite, f"{tag}: non-finite output"
    assert over <= 0, f"{tag}: max|err| {err:.4e} is {frac:.2f} times the derived bound"
    o2, o2_lo = _launch(ops, ldo, F=F, N=N, C=C, scale=scale)
    assert torch.equal(o, o2) and torch.equal(o_lo, o2_lo), f"{tag}: two runs differ"
    return planes, scale, o


# ------------------------------------------------------------------------------------------ the kernel against float64
@pytest.mark.parametrize("pad", [0, 8])
@pytest.mark.parametrize("F", [1, 3])
@pytest.mark.parametrize("N", NS)
@pytest.mark.parametrize("C", CS)
def test_kernel_vs_float64_default_scale(C, N, F, pad):
    _check(f"unit C{C} N{N} F{F} ld+{pad}", "unit", F=F, N=N, C=C, pad=pad)


@pytest.mark.parametrize("C", CS)
def test_spiked_key_late_in_the_frame_runs_the_deferred_rescale(C):
    _check(f"spike C{C} N136 F3", "spike", F=3, N=136, C=C, pad=8)


@pytest.mark.parametrize("C", CS)
def test_operands_around_2e2_with_lo_planes_beyond_e4m3(C):
    planes, _ = ref64.case("large", F=1, N=72, C=C)
    assert planes["q_lo"].abs().max().item() > 200 and planes["k_lo"].abs().max().item() > 200
    _check(f"large C{C} N72 F1", "large", F=1, N=72, C=C, pad=8)


def test_zero_lo_planes_reproduce_the_single_plane_kernel():
    """all lo planes zero: o (the hi plane alone) and pnc_attn_frame_f16 on the same q / k / V^T agree with the float64 attention of the
    hi planes, and with each other, to within the single-plane bound of tests/test_frame_attn_gpu.py (cases.UNIT)"""
    F, N, C = 3, 136, 512
    planes, scale, o = _check(f"zero_lo C{C} N{N} F{F}", "zero_lo", F=F, N=N, C=C, pad=8)
    q, k, v = (planes[n] for n in ("q", "k", "v"))
    vt = v.transpose(1, 2).contiguous()
    ref = single64.attn_frame(q, C, k, C, vt, N, C * N, F=F, N=N, C=C, scale=scale)
    o1 = torch.full((F * N, C), cases.NAN, device=DEV, dtype=torch.float16)
    hip.attn_frame(q.reshape(F * N, C).to(DEV), C, k.reshape(F * N, C).to(DEV), C, vt.to(DEV), N, C * N, o1, C, F=F, N=N, C=C, scale=scale)
    torch.cuda.synchronize()
    o1 = o1.cpu().reshape(F, N, C)
    for tag, a, b in (("split hi vs float64", o, ref), ("single vs float64", o1, ref), ("split hi vs single", o, o1.double())):
        err, over = cases.excess_error(a, b, cases.UNIT)
        print(f"zero_lo {tag}: max|err| {err:.3e}, over the bound by {over:.3e}")
        assert over <= 0, (tag, err)


# ------------------------------------------------------------------------------------------ the refusal table, one case per rule
def test_refusals_leave_o_unchanged():
    F, N, C = 1, 8, 128
    planes, scale = ref64.case("unit", F=F, N=N, C=C)
    t = {n: p.reshape(F * N, C).to(DEV) for n, p in planes.items()}
    o = torch.full((F * N + 1, C + 8), 3.0, device=DEV, dtype=torch.float16)
    o_lo = torch.full((F * N + 1, C + 8), 5.0, device=DEV, dtype=torch.float16)
    lib = hip.load()
    P = ctypes.c_void_p

    def call(F=F, N=N, C=C, ldq=C, ldk=C, ldv=C, ldo=C + 8, **over):
        p = {n: t[n].data_ptr() for n in t}
        p.update(o=o.data_ptr(), o_lo=o_lo.data_ptr())
        p.update(over)
        a = {n: (None if v is None else P(v)) for n, v in p.items()}
        return lib.pnc_attn_frame_split_f16(a["q"], a["q_lo"], ldq, a["k"], a["k_lo"], ldk, a["v"], a["v_lo"], ldv, a["o"], a["o_lo"], ldo,
                                            F, N, C, ctypes.c_float(scale), None)

    rules = [("null pointer", dict(k_lo=None), -1), ("C outside 128 / 256 / 512", dict(C=64, ldq=64, ldk=64, ldv=64), -1),
             ("F < 1", dict(F=0), -1), ("N < 8", dict(N=0), -1), ("N % 8", dict(N=4 + 8), -1),
             ("grid beyond 2^31", dict(F=2 ** 31 - 1, N=2 ** 20), -1), ("leading dimension below C", dict(ldv=C - 8), -1),
             ("leading dimension no multiple of 8", dict(ldo=C + 4), -2), ("pointer off 16 bytes", dict(o_lo=o_lo.data_ptr() + 8), -2)]
    for what, kw, code in rules:
        assert call(**kw) == code, what
        torch.cuda.synchronize()
        assert bool((o == 3.0).all()) and bool((o_lo == 5.0).all()), f"{what}: something was launched"
    assert call() == 0                                            # and the call they all vary is a valid one
    torch.cuda.synchronize()
    assert bool((o[: F * N, :C] != 3.0).any()) and bool((o[:, C:] == 3.0).all()) and bool((o[F * N:] == 3.0).all())
