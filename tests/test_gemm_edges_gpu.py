"""pnc_gemm_f16 / pnc_gemm_wsplit_f16 against float64 at the geometry edges, inside poisoned allocations (MI355X).

Reference: tests/gemm_ref64.py — float64, indexed from the flat storage by the formulae of include/panacea_hip.h, independent of
tests/emu.py (tests/test_gemm_ref64.py holds the emulation to it on the CPU and shows that the bound bites).  Bound: gemm_ref64.bound,
derived from fp32 accumulation and the number formats, not from a kernel's output — an accumulator staged through fp16, or a
bias added behind the fp16 rounding, is outside it.  Cases: tests/gemm_edge_cases.py — every operand plane a view inside a NaN-filled
allocation (margins, leading-dimension gaps, the space between a band and its column block), every output NaN before the launch.

Per case and data set, ONE launch, then: the library returned PNC_OK; every element the reference marks as written is finite and
within the bound (lo planes: the reconstructed hi + 2^-11 lo); every other element of every output allocation still holds its bits.

Second part: an all-zero `w_lo16` plane gives the bits of the launch without it.  The launch with the plane goes through the weight-part
twins of the kernels (pnc_gemm_wsplit_f16), chosen by the same dispatch (csrc/gemm_dispatch.h): same tiles, same K order, and a zero
plane adds +0 to the zeroed accumulators.  Every case above that can carry the plane, plus the two branch families the case table cannot
express: the fused / trailing LayerNorm and the GroupNorm records out of the temporal conv."""
import ctypes

import pytest
import torch

import gemm_edge_cases as cases
import gemm_ref64 as ref64
from helpers import measured
from panacea_amd import hip
from test_attn_edges_gpu import _options

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
_WORST = {}


def _launch(case, data, zero_plane=False, **opts):
    kw, allocs = case.launch(data, device=DEV)
    if zero_plane:
        kw["w_lo16"] = torch.zeros_like(kw["w16"])       # w16's layout and leading dimension
    with _options(**opts):
        if case.spec.get("splitk"):
            p, lib, _ = hip._gemm_params(**{k: v for k, v in kw.items() if k != "w_lo16"}, workspace=False)
            assert lib.pnc_gemm_workspace_floats(ctypes.byref(p)) > 0, f"{case.name}: the library would not split K"
        hip.gemm(**kw)                       # raises PncError on any return code but PNC_OK
        torch.cuda.synchronize()
    return kw, allocs


@pytest.mark.parametrize("data", cases.DATA)
@pytest.mark.parametrize("case", cases.CASES, ids=[c.name for c in cases.CASES])
def test_gemm_vs_float64_in_poisoned_allocations(case, data):
    r = cases.reference(case, data)
    kw, allocs = _launch(case, data, **case.opts)
    worst = cases.check_outputs(case, data, r, ref64.bound, kw, allocs)
    print(f"{case.name} [{data}] err / bound: " + ", ".join(f"{n} {v:.3g}" for n, v in worst.items()))
    measured("gemm_edges " + case.name, data=data, family=case.family.replace(" ", "_"), **worst)
    fam = _WORST.setdefault(case.family, {})
    for n, v in worst.items():
        fam[n] = max(fam.get(n, 0.0), v)
    if case.spec.get("stencil"):
        # PNC_OPT_STENCIL_TILES = 2 takes the spatial-tile kernel wherever the shape allows; the per-tap kernels (0) compute the same
        # products in the same order: not one bit may differ, in any element of any output allocation
        _, per_tap = _launch(case, data, **dict(case.opts, stencil_tiles=0))
        for n, a in allocs.items():
            bits = torch.int32 if a.dtype == torch.float32 else torch.int16
            assert torch.equal(a.view(bits), per_tap[n].view(bits)), f"{case.name} [{data}] {n}: the tile kernel and the per-tap kernel differ"


def test_worst_ratio_per_family():
    """the table of DESIGN.md (numerics / testing): worst err / bound per case family, from the launches above"""
    for fam, w in _WORST.items():
        print(f"{fam}: " + ", ".join(f"{n} {v:.3g}" for n, v in sorted(w.items())))
        measured("gemm_edges_family " + fam.replace(" ", "_"), **w)
        assert max(w.values()) <= 1.0


# ------------------------------------------------------------------------- a zero w_lo16 plane: the bits of the launch without it
def _bits(t):
    return t.view(torch.uint8 if t.dtype == torch.uint8 else torch.int32 if t.dtype == torch.float32 else torch.int16)


# the fp16-A_lo forward of pnc_gemm_wsplit_f16 is pinned by tests/test_precise_ckpt_gpu.py::test_refusals_and_the_forwarded_fp16_a_lo
ZERO_PLANE_CASES = [c for c in cases.CASES if "w_split" not in c.spec and c.spec.get("a_lo") in (None, "e4m3")]


@pytest.mark.parametrize("case", ZERO_PLANE_CASES, ids=[c.name for c in ZERO_PLANE_CASES])
def test_zero_w_lo16_plane_gives_the_bits_of_the_launch_without_it(case):
    _, without = _launch(case, "signed", **case.opts)
    _, with_plane = _launch(case, "signed", zero_plane=True, **case.opts)
    for n, a in without.items():
        assert torch.equal(_bits(a), _bits(with_plane[n])), f"{case.name} {n}: the launch with a zero w_lo16 plane differs"


def _two_launches(kw, outs, **opts):
    """-> the outputs `outs()` builds (a dict of gemm keywords), after the launch as given and after the one with a zero plane"""
    got = []
    for plane in (None, torch.zeros_like(kw["w16"])):
        o = outs()
        with _options(**opts):
            hip.gemm(**kw, **o, w_lo16=plane)
            torch.cuda.synchronize()
        got.append(o)
    return got


@pytest.mark.parametrize("epi", ["o32", "rb+o32", "r1+o32"])
@pytest.mark.parametrize("N,tile,fused", [(128, 1, True), (320, 3, True), (640, 0, False)])
def test_zero_w_lo16_plane_layernorm(N, tile, fused, epi):
    """LayerNorm in the epilogue (E_LN on the two geometries that own whole rows) and by the library's kernel after the GEMM"""
    M, K = 200, 136
    g = torch.Generator().manual_seed(31)
    kw = dict(a16=torch.randn(M, K, generator=g).half().to(DEV), w16=(torch.randn(N, K, generator=g) * K ** -0.5).half().to(DEV), M=M, N=N, K=K,
              lda=K, ldc32=N, ln_gamma=torch.randn(N, generator=g).to(DEV), ln_beta=torch.randn(N, generator=g).to(DEV), ldln=N,
              ln_in_library=True)
    if epi == "rb+o32":
        kw.update(rowbias=torch.randn(4, N, generator=g).to(DEV), rb_rows=50, rb_mod=4)
    if epi == "r1+o32":
        kw.update(res1=torch.randn(M, N, generator=g).to(DEV), ldr1=N)

    def outs():
        return dict(out32=torch.full((M, N), NAN, device=DEV), ln_out16=torch.full((M, N), NAN, device=DEV, dtype=torch.float16))
    with _options(gemm_tile=tile):
        assert hip.gemm_fuses_layernorm(**kw, **outs()) == fused
    without, with_plane = _two_launches(kw, outs, gemm_tile=tile)
    for n in ("out32", "ln_out16"):
        assert torch.isfinite(without[n]).all()
        assert torch.equal(_bits(without[n]), _bits(with_plane[n])), f"{n}: the launch with a zero w_lo16 plane differs"


@pytest.mark.parametrize("gn_stats", [1, 0])
@pytest.mark.parametrize("epi", ["bias+r1alias+rb+o32", "bias+r1+r2+o32", "bias+r1+r2+o32+o16"])
def test_zero_w_lo16_plane_conv1d_records(epi, gn_stats):
    """PncGemmParams.gn_part out of the temporal conv: from the epilogue (E_GS, PNC_OPT_GEMM_GN_STATS on) and by the statistics kernel
    after the launch (off)"""
    B, T, Npix, C = 2, 2, 64, 320
    F, M, N, K = B * T, B * T * Npix, C, 3 * C
    g = torch.Generator().manual_seed(32)
    res = torch.randn(M, N, generator=g).to(DEV)
    kw = dict(a16=torch.randn(M, C, generator=g).half().to(DEV), w16=(torch.randn(N, K, generator=g) * K ** -0.5).half().to(DEV), M=M, N=N, K=K,
              a_mode=hip.A_CONV1D_T, tconv=dict(C=C, T=T, Npix=Npix), bias=torch.randn(N, generator=g).to(DEV), ldr1=N, ldc32=N)
    if "rb" in epi:
        kw.update(rowbias=torch.randn(F, N, generator=g).to(DEV), rb_rows=Npix, rb_mod=F)
    else:
        kw.update(res1=res, res2=torch.randn(M, N, generator=g).to(DEV), ldr2=N)

    def outs():
        o = dict(out32=res.clone() if "r1alias" in epi else torch.full((M, N), NAN, device=DEV),
                 gn_part=torch.full((F * (Npix // 64) * 96,), NAN, device=DEV))
        if "r1alias" in epi:
            o["res1"] = o["out32"]
        if "o16" in epi:
            o.update(out16=torch.full((M, N), NAN, device=DEV, dtype=torch.float16), ldc16=N)
        return o
    without, with_plane = _two_launches(kw, outs, gemm_tile=3, gemm_gn_stats=gn_stats)
    for n in ("out32", "out16", "gn_part"):
        if n in without:
            assert torch.isfinite(without[n]).all()
            assert torch.equal(_bits(without[n]), _bits(with_plane[n])), f"{n}: the launch with a zero w_lo16 plane differs"
