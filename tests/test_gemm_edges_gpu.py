"""pnc_gemm_f16 / pnc_gemm_wsplit_f16 against float64 at the geometry edges, inside poisoned allocations (MI355X).

Reference: tests/gemm_ref64.py — float64, indexed from the flat storage by the formulae of include/panacea_hip.h, independent of
tests/emu.py (tests/test_gemm_ref64.py holds the emulation to it on the CPU and shows that the bound bites).  Bound: gemm_ref64.bound,
derived from fp32 accumulation and the number formats, not from a kernel's output — an accumulator staged through fp16, or a
bias added behind the fp16 rounding, is outside it.  Cases: tests/gemm_edge_cases.py — every operand plane a view inside a NaN-filled
allocation (margins, leading-dimension gaps, the space between a band and its column block), every output NaN before the launch.

Per case and data set, ONE launch, then: the library returned PNC_OK; every element the reference marks as written is finite and
within the bound (lo planes: the reconstructed hi + 2^-11 lo); every other element of every output allocation still holds its bits."""
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
_WORST = {}


def _launch(case, data, **opts):
    kw, allocs = case.launch(data, device=DEV)
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
