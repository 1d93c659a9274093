"""pnc_gemm_f16 / pnc_gemm_wsplit_f16 against float64 over the operand RANGE, inside poisoned allocations (MI355X).

tests/test_gemm_edges_gpu.py walks the geometry on unit-scale data.  Here the same reference (tests/gemm_ref64.py), the same
machinery (tests/gemm_edge_cases.py: RANGE_CASES on the data sets RANGE_DATA) and the same bound walk the number range:

  wide-rows    operands from fp16's subnormals to 2^13 by row, e4m3 A_lo bytes from the format's subnormals to the +-448 a clamped
               producer writes, weights times 2^g with w_lo_exp from ~96 to ~130 and fp16-subnormal weights: the lo pass on the
               block-scaled MFMA, the fp16 lo passes and the weight part at every scale they accept
  graded-cols  outputs from fp16's subnormals to 2^15 by column: out16, fp16 and e4m3 out16_lo beyond the clamp at |v| = 512,
               SiLU / erf GELU far in their tails, GEGLU gates outside the table, and the range monitor as the GEMM's writers feed it

Per case and data set ONE launch between two pnc_range_monitor_collect calls, then: check_outputs (every written element finite and
inside gemm_ref64.bound, every other element of every output allocation untouched) and check_range (gemm_ref64.bound, points 6 and
7: the planes of a launch that writes out32 as exact functions of that out32, no e4m3 NaN code, SiLU's tail, and the monitor's count
— exact from the launch's own out32, bracketed from the reference without one).  A wide-rows case that can carry a `w_lo16` plane
is launched once more with an all-zero one: the bits of the launch without it, at every w_lo_exp.

tests/test_gemm_range_ref64.py (CPU) holds the emulation to the same checks, states the conditions the data sets meet and shows nine
wrong kernels outside them."""
import pytest
import torch

import gemm_edge_cases as cases
import gemm_ref64 as ref64
from helpers import measured
from panacea_amd import hip
from test_gemm_edges_gpu import _bits, _launch

pytestmark = pytest.mark.gpu
DEV = "cuda"
_WORST = {}


@pytest.mark.parametrize("case,data", cases.RANGE_RUNS, ids=cases.RANGE_IDS)
def test_gemm_vs_float64_over_the_range(case, data):
    r = cases.reference(case, data)
    count = torch.zeros(2, dtype=torch.int32, device=DEV)
    hip.range_monitor_collect(count[:1])           # before: whatever earlier launches of this process left
    kw, allocs = _launch(case, data, **case.opts)
    hip.range_monitor_collect(count[1:])
    torch.cuda.synchronize()
    worst = cases.check_outputs(case, data, r, ref64.bound, kw, allocs)
    print(f"{case.name} [{data}] err / bound: " + ", ".join(f"{n} {v:.3g}" for n, v in worst.items()) + f", monitor {int(count[1])}")
    measured("gemm_range " + case.name, data=data, family=case.family.replace(" ", "_"), monitor=int(count[1]), **worst)
    cases.check_range(case, data, r, kw, int(count[1]))
    fam = _WORST.setdefault(case.family, {})
    for n, v in worst.items():
        fam[n] = max(fam.get(n, 0.0), v)
    if case.spec["range"] == "wide-rows" and "w_split" not in case.spec and case.spec.get("a_lo") in (None, "e4m3"):
        _, with_plane = _launch(case, data, zero_plane=True, **case.opts)
        for n, a in allocs.items():
            assert torch.equal(_bits(a), _bits(with_plane[n])), f"{case.name} [{data}] {n}: the launch with a zero w_lo16 plane differs"


def test_worst_ratio_per_family_over_the_range():
    """the table of DESIGN.md (GEMM family over the operand range): worst err / bound per case family, from the launches above"""
    for fam, w in _WORST.items():
        print(f"{fam}: " + ", ".join(f"{n} {v:.3g}" for n, v in sorted(w.items())))
        measured("gemm_range_family " + fam.replace(" ", "_"), **w)
        assert max(w.values()) <= 1.0
