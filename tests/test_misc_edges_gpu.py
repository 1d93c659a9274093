"""Sections 4 and 5 of include/panacea_hip.h — pnc_linear_smallm*, pnc_timestep_embedding*, pnc_nchw_to_tokens_f16, pnc_tokens_to_nchw_f32,
pnc_concat_add, pnc_add_f32, pnc_cast_f16, pnc_softmax_rows_f16 — against float64 at their edge shapes, inside poisoned allocations
(MI355X).

Reference and bounds: tests/misc_ref64.py — float64, indexed from the flat storage by the formulae of the header, independent of
tests/emu.py; every allowance derived from the number formats and the documented accuracy of the instructions, none measured on a
kernel (tests/test_misc_ref64.py holds the emulation to half of them on the CPU and shows that they bite).  Cases: tests/misc_edge_cases.py
— every operand a view inside a NaN-filled allocation, every output NaN before the launch.

Per case and data set, ONE launch, then: the library returned PNC_OK; every element the reference marks as written is bit-equal to the
exact result (fp32 sums, layout moves, hi and lo planes) or finite and within the bound; a masked probability is +0; every other
element of every output allocation still holds its bits.  e4m3 lo planes: the range monitor counts exactly the quads the data clamps.

Then the identities the header states: an all-zero W_lo gives the bits of the launch without it; integer-valued float timesteps give
the int64 kernel's bits; masked score columns may hold NaN / +-Inf without changing one bit of the output; unmasked softmax launches
reproduce the stored output of the kernel before the mask became a predicate (tests/golden/softmax_rows_unmasked.pt)."""
from pathlib import Path

import pytest
import torch

import misc_edge_cases as cases
from helpers import measured
from panacea_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = Path(__file__).resolve().parent / "golden" / "softmax_rows_unmasked.pt"
_WORST = {}


def _launch(case, data, **over):
    t, allocs = case.launch(data, device=DEV)
    case.call(hip, t, **over)                      # raises PncError on any return code but PNC_OK
    torch.cuda.synchronize()
    return t, allocs


@pytest.mark.parametrize("case,data", cases.RUNS, ids=cases.RUN_IDS)
def test_helpers_vs_float64_in_poisoned_allocations(case, data):
    expects, clamped = case.reference(data)
    count = torch.zeros(2, dtype=torch.int32, device=DEV)
    hip.range_monitor_collect(count[:1])           # before: whatever earlier launches of this process left
    t, allocs = _launch(case, data)
    hip.range_monitor_collect(count[1:])
    torch.cuda.synchronize()
    worst = cases.check_outputs(case, data, expects, t, allocs)
    print(f"{case.name} [{data}] err / bound: " + ", ".join(f"{n} {v:.3g}" for n, v in worst.items()))
    measured("misc_edges " + case.name, data=data, family=case.family.replace(" ", "_"), **worst)
    fam = _WORST.setdefault(case.family, {})
    for n, v in worst.items():
        fam[n] = max(fam.get(n, 0.0), v)
    assert int(count[1]) == clamped, f"{case.name}: the range monitor counted {int(count[1])} clamped quads, the data clamps {clamped}"


def test_worst_ratio_per_family():
    """the table of DESIGN.md (numerics / testing): worst err / bound per family, from the launches above (0 = an exact family)"""
    assert _WORST, "no launch above ran"
    for fam, w in _WORST.items():
        print(f"{fam}: " + ", ".join(f"{n} {v:.3g}" for n, v in sorted(w.items())))
        measured("misc_edges_family " + fam.replace(" ", "_"), **w)
        assert max(w.values()) <= 1.0


# ------------------------------------------------------------------------------------------------------------ identities of the header
def _same(a, b, what):
    for n in a:
        assert torch.equal(cases.bits(a[n]), cases.bits(b[n])), f"{what}: {n} differs"


W_LO_CASES = [c for c in cases.CASES if c.spec.get("w_lo")]


@pytest.mark.parametrize("case", W_LO_CASES, ids=[c.name for c in W_LO_CASES])
def test_zero_w_lo_gives_the_bits_of_the_launch_without_it(case):
    t, with_zero = case.launch("signed", device=DEV)
    t["w_lo"].zero_()
    case.call(hip, t)
    t, without = case.launch("signed", device=DEV)
    del t["w_lo"]
    case.call(hip, t)
    torch.cuda.synchronize()
    out = case.build("signed")[1]["out32"].view(without["out32"]).cpu()
    assert torch.isfinite(out[case.reference("signed")[0]["out32"].idx]).all()
    _same(without, with_zero, case.name)


INT_CASES = [c for c in cases.CASES if c.fn == "embed" and c.spec["kind"] == "i64"]


@pytest.mark.parametrize("case", INT_CASES, ids=[c.name for c in INT_CASES])
def test_integer_valued_float_timesteps_give_the_int64_bits(case):
    t, as_int = _launch(case, "t")
    tf, as_float = case.launch("t", device=DEV)
    tf["t"] = tf["t"].float()                      # 2^24 + 1 rounds to 2^24, as the int64 kernel's conversion does
    case.call(hip, tf)
    torch.cuda.synchronize()
    _same(as_int, as_float, case.name)


NONFINITE = [c for c in cases.CASES if "masked-nonfinite" in c.data]


@pytest.mark.parametrize("case", NONFINITE, ids=[c.name for c in NONFINITE])
def test_masked_columns_do_not_influence_the_output_by_one_bit(case):
    """NaN / +Inf / -Inf in every masked column: the bits of the same launch with finite scores there"""
    _, finite = _launch(case, "randn30")
    _, junk = _launch(case, "masked-nonfinite")
    _same(finite, junk, case.name)


def test_unmasked_launches_keep_the_bits_of_the_kernel_before_the_predicate():
    """tests/golden/softmax_rows_unmasked.pt: the p16 of two unmasked cases as the kernel wrote them while its mask was the -3.0e38
    stand-in alone (recorded on the MI355X from the parent of the change; the same bits on repeated launches)"""
    gold = torch.load(GOLDEN)
    assert len(gold) == 2
    for (name, data), want in gold.items():
        t, _ = _launch(cases.BY_NAME[name], data)
        assert torch.equal(cases.bits(t["p16"].cpu()), cases.bits(want)), f"{name} [{data}]"
