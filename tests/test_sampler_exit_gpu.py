"""cfg_sampler_step_kernel<SKIP> (panacea_amd/csrc/misc.hip) on the MI355X (-m gpu), bit for bit against the per-op fp32 reference of
tests/sampler_exit_ref.py: every mode, both instantiations, both kinds of entry, every per-frame selector switched off in some
frame of a launch, every optional operand absent and poisoned, every aliased launch the header allows — the cases and the poisoned
allocations of tests/sampler_exit_cases.py.  No tolerance: the header's contract is a sequence of fp32 roundings, and a contracted
FMA moves an output by a few 1e-6, inside every trajectory test's 2e-5.

Per case ONE launch, then every allocation is compared as int32 with the reference's: the output planes, and the margins, the padding
columns of the eps tokens, the operands and the planes the mode does not write, which keep the bits they started with.  A failure
names the wrong-kernel model (sampler_exit_ref.MUTANTS) whose bits the kernel has.  tests/test_sampler_exit_ref.py holds the
reference itself to account on the CPU."""
import pytest
import torch

import sampler_exit_cases as cases
import sampler_exit_ref as ref
from helpers import measured
from panacea_amd import hip
from sampler_exit_cases import CASES, IDS

pytestmark = pytest.mark.gpu
DEV = "cuda"
_TALLY = {}              # mode name -> [launches, elements compared, elements that differ]


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")


def _run(case):
    """the case's launch on the device -> its allocations, back on the CPU"""
    data = cases.build(case).to(DEV)
    cases.launch(hip, case, data)                   # raises PncError on any return code but PNC_OK
    torch.cuda.synchronize()
    return data.cpu()


def _tally(case, got, want):
    compared, diff = cases.count(case, got, want)
    t = _TALLY.setdefault(ref.MODE_NAMES[case.mode], [0, 0, 0])
    t[0], t[1], t[2] = t[0] + 1, t[1] + compared, t[2] + diff


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_kernel_has_the_reference_bits_in_poisoned_allocations(case):
    got, want = _run(case), cases.reference(case)
    _tally(case, got, want)
    cases.check(case, got, want)


@pytest.mark.parametrize("case", cases.ALIASED, ids=[c.name for c in cases.ALIASED])
def test_aliased_launches_equal_the_unaliased_ones(case):
    """out / out_aux IS x0 / aux / hist[k] (DPM2M out_aux = aux: how DPMPP2MSampler launches it): the bits of the same launch into
    planes of their own, and every other operand untouched"""
    plain = case.unaliased()
    aliased, apart = _run(case), _run(plain)
    _tally(case, aliased, cases.reference(case))
    _tally(plain, apart, cases.reference(plain))
    for o in ("out", "out_aux"):
        if o in aliased.span:
            a, b = aliased.view(o), apart.view(o)
            assert torch.isfinite(b).all()
            bad = cases.bits(a) != cases.bits(b)
            assert not bad.any(), f"{case.name}: {o} differs from the unaliased launch in {int(bad.sum())} elements, first at {int(torch.nonzero(bad)[0])}"
    cases.check(plain, apart, cases.reference(plain))
    cases.check(case, aliased, cases.reference(case))


@pytest.mark.parametrize("case", cases.EULER, ids=[c.name for c in cases.EULER])
def test_euler_entries_equal_heun1_out_of_the_reference(case):
    """pnc_cfg_euler_step[_skip]: `out` of the REFERENCE's HEUN1 on the same operands (and of the struct entry's launch)"""
    got = _run(case)
    base = cases.base_of(case)
    want, struct = cases.reference(base), _run(base)
    _tally(base, struct, want)
    assert torch.equal(cases.bits(got.view("out")), cases.bits(want.view("out"))), case.name
    assert torch.equal(cases.bits(got.view("out")), cases.bits(struct.view("out"))), case.name
    cases.check(base, struct, want)


@pytest.mark.parametrize("case", cases.UNUSED, ids=[c.name for c in cases.UNUSED])
def test_unused_operand_poison_is_inert(case):
    """every operand the mode does not read as a fully poisoned plane / vector: the bits of the launch that passes None, and the
    poisoned out_aux of a mode that writes none is left alone"""
    base = cases.base_of(case)
    poisoned, none = _run(case), _run(base)
    _tally(base, none, cases.reference(base))
    for o in ("out", "out_aux"):
        if o == "out" or case.writes_aux:
            assert torch.equal(cases.bits(poisoned.view(o)), cases.bits(none.view(o))), f"{case.name}: {o}"
    cases.check(case, poisoned, cases.reference(case))           # (every poisoned plane and the unwritten out_aux included)
    cases.check(base, none, cases.reference(base))


def test_summary_per_mode():
    """launches, compared output elements and differing elements (outputs, operands and margins) per mode, from the tests above:
    the line profiles/sampler_exit_bits.md quotes.  The last figure is zero if everything above passed."""
    assert _TALLY, "no launch above ran"
    for mode in ref.MODE_NAMES:
        n, compared, diff = _TALLY.get(mode, [0, 0, 0])
        print(f"sampler-exit-bits {mode}: {n} launches, {compared} elements compared, {diff} differ")
        measured("sampler_exit_bits " + mode, launches=n, compared=compared, differ=diff)
    total = [sum(t[k] for t in _TALLY.values()) for k in range(3)]
    print(f"sampler-exit-bits total: {total[0]} launches, {total[1]} elements compared, {total[2]} differ")
    assert set(_TALLY) == set(ref.MODE_NAMES)
    assert total[2] == 0
