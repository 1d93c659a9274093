"""The reference of the sampler exit kernel's bit-level GPU test (tests/test_sampler_exit_gpu.py), held to account on the CPU:

  * tests/emu.py gives the reference's bits on every case, margins intact — which ties tests/sampler_exit_ref.py, through
    test_fused_steps_are_the_plain_steps… (tests/test_samplers.py), to the plain torch mirrors of the reference's samplers;
  * the reference's output is finite on every case (a condition on the inputs: a failing case gets another `seed`);
  * the reference is the header's formula: float64 agrees within a bound derived per element from the roundings;
  * every selecting vector has a taken and a not-taken frame in one launch, the pure ones a NaN frame;
  * every wrong-kernel model (sampler_exit_ref.MUTANTS) leaves the reference's bits in every case family it applies to;
  * the poison is inert: another poison pattern, and poisoned planes for the operands a mode does not read, change no output bit."""
import pytest
import torch

import emu
import sampler_exit_cases as cases
import sampler_exit_ref as ref
from sampler_exit_cases import CASES, IDS

SELECTING = {ref.HEUN2: (1,), ref.EULER_A: (3,), ref.DPM2S_2: (2, 4), ref.DPM2M: (4,)}
PURE = {ref.EULER_A: (3,), ref.DPM2S_2: (4,), ref.DPM2M: (4,)}

_EVERY = [f for f in cases.FAMILIES if f != "lms-negzero"]
# wrong-kernel model -> the case families in which it must show (it is run on every case of them; the cases it cannot touch — no cfg
# for the CFG halves, the eps path for the skip term, T = 1 for the frame index — are part of their families' sums)
MUTANT_FAMILIES = {
    "fma_all": _EVERY,
    "fma_denoised": _EVERY,
    "fma_update": _EVERY,
    "halves_swapped": _EVERY,                                               # every family has cfg = 1 cases
    "cond_at_C": _EVERY,                                                    # ... with ld > C
    "frame_npix_plus_1": _EVERY,                                            # ... and T >= 2
    "select_ge": ["grid-HEUN2", "grid-EULER_A", "grid-DPM2S_2", "grid-DPM2M", "alias-HEUN2", "alias-DPM2S_2", "alias-DPM2M", "s_noise",
                  "scale", "unused"],                                       # a 0.0 or -0.0 frame in some launch of each
    "select_nan_true": ["grid-EULER_A", "grid-DPM2S_2", "grid-DPM2M"],     # the T = 5 shape's NaN frames
    "select_sigma_up": ["grid-EULER_A", "grid-DPM2S_2", "alias-DPM2S_2", "s_noise"],
    "noise_assoc": ["grid-EULER_A", "grid-DPM2S_2", "alias-DPM2S_2", "s_noise"],
    "lms_oldest_first": ["grid-LMS", "lms-hist", "alias-LMS"],
    "lms_sum_reversed": ["grid-LMS", "lms-hist", "alias-LMS"],
    "lms_no_zero_start": ["lms-negzero"],                                   # distinguishable: x = -0.0 and coeff_0 * d = -0.0
    "dpm2m_aux_clobbered": ["alias-DPM2M"],
    "heun2_select_sigma_hat": ["grid-HEUN2", "alias-HEUN2"],
    "skip_adds_x": [f for f in _EVERY if f.startswith("grid-") or f in ("euler", "unused", "dpm2m-noaux", "lms-hist")],
}


def test_case_list_covers_the_grid():
    assert set(MUTANT_FAMILIES) == set(ref.MUTANTS)
    grid = {(c.mode, c.shape, c.cfg, c.skip) for c in CASES if c.family.startswith("grid-")}
    assert len(grid) == 7 * 4 * 2 * 2
    assert {c.n_hist for c in CASES if c.family == "lms-hist"} == {0, 1, 2, 3}
    assert {c.scale for c in CASES if c.family == "scale"} == {5.0, 1.0, 0.0, -1.5}
    assert {c.s_noise for c in CASES if c.family == "s_noise"} == {0.9, 1.0, 0.0}
    assert {(c.mode, c.alias[0]) for c in cases.ALIASED} == (
        {(m, ("out", o)) for m in (ref.HEUN2, ref.DPM2S_2) for o in ("x0", "aux")} | {(ref.DPM2M, ("out_aux", "aux")), (ref.DPM2M, ("out", "aux"))}
        | {(ref.LMS, (o, f"hist{k}")) for o in ("out", "out_aux") for k in range(3)})
    print(f"{len(CASES)} cases in {len(cases.FAMILIES)} families: " +
          ", ".join(f"{f} {sum(c.family == f for c in CASES)}" for f in cases.FAMILIES))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_emulation_has_the_reference_bits(case):
    got = cases.build(case).to("cpu")
    cases.launch(emu, case, got)
    cases.check(case, got, cases.reference(case))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_is_finite(case):
    want = cases.reference(case)
    for o in ("out", "out_aux"):
        if o == "out" or case.writes_aux:
            assert torch.isfinite(want.view(o)).all(), f"{case.name}: {o} of the reference is not finite — re-seed the case"


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_reference_is_the_formula_in_float64(case):
    """A sanity check of the reference, not the kernel's gate.  The bound is not a constant: sampler_exit_ref.Tracked evaluates the
    header's formula in float64 and carries, per element, the error the fp32 evaluation can have under the standard model — each
    of the n fp32 roundings on the path contributes 2^-24 of its float64 intermediate's magnitude, and each later operation
    scales what came before by its other operand (a division by sigma in [0.5, 1.5) up to doubles it, scale = 5 multiplies it by 5).
    The float64 evaluation's own roundings (2^-53 each) are covered by the factor 1.001."""
    data = cases.build(case)
    n = ref.ROUNDINGS_D + ref.ROUNDINGS_UPDATE[case.mode]
    for name, got, tr in zip(("out", "out_aux"), cases.outputs(case, data), cases.outputs(case, data, tracked=True)):
        if got is None:
            continue
        err = (got.double() - tr.val).abs()
        bound = tr.err.expand_as(err) * 1.001 + 1e-300
        assert torch.isfinite(bound).all() and (err <= bound).all(), \
            f"{case.name} {name}: |fp32 - float64| {err.max().item():.3e} exceeds its bound at {int((err > bound).sum())} elements"
        # ... and it is no loose bound: at most (roundings on the longest path) x 2^-24 x (largest output) x 64, where 64 covers what
        # the later operations multiply an early rounding by: |scale| <= 5, 1 / sigma <= 2, |dt| or a coefficient <= 2.2 (product 22),
        # and intermediates larger than the output they cancel into
        flat = n * ref.U32 * max(1.0, tr.val.abs().max().item()) * 64.0
        assert bound.max().item() <= flat, f"{case.name} {name}: bound {bound.max().item():.3e} above {flat:.3e}"
    print(f"{case.name}: {n} roundings on the longest path, worst |fp32 - float64| / bound {float((err / bound).max()):.3f}")


def test_selector_coverage_is_counted():
    """every selecting vector of every selecting mode: every T >= 3 launch holds a positive frame and one of 0.0 / -0.0 / negative,
    all three kinds occur among the launches, and the pure selectors (only they) have a NaN frame"""
    for mode, ks in SELECTING.items():
        for k in ks:
            kinds, both, nan, all_in_one = set(), 0, 0, 0
            for c in CASES:
                if c.mode != mode or c.nv <= k:
                    continue
                v = cases.build(c).view(f"v{k}")
                taken, zero, negzero, neg = v > 0, (v == 0) & ~torch.signbit(v), (v == 0) & torch.signbit(v), v < 0
                if c.shape[0] >= 3:
                    assert taken.any() and (zero | negzero | neg).any(), f"{c.name}: v[{k}] takes one side only"
                    both += 1
                    all_in_one += bool(zero.any() and negzero.any() and neg.any())
                kinds |= {n for n, m in (("0.0", zero), ("-0.0", negzero), ("negative", neg)) if m.any()}
                nan += bool(torch.isnan(v).any())
            print(f"{ref.MODE_NAMES[mode]} v[{k}]: {both} launches take both sides, {all_in_one} hold all of 0.0 / -0.0 / negative, {nan} a NaN frame")
            assert both and kinds == {"0.0", "-0.0", "negative"}
            assert (nan > 0) == (k in PURE.get(mode, ())), f"{ref.MODE_NAMES[mode]} v[{k}]: NaN frames {nan}"
    for c in CASES:                                   # DPM2S_2: v[2] and v[4] independently — all four combinations in one launch at T = 5
        if c.mode == ref.DPM2S_2 and c.shape[0] == 5:
            a, b = cases.build(c).view("v2") > 0, cases.build(c).view("v4") > 0
            assert {(bool(p), bool(q)) for p, q in zip(a, b)} == {(True, True), (True, False), (False, True), (False, False)}
    for c in CASES:                                   # the divisors of selected paths
        if c.mode in (ref.HEUN1, ref.EULER_A, ref.DPM2S_1, ref.LMS):
            v0 = cases.build(c).view("v0")
            assert ((v0 >= 0.5) & (v0 < 1.5)).all()


@pytest.mark.parametrize("mutant", sorted(ref.MUTANTS))
def test_wrong_kernels_are_seen(mutant):
    """the model differs from the reference in at least one compared element (out or out_aux; the margins are the same) of every
    family it applies to; prints the differing elements per family and the range per case"""
    lines, unseen = [], []
    for fam in MUTANT_FAMILIES[mutant]:
        per_case = []
        for c in CASES:
            if c.family == fam:
                compared, diff = cases.count(c, cases.reference(c, mutant=mutant), cases.reference(c))
                per_case.append((diff, compared))
        total = sum(d for d, _ in per_case)
        hit = [d for d, _ in per_case if d]
        lines.append(f"{mutant} | {fam} | {total} of {sum(n for _, n in per_case)} elements differ, in {len(hit)} of {len(per_case)} cases"
                     + (f" ({min(hit)}..{max(hit)} per case)" if hit else ""))
        if not total:
            unseen.append(fam)
    print("\n".join(lines))
    assert not unseen, f"{mutant} ({ref.MUTANTS[mutant]}) has the reference's bits in all of {unseen}:\n" + "\n".join(lines)


def test_whole_fma_mutant_changes_a_tenth_to_a_half_of_a_plane():
    """the contraction the 2e-5 trajectory tolerances cannot see: how much of one plane it changes, and by how little"""
    for c in CASES:
        if c.family.startswith("grid-") and c.shape == cases.S1:
            w, m = cases.reference(c), cases.reference(c, mutant="fma_all")
            a, b = w.view("out"), m.view("out")
            diff = int((cases.bits(a) != cases.bits(b)).sum())
            print(f"{c.name}: fma_all changes {diff} of {a.numel()} out elements, by at most {torch.nan_to_num((a - b).abs()).max().item():.2e}")
            assert diff > 0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_poison_is_inert(case):
    """another poison pattern (a large finite value, which arithmetic would carry into an output) changes no output bit"""
    a, b = cases.reference(case), cases.reference(case, poison_bits=cases.OTHER_POISON_BITS)
    for o in ("out", "out_aux"):
        if o in a.span and (o == "out" or case.writes_aux):
            assert torch.equal(cases.bits(a.view(o)), cases.bits(b.view(o))), f"{case.name}: {o} depends on the poison"


@pytest.mark.parametrize("case", cases.UNUSED + cases.EULER, ids=[c.name for c in cases.UNUSED + cases.EULER])
def test_unused_operands_and_the_euler_entry_keep_the_base_bits(case):
    """poisoned planes for what a mode does not read, and the Euler entry: the output bits of the launch with None / of HEUN1"""
    a, b = cases.reference(case), cases.reference(cases.base_of(case))
    assert torch.equal(cases.bits(a.view("out")), cases.bits(b.view("out")))
    if case.writes_aux:
        assert torch.equal(cases.bits(a.view("out_aux")), cases.bits(b.view("out_aux")))
    for name in a.allocs:                           # what only the poisoned launch passes stays as it was
        if name not in b.allocs or (name == "out_aux" and not case.writes_aux):
            assert torch.equal(cases.bits(a.allocs[name]), cases.bits(cases.build(case).allocs[name])), name
