"""The GEMM family over the operand range, on the CPU (no kernel runs here; tests/test_gemm_range_gpu.py holds the kernels to the same
reference, bound and checks).  Cases: gemm_edge_cases.RANGE_CASES on the data sets RANGE_DATA.

  1. conditions on the inputs, from the operand planes and the float64 reference alone: the e4m3 A_lo planes carry clamped residuals,
     fp16-subnormal partners and every exponent field; w_lo_exp leaves [101, 127] on both sides; the graded outputs reach beyond the
     clamp and below fp16's normals, the pre-activations beyond +-88, the GEGLU gates beyond +-8; the bracket of the monitor is tight
  2. tests/emu.py (honest fp32) stays inside the bound on every launch and meets the exact statements of check_range
  3. the checks bite: nine wrong kernels are outside them on every launch they apply to — four that misread an operand
     (gemm_ref64.gemm(mutate=...)) against the bound, five that miswrite an output plane or miscount (gemm_ref64.model_outputs) against
     check_outputs / check_range; the unmutated model passes both with the exact monitor count
  4. the poison is inert for the reference"""
import pytest
import torch

import emu
import gemm_edge_cases as cases
import gemm_ref64 as ref64

RUNS, IDS = cases.RANGE_RUNS, cases.RANGE_IDS
reference = cases.reference


def _runs(pred):
    sel = [(c, d) for c, d in RUNS if pred(c, d)]
    return dict(argvalues=sel, ids=[f"{c.name}-{d}" for c, d in sel])


def _wide(c):
    return c.spec["range"] == "wide-rows"


def _lo8_out(c):
    return "lo8" in c.spec["epi"].split("+")


def _has(c, word):
    return word in c.spec["epi"].split("+")


# ------------------------------------------------------------------------------------------------------ 1. conditions on the inputs
@pytest.mark.parametrize("case,data", **_runs(lambda c, d: _wide(c) and c.spec.get("a_lo") == "e4m3"))
def test_wide_rows_e4m3_planes_cover_the_format(case, data):
    _, planes, _, _, w_exp = case.build(data)
    hi, lo = (planes[n].alloc[cases.MARGIN:-cases.MARGIN] for n in ("a16", "a16_lo"))
    real = ~torch.isnan(hi)                                    # (leading-dimension gaps are poison)
    hi, lo = hi[real], lo[real]
    assert planes["a16_lo"].clamped >= 0.05, planes["a16_lo"].clamped
    sub = (hi.float().abs() < 2.0 ** -14).float().mean().item()
    assert sub >= 0.10, sub
    fields = set(((lo >> 3) & 15).unique().tolist())
    assert fields == set(range(16)), sorted(fields)
    assert ((lo & 0x7F) == 0x7E).any() and not ((lo & 0x7F) == 0x7F).any()       # the 448 code occurs, the NaN code does not
    assert 1 <= w_exp <= 254


def test_wide_rows_w_lo_exp_leaves_the_unit_band():
    exps = sorted({c.build(d)[4] for c, d in RUNS if _wide(c) and c.spec.get("a_lo") == "e4m3"})
    print("w_lo_exp over the wide-rows cases:", exps)
    assert exps[0] <= 100 and exps[-1] >= 128
    w = torch.cat([c.build("wide-rows")[1]["w16"].alloc[cases.MARGIN:-cases.MARGIN] for c in cases.RANGE_CASES if _wide(c) and c.spec["g"] == -20])
    w = w[~torch.isnan(w)].float().abs()
    assert ((w > 0) & (w < 2.0 ** -14)).float().mean() > 0.5                      # g = -20: fp16-subnormal weights
    assert max(c.build("wide-rows")[1]["w16"].alloc.nan_to_num(0.0).abs().max().item() for c in cases.RANGE_CASES if _wide(c)) > 448.0


@pytest.mark.parametrize("case,data", **_runs(lambda c, d: not _wide(c) and _lo8_out(c)))
def test_graded_cols_lo8_outputs_leave_the_range(case, data):
    r = reference(case, data)
    v = r["v"][:, r["outs"]["out16_lo"][1]].abs()
    big, sub = (v >= 512.0).double().mean().item(), (v < 2.0 ** -14).double().mean().item()
    quads = ref64.monitor_bracket(r, "quads", slack=0.0)[0]   # what the float64 value itself clamps
    print(f"{case.name} [{data}] top grade {case.top[data]}: {100 * big:.1f} % at or above 512, {100 * sub:.1f} % fp16-subnormal, "
          f"{quads} clamped quads, max |v| {v.max().item():.6g}")
    assert big >= 0.03 and sub >= 0.10 and quads >= 100
    assert v.max() < 32768.0
    if "out32" not in r["outs"]:                               # the bracketed monitor case
        lower, upper = ref64.monitor_bracket(r, case.spec["unit"])
        print(f"the bracket of the monitor: [{lower}, {upper}]")
        assert lower > 0 and upper - lower <= 0.10 * lower, (lower, upper)


@pytest.mark.parametrize("case,data", **_runs(lambda c, d: not _wide(c) and (_has(c, "silu") or _has(c, "gelu") or _has(c, "geglu"))))
def test_graded_cols_activations_reach_their_tails(case, data):
    r = reference(case, data)
    x, edge = (r["gate"], 8.0) if r["geglu"] else (r["pre"], 88.0)
    assert (x > edge).any()
    if data == "graded-cols":                                  # (the positive variant has no negative pre-activations)
        assert (x < -edge).any()
        if _has(case, "silu") and not r["res_adds"]:
            assert ref64.silu_tail(r).any()


# ----------------------------------------------------------------------------------------- 2. honest fp32 is inside every check
_EMU_WORST = {}


@pytest.mark.parametrize("case,data", RUNS, ids=IDS)
def test_emulation_meets_every_check(case, data):
    r = reference(case, data)
    kw, allocs = case.launch(data)
    count = torch.zeros(2, dtype=torch.int32)
    emu.range_monitor_collect(count[:1])
    emu.gemm(**kw)
    emu.range_monitor_collect(count[1:])
    worst = cases.check_outputs(case, data, r, ref64.bound, kw, allocs)
    print(f"{case.name} [{data}] emu err / bound: " + ", ".join(f"{n} {v:.3g}" for n, v in worst.items()))
    # the emulation counts quads everywhere: where the kernel's unit is the element only (count > 0) == (the data clamps) is compared
    per_element = case.spec.get("unit") == "elements"
    expect = cases.check_range(case, data, r, kw, None if per_element else int(count[1]))
    if per_element:
        assert (int(count[1]) > 0) == (expect > 0)
    fam = _EMU_WORST.setdefault(case.family, {})
    for n, v in worst.items():
        fam[n] = max(fam.get(n, 0.0), v)


def test_emulation_ratio_per_family():
    """the table of DESIGN.md: worst err / bound of the emulation per case family (run with -s; after the test above)"""
    for fam, w in _EMU_WORST.items():
        print(f"{fam}: " + ", ".join(f"{n} {v:.3g}" for n, v in sorted(w.items())))
        assert max(w.values()) <= 1.0


# ------------------------------------------------------------------------------------------------------------ 3. the checks bite
def _over(case, data, mutate):
    r = reference(case, data)
    mut = ref64.gemm(**case.launch(data)[0], mutate=mutate)
    return ((mut["v"] - r["v"]).abs() > ref64.bound(r, "out32")).double().mean().item()


def _sharp(c, d):
    """the sharp check of the e4m3 lo pass: K = 48, positive data (2^-12 mag against a bound of 2 K_passes u mag)"""
    return _wide(c) and c.spec.get("a_lo") == "e4m3" and c.K == 48 and d == "wide-rows+"


@pytest.mark.parametrize("mutate", ["wexp_ignored", "wexp_off_by_one", "e4m3_fnuz"])
@pytest.mark.parametrize("case,data", **_runs(_sharp))
def test_a_wrong_lo_pass_is_outside_the_bound(case, data, mutate):
    assert case.build(data)[4] != 116          # (a condition on the cases: there `wexp_ignored` would be the correct kernel)
    frac = _over(case, data, mutate)
    print(f"{case.name} [{data}] {mutate} (w_lo_exp {case.build(data)[4]}): outside the bound on {100 * frac:.1f} % of the elements")
    assert frac > 0


@pytest.mark.parametrize("case,data", **_runs(lambda c, d: _wide(c) and c.spec["mode"] == cases.A_PLAIN))
def test_flushed_fp16_subnormal_operands_are_outside_the_bound(case, data):
    """rows of A below 2^-14 (and the weights at g = -20) read as 0: the row's sum is 0 against a bound relative to `mag` (the bias of
    the wide-rows cases is at the weights' scale, so that it does not own `mag`).  Plain A only: a row of a conv gather sums taps
    from pixels of several binades, and where a larger neighbour owns `mag` the flushed tap is below the bound."""
    frac = _over(case, data, "flush16_in")
    print(f"{case.name} [{data}] flush16_in: outside the bound on {100 * frac:.1f} % of the elements")
    assert frac > 0


def _model(case, data, mutate=None):
    r = reference(case, data)
    kw, allocs = case.launch(data)
    count = ref64.model_outputs(r, kw, case.spec.get("unit", "quads"), mutate)
    cases.check_outputs(case, data, r, ref64.bound, kw, allocs)
    cases.check_range(case, data, r, kw, count)


@pytest.mark.parametrize("case,data", RUNS, ids=IDS)
def test_exact_model_meets_every_check(case, data):
    _model(case, data)


OUT_MUTANTS = {                       # mutant -> the launches it applies to
    "flush16_out": lambda c, d: not _wide(c),
    "hi_rtz": lambda c, d: not _wide(c),
    "lo_sat_240": lambda c, d: _lo8_out(c) and _has(c, "o32"),        # (without out32 a clamp at 240 stays inside "degrades gracefully")
    "lo_unclamped": lambda c, d: _lo8_out(c),
    "monitor_per_element": lambda c, d: _lo8_out(c) and c.spec["unit"] == "quads",
}
_MUT_RUNS = [(m, c, d) for m, pred in OUT_MUTANTS.items() for c, d in RUNS if pred(c, d)]


@pytest.mark.parametrize("mutate,case,data", _MUT_RUNS, ids=[f"{m}-{c.name}-{d}" for m, c, d in _MUT_RUNS])
def test_wrong_writers_are_caught(mutate, case, data):
    with pytest.raises(AssertionError) as e:
        _model(case, data, mutate)
    print(f"{case.name} [{data}] {mutate}: {str(e.value)[:160]}")


def test_every_range_mutant_is_shown():
    assert set(OUT_MUTANTS) == set(ref64.RANGE_MUTANTS_OUT)
    assert set(ref64.RANGE_MUTANTS_IN) == {"wexp_ignored", "wexp_off_by_one", "e4m3_fnuz", "flush16_in"}


# ------------------------------------------------------------------------------------------------------ 4. the poison is inert
@pytest.mark.parametrize("case,data", RUNS, ids=IDS)
def test_poison_is_inert_for_the_reference(case, data):
    r = reference(case, data)
    z = ref64.gemm(**case.launch(data, zero_poison=True)[0])
    assert torch.isfinite(r["v"]).all()
    assert torch.equal(z["v"], r["v"]) and torch.equal(z["pre_mag"], r["pre_mag"])
    for n, (idx, cols) in r["outs"].items():
        assert torch.equal(z["outs"][n][0], idx) and z["outs"][n][1] == cols
