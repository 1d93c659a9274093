"""The float64 references of the helpers and the row softmax (tests/misc_ref64.py) and their bounds, on the CPU:
  1. the references agree with torch float64 / exact formulations written independently (no shared indexing code);
  2. tests/emu.py's counterparts stay within HALF of each allowance on every case and data set of tests/misc_edge_cases.py (the output
     format's own half step, where there is one, is not halved: an honest fp16 rounding reaches it), and reproduce every exact output;
  3. the poison is inert for the reference, the reference alone is finite everywhere, and no written element is skipped or written twice;
  4. the bounds bite: each wrong kernel below — what a plausible slip in csrc/misc.hip would compute — is outside on at least one case."""
import math

import pytest
import torch
import torch.nn.functional as TF

import emu
import misc_edge_cases as cases
import misc_ref64 as ref64

BY = cases.BY_NAME


def _strided64(t, R, C, ld):
    return torch.as_strided(t.reshape(-1), (R, C), (ld, 1)).double()


# ------------------------------------------------------------------------------------------ 1. independent formulations
@pytest.mark.parametrize("name", ["linear-K520-N5-M7-silu11-pm30", "linear-K1288-N320-M16-wlo", "linear-K8-N1-M1-bias", "linear-K72-N5-M7-nobias"])
def test_linear_reference_is_the_float64_linear(name):
    case = BY[name]
    s = case.spec
    t, _ = case.launch("signed")
    ex = case.reference("signed")[0]["out32"]
    M, N, K = s["Mtot"], s["N"], s["K"]
    A = _strided64(t["a32"], M, K, K + 4)
    W = t["w16"].double().view(N, K)
    if "w_lo" in t:
        W = W + t["w_lo"].double().view(N, K) / 2048.0
    y = TF.linear(TF.silu(A) if s.get("silu_in") else A, W, t["bias"].double() if "bias" in t else None)
    y = TF.silu(y) if s.get("silu_out") else y
    assert torch.allclose(ex.v, y, rtol=1e-12, atol=1e-13)
    assert torch.equal(ex.idx, torch.arange(M).view(M, 1) * (N + 3) + torch.arange(N))
    assert (ex.allow > 0).all()


def test_segment_layout_is_the_headers():
    """out[seg_start[s] * Mtot + (m0 + m) * width_s + (n - seg_start[s])], element by element in plain Python"""
    case = BY["segments-4+8+64-K72-Mtot21"]
    t, _ = case.launch("signed")
    ex = case.reference("signed")[0]["out32"]
    A = _strided64(t["a32"], 21, 72, 76)
    y = TF.linear(TF.silu(A), t["w16"].double().view(76, 72), t["bias"].double())
    starts = [0, 4, 12, 76]
    want = torch.full((76 * 21,), float("nan"), dtype=torch.float64)
    for si in range(3):
        for m in range(21):
            for n in range(starts[si], starts[si + 1]):
                want[starts[si] * 21 + m * (starts[si + 1] - starts[si]) + (n - starts[si])] = y[m, n]
    got = torch.full_like(want, float("nan"))
    got[ex.idx.reshape(-1)] = ex.v.reshape(-1)
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-13)                # (no NaN left: every element of the output is written)


@pytest.mark.parametrize("name", ["embed-i64-dim7-F5", "embed-f32-dim320-F5", "embed-i64-dim2-F1-t3"])
def test_embedding_reference(name):
    case = BY[name]
    t, _ = case.launch("t")
    ex = case.reference("t")[0]["out32"]
    dim, half = case.spec["dim"], case.spec["dim"] // 2
    arg = t["t"].float()[:, None] * t["freqs"][None, :]                    # the reference project's fp32 product
    want = torch.cat([torch.cos(arg.double()), torch.sin(arg.double()), torch.zeros(arg.shape[0], dim - 2 * half, dtype=torch.float64)], dim=1)
    assert torch.equal(ex.v, want)
    assert (ex.allow[:, :2 * half] == 2.0 ** -22).all() and (ex.allow[:, 2 * half:] == 0).all()


@pytest.mark.parametrize("name", ["nchw-F4-af2-scale-C19+4-pad24-Npix77", "nchw-F4-af2-scale-C4+4-pad8-Npix77-lo", "nchw-F2-af1-scale-C4+4-pad8-Npix77-lo"])
def test_nchw_reference_is_a_scaled_permutation(name):
    case = BY[name]
    s = case.spec
    t, _ = case.launch("v")
    ex = case.reference("v")[0]
    F, af, C1, C2, Npix, Cpad = s["F"], s["af"], s["C1"], s["C2"], s["Npix"], s["Cpad"]
    a = t["a32"].view(af, C1, Npix).repeat(F // af, 1, 1) * t["a_scale"].view(F, 1, 1)              # fp32 product
    v = torch.zeros(F, Npix, Cpad)
    v[:, :, :C1] = a.permute(0, 2, 1)
    v[:, :, C1:C1 + C2] = t["b32"].view(F, C2, Npix).permute(0, 2, 1)
    assert torch.equal(cases.bits(ex["out16"].exact), cases.bits(v.half()))
    assert torch.equal(ex["out16"].idx.reshape(-1), torch.arange(F * Npix * Cpad))
    assert ("out16_lo" in ex) == s["lo"]
    if s["lo"]:
        assert torch.equal(cases.bits(ex["out16_lo"].exact), cases.bits(((v - v.half().float()) * 2048.0).half()))


def test_tokens_to_nchw_reference_is_a_permutation():
    case = BY["tokens_to_nchw-C4-ld9-Npix257"]
    t, _ = case.launch("v")
    ex = case.reference("v")[0]["out32"]
    want = torch.as_strided(t["x32"], (2, 257, 4), (257 * 9, 9, 1)).permute(0, 2, 1)
    assert torch.equal(ex.exact, want) and torch.equal(ex.idx.reshape(-1), torch.arange(2 * 4 * 257))


@pytest.mark.parametrize("name", ["concat-C68+4-M300-c-o32-loe4m3", "concat-C4+68-M1-noc-o32-loe4m3", "add-n1028-loe4m3", "add-n1028-lof16-inplace", "cast-n4-loe4m3"])
def test_elementwise_references_are_fp32_torch(name):
    case = BY[name]
    s = case.spec
    t, _ = case.launch("v")
    ex, clamped = case.reference("v")
    if case.fn == "concat":
        sv = t["s32"] + t["c32"] if "c32" in t else t["s32"]
        v = torch.cat([t["a32"].view(s["M"], s["C1"]), sv.view(s["M"], s["C2"])], dim=1)
    else:
        v = t["x32"] + t["a32"] if "a32" in t else t["x32"].clone()
    hi = v.half()
    r = (v - hi.float()) * 2048.0
    if "out32" in ex:
        assert torch.equal(cases.bits(ex["out32"].exact.reshape(-1)), cases.bits(v.reshape(-1)))
    assert torch.equal(cases.bits(ex["out16"].exact.reshape(-1)), cases.bits(hi.reshape(-1)))
    lo = ex["out16_lo"].exact.reshape(-1)
    if s["lo"] == "f16":
        assert torch.equal(cases.bits(lo), cases.bits(r.half().reshape(-1))) and clamped == 0
    else:
        assert torch.equal(lo, r.clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8).reshape(-1))
        assert clamped == int((r.abs() > 448).reshape(-1, 4).any(1).sum())


def test_e4m3_cases_clamp_a_known_number_of_quads():
    """the special values 700.24, -1200.4, 60007.3 lie off the fp16 grid where its step is >= 0.5: their residual is beyond 448"""
    seen = 0
    for case in cases.CASES:
        if case.spec.get("lo") == "e4m3":
            clamped = case.reference("v")[1]
            assert clamped >= 1, case.name
            seen += 1
    assert seen >= 20
    assert BY["cast-n1028-loe4m3"].reference("v")[1] == 3        # 700.24 | -1200.4 | 60007.3 in quads 0, 1 and 2


@pytest.mark.parametrize("name", [c.name for c in cases.CASES if c.fn == "softmax" and c.spec["N"] <= 1028])
def test_softmax_reference_is_the_masked_float64_softmax(name):
    case = BY[name]
    s = case.spec
    M, N = s["M"], s["N"]
    for data in case.data:
        t, _ = case.launch(data)
        ex = case.reference(data)[0]["p16"]
        keep = cases.visible(M, N, s["n_valid"], s["causal"])
        S = _strided64(t["s32"], M, N, s["lds"]).nan_to_num(0.0, 0.0, 0.0)
        sc = float(torch.tensor(s["scale"]).float())
        want = torch.softmax((sc * S).masked_fill(~keep, -math.inf), dim=1)
        assert torch.allclose(ex.v, want, rtol=1e-12, atol=0.0)
        assert (ex.v[~keep] == 0).all() and (ex.bound()[~keep] == 0).all() and (ex.bound()[keep] > 0).all()
        assert torch.equal(ex.idx, torch.arange(M).view(M, 1) * s["ldp"] + torch.arange(N))
        if s["scale"] in (0.0, 1e-38):         # uniform over the visible columns
            assert torch.equal(ex.v, keep.double() / keep.sum(1, keepdim=True))


# ------------------------------------------------------------------------------------------ 2. the emulation, 3. poison and coverage
@pytest.mark.parametrize("case,data", cases.RUNS, ids=cases.RUN_IDS)
def test_emulation_within_half_the_allowance(case, data):
    ex, clamped = case.reference(data)
    t, allocs = case.launch(data)
    before = torch.zeros(1, dtype=torch.int32)
    emu.range_monitor_collect(before)
    case.call(emu, t)
    cases.check_outputs(case, data, ex, t, allocs, share=0.5)
    count = torch.zeros(1, dtype=torch.int32)
    emu.range_monitor_collect(count)
    assert int(count) == clamped


@pytest.mark.parametrize("case,data", cases.RUNS, ids=cases.RUN_IDS)
def test_poison_is_inert_and_every_written_element_is_checked(case, data):
    ex, clamped = case.reference(data)
    z, zc = cases._REF[case.fn](case.spec, case.launch(data, zero_poison=True)[0])
    assert zc == clamped and set(z) == set(ex)
    outs = case.build(data)[1]
    assert set(ex) == set(outs), "an output of the launch has no expectation"
    for name, e in ex.items():
        assert torch.isfinite(e.v).all(), f"{name}: the reference is not finite"
        assert torch.equal(e.idx, z[name].idx) and torch.equal(e.v, z[name].v)
        flat = e.idx.reshape(-1)
        assert flat.unique().numel() == flat.numel() and 0 <= int(flat.min()) and int(flat.max()) < outs[name].n
        if e.exact is not None:
            assert torch.equal(cases.bits(e.exact), cases.bits(z[name].exact)) and e.exact.shape == e.idx.shape
            if e.exact.dtype != torch.uint8:
                assert torch.isfinite(e.exact.float()).all()
        else:
            assert torch.isfinite(e.bound()).all() and (e.bound() >= 0).all() and e.v.shape == e.idx.shape == e.bound().shape
            assert torch.equal(e.bound(), z[name].bound())


# ------------------------------------------------------------------------------------------ 4. the bounds bite
def _outside(case, data, fill):
    """`fill(case, t)` writes a wrong kernel's outputs into the tensors of a launch -> True when check_outputs refuses them"""
    t, allocs = case.launch(data)
    fill(case, t)
    try:
        cases.check_outputs(case, data, case.reference(data)[0], t, allocs)
    except AssertionError:
        return True
    return False


def _linear_model(stage16=False, bias_after=False, lo_scale=2.0 ** -11, drop_tail=False):
    """fp32 torch model of linear_smallm_kernel with one slip"""
    def fill(case, t):
        s = case.spec
        M, N, K = s["Mtot"], s["N"], s["K"]
        A = torch.as_strided(t["a32"], (M, K), (K + 4, 1))
        A = TF.silu(A) if s.get("silu_in") else A
        W = t["w16"].float().view(N, K)
        if "w_lo" in t:
            W = W + t["w_lo"].float().view(N, K) * lo_scale
        Ke = K - K % 512 if drop_tail else K
        acc = A[:, :Ke] @ W[:, :Ke].t()
        if stage16:
            acc = acc.half().float()
        b = t["bias"] if "bias" in t else 0.0
        y = (TF.silu(acc) + b) if bias_after else (TF.silu(acc + b) if s.get("silu_out") else acc + b)
        torch.as_strided(t["out32"], (M, N), (N + 3, 1)).copy_(y)
    return fill


def _embed_model(swap=False, shift=False):
    def fill(case, t):
        F, dim = case.spec["F"], case.spec["dim"]
        half = dim // 2
        fr = torch.cat([t["freqs"][1:], t["freqs"][-1:] * 0.5]) if shift else t["freqs"]
        arg = t["t"].float()[:, None] * fr[None, :]
        c, s = torch.cos(arg), torch.sin(arg)
        o = t["out32"].view(F, dim)
        o[:, :half], o[:, half:2 * half] = (s, c) if swap else (c, s)
        o[:, 2 * half:] = 0.0
    return fill


def _nchw_model(scale_mod=False, a_plain=False):
    def fill(case, t):
        s = case.spec
        F, af, C1, C2, Npix, Cpad = s["F"], s["af"], s["C1"], s["C2"], s["Npix"], s["Cpad"]
        a = torch.cat([t["a32"].view(af, C1, Npix), torch.full((F - af, C1, Npix), float("nan"))])      # frames >= a_frames: the poisoned margin
        fi = torch.arange(F)
        a = a[fi if a_plain else fi % af]
        if "a_scale" in t:
            a = a * t["a_scale"][fi % af if scale_mod else fi].view(F, 1, 1)
        v = torch.zeros(F, Npix, Cpad)
        v[:, :, :C1] = a.permute(0, 2, 1)
        if C2:
            v[:, :, C1:C1 + C2] = t["b32"].view(F, C2, Npix).permute(0, 2, 1)
        t["out16"].view(F, Npix, Cpad).copy_(v.half())
        if "out16_lo" in t:
            t["out16_lo"].view(F, Npix, Cpad).copy_(((v - v.half().float()) * 2048.0).half())
    return fill


def _softmax_model(causal_shift=0, predicate=True, fma=True, sum16=False):
    """fp32 torch model of softmax_rows_kernel: the -3.0e38 stand-in under the maximum, sc = scale * log2 e, exp2(fma(s, sc, -max sc)),
    the fp32 sum, one reciprocal.  predicate = False: the stand-in alone masks (the kernel before the predicate); fma = False: the
    product rounded before the subtraction; sum16: the sum taken over fp16-rounded powers"""
    def fill(case, t):
        s = case.spec
        M, N = s["M"], s["N"]
        m, j = torch.arange(M).view(M, 1), torch.arange(N).view(1, N)
        vis = j < (s["n_valid"] if s["n_valid"] > 0 else N)
        if s["causal"]:
            vis = vis & (j <= m + causal_shift)
        v = torch.where(vis, torch.as_strided(t["s32"], (M, N), (s["lds"], 1)), torch.tensor(-3.0e38))
        mx = v.amax(dim=1, keepdim=True)
        sc = torch.tensor(s["scale"], dtype=torch.float32) * torch.tensor(ref64.LOG2E, dtype=torch.float32)
        off = mx * sc
        x = (v.double() * sc.double() - off.double()).float() if fma else v * sc - off
        e = torch.exp2(x)
        if predicate:
            e = torch.where(vis, e, torch.zeros(()))
        tot = (e.half().float() if sum16 else e).sum(dim=1, keepdim=True)
        torch.as_strided(t["p16"], (M, N), (s["ldp"], 1)).copy_((e * (1.0 / tot)).half())
    return fill


SOFTMAX_RUNS = [(c, d) for c, d in cases.RUNS if c.fn == "softmax"]


def test_kernel_models_are_inside_the_bound():
    """the models above WITHOUT a slip are inside on every case: what the mutants below leave is the slip's doing"""
    for case, data in SOFTMAX_RUNS:
        assert not _outside(case, data, _softmax_model()), (case.name, data)
    for case, data in cases.RUNS:
        if case.fn == "linear" and not case.spec.get("segs"):
            assert not _outside(case, data, _linear_model()), (case.name, data)
        if case.fn == "embed":
            assert not _outside(case, data, _embed_model()), case.name
        if case.fn == "nchw":
            assert not _outside(case, data, _nchw_model()), case.name


def _count(runs, fill):
    hit = [f"{c.name}[{d}]" for c, d in runs if _outside(c, d, fill)]
    print(f"outside the bound on {len(hit)} of {len(runs)} runs" + (f", e.g. {hit[0]}" if hit else ""))
    return len(hit)


def _runs(pred):
    return [(c, d) for c, d in cases.RUNS if pred(c)]


@pytest.mark.parametrize("mutant", ["stage16", "bias_after_silu_out", "w_lo_2^-10", "last_k_chunk_dropped", "cos_sin_swapped", "freqs_j+1",
                                    "a_scale[f%a_frames]", "a[f]", "causal_off_by_one", "sentinel_mask_at_scale_0", "no_fma_on_offset_data",
                                    "sum_over_fp16_probabilities"])
def test_wrong_kernels_are_outside_the_bound(mutant):
    plain = lambda c: c.fn == "linear" and not c.spec.get("segs")                          # noqa: E731
    runs, fill = {
        "stage16": (_runs(plain), _linear_model(stage16=True)),
        "bias_after_silu_out": (_runs(lambda c: plain(c) and c.spec.get("silu_out")), _linear_model(bias_after=True)),
        "w_lo_2^-10": (_runs(lambda c: plain(c) and c.spec.get("w_lo")), _linear_model(lo_scale=2.0 ** -10)),
        "last_k_chunk_dropped": (_runs(lambda c: plain(c) and c.spec["K"] % 512 and c.spec["K"] > 512), _linear_model(drop_tail=True)),
        "cos_sin_swapped": (_runs(lambda c: c.fn == "embed"), _embed_model(swap=True)),
        "freqs_j+1": (_runs(lambda c: c.fn == "embed" and c.spec["dim"] > 2), _embed_model(shift=True)),
        "a_scale[f%a_frames]": (_runs(lambda c: c.fn == "nchw" and c.spec["scale"] and c.spec["af"] < c.spec["F"]), _nchw_model(scale_mod=True)),
        "a[f]": (_runs(lambda c: c.fn == "nchw" and c.spec["af"] < c.spec["F"]), _nchw_model(a_plain=True)),
        "causal_off_by_one": ([r for r in SOFTMAX_RUNS if r[0].spec["causal"]], _softmax_model(causal_shift=1)),
        "sentinel_mask_at_scale_0": ([r for r in SOFTMAX_RUNS if r[0].spec["scale"] in (0.0, 1e-38) and "masked" in r[0].name],
                                     _softmax_model(predicate=False)),
        "no_fma_on_offset_data": ([r for r in SOFTMAX_RUNS if r[1] == "offset"], _softmax_model(fma=False)),
        "sum_over_fp16_probabilities": (SOFTMAX_RUNS, _softmax_model(sum16=True)),
    }[mutant]
    assert len(runs) > 0
    hits = _count(runs, fill)
    assert hits >= 1
