"""The GEMM float64 reference, its bound and the edge cases, on the CPU (no kernel runs here; tests/test_gemm_edges_gpu.py holds the
kernels to the same reference and bound).

  1. the reference holds itself up: gemm_ref64 — flat-storage indexing from the header — against torch's float64 conv2d / conv1d /
     matmul on weights this file re-orders to OIHW by its own reading of the header, to 1e-12 relative
  2. tests/emu.py on the CPU (honest fp32) stays inside `bound` on every case and data set: the bound is attainable, and the
     builder's emulation agrees with the header
  3. the bound bites: an accumulator rounded to fp16 ahead of the epilogue is outside it on at least half of the elements of every
     short-K case; six further wrong kernels are outside it on their cases
  4. the poison is inert for the reference"""
import pytest
import torch
import torch.nn.functional as TF

import emu
import gemm_edge_cases as cases
import gemm_ref64 as ref64

CASES = cases.CASES
IDS = [c.name for c in CASES]
reference = cases.reference


# ------------------------------------------------------------------------------------------ 1. the reference against torch float64
def _torch_contraction(kw):
    """A W^T of the hi planes by torch's own float64 operators.  Layout knowledge used here, read from the header independently of
    gemm_ref64: NHWC image, K order (ky, kx, ci) or (ci/64, ky, kx, ci%64); the column block [2][F][Hin][Cin]; conv1d rows (b, t, p)."""
    M, N, K = kw["M"], kw["N"], kw["K"]
    a = kw["a16"].reshape(-1).double()
    W = torch.as_strided(kw["w16"].reshape(-1), (N, K), (kw.get("w_ld", 0) or K, 1)).double()
    if kw["a_mode"] == cases.A_PLAIN:
        return torch.as_strided(a, (M, K), (kw["lda"], 1)) @ W.t()
    if kw["a_mode"] == cases.A_CONV3X3:
        c = kw["conv"]
        C, Hin, Win, Hout, Wout = c["Cin"], c["Hin"], c["Win"], c["Hout"], c["Wout"]
        F = M // (Hout * Wout)
        x = a[: F * Hin * Win * C].view(F, Hin, Win, C).permute(0, 3, 1, 2)
        w = W.view(N, C // 64, 3, 3, 64).permute(0, 1, 4, 2, 3).reshape(N, C, 3, 3) if C % 64 == 0 else W.view(N, 3, 3, C).permute(0, 3, 1, 2)
        xh = c.get("x_halo_off", 0)
        side = [torch.zeros(F, C, Hin, 1, dtype=torch.float64)] * 2
        if xh:
            blk = a[xh: xh + 2 * F * Hin * C].view(2, F, Hin, C).permute(0, 1, 3, 2)
            side = [blk[0][..., None], blk[1][..., None]]
        x = torch.cat([side[0], x, side[1]], dim=3)                       # columns -1 .. Win
        if c.get("upsample"):
            x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)[..., 1:-1]      # nearest x2; columns -1 .. 2 Win
        if c.get("pad_br"):
            y = TF.conv2d(TF.pad(x[..., 1:-1], (0, 1, 0, 1)), w, stride=2)
        else:
            y = TF.conv2d(TF.pad(x, (0, 0, 1, 1)), w, stride=c["stride"])
        assert y.shape[2:] == (Hout, Wout)
        return y.permute(0, 2, 3, 1).reshape(M, N)
    t = kw["tconv"]
    C, T, Npix, halo = t["C"], t["T"], t["Npix"], t.get("halo", 0)
    B = M // (T * Npix)
    x = a.view(B, T + 2 * halo, Npix, C).permute(0, 2, 3, 1).reshape(B * Npix, C, T + 2 * halo)
    w = W.view(N, C // 64, 3, 64).permute(0, 1, 3, 2).reshape(N, C, 3) if C % 64 == 0 else W.view(N, 3, C).permute(0, 2, 1)
    y = TF.conv1d(x, w, padding=0 if halo else 1)
    return y.view(B, Npix, N, T).permute(0, 3, 1, 2).reshape(M, N)


_GEOMETRIES = {}
for _c in CASES:       # one case per distinct gather geometry (the epilogue and the lo planes do not enter the hi contraction)
    _s = _c.spec
    _GEOMETRIES.setdefault(repr((_s["mode"], _s["M"], _s["N"], _s["K"], _s.get("conv"), _s.get("tconv"), _s.get("x_halo"), _s.get("lda"))), _c)


@pytest.mark.parametrize("case", list(_GEOMETRIES.values()), ids=lambda c: c.name)
def test_reference_agrees_with_torch_float64(case):
    kw, _ = case.launch("signed", zero_poison=True)        # torch's operators read whole tensors: zeros in the slack, and see 4.
    keep = ("M", "N", "K", "lda", "a_mode", "conv", "tconv", "w_ld")
    want = _torch_contraction(kw)
    got = ref64.gemm(kw["a16"], kw["w16"], out32=True, ldc32=kw["N"], **{k: kw[k] for k in keep if k in kw})["v"]
    rel = ((got - want).abs().max() / want.abs().max()).item()
    assert rel < 1e-12, rel


def test_reference_epilogue_against_plain_formulae():
    """bias, rowbias row index, GEGLU block pairing, SiLU / GELU, residuals and the V^T address, spelled out element by element"""
    M, N, K = 12, 128, 16
    g = torch.Generator().manual_seed(5)
    a, w = torch.randn(M, K, generator=g).half(), torch.randn(N, K, generator=g).half()
    bias, rb, r1 = torch.randn(N, generator=g), torch.randn(3, N, generator=g), torch.randn(M, N + 4, generator=g)
    acc = a.double() @ w.double().t()
    r = ref64.gemm(a, w, M=M, N=N, K=K, lda=K, bias=bias, rowbias=rb, rb_rows=2, rb_mod=3, act=ref64.ACT_SILU, res1=r1, ldr1=N + 4,
                   out32=True, ldc32=N + 1)
    for m, n in ((0, 0), (5, 77), (11, 127)):
        pre = acc[m, n] + bias[n].double() + rb[(m // 2) % 3, n].double()
        assert abs(r["v"][m, n] - (pre / (1 + torch.exp(-pre)) + r1[m, n].double())) < 1e-12
        assert r["outs"]["out32"][0][m, n] == m * (N + 1) + n
    r = ref64.gemm(a, w, M=M, N=N, K=K, lda=K, bias=bias, geglu=True, out16=True, ldc16=N // 2)
    for m, n in ((0, 0), (3, 31), (7, 32), (11, 63)):
        val, gate = (acc[m, (n // 32) * 64 + off + n % 32] + bias[(n // 32) * 64 + off + n % 32].double() for off in (0, 32))
        assert abs(r["v"][m, n] - val * 0.5 * gate * (1 + torch.erf(gate / 2 ** 0.5))) < 1e-12
    r = ref64.gemm(a, w, M=M, N=N, K=K, lda=K, act=ref64.ACT_GELU, out16=True, ldc16=64, out16t=True, ldt=5, t_rows=4, t_gstride=700, n_split=0)
    idx, cols = r["outs"]["out16t"]
    assert cols == slice(0, N) and idx[9, 17] == (9 // 4) * 700 + 17 * 5 + 9 % 4
    assert abs(r["v"][9, 17] - acc[9, 17] * 0.5 * (1 + torch.erf(acc[9, 17] / 2 ** 0.5))) < 1e-12
    with pytest.raises(ValueError):
        ref64.gemm(a, w, M=M, N=N, K=K, lda=K, out32=True, ldc32=N, ln_out16=True)
    with pytest.raises(ValueError):
        ref64.gemm(a, w, M=M, N=N, K=K, lda=K, out32=True, ldc32=N, gn_part=True)


def test_reference_split_operand_sums():
    """the four contractions of the header on one small problem, from the planes' values"""
    from panacea_amd import engine
    M, N, K = 8, 16, 32
    g = torch.Generator().manual_seed(6)
    a32, w32 = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    ah, al = cases.split_planes(a32, "f16")
    _, a8 = cases.split_planes(a32, "e4m3")
    wh = w32.half()
    wl = ((w32 - wh.float()) * 2048).half()
    w8, e = engine.pk_lo8(wh)
    A, L, W, V = ah.double(), al.double(), wh.double(), wl.double()
    A8, W8 = cases.lo_values(a8).double(), cases.lo_values(w8).double() * 2.0 ** (e - 127)
    kw = dict(M=M, N=N, K=K, lda=K, out32=True, ldc32=N)
    S = 2.0 ** -11
    for extra, want, passes in ((dict(a16_lo=al), (A + S * L) @ W.t(), 2),
                                (dict(a16_lo=al, w_lo=wl), A @ W.t() + S * (L @ W.t() + A @ V.t()), 3),
                                (dict(a16_lo=al, w_lo16=wl), A @ W.t() + S * (L @ W.t() + A @ V.t()), 3),
                                (dict(w_lo16=wl), A @ W.t() + S * (A @ V.t()), 2),
                                (dict(a16_lo=a8, w_lo=(w8, e)), A @ W.t() + S * (A8 @ W8.t()), 2),
                                (dict(a16_lo=a8, w_lo=(w8, e), w_lo16=wl), A @ W.t() + S * (A8 @ W8.t() + A @ V.t()), 3)):
        r = ref64.gemm(ah, wh, **kw, **extra)
        assert (r["v"] - want).abs().max() < 1e-13 and r["K_passes"] == passes * K


# ------------------------------------------------------------------------------------------ 2. honest fp32 is inside the bound
_EMU_WORST = {}


@pytest.mark.parametrize("data", cases.DATA)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_emulation_stays_inside_the_bound(case, data):
    r = reference(case, data)
    kw, allocs = case.launch(data)
    emu.gemm(**kw)
    worst = cases.check_outputs(case, data, r, ref64.bound, kw, allocs)
    print(f"{case.name} [{data}] emu err / bound: " + ", ".join(f"{n} {v:.3g}" for n, v in worst.items()))
    fam = _EMU_WORST.setdefault(case.family, {})
    for n, v in worst.items():
        fam[n] = max(fam.get(n, 0.0), v)


def test_emulation_ratio_per_family():
    """the table of DESIGN.md: worst err / bound of the emulation per case family (run with -s; after the test above)"""
    for fam, w in _EMU_WORST.items():
        print(f"{fam}: " + ", ".join(f"{n} {v:.3g}" for n, v in sorted(w.items())))
        assert max(w.values()) <= 1.0


# ------------------------------------------------------------------------------------------ 3. the bound bites
def _sharpest(r):
    """the output through which a case shows its value most precisely"""
    return next(n for n in ("out32", "out16_lo", "out16", "out16t") if n in r["outs"])


def _over(case, data, mutate):
    """-> fraction of the elements of the case's sharpest output on which the mutant expectation is outside the bound"""
    r = reference(case, data)
    kw, _ = case.launch(data)
    mut = ref64.gemm(**kw, mutate=mutate)
    name = _sharpest(r)
    cols = r["outs"][name][1]
    return ((mut["v"][:, cols] - r["v"][:, cols]).abs() > ref64.bound(r, name)).double().mean().item()


@pytest.mark.parametrize("case", [c for c in CASES if c.K <= 576], ids=lambda c: c.name)
def test_fp16_staged_accumulator_is_outside_the_bound(case):
    """A condition on the cases, not a measurement: with positive data a kernel that rounds its accumulator to fp16 before the epilogue
    leaves the bound on at least half of the elements of every case with K <= 576."""
    frac = _over(case, "positive", "acc16")
    print(f"{case.name}: fp16-staged accumulator outside the bound on {100 * frac:.0f} % of the elements")
    assert frac >= 0.5, frac


def _find(prefix):
    """the one case whose name starts with `prefix` (the conv cases' N follows from their place in the list)"""
    hit = [c for c in CASES if c.name == prefix or c.name.startswith(prefix + "-")]
    assert len(hit) == 1, (prefix, hit)
    return hit[0]


@pytest.mark.parametrize("mutate,name", [
    ("drop_last_chunk", "plain-t1-N200-o32"), ("drop_last_chunk", "conv1d-T3-C24-bias+r1+r2+o32+o16"),
    ("halo_zero", "conv3x3-s1-9x11-halo-C8"), ("halo_zero", "conv3x3-s2-9x11-halo-C64"), ("halo_zero", "conv3x3-up-5x7-halo-C24"),
    ("halo_zero", "stencil-16x16-C64-N320-bias+o32-halo"),
    ("ignore_pad_br", "conv3x3-padbr-9x11-C8"), ("ignore_pad_br", "conv3x3-padbr-8x10-C64"),
    ("rb_mod_m", "plain-t3-N320-bias+rb+r1alias+r2+o32"), ("rb_mod_m", "conv1d-T2-C64-bias+r1alias+rb+o32"),
    ("geglu_halves", "plain-t4-N512-geglu"),
    ("frame_neighbour", "conv3x3-s1-9x11-C24"), ("frame_neighbour", "stencil-8x32-C128-N192-bias+r1alias+o32+o16-alo16"),
    ("frame_neighbour", "conv1d-T3-C128-bias+r1alias+rb+o32"), ("frame_neighbour", "conv1d-T1-C64-bias+r1+r2+o32+o16"),
])
@pytest.mark.parametrize("data", cases.DATA)
def test_wrong_kernels_are_outside_the_bound(mutate, name, data):
    frac = _over(_find(name), data, mutate)
    print(f"{name} [{data}] {mutate}: outside the bound on {100 * frac:.1f} % of the elements")
    assert frac > 0


# ------------------------------------------------------------------------------------------ 4. the poison is inert
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_poison_is_inert_for_the_reference(case):
    r = reference(case, "signed")
    kw, _ = case.launch("signed", zero_poison=True)
    z = ref64.gemm(**kw)
    assert torch.isfinite(r["v"]).all()
    assert torch.equal(z["v"], r["v"]) and torch.equal(z["pre_mag"], r["pre_mag"])
    for n, (idx, cols) in r["outs"].items():
        assert torch.equal(z["outs"][n][0], idx) and z["outs"][n][1] == cols
