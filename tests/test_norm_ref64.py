"""The float64 norm references and the offset cases, checked on the CPU (no GPU needed).

  (a) tests/norm_ref64.py against torch.nn.functional.group_norm / layer_norm in float64 on permuted views, on every case shape
  (b) the generators of tests/norm_offset_cases.py realise the requested offset ratio r = |mean| / std within 10 %
  (c) the emulation (tests/emu.py: groupnorm_stats / apply / temporal_silu / layernorm / concat_add) stays within HALF of the
      bounds the kernels are held to
  (d) the bounds have teeth: two numpy fp32 models that walk the kernels' summation orders (per-(wave, channel) sequential sums,
      then the fixed-order group sum) — one with the raw-moment form sum x^2 - (sum x)^2 / n, one with the subtract-first form the
      kernels hold.  The raw-moment model must violate the statistics bound at r = 8 and r = 32 for the spatial GroupNorm, the
      temporal GroupNorm and the LayerNorm; the subtract-first model must pass at every r with at least 4x to spare."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import emu
import norm_offset_cases as cases
import norm_ref64 as ref64

f32 = np.float32


# ------------------------------------------------------------------------------------------ (a) the reference against torch
@pytest.mark.parametrize("F,Npix,C,ppc", cases.SPATIAL + cases.LADDER["spatial"])
def test_ref64_spatial_vs_torch(F, Npix, C, ppc):
    x = cases.spatial(F, Npix, C, 8.0)
    gamma, beta = cases.affine(C)
    want = TF.group_norm(x.double().view(F, Npix, C).permute(0, 2, 1), 32, gamma.double(), beta.double(), cases.EPS)
    for silu in (0, 1):
        y, xhat = ref64.groupnorm(x, C, F, Npix, C, gamma, beta, cases.EPS, silu)
        w = TF.silu(want) if silu else want
        assert (y.view(F, Npix, C).permute(0, 2, 1) - w).abs().max().item() < 1e-11
    assert (xhat * gamma.double() + beta.double() - want.permute(0, 2, 1).reshape(-1, C)).abs().max().item() < 1e-11
    # records -> combination = the statistics of the whole frame; a strided buffer reads the same values
    P = ref64.groupnorm_records(x, C, F, Npix, C, ppc)
    assert P.shape[1] == -(-Npix // ppc) and P[..., 0].sum(1).eq(Npix * (C // 32)).all()
    n, mean, var = ref64.combine_records(P)
    m64, v64 = ref64.groupnorm_sets(x, C, F, Npix, C)
    assert (mean - m64).abs().max().item() < 1e-12 * (1 + m64.abs().max().item()) and (var / v64.clamp_min(1e-300) - 1)[v64 > 0].abs().max().item() < 1e-11
    wide = torch.full((F * Npix, C + 8), float("nan"))
    wide[:, :C] = x
    assert torch.equal(ref64.groupnorm(wide, C + 8, F, Npix, C, gamma, beta, cases.EPS, 1)[0], ref64.groupnorm(x, C, F, Npix, C, gamma, beta, cases.EPS, 1)[0])


@pytest.mark.parametrize("B,T,Npix,C", cases.TEMPORAL + cases.LADDER["temporal"])
def test_ref64_temporal_vs_torch(B, T, Npix, C):
    x = cases.temporal(B, T, Npix, C, 8.0)
    gamma, beta = cases.affine(C)
    X = x.double().view(B, T, Npix, C).permute(0, 2, 3, 1).reshape(B * Npix, C, T)
    want = TF.silu(TF.group_norm(X, 32, gamma.double(), beta.double(), cases.EPS)).view(B, Npix, C, T).permute(0, 3, 1, 2)
    y, xhat = ref64.groupnorm_temporal_silu(x, B, T, Npix, C, gamma, beta, cases.EPS)
    assert y.shape == (B, T, Npix, C) and (y - want).abs().max().item() < 1e-11
    yp, xp = ref64.groupnorm_temporal_silu(x, B, T, Npix, C, gamma, beta, cases.EPS, t_pad=1)
    assert yp.shape == (B, T + 2, Npix, C) and torch.isnan(yp[:, 0]).all() and torch.isnan(yp[:, -1]).all() and torch.isnan(xp[:, 0]).all()
    assert torch.equal(yp[:, 1:T + 1], y) and torch.equal(xp[:, 1:T + 1], xhat)


@pytest.mark.parametrize("M,C", cases.LAYERNORM + cases.LADDER["layernorm"])
def test_ref64_layernorm_vs_torch(M, C):
    x = cases.row_sets(M, C, 8.0)
    gamma, beta = cases.affine(C)
    y, xhat = ref64.layernorm(x, C, M, C, gamma, beta, cases.EPS)
    assert (y - TF.layer_norm(x.double(), (C,), gamma.double(), beta.double(), cases.EPS)).abs().max().item() < 1e-11
    assert (xhat.mean(1).abs().max().item() < 1e-12) and ((xhat.pow(2).mean(1) - 1).abs().max().item() < 1e-3)


# ------------------------------------------------------------------------------------------ (b) the generator realises r
def _realised(mean, var, r):
    rr = cases.realised_r(mean, var)
    nz = var > 0
    assert (rr[nz] / r - 1).abs().max().item() < 0.1, (r, rr[nz].min().item(), rr[nz].max().item())
    return int((~nz).sum())


@pytest.mark.parametrize("r", cases.R)
def test_generators_realise_the_offset_ratio(r):
    for F, Npix, C, _ in cases.SPATIAL:
        assert _realised(*ref64.groupnorm_sets(cases.spatial(F, Npix, C, r), C, F, Npix, C), r) == 1        # one all-zero set
    for F, Npix, C1, C2, ctrl, _ in cases.CONCAT:
        a, s, c = cases.concat(F, Npix, C1, C2, ctrl, r)
        out = ref64.concat_add(a, C1, s, c, C2, F * Npix).float()
        assert _realised(*ref64.groupnorm_sets(out, C1 + C2, F, Npix, C1 + C2), r) == 1
    for B, T, Npix, C in cases.TEMPORAL:
        x = cases.temporal(B, T, Npix, C, r)
        mean, var = ref64.groupnorm_temporal_sets(x, B, T, Npix, C)
        assert _realised(mean, var, r) == 1
        # neighbouring sets have means of opposite sign
        assert (mean[:, :, 4] * mean[:, :, 5] < 0).all() and (mean[:, 2, 8] * mean[:, 3, 8] < 0).all()
    for M, C in cases.LAYERNORM:
        assert _realised(*ref64.layernorm_sets(cases.row_sets(M, C, r), C, M, C), r) == 0


# ------------------------------------------------------------------------------------------ (c) the emulation, half the bounds
def _half(tag, got, y64, xhat, gamma, r, lo=None):
    err, ratio = cases.output_excess(got, y64, xhat, gamma, r, lo, share=0.5)
    print(f"{tag} r={r:g}: emulation vs float64 max|err| {err:.3e} = {ratio:.3f} of floor + half the allowance")
    assert ratio <= 1.0, (tag, r, err, ratio)


@pytest.mark.parametrize("r", cases.R)
def test_emulation_within_half_of_the_bounds(r):
    _emulation_within_half(r, cases.SPATIAL, cases.CONCAT, cases.TEMPORAL, cases.LAYERNORM)


@pytest.mark.parametrize("r", cases.R)
def test_emulation_within_half_of_the_bounds_on_the_ladder(r):
    """cases.LADDER, the shapes tests/test_norm_offsets_gpu.py adds for the rungs of the host dispatch: the same walk"""
    _emulation_within_half(r, cases.LADDER["spatial"], [], cases.LADDER["temporal"], cases.LADDER["layernorm"])


def test_emulated_temporal_parts_within_half_of_the_bounds_on_the_ladder():
    """pnc_groupnorm_temporal_part mode 1 then 2 with every frame local, the way the GPU test calls the kernel (at cases.LADDER_PART_R)"""
    r = cases.LADDER_PART_R
    for B, T, Npix, C in cases.LADDER["temporal"]:
        x = cases.temporal(B, T, Npix, C, r)
        gamma, beta = cases.affine(C)
        y64, xhat = ref64.groupnorm_temporal_silu(x, B, T, Npix, C, gamma, beta, cases.EPS)
        stats = torch.zeros(B * Npix * 64)
        emu.groupnorm_temporal_part(x, B, T, Npix, C, gamma, beta, cases.EPS, stats, 1, T)
        for lo in (None, "f16", "e4m3"):
            y16 = torch.zeros(B * T * Npix, C, dtype=torch.float16)
            ylo = None if lo is None else torch.zeros(B * T * Npix, C, dtype=cases.LO_DTYPE[lo])
            emu.groupnorm_temporal_part(x, B, T, Npix, C, gamma, beta, cases.EPS, stats, 2, T, y16, ylo)
            _half(f"temporal part {B}x{T}x{Npix}x{C} lo={lo}", cases.joined(y16, ylo).view(B, T, Npix, C), y64, xhat, gamma, r, lo)


def _emulation_within_half(r, spatial, concat, temporal, layernorm):
    for F, Npix, C, ppc in spatial:
        x = cases.spatial(F, Npix, C, r)
        gamma, beta = cases.affine(C)
        nchunk = -(-Npix // ppc)
        part = torch.zeros(F * nchunk * 96)
        emu.groupnorm_stats(x, C, F, Npix, C, ppc, part)
        P64 = ref64.groupnorm_records(x, C, F, Npix, C, ppc)
        P = part.view(F, nchunk, 32, 3)
        assert torch.equal(P[..., 0].double(), P64[..., 0])
        v64 = P64[..., 2] / P64[..., 0]
        st = cases.stats_excess(P[..., 1], P[..., 2] / P[..., 0], P64[..., 1], v64, cases.realised_r(P64[..., 1], v64).nan_to_num(0.0))
        print(f"spatial {F}x{Npix}x{C} r={r:g}: emulated records var {st[0]:.2e} ({st[1]:.3f} of the bound), mean {st[2]:.2e} ({st[3]:.3f})")
        assert st[1] <= 0.5 and st[3] <= 0.5
        for silu in (0, 1):
            y64, xhat = ref64.groupnorm(x, C, F, Npix, C, gamma, beta, cases.EPS, silu)
            for lo in (None, "f16", "e4m3"):
                y16 = torch.zeros(F * Npix, C, dtype=torch.float16)
                ylo = None if lo is None else torch.zeros(F * Npix, C, dtype=cases.LO_DTYPE[lo])
                emu.groupnorm_apply(x, C, F, Npix, C, ppc, part, gamma, beta, cases.EPS, silu, y16, C, ylo)
                _half(f"spatial {F}x{Npix}x{C} silu={silu} lo={lo}", cases.joined(y16, ylo), y64, xhat, gamma, r, lo)
    for F, Npix, C1, C2, ctrl, ppc in concat:
        a, s, c = cases.concat(F, Npix, C1, C2, ctrl, r)
        C, M, nchunk = C1 + C2, F * Npix, -(-Npix // ppc)
        o32, part = torch.zeros(M, C), torch.zeros(F * nchunk * 96)
        emu.concat_add(a, C1, s, c, C2, M, o32, None, gn_part=part, frames=F, ppc=ppc)
        assert torch.equal(o32, ref64.concat_add(a, C1, s, c, C2, M).float())
        P64 = ref64.groupnorm_records(o32, C, F, Npix, C, ppc)
        P = part.view(F, nchunk, 32, 3)
        v64 = P64[..., 2] / P64[..., 0]
        st = cases.stats_excess(P[..., 1], P[..., 2] / P[..., 0], P64[..., 1], v64, cases.realised_r(P64[..., 1], v64).nan_to_num(0.0))
        assert st[1] <= 0.5 and st[3] <= 0.5, st
    for B, T, Npix, C in temporal:
        x = cases.temporal(B, T, Npix, C, r)
        gamma, beta = cases.affine(C)
        y64, xhat = ref64.groupnorm_temporal_silu(x, B, T, Npix, C, gamma, beta, cases.EPS)
        for lo in (None, "f16", "e4m3"):
            y16 = torch.zeros(B * T * Npix, C, dtype=torch.float16)
            ylo = None if lo is None else torch.zeros(B * T * Npix, C, dtype=cases.LO_DTYPE[lo])
            emu.groupnorm_temporal_silu(x, B, T, Npix, C, gamma, beta, cases.EPS, y16, ylo)
            _half(f"temporal {B}x{T}x{Npix}x{C} lo={lo}", cases.joined(y16, ylo).view(B, T, Npix, C), y64, xhat, gamma, r, lo)
    for M, C in layernorm:
        x = cases.row_sets(M, C, r)
        gamma, beta = cases.affine(C)
        y64, xhat = ref64.layernorm(x, C, M, C, gamma, beta, cases.EPS)
        for lo in (None, "f16"):
            y16 = torch.zeros(M, C, dtype=torch.float16)
            ylo = None if lo is None else torch.zeros(M, C, dtype=torch.float16)
            emu.layernorm(x, C, M, C, gamma, beta, cases.EPS, y16, C, ylo)
            _half(f"layernorm {M}x{C} lo={lo}", cases.joined(y16, ylo), y64, xhat, gamma, r, lo)


# ------------------------------------------------------------------------------------------ (d) fp32 models of the kernels' sums
def _fma(a, b, c):
    """fp32 fused multiply-add: the product of two fp32 values is exact in float64"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def _seq(a, axis):
    """fp32 sum along `axis`, one element after the other (np.sum would add pairwise)"""
    a = np.moveaxis(a, axis, 0)
    acc = np.zeros(a.shape[1:], f32)
    for k in range(a.shape[0]):
        acc = acc + a[k]
    return acc


def _wave_pixels(npix, w):
    return (npix - w + 3) // 4 if npix > w else 0


def spatial_record_raw(x):
    """gn_stats_kernel's raw-moment form: x fp32 [np, C] (one chunk of one frame) -> (n, mean, M2) per group.  Wave w of 4 adds
    pixels w, w + 4, ... per channel; one thread per group adds the [wave][channel] sums in that order."""
    npix, C = x.shape
    cpg = C // 32
    s, q = np.zeros((4, C), f32), np.zeros((4, C), f32)
    for p in range(npix):
        s[p % 4] = s[p % 4] + x[p]
        q[p % 4] = _fma(x[p], x[p], q[p % 4])
    ts = _seq(s.reshape(4, 32, cpg).transpose(1, 0, 2).reshape(32, 4 * cpg), 1)
    tq = _seq(q.reshape(4, 32, cpg).transpose(1, 0, 2).reshape(32, 4 * cpg), 1)
    n = f32(npix * cpg)
    mean = ts / n
    return n, mean, np.maximum(tq - ts * mean, f32(0))


def spatial_record_pivot(x):
    """the form gn_stats_kernel / concat_add_stats_kernel hold: sums of d = x - pivot per (wave, channel), the pivot of a channel
    pair its value at the wave's first pixel; m_wc = pivot + sum d / n_w; group mean = P + sum n_w (m_wc - P) / n with P the
    group's first m_0c; M2 = sum of M2_wc + n_w (m_wc - mean)^2 in the order (wave, channel)"""
    npix, C = x.shape
    cpg = C // 32
    s, q, pv = np.zeros((4, C), f32), np.zeros((4, C), f32), np.zeros((4, C), f32)
    for p in range(npix):
        w = p % 4
        if p < 4:
            pv[w] = np.repeat(x[p, 0::2], 2)
        d = x[p] - pv[w]
        s[w] = s[w] + d
        q[w] = _fma(d, d, q[w])
    nw = np.array([_wave_pixels(npix, w) for w in range(4)], f32)
    inw = np.where(nw > 0, f32(1) / np.maximum(nw, f32(1)), f32(0)).astype(f32)
    m = _fma(s, np.broadcast_to(inw[:, None], s.shape), pv)
    mg = m.reshape(4, 32, cpg)
    P = mg[0, :, 0]
    acc = np.zeros(32, f32)
    for w in range(4):
        acc = _fma(np.full(32, nw[w], f32), _seq(mg[w] - P[:, None], 1), acc)
    n = f32(npix * cpg)
    mean = P + acc / n
    dm = m - np.repeat(mean, cpg)[None, :]
    m2wc = np.maximum(_fma(-s * inw[:, None], s, q), f32(0))
    e = _fma(nw[:, None] * dm, dm, m2wc)
    return n, mean, _seq(e.reshape(4, 32, cpg).transpose(1, 0, 2).reshape(32, 4 * cpg), 1)


def chan_combine(recs):
    """gn_apply_kernel's combination of the chunk records of a frame (fp32, in chunk order; fewer than 8 chunks: a slice each, the
    merge of the slices is the same formula)"""
    n, mean, m2 = f32(0), np.zeros(32, f32), np.zeros(32, f32)
    for nb, mb, m2b in recs:
        nt = n + nb
        d = mb - mean
        w = nb / max(nt, f32(1))
        m2 = m2 + (m2b + d * d * (n * w))
        mean = _fma(d, np.full(32, w, f32), mean)
        n = nt
    return mean, m2 / n


def temporal_raw(x):
    """gn_temporal_kernel's raw-moment form (modes 1 and 2 still exchange these sums): x fp32 [sets, T, cpg] -> (mean, var)"""
    S, T, cpg = x.shape
    s, q = np.zeros((S, cpg // 2), f32), np.zeros((S, cpg // 2), f32)
    for t in range(T):
        s = s + (x[:, t, 0::2] + x[:, t, 1::2])
        q = _fma(x[:, t, 0::2], x[:, t, 0::2], q)
        q = _fma(x[:, t, 1::2], x[:, t, 1::2], q)
    n = f32(T * cpg)
    mean = _seq(s, 1) / n
    return mean, np.maximum(_seq(q, 1) / n - mean * mean, f32(0))


def temporal_two_pass(x):
    """gn_temporal_kernel mode 0: pair means as pivot + mean(x - pivot), group mean = P + mean(pair mean - P), then the squares of
    x - group mean per pair, added per group in pair order"""
    S, T, cpg = x.shape
    pv = x[:, 0, 0::2]
    s = np.zeros((S, cpg // 2), f32)
    for t in range(T):
        s = s + ((x[:, t, 0::2] - pv) + (x[:, t, 1::2] - pv))
    pm = _fma(s, np.full_like(s, f32(1) / f32(2 * T)), pv)
    P = pm[:, 0]
    mean = P + _seq(pm - P[:, None], 1) / f32(cpg // 2)
    q = np.zeros((S, cpg // 2), f32)
    for t in range(T):
        d0, d1 = x[:, t, 0::2] - mean[:, None], x[:, t, 1::2] - mean[:, None]
        q = _fma(d0, d0, q)
        q = _fma(d1, d1, q)
    return mean, _seq(q, 1) / f32(T * cpg)


def _butterfly(a):
    """__shfl_xor reduction over the last axis (a power of two of lanes): every lane ends with the same fp32 sum"""
    n = a.shape[-1]
    idx = np.arange(n)
    o = n // 2
    while o:
        a = a + a[..., idx ^ o]
        o //= 2
    return a[..., 0]


def layernorm_raw(x):
    """the fused LayerNorm of the GEMM epilogue (E_LN), rows of N = 320 under the 256x320 tile: two waves own 160 columns each, in
    slabs of 64, 64 and 32 columns; a lane adds the values and squares of 8 columns, the slab's lanes butterfly, slabs add up in
    order, the two waves' sums are added; var = E[x^2] - mean^2 with the product fused.  x fp32 [M, 320] -> (mean, var)"""
    M, N = x.shape
    assert N == 320
    tot = []
    for half in range(2):
        S, Q = np.zeros(M, f32), np.zeros(M, f32)
        c0 = half * 160
        for width in (64, 64, 32):
            blk = x[:, c0:c0 + width].reshape(M, width // 8, 8)
            sm, sq = np.zeros((M, width // 8), f32), np.zeros((M, width // 8), f32)
            for e in range(8):
                sm = sm + blk[:, :, e]
                sq = _fma(blk[:, :, e], blk[:, :, e], sq)
            S, Q = S + _butterfly(sm), Q + _butterfly(sq)
            c0 += width
        tot.append((S, Q))
    invn = f32(1) / f32(N)
    mean = (tot[0][0] + tot[1][0]) * invn
    return mean, np.maximum(_fma(-mean, mean, (tot[0][1] + tot[1][1]) * invn), f32(0))


def layernorm_two_pass(x):
    """layernorm_kernel: lane l of 64 owns the float4 vectors l, l + 64, ...; sum -> butterfly -> first mean m0, then the squares
    and the sum of x - m0 the same way: mean = m0 + mean(x - m0), var = mean((x - m0)^2) - mean(x - m0)^2.  x fp32 [M, C] -> (mean, var)"""
    M, C = x.shape
    J = -(-C // 256)
    v = np.zeros((M, J * 256), f32)
    v[:, :C] = x
    on = (np.arange(J * 256) < C).reshape(J, 64, 4)
    v = v.reshape(M, J, 64, 4)
    invc = f32(1) / f32(C)
    s = np.zeros((M, 64), f32)
    for j in range(J):
        s = s + ((v[:, j, :, 0] + v[:, j, :, 1]) + (v[:, j, :, 2] + v[:, j, :, 3]))
    m0 = _butterfly(s) * invc
    q, s1 = np.zeros((M, 64), f32), np.zeros((M, 64), f32)
    for j in range(J):
        for e in range(4):
            d = np.where(on[j, :, e], v[:, j, :, e] - m0[:, None], f32(0)).astype(f32)
            q = _fma(d, d, q)
            s1 = s1 + d
    dm = _butterfly(s1) * invc
    return m0 + dm, _fma(-dm, dm, _butterfly(q) * invc)


def _model_ratios(kind, r, draws):
    """-> worst (variance, mean) error of the raw-moment and of the subtract-first model as multiples of the statistics bound"""
    worst = {"raw": [0.0, 0.0], "kept": [0.0, 0.0]}
    for seed in range(draws):
        if kind == "spatial":                 # 2 chunks x 128 pixels x 10 channels per group, combined like gn_apply_kernel
            F, Npix, C = 1, 256, 320
            x = cases.spatial(F, Npix, C, r, seed=seed + 10, zero=False)
            m64, v64 = ref64.groupnorm_sets(x, C, F, Npix, C)
            got = {"raw": chan_combine([spatial_record_raw(x.numpy()[c * 128:(c + 1) * 128]) for c in range(2)]),
                   "kept": chan_combine([spatial_record_pivot(x.numpy()[c * 128:(c + 1) * 128]) for c in range(2)])}
            m64, v64 = m64.reshape(-1), v64.reshape(-1)
        elif kind == "temporal":              # T = 8 x 10 channels per group
            B, T, Npix, C = 1, 8, 16, 320
            x = cases.temporal(B, T, Npix, C, r, seed=seed + 20, zero=False)
            m64, v64 = (t.reshape(-1) for t in ref64.groupnorm_temporal_sets(x, B, T, Npix, C))
            xs = x.numpy().reshape(T, Npix * 32, 10).transpose(1, 0, 2)
            got = {"raw": temporal_raw(xs), "kept": temporal_two_pass(xs)}
        else:                                 # rows of 320
            M, C = 64, 320
            x = cases.row_sets(M, C, r, seed=seed + 30)
            m64, v64 = ref64.layernorm_sets(x, C, M, C)
            got = {"raw": layernorm_raw(x.numpy()), "kept": layernorm_two_pass(x.numpy())}
        for k, (mean, var) in got.items():
            st = cases.stats_excess(torch.from_numpy(np.asarray(mean, f32)), torch.from_numpy(np.asarray(var, f32)), m64, v64, r)
            worst[k] = [max(worst[k][0], st[1]), max(worst[k][1], st[3])]
    return worst


@pytest.mark.parametrize("kind", ["spatial", "temporal", "layernorm"])
def test_bounds_separate_raw_moments_from_subtract_first(kind):
    """LayerNorm: the subtract-first model is the stand-alone layernorm_kernel; the raw-moment model is the form the fused epilogue
    (E_LN) holds."""
    for r in cases.R:
        w = _model_ratios(kind, r, draws=8)
        print(f"{kind} r={r:g}: raw moments at {w['raw'][0]:.3f} (variance) / {w['raw'][1]:.3f} (mean) of the statistics bound; "
              f"subtract-first at {w['kept'][0]:.3f} / {w['kept'][1]:.3f} — {1 / max(w['kept']):.1f}x to spare")
        assert max(w["kept"]) <= 0.25, (kind, r, w)
        if r >= 8:
            assert w["raw"][0] > 1.0, (kind, r, w)
