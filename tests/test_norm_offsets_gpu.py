"""Norm statistics against float64 on offset data (MI355X): every producer and consumer of GroupNorm / LayerNorm statistics at
offset ratios r = |mean| / std of 0.5, 8 and 32.

Reference: tests/norm_ref64.py (float64, independent of tests/emu.py).  Data and bounds: tests/norm_offset_cases.py — the bounds are
derived there from the fp32 format and the structure of a subtract-first variance, not measured on these kernels; a raw-moment
variance (sum x^2 - (sum x)^2 / n) breaks them from r = 8 on (tests/test_norm_ref64.py shows both on the CPU).  Shapes: the smallest
that reach every kernel template and guard (named at each test)."""
import pytest
import torch

import norm_offset_cases as cases
import norm_ref64 as ref64
from helpers import measured
from panacea_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
TILES = {"128x128": 1, "256x128": 2, "256x320": 3, "256x256": 4}


def _lo_plane(lo, rows, C):
    return None if lo is None else torch.zeros(rows, C, device=DEV, dtype=cases.LO_DTYPE[lo])


def _check_output(tag, hi, lo_t, lo, y64, xhat, gamma, r, kernel):
    got = cases.joined(hi, lo_t).view_as(y64)
    assert torch.isfinite(got[~torch.isnan(y64)]).all(), f"{tag}: non-finite output"
    err, ratio = cases.output_excess(got, y64, xhat, gamma, r, lo)
    print(f"{tag}: {kernel} vs float64 max|err| {err:.3e}, {ratio:.3f} of the output bound")
    measured("norm_offsets " + tag.replace(" ", "_"), kernel=kernel, max_err=err, of_bound=ratio)
    assert ratio <= 1.0, f"{tag}: max|err| {err:.4e} is {ratio:.3f} of the bound"


def _check_records(tag, part, P64, kernel):
    """{n, mean, M2} per (frame, chunk, group) against float64 under the statistics bound, r = the chunk's own realised ratio"""
    P = part.view(P64.shape).cpu()
    assert torch.isfinite(P).all(), f"{tag}: non-finite records"
    assert torch.equal(P[..., 0].double(), P64[..., 0]), f"{tag}: record counts"
    v64 = P64[..., 2] / P64[..., 0]
    r_rec = cases.realised_r(P64[..., 1], v64).nan_to_num(0.0)
    ev, rv, em, rm = cases.stats_excess(P[..., 1], P[..., 2] / P[..., 0], P64[..., 1], v64, r_rec)
    print(f"{tag}: {kernel} records vs float64: variance {ev:.3e} ({rv:.3f} of the bound), mean {em:.3e} sigma ({rm:.3f})")
    measured("norm_offsets " + tag.replace(" ", "_"), kernel=kernel, var_rel_err=ev, var_of_bound=rv, mean_err_sigma=em, mean_of_bound=rm)
    assert rv <= 1.0 and rm <= 1.0, f"{tag}: variance {ev:.3e} = {rv:.3f} of the bound, mean {em:.3e} sigma = {rm:.3f} of the bound"


# ------------------------------------------------------------------------------------------ pnc_groupnorm_stats + pnc_groupnorm_apply
# J = 1, 2, 5, 8, 12 float4 vectors per lane; 10 channels per group (a float4 straddles two groups); a last chunk of ONE pixel
# (129 = 128 + 1, 77 = 4 * 16 + 13, 130 = 2 * 64 + 2: waves without a pixel give n = 0 partials); 18 chunks (1100 / 64: every slice
# of the combination walks three)
@pytest.mark.parametrize("r", cases.R)
@pytest.mark.parametrize("F,Npix,C,ppc", cases.SPATIAL)
def test_groupnorm_spatial_offsets(F, Npix, C, ppc, r):
    x = cases.spatial(F, Npix, C, r)
    gamma, beta = cases.affine(C)
    P64 = ref64.groupnorm_records(x, C, F, Npix, C, ppc)
    outs = [ref64.groupnorm(x, C, F, Npix, C, gamma, beta, cases.EPS, silu) for silu in (0, 1)]
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    nchunk = -(-Npix // ppc)
    part = torch.full((F * nchunk * 96,), float("nan"), device=DEV)
    part2 = torch.full_like(part, float("nan"))
    hip.groupnorm_stats(xd, C, F, Npix, C, ppc, part)
    hip.groupnorm_stats(xd, C, F, Npix, C, ppc, part2)
    torch.cuda.synchronize()
    tag = f"spatial {F}x{Npix}x{C} ppc{ppc} r={r:g}"
    assert torch.equal(part, part2), f"{tag}: the records are not reproducible"
    _check_records(tag, part, P64, "gn_stats_kernel")
    for silu in (0, 1):
        y64, xhat = outs[silu]
        for lo in (None, "f16", "e4m3"):
            y = torch.full((F * Npix, C), float("nan"), device=DEV, dtype=torch.float16)
            ylo = _lo_plane(lo, F * Npix, C)
            hip.groupnorm_apply(xd, C, F, Npix, C, ppc, part, gd, bd, cases.EPS, silu, y, C, ylo)
            torch.cuda.synchronize()
            _check_output(f"{tag} silu={silu} lo={lo}", y, ylo, lo, y64, xhat, gamma, r, "gn_apply_kernel")


# ------------------------------------------------------------------------------------------ pnc_concat_add_stats
# S = 1, 2, 4 channel slices; 1280 + 640: the boundary between the two sources lies inside a group of 60 channels
@pytest.mark.parametrize("r", cases.R)
@pytest.mark.parametrize("F,Npix,C1,C2,ctrl,ppc", cases.CONCAT)
def test_concat_add_records_offsets(F, Npix, C1, C2, ctrl, ppc, r):
    C, M, nrec = C1 + C2, F * Npix, -(-Npix // ppc)
    a, s, c = cases.concat(F, Npix, C1, C2, ctrl, r)
    want = ref64.concat_add(a, C1, s, c, C2, M).float()
    m64, v64 = ref64.groupnorm_sets(want, C, F, Npix, C)
    rr = cases.realised_r(m64, v64)
    assert ((rr / r - 1).abs()[v64 > 0] < 0.1).all()
    gamma, beta = cases.affine(C)
    o32 = torch.full((M, C), float("nan"), device=DEV)
    o16 = torch.zeros(M, C, device=DEV, dtype=torch.float16)
    part = torch.full((F * nrec * 96,), float("nan"), device=DEV)
    hip.concat_add(a.to(DEV), C1, s.to(DEV), None if c is None else c.to(DEV), C2, M, o32, o16, gn_part=part, frames=F, ppc=ppc)
    torch.cuda.synchronize()
    tag = f"concat {F}x{Npix}x({C1}+{C2}) ppc{ppc} r={r:g}"
    assert torch.equal(o32.cpu(), want), f"{tag}: the concatenated values"
    _check_records(tag, part, ref64.groupnorm_records(want, C, F, Npix, C, ppc), "concat_add_stats_kernel")
    y64, xhat = ref64.groupnorm(want, C, F, Npix, C, gamma, beta, cases.EPS, 1)
    y = torch.full((M, C), float("nan"), device=DEV, dtype=torch.float16)
    hip.groupnorm_apply(o32, C, F, Npix, C, 128, part, gamma.to(DEV), beta.to(DEV), cases.EPS, 1, y, C, n_records=nrec)
    torch.cuda.synchronize()
    _check_output(f"{tag} apply", y, None, None, y64, xhat, gamma, r, "gn_apply_kernel on the concat's records")


# ------------------------------------------------------------------------------------------ pnc_groupnorm_temporal_silu
# T = 1: two values per group at C = 64; T <= 8 (two items per lane) and T > 8 (one); 16 pixels per block with a ragged last block
# (77 = 4 * 16 + 13 at C = 64), 6 per block at C = 320, 1 at C = 1280 and 2048
@pytest.mark.parametrize("r", cases.R)
@pytest.mark.parametrize("B,T,Npix,C", cases.TEMPORAL)
def test_groupnorm_temporal_offsets(B, T, Npix, C, r):
    x = cases.temporal(B, T, Npix, C, r)
    gamma, beta = cases.affine(C)
    y64, xhat = ref64.groupnorm_temporal_silu(x, B, T, Npix, C, gamma, beta, cases.EPS)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    for lo in (None, "f16", "e4m3"):
        y = torch.full((B * T * Npix, C), float("nan"), device=DEV, dtype=torch.float16)
        ylo = _lo_plane(lo, B * T * Npix, C)
        hip.groupnorm_temporal_silu(xd, B, T, Npix, C, gd, bd, cases.EPS, y, ylo)
        torch.cuda.synchronize()
        _check_output(f"temporal {B}x{T}x{Npix}x{C} lo={lo} r={r:g}", y, ylo, lo, y64, xhat, gamma, r, "gn_temporal_kernel")


# ------------------------------------------------------------------------------------------ pnc_layernorm
@pytest.mark.parametrize("r", cases.R)
@pytest.mark.parametrize("M,C", cases.LAYERNORM)
def test_layernorm_offsets(M, C, r):
    """the stand-alone kernel, the peer of the GEMM's fused LayerNorm below"""
    x = cases.row_sets(M, C, r)
    gamma, beta = cases.affine(C)
    y64, xhat = ref64.layernorm(x, C, M, C, gamma, beta, cases.EPS)
    for lo in (None, "f16"):
        y = torch.full((M, C), float("nan"), device=DEV, dtype=torch.float16)
        ylo = _lo_plane(lo, M, C)
        hip.layernorm(x.to(DEV), C, M, C, gamma.to(DEV), beta.to(DEV), cases.EPS, y, C, ylo)
        torch.cuda.synchronize()
        _check_output(f"layernorm {M}x{C} lo={lo} r={r:g}", y, ylo, lo, y64, xhat, gamma, r, "layernorm_kernel")


# ------------------------------------------------------------------------------------------ every rung of the host dispatch
# cases.LADDER: the J rungs and frame counts the shapes above leave out; the same references and bounds
@pytest.mark.parametrize("r", cases.R)
@pytest.mark.parametrize("F,Npix,C,ppc", cases.LADDER["spatial"])
def test_ladder_groupnorm_spatial(F, Npix, C, ppc, r):
    test_groupnorm_spatial_offsets(F, Npix, C, ppc, r)


@pytest.mark.parametrize("r", cases.R)
@pytest.mark.parametrize("M,C", cases.LADDER["layernorm"])
def test_ladder_layernorm(M, C, r):
    test_layernorm_offsets(M, C, r)


@pytest.mark.parametrize("r", cases.R)
@pytest.mark.parametrize("B,T,Npix,C", cases.LADDER["temporal"])
def test_ladder_groupnorm_temporal(B, T, Npix, C, r):
    test_groupnorm_temporal_offsets(B, T, Npix, C, r)


@pytest.mark.parametrize("B,T,Npix,C", cases.LADDER["temporal"])
def test_ladder_groupnorm_temporal_part(B, T, Npix, C):
    """pnc_groupnorm_temporal_part, mode 1 then mode 2 with every frame local (T_total = T): the output of
    pnc_groupnorm_temporal_silu, under the same bound"""
    r = cases.LADDER_PART_R
    x = cases.temporal(B, T, Npix, C, r)
    gamma, beta = cases.affine(C)
    y64, xhat = ref64.groupnorm_temporal_silu(x, B, T, Npix, C, gamma, beta, cases.EPS)
    xd, gd, bd = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    stats = torch.full((B * Npix * 64,), float("nan"), device=DEV)
    hip.groupnorm_temporal_part(xd, B, T, Npix, C, gd, bd, cases.EPS, stats, 1, T)
    for lo in (None, "f16", "e4m3"):
        y = torch.full((B * T * Npix, C), float("nan"), device=DEV, dtype=torch.float16)
        ylo = _lo_plane(lo, B * T * Npix, C)
        hip.groupnorm_temporal_part(xd, B, T, Npix, C, gd, bd, cases.EPS, stats, 2, T, y, ylo)
        torch.cuda.synchronize()
        _check_output(f"temporal part {B}x{T}x{Npix}x{C} lo={lo} r={r:g}", y, ylo, lo, y64, xhat, gamma, r, "gn_temporal_kernel modes 1, 2")


# ------------------------------------------------------------------------------------------ channels with gamma = 0
def test_zero_gamma_channels():
    """cases.affine keeps |gamma| >= 0.5; here every 8th channel has gamma = 0: the allowance vanishes there, the output is beta (or
    SiLU(beta)) under the format's floor alone — a wrong beta or a gamma of the wrong channel shows at once."""
    r = 8.0
    F, Npix, C, ppc = 2, 300, 320, 128
    gamma, beta = cases.affine(C, zero_every=8)
    gd, bd = gamma.to(DEV), beta.to(DEV)
    x = cases.spatial(F, Npix, C, r)
    part = torch.zeros(F * 3 * 96, device=DEV)
    hip.groupnorm_stats(x.to(DEV), C, F, Npix, C, ppc, part)
    for silu in (0, 1):
        y64, xhat = ref64.groupnorm(x, C, F, Npix, C, gamma, beta, cases.EPS, silu)
        y = torch.full((F * Npix, C), float("nan"), device=DEV, dtype=torch.float16)
        hip.groupnorm_apply(x.to(DEV), C, F, Npix, C, ppc, part, gd, bd, cases.EPS, silu, y, C)
        torch.cuda.synchronize()
        _check_output(f"zero gamma spatial silu={silu}", y, None, None, y64, xhat, gamma, r, "gn_apply_kernel")
    B, T, Np = 1, 3, 33
    xt = cases.temporal(B, T, Np, C, r)
    y64, xhat = ref64.groupnorm_temporal_silu(xt, B, T, Np, C, gamma, beta, cases.EPS)
    y = torch.full((B * T * Np, C), float("nan"), device=DEV, dtype=torch.float16)
    hip.groupnorm_temporal_silu(xt.to(DEV), B, T, Np, C, gd, bd, cases.EPS, y)
    torch.cuda.synchronize()
    _check_output("zero gamma temporal", y, None, None, y64, xhat, gamma, r, "gn_temporal_kernel")
    M = 513
    xl = cases.row_sets(M, C, r)
    y64, xhat = ref64.layernorm(xl, C, M, C, gamma, beta, cases.EPS)
    y = torch.full((M, C), float("nan"), device=DEV, dtype=torch.float16)
    hip.layernorm(xl.to(DEV), C, M, C, gd, bd, cases.EPS, y, C)
    torch.cuda.synchronize()
    _check_output("zero gamma layernorm", y, None, None, y64, xhat, gamma, r, "layernorm_kernel")


# ------------------------------------------------------------------------------------------ LayerNorm of a GEMM's output rows
def _scaled_product(M, N, K, seed, target):
    """fp16 A [M, K], W [N, K] whose product has elements of about `target` in size: unit A, W of target / sqrt(K)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g).half(), (torch.randn(N, K, generator=g) * (target * K ** -0.5)).half()


@pytest.mark.parametrize("r", cases.R)
@pytest.mark.parametrize("kind", ["res", "rowbias"])
@pytest.mark.parametrize("M,N,K,tile", [(300, 64, 64, "128x128"), (777, 128, 192, "128x128"), (1000, 320, 320, "256x320")])
def test_gemm_trailing_layernorm_offsets(M, N, K, tile, kind, r):
    """out = A W^T + bias + res (or + rowbias) with ln_out16 and PNC_OPT_GEMM_FUSE_LN = 0 (pnc_gemm_fuses_layernorm says so): the
    LayerNorm kernel after the GEMM.  The offsets arrive through res1 / rowbias, the product is a tenth of the smallest sigma so
    that it moves no row's ratio by 10 %.  ln_out16 against the float64 LayerNorm of the launch's OWN out32 under the fp16 bound.

    NOT held to this bound: the same launches with the LayerNorm fused into the epilogue (E_LN), whose variance is still
    E[x^2] - mean^2.  Measured on these shapes, as multiples of the bound: 0.998 at r = 0.5, 0.99 .. 1.11 at r = 8, 1.9 .. 4.6 at
    r = 32 (max|err| 2.2e-3 .. 3.0e-3 of the fp16 output, where the kernel after the GEMM stays at 0.95 .. 0.998)."""
    a, w = _scaled_product(M, N, K, 11, 0.02)
    gamma, beta = cases.affine(N)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(12)) * 0.02
    kw = dict(a16=a.to(DEV), w16=w.to(DEV), M=M, N=N, K=K, lda=K, bias=bias.to(DEV), ldc32=N, ln_gamma=gamma.to(DEV), ln_beta=beta.to(DEV),
              ldln=N, ln_eps=cases.EPS)
    if kind == "res":
        o32 = cases.row_sets(M, N, r, seed=13).to(DEV)
        kw.update(res1=o32, ldr1=N)
    else:       # 4 rows of rowbias, row m gets rowbias[(m / 100) % 4]: every output row is one of four offset rows + the product
        o32 = torch.full((M, N), float("nan"), device=DEV)
        kw.update(rowbias=cases.row_sets(4, N, r, seed=14).to(DEV), rb_rows=100, rb_mod=4)
    ln = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float16)
    kw.update(out32=o32, ln_out16=ln)
    prev_tile, prev = hip.set_option(hip.OPT_GEMM_TILE, TILES[tile]), hip.set_option(hip.OPT_GEMM_FUSE_LN, 0)
    try:
        assert not hip.gemm_fuses_layernorm(**kw)
        hip.gemm(**kw)
        torch.cuda.synchronize()
    finally:
        hip.set_option(hip.OPT_GEMM_FUSE_LN, prev)
        hip.set_option(hip.OPT_GEMM_TILE, prev_tile)
    o32 = o32.cpu()
    m64, v64 = ref64.layernorm_sets(o32, N, M, N)
    assert ((cases.realised_r(m64, v64) / r - 1).abs() < 0.1).all(), "the product moved a row's offset ratio by more than 10 %"
    y64, xhat = ref64.layernorm(o32, N, M, N, gamma, beta, cases.EPS)
    _check_output(f"gemm + layernorm {M}x{N}x{K} {tile} {kind} r={r:g}", ln, None, None, y64, xhat, gamma, r, "layernorm_kernel after the gemm")


# ------------------------------------------------------------------------------------------ the temporal conv's records
@pytest.mark.parametrize("r", cases.R)
@pytest.mark.parametrize("B,T,Npix,C,epi", [(1, 2, 640, 640, "rb"), (1, 4, 1024, 320, "r2+o16")])
def test_gemm_conv1d_records_offsets(B, T, Npix, C, epi, r):
    """PncGemmParams.gn_part with PNC_OPT_GEMM_GN_STATS = 0: out = conv1d_t(x) + bias (+ rowbias) + res1 (+ res2) with the offsets in
    res1; the records of the launch's OWN fp32 output per (frame, 64-pixel block, group), written by the statistics launch after
    the GEMM, under the statistics bound; the output is the launch's without gn_part to the bit, also with the records taken from
    the epilogue (E_GS, PNC_OPT_GEMM_GN_STATS = 1 on the 256x320 tile, which these small shapes get only when it is asked for).
    640 pixels = 2.5 tiles per frame: a tile's wave blocks belong to two frames.

    NOT held to the bound: the records of E_GS itself, still raw moments (the same sums as the statistics kernel held before:
    4e-5 .. 1e-4 at r = 8, 6e-4 .. 1.5e-3 at r = 32 there).  A subtract-first E_GS measured 1.2e-6 / 1.6e-6 at r = 8 / 32 and was not
    kept: its kernels gained spills (profiles/norm_offsets_codeobj.md)."""
    F, M, N, K = B * T, B * T * Npix, C, 3 * C
    x, w = _scaled_product(M, N, K, 21, 0.02)
    x = x[:, :C].contiguous()
    g = torch.Generator().manual_seed(22)
    bias, emb, skip = torch.randn(N, generator=g) * 0.02, torch.randn(F, N, generator=g) * 0.02, torch.randn(M, N, generator=g) * 0.02
    res = cases.spatial(F, Npix, C, r, seed=23, zero=False).to(DEV)       # (a GEMM output has no all-zero set)
    kw = dict(a16=x.to(DEV), w16=w.to(DEV), M=M, N=N, K=K, a_mode=hip.A_CONV1D_T, tconv=dict(C=C, T=T, Npix=Npix), bias=bias.to(DEV), ldr1=N, ldc32=N)
    if epi == "rb":
        kw.update(rowbias=emb.to(DEV), rb_rows=Npix, rb_mod=F)
    else:
        kw.update(res2=skip.to(DEV), ldr2=N, out16=torch.zeros(M, N, device=DEV, dtype=torch.float16), ldc16=N)
    nrec = Npix // 64

    def run(opt, with_part):
        prev, prev_tile = hip.set_option(hip.OPT_GEMM_GN_STATS, opt), hip.set_option(hip.OPT_GEMM_TILE, TILES["256x320"] if opt else 0)
        try:
            out = res.clone()
            part = torch.full((F * nrec * 96,), float("nan"), device=DEV) if with_part else None
            hip.gemm(res1=out, out32=out, gn_part=part, **kw)
            torch.cuda.synchronize()
        finally:
            hip.set_option(hip.OPT_GEMM_GN_STATS, prev)
            hip.set_option(hip.OPT_GEMM_TILE, prev_tile)
        return out, part
    for opt in (1, 0):
        plain, _ = run(opt, False)
        out, part = run(opt, True)
        assert torch.equal(out, plain), f"GN_STATS={opt}: the output changed with gn_part"
        assert torch.isfinite(part).all()
    o32 = plain.cpu()
    m64, v64 = ref64.groupnorm_sets(o32, C, F, Npix, C)
    assert ((cases.realised_r(m64, v64) / r - 1).abs() < 0.1).all(), "the product moved a set's offset ratio by more than 10 %"
    _check_records(f"conv1d records {B}x{T}x{Npix}x{C} {epi} GN_STATS=0 r={r:g}", part, ref64.groupnorm_records(o32, C, F, Npix, C, 64),
                   "gn_stats_kernel after the gemm")
