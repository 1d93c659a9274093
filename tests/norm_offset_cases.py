"""Offset data and derived bounds for the normalisation tests (tests/test_norm_ref64.py on the CPU, tests/test_norm_offsets_gpu.py
on the MI355X).

DATA.  A normalised set is a (frame, group) of the spatial GroupNorm, a (sample, pixel, group) of the temporal one, a row of a
LayerNorm.  Every set gets its own standard deviation sigma in [0.25, 2] and the mean +- r sigma, r = |mean| / std the OFFSET RATIO
of the case (R: 0.5 — what the rest of the suite draws — 8 and 32); the sign alternates between neighbouring sets, so a channel
counted into the wrong group is grossly wrong.  The unit draws are standardised per set in float64, so the realised ratio is the
requested one up to the fp32 rounding of the values (also for sets of two values).  Spatial and temporal cases hold one all-zero
set: var = 0 with n > 0, the output there is exactly SiLU(beta) / beta.

BOUNDS, derived — nothing here was measured on the code under test.  A form that subtracts (a pivot, a local mean) before it
squares never sees the offset in its squares; the offset enters once, when a mean of the size of r sigma is rounded to fp32:
2^-24 |mean| = 2^-24 r sigma.  That error enters the variance linearly (through the distance of partial means), next to the
r-independent 2^-24-per-operation error of the sums.  Raw moments, sum x^2 - (sum x)^2 / n, subtract two numbers (1 + r^2) times
the result: r^2 2^-24 times the growth of the accumulation.  Allowed:
    statistics   |var / var64 - 1| <= 2^-20 (1 + r)          |mean - mean64| <= 2^-21 (1 + r) sigma
    outputs      |y - y64| <= floor(y64) + 1.1 |gamma| (2^-21 (1 + r) |xhat| + 2^-21 (1 + r))
The first output term is the variance's share (half the relative variance error, times |xhat|), the second the mean's, 1.1 is
SiLU's Lipschitz constant.  floor = what the output FORMAT cannot resolve: half an fp16 ulp of y64 for an fp16 output; for a
reconstructed hi + lo / 2048 pair the floors of tests/test_lo8_gpu.py — 6e-5 + 6e-5 |y64| (e4m3 lo plane), 2^-20 max(1, |y64|)
(fp16 lo plane).  torch's own fp32 group_norm / layer_norm sit at 1.3e-6 / 3.7e-6 / 1.4e-5 max error on this data for
r = 0.5 / 8 / 32: inside.  For a RECORD of a pixel chunk r is the chunk's own realised ratio (a chunk of one pixel of a two-channel
group is a set of two values: its std is not the frame's)."""
import torch

R = (0.5, 8.0, 32.0)
GROUPS = 32
EPS = 1e-5

# the shapes of tests/test_norm_offsets_gpu.py (tests/test_norm_ref64.py walks the same ones on the CPU)
SPATIAL = [(2, 129, 64, 128), (2, 300, 320, 128), (1, 77, 1280, 16), (1, 1100, 320, 64), (1, 130, 1920, 64), (1, 70, 2560, 16)]   # F, Npix, C, ppc
CONCAT = [(2, 100, 320, 320, True, 64), (1, 70, 1280, 640, False, 16), (1, 65, 1280, 1280, True, 64)]        # F, Npix, C1, C2, ctrl, ppc
TEMPORAL = [(2, 1, 77, 64), (1, 3, 33, 320), (2, 8, 21, 1280), (1, 9, 19, 320), (1, 16, 5, 2048)]                # B, T, Npix, C
LAYERNORM = [(7, 64), (513, 320), (33, 1280), (5, 3072)]                                                         # M, C
# The rungs of the host dispatch the shapes above do not reach.  The row kernels are instantiated for J = 1, 2, 3, 5, 8, 12 float4
# vectors per lane and a row of C channels needs ceil(C / 256): C = 1024 / 1536 / 2048 / 2304 need 4 / 6 / 8 / 9 and run on 5 / 8 / 8 /
# 12 (GroupNorm: C = 640 needs 3).  The temporal kernel is instantiated per frame count, 1 .. 16, in three modes.  A wrong rung drops
# or repeats channels (frames): these are the smallest shapes that show it.  Data, references and bounds are their neighbours'.
LADDER = {"layernorm": [(5, C) for C in (1024, 1536, 2048, 2304)],                                               # M, C
          "spatial": [(1, 70, C, 16) for C in (640, 1024, 1536, 2304)],                                          # F, Npix, C, ppc
          "temporal": [(1, T, 5, 64) for T in range(1, 17)]}                                                     # B, T, Npix, C
# pnc_groupnorm_temporal_part walks the temporal shapes at LADDER_PART_R only: modes 1 and 2 exchange raw moments (sum x, sum x^2), a
# form that the bounds here separate from the kernels' own from r = 8 on (tests/test_norm_ref64.py, temporal_raw).  r = 0.5 is what
# the rest of the suite draws for it, and the rung does not depend on r.
LADDER_PART_R = 0.5


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _unit(g, *shape):
    """float64 draws, standardised over the last axis: mean 0, biased variance 1"""
    z = torch.randn(*shape, generator=g, dtype=torch.float64)
    z = z - z.mean(-1, keepdim=True)
    return z / z.pow(2).mean(-1, keepdim=True).sqrt()


def _sigma(g, *shape):
    return 0.25 + 1.75 * torch.rand(*shape, generator=g, dtype=torch.float64)


def _sign(*axes):
    """+-1, alternating along every axis: axes = 1-D index tensors already shaped for broadcasting"""
    return 1.0 - 2.0 * (sum(axes) % 2).double()


def affine(C, seed=5, zero_every=0):
    """gamma, beta of a norm: |gamma| in [0.5, 2], a quarter of the channels negative; beta = 0.3 N(0, 1).  The allowance is
    proportional to |gamma| while the fp32 evaluation of gamma xhat + beta (and of its SiLU) leaves an error proportional to |y|,
    about 4 x 2^-24 (|gamma xhat| + |beta|), which no term of the bound names: where the format's floor is used up — an fp16 output
    next to a rounding tie — the allowance has to cover it, 13 x 2^-24 |gamma| (|xhat| + 1) at r = 0.5.  It does for |gamma| >= 0.5
    and |beta| <= 1.3; it could not for the gamma ~ 0 channels that 0.5 N(0, 1) + 1 draws.  `zero_every` = k sets gamma = 0 in every
    k-th channel: there the allowance is 0 and the output, beta or SiLU(beta), is held to the format's floor alone."""
    g = _gen(seed)
    mag = 0.5 + 1.5 * torch.rand(C, generator=g)
    sgn = 1.0 - 2.0 * (torch.rand(C, generator=g) < 0.25).float()
    gamma = mag * sgn
    if zero_every:
        gamma[3::zero_every] = 0.0
    return gamma, torch.randn(C, generator=g) * 0.3


def spatial(F, Npix, C, r, seed=1, zero=True):
    """-> fp32 [F * Npix, C]; the all-zero set is (frame F - 1, group 7)"""
    g, cpg = _gen(seed), C // GROUPS
    sig = _sigma(g, F, GROUPS, 1)
    sgn = _sign(torch.arange(F).view(F, 1, 1), torch.arange(GROUPS).view(1, GROUPS, 1))
    x = sgn * r * sig + sig * _unit(g, F, GROUPS, Npix * cpg)
    if zero:
        x[F - 1, 7] = 0.0
    return x.view(F, GROUPS, Npix, cpg).permute(0, 2, 1, 3).reshape(F * Npix, C).float().contiguous()


def temporal(B, T, Npix, C, r, seed=2, zero=True):
    """-> fp32 [B * T * Npix, C]; the all-zero set is (sample 0, pixel 1, group 3)"""
    g, cpg = _gen(seed), C // GROUPS
    sig = _sigma(g, B, Npix, GROUPS, 1)
    sgn = _sign(torch.arange(Npix).view(1, Npix, 1, 1), torch.arange(GROUPS).view(1, 1, GROUPS, 1))
    x = sgn * r * sig + sig * _unit(g, B, Npix, GROUPS, T * cpg)
    if zero:
        x[0, 1, 3] = 0.0
    return x.view(B, Npix, GROUPS, T, cpg).permute(0, 3, 1, 2, 4).reshape(B * T * Npix, C).float().contiguous()


def row_sets(M, C, r, seed=3):
    """-> fp32 [M, C], a set per row"""
    g = _gen(seed)
    sig = _sigma(g, M, 1)
    x = _sign(torch.arange(M).view(M, 1)) * r * sig + sig * _unit(g, M, C)
    return x.float().contiguous()


def concat(F, Npix, C1, C2, ctrl, r, seed=4):
    """operands (a, s, c or None) of pnc_concat_add whose result is spatial(F, Npix, C1 + C2, r) up to the fp32 rounding of s + c:
    the control branch c is unit noise, the skip s carries the offsets"""
    M = F * Npix
    out = spatial(F, Npix, C1 + C2, r, seed).double()
    a, s, c = out[:, :C1], out[:, C1:], None
    if ctrl:
        c = torch.randn(M, C2, generator=_gen(seed + 100), dtype=torch.float64).float()
        s = s - c.double()
    return a.float().contiguous(), s.float().contiguous(), c


def realised_r(mean, var):
    """|mean| / std per set, NaN for an all-zero set"""
    return mean.abs() / var.sqrt()


# ---- bounds --------------------------------------------------------------------------------------------------------------------
def var_bound(r):
    return 2.0 ** -20 * (1.0 + r)


def mean_bound(r, sigma):
    return 2.0 ** -21 * (1.0 + r) * sigma


def floor_f16(y64):
    """half an fp16 ulp of y64 (the subnormal spacing 2^-24 below 2^-14)"""
    e = torch.floor(torch.log2(y64.abs().clamp_min(2.0 ** -14)))
    return 0.5 * torch.exp2(e - 10.0)


def floor_e4m3(y64):
    return 6e-5 + 6e-5 * y64.abs()


def floor_f16lo(y64):
    return 2.0 ** -20 * y64.abs().clamp_min(1.0)


FLOORS = {None: floor_f16, "f16": floor_f16lo, "e4m3": floor_e4m3}
LO_DTYPE = {"f16": torch.float16, "e4m3": torch.uint8}


def allowance(xhat, gamma, r):
    """the statistics' share of the output bound, per element of a [rows, C] output"""
    return 1.1 * gamma.double().abs() * (2.0 ** -21 * (1.0 + r) * xhat.abs() + 2.0 ** -21 * (1.0 + r))


def joined(hi, lo):
    """float64 value of an output: the fp16 plane alone, or hi + lo / 2048 of a split operand in either lo format"""
    v = hi.double().cpu()
    if lo is not None:
        lo = lo.cpu()
        v = v + (lo.view(torch.float8_e4m3fn).float() if lo.dtype == torch.uint8 else lo.float()).double() / 2048.0
    return v


def output_excess(got, y64, xhat, gamma, r, lo=None, share=1.0):
    """-> (max |got - y64|, max of |got - y64| / bound): the second is <= 1 inside the output bound.  `share` scales the statistics'
    allowance (not the format's floor)"""
    ok = ~torch.isnan(y64)
    err = (got - y64).abs()
    bound = FLOORS[lo](y64) + share * allowance(xhat, gamma, r)
    return err[ok].max().item(), (err / bound)[ok].max().item()


def stats_excess(mean, var, mean64, var64, r):
    """-> (max |var / var64 - 1|, its ratio to the bound, max |mean - mean64| / sigma, its ratio to the bound) over the sets with
    var64 > 0; r: a number or a tensor per set.  Sets with var64 == 0 (all-zero data) must be reproduced exactly."""
    mean, var = mean.double().cpu(), var.double().cpu()
    zero = var64 == 0
    assert (var[zero] == 0).all() and (mean[zero] == mean64[zero]).all(), "an all-zero set must give mean 0 and var 0 exactly"
    nz = ~zero
    r = torch.as_tensor(r, dtype=torch.float64).expand_as(var64)[nz]
    ev = (var[nz] / var64[nz] - 1.0).abs()
    em = (mean[nz] - mean64[nz]).abs() / var64[nz].sqrt()
    return ev.max().item(), (ev / var_bound(r)).max().item(), em.max().item(), (em / mean_bound(r, 1.0)).max().item()
