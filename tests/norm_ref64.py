"""Float64 references of the normalisation entry points (include/panacea_hip.h), written from the header's layouts and indexed
on the channels-last token buffers themselves.  Independent of tests/emu.py: tests/test_norm_ref64.py holds the emulation to
these, tests/test_norm_offsets_gpu.py the kernels.

Every function takes the fp32 buffers a launch reads (CPU tensors) and returns float64.  Functions that produce an operand return
(y, xhat): the output value next to the pre-affine normalised value xhat = (x - mean) / sqrt(var + eps) of the same element — the
error allowance of tests/norm_offset_cases.py scales with |xhat|."""
import torch

GROUPS = 32


def rows(x32, M, C, ld):
    """[M, C] float64 copy of the rows of a buffer with row stride ld"""
    return torch.as_strided(x32.reshape(-1), (M, C), (ld, 1)).double()


def _silu(v):
    return v * torch.sigmoid(v)


def _normalise(X, dims, eps):
    """X float64; statistics over `dims` (biased variance) -> (xhat, mean, var), the latter two with the dims kept"""
    mean = X.mean(dim=dims, keepdim=True)
    var = ((X - mean) ** 2).mean(dim=dims, keepdim=True)
    return (X - mean) / torch.sqrt(var + eps), mean, var


# ---- spatial GroupNorm(32): a set = (frame, group) = Npix pixels x C / 32 consecutive channels -------------------------------
def groupnorm_sets(x32, ldx, F, Npix, C):
    """-> (mean, var) float64 [F, 32] of pnc_groupnorm_stats + the combination pnc_groupnorm_apply performs"""
    X = rows(x32, F * Npix, C, ldx).view(F, Npix, GROUPS, C // GROUPS)
    _, mean, var = _normalise(X, (1, 3), 0.0)
    return mean.reshape(F, GROUPS), var.reshape(F, GROUPS)


def groupnorm(x32, ldx, F, Npix, C, gamma, beta, eps, silu):
    """pnc_groupnorm_stats + pnc_groupnorm_apply -> (y, xhat) [F * Npix, C]"""
    X = rows(x32, F * Npix, C, ldx).view(F, Npix, GROUPS, C // GROUPS)
    xhat = _normalise(X, (1, 3), eps)[0].reshape(F * Npix, C)
    y = xhat * gamma.double().reshape(-1)[:C] + beta.double().reshape(-1)[:C]
    return (_silu(y) if silu else y), xhat


def groupnorm_records(x32, ldx, F, Npix, C, ppc):
    """the records pnc_groupnorm_stats / pnc_concat_add_stats / PncGemmParams.gn_part write: [F, ceil(Npix / ppc), 32, 3] =
    {n, mean, M2 = sum (x - mean)^2} of the chunk's pixels x the group's channels"""
    X = rows(x32, F * Npix, C, ldx).view(F, Npix, GROUPS, C // GROUPS)
    nchunk = (Npix + ppc - 1) // ppc
    P = torch.zeros(F, nchunk, GROUPS, 3, dtype=torch.float64)
    for c in range(nchunk):
        xs = X[:, c * ppc:(c + 1) * ppc]
        mean = xs.mean(dim=(1, 3))
        P[:, c, :, 0] = xs.shape[1] * xs.shape[3]
        P[:, c, :, 1] = mean
        P[:, c, :, 2] = ((xs - mean[:, None, :, None]) ** 2).sum(dim=(1, 3))
    return P


def combine_records(P):
    """[F, records, 32, 3] (any float dtype) -> (n, mean, var) float64 [F, 32]: what pnc_groupnorm_apply / pnc_groupnorm_combine
    make of the records of a frame"""
    P = P.double()
    n = P[..., 0].sum(1)
    mean = (P[..., 0] * P[..., 1]).sum(1) / n
    m2 = (P[..., 2] + P[..., 0] * (P[..., 1] - mean[:, None]) ** 2).sum(1)
    return n, mean, m2 / n


def concat_add(a32, C1, s32, c32, C2, M):
    """pnc_concat_add: [a | s + c] -> float64 [M, C1 + C2]"""
    s = rows(s32, M, C2, C2)
    if c32 is not None:
        s = s + rows(c32, M, C2, C2)
    return torch.cat([rows(a32, M, C1, C1), s], dim=1)


# ---- temporal GroupNorm(32) + SiLU: a set = (sample, pixel, group) = T frames x C / 32 channels ------------------------------
def groupnorm_temporal_sets(x32, B, T, Npix, C):
    """-> (mean, var) float64 [B, Npix, 32]"""
    X = x32.reshape(-1)[: B * T * Npix * C].double().view(B, T, Npix, GROUPS, C // GROUPS)
    _, mean, var = _normalise(X, (1, 4), 0.0)
    return mean.reshape(B, Npix, GROUPS), var.reshape(B, Npix, GROUPS)


def groupnorm_temporal_silu(x32, B, T, Npix, C, gamma, beta, eps, t_pad=0):
    """pnc_groupnorm_temporal_silu (t_pad = 0) / pnc_groupnorm_temporal_part mode 2 with every frame local: (y, xhat) in the
    [B, T + 2 t_pad, Npix, C] layout of the output, frame t in slot t + t_pad; the halo slots, which the kernel leaves alone, are NaN"""
    X = x32.reshape(-1)[: B * T * Npix * C].double().view(B, T, Npix, GROUPS, C // GROUPS)
    xhat = _normalise(X, (1, 4), eps)[0].reshape(B, T, Npix, C)
    y = _silu(xhat * gamma.double().reshape(-1)[:C] + beta.double().reshape(-1)[:C])
    out = torch.full((2, B, T + 2 * t_pad, Npix, C), float("nan"), dtype=torch.float64)
    out[0, :, t_pad:t_pad + T] = y
    out[1, :, t_pad:t_pad + T] = xhat
    return out[0], out[1]


# ---- LayerNorm: a set = a row --------------------------------------------------------------------------------------------------
def layernorm_sets(x32, ldx, M, C):
    """-> (mean, var) float64 [M]"""
    _, mean, var = _normalise(rows(x32, M, C, ldx), (1,), 0.0)
    return mean.reshape(M), var.reshape(M)


def layernorm(x32, ldx, M, C, gamma, beta, eps):
    """pnc_layernorm / the ln_out16 of a GEMM on its fp32 output rows -> (y, xhat) [M, C]"""
    xhat = _normalise(rows(x32, M, C, ldx), (1,), eps)[0]
    return xhat * gamma.double().reshape(-1)[:C] + beta.double().reshape(-1)[:C], xhat
