"""CPU emulation of split WEIGHTS (include/panacea_hip.h: PncGemmParams.W_lo next to an fp16 A_lo, pnc_linear_smallm_split,
pnc_linear_smallm_segments_split) for the emu backend of tests/emu.py: `gemm`, `linear_smallm` and `linear_smallm_segments` that
take the fp16 lo plane of the weights as `w_lo` and hand everything else to tests/emu.py.  tests/test_precise_full.py attaches them
to `emu` with monkeypatch, next to the split attention of tests/emu_wide.py.

The GEMM is the kernels' sum: A W ~= A_hi W_hi + 2^-11 (A_lo W_hi + A_hi W_lo), the 2^-22 A_lo W_lo term dropped.  It is linear in
W, so the emulation calls emu.gemm once with the raw (A_hi + 2^-11 A_lo) W_hi product and adds 2^-11 A_hi W_lo through emu.ACC_HOOK,
ahead of the epilogue.  The small-M linears join w = W + 2^-11 W_lo in fp32 as their kernels do."""
import torch

import emu

S = 1.0 / emu.LO_SCALE
_gemm, _smallm, _smallm_seg = emu.gemm, emu.linear_smallm, emu.linear_smallm_segments


def gemm(a16, w16, *, w_lo=None, **kw):
    if not isinstance(w_lo, torch.Tensor):               # None, or the (bytes, exponent) pair of an e4m3 lo pass
        return _gemm(a16, w16, w_lo=w_lo, **kw)
    a_lo = kw.get("a16_lo")
    if a_lo is None:
        raise emu.PncError("W_lo without A_lo (PNC_EINVAL)")
    if a_lo.dtype != torch.float16 or w_lo.dtype != torch.float16:
        raise emu.PncError("split weights go with fp16 lo planes")
    M, N, K = kw["M"], kw["N"], kw["K"]
    Wl = emu._mat(w_lo, N, K, kw.get("w_ld", 0) or K).float()
    extra = emu._contract(a16, Wl, M, N, K, kw.get("lda", 0), kw.get("a_mode", emu.A_PLAIN), kw.get("conv"), kw.get("tconv")) * S
    prev = emu.ACC_HOOK
    emu.ACC_HOOK = lambda acc, *a: (acc if prev is None else prev(acc, *a)) + extra
    try:
        return _gemm(a16, w16, **kw)
    finally:
        emu.ACC_HOOK = prev


def _join(w16, w_lo):
    return w16 if w_lo is None else w16.float() + w_lo.float() * S


def linear_smallm(a32, lda, w16, bias, out32, ldo, M, N, K, silu_in=False, silu_out=False, w_lo=None):
    return _smallm(a32, lda, _join(w16, w_lo), bias, out32, ldo, M, N, K, silu_in, silu_out)


def linear_smallm_segments(a32, lda, w16, bias, out32, M, m0, Mtot, N, K, seg_start, silu_in=False, silu_out=False, w_lo=None):
    return _smallm_seg(a32, lda, _join(w16, w_lo), bias, out32, M, m0, Mtot, N, K, seg_start, silu_in, silu_out)
