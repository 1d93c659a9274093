"""CPU emulation of pnc_gemm_wsplit_f16 (include/panacea_hip.h: the fp16 lo plane of the weights BESIDE the parameter block, the
`precise-ckpt` operand policy) for the emu backend of tests/emu.py: a `gemm` that takes the plane as `w_lo16` and hands everything
else to tests/emu_weights.py / tests/emu.py.  tests/test_precise_ckpt.py attaches it to `emu` with monkeypatch, next to the small-M
linears of tests/emu_weights.py (the policy's `weights` attribute is True: they receive their twins as under `precise-full`).

The kernels' sum is A W ~= A_hi W_hi + 2^-11 (A_lo W_hi [where A is split] + A_hi W_lo16).  It is linear in W, so the emulation adds
2^-11 A_hi W_lo16 through emu.ACC_HOOK, ahead of the epilogue, to whatever emu.gemm computes for the other operands (an e4m3 A_lo
keeps its e4m3 `w_lo` pair).  An fp16 A_lo is forwarded to the three-part launch, as the library does."""
import torch

import emu
import emu_weights

S = 1.0 / emu.LO_SCALE


def gemm(a16, w16, *, w_lo16=None, w_lo=None, **kw):
    if w_lo16 is None:
        return emu_weights.gemm(a16, w16, w_lo=w_lo, **kw)
    if w_lo16.dtype != torch.float16 or w_lo16.shape != w16.shape:
        raise emu.PncError("w_lo16: the fp16 lo plane of the weights in w16's layout")
    a_lo = kw.get("a16_lo")
    if a_lo is not None and a_lo.dtype == torch.float16:
        if w_lo is not None:
            raise emu.PncError("an fp16 A_lo is forwarded with W_lo = W_lo16: W_lo must be NULL (PNC_EINVAL)")
        return emu_weights.gemm(a16, w16, w_lo=w_lo16, **kw)
    M, N, K = kw["M"], kw["N"], kw["K"]
    Wl = emu._mat(w_lo16, N, K, kw.get("w_ld", 0) or K).float()
    extra = emu._contract(a16, Wl, M, N, K, kw.get("lda", 0), kw.get("a_mode", emu.A_PLAIN), kw.get("conv"), kw.get("tconv")) * S
    prev = emu.ACC_HOOK
    emu.ACC_HOOK = lambda acc, *a: (acc if prev is None else prev(acc, *a)) + extra
    try:
        return emu_weights._gemm(a16, w16, w_lo=w_lo, **kw)
    finally:
        emu.ACC_HOOK = prev
