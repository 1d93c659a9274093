"""ctypes binding of libpanacea_hip.so (the C-ABI declared in include/panacea_hip.h).

This is the ONLY compute backend of the package: there is no CPU or eager fallback.  Importing the
module is cheap; the shared object is loaded on first use and a missing / stale library raises
`HipLibraryError` (run `python -m panacea_amd.build`).  Every wrapper takes torch tensors that already
live in HBM, enqueues on the CURRENT torch stream and returns immediately (hipGraph-capturable).
"""
from __future__ import annotations

import ctypes as C
import re
from pathlib import Path
from typing import Optional

import torch

PKG = Path(__file__).resolve().parent
LIB_PATH = PKG / "lib" / "libpanacea_hip.so"
HEADER = PKG.parent / "include" / "panacea_hip.h"

A_PLAIN, A_CONV3X3, A_CONV1D_T = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
ABI_VERSION = 8          # PNC_ABI_VERSION of include/panacea_hip.h this binding was written against
LO_F16, LO_E4M3 = 0, 1   # PNC_LO_*: storage format of the lo plane of a precise operand
# dtype of a lo-plane tensor <-> format: an fp16 tensor holds fp16(r), a uint8 tensor OCP e4m3 bytes (one per element)
LO_DTYPE = {LO_F16: torch.float16, LO_E4M3: torch.uint8}


def lo_fmt(t: Optional[torch.Tensor]) -> int:
    """PNC_LO_* of a lo-plane tensor, from its dtype (None -> PNC_LO_F16, the argument is ignored by the kernels then)"""
    if t is None or t.dtype == torch.float16:
        return LO_F16
    if t.dtype == torch.uint8:
        return LO_E4M3
    raise PncError(f"a lo plane is fp16 (PNC_LO_F16) or uint8 e4m3 bytes (PNC_LO_E4M3), got {t.dtype}")


class HipLibraryError(RuntimeError):
    pass


class PncError(RuntimeError):
    pass


class GemmParams(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("W", C.c_void_p),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("lda", C.c_int32), ("a_mode", C.c_int32),
        ("Cin", C.c_int32), ("Hin", C.c_int32), ("Win", C.c_int32), ("Hout", C.c_int32),
        ("Wout", C.c_int32), ("stride", C.c_int32), ("upsample", C.c_int32),
        ("T", C.c_int32), ("Npix", C.c_int32),
        ("bias", C.c_void_p), ("rowbias", C.c_void_p),
        ("rb_rows", C.c_int32), ("rb_mod", C.c_int32),
        ("res1", C.c_void_p), ("ldr1", C.c_int32),
        ("res2", C.c_void_p), ("ldr2", C.c_int32),
        ("out32", C.c_void_p), ("ldc32", C.c_int32),
        ("out16", C.c_void_p), ("ldc16", C.c_int32),
        ("out16t", C.c_void_p), ("ldt", C.c_int32), ("t_rows", C.c_int32), ("t_gstride", C.c_int64),
        ("n_split", C.c_int32), ("act", C.c_int32), ("geglu", C.c_int32),
        ("ws", C.c_void_p), ("ws_floats", C.c_int64),
        ("conv_pad_br", C.c_int32), ("struct_bytes", C.c_int32),
        ("A_lo", C.c_void_p), ("out16_lo", C.c_void_p),
        ("ldw", C.c_int32), ("ln_eps", C.c_float),
        ("ln_gamma", C.c_void_p), ("ln_beta", C.c_void_p), ("ln_out16", C.c_void_p),
        ("ldln", C.c_int32), ("a_lo_fmt", C.c_int32),
        ("out_lo_fmt", C.c_int32), ("ldw_lo", C.c_int32),
        ("W_lo", C.c_void_p), ("w_lo_exp", C.c_int32), ("t_halo", C.c_int32),
        ("x_halo_off", C.c_int64), ("gn_part", C.c_void_p),
    ]


class AttnParams(C.Structure):
    _fields_ = [
        ("q", C.c_void_p), ("ldq", C.c_int32),
        ("k", C.c_void_p), ("ldk", C.c_int32),
        ("vt", C.c_void_p), ("ldvt", C.c_int32), ("vt_gstride", C.c_int64),
        ("o", C.c_void_p), ("ldo", C.c_int32),
        ("groups", C.c_int32), ("heads", C.c_int32),
        ("H", C.c_int32), ("W", C.c_int32), ("views", C.c_int32),
        ("kvH", C.c_int32), ("kvW", C.c_int32), ("kv_views", C.c_int32),
        ("kv_rows_per_group", C.c_int32), ("q_per_kv", C.c_int32), ("kv_valid", C.c_int32),
        ("nseg", C.c_int32 * 8), ("seg", (C.c_int32 * 2) * 8),
        ("scale", C.c_float), ("causal", C.c_int32),
        ("k_halo", C.c_void_p * 2), ("vt_halo", C.c_void_p * 2),
    ]


class AttnSplitParams(C.Structure):
    _fields_ = [
        ("struct_bytes", C.c_int32), ("a", AttnParams),
        ("q_lo", C.c_void_p), ("k_lo", C.c_void_p), ("v_lo", C.c_void_p), ("o_lo", C.c_void_p),
    ]


class SamplerStepParams(C.Structure):
    _fields_ = [
        ("struct_bytes", C.c_int32), ("mode", C.c_int32),
        ("eps_tok", C.c_void_p), ("ld", C.c_int32), ("T", C.c_int32), ("Npix", C.c_int32), ("C", C.c_int32),
        ("cfg", C.c_int32), ("scale", C.c_float),
        ("x", C.c_void_p), ("c_out", C.c_void_p), ("x0", C.c_void_p), ("aux", C.c_void_p),
        ("hist", C.c_void_p * 4), ("n_hist", C.c_int32), ("s_noise", C.c_float), ("noise", C.c_void_p),
        ("v", C.c_void_p * 6), ("out", C.c_void_p), ("out_aux", C.c_void_p),
    ]


# PNC_SAMPLER_*: the update pnc_cfg_sampler_step applies after forming denoised
SAMPLER_HEUN1, SAMPLER_HEUN2, SAMPLER_EULER_A, SAMPLER_DPM2S_1, SAMPLER_DPM2S_2, SAMPLER_DPM2M, SAMPLER_LMS = range(7)


_P, _I, _L, _F = C.c_void_p, C.c_int, C.c_int64, C.c_float
_SIGNATURES = {
    "pnc_version": (C.c_char_p, []),
    "pnc_abi_version": (_I, []),
    "pnc_build_digest": (C.c_char_p, []),
    "pnc_set_option": (_I, [_I, _I]),
    "pnc_gemm_f16": (_I, [C.POINTER(GemmParams), _P]),
    "pnc_gemm_wsplit_f16": (_I, [C.POINTER(GemmParams), _P, _P]),
    "pnc_gemm_workspace_floats": (_L, [C.POINTER(GemmParams)]),
    "pnc_gemm_fuses_layernorm": (_I, [C.POINTER(GemmParams)]),
    "pnc_attn_views_f16": (_I, [C.POINTER(AttnParams), _P]),
    "pnc_attn_uses_text_kernel": (_I, [C.POINTER(AttnParams)]),
    "pnc_attn_views_split_f16": (_I, [C.POINTER(AttnSplitParams), _P]),
    "pnc_attn_temporal_split_f16": (_I, [_P, _P, _I, _P, _P, _I, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _P]),
    "pnc_softmax_rows_f16": (_I, [_P, _L, _I, _I, _F, _I, _I, _P, _L, _P]),
    "pnc_attn_temporal_f16": (_I, [_P, _I, _P, _I, _P, _I, _P, _I, _I, _I, _I, _I, _F, _P]),
    "pnc_attn_frame_f16": (_I, [_P, _L, _P, _L, _P, _L, _L, _P, _L, _I, _I, _I, _F, _P]),
    "pnc_attn_frame_split_f16": (_I, [_P, _P, _L, _P, _P, _L, _P, _P, _L, _P, _P, _L, _I, _I, _I, _F, _P]),
    "pnc_attn_text_split_f16": (_I, [_P, _P, _L, _P, _P, _L, _P, _P, _L, _P, _P, _L, _I, _I, _I, _I, _F, _P]),
    "pnc_groupnorm_stats": (_I, [_P, _I, _I, _I, _I, _I, _P, _P]),
    "pnc_groupnorm_apply": (_I, [_P, _I, _I, _I, _I, _I, _P, _P, _P, _F, _I, _P, _I, _P, _I, _I, _P]),
    "pnc_groupnorm_combine": (_I, [_P, _I, _I, _I, _P, _P]),
    "pnc_groupnorm_temporal_part": (_I, [_P, _I, _I, _I, _I, _P, _P, _F, _P, _I, _I, _P, _P, _I, _I, _P]),
    "pnc_groupnorm_temporal_silu": (_I, [_P, _I, _I, _I, _I, _P, _P, _F, _P, _P, _I, _P]),
    "pnc_layernorm": (_I, [_P, _I, _I, _I, _P, _P, _F, _P, _I, _P, _P]),
    "pnc_linear_smallm": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "pnc_linear_smallm_segments": (_I, [_P, _I, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _I, _P]),
    "pnc_linear_smallm_split": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P]),
    "pnc_linear_smallm_segments_split": (_I, [_P, _I, _P, _P, _P, _P, _I, _I, _I, _I, _I, _P, _I, _I, _I, _P]),
    "pnc_timestep_embedding": (_I, [_P, _I, _I, _P, _P, _P]),
    "pnc_timestep_embedding_f32": (_I, [_P, _I, _I, _P, _P, _P]),
    "pnc_nchw_to_tokens_f16": (_I, [_P, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _P]),
    "pnc_cfg_euler_step": (_I, [_P, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P]),
    "pnc_cfg_sampler_step": (_I, [C.POINTER(SamplerStepParams), _P]),
    "pnc_cfg_euler_step_skip": (_I, [_P, _I, _I, _I, _I, _I, _F, _P, _P, _P, _P, _P, _P, _P]),
    "pnc_cfg_sampler_step_skip": (_I, [C.POINTER(SamplerStepParams), _P, _P]),
    "pnc_tokens_to_nchw_f32": (_I, [_P, _I, _I, _I, _I, _P, _P]),
    "pnc_concat_add": (_I, [_P, _I, _P, _P, _I, _L, _P, _P, _P, _I, _P]),
    "pnc_concat_add_stats": (_I, [_P, _I, _P, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P, _P]),
    "pnc_add_f32": (_I, [_P, _P, _L, _P, _P, _P, _I, _P]),
    "pnc_cast_f16": (_I, [_P, _L, _P, _P, _I, _P]),
    "pnc_upsample_combine": (_I, [_P, _L, _P, _I, _I, _I, _I, _P, _P, _P, _I, _P]),
    "pnc_range_monitor_collect": (_I, [_P, _P]),
    "pnc_operand_stats_f16": (_I, [_P, _P, _I, _L, _I, _L, _P, _P]),
    "pnc_u8_to_tokens_f16": (_I, [_P, _P, _I, _I, _I, _I, _P, _P, _P]),
    "pnc_tokens_to_u8": (_I, [_P, _I, _L, _I, _P, _P]),
    "pnc_frames_renoise": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _L, _P]),
    "pnc_latent_renoise_masked": (_I, [_P, _P, _P, _P, _P, _P, _I, _I, _L, _P]),
    "pnc_mask_pool_u8": (_I, [_P, _P, _I, _I, _I, _I, _P]),
    "pnc_u8_select": (_I, [_P, _P, _P, _P, _L, _I, _P]),
}

_lib = None


def header_symbols() -> list[str]:
    """Every function name declared in include/panacea_hip.h."""
    txt = HEADER.read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(pnc_[a-z0-9_]+)\s*\(", txt)))


def load():
    """Load the shared library (once) and declare the prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    import os
    global LIB_PATH
    if os.environ.get("PANACEA_HIP_LIB"):          # A/B runs of two builds of the SAME ABI (tools/exp); never a fallback
        LIB_PATH = Path(os.environ["PANACEA_HIP_LIB"])
    if not LIB_PATH.exists():
        raise HipLibraryError(
            f"{LIB_PATH} is missing: the HIP extension is the only compute path of panacea_amd. "
            "Build it with `python -m panacea_amd.build` (hipcc --offload-arch=gfx950).")
    try:
        lib = C.CDLL(str(LIB_PATH))
    except OSError as e:  # pragma: no cover
        raise HipLibraryError(f"cannot load {LIB_PATH}: {e}") from e
    if not os.environ.get("PANACEA_HIP_LIB"):
        # a library built from other sources than the ones next to it is an ABI hazard (argument lists change): refuse it, do
        # not guess.  The digest is compiled INTO the library (pnc_build_digest), so no side file can vouch for a stale build.
        from . import build as _build
        try:
            lib.pnc_build_digest.restype = C.c_char_p
            have = lib.pnc_build_digest().decode()
        except AttributeError:
            have = "(a library older than pnc_build_digest)"
        if _build.CSRC.exists() and have != _build._digest():
            raise HipLibraryError(f"{LIB_PATH} was built from other sources ({have[:12]}) than panacea_amd/csrc holds now "
                                  f"({_build._digest()[:12]}); rebuild it with `python -m panacea_amd.build`")
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise HipLibraryError(f"{LIB_PATH} does not export {name}; rebuild the extension") from e
        fn.restype = res
        fn.argtypes = args
    if lib.pnc_abi_version() != ABI_VERSION:
        raise HipLibraryError(f"{LIB_PATH} implements C-ABI version {lib.pnc_abi_version()}, this binding needs "
                              f"{ABI_VERSION}; rebuild the extension (`python -m panacea_amd.build --force`)")
    _lib = lib
    return lib


OPT_GEMM_TAIL_SPLIT, OPT_GEMM_TILE, OPT_ATTN_VARIANT, OPT_ATTN_DMA, OPT_GEMM_FUSE_LN, OPT_GEMM_GROUP_M, OPT_STENCIL_TILES = 0, 1, 2, 3, 4, 5, 6
OPT_GEMM_PERSIST = 7
OPT_ATTN_DEFER_MAX = 8
OPT_GEMM_GN_STATS = 9
OPT_GEMM_STAGGER = 10
OPT_ATTN_SUM_TRIGGER = 11


def build_digest() -> str:
    """pnc_build_digest() of the loaded library (what bench.py / tools/pmc_traffic.py stamp their records with)"""
    return load().pnc_build_digest().decode()


def set_option(option: int, value: int) -> int:
    """pnc_set_option: process-global tuning / test switch of the library; returns the previous value."""
    if not 0 <= option <= OPT_ATTN_SUM_TRIGGER:
        raise PncError(f"unknown library option {option}")
    return load().pnc_set_option(option, value)


CU_MASK_PATTERNS = {            # complementary halves of the 256 CUs, as 8 x 32-bit words (hipExtStreamCreateWithCUMask)
    "even-odd": ([0x55555555] * 8, [0xAAAAAAAA] * 8),
    "nibbles": ([0x0F0F0F0F] * 8, [0xF0F0F0F0] * 8),
    "halves": ([0xFFFFFFFF] * 4 + [0] * 4, [0] * 4 + [0xFFFFFFFF] * 4),
}


def masked_stream(words) -> "torch.cuda.Stream":
    """A HIP stream whose kernels run on the CUs of `words` only (hipExtStreamCreateWithCUMask of the HIP runtime this process
    already uses), wrapped for torch.  Round 6 experiment: two sample chains on complementary halves of
    the chip.  The stream lives as long as the process."""
    rt = None
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            rt = C.CDLL(line.split()[-1])
            break
    if rt is None:
        raise PncError("the HIP runtime is not loaded")
    rt.hipExtStreamCreateWithCUMask.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_uint32)]
    rt.hipExtStreamCreateWithCUMask.restype = C.c_int
    st = C.c_void_p()
    arr = (C.c_uint32 * len(words))(*words)
    rc = rt.hipExtStreamCreateWithCUMask(C.byref(st), C.c_uint32(len(words)), arr)
    if rc != 0:
        raise PncError(f"hipExtStreamCreateWithCUMask failed with {rc}")
    return torch.cuda.ExternalStream(st.value)


class Profiler:
    """Per-launch HIP-event timing by kernel family (bench.py's instrumented pass; off by default).
    Events are recorded on the current torch stream, which is the stream every kernel is launched on."""

    def __init__(self):
        self.records = []          # (family, ev0, ev1, flops, bytes)

    def summary(self) -> dict:
        torch.cuda.synchronize()
        out = {}
        for fam, e0, e1, fl, by in self.records:
            d = out.setdefault(fam, dict(launches=0, ms=0.0, flops=0.0, bytes=0.0))
            d["launches"] += 1
            d["ms"] += e0.elapsed_time(e1)
            d["flops"] += fl
            d["bytes"] += by
        return out


_PROF: Optional[Profiler] = None


def set_profiler(p: Optional[Profiler]):
    global _PROF
    _PROF = p


def _timed(family: str, flops: float, nbytes: float, fn, *args):
    if _PROF is None:
        return fn(*args)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = fn(*args)
    e1.record()
    _PROF.records.append((family, e0, e1, flops, nbytes))
    return rc


def _check(rc: int, what: str):
    if rc != 0:
        kind = {-1: "PNC_EINVAL (unsupported shape/argument)", -2: "PNC_EALIGN (alignment)",
                -3: "PNC_EABI (parameter struct of another header version)"}.get(rc, f"hipError {rc}")
        raise PncError(f"{what} failed: {kind}")


def _sibling(entry: str, suffix: str, extra, what: str, dtype):
    """(entry point, inserted arguments) of a wrapper that serves an entry and its `suffix` sibling, which takes one more pointer:
    the sibling and that pointer when the operand `extra` is given, the entry and nothing otherwise"""
    return (entry, ()) if extra is None else (entry + suffix, (_ptr(extra, dtype, what),))


def _stream() -> int:
    """the CURRENT torch stream of the CURRENT device: every wrapper launches there, and `_ptr` refuses operands that
    live on another device (a launch on device A's stream with device B's pointers reads garbage without an error)"""
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor], dtype=None, name: str = "operand") -> Optional[int]:
    if t is None:
        return None
    if not t.is_cuda:
        raise PncError("panacea_amd kernels need tensors resident in HBM (got a CPU tensor); "
                       "there is no CPU fallback")
    if t.device.index != torch.cuda.current_device():
        raise PncError(f"{name} lives on cuda:{t.device.index} but the current device is cuda:{torch.cuda.current_device()}: "
                       "select the tensors' device (torch.cuda.device / set_device) before calling the kernels")
    if dtype is not None and t.dtype != dtype:
        raise PncError(f"{name}: expected {dtype}, got {t.dtype}")
    return t.data_ptr()


# ----------------------------------------------------------------------------------------------
# wrappers (names mirror the C entry points)
# ----------------------------------------------------------------------------------------------
def gemm(a16: torch.Tensor, w16: torch.Tensor, *, M: int, N: int, K: int, lda: int = 0,
         a_mode: int = A_PLAIN, conv: Optional[dict] = None, tconv: Optional[dict] = None,
         bias: Optional[torch.Tensor] = None, rowbias: Optional[torch.Tensor] = None,
         rb_rows: int = 0, rb_mod: int = 0,
         res1: Optional[torch.Tensor] = None, ldr1: int = 0,
         res2: Optional[torch.Tensor] = None, ldr2: int = 0,
         out32: Optional[torch.Tensor] = None, ldc32: int = 0,
         out16: Optional[torch.Tensor] = None, ldc16: int = 0,
         out16t: Optional[torch.Tensor] = None, ldt: int = 0, t_rows: int = 0, t_gstride: int = 0,
         n_split: int = 0, act: int = ACT_NONE, geglu: bool = False,
         a16_lo: Optional[torch.Tensor] = None, out16_lo: Optional[torch.Tensor] = None, w_ld: int = 0,
         w_lo: Optional[tuple] = None, w_lo16: Optional[torch.Tensor] = None,
         ln_gamma: Optional[torch.Tensor] = None, ln_beta: Optional[torch.Tensor] = None,
         ln_out16: Optional[torch.Tensor] = None, ldln: int = 0, ln_eps: float = 1e-5, ln_in_library: bool = False,
         gn_part: Optional[torch.Tensor] = None):
    """`gn_part` (temporal conv only): receives the GroupNorm(32) records of the fp32 output, ceil(Npix / 64) per frame
    (PncGemmParams.gn_part).  `a16_lo` / `out16_lo`: lo planes of precise (split) operands, see PncGemmParams.A_lo in the header; their dtype names the
    format (fp16, or uint8 = e4m3 bytes).  `w_lo` = (W_lo e4m3 bytes [N, K], w_lo_exp E8M0 byte of the tensor) — engine.pk_lo8 —
    is the weight side of an e4m3 lo pass; `w_lo` = an fp16 tensor in w16's layout is the lo plane of split weights (engine.wlo under
    the `precise-full` policy, PncGemmParams.W_lo): it goes with an fp16 `a16_lo`.  `w_lo16`: the same fp16 lo plane handed over BESIDE
    the struct (pnc_gemm_wsplit_f16, the `precise-ckpt` policy): it goes with every `a16_lo` — none, e4m3 (`w_lo` then stays the e4m3
    pair) or fp16 (the library forwards that launch to the three-part one; `w_lo` must be None)."""
    if w_lo16 is not None and (w_lo16.dtype != torch.float16 or w_lo16.shape != w16.shape):
        raise PncError(f"w_lo16: the fp16 lo plane of the weights in w16's layout {tuple(w16.shape)}, got {w_lo16.dtype} "
                       f"{tuple(w_lo16.shape)}")
    p, lib, _ws = _gemm_params(a16, w16, M=M, N=N, K=K, lda=lda, a_mode=a_mode, conv=conv, tconv=tconv, bias=bias, rowbias=rowbias,
                               rb_rows=rb_rows, rb_mod=rb_mod, res1=res1, ldr1=ldr1, res2=res2, ldr2=ldr2, out32=out32, ldc32=ldc32,
                               out16=out16, ldc16=ldc16, out16t=out16t, ldt=ldt, t_rows=t_rows, t_gstride=t_gstride, n_split=n_split,
                               act=act, geglu=geglu, a16_lo=a16_lo, out16_lo=out16_lo, w_ld=w_ld, w_lo=w_lo, ln_gamma=ln_gamma,
                               ln_beta=ln_beta, ln_out16=ln_out16, ldln=ldln, ln_eps=ln_eps, gn_part=gn_part)
    fam = ("gemm_plain", "gemm_conv3x3", "gemm_conv1d_t")[a_mode]
    trailing_ln = ln_out16 is not None and not ln_in_library and not lib.pnc_gemm_fuses_layernorm(C.byref(p))
    if trailing_ln:
        # rows span several workgroups: the library would launch its LayerNorm kernel after the GEMM.  Issue the two launches
        # from here instead (the same two kernels) so that the per-family timing of bench.py sees them separately.
        p.ln_gamma = p.ln_beta = p.ln_out16 = None
    if w_lo16 is not None:
        _check(_timed(fam, 2.0 * M * N * K, 0.0, lib.pnc_gemm_wsplit_f16, C.byref(p), _ptr(w_lo16, torch.float16, "w_lo16"), _stream()),
               "pnc_gemm_wsplit_f16")
    else:
        _check(_timed(fam, 2.0 * M * N * K, 0.0, lib.pnc_gemm_f16, C.byref(p), _stream()), "pnc_gemm_f16")
    if trailing_ln:
        layernorm(out32, ldc32, M, N, ln_gamma, ln_beta, ln_eps, ln_out16, ldln)


def gemm_fuses_layernorm(**kw) -> bool:
    """pnc_gemm_fuses_layernorm for the arguments of `gemm`: does the launch normalise its rows in its own epilogue?"""
    kw.pop("ln_in_library", None)
    p, lib, _ws = _gemm_params(**kw, workspace=False)
    return bool(lib.pnc_gemm_fuses_layernorm(C.byref(p)))


def _gemm_params(a16, w16, *, M, N, K, lda=0, a_mode=A_PLAIN, conv=None, tconv=None, bias=None, rowbias=None, rb_rows=0, rb_mod=0,
                 res1=None, ldr1=0, res2=None, ldr2=0, out32=None, ldc32=0, out16=None, ldc16=0, out16t=None, ldt=0, t_rows=0,
                 t_gstride=0, n_split=0, act=ACT_NONE, geglu=False, a16_lo=None, out16_lo=None, w_ld=0, w_lo=None, ln_gamma=None,
                 ln_beta=None, ln_out16=None, ldln=0, ln_eps=1e-5, gn_part=None, workspace=True):
    """-> (PncGemmParams of the arguments of `gemm`, the library, the split-K workspace the struct points to or None); workspace =
    False: a struct for a query only, no workspace is allocated"""
    p = GemmParams()
    p.struct_bytes = C.sizeof(GemmParams)
    f16, f32 = torch.float16, torch.float32
    p.A, p.W = _ptr(a16, f16, "a16"), _ptr(w16, f16, "w16")
    p.a_lo_fmt, p.out_lo_fmt = lo_fmt(a16_lo), lo_fmt(out16_lo)
    p.A_lo, p.out16_lo = _ptr(a16_lo, LO_DTYPE[p.a_lo_fmt], "a16_lo"), _ptr(out16_lo, LO_DTYPE[p.out_lo_fmt], "out16_lo")
    if p.a_lo_fmt == LO_E4M3:
        if w_lo is None:
            raise PncError("an e4m3 lo plane needs the e4m3 copy of the weights (w_lo = engine.pk_lo8(w16))")
        p.W_lo, p.w_lo_exp = _ptr(w_lo[0], torch.uint8, "w_lo"), int(w_lo[1])
        p.ldw_lo = w_lo[0].shape[-1]
    elif w_lo is not None:         # split weights; the library refuses the plane without an fp16 a16_lo
        p.W_lo, p.ldw_lo = _ptr(w_lo, f16, "w_lo"), w_ld
    p.M, p.N, p.K, p.lda, p.a_mode, p.ldw = M, N, K, lda, a_mode, w_ld
    if ln_out16 is not None:       # LayerNorm of the fp32 output rows, fused into the GEMM where a workgroup owns whole rows
        p.ln_gamma, p.ln_beta, p.ln_out16 = _ptr(ln_gamma, torch.float32, "ln_gamma"), _ptr(ln_beta, torch.float32, "ln_beta"), \
            _ptr(ln_out16, torch.float16, "ln_out16")
        p.ldln, p.ln_eps = ldln, ln_eps
    if conv:
        p.Cin, p.Hin, p.Win = conv["Cin"], conv["Hin"], conv["Win"]
        p.Hout, p.Wout = conv["Hout"], conv["Wout"]
        p.stride, p.upsample = conv.get("stride", 1), int(conv.get("upsample", 0))
        p.conv_pad_br = int(conv.get("pad_br", 0))
        p.x_halo_off = int(conv.get("x_halo_off", 0))
    if tconv:
        p.Cin, p.T, p.Npix = tconv["C"], tconv["T"], tconv["Npix"]
        p.t_halo = int(tconv.get("halo", 0))
    p.gn_part = _ptr(gn_part, f32, "gn_part")
    p.bias, p.rowbias, p.rb_rows, p.rb_mod = _ptr(bias, f32, "bias"), _ptr(rowbias, f32, "rowbias"), rb_rows, rb_mod
    p.res1, p.ldr1, p.res2, p.ldr2 = _ptr(res1, f32, "res1"), ldr1, _ptr(res2, f32, "res2"), ldr2
    p.out32, p.ldc32, p.out16, p.ldc16 = _ptr(out32, f32, "out32"), ldc32, _ptr(out16, f16, "out16"), ldc16
    p.out16t, p.ldt, p.t_rows, p.t_gstride = _ptr(out16t, f16, "out16t"), ldt, t_rows, t_gstride
    p.n_split = n_split if out16t is not None else N
    p.act, p.geglu = act, int(geglu)
    lib = load()
    nws = lib.pnc_gemm_workspace_floats(C.byref(p))      # > 0: the library wants to split K (small-M shapes)
    ws = None
    if nws > 0 and workspace:
        ws = torch.empty(nws, device=a16.device, dtype=torch.float32)
        p.ws, p.ws_floats = _ptr(ws), nws
    return p, lib, ws


def _attn_struct(q, ldq, k, ldk, vt, ldvt, vt_gstride, o, ldo, groups, heads, H, W, views, kvH, kvW, kv_views,
                 kv_rows_per_group, q_per_kv, kv_valid, segs, scale, causal=False, k_halo=None, vt_halo=None, into=None):
    """The filled PncAttnParams of `attn_views` / `attn_uses_text_kernel` / `attn_views_split` (`into`: its AttnSplitParams.a)"""
    p = AttnParams() if into is None else into
    p.q, p.ldq, p.k, p.ldk = _ptr(q), ldq, _ptr(k), ldk
    p.vt, p.ldvt, p.vt_gstride, p.o, p.ldo = _ptr(vt), ldvt, vt_gstride, _ptr(o), ldo
    p.groups, p.heads, p.H, p.W, p.views = groups, heads, H, W, views
    p.kvH, p.kvW, p.kv_views = kvH, kvW, kv_views
    p.kv_rows_per_group, p.q_per_kv, p.kv_valid = kv_rows_per_group, q_per_kv, kv_valid
    for v, s in enumerate(segs):
        p.nseg[v] = len(s)
        for j, u in enumerate(s):
            p.seg[v][j] = u
    p.scale, p.causal = scale, int(causal)
    if k_halo is not None:
        for i in range(2):
            p.k_halo[i], p.vt_halo[i] = _ptr(k_halo[i]), _ptr(vt_halo[i])
    return p


def attn_views(q, ldq, k, ldk, vt, ldvt, vt_gstride, o, ldo, *, groups, heads, H, W, views,
               kvH, kvW, kv_views, kv_rows_per_group, q_per_kv, kv_valid, segs, scale, causal=False, k_halo=None, vt_halo=None):
    """`k_halo` / `vt_halo`: pairs (left, right) of buffers with the geometry of k / vt whose view column 0 holds a neighbour rank's
    view — kv view id -1 / kv_views in `segs` (PncAttnParams.k_halo)"""
    p = _attn_struct(q, ldq, k, ldk, vt, ldvt, vt_gstride, o, ldo, groups, heads, H, W, views, kvH, kvW, kv_views, kv_rows_per_group,
                     q_per_kv, kv_valid, segs, scale, causal, k_halo, vt_halo)
    nq = H * (W // views)
    nkeys = sum(len(sv) for sv in segs) * kv_valid
    _check(_timed("attn_views", 4.0 * groups * heads * nq * nkeys * 64, 0.0, load().pnc_attn_views_f16,
                  C.byref(p), _stream()), "pnc_attn_views_f16")


def attn_uses_text_kernel(q, ldq, k, ldk, vt, ldvt, vt_gstride, o, ldo, *, groups, heads, H, W, views,
                          kvH, kvW, kv_views, kv_rows_per_group, q_per_kv, kv_valid, segs, scale, causal=False, k_halo=None, vt_halo=None) -> bool:
    """pnc_attn_uses_text_kernel: would `attn_views` with these arguments, under the current options, launch the single-pass few-key
    kernel?  Answered by the library's own dispatch predicate; nothing is launched."""
    p = _attn_struct(q, ldq, k, ldk, vt, ldvt, vt_gstride, o, ldo, groups, heads, H, W, views, kvH, kvW, kv_views, kv_rows_per_group,
                     q_per_kv, kv_valid, segs, scale, causal, k_halo, vt_halo)
    return bool(load().pnc_attn_uses_text_kernel(C.byref(p)))


def attn_views_split(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, *, groups, heads, H, W, views, kvH, kvW, kv_views,
                     kv_rows_per_group, q_per_kv, kv_valid, segs, scale):
    """pnc_attn_views_split_f16: the geometry of `attn_views` on split operands (every *_lo an fp16 plane with its hi plane's
    leading dimension); V is ROW-major, laid out like K"""
    f16 = torch.float16
    sp = AttnSplitParams()
    sp.struct_bytes = C.sizeof(AttnSplitParams)
    _attn_struct(q, ldq, k, ldk, v, ldv, 0, o, ldo, groups, heads, H, W, views, kvH, kvW, kv_views, kv_rows_per_group, q_per_kv,
                 kv_valid, segs, scale, into=sp.a)
    sp.q_lo, sp.k_lo = _ptr(q_lo, f16, "q_lo"), _ptr(k_lo, f16, "k_lo")
    sp.v_lo, sp.o_lo = _ptr(v_lo, f16, "v_lo"), _ptr(o_lo, f16, "o_lo")
    nq = H * (W // views)
    nkeys = sum(len(sv) for sv in segs) * kv_valid
    _check(_timed("attn_views_split", 12.0 * groups * heads * nq * nkeys * 64, 0.0, load().pnc_attn_views_split_f16,
                  C.byref(sp), _stream()), "pnc_attn_views_split_f16")


def attn_temporal_split(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, *, B, T, Npix, heads, scale):
    f16 = torch.float16
    nb = 16.0 * B * T * Npix * heads * 64
    _check(_timed("attn_temporal_split", 0.0, nb, load().pnc_attn_temporal_split_f16,
                  _ptr(q, f16, "q"), _ptr(q_lo, f16, "q_lo"), ldq, _ptr(k, f16, "k"), _ptr(k_lo, f16, "k_lo"), ldk,
                  _ptr(v, f16, "v"), _ptr(v_lo, f16, "v_lo"), ldv, _ptr(o, f16, "o"), _ptr(o_lo, f16, "o_lo"), ldo,
                  B, T, Npix, heads, scale, _stream()), "pnc_attn_temporal_split_f16")


def softmax_rows(s32, lds, M, N, scale, p16, ldp, causal=False, n_valid=0):
    _check(_timed("softmax_rows", 0.0, 6.0 * M * N, load().pnc_softmax_rows_f16, _ptr(s32), lds, M, N, scale, int(causal),
                  n_valid, _ptr(p16), ldp, _stream()), "pnc_softmax_rows_f16")


def attn_frame(q, ldq, k, ldk, vt, ldvt, vt_fstride, o, ldo, *, F, N, C, scale):
    """pnc_attn_frame_f16: o = softmax(scale * q k^T) v over the N tokens of each of F frames, single head of dim C (128 / 256 / 512),
    fused (online softmax, no N x N matrix), one launch; vt is V channel-major per frame (include/panacea_hip.h section 6)"""
    f16 = torch.float16
    _check(_timed("attn_frame", 4.0 * F * N * N * C, 0.0, load().pnc_attn_frame_f16, _ptr(q, f16, "q"), ldq, _ptr(k, f16, "k"), ldk,
                  _ptr(vt, f16, "vt"), ldvt, vt_fstride, _ptr(o, f16, "o"), ldo, F, N, C, scale, _stream()), "pnc_attn_frame_f16")


def attn_frame_split(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, *, F, N, C, scale):
    """pnc_attn_frame_split_f16: `attn_frame` on split operands (every *_lo an fp16 plane with its hi plane's leading dimension); V
    is ROW-major, laid out like K; three MFMA products per product of the single-plane kernel (include/panacea_hip.h section 6b)"""
    f16 = torch.float16
    _check(_timed("attn_frame_split", 12.0 * F * N * N * C, 0.0, load().pnc_attn_frame_split_f16,
                  _ptr(q, f16, "q"), _ptr(q_lo, f16, "q_lo"), ldq, _ptr(k, f16, "k"), _ptr(k_lo, f16, "k_lo"), ldk,
                  _ptr(v, f16, "v"), _ptr(v_lo, f16, "v_lo"), ldv, _ptr(o, f16, "o"), _ptr(o_lo, f16, "o_lo"), ldo,
                  F, N, C, scale, _stream()), "pnc_attn_frame_split_f16")


def attn_text_split(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, *, groups, heads, Lp, kv_valid, scale):
    """pnc_attn_text_split_f16: the text tower's causal self-attention on split operands, all heads (of 64) of all prompts (groups of
    Lp <= 96 token rows, the first kv_valid of them real keys) in one launch; V is ROW-major like K, so q / k / v may be column blocks
    of one QKV buffer (include/panacea_hip.h section 6c).  Flops: three MFMA products per product, about half the tiles causal."""
    f16 = torch.float16
    _check(_timed("attn_text_split", 6.0 * groups * heads * Lp * kv_valid * 64, 0.0, load().pnc_attn_text_split_f16,
                  _ptr(q, f16, "q"), _ptr(q_lo, f16, "q_lo"), ldq, _ptr(k, f16, "k"), _ptr(k_lo, f16, "k_lo"), ldk,
                  _ptr(v, f16, "v"), _ptr(v_lo, f16, "v_lo"), ldv, _ptr(o, f16, "o"), _ptr(o_lo, f16, "o_lo"), ldo,
                  groups, heads, Lp, kv_valid, scale, _stream()), "pnc_attn_text_split_f16")


def attn_temporal(q, ldq, k, ldk, v, ldv, o, ldo, *, B, T, Npix, heads, scale):
    nb = 8.0 * B * T * Npix * heads * 64
    _check(_timed("attn_temporal", 0.0, nb, load().pnc_attn_temporal_f16, _ptr(q), ldq, _ptr(k), ldk, _ptr(v), ldv,
                  _ptr(o), ldo, B, T, Npix, heads, scale, _stream()), "pnc_attn_temporal_f16")


def _lo_bytes(t) -> float:
    return 0.0 if t is None else float(t.element_size())


def groupnorm_stats(x32, ldx, F, Npix, Cch, ppc, partial):
    _check(_timed("groupnorm", 0.0, 4.0 * F * Npix * Cch, load().pnc_groupnorm_stats, _ptr(x32), ldx, F, Npix, Cch,
                  ppc, _ptr(partial), _stream()), "pnc_groupnorm_stats")


def groupnorm_combine(parts_in, parts, F, nchunk, out):
    _check(load().pnc_groupnorm_combine(_ptr(parts_in), parts, F, nchunk, _ptr(out), _stream()), "pnc_groupnorm_combine")


def groupnorm_apply(x32, ldx, F, Npix, Cch, ppc, partial, gamma, beta, eps, silu, y16, ldy, y16_lo=None, n_records=0):
    nb = (6.0 + _lo_bytes(y16_lo)) * F * Npix * Cch
    _check(_timed("groupnorm", 0.0, nb, load().pnc_groupnorm_apply, _ptr(x32), ldx, F, Npix, Cch,
                  ppc, _ptr(partial), _ptr(gamma), _ptr(beta), eps, int(silu), _ptr(y16), ldy, _ptr(y16_lo), lo_fmt(y16_lo),
                  int(n_records), _stream()),
           "pnc_groupnorm_apply")


def groupnorm_temporal_silu(x32, B, T, Npix, Cch, gamma, beta, eps, y16, y16_lo=None):
    nb = (6.0 + _lo_bytes(y16_lo)) * B * T * Npix * Cch
    _check(_timed("groupnorm_temporal", 0.0, nb, load().pnc_groupnorm_temporal_silu,
                  _ptr(x32), B, T, Npix, Cch, _ptr(gamma), _ptr(beta), eps, _ptr(y16), _ptr(y16_lo), lo_fmt(y16_lo), _stream()),
           "pnc_groupnorm_temporal_silu")


def groupnorm_temporal_part(x32, B, T, Npix, Cch, gamma, beta, eps, stats, mode, T_total, y16=None, y16_lo=None, t_pad=0):
    """mode 1: this rank's {sum, sum of squares} per (pixel, group) over its T frames -> stats [B*Npix, 32, 2]; mode 2: normalise +
    SiLU with the sums of the whole frame group (T_total frames per sample), into the (T + 2 t_pad)-frame layout"""
    nb = (4.0 if mode == 1 else 6.0 + _lo_bytes(y16_lo)) * B * T * Npix * Cch
    _check(_timed("groupnorm", 0.0, nb, load().pnc_groupnorm_temporal_part, _ptr(x32), B, T, Npix, Cch, _ptr(gamma), _ptr(beta), eps,
                  _ptr(stats), mode, T_total, _ptr(y16), _ptr(y16_lo), lo_fmt(y16_lo), t_pad, _stream()), "pnc_groupnorm_temporal_part")


def layernorm(x32, ldx, M, Cch, gamma, beta, eps, y16, ldy, y16_lo=None):
    nb = (8.0 if y16_lo is not None else 6.0) * M * Cch
    _check(_timed("layernorm", 0.0, nb, load().pnc_layernorm, _ptr(x32), ldx, M, Cch, _ptr(gamma),
                  _ptr(beta), eps, _ptr(y16), ldy, _ptr(y16_lo), _stream()), "pnc_layernorm")


def linear_smallm(a32, lda, w16, bias, out32, ldo, M, N, K, silu_in=False, silu_out=False, w_lo=None):
    """`w_lo`: the fp16 lo plane of split weights (pnc_linear_smallm_split)"""
    name, lo = _sibling("pnc_linear_smallm", "_split", w_lo, "w_lo", torch.float16)
    _check(_timed("linear_smallm", 2.0 * M * N * K, (2.0 + 2.0 * len(lo)) * N * K, getattr(load(), name), _ptr(a32), lda, _ptr(w16), *lo,
                  _ptr(bias), _ptr(out32), ldo, M, N, K, int(silu_in), int(silu_out), _stream()), name)


def linear_smallm_segments(a32, lda, w16, bias, out32, M, m0, Mtot, N, K, seg_start, silu_in=False, silu_out=False, w_lo=None):
    """the same linear for len(seg_start) - 1 sites in one launch: out32 = one contiguous [Mtot, width] block per site, blocks back
    to back (include/panacea_hip.h); `seg_start` = the sites' first columns + [N], a host sequence; `w_lo`: the fp16 lo plane of
    split weights (pnc_linear_smallm_segments_split)"""
    segs = (C.c_int32 * len(seg_start))(*seg_start)
    name, lo = _sibling("pnc_linear_smallm_segments", "_split", w_lo, "w_lo", torch.float16)
    _check(_timed("linear_smallm", 2.0 * M * N * K, (2.0 + 2.0 * len(lo)) * N * K, getattr(load(), name), _ptr(a32), lda, _ptr(w16), *lo,
                  _ptr(bias), _ptr(out32), M, m0, Mtot, N, K, C.cast(segs, C.c_void_p), len(seg_start) - 1, int(silu_in),
                  int(silu_out), _stream()), name)


def timestep_embedding(t_i64, F, dim, freqs, out32):
    _check(load().pnc_timestep_embedding(_ptr(t_i64), F, dim, _ptr(freqs), _ptr(out32), _stream()),
           "pnc_timestep_embedding")


def timestep_embedding_f32(t_f32, F, dim, freqs, out32):
    """pnc_timestep_embedding_f32: float timesteps (a continuous c_noise), evaluated as given"""
    _check(load().pnc_timestep_embedding_f32(_ptr(t_f32, torch.float32, "t"), F, dim, _ptr(freqs), _ptr(out32), _stream()),
           "pnc_timestep_embedding_f32")


def nchw_to_tokens_f16(a32, C1, b32, C2, F, Npix, Cpad, out16, out16_lo=None, a_scale=None, a_frames=0):
    _check(_timed("layout", 0.0, F * Npix * (4.0 * (C1 + C2) + 2.0 * Cpad), load().pnc_nchw_to_tokens_f16, _ptr(a32),
                  C1, _ptr(a_scale), a_frames or F, _ptr(b32), C2, F, Npix, Cpad, _ptr(out16), _ptr(out16_lo), _stream()),
           "pnc_nchw_to_tokens_f16")


def u8_to_tokens_f16(src_u8, lut32, F, Npix, Cch, Cpad, out16, out16_lo=None):
    """pnc_u8_to_tokens_f16: uint8 channels-last frames [F, Npix, Cch] (contiguous, any byte address) -> fp16 tokens [F * Npix, Cpad]
    (+ lo plane) through the 256-entry fp32 device table `lut32`"""
    if not src_u8.is_contiguous() or src_u8.numel() != F * Npix * Cch:
        raise PncError(f"u8_to_tokens_f16: src is {F} x {Npix} x {Cch} contiguous bytes, got {tuple(src_u8.shape)} "
                       f"(contiguous: {src_u8.is_contiguous()})")
    if lut32.numel() != 256 or not lut32.is_contiguous():
        raise PncError(f"u8_to_tokens_f16: the table is 256 contiguous fp32 values, got {tuple(lut32.shape)}")
    nb = F * Npix * (1.0 * Cch + (2.0 if out16_lo is None else 4.0) * Cpad)
    _check(_timed("layout", 0.0, nb, load().pnc_u8_to_tokens_f16, _ptr(src_u8, torch.uint8, "src"), _ptr(lut32, torch.float32, "lut"),
                  F, Npix, Cch, Cpad, _ptr(out16, torch.float16, "out16"), _ptr(out16_lo, torch.float16, "out16_lo"), _stream()),
           "pnc_u8_to_tokens_f16")


def tokens_to_u8(x32, ld, M, Cch, out_u8):
    """pnc_tokens_to_u8: the first Cch <= 8 columns of M fp32 token rows (row stride ld) -> uint8 [M, Cch], the reference's
    clamp / (x + 1) / 2 / * 255 / truncate per element (inference.py:189-193)"""
    if not out_u8.is_contiguous() or out_u8.numel() != M * Cch:
        raise PncError(f"tokens_to_u8: out is {M} x {Cch} contiguous bytes, got {tuple(out_u8.shape)}")
    _check(_timed("layout", 0.0, M * Cch * 5.0, load().pnc_tokens_to_u8, _ptr(x32, torch.float32, "x"), ld, M, Cch,
                  _ptr(out_u8, torch.uint8, "out"), _stream()), "pnc_tokens_to_u8")


def cfg_euler_step(eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, sigma, sigma_next, x_next, c_skip=None):
    """`c_skip`: a [T] fp32 vector selects pnc_cfg_euler_step_skip (D = eps * c_out + x * c_skip); None = the eps path"""
    name, skip = _sibling("pnc_cfg_euler_step", "_skip", c_skip, "c_skip", torch.float32)
    _check(_timed("elementwise", 0.0, T * Npix * Cch * (16.0 if cfg else 12.0), getattr(load(), name), _ptr(eps_tok), ld, T, Npix, Cch,
                  int(cfg), float(scale), _ptr(x), *skip, _ptr(c_out), _ptr(sigma), _ptr(sigma_next), _ptr(x_next), _stream()), name)


def cfg_sampler_step(mode, eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, v, out, out_aux=None, x0=None, aux=None,
                     hist=(), noise=None, s_noise=1.0, c_skip=None):
    """pnc_cfg_sampler_step: `v` = the mode's per-frame [T] fp32 vectors in header order, `hist` = previous LMS d planes newest first;
    `c_skip`: a [T] fp32 vector selects pnc_cfg_sampler_step_skip (D = eps * c_out + x * c_skip); None = the eps path"""
    p = SamplerStepParams()
    p.struct_bytes = C.sizeof(SamplerStepParams)
    f32 = torch.float32
    p.mode, p.ld, p.T, p.Npix, p.C, p.cfg, p.scale = mode, ld, T, Npix, Cch, int(cfg), float(scale)
    p.eps_tok, p.x, p.c_out = _ptr(eps_tok, f32, "eps_tok"), _ptr(x, f32, "x"), _ptr(c_out, f32, "c_out")
    p.x0, p.aux, p.noise = _ptr(x0, f32, "x0"), _ptr(aux, f32, "aux"), _ptr(noise, f32, "noise")
    p.out, p.out_aux = _ptr(out, f32, "out"), _ptr(out_aux, f32, "out_aux")
    if len(v) > 6 or len(hist) > 4:
        raise PncError("cfg_sampler_step: at most 6 per-frame vectors and 4 history planes")
    for k, t in enumerate(v):
        p.v[k] = _ptr(t, f32, f"v[{k}]")
    for k, t in enumerate(hist):
        p.hist[k] = _ptr(t, f32, f"hist[{k}]")
    p.n_hist, p.s_noise = len(hist), float(s_noise)
    planes = 3 + (x0 is not None) + (aux is not None) + (noise is not None) + (out_aux is not None) + len(hist)
    nbytes = T * Npix * Cch * (4.0 * planes + (4.0 if cfg else 0.0))
    name, skip = _sibling("pnc_cfg_sampler_step", "_skip", c_skip, "c_skip", f32)
    _check(_timed("elementwise", 0.0, nbytes, getattr(load(), name), C.byref(p), *skip, _stream()), name)


def frames_renoise(z, noise, sigma, out, keep=None, x=None):
    """pnc_frames_renoise on (T, C, ...) fp32 latents: out[t] = z[t] + noise[t] * sigma[t] where keep[t] > 0 (`keep` None: every
    frame), x[t] elsewhere; `sigma`, `keep`: [T] fp32 on the device.  `out` may be `x` (frames that are not kept stay untouched)"""
    f32 = torch.float32
    T, Cch = z.shape[0], z.shape[1]
    planes = [("z", z), ("noise", noise), ("out", out)] + ([] if x is None else [("x", x)])
    for name, t in planes:
        if t.shape != z.shape or not t.is_contiguous():
            raise PncError(f"frames_renoise: {name} is a contiguous {tuple(z.shape)} latent, got {tuple(t.shape)} "
                           f"(contiguous: {t.is_contiguous()})")
    for name, t in (("sigma", sigma), ("keep", keep)):
        if t is not None and (t.shape != (T,) or not t.is_contiguous()):
            raise PncError(f"frames_renoise: {name} is a contiguous [{T}] vector, got {tuple(t.shape)}")
    if keep is not None and x is None:
        raise PncError("frames_renoise: frames that are not kept come from `x`")
    Npix = z[0, 0].numel() if z.dim() > 2 else 1
    _check(_timed("elementwise", 0.0, 12.0 * z.numel(), load().pnc_frames_renoise, _ptr(z, f32, "z"), _ptr(noise, f32, "noise"),
                  _ptr(sigma, f32, "sigma"), _ptr(keep, f32, "keep"), _ptr(x, f32, "x"), _ptr(out, f32, "out"), T, Cch, Npix,
                  _stream()), "pnc_frames_renoise")


def latent_renoise_masked(z, noise, sigma, mask, x, out):
    """pnc_latent_renoise_masked on (T, C, ...) fp32 latents: per element out = z + noise * sigma[t] where mask[t] > 0 at its pixel,
    x elsewhere; `mask`: (T, ...) fp32 of a frame's pixels (one row for the C planes), `sigma`: [T] fp32.  `out` may be `x`"""
    f32 = torch.float32
    T, Cch = z.shape[0], z.shape[1]
    for name, t in (("z", z), ("noise", noise), ("x", x), ("out", out)):
        if t.shape != z.shape or not t.is_contiguous():
            raise PncError(f"latent_renoise_masked: {name} is a contiguous {tuple(z.shape)} latent, got {tuple(t.shape)} "
                           f"(contiguous: {t.is_contiguous()})")
    if sigma.shape != (T,) or not sigma.is_contiguous():
        raise PncError(f"latent_renoise_masked: sigma is a contiguous [{T}] vector, got {tuple(sigma.shape)}")
    if mask.shape != (T,) + tuple(z.shape[2:]) or not mask.is_contiguous():
        raise PncError(f"latent_renoise_masked: mask is a contiguous {(T,) + tuple(z.shape[2:])} selector, got {tuple(mask.shape)} "
                       f"(contiguous: {mask.is_contiguous()})")
    Npix = z[0, 0].numel() if z.dim() > 2 else 1
    # what the entry must move at most: z, noise and out of every element, the mask once per frame (x only where nothing is kept)
    _check(_timed("elementwise", 0.0, 12.0 * z.numel() + 4.0 * mask.numel(), load().pnc_latent_renoise_masked, _ptr(z, f32, "z"),
                  _ptr(noise, f32, "noise"), _ptr(sigma, f32, "sigma"), _ptr(mask, f32, "mask"), _ptr(x, f32, "x"),
                  _ptr(out, f32, "out"), T, Cch, Npix, _stream()), "pnc_latent_renoise_masked")


def mask_pool_u8(mask_u8, f, out):
    """pnc_mask_pool_u8: a (T, H, W) uint8 pixel mask -> the (T, H / f, W / f) fp32 selector `out`: 1.0 where all f x f bytes of the
    cell are nonzero, 0.0 elsewhere"""
    if mask_u8.dim() != 3 or not mask_u8.is_contiguous():
        raise PncError(f"mask_pool_u8: mask_u8 is a contiguous (T, H, W) byte mask, got {tuple(mask_u8.shape)} "
                       f"(contiguous: {mask_u8.is_contiguous()})")
    T, H, W = mask_u8.shape
    if isinstance(f, bool) or not isinstance(f, int) or not 1 <= f <= 16 or H % f or W % f:
        raise PncError(f"mask_pool_u8: f is an int in 1 .. 16 that divides {H} and {W}, got {f!r}")
    if out.shape != (T, H // f, W // f) or not out.is_contiguous():
        raise PncError(f"mask_pool_u8: out is a contiguous {(T, H // f, W // f)} selector, got {tuple(out.shape)}")
    _check(_timed("elementwise", 0.0, 1.0 * mask_u8.numel() + 4.0 * out.numel(), load().pnc_mask_pool_u8,
                  _ptr(mask_u8, torch.uint8, "mask_u8"), _ptr(out, torch.float32, "out"), T, H, W, f, _stream()), "pnc_mask_pool_u8")


def u8_select(src, gen, mask_u8, out):
    """pnc_u8_select on (..., C <= 4) uint8 channels-last frames: out = src where the pixel's byte of `mask_u8` (the frames' shape
    without the channels) is nonzero, gen elsewhere.  `out` may be `gen`, never `src`"""
    for name, t in (("src", src), ("gen", gen), ("out", out)):
        if t.shape != src.shape or not t.is_contiguous():
            raise PncError(f"u8_select: {name} holds contiguous {tuple(src.shape)} frames, got {tuple(t.shape)} "
                           f"(contiguous: {t.is_contiguous()})")
    if src.dim() < 2 or not 1 <= src.shape[-1] <= 4:
        raise PncError(f"u8_select: channels-last frames of 1 .. 4 channels, got {tuple(src.shape)}")
    if mask_u8.shape != src.shape[:-1] or not mask_u8.is_contiguous():
        raise PncError(f"u8_select: mask_u8 is a contiguous {tuple(src.shape[:-1])} byte mask, got {tuple(mask_u8.shape)}")
    u8 = torch.uint8
    _check(_timed("elementwise", 0.0, 3.0 * src.numel() + 1.0 * mask_u8.numel(), load().pnc_u8_select, _ptr(src, u8, "src"),
                  _ptr(gen, u8, "gen"), _ptr(mask_u8, u8, "mask_u8"), _ptr(out, u8, "out"), mask_u8.numel(), src.shape[-1], _stream()),
           "pnc_u8_select")


def tokens_to_nchw_f32(x32, ld, F, Npix, Cch, out32):
    _check(load().pnc_tokens_to_nchw_f32(_ptr(x32), ld, F, Npix, Cch, _ptr(out32), _stream()),
           "pnc_tokens_to_nchw_f32")


def concat_add(a32, C1, s32, c32, C2, M, out32, out16, out16_lo=None, gn_part=None, frames=0, ppc=64):
    """`gn_part` (+ `frames`: M = frames * Npix; `ppc`: pixels per record): also write the GroupNorm(32) records of the output
    (pnc_concat_add_stats; [frames][ceil(Npix / ppc)][32][3] floats) — the GroupNorm that reads the concat then launches no statistics"""
    nb = M * (4.0 * C1 + (8.0 if c32 is not None else 4.0) * C2 + (6.0 + _lo_bytes(out16_lo)) * (C1 + C2))
    if gn_part is not None and (frames < 1 or M % frames):
        raise PncError(f"concat_add with gn_part: M = {M} rows are not {frames} whole frames")
    name, part = _sibling("pnc_concat_add", "_stats", gn_part, "gn_part", torch.float32)
    rows = (frames, M // frames, ppc) if part else (M,)          # the sibling takes the rows as frames x pixels, and the record size
    _check(_timed("elementwise", 0.0, nb, getattr(load(), name), _ptr(a32), C1, _ptr(s32), _ptr(c32), C2, *rows, _ptr(out32), _ptr(out16),
                  _ptr(out16_lo), lo_fmt(out16_lo), *part, _stream()), name)


def add_f32(x32, a32, n, y32, y16, y16_lo=None):
    _check(_timed("elementwise", 0.0, 12.0 * n, load().pnc_add_f32, _ptr(x32), _ptr(a32), n, _ptr(y32), _ptr(y16),
                  _ptr(y16_lo), lo_fmt(y16_lo), _stream()), "pnc_add_f32")


def upsample_combine(P, ldp, bias, F, Hin, Win, Cout, out32, out16=None, out16_lo=None):
    """pnc_upsample_combine: the nine tap products P [F * Hin * Win, ldp >= 9 * Cout] fp32 of a nearest-x2 Upsample conv, one row per
    SOURCE pixel (column (u * 3 + v) * Cout + n), summed with `bias` into out32 [F * 2 Hin * 2 Win, Cout] (+ its fp16 / lo planes)"""
    rows, outs = F * Hin * Win, 4 * F * Hin * Win * Cout
    short = [t for t in (out32, out16, out16_lo) if t is not None and t.numel() < outs]      # (the library sees pointers only)
    if P.numel() < (rows - 1) * ldp + 9 * Cout or short:
        raise PncError(f"upsample_combine: P holds {rows} rows of {9 * Cout} products (ldp {ldp}) and every output {outs} elements")
    fmt = lo_fmt(out16_lo)
    nb = 36.0 * rows * Cout + outs * (4.0 + (2.0 if out16 is not None else 0.0) + _lo_bytes(out16_lo))
    _check(_timed("upsample_combine", 0.0, nb, load().pnc_upsample_combine, _ptr(P, torch.float32, "P"), ldp,
                  _ptr(bias, torch.float32, "bias"), F, Hin, Win, Cout, _ptr(out32, torch.float32, "out32"),
                  _ptr(out16, torch.float16, "out16"), _ptr(out16_lo, LO_DTYPE[fmt], "out16_lo"), fmt, _stream()),
           "pnc_upsample_combine")


def range_monitor_collect(out_i32: torch.Tensor):
    """adds the number of e4m3 lo-plane quads that CLAMPED since the previous call to out_i32[0] (a device int32 word) and resets the
    library's counters (include/panacea_hip.h: pnc_range_monitor_collect)"""
    _check(load().pnc_range_monitor_collect(_ptr(out_i32, torch.int32, "out"), _stream()), "pnc_range_monitor_collect")


STATS_WORDS = 36         # PNC_STATS_WORDS: 64-bit words of one record of pnc_operand_stats_f16


def operand_stats(hi, lo, rows, cols, ld, rec):
    """pnc_operand_stats_f16: ADDS the range statistics of the operand plane `hi` (fp16; `rows` rows of `cols` elements, `ld` elements
    between rows) and of its lo plane `lo` (None, fp16 or uint8 = e4m3 bytes, same ld in elements) to the record `rec`, an int64
    device tensor of at least STATS_WORDS contiguous words (binade histogram, maximum, saturation counts: include/panacea_hip.h)"""
    if rec.dtype != torch.int64 or rec.numel() < STATS_WORDS or not rec.is_contiguous():
        raise PncError(f"operand_stats: the record is {STATS_WORDS} contiguous int64 words, got {rec.dtype} x {rec.numel()}")
    fmt = lo_fmt(lo)
    nb = rows * cols * (2.0 + _lo_bytes(lo))
    _check(_timed("operand_stats", 0.0, nb, load().pnc_operand_stats_f16, _ptr(hi, torch.float16, "hi"), _ptr(lo, LO_DTYPE[fmt], "lo"),
                  fmt, rows, cols, ld, _ptr(rec, torch.int64, "rec"), _stream()), "pnc_operand_stats_f16")


def cast_f16(x32, n, y16, y16_lo=None):
    _check(load().pnc_cast_f16(_ptr(x32), n, _ptr(y16), _ptr(y16_lo), lo_fmt(y16_lo), _stream()), "pnc_cast_f16")
