"""The fused first-stage attention (include/panacea_hip.h section 6, pnc_attn_frame_f16) without a GPU: header and binding, the
argument checks of the entry point (nothing is launched), the dispatch of AttnBlock on a stub backend that offers the capability,
the float64 reference against torch's own attention, and the source scan that keeps tests/test_emu_surface.py meaningful.

The kernel itself is held to the same float64 reference in tests/test_frame_attn_gpu.py."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest
import torch

import attn_edge_cases as cases
import emu
import frame_attn_ref64 as ref64
from panacea_amd import engine as E, hip
from panacea_amd.nn import model

PKG = Path(hip.__file__).resolve().parent
STRUCTS = {"PncGemmParams": hip.GemmParams, "PncAttnParams": hip.AttnParams, "PncAttnSplitParams": hip.AttnSplitParams,
           "PncSamplerStepParams": hip.SamplerStepParams}


# ------------------------------------------------------------------------------------------ 1. header and binding
def test_header_and_binding(tmp_path):
    assert "pnc_attn_frame_f16" in hip.header_symbols() and "pnc_attn_frame_f16" in hip._SIGNATURES
    assert set(hip.header_symbols()) == set(hip._SIGNATURES)
    res, args = hip._SIGNATURES["pnc_attn_frame_f16"]
    L, P, I = ctypes.c_int64, ctypes.c_void_p, ctypes.c_int
    assert res is I and args == [P, L, P, L, P, L, L, P, L, I, I, I, ctypes.c_float, P]
    src = ['#include <stdio.h>', f'#include "{hip.HEADER}"', 'int main(void) {']
    src += [f'printf("{st} %zu\\n", sizeof({st}));' for st in STRUCTS]
    src.append('printf("abi %d\\n", PNC_ABI_VERSION); return 0; }')
    c = tmp_path / "sizes.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "sizes"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(c), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    for st, cls in STRUCTS.items():
        assert int(got[st]) == ctypes.sizeof(cls), st
    assert int(got["abi"]) == hip.ABI_VERSION == 8
    assert hip.OPT_ATTN_SUM_TRIGGER == 11                 # no new library option: set_option range-checks against this one
    with pytest.raises(hip.PncError):
        hip.set_option(12, 0)


# ------------------------------------------------------------------------------------------ 2. argument checks, no device
def test_entry_point_refuses_before_any_launch():
    lib = hip.load()
    buf = (ctypes.c_char * 64)()
    a16 = (ctypes.addressof(buf) + 15) & ~15
    ok, odd = ctypes.c_void_p(a16), ctypes.c_void_p(a16 + 2)

    def call(q=ok, k=ok, vt=ok, o=ok, F=2, N=64, C=128, ldq=None, ldk=None, ldvt=None, fstride=None, ldo=None):
        ldq, ldk, ldo = (C if v is None else v for v in (ldq, ldk, ldo))
        ldvt = N if ldvt is None else ldvt
        fstride = C * ldvt if fstride is None else fstride
        return lib.pnc_attn_frame_f16(q, ldq, k, ldk, vt, ldvt, fstride, o, ldo, F, N, C, 0.125, None)

    EINVAL, EALIGN = -1, -2
    # ranges are looked at before alignment: the pointers of these calls are misaligned as well
    for kw in (dict(C=64), dict(C=384), dict(N=0), dict(N=12), dict(F=0), dict(N=-8), dict(C=0)):
        assert call(q=odd, k=odd, vt=odd, o=odd, **kw) == EINVAL, kw
        assert call(**kw) == EINVAL, kw
    for name in ("q", "k", "vt", "o"):
        assert call(**{name: None}) == EINVAL, name
        assert call(**dict(dict(q=odd, k=odd, vt=odd, o=odd), **{name: None})) == EINVAL, name
    # one workgroup per 64 queries of a frame: the grid must fit
    assert call(q=odd, F=2 ** 31 - 1, N=2 ** 20) == EINVAL
    # leading dimensions (aligned pointers: the leading dimensions come first)
    for kw in (dict(ldq=132), dict(ldk=129), dict(ldo=130), dict(ldvt=68), dict(fstride=128 * 64 + 4)):
        assert call(**kw) == EALIGN, kw
    # pointers
    for name in ("q", "k", "vt", "o"):
        assert call(**{name: odd}) == EALIGN, name
    # valid-looking ranges of every instantiated width stop at the alignment check
    for C in (128, 256, 512):
        for F, N in ((1, 8), (3, 264), (1, 49152), (8, 12288)):
            assert call(q=odd, k=odd, vt=odd, o=odd, F=F, N=N, C=C) == EALIGN, (F, N, C)
            assert call(o=odd, F=F, N=N, C=C, ldq=C + 8, ldk=C + 16, ldo=C + 8, ldvt=N + 8, fstride=C * (N + 8) + 8) == EALIGN


# ------------------------------------------------------------------------------------------ 3. host dispatch on a stub backend
class _Stub:
    """tests/emu.py plus the optional capability: `attn_frame` computed by the float64 reference, rounded to fp16"""

    def __init__(self):
        self.frame_calls, self.softmax_calls = [], 0

    def __getattr__(self, name):
        return getattr(emu, name)

    def softmax_rows(self, *a, **kw):
        self.softmax_calls += 1
        return emu.softmax_rows(*a, **kw)

    def attn_frame(self, q, ldq, k, ldk, vt, ldvt, vt_fstride, o, ldo, *, F, N, C, scale):
        ref = ref64.attn_frame(q, ldq, k, ldk, vt, ldvt, vt_fstride, F=F, N=N, C=C, scale=scale)
        ref64.scatter_o(o, ldo, ref, F=F, N=N, C=C)
        self.frame_calls.append(dict(ldq=ldq, ldk=ldk, ldvt=ldvt, vt_fstride=vt_fstride, ldo=ldo, F=F, N=N, C=C, scale=scale,
                                     shapes=(tuple(q.shape), tuple(k.shape), tuple(vt.shape), tuple(o.shape)), ref=ref))


def _block(C, seed=5):
    torch.manual_seed(seed)
    blk = model.AttnBlock(C)
    with torch.no_grad():
        blk.norm.weight.uniform_(0.5, 1.5)
        blk.norm.bias.uniform_(-0.5, 0.5)
    return blk


def test_dispatch_fused_path_on_a_stub_backend(monkeypatch):
    """F = 3 frames of 8 x 33 tokens through AttnBlock(128) with the threshold at 0: ONE attn_frame call over all frames with the
    block's own strides, no row softmax, and an output next to the three-launch emulated path's.

    Bound.  Both runs form the same q / k / V^T (the emulation is deterministic) and differ in o16 alone.  The stub's o16 is the
    float64 attention a rounded to fp16 (|error| <= 2^-11 |a|, inside the unit-scale bound b = 3e-3 + 2e-3 |a|); the three-launch
    path is held to b like every attention of the project.  So |delta o16| <= 2 b elementwise, and through
    out = o16 W^T + bias + x the outputs differ by at most sum_c |W[n, c]| 2 b[m, c], plus the fp32 rounding of two
    C-term dot products and two final sums ((C + 2) 2^-24 of the sum of magnitudes, each)."""
    F, H, W, C = 3, 8, 33, 128
    N = H * W
    blk = _block(C)
    x = torch.randn(F, C, H, W, generator=torch.Generator().manual_seed(9))
    with E.use_backend(emu), torch.no_grad():
        base = blk(x)
    stub = _Stub()
    monkeypatch.setattr(model, "FUSED_ATTN_MIN_TOKENS", 0)
    with E.use_backend(stub), torch.no_grad():
        got = blk(x)
    assert len(stub.frame_calls) == 1 and stub.softmax_calls == 0
    call = stub.frame_calls[0]
    assert (call["F"], call["N"], call["C"]) == (F, N, C) and call["scale"] == float(C) ** -0.5
    assert (call["ldq"], call["ldk"], call["ldvt"], call["vt_fstride"], call["ldo"]) == (C, C, N, C * N, C)
    assert call["shapes"] == ((F * N, C), (F * N, C), (F, C, N), (F * N, C))
    assert got.dtype == torch.float32 and got.shape == base.shape and torch.isfinite(got).all()
    a = call["ref"].reshape(F * N, C)                                   # float64 attention output, token rows
    Wo = blk.proj_out.weight.detach().reshape(C, C).half().double().abs()
    atol, rtol = cases.UNIT
    tol = (2.0 * (atol + rtol * a.abs())) @ Wo.t()
    mag = a.abs() @ Wo.t() + blk.proj_out.bias.detach().double().abs()[None, :] + x.permute(0, 2, 3, 1).reshape(F * N, C).double().abs()
    tol = tol + 2.0 * (C + 2) * 2.0 ** -24 * mag
    diff = (got.double() - base.double()).permute(0, 2, 3, 1).reshape(F * N, C).abs()
    print(f"fused (float64 stub) vs three-launch emulation: max |diff| {diff.max():.3e}, max diff / bound {(diff / tol).max():.3g}")
    assert (diff <= tol).all()
    assert diff.max() > 0                                               # the two paths are not the same arithmetic


def test_dispatch_default_threshold_keeps_the_three_launch_path():
    assert model.FUSED_ATTN_MIN_TOKENS == 16385 == model.SOFTMAX_ROWS_MAX_TOKENS + 1
    blk = _block(128)
    x = torch.randn(3, 128, 8, 33, generator=torch.Generator().manual_seed(9))
    stub = _Stub()
    with E.use_backend(stub), torch.no_grad():
        got = blk(x)
    with E.use_backend(emu), torch.no_grad():
        base = blk(x)
    assert stub.frame_calls == [] and stub.softmax_calls == 3
    assert torch.equal(got, base)


class _NoAlloc(E.Runtime):
    def empty(self, *a, **kw):
        raise AssertionError("allocated before refusing")

    zeros = empty


@pytest.mark.parametrize("backend,C,match", [("emu", 128, r"backend"), ("stub", 64, r"64 channels")])
def test_long_frames_are_refused_before_any_allocation(backend, C, match):
    """N = 16392 (an 8 x 2049 frame) is beyond the row softmax: without the fused kernel — a backend that lacks it, or a channel count
    it is not built for — the block refuses at the top of _run and says which of the two it was"""
    be = emu if backend == "emu" else _Stub()
    blk = model.AttnBlock(C)
    blk.packed = lambda: (_ for _ in ()).throw(AssertionError("packed the weights before refusing"))
    with E.use_backend(be):
        rt = _NoAlloc(torch.device("cpu"), 1, 1)
        with pytest.raises(NotImplementedError, match=match) as ei:
            blk._run(rt, E.Act(1, 8, 2049, C))
    assert "16392" in str(ei.value)
    if backend == "stub":
        assert be.frame_calls == []
    # N % 8 stays required on both paths
    with E.use_backend(be), pytest.raises(NotImplementedError, match="multiples of 8"):
        blk._run(_NoAlloc(torch.device("cpu"), 1, 1), E.Act(1, 3, 7, C))


def test_threshold_from_the_environment(monkeypatch):
    monkeypatch.delenv("PNC_VAE_FUSED_ATTN_MIN_TOKENS", raising=False)
    assert model._fused_attn_min_tokens() == 16385
    for raw, want in (("0", 0), (" 4096 ", 4096), ("", 16385)):
        monkeypatch.setenv("PNC_VAE_FUSED_ATTN_MIN_TOKENS", raw)
        assert model._fused_attn_min_tokens() == want
    for raw in ("-1", "many", "1.5"):
        monkeypatch.setenv("PNC_VAE_FUSED_ATTN_MIN_TOKENS", raw)
        with pytest.raises(ValueError, match="PNC_VAE_FUSED_ATTN_MIN_TOKENS"):
            model._fused_attn_min_tokens()


# ------------------------------------------------------------------------------------------ 4. the reference against torch's attention
@pytest.mark.parametrize("F,N,C", [(2, 40, 128), (1, 72, 512)])
def test_reference_equals_torch_attention_in_float64(F, N, C):
    g = torch.Generator().manual_seed(N)
    q, k, v = (torch.randn(F, N, C, generator=g).half() for _ in range(3))
    scale = float(C) ** -0.5
    want = torch.nn.functional.scaled_dot_product_attention(q.double(), k.double(), v.double(), scale=scale)
    # dense storage, and the same values inside padded, NaN-filled storage with the strides of the GPU test
    dense = ref64.attn_frame(q, C, k, C, v.transpose(1, 2).contiguous(), N, C * N, F=F, N=N, C=C, scale=scale)
    assert (dense - want).abs().max() < 1e-12
    ldq, ldk, ldvt = C + 8, C + 16, N + 8
    fstride = C * ldvt + 8
    qp = torch.full((F * N, ldq), cases.NAN, dtype=torch.float16)
    kp = torch.full((F * N, ldk), cases.NAN, dtype=torch.float16)
    vp = torch.full((F * fstride,), cases.NAN, dtype=torch.float16)
    qp[:, :C], kp[:, :C] = q.reshape(F * N, C), k.reshape(F * N, C)
    for f in range(F):
        vp[f * fstride:f * fstride + C * ldvt].view(C, ldvt)[:, :N] = v[f].t()
    padded = ref64.attn_frame(qp, ldq, kp, ldk, vp, ldvt, fstride, F=F, N=N, C=C, scale=scale)
    assert torch.equal(padded, dense)
    rows = torch.tensor([0, 7, N - 1])
    assert torch.equal(ref64.attn_frame(qp, ldq, kp, ldk, vp, ldvt, fstride, F=F, N=N, C=C, scale=scale, rows=rows), dense[:, rows])
    o = torch.full((F * N + 2, C + 8), cases.NAN, dtype=torch.float16)
    ref64.scatter_o(o, C + 8, dense, F=F, N=N, C=C)
    assert torch.equal(o[:F * N, :C].double(), dense.reshape(F * N, C).half().double())
    assert torch.isnan(o[:, C:]).all() and torch.isnan(o[F * N:]).all()


# ------------------------------------------------------------------------------------------ 5. the capability is looked up, not called
def test_the_package_never_calls_the_capability_through_the_backend_handle():
    """tests/test_emu_surface.py demands every name called as `.be.NAME(` from tests/emu.py, which has no twin of the fused kernel:
    AttnBlock looks the capability up with getattr.  The scan's own expression must not find it either."""
    for f in PKG.rglob("*.py"):
        txt = f.read_text()
        assert ".be.attn_frame(" not in txt, f
        assert "attn_frame" not in re.findall(r"(?:\.be|backend\(\)|\bbe)\.([A-Za-z_]\w*)\s*\(", txt), f
    assert not hasattr(emu, "attn_frame")
    assert 'getattr(rt.be, "attn_frame", None)' in (PKG / "nn" / "model.py").read_text()
