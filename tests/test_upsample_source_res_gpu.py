"""The denoiser's Upsample conv at SOURCE resolution (MI355X): nn.openaimodel.Upsample._run through the plain-A GEMM on the source
pixels + pnc_upsample_combine, against the output-resolution conv it replaces (engine.UPSAMPLE_SOURCE_RES off, same process) and a
float64 conv; and pnc_upsample_combine alone, bit for bit, inside poisoned allocations.

Acceptance of the path (the summation tree differs, the operands do not): at every shape the new path's max-abs error against the
float64 conv on the SAME operand planes (hi + 2^-11 lo as the kernels read them) and fp16-rounded weights is at most twice the old
path's.  The kernel alone adds fp32 numbers in a specified order, so it must equal a torch emulation of the header's formula exactly."""
import pytest
import torch
import torch.nn.functional as TF

from helpers import measured
from panacea_amd import engine as E
from panacea_amd import hip
from panacea_amd.nn.openaimodel import Upsample

pytestmark = pytest.mark.gpu
DEV = "cuda"

# (F, Hin, Win, Cin, Cout, forced frames per chunk)
SHAPES = [
    (1, 1, 1, 64, 64, 0),          # every border at once
    (2, 2, 3, 64, 64, 0),
    (2, 3, 8, 128, 64, 0),         # odd height, several source tiles
    (1, 4, 6, 64, 320, 0),         # N = 2880: several column tiles, ragged against 256
    (3, 2, 4, 64, 64, 2),          # a last partial chunk
]


def _conv64(x_planes, F, H, W, C, w, b):
    """float64 nearest-x2 + conv2d on the operand the kernels read: hi + 2^-11 lo (lo: fp16, or e4m3 bytes), fp16-rounded weights"""
    x = x_planes.hi.double().cpu()
    if x_planes.lo is not None:
        lo = x_planes.lo.view(torch.float8_e4m3fn) if x_planes.lo.dtype == torch.uint8 else x_planes.lo
        x = x + lo.double().cpu() / 2048.0
    x = x.view(F, H, W, C).permute(0, 3, 1, 2)
    y = TF.conv2d(TF.interpolate(x, scale_factor=2, mode="nearest"), w.half().double().cpu(), b.double().cpu(), padding=1)
    return y.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


def _lo_planes_of(v32, lo_dtype):
    """the `stream` class's own writer on the same fp32 values: pnc_cast_f16"""
    hi = torch.empty(v32.shape, device=DEV, dtype=torch.float16)
    lo = torch.empty(v32.shape, device=DEV, dtype=lo_dtype)
    hip.cast_f16(v32, v32.numel(), hi, lo)
    return hi, lo


@pytest.mark.parametrize("prec", ["precise", "fast"])
@pytest.mark.parametrize("want_f16", [False, True], ids=["f32", "f32+f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_source_res_path_vs_output_res_path_and_float64(shape, want_f16, prec, monkeypatch):
    F, H, W, Cin, Cout, chunk = shape
    torch.manual_seed(1000 + 7 * F + H * W + Cout)
    up = Upsample(Cin, True, dims=2, out_channels=Cout).to(DEV)
    with torch.no_grad():
        up.conv.weight.normal_(0.0, (9 * Cin) ** -0.5)
        up.conv.bias.normal_(0.0, 0.1)
    x32 = torch.randn(F * H * W, Cin, device=DEV) * 1.5
    rt = E.Runtime(torch.device(DEV), 1, F)
    rt.prec = E.precision(prec)
    act = E.Act(F, H, W, Cin, f32=x32)
    planes = act.need_f16(rt)                       # both paths read these planes
    monkeypatch.setattr(E, "UPSAMPLE_CHUNK_FRAMES", chunk)
    out = {}
    for name, on in (("old", False), ("new", True)):
        monkeypatch.setattr(E, "UPSAMPLE_SOURCE_RES", on)
        with torch.no_grad():
            out[name] = up._run(rt, act, want_f16=want_f16)
    torch.cuda.synchronize()
    ref = _conv64(planes, F, H, W, Cin, up.conv.weight, up.conv.bias)
    err = {k: (o.f32.double().cpu() - ref).abs().max().item() for k, o in out.items()}
    print(f"upsample {shape} {prec} f16={want_f16}: max-abs err vs float64 old {err['old']:.3e} new {err['new']:.3e}")
    measured("upsample_source_res " + "x".join(map(str, shape)), prec=prec, f16=int(want_f16), old=err["old"], new=err["new"])
    new = out["new"]
    assert (new.F, new.H, new.W, new.C) == (F, 2 * H, 2 * W, Cout) and new.f32.shape == out["old"].f32.shape
    assert torch.isfinite(new.f32).all()
    assert err["new"] <= 2.0 * err["old"], err
    if want_f16:
        assert (new.f16.lo is None) == (out["old"].f16.lo is None)
        assert torch.equal(new.f16.hi, new.f32.half())
        if new.f16.lo is not None:
            assert new.f16.lo.dtype == out["old"].f16.lo.dtype
            assert torch.equal(new.f16.lo, _lo_planes_of(new.f32, new.f16.lo.dtype)[1])
    else:
        assert new.f16 is None


# ---------------------------------------------------------------------------------------------- pnc_upsample_combine alone
def _emulate(P, ldp, bias, F, Hin, Win, Cout):
    """the formula of include/panacea_hip.h in fp32, the additions in its order (CPU)"""
    Pv = P.view(F, Hin, Win, ldp)
    out = bias.view(1, 1, 1, Cout).expand(F, 2 * Hin, 2 * Win, Cout).clone()
    ys, xs = torch.arange(2 * Hin), torch.arange(2 * Win)
    for u in range(3):
        for v in range(3):
            yy, xx = ys + u - 1, xs + v - 1
            ok = ((yy >= 0) & (yy < 2 * Hin))[:, None] & ((xx >= 0) & (xx < 2 * Win))[None, :]
            sy, sx = (yy.clamp(0, 2 * Hin - 1) >> 1), (xx.clamp(0, 2 * Win - 1) >> 1)
            term = Pv[:, sy][:, :, sx][..., (u * 3 + v) * Cout:(u * 3 + v + 1) * Cout]
            out = torch.where(ok[None, :, :, None], out + term, out)
    return out.reshape(-1, Cout)


def _bits(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _poisoned(n, dtype, margin=64):
    """a view of n elements inside an allocation whose every byte is the poison (NaN for floats); margin elements keep it 16-byte aligned"""
    poison = 0x7F if dtype == torch.uint8 else float("nan")                              # (0x7F: the e4m3 NaN)
    whole = torch.full((n + 2 * margin,), poison, device=DEV, dtype=dtype)
    return whole, whole[margin:margin + n]


KERNEL_SHAPES = [(1, 1, 1, 64, 0), (2, 2, 3, 64, 4), (2, 3, 8, 64, 0), (1, 4, 6, 320, 8), (3, 2, 4, 64, 0), (1, 3, 5, 12, 4),
                 (2, 5, 9, 132, 0)]       # (F, Hin, Win, Cout, ldp - 9 Cout)


@pytest.mark.parametrize("lo", [None, torch.uint8, torch.float16], ids=["f32", "e4m3", "f16lo"])
@pytest.mark.parametrize("shape", KERNEL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_combine_kernel_bits_in_poisoned_allocations(shape, lo):
    F, Hin, Win, Cout, pad = shape
    ldp, rows, nout = 9 * Cout + pad, F * Hin * Win, 4 * F * Hin * Win * Cout
    g = torch.Generator().manual_seed(31 * Cout + rows)
    Pc = torch.full((rows, ldp), float("nan"))
    Pc[:, :9 * Cout] = torch.randn(rows, 9 * Cout, generator=g)          # the slack columns of every row stay poisoned
    bias = torch.randn(Cout, generator=g)
    Pw, P = _poisoned(rows * ldp, torch.float32)
    P.copy_(Pc.view(-1))
    o32w, o32 = _poisoned(nout, torch.float32)
    o16w, o16 = _poisoned(nout, torch.float16) if lo is not None else (None, None)
    olw, ol = _poisoned(nout, lo) if lo is not None else (None, None)
    before = {k: _bits(w).clone() for k, w in (("o32", o32w), ("o16", o16w), ("lo", olw), ("P", Pw)) if w is not None}
    hip.upsample_combine(P, ldp, bias.to(DEV), F, Hin, Win, Cout, o32, o16, ol)
    torch.cuda.synchronize()
    want = _emulate(Pc, ldp, bias, F, Hin, Win, Cout)
    assert torch.isfinite(want).all()
    assert torch.equal(_bits(o32.cpu()), _bits(want.view(-1))), "out32 is not the emulation's bits"
    m = 64
    for k, w in (("o32", o32w), ("o16", o16w), ("lo", olw)):
        if w is not None:
            now = _bits(w)
            assert torch.equal(now[:m], before[k][:m]) and torch.equal(now[-m:], before[k][-m:]), f"{k}: a margin changed"
    assert torch.equal(_bits(Pw), before["P"])
    if lo is not None:
        hi_want, lo_want = _lo_planes_of(o32, lo)
        assert torch.equal(_bits(o16), _bits(hi_want)) and torch.equal(_bits(ol), _bits(lo_want))


def test_combine_counts_clamped_lo_quads_for_the_range_monitor():
    """values beyond the e4m3 lo plane's range: the monitor counts exactly the quads whose residual leaves +-448"""
    F, Hin, Win, Cout = 1, 3, 4, 64
    g = torch.Generator().manual_seed(5)
    P = (torch.randn(F * Hin * Win, 9 * Cout, generator=g) * 700.0).to(DEV)
    nout = 4 * F * Hin * Win * Cout
    o32, o16 = torch.empty(nout, device=DEV), torch.empty(nout, device=DEV, dtype=torch.float16)
    ol = torch.empty(nout, device=DEV, dtype=torch.uint8)
    count = torch.zeros(2, dtype=torch.int32, device=DEV)
    hip.range_monitor_collect(count[:1])
    hip.upsample_combine(P, 9 * Cout, None, F, Hin, Win, Cout, o32, o16, ol)
    hip.range_monitor_collect(count[1:])
    torch.cuda.synchronize()
    r = ((o32 - o32.half().float()) * 2048.0).view(-1, 4).abs().max(dim=1).values
    clamped = int((r > 448.0).sum())
    assert clamped > 0 and int(count[1]) == clamped
    assert torch.equal(ol, _lo_planes_of(o32, torch.uint8)[1])


def test_combine_refuses_before_any_launch():
    F, Hin, Win, Cout = 1, 2, 2, 8
    P = torch.zeros(F * Hin * Win * 9 * Cout + 8, device=DEV)
    out = torch.full((4 * F * Hin * Win * Cout + 8,), float("nan"), device=DEV)
    o16 = torch.zeros(4 * F * Hin * Win * Cout + 8, device=DEV, dtype=torch.float16)
    bias = torch.zeros(Cout + 4, device=DEV)
    with pytest.raises(hip.PncError, match="PNC_EALIGN"):
        hip.upsample_combine(P[1:], 9 * Cout, bias, F, Hin, Win, Cout, out)                 # misaligned P
    with pytest.raises(hip.PncError, match="PNC_EALIGN"):
        hip.upsample_combine(P, 9 * Cout, bias, F, Hin, Win, Cout, out[1:])                 # misaligned out32
    with pytest.raises(hip.PncError, match="PNC_EALIGN"):
        hip.upsample_combine(P, 9 * Cout, bias, F, Hin, Win, Cout, out, o16[4:])            # out16 on 8 bytes only
    with pytest.raises(hip.PncError, match="PNC_EALIGN"):
        hip.upsample_combine(P, 9 * Cout, bias[1:], F, Hin, Win, Cout, out)                 # misaligned bias
    with pytest.raises(hip.PncError, match="PNC_EINVAL"):
        hip.upsample_combine(P, 9 * 6, bias, F, Hin, Win, 6, out)                           # Cout % 4
    with pytest.raises(hip.PncError, match="PNC_EINVAL"):
        hip.upsample_combine(P, 9 * Cout + 2, bias, F, 1, 1, Cout, out)                     # ldp % 4
    with pytest.raises(hip.PncError, match="PNC_EINVAL"):
        hip.upsample_combine(P, 8 * Cout, bias, F, 1, 1, Cout, out)                         # ldp < 9 Cout
    torch.cuda.synchronize()
    assert torch.isnan(out).all()
