"""Upsample at source resolution, host side (CPU): the packed tap weight, the gate of the new path and the chunk rule.  The emulated
C-ABI has no `upsample_combine`, so on it Upsample._run is the output-resolution conv of the parent, bit for bit."""
import pytest
import torch

import emu
from panacea_amd import engine as E
from panacea_amd import hip
from panacea_amd.nn import openaimodel as om


def _upsample(Cin, Cout, seed=0):
    torch.manual_seed(seed)
    up = om.Upsample(Cin, True, dims=2, out_channels=Cout)
    with torch.no_grad():
        up.conv.weight.normal_(0.0, (9 * Cin) ** -0.5)
        up.conv.bias.normal_(0.0, 0.1)
    return up


@pytest.mark.parametrize("lo", [False, True])
def test_w9_is_the_permuted_conv_weight(lo):
    Cin, Cout = 64, 24
    up = _upsample(Cin, Cout)
    w9 = E.pk_conv3x3_taps(up.conv.weight, lo)
    assert w9.shape == (9 * Cout, Cin) and w9.dtype == torch.float16 and w9.is_contiguous()
    plane = E._cast16(up.conv.weight, lo)                  # what pk_linear stores of every element
    for u in range(3):
        for v in range(3):
            assert torch.equal(w9[(u * 3 + v) * Cout:(u * 3 + v + 1) * Cout], plane[:, :, u, v])
    pk = up._pack(lo)
    assert torch.equal(pk["w9"], w9) and torch.equal(pk["w"], E.pk_conv3x3(up.conv.weight, lo=lo))
    if not lo:
        assert torch.equal(up.packed()["w9"], w9) and torch.equal(up.packed_lo()["w9"], E.pk_conv3x3_taps(up.conv.weight, True))


@pytest.mark.parametrize("prec", ["precise", "fast"])
@pytest.mark.parametrize("want_f16", [False, True])
def test_emulated_backend_takes_the_output_resolution_conv(prec, want_f16):
    assert not hasattr(emu, "upsample_combine") and E.UPSAMPLE_SOURCE_RES
    F, H, W, Cin, Cout = 2, 3, 4, 64, 64
    up = _upsample(Cin, Cout, seed=1)
    x32 = torch.randn(F * H * W, Cin) * 1.5
    with E.use_backend(emu), torch.no_grad():
        rt = E.Runtime(torch.device("cpu"), 1, F)
        rt.prec = E.precision(prec)
        act = E.Act(F, H, W, Cin, f32=x32)
        got = up._run(rt, act, want_f16=want_f16)
        pk = up.packed()
        ref = om.run_conv3x3(rt, act.need_f16(rt), F, H, W, Cin, pk, "w", Cout, pk["b"], upsample=True, out16=want_f16,
                             split_out="stream")                      # the parent's Upsample._run
    assert (got.F, got.H, got.W, got.C) == (F, 2 * H, 2 * W, Cout)
    assert torch.equal(got.f32, ref.f32)
    if want_f16:
        assert torch.equal(got.f16.hi, ref.f16.hi)
        assert (got.f16.lo is None) == (ref.f16.lo is None) and (got.f16.lo is None or torch.equal(got.f16.lo, ref.f16.lo))
    else:
        assert got.f16 is None


def test_binding_and_switches():
    assert "pnc_upsample_combine" in hip.header_symbols() and len(hip._SIGNATURES["pnc_upsample_combine"][1]) == 12
    assert hasattr(hip, "upsample_combine") and hip.ABI_VERSION == 8           # additive: the ABI version did not move
    for F in (1, 2, 3, 16):
        for shape in ((32, 96, 640), (16, 48, 1280), (8, 24, 1280), (1, 1, 64)):
            fc = E.upsample_chunk_frames(F, *shape)
            assert 1 <= fc <= F and fc == E.upsample_chunk_frames(F, *shape)      # a function of the shapes alone


class _Recorder:
    """a backend that HAS the combine entry: records the launches of the new path"""

    def __init__(self):
        self.calls = []

    def gemm(self, a, w, **kw):
        self.calls.append(("gemm", a, w, kw))

    def upsample_combine(self, *a):
        self.calls.append(("combine",) + a)

    def cast_f16(self, x32, n, y16, y16_lo=None):
        emu.cast_f16(x32, n, y16, y16_lo)


@pytest.mark.parametrize("chunk,rounds", [(0, None), (2, [(0, 2), (2, 1)])])
def test_new_path_launches_gemm_and_combine_per_chunk(chunk, rounds, monkeypatch):
    F, H, W, Cin, Cout = 3, 2, 4, 64, 64
    N = H * W
    up = _upsample(Cin, Cout, seed=2)
    be = _Recorder()
    monkeypatch.setattr(E, "UPSAMPLE_CHUNK_FRAMES", chunk)
    with E.use_backend(be), torch.no_grad():
        rt = E.Runtime(torch.device("cpu"), 1, F)
        rt.prec = E.PRECISE
        act = E.Act(F, H, W, Cin, f32=torch.randn(F * N, Cin))
        x16 = act.need_f16(rt)
        out = up._run(rt, act, want_f16=True)
    rounds = rounds or [(f0, min(E.upsample_chunk_frames(F, H, W, Cout), F - f0))
                        for f0 in range(0, F, E.upsample_chunk_frames(F, H, W, Cout))]
    assert [c[0] for c in be.calls] == ["gemm", "combine"] * len(rounds)
    pk = up.packed()
    for r, (f0, nf) in enumerate(rounds):
        _, a, w, kw = be.calls[2 * r]
        assert w is pk["w9"] and kw["M"] == nf * N and kw["N"] == 9 * Cout and kw["K"] == Cin and kw["lda"] == Cin
        assert kw.get("bias") is None and kw["ldc32"] == 9 * Cout and kw["w_lo"] is pk[("w9", "lo8")]
        assert a.data_ptr() == x16.hi[f0 * N:].data_ptr() and kw["a16_lo"].data_ptr() == x16.lo[f0 * N:].data_ptr()
        _, P, ldp, bias, nfr, h, wd, co, o32, o16, olo = be.calls[2 * r + 1]
        assert P is kw["out32"] and ldp == 9 * Cout and bias is pk["b"] and (nfr, h, wd, co) == (nf, H, W, Cout)
        assert o32.data_ptr() == out.f32[4 * f0 * N:].data_ptr() and o16.data_ptr() == out.f16.hi[4 * f0 * N:].data_ptr()
        assert olo.data_ptr() == out.f16.lo[4 * f0 * N:].data_ptr()
    assert out.f32.shape == (4 * F * N, Cout) and (out.H, out.W) == (2 * H, 2 * W)
    # a view shard, an odd channel count or the switch send the call to the output-resolution conv
    be.calls.clear()
    monkeypatch.setattr(E, "UPSAMPLE_SOURCE_RES", False)
    with E.use_backend(be), torch.no_grad():
        up._run(rt, act, want_f16=False)
    assert [c[0] for c in be.calls] == ["gemm"] and be.calls[0][3]["a_mode"] == hip.A_CONV3X3
