"""The first stage's operand policies (`precision=` of nn.model.FirstStageDecoder / FirstStageEncoder) on the emulated backend:
tests/emu.py plus `attn_frame_split` evaluated in float64 from the header's formulae (tests/emu_first_stage.py).

Fixture and bound: tests/first_stage_w32.py — unrounded fp32 weights, truth = the float64 oracle, bound 16 e32 per output with e32 the
reference's own fp32 distance from truth.  Measured on the emulation: `precise-full` 2.4 e32 (decode) / 2.3 e32 (moments);
`precise-wide` 1.1e3 / 8.7e2 e32 (the weights' fp16 rounding); `fast` 1.7e3 / 1.3e3 e32.

The same fixture goes through the library in tests/test_first_stage_precision_gpu.py."""
import pytest
import torch

import emu
import emu_first_stage as efs
import first_stage_w32 as fx
from panacea_amd import engine as E
from panacea_amd.nn import model


def _run(kind, net, be=None):
    f = fx.fixture()
    with E.use_backend(be or efs.Backend()):
        return net.decode(f["z"]) if kind == "dec" else net.moments(f["x"])


TRUTH = dict(dec=("img_truth", "e32_img"), enc=("moments_truth", "e32_moments"))


@pytest.mark.parametrize("kind", ["dec", "enc"])
def test_precise_full_within_16_e32_of_truth_fast_and_wide_outside(kind):
    f = fx.fixture()
    truth, e32 = f[TRUTH[kind][0]], f[TRUTH[kind][1]]
    bound = fx.FACTOR * e32
    errs = {p: fx.err(_run(kind, fx.stage(kind, p)), truth) for p in model.FIRST_STAGE_PRECISIONS}
    print(kind, "e32", e32, {p: f"{e:.3e} = {e / e32:.1f} e32" for p, e in errs.items()})
    assert errs["precise-full"] <= bound, errs
    # more than half of the bound on the emulation would mean an operand still travels single-plane
    assert errs["precise-full"] <= 0.5 * bound, errs
    assert errs["fast"] >= 10.0 * bound, errs
    assert errs["precise-wide"] > bound, errs                    # the weight planes are in use: without them the weights' rounding stays


@pytest.mark.parametrize("kind", ["dec", "enc"])
def test_fast_and_the_omitted_keyword_give_the_same_bits(kind):
    a, b = _run(kind, fx.stage(kind)), _run(kind, fx.stage(kind, "fast"))
    c = _run(kind, fx.stage(kind, E.FAST), be=emu)               # and on the plain emulation: no capability is asked for
    assert torch.equal(a, b) and torch.equal(a, c)
    assert fx.stage(kind).precision is E.FAST


@pytest.mark.parametrize("kind", ["dec", "enc"])
def test_wide_and_full_differ_on_unrounded_weights_and_agree_on_fp16_ones(kind):
    wide, full = (_run(kind, fx.stage(kind, p)) for p in ("precise-wide", "precise-full"))
    assert not torch.equal(wide, full)
    wide, full = (_run(kind, fx.stage(kind, p, rounded=True)) for p in (E.PRECISE_WIDE, E.PRECISE_FULL))
    assert torch.equal(wide, full)                               # all-zero lo twins add exact zeros


def test_refusals():
    for cls in (model.FirstStageDecoder, model.FirstStageEncoder):
        for bad in ("precise", "precise-ckpt", "precise-all", "precise-f16lo", "nonsense", E.PRECISE, E.PRECISE_CKPT, None, 3):
            with pytest.raises(ValueError) as e:
                cls(4, fx.TINY, precision=bad)
            msg = str(e.value)
            assert all(n in msg for n in model.FIRST_STAGE_PRECISIONS) and "e4m3" in msg, msg
        with pytest.raises(TypeError):
            cls(4, fx.TINY, "precise-full")                      # keyword-only
    f = fx.fixture()
    # a backend without the capability: refused before anything is launched
    class Counting:
        calls = 0

        def __getattr__(self, name):
            fn = getattr(emu, name)
            if not callable(fn):
                return fn

            def wrapped(*a, **kw):
                Counting.calls += 1
                return fn(*a, **kw)
            return wrapped

    for kind, arg in (("dec", f["z"]), ("enc", f["x"])):
        net = fx.stage(kind, "precise-wide")
        net.packed()
        with E.use_backend(Counting()):
            with pytest.raises(NotImplementedError, match="attn_frame_split"):
                net.decode(arg) if kind == "dec" else net.moments(arg)
        assert Counting.calls == 0
    assert not hasattr(emu, "attn_frame_split") and not hasattr(efs.Backend(with_split=False), "attn_frame_split")
    # a width the kernel is not built for
    blk = model.AttnBlock(192)
    model.set_precision(blk, "precise-full")
    with E.use_backend(efs.Backend()):
        with pytest.raises(NotImplementedError, match="192 channels"):
            blk(torch.zeros(1, 192, 4, 8))


def test_one_split_launch_serves_all_frames_and_no_three_launch_form():
    be = efs.Backend()
    softmax = []
    be.softmax_rows = lambda *a, **kw: softmax.append(1) or emu.softmax_rows(*a, **kw)
    _run("dec", fx.stage("dec", "precise-full"), be)
    assert be.split_calls == [dict(F=2, N=8 * 48, C=128, scale=128.0 ** -0.5, lds=(128, 128, 128, 128))] and softmax == []
    _run("dec", fx.stage("dec", "fast"), be)
    assert len(be.split_calls) == 1 and len(softmax) == 2         # `fast` keeps its three launches per frame


def test_invalidation_repacks_the_lo_twins():
    net = fx.stage("dec", "precise-full")
    a = _run("dec", net)
    blk = net.decoder.mid.block_1
    twin = blk.packed_lo()["c1"][0]
    assert twin.dtype == torch.float16 and bool(twin.ne(0).any()) and blk.packed_lo()["n1"] == (None, None)
    pq = net.packed_lo()["w"]                                    # the hand-packed post_quant_conv weight has its twin, padded alike
    w = net.post_quant_conv.weight.detach().reshape(4, 4)
    assert pq.shape == net.packed()["w"].shape == (8, 8) and torch.equal(pq[:4, :4], E.split_lo(w, w.half())) and not pq[4:].any()
    with torch.no_grad():
        blk.conv1.weight.mul_(1.0 + 2.0 ** -13)                  # moves (almost) only the lo plane
    assert torch.equal(_run("dec", net), a)                      # the packed copies are still the old ones
    blk.invalidate_packed()
    assert blk._pk is None and blk._pk_lo is None
    b = _run("dec", net)
    assert not torch.equal(a, b) and not torch.equal(blk.packed_lo()["c1"][0], twin)


def test_posterior_draw_is_that_of_fast():
    f = fx.fixture()
    draws = {}
    for p in ("fast", "precise-full"):
        with E.use_backend(efs.Backend()):
            net = fx.stage("enc", p)
            mom = net.moments(f["x"])
            z = net.encode(f["x"], generator=torch.Generator().manual_seed(5))
        mean, logvar = torch.chunk(mom, 2, dim=1)
        draws[p] = (z - mean) / torch.exp(0.5 * logvar.clamp(-30.0, 20.0))
    assert (draws["fast"] - draws["precise-full"]).abs().max().item() < 1e-4      # the same randn; only the moments differ
