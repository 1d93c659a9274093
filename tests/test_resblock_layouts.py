"""ResBlock3D's temporal sites in the three frame layouts (resident, FrameShard "halo", FrameShard "transpose"): the order of the
backend launches AND of the exchanges of one block — what tools/launch_trace.py, which records launches only, cannot see."""
import types

import pytest
import torch

import emu
from helpers import gn_statistics_from_launches, product_network
from panacea_amd import engine as E, shard
from panacea_amd.nn.openaimodel import ResBlock3D

B, T, H, W = 2, 2, 4, 48


class NamesOver(types.ModuleType):
    """tests/emu.py as a backend; every wrapper call appends its name to `events`"""

    def __init__(self, events):
        super().__init__("resblock_layouts_backend")
        self.events = events

    def __getattr__(self, name):
        fn = getattr(emu, name)
        if not callable(fn) or isinstance(fn, type):
            return fn

        def call(*a, **k):
            self.events.append(name)
            return fn(*a, **k)
        return call


class LoggedFrameShard(E.FrameShard):
    """the loop-back frame shard; its exchanges append their names to `events`"""

    def __init__(self, events, resblock):
        super().__init__(1, 0, None, resblock=resblock)
        self.events = events


for _name in ("to_pixels_start", "to_frames", "allreduce_sum", "halo_frames"):
    def _logged(self, *a, _name=_name, **k):
        self.events.append(_name)
        return getattr(E.FrameShard, _name)(self, *a, **k)
    setattr(LoggedFrameShard, _name, _logged)


GN_IN = ["groupnorm_stats", "groupnorm_apply"]                     # a spatial GroupNorm without records of its input
TO_PIXELS, TO_FRAMES = ["to_pixels_start", "result"], ["to_frames", "result"]
GNT_HALO = ["groupnorm_temporal_part", "allreduce_sum", "groupnorm_temporal_part", "halo_frames", "result"]
EXPECTED = {
    None: GN_IN + ["gemm", "linear_smallm", "groupnorm_temporal_silu", "gemm", "groupnorm_apply", "gemm", "cast_f16", "gemm",
                   "groupnorm_temporal_silu", "gemm"],
    "halo": GN_IN + ["gemm", "linear_smallm"] + GNT_HALO + ["gemm", "groupnorm_apply", "gemm", "cast_f16", "gemm"] + GNT_HALO + ["gemm"],
    "transpose": GN_IN + ["gemm", "to_pixels_start", "linear_smallm", "cast_f16", "gemm", "result", "groupnorm_temporal_silu", "gemm"]
    + TO_FRAMES + GN_IN + ["gemm"] + TO_PIXELS + ["groupnorm_temporal_silu", "gemm"] + TO_FRAMES + ["add_f32"],
}


def run_block(layout, monkeypatch):
    events = []
    result = shard.Pending.result
    w, _, _ = product_network("tiny")
    blk = next(m for m in w.diffusion_model.modules() if isinstance(m, ResBlock3D) and m.channels != m.out_channels)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B * T * H * W, blk.channels, generator=g)
    emb = torch.nn.functional.silu(torch.randn(B * T, blk.emb_channels, generator=g))
    with E.use_backend(NamesOver(events)), torch.no_grad(), monkeypatch.context() as mp:
        mp.setattr(shard.Pending, "result", lambda self: (events.append("result"), result(self))[1])
        rt = E.Runtime(x.device, B, T, None if layout is None else LoggedFrameShard(events, layout))
        rt.prec = E.precision("precise")
        rt.emb_all = emb            # G = 1: the rows of all frames are this rank's (UNetModel3D._time_embedding gathers them)
        out = blk._run(rt, E.Act(B * T, H, W, blk.channels, f32=x), emb, want_f16=True, want_stats=True)
    return events, out


@pytest.mark.parametrize("layout", [None, "halo", "transpose"])
def test_launch_and_exchange_order(layout, monkeypatch):
    """The merged sequence of backend wrapper names and FrameShard exchange events of one block with a skip 1x1 conv, under `precise`
    with the fp16 output and the output's GroupNorm records asked for.  The literal lists in EXPECTED were produced by running this
    body on the commit before ResBlock3D._run got its one temporal-site function; "result" is shard.Pending.result (to_pixels is
    to_pixels_start + result; to_frames and halo_frames wait for their own exchange)."""
    events, out = run_block(layout, monkeypatch)
    assert events == EXPECTED[layout]
    assert out.f16 is not None and out.f16.hi.shape == out.f32.shape
    assert (out.gn_part is None) == (layout == "transpose")        # records come out of a frame-layout epilogue only
    if layout == "transpose":
        # what does not depend on the stream in flight is enqueued under its transfer: the emb_layers linear and the skip 1x1 GEMM
        start = events.index("to_pixels_start")
        under = events[start + 1:events.index("result", start)]
        assert under == ["linear_smallm", "cast_f16", "gemm"]


def test_transpose_only_moves_data(monkeypatch):
    """the transposed layout computes the resident block's bits when every GroupNorm launches its own statistics
    (test_engine_emu.py's claim for the network, here for one block)"""
    with gn_statistics_from_launches():
        _, ref = run_block(None, monkeypatch)
        _, got = run_block("transpose", monkeypatch)
    assert torch.equal(got.f32, ref.f32)
    assert all(torch.equal(a, b) for a, b in zip(got.f16.planes(), ref.f16.planes()))
