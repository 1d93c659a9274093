"""The first stage's operand policies on the MI355X: the fixture and the bound of tests/first_stage_w32.py (unrounded fp32 weights,
truth = the float64 oracle, 16 e32 per output) through the library — pnc_attn_frame_split_f16 in the mid block, split operands and
split weights in every GEMM — plus the uint8 entries and a two-window rollout on top of split first stages."""
from pathlib import Path

import numpy as np
import pytest
import torch

import first_stage_w32 as fx
import image_boundary_cases as ib
import rollout_cases as rc
from helpers import measured
from panacea_amd import hip, pipeline
from panacea_amd.image import SparseClip
from panacea_amd.nn import model

pytestmark = pytest.mark.gpu
DEV = "cuda"
TRUTH = dict(dec=("img_truth", "e32_img"), enc=("moments_truth", "e32_moments"))


class _count_split:
    def __enter__(self):
        self.calls, self.real = [], hip.attn_frame_split
        hip.attn_frame_split = lambda *a, **kw: (self.calls.append((kw["F"], kw["N"], kw["C"])), self.real(*a, **kw))[1]
        return self.calls

    def __exit__(self, *exc):
        hip.attn_frame_split = self.real


def _run(kind, precision):
    f = fx.fixture()
    net = fx.stage(kind, precision, device=DEV)
    out = net.decode(f["z"].to(DEV)) if kind == "dec" else net.moments(f["x"].to(DEV))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("kind", ["dec", "enc"])
def test_decode_and_moments_against_truth(kind):
    f = fx.fixture()
    truth, e32 = f[TRUTH[kind][0]], f[TRUTH[kind][1]]
    bound = fx.FACTOR * e32
    with _count_split() as calls:
        errs = {p: fx.err(_run(kind, p), truth) for p in model.FIRST_STAGE_PRECISIONS}
    print(f"first stage {kind}: e32 {e32:.3e}, bound {bound:.3e};", {p: f"{e:.3e} = {e / e32:.1f} e32" for p, e in errs.items()})
    measured(f"first_stage_precision {kind}", e32=e32, **{p.replace("-", "_"): e for p, e in errs.items()})
    assert calls == [(2, 8 * 48, 128)] * 2                       # one split launch per split policy, none under `fast`
    assert "libpanacea_hip.so" in Path("/proc/self/maps").read_text()
    assert errs["precise-full"] <= bound, errs
    assert errs["fast"] >= 10.0 * bound, errs
    assert errs["precise-wide"] > bound, errs                    # the weight planes are in use
    assert torch.equal(_run(kind, "precise-full"), _run(kind, "precise-full"))


def test_uint8_entries_under_precise_full_have_the_bits_of_the_float_image():
    """moments_u8 / encode_u8 / moments_sparse_u8 (all slots given: the same rows, the same launches) against `moments` of the float
    image the table stands for — bit-equal, as tests/test_image_boundary_gpu.py asserts for `fast`; with blank slots the run has other
    row counts, so the given frame is held to twice the bound (both runs are within 16 e32 of the exact moments) and the blank slots
    to each other"""
    enc = fx.stage("enc", "precise-full", device=DEV)
    u8 = torch.from_numpy(np.random.default_rng(3).integers(0, 256, (2, 16, 96, 3), dtype=np.uint8))
    x = torch.from_numpy(ib.scaled_nchw(u8.numpy(), "image")).to(DEV)
    want = enc.moments(x)
    assert torch.equal(enc.moments_u8(u8.to(DEV)), want)
    assert torch.equal(enc.moments_sparse_u8(SparseClip(u8.to(DEV), [0, 1], 2)), want)
    assert torch.equal(enc.encode_u8(u8.to(DEV), sample=False), want[:, :4])
    g1, g2 = (torch.Generator(device=DEV).manual_seed(9) for _ in range(2))
    assert torch.equal(enc.encode_u8(u8.to(DEV), generator=g1), enc.encode(x, generator=g2))
    sparse = enc.moments_sparse_u8(SparseClip(u8[:1].to(DEV), [1], 3))
    assert sparse.shape == (3, 8, 8, 48) and torch.isfinite(sparse).all() and torch.equal(sparse[0], sparse[2])
    d = (sparse[1] - want[0]).abs().max().item()
    print(f"sparse (1 of 3 frames) vs dense moments, given frame: max-abs {d:.3e}")
    assert d <= 2.0 * fx.FACTOR * fx.fixture()["e32_moments"], d
    zero = enc.moments(torch.zeros(1, 3, 16, 96, device=DEV))
    assert (sparse[0] - zero[0]).abs().max().item() <= 2.0 * fx.FACTOR * fx.fixture()["e32_moments"]


def test_decode_u8_bytes_against_the_quantised_truth():
    f = fx.fixture()
    tol = 127.5 * fx.FACTOR * f["e32_img"]
    want, near = fx.expected_bytes(f["img_truth"], tol)          # near: truth within the bound of a truncation step
    frac = near.double().mean().item()
    assert frac < 0.01, frac                                     # from truth alone
    got = fx.stage("dec", "precise-full", device=DEV).decode_u8(f["z"].to(DEV)).cpu()
    assert got.shape == want.shape and got.dtype == torch.uint8
    diff = got != want
    print(f"decode_u8 under precise-full: {int(diff.sum())} of {diff.numel()} bytes differ; {int(near.sum())} lie within {tol:.2e} of a step")
    measured("first_stage_precision decode_u8", differ=int(diff.sum()), near=int(near.sum()), total=diff.numel())
    assert not bool((diff & ~near).any())
    assert int((got.to(torch.int16) - want.to(torch.int16)).abs().max()) <= 1


def test_two_window_rollout_on_split_first_stages():
    pipe = rc.tiny_rollout_pipeline(DEV)
    inp = rc.rollout_inputs(2, "last", "uint8", DEV)
    outs = {}
    for p in ("fast", "precise-full"):
        dec, enc = model.FirstStageDecoder(4, rc.tv.TINY, precision=p), model.FirstStageEncoder(4, rc.tv.TINY, precision=p)
        dec.load_state_dict(pipe["dec"].state_dict(), strict=True)
        enc.load_state_dict(pipe["enc"].state_dict(), strict=True)
        with _count_split() as calls:
            outs[p] = pipeline.rollout_frames(pipe["net"], dec.to(DEV), enc.to(DEV), inp["anchor"], inp["windows"], inp["noise"],
                                              anchor="last", sample_posterior=False, num_steps=2)
            torch.cuda.synchronize()
        assert bool(calls) == (p != "fast")
    a, b = outs["fast"], outs["precise-full"]
    assert a.shape == b.shape == (rc.T + (rc.T - 1), rc.H, rc.W, 3) and b.dtype == torch.uint8
    assert len({int(fr.float().mean().item() * 1000) for fr in b}) > 1           # frames, not one constant
