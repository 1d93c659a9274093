"""Videos past one clip on the MI355X: the sparse first-stage encode and pipeline.rollout_frames on the HIP kernels, at the tiny
shapes of tests/test_rollout.py (T = 3 frames of 16 x 192 pixels, latents 8 x 96) and against the same golden file
(tests/golden/rollout_tiny.npz) under the same bounds — the first-stage encoder's of tests/test_vae.py and the sampler trajectory's of
tests/test_sampler_acceptance.py (rollout_cases.ENC_MAX / ENC_MEAN / Z_TOL)."""
from pathlib import Path

import pytest
import torch

import rollout_cases as rc
from helpers import measured
from panacea_amd import pipeline, sampling
from panacea_amd.image import SparseClip

pytestmark = pytest.mark.gpu
DEV = "cuda"
T = rc.T


@pytest.fixture(scope="module")
def pipe():
    return rc.tiny_rollout_pipeline(DEV)


@pytest.mark.parametrize("tag", ["last", "first"])
@pytest.mark.parametrize("k", [0, 1])
def test_sparse_moments_and_concat_against_the_reference(pipe, tag, k):
    rc.check_moments_and_concat(pipe["enc"], DEV, tag, k, "gpu")
    assert "libpanacea_hip.so" in Path("/proc/self/maps").read_text()


def test_sparse_against_dense_moments_u8_of_the_same_frames(pipe):
    """K = 1, T = 3: the sparse run has M = 2 frames of rows, the dense one 3, so tile and split-K choices may differ and equality
    is not required; the difference has to sit inside the bound both runs are held to against the reference"""
    enc = pipe["enc"]
    u8 = rc.frames_u8(1, seed=12).to(DEV)
    for slot in (0, 1, T - 1):
        dense = torch.zeros((T,) + tuple(u8.shape[1:]), dtype=torch.uint8, device=DEV)
        dense[slot] = u8[0]
        got = enc.moments_sparse_u8(SparseClip(u8, [slot], T))
        # (no byte is the blank frame: the dense uint8 clip serves the given frame's slot; the blank slots against the float clip)
        want_u8 = enc.moments_u8(dense)
        want_f = enc.moments(rc.dense_clip(u8, [slot]))
        d_given = (got[slot] - want_u8[slot]).abs().max().item()
        d_all = (got - want_f).abs()
        print(f"sparse vs dense, slot {slot}: given frame vs moments_u8 max-abs {d_given:.3e}; whole clip vs float moments max-abs "
              f"{d_all.max().item():.3e} mean-abs {d_all.mean().item():.3e}")
        measured(f"rollout_sparse_vs_dense_slot{slot}", given_max=d_given, all_max=d_all.max().item(), all_mean=d_all.mean().item())
        assert got.shape == want_f.shape and torch.isfinite(got).all()
        assert d_given < rc.ENC_MAX and d_all.max().item() < rc.ENC_MAX and d_all.mean().item() < rc.ENC_MEAN
        blank = [s for s in range(T) if s != slot]
        assert torch.equal(got[blank[0]], got[blank[1]])                  # one blank frame, repeated


@pytest.mark.parametrize("anchor,hint", [("last", "uint8"), ("first", "float")])
def test_rollout_is_the_manual_composition_and_hands_the_far_frame_over(pipe, anchor, hint):
    Wn = 3
    inp = rc.rollout_inputs(Wn, anchor, hint, DEV)
    rec = rc.Recorder(pipe["dec"], pipe["enc"])
    out = pipeline.rollout_frames(pipe["net"], rec, rec, inp["anchor"], inp["windows"], inp["noise"], anchor=anchor,
                                  sample_posterior=False, num_steps=2)
    N = T + (Wn - 1) * (T - 1)
    assert out.shape == (N, rc.H, rc.W, 3) and out.dtype == torch.uint8 and out.device.type == "cuda"
    # by hand: sample_frames(output="uint8") on the concat of encode_sparse_u8, window by window
    slot, far = (T - 1, 0) if anchor == "last" else (0, T - 1)
    frame, wins = inp["anchor"], []
    for k, (c, uc) in enumerate(inp["windows"]):
        clip = SparseClip(frame[None], [slot], T)
        cc = pipeline.SCALE_FACTOR * pipe["enc"].encode_sparse_u8(clip, sample=False)
        ucc = pipeline.SCALE_FACTOR * pipe["enc"].encode_sparse_u8(clip, sample=False)
        wins.append(pipeline.sample_frames(pipe["net"], pipe["dec"], dict(c, concat=cc), dict(uc, concat=ucc),
                                           sampling.share_noise_init(inp["noise"][k], cc, 0.07), num_steps=2, output="uint8"))
        frame = wins[-1][far]
    video = torch.cat([w[:-1] for w in wins[:0:-1]] + [wins[0]]) if anchor == "last" else torch.cat([wins[0]] + [w[1:] for w in wins[1:]])
    torch.cuda.synchronize()
    assert torch.equal(out, video)
    # the junctions: window k + 1 is anchored on window k's far-end frame, which is in the video where the two meet
    assert len(rec.clips) == 2 * Wn and torch.equal(rec.clips[0].frames_u8[0], inp["anchor"])
    for k in range(Wn - 1):
        junction = rec.decoded[k][far]
        assert torch.equal(rec.clips[2 * k + 2].frames_u8[0], junction) and torch.equal(rec.clips[2 * k + 3].frames_u8[0], junction)
        assert torch.equal(out[(Wn - 1 - k) * (T - 1) if anchor == "last" else (k + 1) * (T - 1)], junction)
    assert len({int(f.float().mean().item() * 1000) for f in out}) > 1                   # frames, not one constant


@pytest.mark.parametrize("tag", ["last", "first"])
def test_second_window_latent_against_the_reference(pipe, tag):
    rc.check_window_latent(pipe, DEV, tag, 1, "gpu")
