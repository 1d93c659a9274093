"""The fixture of the first stage's operand-policy tests: tests/golden/vae_tiny_w32.npz (tools/gen_golden_vae_w32.py) — the TINY first
stage of tests/test_vae.py on UNROUNDED fp32 synthetic weights, the reference's fp32 outputs, "truth" (oracle/vae_oracle.py in float64
on the same weights) and e32 = max|reference fp32 - truth| per output.

The end-to-end bound of `precise-full` is 16 e32 per output, from the formats alone: a split pair carries about 22 bits against fp32's
24, four times fp32's rounding, and another factor of four covers the dropped lo.lo products and a summation order other than the
reference's.  Nothing in it comes from this project's own output."""
import functools
import json
from pathlib import Path

import numpy as np
import torch

from panacea_amd import synth
from panacea_amd.nn import model

GOLDEN = Path(__file__).resolve().parent / "golden"
TINY = dict(double_z=True, z_channels=4, resolution=16, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2], num_res_blocks=1,
            attn_resolutions=[], dropout=0.0)                    # tests/test_vae.py: mid block of 128 channels
FACTOR = 16.0


@functools.lru_cache(maxsize=None)
def fixture():
    g = np.load(GOLDEN / "vae_tiny_w32.npz")
    out = {k: torch.from_numpy(g[k]) for k in ("z", "x", "img_ref32", "moments_ref32", "img_truth", "moments_truth")}
    out.update(e32_img=float(g["e32_img"]), e32_moments=float(g["e32_moments"]), salt=int(g["salt"]))
    assert out["img_truth"].dtype == torch.float64 and out["moments_truth"].dtype == torch.float64
    return out


@functools.lru_cache(maxsize=None)
def weights(kind, rounded=False):
    """the synthetic state dict of the TINY decoder ("dec") or encoder ("enc"): unrounded fp32 values, or their fp16 roundings"""
    man = json.loads((GOLDEN / ("manifest_vae_tiny.json" if kind == "dec" else "manifest_vae_enc_tiny.json")).read_text())
    return synth.synth_state_dict(man, salt=fixture()["salt"], round_fp16=rounded)


def stage(kind, precision=None, rounded=False, device=None):
    kw = {} if precision is None else dict(precision=precision)
    net = (model.FirstStageDecoder if kind == "dec" else model.FirstStageEncoder)(4, TINY, **kw)
    net.load_state_dict(weights(kind, rounded), strict=True)
    return net if device is None else net.to(device)


def err(got, truth):
    return (got.detach().cpu().double() - truth).abs().max().item()


def expected_bytes(truth_img, tol):
    """-> (the bytes of the header's quantisation formula (section 7, pnc_tokens_to_u8) applied to truth, channels-last; the mask of
    the bytes a value within `tol` (in units of t * 255) of truth may truncate differently).  Such a byte has truth's pre-truncation
    value t * 255 within tol of an integer; of the values the clamp holds at exactly 0 or 255 — integers all of them — only those count
    whose unclamped value lies within tol of the clamp: the others stay clamped whatever the error.  From truth alone."""
    u = (truth_img.permute(0, 2, 3, 1).contiguous() + 1.0) * 0.5 * 255.0         # unclamped
    t = u.clamp(0.0, 255.0)
    near = ((t - t.round()).abs() <= tol) & (u > -tol) & (u < 255.0 + tol)
    return t.to(torch.int64).to(torch.uint8), near
