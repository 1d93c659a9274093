"""Timings of the first stage's operand policies (profiles/first_stage_precise.md).

    python tools/exp/first_stage_precise_timing.py [--rounds 5] [--reps 2] [--skip-stage]

One MI355X.  Device events around --reps back-to-back runs after a warm-up, in --rounds interleaved rounds (every variant once per
round, in turn); median and minimum over the rounds, one process.

  1. pnc_attn_frame_split_f16 against pnc_attn_frame_f16 on the same hi planes (lo planes: the residuals of fp32 data), C = 512:
     F = 8, N = 12288 (the product's mid block) and F = 1, N = 49152.  FLOP = 4 N^2 C per frame for the single-plane kernel, three
     times that for the split one.
  2. ms per 8-frame decode (latent 32 x 384 -> 256 x 3072) and encode at the product's size, full-width synthetic first stage, for
     `fast`, `precise-wide`, `precise-full`.
"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

from frame_attn_timing import interleaved  # noqa: E402
from panacea_amd import hip, synth  # noqa: E402
from panacea_amd.nn import model  # noqa: E402

DEV = "cuda"
FULL = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
            num_res_blocks=2, attn_resolutions=[], dropout=0.0)          # configs/inference_nuscenes.yaml:101-111


def pair(*shape, seed):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    hi = x.half()
    return hi.to(DEV), ((x - hi.float()) * 2048.0).half().to(DEV)


def kernels(F, N, rounds, reps):
    C = 512
    scale = float(C) ** -0.5
    print(f"## attention, F = {F}, N = {N}, C = {C} (median / min over {rounds} rounds of {reps} runs)")
    (q, ql), (k, kl), (v, vl) = pair(F * N, C, seed=1), pair(F * N, C, seed=2), pair(F * N, C, seed=3)
    vt = v.view(F, N, C).transpose(1, 2).contiguous()
    o1, o, ol = (torch.zeros(F * N, C, device=DEV, dtype=torch.float16) for _ in range(3))
    res = interleaved({"pnc_attn_frame_f16": lambda: hip.attn_frame(q, C, k, C, vt, N, C * N, o1, C, F=F, N=N, C=C, scale=scale),
                       "pnc_attn_frame_split_f16": lambda: hip.attn_frame_split(q, ql, C, k, kl, C, v, vl, C, o, ol, C, F=F, N=N, C=C,
                                                                                scale=scale)}, rounds, reps)
    for name, (med, mn) in res.items():
        fl = (12.0 if "split" in name else 4.0) * F * N * N * C
        print(f"  {name:<28} {med / 1e3:9.2f} / {mn / 1e3:9.2f} ms   {fl / med / 1e6:7.1f} TFLOP/s of MFMA work (median)")
    a, b = res["pnc_attn_frame_f16"][0], res["pnc_attn_frame_split_f16"][0]
    d = (o.float() - o1.float()).abs().max().item()
    print(f"  split / single = {b / a:.2f}; max |o_hi - single| = {d:.3e}; finite: {bool(torch.isfinite(o).all() and torch.isfinite(ol).all())}")


def stages(rounds, reps):
    F, h, w = 8, 32, 384
    print(f"## first stage, {F} frames of {8 * h} x {8 * w}, full width (ms per call: median / min over {rounds} rounds of {reps} runs)")
    z = (torch.randn(F, 4, h, w, generator=torch.Generator().manual_seed(3)) * 2.0).to(DEV)
    x = torch.tanh(torch.randn(F, 3, 8 * h, 8 * w, generator=torch.Generator().manual_seed(4))).to(DEV)
    dec, enc = {}, {}
    for p in model.FIRST_STAGE_PRECISIONS:
        for cls, nets in ((model.FirstStageDecoder, dec), (model.FirstStageEncoder, enc)):
            net = cls(4, FULL, precision=p)
            net.load_state_dict(synth.synth_state_dict({k: list(v.shape) for k, v in net.state_dict().items()}, round_fp16=False), strict=True)
            nets[p] = net.to(DEV)
    for what, nets, run in (("decode", dec, lambda n: n.decode(z)), ("encode (moments)", enc, lambda n: n.moments(x))):
        res = interleaved({p: (lambda n=n: run(n)) for p, n in nets.items()}, rounds, reps)
        base = res["fast"][0]
        for p, (med, mn) in res.items():
            print(f"  {what:<18} {p:<14} {med / 1e3:9.1f} / {mn / 1e3:9.1f} ms   {med / base:5.2f} x fast")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--skip-stage", action="store_true")
    a = ap.parse_args()
    print(f"build digest {hip.build_digest()[:16]}; {torch.cuda.get_device_name(0)}")
    kernels(8, 12288, a.rounds, a.reps)
    kernels(1, 49152, a.rounds, a.reps)
    if not a.skip_stage:
        stages(a.rounds, a.reps)
