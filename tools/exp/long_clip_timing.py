"""Timings of the 9..16-frame kernels and of one evaluation at 16 frames (profiles/long_clips.md).

    python tools/exp/long_clip_timing.py [--rounds 7] [--reps 20] [--skip-network]

One MI355X.  Kernel times are device events around --reps back-to-back launches after a warm-up, in --rounds interleaved rounds
(every variant once per round, in turn); median and minimum over the rounds.  Bytes are the algorithm's: what the kernel has to
read and write once, computed from the shapes.

  1. temporal attention at the level-0 / 1 / 2 shapes of BASELINE config 3 (B = 2, Npix = 12288 / 3072 / 768, heads 5 / 10 / 20):
     pnc_attn_temporal_f16 at T = 16 (attn_temporal_wide_kernel) against pnc_attn_temporal_split_f16 on the same q / k / v (plus lo
     planes), and the T = 8 kernel at the same shapes for its GB/s.
  2. temporal GroupNorm + SiLU (e4m3 lo plane, the `precise` form) at T = 16 and T = 8, C = 320 / 640 / 1280 at those pixel counts.
  3. one fused + hoisted Euler / CFG step (= one evaluation of the CFG pair) of the full network under `precise` at config-3
     geometry, T = 8 and T = 16.
"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

from panacea_amd import configs, hip  # noqa: E402

DEV = "cuda"
LEVELS = [(12288, 5, 320), (3072, 10, 640), (768, 20, 1280)]      # (pixels per frame, heads, channels) of levels 0 / 1 / 2


def rnd(*shape, dtype=torch.float16, seed=1, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def interleaved(variants, rounds, reps):
    """variants: {name: fn}; returns {name: (median_us, min_us)} per launch"""
    for fn in variants.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1) / reps * 1e3)
    return {k: (statistics.median(v), min(v)) for k, v in out.items()}


def attention(rounds, reps):
    print("## temporal attention (B = 2; us per launch: median / min over the rounds; GB/s from the median)")
    B = 2
    for Npix, heads, C in LEVELS:
        t = {}
        for T in (16, 8):
            M = B * T * Npix
            qkv = rnd(M, 3 * C, seed=T)
            t[T] = (qkv, torch.zeros(M, C, device=DEV, dtype=torch.float16))
        qkv, o = t[16]
        lo = rnd(B * 16 * Npix, 3 * C, seed=3, scale=0.3)
        o2, o2lo = torch.zeros_like(o), torch.zeros_like(o)
        q8, o8 = t[8]
        kw = dict(B=B, Npix=Npix, heads=heads, scale=0.125)
        res = interleaved({
            "T=16 mfma": lambda: hip.attn_temporal(qkv, 3 * C, qkv[:, C:], 3 * C, qkv[:, 2 * C:], 3 * C, o, C, T=16, **kw),
            "T=16 split": lambda: hip.attn_temporal_split(qkv, lo, 3 * C, qkv[:, C:], lo[:, C:], 3 * C, qkv[:, 2 * C:], lo[:, 2 * C:],
                                                          3 * C, o2, o2lo, C, T=16, **kw),
            "T=8 valu": lambda: hip.attn_temporal(q8, 3 * C, q8[:, C:], 3 * C, q8[:, 2 * C:], 3 * C, o8, C, T=8, **kw),
        }, rounds, reps)
        for name, (med, mn) in res.items():
            T = 8 if name.startswith("T=8") else 16
            nbytes = (16.0 if "split" in name else 8.0) * B * T * Npix * C          # q, k, v in + o out, fp16 (x 2 planes when split)
            print(f"Npix {Npix:5d} heads {heads:2d}  {name:10s}: {med:8.1f} / {mn:8.1f} us   {nbytes / med / 1e3:7.0f} GB/s")
        ok = res["T=16 mfma"][0] <= res["T=16 split"][0]
        print(f"Npix {Npix:5d}: T=16 mfma not slower than the split kernel: {ok}")
        assert torch.isfinite(o).all()


def groupnorm(rounds, reps):
    print("## temporal GroupNorm + SiLU, e4m3 lo plane (B = 2; us per launch: median / min; GB/s from the median)")
    B = 2
    for Npix, _, C in LEVELS:
        gamma, beta = rnd(C, dtype=torch.float32, seed=5) * 0.5 + 1, rnd(C, dtype=torch.float32, seed=6) * 0.3
        bufs = {}
        for T in (16, 8):
            M = B * T * Npix
            bufs[T] = (rnd(M, C, dtype=torch.float32, seed=T), torch.zeros(M, C, device=DEV, dtype=torch.float16),
                       torch.zeros(M, C, device=DEV, dtype=torch.uint8))
        res = interleaved({f"T={T}": (lambda T=T: hip.groupnorm_temporal_silu(bufs[T][0], B, T, Npix, C, gamma, beta, 1e-5, bufs[T][1],
                                                                             bufs[T][2])) for T in (16, 8)}, rounds, reps)
        for name, (med, mn) in res.items():
            T = int(name[2:])
            nbytes = 7.0 * B * T * Npix * C                                         # fp32 in, fp16 + e4m3 out
            print(f"Npix {Npix:5d} C {C:4d}  {name:5s}: {med:8.1f} / {mn:8.1f} us   {nbytes / med / 1e3:7.0f} GB/s")


def network(reps):
    from helpers import manifest
    from panacea_amd import build_network, sampling as S, synth
    print("## one fused + hoisted Euler / CFG step of the full network, `precise`, config-3 geometry (32x384 latent, CFG pair)")
    sd = synth.synth_state_dict(manifest("full"))
    for T in (8, 16):
        kw = configs.with_frames(configs.get("full"), T)
        w = build_network(kw)
        w.diffusion_model.load_state_dict(sd, strict=True)
        w = w.to(DEV)
        assert w.diffusion_model.precision == "precise"
        inp = {k: v.to(DEV) for k, v in synth.synth_inputs(2, T, 32, 384, context_dim=kw["context_dim"]).items()}
        c = {"crossattn": inp["crossattn"][1:2], "concat": inp["concat"][T:], "cond_feat": inp["cond_feat"][T:]}
        uc = {"crossattn": inp["crossattn"][0:1], "concat": inp["concat"][:T], "cond_feat": inp["cond_feat"][:T]}
        smp = S.EulerEDMSampler(25, guider=S.VanillaCFG(5.0), device=DEV)
        sig = smp.sigmas()
        x0 = inp["x"][T:] * 14.6
        s_in = x0.new_ones([T])
        bd = S.BoundDenoiser(S.DiscreteDenoiser().to(DEV), w)
        with torch.no_grad():
            c2, u2 = S.hoist_invariants(w, smp.guider, c, uc)
            assert smp._fusable(bd, x0, c2)
            x = x0
            for i in range(2):
                x = smp.sampler_step(s_in * sig[i], s_in * sig[i + 1], bd, x, c2, u2)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(reps):
                x = smp.sampler_step(s_in * sig[2 + i], s_in * sig[3 + i], bd, x, c2, u2)
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) / reps * 1e3
        assert torch.isfinite(x).all()
        print(f"T = {T:2d}: {ms:8.1f} ms per evaluation ({ms / T:.1f} ms per frame), eager launches, {reps} steps timed")
        del w, bd, c2, u2
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-network", action="store_true")
    a = ap.parse_args()
    print("library", hip.build_digest()[:12], torch.cuda.get_device_name(0))
    attention(a.rounds, a.reps)
    groupnorm(a.rounds, a.reps)
    if not a.skip_network:
        network(min(a.reps, 10))


if __name__ == "__main__":
    main()
