"""Timings of the fused first-stage attention (profiles/frame_attention.md).

    python tools/exp/frame_attn_timing.py [--rounds 7] [--reps 3] [--skip-long]

One MI355X.  Times are device events around --reps back-to-back runs after a warm-up, in --rounds interleaved rounds (every variant
once per round, in turn); median and minimum over the rounds.  FLOP = 4 N^2 C per frame (both products).

  1. the product's shape, F = 8 frames of N = 12288 tokens, C = 512, on the same q / k / V^T: pnc_attn_frame_f16 (one launch) against
     the three launches per frame AttnBlock uses by default (pnc_gemm_f16 -> pnc_softmax_rows_f16 -> pnc_gemm_f16, F times);
     max-abs difference of the two outputs.
  2. above the row softmax's limit: F = 1, N = 49152 (six views of 512 x 1024: latent 64 x 768), C = 512, fused; finite output and
     32 sampled query rows against the float64 reference of tests/frame_attn_ref64.py.
  3. AttnBlock(512) on that frame: runs, finite, peak memory growth (the N x N fp32 scores alone would be 9.7 GB).
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import frame_attn_ref64 as ref64  # noqa: E402
from panacea_amd import hip  # noqa: E402
from panacea_amd.nn import model  # noqa: E402

DEV = "cuda"


def rnd(*shape, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).half().to(DEV)


def interleaved(variants, rounds, reps):
    """variants: {name: fn}; returns {name: (median_us, min_us)} per run"""
    for fn in variants.values():
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


def report(name, med, mn, F, N, C):
    fl = 4.0 * F * N * N * C
    print(f"  {name:<28} {med / F:10.1f} / {mn / F:10.1f} us per frame   {fl / med / 1e6:7.1f} TFLOP/s (median)   "
          f"{med / 1e3:8.2f} ms for the {F} frame(s)")


def product_shape(rounds, reps):
    F, N, C = 8, 12288, 512
    scale = float(C) ** -0.5
    print(f"## 1. F = {F}, N = {N}, C = {C} (us per frame: median / min over {rounds} rounds of {reps} runs)")
    q, k, vt = rnd(F * N, C, seed=1), rnd(F * N, C, seed=2), rnd(F, C, N, seed=3)
    o_f, o_3 = torch.zeros(F * N, C, device=DEV, dtype=torch.float16), torch.zeros(F * N, C, device=DEV, dtype=torch.float16)
    s32 = torch.empty(N, N, device=DEV, dtype=torch.float32)
    p16 = torch.empty(N, N, device=DEV, dtype=torch.float16)

    def fused():
        hip.attn_frame(q, C, k, C, vt, N, C * N, o_f, C, F=F, N=N, C=C, scale=scale)

    def three():
        for f in range(F):
            hip.gemm(q[f * N:], k[f * N:(f + 1) * N], M=N, N=N, K=C, lda=C, out32=s32, ldc32=N)
            hip.softmax_rows(s32, N, N, N, scale, p16, N)
            hip.gemm(p16, vt[f], M=N, N=C, K=N, lda=N, out16=o_3[f * N:], ldc16=C)

    res = interleaved({"fused (1 launch)": fused, f"three launches x {F}": three}, rounds, reps)
    for name, (med, mn) in res.items():
        report(name, med, mn, F, N, C)
    d = (o_f.float() - o_3.float()).abs()
    print(f"  max |fused - three launches| = {d.max().item():.3e}   (|o| max {o_3.float().abs().max().item():.3f}); both finite: "
          f"{bool(torch.isfinite(o_f).all() and torch.isfinite(o_3).all())}")


def long_frame(rounds, reps):
    F, N, C = 1, 49152, 512
    scale = float(C) ** -0.5
    print(f"## 2. F = {F}, N = {N}, C = {C}, fused")
    q, k, vt = rnd(N, C, seed=4), rnd(N, C, seed=5), rnd(1, C, N, seed=6)
    o = torch.zeros(N, C, device=DEV, dtype=torch.float16)
    res = interleaved({"fused (1 launch)": lambda: hip.attn_frame(q, C, k, C, vt, N, C * N, o, C, F=F, N=N, C=C, scale=scale)}, rounds, reps)
    for name, (med, mn) in res.items():
        report(name, med, mn, F, N, C)
    rows = torch.cat([torch.arange(8), N // 2 + torch.arange(16), torch.arange(N - 8, N)])
    ref = ref64.attn_frame(q, C, k, C, vt, N, C * N, F=F, N=N, C=C, scale=scale, rows=rows)[0]
    err = (o[rows.to(DEV)].cpu().double() - ref).abs()
    over = (err - (3e-3 + 2e-3 * ref.abs())).max().item()
    print(f"  finite: {bool(torch.isfinite(o).all())}; {rows.numel()} sampled rows vs float64: max |err| {err.max().item():.3e} "
          f"(|ref| max {ref.abs().max().item():.3f}), over atol 3e-3 + rtol 2e-3 by {over:.3e}")
    print(f"## 3. AttnBlock({C}) on one 64 x 768 frame ({N} tokens)")
    torch.manual_seed(0)
    blk = model.AttnBlock(C).to(DEV)
    x = torch.randn(1, C, 64, 768, generator=torch.Generator().manual_seed(7)).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.no_grad():
        out = blk(x)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - before
    print(f"  output finite: {bool(torch.isfinite(out).all())}; peak memory growth {growth / 2 ** 20:.0f} MiB "
          f"(N x N fp32 scores would be {4.0 * N * N / 2 ** 20:.0f} MiB)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--skip-long", action="store_true")
    a = ap.parse_args()
    print(f"build digest {hip.build_digest()[:16]}; {torch.cuda.get_device_name(0)}")
    product_shape(a.rounds, a.reps)
    if not a.skip_long:
        long_frame(a.rounds, a.reps)
