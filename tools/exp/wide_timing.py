"""Wall-clock cost of the `precise-wide` policy and of on_range_exceeded = "escalate" at BASELINE config 3.

    python tools/exp/wide_timing.py [--reps 5]

One MI355X, the full network on synthetic weights: ms per evaluation (mean of --reps after two warm-ups) under `precise` with "warn",
`precise` with "escalate" (ordinary weights: never triggers, adds one synchronous counter read per evaluation), `precise-wide` and
`precise-full` (split weights on top: profiles/precise_full.md),
then the per-launch time of the split attention kernels from one profiled `precise-wide` evaluation (hip.Profiler, HIP events).

    python tools/exp/wide_timing.py --ckpt [--rounds 3] [--reps 5]

`precise`, `precise-ckpt` and `precise-full` INTERLEAVED: --rounds rounds of (policy A, policy B, policy C), each --reps evaluations
after two warm-ups, so that drift of the box hits all three alike; per policy the per-round means, their mean and their spread
(max - min), then the per-family split of one profiled evaluation each (profiles/precise_ckpt.md)."""
import argparse
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

from helpers import cond, product_network, step_inputs  # noqa: E402
from panacea_amd import hip  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--ckpt", action="store_true", help="precise / precise-ckpt / precise-full interleaved + their per-family split")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    w, _, kw = product_network("full", "cpu")
    w = w.to("cuda")
    m = w.diffusion_model
    inp = step_inputs("full", kw, "cuda")

    def ms():
        for _ in range(2):
            w(inp["x"], inp["t"], cond(inp))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            w(inp["x"], inp["t"], cond(inp))
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / a.reps * 1e3

    if a.ckpt:
        policies = ("precise", "precise-ckpt", "precise-full")
        per = {p: [] for p in policies}
        with torch.no_grad():
            for _ in range(a.rounds):
                for p in policies:
                    m.precision = p
                    per[p].append(ms())
            for p in policies:
                v = per[p]
                print(f"{p}: {sum(v) / len(v):.1f} ms per evaluation (rounds: {', '.join(f'{x:.1f}' for x in v)}; "
                      f"spread {max(v) - min(v):.1f})", flush=True)
            for p in policies:
                m.precision = p
                prof = hip.Profiler()
                hip.set_profiler(prof)
                w(inp["x"], inp["t"], cond(inp))
                hip.set_profiler(None)
                fam = sorted(prof.summary().items(), key=lambda kv: -kv[1]["ms"])
                print(f"{p} per family (ms): " + ", ".join(f"{k} {v['ms']:.1f}" for k, v in fam if v["ms"] >= 0.5), flush=True)
            # A/B of the persistent GEGLU kernel's weight part: PNC_OPT_GEMM_PERSIST bit 0 off sends FF1 to the one-tile-per-workgroup
            # kernel (gemm_glds_ws_kernel), everything else as before
            m.precision = "precise-ckpt"
            ab = {3: [], 2: []}
            for _ in range(a.rounds):
                for opt in (3, 2):
                    hip.set_option(hip.OPT_GEMM_PERSIST, opt)
                    ab[opt].append(ms())
            hip.set_option(hip.OPT_GEMM_PERSIST, 3)
            for opt, what in ((3, "FF1 on the persistent GEGLU kernel"), (2, "FF1 one tile per workgroup")):
                v = ab[opt]
                print(f"precise-ckpt, {what}: {sum(v) / len(v):.1f} ms (rounds: {', '.join(f'{x:.1f}' for x in v)})", flush=True)
        return
    with torch.no_grad():
        print(f"precise, warn: {ms():.1f} ms per evaluation")
        m.on_range_exceeded = "escalate"
        print(f"precise, escalate: {ms():.1f} ms per evaluation (escalated: {m.escalated})")
        m.on_range_exceeded = "warn"
        m.precision = "precise-wide"
        print(f"precise-wide: {ms():.1f} ms per evaluation")
        m.precision = "precise-full"
        print(f"precise-full: {ms():.1f} ms per evaluation")
        m.precision = "precise-wide"
        p = hip.Profiler()
        hip.set_profiler(p)
        w(inp["x"], inp["t"], cond(inp))
        hip.set_profiler(None)
    for fam, v in sorted(p.summary().items()):
        if "split" in fam:
            print(f"{fam}: {v['launches']} launches, {v['ms']:.2f} ms, {v['ms'] / v['launches'] * 1e3:.1f} us per launch")


if __name__ == "__main__":
    main()
