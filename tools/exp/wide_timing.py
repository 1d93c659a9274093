"""Wall-clock cost of the `precise-wide` policy and of on_range_exceeded = "escalate" at BASELINE config 3.

    python tools/exp/wide_timing.py [--reps 5]

One MI355X, the full network on synthetic weights: ms per evaluation (mean of --reps after two warm-ups) under `precise` with "warn",
`precise` with "escalate" (ordinary weights: never triggers, adds one synchronous counter read per evaluation), `precise-wide` and
`precise-full` (split weights on top: profiles/precise_full.md),
then the per-launch time of the split attention kernels from one profiled `precise-wide` evaluation (hip.Profiler, HIP events)."""
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
