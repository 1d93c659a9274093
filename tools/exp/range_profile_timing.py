"""Measurements of the operand range profile (profiles/range_profile.md).

    python tools/exp/range_profile_timing.py kernel  [--rounds 7] [--reps 20]
    python tools/exp/range_profile_timing.py network [--rounds 5]          ms per evaluation, profile off / on, interleaved; then
                                                                           the class table of one evaluation
    python tools/exp/range_profile_timing.py report  [--tail 64]           class table of one full-size evaluation under `precise`
    python tools/exp/range_profile_timing.py eval    [--reps 10]           ms per evaluation only (runs on a tree without the profile
                                                                           too: the parent / this-tree comparison, one process each)

One MI355X.  Kernel times: device events around --reps back-to-back launches after a warm-up, --rounds interleaved rounds (every
variant once per round, in turn), median and minimum over the rounds; bytes are the ones the kernel reads.  The yardstick is the
library's pnc_layernorm on the same rows (fp32 in, fp16 out: 6 bytes per element).  One evaluation = the full network (UNet +
ControlNet, CFG pair, 8 frames, 32 x 384 latent: BASELINE config 3) called eagerly on synthetic weights under `precise`."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT))

from panacea_amd import build_network, configs, hip, synth  # noqa: E402

DEV = "cuda"
SHAPES = [(196608, 320), (49152, 640)]


def interleaved(variants, rounds, reps):
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


def kernel(rounds, reps):
    print("## pnc_operand_stats_f16 (us per launch: median / min over the rounds; GB/s of the bytes read, from the median)")
    for rows, C in SHAPES:
        g = torch.Generator().manual_seed(rows)
        x32 = (torch.randn(rows, C, generator=g) * 3.0).to(DEV)            # an activation plane (a slot of 64 values spans six or seven binades)
        hi = x32.half()
        lo8 = ((x32 - hi.float()) * 2048.0).clamp(-448, 448).to(torch.float8_e4m3fn).view(torch.uint8)
        lo16 = ((x32 - hi.float()) * 2048.0).half()
        wide = (x32 * torch.exp2(torch.randint(-14, 10, (rows, C), generator=g).float().to(DEV))).half()      # ~24 binades
        y16 = torch.empty_like(hi)
        gamma, beta = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        rec = torch.zeros(36, dtype=torch.int64, device=DEV)
        variants = {
            "fp16 + e4m3 lo": (lambda: hip.operand_stats(hi, lo8, rows, C, C, rec), 3.0),
            "fp16 alone": (lambda: hip.operand_stats(hi, None, rows, C, C, rec), 2.0),
            "fp16 + fp16 lo": (lambda: hip.operand_stats(hi, lo16, rows, C, C, rec), 4.0),
            "fp16 alone, 24 binades": (lambda: hip.operand_stats(wide, None, rows, C, C, rec), 2.0),
            "pnc_layernorm": (lambda: hip.layernorm(x32, C, rows, C, gamma, beta, 1e-5, y16, C), 6.0),
        }
        res = interleaved({k: v[0] for k, v in variants.items()}, rounds, reps)
        ln = res["pnc_layernorm"][0]
        for name, (med, mn) in res.items():
            nbytes = variants[name][1] * rows * C
            print(f"[{rows:6d}, {C:3d}] {name:24s}: {med:8.1f} / {mn:8.1f} us   {nbytes / med / 1e3:6.0f} GB/s   "
                  f"{med / ln:5.2f}x the layernorm's time")


def full_network(tail=0.0):
    man = json.loads((ROOT / "tests/golden/manifest_full.json").read_text())
    kw = configs.get("full")
    w = build_network(kw)
    w.diffusion_model.load_state_dict(synth.synth_state_dict(man, tail=tail), strict=True)
    w = w.to(DEV)
    w.diffusion_model.precision = "precise"
    T = kw["num_frames"]
    inp = {k: v.to(DEV) for k, v in synth.synth_inputs(2, T, 32, 384, context_dim=kw["context_dim"]).items()}
    cond = {k: inp[k] for k in ("concat", "crossattn", "cond_feat")}
    return w, inp, cond


def timed(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def evaluation(reps):
    w, inp, cond = full_network()
    with torch.no_grad():
        for _ in range(2):
            w(inp["x"], inp["t"], cond)
        ms = [timed(lambda: w(inp["x"], inp["t"], cond), reps) for _ in range(3)]
    print(f"evaluation, profile off ({ROOT.name}, library {hip.build_digest()[:12]}): " + " ".join(f"{v:.2f}" for v in ms) + " ms")


def network(rounds):
    w, inp, cond = full_network()
    m = w.diffusion_model
    off, on = [], []
    with torch.no_grad():
        for _ in range(2):
            ref = w(inp["x"], inp["t"], cond)
        for _ in range(rounds):
            off.append(timed(lambda: w(inp["x"], inp["t"], cond), 3))
            with m.profile_ranges() as prof:
                w(inp["x"], inp["t"], cond)                          # (first observed evaluation: names and slots are made here)
                on.append(timed(lambda: w(inp["x"], inp["t"], cond), 3))
                got = w(inp["x"], inp["t"], cond)
    torch.cuda.synchronize()
    print("## one evaluation, ms (3 evaluations per figure)")
    print("profile off:", " ".join(f"{v:.2f}" for v in off), f"  median {statistics.median(off):.2f}")
    print("profile on :", " ".join(f"{v:.2f}" for v in on), f"  median {statistics.median(on):.2f}")
    print("bit-identical with the profile on:", bool(torch.equal(ref, got)), " sites:", len(prof.report()["sites"]))
    report(0.0, (w, inp, cond))


def report(tail, net=None):
    sys.path.insert(0, str(ROOT / "tools"))
    from sample import print_range_profile
    w, inp, cond = net or full_network(tail)
    m = w.diffusion_model
    import warnings
    with torch.no_grad(), warnings.catch_warnings(), m.profile_ranges() as prof:
        warnings.simplefilter("ignore")
        w(inp["x"], inp["t"], cond)
        print(f"## weights: synthetic, tail = {tail}; lo_clamped (range monitor, quads) = {m.lo_clamped}")
    print_range_profile(prof, m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["kernel", "network", "report", "eval"])
    ap.add_argument("--rounds", type=int, default=None)
    ap.add_argument("--reps", type=int, default=None)
    ap.add_argument("--tail", type=float, default=0.0)
    a = ap.parse_args()
    print("library", hip.build_digest()[:12], torch.cuda.get_device_name(0))
    if a.what == "kernel":
        kernel(a.rounds or 7, a.reps or 20)
    elif a.what == "network":
        network(a.rounds or 5)
    elif a.what == "report":
        report(a.tail)
    else:
        evaluation(a.reps or 10)


if __name__ == "__main__":
    main()
