#!/usr/bin/env python
"""Timing of pnc_frames_renoise next to pnc_add_f32 on the same number of bytes (profiles/clip_editing.md).

    python tools/exp/frames_renoise_timing.py [--launches 200] [--rounds 5]

Shapes: the config-3 latent (8, 4, 12288) and (16, 4, 12288).  Per shape and round, in one process, alternating:
  renoise-all   z, noise -> out, every frame kept (the start of a schedule): 12 bytes per element
  add_f32       x + a -> y32 (the yardstick: an elementwise pass of this library): 12 bytes per element
  renoise-keep2 frames 0 and T-1 kept, in place on x (the launch after a step): 12 bytes per element of the two frames
Two clocks per entry: HIP events around `launches` back-to-back launches from the host ("eager": the host's launch rate bounds it
from below), and around one replay of a hipGraph that holds the same `launches` launches ("graph": the device's launch-to-launch
time).  One JSON line per (shape, entry, round); a median table at the end.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--launches", type=int, default=200)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
sys.path.insert(0, str(Path(__file__).resolve().parent.parent.parent))
import torch  # noqa: E402
from panacea_amd import hip  # noqa: E402

assert torch.cuda.is_available(), "this measurement needs the MI355X"
DEV = torch.device("cuda", 0)
hip.load()


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n                 # us per launch


def graphed(fn, n):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(n):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return lambda: timed(g.replay, 1) / n


rows = {}
for T in (8, 16):
    shape = (T, 4, 12288)
    gen = torch.Generator().manual_seed(T)
    z, noise, x = (torch.randn(shape, generator=gen).to(DEV) for _ in range(3))
    out, y = torch.empty_like(z), torch.empty_like(z)
    sigma = (torch.rand(T, generator=gen) * 14 + 0.03).to(DEV)
    keep = torch.zeros(T)
    keep[0] = keep[T - 1] = 1.0
    keep = keep.to(DEV)
    n = z.numel()
    entries = {
        "renoise-all": (lambda: hip.frames_renoise(z, noise, sigma, out), 12.0 * n),
        "add_f32": (lambda: hip.add_f32(z, noise, n, y, None), 12.0 * n),
        "renoise-keep2": (lambda: hip.frames_renoise(z, noise, sigma, x, keep=keep, x=x), 12.0 * n * 2 / T),
    }
    replays = {}
    for name, (fn, _) in entries.items():                # warm-up: code objects, then the captured form
        timed(fn, 20)
        replays[name] = graphed(fn, a.launches)
    for r in range(a.rounds):
        for name, (fn, nbytes) in entries.items():
            us_e, us_g = timed(fn, a.launches), replays[name]()
            rows.setdefault((shape, name), []).append((us_e, us_g))
            print(json.dumps(dict(shape=shape, entry=name, round=r, bytes=nbytes, us_eager=round(us_e, 3), us_graph=round(us_g, 3),
                                  gbs_eager=round(nbytes / us_e / 1e3, 1), gbs_graph=round(nbytes / us_g / 1e3, 1))), flush=True)
    assert torch.equal(out, z + noise * sigma[:, None, None])
print(f"\nmedian of {a.rounds} rounds, {a.launches} launches each")
print(f"{'shape':18s} {'entry':14s} {'MB':>7s} {'eager us':>9s} {'GB/s':>7s} {'graph us':>9s} {'GB/s':>7s}")
for (shape, name), v in rows.items():
    nbytes = 12.0 * shape[0] * shape[1] * shape[2] * (2 / shape[0] if name == "renoise-keep2" else 1)
    e, g = statistics.median(t[0] for t in v), statistics.median(t[1] for t in v)
    print(f"{str(shape):18s} {name:14s} {nbytes / 1e6:7.2f} {e:9.2f} {nbytes / e / 1e3:7.0f} {g:9.2f} {nbytes / g / 1e3:7.0f}")
for shape in {k[0] for k in rows}:
    for col, what in ((0, "eager"), (1, "graph")):
        r = statistics.median(t[col] for t in rows[(shape, "add_f32")]) / statistics.median(t[col] for t in rows[(shape, "renoise-all")])
        print(f"{shape}: renoise-all reaches {r:.2f} of add_f32's bandwidth ({what})")
