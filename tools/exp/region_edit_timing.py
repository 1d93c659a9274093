#!/usr/bin/env python
"""Timing of the region-editing kernels (profiles/region_editing.md).

    python tools/exp/region_edit_timing.py [--launches 200] [--rounds 5]

Latents: the config-3 latent (8, 4, 12288) and (16, 4, 12288).  Per shape and round, in one process, alternating:
  masked-all    pnc_latent_renoise_masked, every pixel kept, in place on x: z, noise, the mask and out — 12 bytes per element + the mask
  masked-view   the same with one of six view bands kept (the launch after a step of a view edit): 12 bytes per kept element + the mask
  renoise-all   pnc_frames_renoise, every frame kept, z, noise -> out (the yardstick of the gate): 12 bytes per element
  add_f32       pnc_add_f32 on the same elements: 12 bytes per element
Two clocks per entry, as in frames_renoise_timing.py: HIP events around `launches` back-to-back launches from the host ("eager"), and
around one replay of a hipGraph that holds the same `launches` launches ("graph": the device's launch-to-launch time).
The gate (profiles/clip_editing.md's, on the graph clock): masked-all reaches at least 0.8 of renoise-all's rate on the same shape.

Frames: pnc_mask_pool_u8 (f = 8) and pnc_u8_select (C = 3) at the product's 8 x 256 x 3072 frames next to a torch copy of the same
bytes; each runs once per edit, so these are reported only.  One JSON line per (shape, entry, round); median tables at the end.
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
print("build digest", hip.load().pnc_build_digest().decode()[:16])


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


def measure(shape, entries, rows):
    replays = {}
    for name, (fn, _) in entries.items():                # warm-up: code objects, then the captured form
        timed(fn, 20)
        replays[name] = graphed(fn, a.launches)
    for r in range(a.rounds):
        for name, (fn, nbytes) in entries.items():
            us_e, us_g = timed(fn, a.launches), replays[name]()
            rows.setdefault((shape, name), []).append((us_e, us_g, nbytes))
            print(json.dumps(dict(shape=shape, entry=name, round=r, bytes=nbytes, us_eager=round(us_e, 3), us_graph=round(us_g, 3),
                                  gbs_eager=round(nbytes / us_e / 1e3, 1), gbs_graph=round(nbytes / us_g / 1e3, 1))), flush=True)


rows = {}
for T in (8, 16):
    shape = (T, 4, 12288)
    h, w = 32, 384
    gen = torch.Generator().manual_seed(T)
    z, noise, x0 = (torch.randn(shape, generator=gen).to(DEV) for _ in range(3))
    x_all, x_view, out, y = x0.clone(), x0.clone(), torch.empty_like(z), torch.empty_like(z)
    sigma = (torch.rand(T, generator=gen) * 14 + 0.03).to(DEV)
    every = torch.ones(T, h * w, device=DEV)
    view = torch.zeros(T, h, w)
    view[:, :, :w // 6] = 1.0
    view = view.reshape(T, h * w).to(DEV)
    n = z.numel()
    entries = {
        "masked-all": (lambda: hip.latent_renoise_masked(z, noise, sigma, every, x_all, x_all), 12.0 * n + 4.0 * every.numel()),
        "renoise-all": (lambda: hip.frames_renoise(z, noise, sigma, out), 12.0 * n),
        "masked-view": (lambda: hip.latent_renoise_masked(z, noise, sigma, view, x_view, x_view), 12.0 * n / 6 + 4.0 * view.numel()),
        "add_f32": (lambda: hip.add_f32(z, noise, n, y, None), 12.0 * n),
    }
    measure(shape, entries, rows)
    want = z + noise * sigma[:, None, None]
    assert torch.equal(out, want) and torch.equal(x_all, want)
    kept = (view > 0).view(T, 1, h * w).expand(shape)
    assert torch.equal(x_view, torch.where(kept, want, x0))

# the byte kernels at the product's frames
T, H, W = 8, 256, 3072
gen = torch.Generator().manual_seed(3)
mask = torch.zeros(T, H, W, dtype=torch.uint8)
mask[:, :, :W // 6] = 255
mask = mask.to(DEV)
pooled = torch.empty(T, H // 8, W // 8, device=DEV)
src, dec = (torch.randint(0, 256, (T, H, W, 3), generator=gen, dtype=torch.uint8).to(DEV) for _ in range(2))
sel, mask2, src2 = torch.empty_like(src), torch.empty_like(mask), torch.empty_like(src)
frames = {
    "mask_pool_u8": (lambda: hip.mask_pool_u8(mask, 8, pooled), 1.0 * mask.numel() + 4.0 * pooled.numel()),
    "copy of the mask": (lambda: mask2.copy_(mask), 2.0 * mask.numel()),
    "u8_select": (lambda: hip.u8_select(src, dec, mask, sel), 3.0 * src.numel() + 1.0 * mask.numel()),
    "copy of the frames": (lambda: src2.copy_(src), 2.0 * src.numel()),
}
measure((T, H, W), frames, rows)
assert torch.equal(pooled, (mask != 0).view(T, H // 8, 8, W // 8, 8).all(4).all(2).float())
assert torch.equal(sel, torch.where((mask != 0)[..., None], src, dec))

print(f"\nmedian (min .. max) of {a.rounds} rounds, {a.launches} launches each")
print(f"{'shape':18s} {'entry':20s} {'MB':>7s} {'graph us':>24s} {'GB/s':>7s} {'eager us':>24s} {'GB/s':>7s}")
med = {}
for (shape, name), v in rows.items():
    nbytes = v[0][2]
    e, g = [t[0] for t in v], [t[1] for t in v]
    med[(shape, name)] = (statistics.median(e), statistics.median(g))
    cell = lambda s: f"{statistics.median(s):.2f} ({min(s):.2f} .. {max(s):.2f})"      # noqa: E731
    print(f"{str(shape):18s} {name:20s} {nbytes / 1e6:7.2f} {cell(g):>24s} {nbytes / statistics.median(g) / 1e3:7.0f} "
          f"{cell(e):>24s} {nbytes / statistics.median(e) / 1e3:7.0f}")
for shape in [k[0] for k in rows if k[1] == "masked-all"]:
    for col, what in ((1, "graph"), (0, "eager")):
        # rate = the bytes each entry must move / its time; the ratio of the rates on this shape
        rate = lambda name: rows[(shape, name)][0][2] / med[(shape, name)][col]      # noqa: E731
        print(f"{shape}: masked-all reaches {rate('masked-all') / rate('renoise-all'):.2f} of renoise-all's rate, "
              f"{med[(shape, 'masked-all')][col] / med[(shape, 'renoise-all')][col]:.2f} of its time ({what}); gate 0.8 on the graph clock")
