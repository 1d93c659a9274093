#!/usr/bin/env python
"""Timing of the image boundary at the product's size (8 frames of 256 x 3072; profiles/image_boundary.md).

    python tools/exp/image_boundary_timing.py --legs old [--root OTHER_TREE]     the float legs (any tree that has the float path)
    python tools/exp/image_boundary_timing.py --legs new                         the uint8 legs (this tree)
    python tools/exp/image_boundary_timing.py --kernels                          µs and GB/s of the two kernels, next to pnc_layernorm

Legs are wall-clock times around host work + copies + kernels, synchronised at both ends; one JSON line per leg and repetition.
  in : host uint8 layout (F, H, W, 19) -> filled operand planes of the hint stem ([F*H*W, 24] fp16)
       old: `astype(float32) / 255.0` on the host, H2D copy of the floats, permute to NCHW on the device, pnc_nchw_to_tokens_f16
            (`old-hostperm`: the permute on the host instead, before the copy)
       new: H2D copy of the bytes, pnc_u8_to_tokens_f16
  out: the decoder's token matrix ([F*H*W, 3] fp32 on the device) -> host uint8 (F, H, W, 3)
       old: Act.to_nchw(), then checkpoint._to_uint8 per frame (D2H copy of the floats, clamp / scale / permute / cast on the host)
       new: pnc_tokens_to_u8, one D2H copy of the bytes
`--root` runs the old legs against another checkout (the parent commit) for an interleaved comparison on one box.
"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--legs", choices=["old", "new"], default=None)
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent.parent))
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--frames", type=int, default=8)
ap.add_argument("--tag", default="")
a = ap.parse_args()
sys.path.insert(0, a.root)
import torch  # noqa: E402
from panacea_amd import checkpoint, hip  # noqa: E402
from panacea_amd.engine import Act  # noqa: E402

DEV = torch.device("cuda", 0)
F, H, W, C, CP = a.frames, 256, 3072, 19, 24
ROWS = F * H * W


def sync():
    torch.cuda.synchronize()


def emit(**kw):
    print(json.dumps(dict(kw, tag=a.tag, digest=hip.build_digest()[:16])), flush=True)


def timed(fn):
    sync()
    t0 = time.perf_counter()
    out = fn()
    sync()
    return (time.perf_counter() - t0) * 1e3, out


def legs():
    rng = np.random.default_rng(0)
    layout = rng.integers(0, 256, (F, H, W, C), dtype=np.uint8)
    tokens = (torch.randn((ROWS, 3), generator=torch.Generator().manual_seed(1)) * 0.7).to(DEV)
    planes = torch.empty((ROWS, CP), dtype=torch.float16, device=DEV)

    def in_old(host_permute):
        x = layout.astype(np.float32) / 255.0
        t = torch.from_numpy(x)
        if host_permute:
            d = t.permute(0, 3, 1, 2).contiguous().to(DEV)
        else:
            d = t.to(DEV).permute(0, 3, 1, 2).contiguous()
        hip.nchw_to_tokens_f16(d, C, None, 0, F, H * W, CP, planes)

    def in_new():
        from panacea_amd import image
        d = torch.from_numpy(layout).to(DEV)
        hip.u8_to_tokens_f16(d, image.device_table("layout", DEV), F, H * W, C, CP, planes)

    def out_old():
        img = Act(F, H, W, 3, f32=tokens).to_nchw()
        return np.stack([checkpoint._to_uint8(f) for f in img])

    def out_new():
        out = torch.empty((F, H, W, 3), dtype=torch.uint8, device=DEV)
        hip.tokens_to_u8(tokens, 3, ROWS, 3, out)
        return out.cpu().numpy()

    if a.legs == "old":
        runs = [("in", "old", lambda: in_old(False)), ("in", "old-hostperm", lambda: in_old(True)), ("out", "old", out_old)]
    else:
        runs = [("in", "new", in_new), ("out", "new", out_new)]
    sums = {}
    for leg, how, fn in runs:
        timed(fn)                                        # warm-up: allocator, first launch, lazily built tables
        for r in range(a.reps):
            ms, out = timed(fn)
            emit(leg=leg, how=how, rep=r, ms=round(ms, 3))
        if leg == "in":
            sums[how] = int(planes.view(torch.int16).long().sum().item())
        else:
            sums[how] = int(np.asarray(out, dtype=np.int64).sum())
    emit(checksums=sums)                                 # old and new legs of one kind must agree


def events(fn, n=10):
    fn()
    sync()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    sync()
    return e0.elapsed_time(e1) * 1e3 / n                 # µs per launch


def kernels():
    from panacea_amd import image
    src = torch.randint(0, 256, (F, H * W, C), dtype=torch.uint8, device=DEV)
    lut = image.device_table("layout", DEV)
    hi = torch.empty((ROWS, CP), dtype=torch.float16, device=DEV)
    lo = torch.empty_like(hi)
    f32 = src.float().div(255.0).permute(0, 2, 1).contiguous()
    tok = torch.randn((ROWS, 3), device=DEV)
    out = torch.empty((ROWS, 3), dtype=torch.uint8, device=DEV)
    nchw = torch.empty((F, 3, H * W), device=DEV)
    M, CH = 196608, 320                                  # the level-0 LayerNorm of the denoiser: the streaming yardstick
    x = torch.randn((M, CH), device=DEV)
    gam, bet = torch.ones(CH, device=DEV), torch.zeros(CH, device=DEV)
    y = torch.empty((M, CH), dtype=torch.float16, device=DEV)
    cases = [
        ("pnc_u8_to_tokens_f16 (hi plane)", lambda: hip.u8_to_tokens_f16(src, lut, F, H * W, C, CP, hi), ROWS * (C + 2 * CP)),
        ("pnc_u8_to_tokens_f16 (hi + lo)", lambda: hip.u8_to_tokens_f16(src, lut, F, H * W, C, CP, hi, lo), ROWS * (C + 4 * CP)),
        ("pnc_nchw_to_tokens_f16 (hi plane, the float entry)", lambda: hip.nchw_to_tokens_f16(f32, C, None, 0, F, H * W, CP, hi),
         ROWS * (4 * C + 2 * CP)),
        ("pnc_tokens_to_u8", lambda: hip.tokens_to_u8(tok, 3, ROWS, 3, out), ROWS * 3 * 5),
        ("pnc_tokens_to_nchw_f32 (the float exit)", lambda: hip.tokens_to_nchw_f32(tok, 3, F, H * W, 3, nchw), ROWS * 3 * 8),
        ("pnc_layernorm 196608 x 320", lambda: hip.layernorm(x, CH, M, CH, gam, bet, 1e-5, y, CH), M * CH * 6),
    ]
    for rnd in range(a.reps):
        for name, fn, nbytes in cases:
            us = events(fn)
            emit(kernel=name, round=rnd, us=round(us, 2), gbps=round(nbytes / us * 1e-3, 1), bytes=nbytes)


if a.legs:
    legs()
if a.kernels:
    kernels()
