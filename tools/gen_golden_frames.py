#!/usr/bin/env python
"""Golden vectors of the reference's `tiny` network at 12 and 16 frames (needs the reference tree next to the checkout; CPU only):

  tests/golden/tiny_t12.npz, tests/golden/tiny_t16.npz

The reference network is built with `num_frames` = T (its sinusoidal temporal position table is computed, not stored: the state
dict is the one of manifest_tiny.json), loaded with the deterministic synthetic weights (panacea_amd/synth.py) and run through
`OpenAIWrapperControlLDM3D.forward` on synth.synth_inputs(2, T, 8, 96).  Stored like oracle/gen_golden.py::run_config stores a
configuration — eps whole, a fixed-stride sample of the flattened ControlNet residuals and of every top-level block output — but
with a stride PER TENSOR in the place of 7: the twenty traced tensors hold 18 M / 24 M values at 12 / 16 frames, and a stride-7
sample of them is 10 / 13 MB where a committed fixture has to stay below 1 MiB.  Every tensor contributes about SAMPLES values: its
stride is the smallest prime >= numel / SAMPLES (43 .. 457: the small tensors are sampled more densely), stored as `stride.<key>`.
The oracle (oracle/panacea_oracle.py) must agree with the same run to 2e-5 before anything is written.  Only data is written.

    python tools/gen_golden_frames.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import panacea_oracle as po            # noqa: E402
from oracle import ref_import                      # noqa: E402
from oracle.gen_golden import GOLDEN, oracle_cfg   # noqa: E402
from panacea_amd import configs, synth             # noqa: E402

FRAMES = (12, 16)
SAMPLES = 7000              # values kept per traced tensor (see above)
SHAPE = (2, 8, 96)          # CFG batch, latent height, latent width (6 views of 16): the `tiny` shape of configs.SHAPES


def stride_for(numel: int) -> int:
    n = max(2, -(-numel // SAMPLES))
    while any(n % d == 0 for d in range(2, int(n ** 0.5) + 1)):
        n += 1
    return n


def run_frames(ns, T: int):
    kw = configs.with_frames(configs.get("tiny"), T)
    B, h, w = SHAPE
    net, wrapper = ref_import.build_reference_network(ns, kw)
    manifest = {k: list(v.shape) for k, v in net.state_dict().items()}
    sd = synth.synth_state_dict(manifest)
    net.load_state_dict(sd, strict=True)
    inp = synth.synth_inputs(B, T, h, w, context_dim=kw["context_dim"])

    trace = {}

    def hook(prefix):
        def fn(_m, _i, out):
            trace[prefix] = out.detach().clone()
        return fn
    for i, m in enumerate(net.input_blocks):
        m.register_forward_hook(hook(f"input_blocks.{i}"))
    net.middle_block.register_forward_hook(hook("middle_block"))
    for i, m in enumerate(net.output_blocks):
        m.register_forward_hook(hook(f"output_blocks.{i}"))
    for i, m in enumerate(net.controlnet.input_blocks):
        m.register_forward_hook(hook(f"controlnet.input_blocks.{i}"))
    net.controlnet.middle_block.register_forward_hook(hook("controlnet.middle_block"))
    net.controlnet.input_hint_block.register_forward_hook(hook("controlnet.input_hint_block"))
    controls = {}

    def cn_hook(_m, _i, out):
        for j, c in enumerate(out):
            controls[f"control.{j}"] = c.detach().clone()
    net.controlnet.register_forward_hook(cn_hook)

    c = {k: inp[k].clone() for k in ("concat", "crossattn", "cond_feat")}
    with torch.no_grad():
        eps = wrapper(inp["x"].clone(), inp["t"].clone(), c)

    po.TRACE = {}
    eps_o = po.wrapper_forward(sd, oracle_cfg(kw), inp["x"], inp["t"], {k: inp[k] for k in ("concat", "crossattn", "cond_feat")})
    otrace, po.TRACE = po.TRACE, None
    d = (eps - eps_o).abs().max().item()
    print(f"[tiny, T={T}] eps rms {eps.pow(2).mean().sqrt():.4f} max {eps.abs().max():.4f}; oracle vs reference max-abs {d:.3e}")
    assert d <= 2e-5, "oracle disagrees with the reference"
    for k, v in trace.items():
        if k == "controlnet.input_hint_block":
            continue
        dk = (v - otrace[k]).abs().max().item()
        assert dk <= 5e-5 * max(1.0, v.abs().max().item()), (k, dk)

    out = {"eps": eps.numpy()}
    for k, v in list(controls.items()) + [("block." + k, v) for k, v in trace.items()]:
        st = stride_for(v.numel())
        out[k] = v.reshape(-1)[::st].numpy()
        out["stride." + k] = np.int32(st)
    path = GOLDEN / f"tiny_t{T}.npz"
    np.savez_compressed(path, **out)
    assert path.stat().st_size < (1 << 20), path.stat().st_size
    print(f"[tiny, T={T}] wrote {len(out)} arrays, {path.stat().st_size} bytes; {len(manifest)} tensors in the state dict")


if __name__ == "__main__":
    torch.manual_seed(0)
    ns = ref_import.import_reference()
    for T in FRAMES:
        run_frames(ns, T)
