#!/usr/bin/env python
"""Golden vector of the reference's `tiny` network on weights that are NOT fp16-representable (needs the reference tree next to the
checkout; CPU only):

  tests/golden/tiny_w32.npz

The weights are the deterministic synthetic set WITHOUT its final fp16 rounding (synth.synth_state_dict(..., round_fp16=False)):
plain fp32 values, as an fp32 checkpoint holds them.  The reference network runs its own fp32 forward
(`OpenAIWrapperControlLDM3D.forward`) on synth.synth_inputs of the `tiny` shape; the whole eps is stored.  The same run on the weights rounded to fp16 is printed next to
it — the difference is the weight-rounding term that the `precise-full` operand policy removes.  The oracle (oracle/panacea_oracle.py) must agree with the reference run to 2e-5 before anything is
written.  Only data is written.

    python tools/gen_golden_w32.py
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

SALT = 0


def main():
    kw = configs.get("tiny")
    B, T, h, w = configs.SHAPES["tiny"]
    ns = ref_import.import_reference()
    net, wrapper = ref_import.build_reference_network(ns, kw)
    manifest = {k: list(v.shape) for k, v in net.state_dict().items()}
    inp = synth.synth_inputs(B, T, h, w, context_dim=kw["context_dim"])
    out = {}
    for key, rnd in (("eps", False), ("eps_w16", True)):
        sd = synth.synth_state_dict(manifest, salt=SALT, round_fp16=rnd)
        net.load_state_dict(sd, strict=True)
        c = {k: inp[k].clone() for k in ("concat", "crossattn", "cond_feat")}
        with torch.no_grad():
            eps = wrapper(inp["x"].clone(), inp["t"].clone(), c)
        eps_o = po.wrapper_forward(sd, oracle_cfg(kw), inp["x"], inp["t"], {k: inp[k] for k in ("concat", "crossattn", "cond_feat")})
        d = (eps - eps_o).abs().max().item()
        print(f"[tiny, {'fp16-rounded' if rnd else 'unrounded'} weights] eps rms {eps.pow(2).mean().sqrt():.4f} max {eps.abs().max():.4f}; "
              f"oracle vs reference max-abs {d:.3e}")
        assert d <= 2e-5, "oracle disagrees with the reference"
        out[key] = eps.numpy()
    dw = np.abs(out["eps"] - out.pop("eps_w16"))
    print(f"weight-rounding term: eps max-abs {dw.max():.3e} mean-abs {dw.mean():.3e}")
    out["salt"] = np.int32(SALT)
    path = GOLDEN / "tiny_w32.npz"
    np.savez_compressed(path, **out)
    assert path.stat().st_size < (1 << 20), path.stat().st_size
    print(f"wrote {path.name}: {path.stat().st_size} bytes")


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
