#!/usr/bin/env python
"""Golden vectors of the reference's first stage on weights that are NOT fp16-representable (needs the reference tree next to the
checkout; CPU only):

  tests/golden/vae_tiny_w32.npz

The reference's own `Decoder` + post_quant_conv and `Encoder` + quant_conv (sgm/modules/diffusionmodules/model.py, the TINY config of
tests/test_vae.py: mid block of 128 channels) run their fp32 forward on the deterministic synthetic weights WITHOUT the final fp16
rounding (synth.synth_state_dict(manifest, salt=SALT, round_fp16=False): plain fp32 values, as an fp32 checkpoint holds them; the file
stores the salt, not the tensors) and on the inputs of the existing tiny goldens (the z of vae_tiny.npz, the image of vae_enc_tiny.npz).
Next to the reference's outputs the file holds "truth" — oracle/vae_oracle.py evaluated in float64 on the same weights — and
e32 = max|reference fp32 - truth| per output: the fp32 forward's own distance from the exact result, the unit of the bound of
tests/test_first_stage_precision*.py.  Only data is written.

    python tools/gen_golden_vae_w32.py
"""
from __future__ import annotations

import contextlib
import importlib
import io
import json
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from oracle import ref_import, vae_oracle as vo       # noqa: E402
from oracle.gen_golden_vae import TINY                # noqa: E402
from panacea_amd import synth                         # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
SALT = 0
CFG = dict(ch=64, ch_mult=[1, 2], num_res_blocks=1)


def _sub(sd, prefix):
    return {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}


def main():
    ref_import.import_reference()
    with contextlib.redirect_stdout(io.StringIO()):
        mdl = importlib.import_module("sgm.modules.diffusionmodules.model")
        dec, enc = mdl.Decoder(**TINY).eval(), mdl.Encoder(**TINY).eval()
    pq, qc = torch.nn.Conv2d(4, 4, 1), torch.nn.Conv2d(8, 8, 1)          # AutoencoderKL.post_quant_conv / quant_conv
    dman = json.loads((GOLDEN / "manifest_vae_tiny.json").read_text())
    eman = json.loads((GOLDEN / "manifest_vae_enc_tiny.json").read_text())
    dsd = synth.synth_state_dict(dman, salt=SALT, round_fp16=False)
    esd = synth.synth_state_dict(eman, salt=SALT, round_fp16=False)
    assert any(not torch.equal(v, v.half().float()) for v in dsd.values()), "the weights are fp16-representable"
    dec.load_state_dict(_sub(dsd, "decoder."), strict=True)
    pq.load_state_dict(_sub(dsd, "post_quant_conv."), strict=True)
    enc.load_state_dict(_sub(esd, "encoder."), strict=True)
    qc.load_state_dict(_sub(esd, "quant_conv."), strict=True)
    z = torch.from_numpy(np.load(GOLDEN / "vae_tiny.npz")["z"])
    x = torch.from_numpy(np.load(GOLDEN / "vae_enc_tiny.npz")["x"])
    with torch.no_grad():
        img32, mom32 = dec(pq(z)), qc(enc(x))
        img64 = vo.decode({k: v.double() for k, v in dsd.items()}, vo.VaeConfig(**CFG), z.double())
        mom64 = vo.encode_moments({k: v.double() for k, v in esd.items()}, vo.VaeConfig(**CFG), x.double())
    assert img64.dtype == torch.float64 and mom64.dtype == torch.float64
    e_img, e_mom = (img32.double() - img64).abs().max().item(), (mom32.double() - mom64).abs().max().item()
    print(f"decoder {tuple(img32.shape)} |img| max {img32.abs().max():.3f}: e32 = max|reference fp32 - float64 oracle| = {e_img:.3e}")
    print(f"encoder {tuple(mom32.shape)} |moments| max {mom32.abs().max():.3f}: e32 = {e_mom:.3e}")
    assert e_img < 1e-4 and e_mom < 1e-4, "the oracle disagrees with the reference"
    path = GOLDEN / "vae_tiny_w32.npz"
    np.savez_compressed(path, z=z.numpy(), x=x.numpy(), img_ref32=img32.numpy(), moments_ref32=mom32.numpy(), img_truth=img64.numpy(),
                        moments_truth=mom64.numpy(), e32_img=np.float64(e_img), e32_moments=np.float64(e_mom), salt=np.int32(SALT))
    assert path.stat().st_size < (1 << 20), path.stat().st_size
    print(f"wrote {path.name}: {path.stat().st_size} bytes")


if __name__ == "__main__":
    torch.manual_seed(0)
    main()
