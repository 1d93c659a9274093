#!/usr/bin/env python
"""Generate tests/golden/rollout_tiny.npz: two windows of a rollout as the REFERENCE's own classes compute them (build container
only; the reference is imported through oracle/ref_import.py, runs on the CPU, and only data is written).

    python tools/gen_golden_rollout.py

For each `use_last_frame` setting (the anchor in the last / the first slot), T = 3 frames per window:

  * the tiny first stage, built as oracle/gen_golden_vae.py builds it: the reference's Encoder / Decoder (diffusionmodules/model.py)
    with a quant_conv / post_quant_conv and the synthetic weights of tests/golden/manifest_vae_enc_tiny.json / manifest_vae_tiny.json;
  * the dense float `final_cond_zero` clip, built with the statements of nuscenes_datasets_video.py:552,559-566 from the anchor's
    bytes, through the reference's VAEEmbedder (encoders/modules.py:1016-1058) -> `concat`; the posterior MEAN stands in for the
    sample, so the file does not depend on a random stream (the draw order is tested on the CPU, tests/test_rollout.py);
  * the tiny network at num_frames = 3 with synthetic weights under EulerEDMSampler(2) + VanillaCFG(5) + DiscreteDenoiser from the
    `share_noise_level` start of DiffusionEngine3D.sample (diffusion.py:242-249);
  * decode_first_stage (diffusion.py:138-143) and the quantisation of inference.py:189-193 -> bytes; the frame at the far end from
    the anchor is the next window's anchor.

Stored: the anchor bytes, the windows' layouts (uint8 channels-last, blocks of 8 x 8 pixels), contexts and noises, and per anchor
setting the encoder moments and posterior-mean `concat` of both windows' dense clips, the final latents z_k, and every window's
far-end frame bytes."""
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
from oracle import gen_golden_conditioner, ref_import      # noqa: E402
from panacea_amd import configs, synth                     # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
P = "sgm.modules.diffusionmodules."
VAE = dict(double_z=True, z_channels=4, resolution=16, in_channels=3, out_ch=3, ch=64, ch_mult=[1, 2], num_res_blocks=1,
           attn_resolutions=[], dropout=0.0)
T, WINDOWS, STEPS, CFG_SCALE, SCALE_FACTOR, SHARE_NOISE_LEVEL = 3, 2, 2, 5.0, 0.18215, 0.07
N = T + (WINDOWS - 1) * (T - 1)                            # frames of the video
HINT_BLOCK = 8                                             # the synthetic layout is constant over blocks of 8 x 8 pixels


def _load(module, manifest, prefix):
    sd = synth.synth_state_dict(json.loads((GOLDEN / manifest).read_text()))
    module.load_state_dict({k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}, strict=True)
    return module.eval()


class TinyFirstStage(torch.nn.Module):
    """AutoencoderKL's encode / decode (autoencoder.py:333-368) around the reference's Encoder / Decoder; `encode` gives the
    posterior's mode"""

    def __init__(self, mdl, dist):
        super().__init__()
        with contextlib.redirect_stdout(io.StringIO()):
            self.encoder = _load(mdl.Encoder(**VAE), "manifest_vae_enc_tiny.json", "encoder.")
            self.decoder = _load(mdl.Decoder(**VAE), "manifest_vae_tiny.json", "decoder.")
        self.quant_conv = _load(torch.nn.Conv2d(8, 8, 1), "manifest_vae_enc_tiny.json", "quant_conv.")
        self.post_quant_conv = _load(torch.nn.Conv2d(4, 4, 1), "manifest_vae_tiny.json", "post_quant_conv.")
        self.dist = dist

    def moments(self, x):
        return self.quant_conv(self.encoder(x))

    def encode(self, x):
        return self.dist.DiagonalGaussianDistribution(self.moments(x)).mode()

    def decode(self, z):
        return self.decoder(self.post_quant_conv(z))


def final_cond_zero(anchor_u8: np.ndarray, use_last_frame: bool) -> np.ndarray:
    """the dense float clip the dataset hands out as `final_cond_zero` (nuscenes_datasets_video.py:552,559-566) when the anchor frame
    has the bytes `anchor_u8` (H, W, 3): float32 zeros, the anchor scaled byte / 127.5 - 1 in the last or the first slot; (T, 3, H, W)"""
    clip = np.zeros((T, 3) + anchor_u8.shape[:2], dtype=np.float32)
    clip[T - 1 if use_last_frame else 0] = anchor_u8.transpose(2, 0, 1).astype(np.float32) / 127.5 - 1.0
    return clip


def to_bytes(frames: torch.Tensor) -> np.ndarray:
    """inference.py:188-199 on (T, 3, H, W) frames -> (T, H, W, 3) uint8"""
    x = torch.clamp(frames.detach().float().cpu(), -1.0, 1.0)
    x = (x + 1.0) / 2.0
    return (x.permute(0, 2, 3, 1).numpy() * 255).astype(np.uint8)


def window_frames(k: int, use_last_frame: bool) -> slice:
    """the frames of the video that window k covers: windows overlap by one frame, and with the anchor in the last slot window
    k + 1 lies before window k"""
    first = (WINDOWS - 1 - k) * (T - 1) if use_last_frame else k * (T - 1)
    return slice(first, first + T)


def main():
    ns = ref_import.import_reference()
    enc_modules = gen_golden_conditioner.import_conditioner()
    for m in ("guiders", "discretizer", "denoiser_scaling", "denoiser_weighting", "sampling_utils"):
        importlib.import_module(P + m)
    mdl = importlib.import_module(P + "model")
    dist = importlib.import_module("sgm.modules.distributions.distributions")
    fs = TinyFirstStage(mdl, dist)
    emb = enc_modules.VAEEmbedder()
    emb.first_stage_model, emb.disable_first_stage_autocast, emb.scale_factor = fs, True, SCALE_FACTOR      # diffusion.py:114-124
    emb.freeze()

    kw = configs.with_frames(configs.get("tiny"), T)
    net, wrapper = ref_import.build_reference_network(ns, kw)
    manifest = json.loads((GOLDEN / "manifest_tiny.json").read_text())
    assert {k: list(v.shape) for k, v in net.state_dict().items()} == manifest, "the tiny manifest does not fit num_frames = 3"
    net.load_state_dict(synth.synth_state_dict(manifest), strict=True)
    disc = {"target": P + "discretizer.LegacyDDPMDiscretization"}
    den = ns.dn.DiscreteDenoiser(weighting_config={"target": P + "denoiser_weighting.EpsWeighting"},
                                 scaling_config={"target": P + "denoiser_scaling.EpsScaling"}, num_idx=1000, discretization_config=disc)
    smp = ns.sp.EulerEDMSampler(num_steps=STEPS, discretization_config=disc, device="cpu",
                                guider_config={"target": P + "guiders.VanillaCFG", "params": {"scale": CFG_SCALE}})

    _, _, h, w = configs.SHAPES["tiny"]
    H, W = 2 * h, 2 * w                                    # the tiny first stage halves the resolution once
    rng = np.random.default_rng(20)
    anchor = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    coarse = rng.integers(0, 256, (N, 8 * h // HINT_BLOCK, 8 * w // HINT_BLOCK, 19), dtype=np.uint8)
    layout = coarse.repeat(HINT_BLOCK, axis=1).repeat(HINT_BLOCK, axis=2)                  # (N, 8h, 8w, 19), one per video frame
    g = torch.Generator().manual_seed(21)
    noise = torch.randn(WINDOWS, T, 4, h, w, generator=g)
    ctx_c, ctx_uc = torch.randn(WINDOWS, 1, 77, kw["context_dim"], generator=g), torch.randn(1, 77, kw["context_dim"], generator=g)
    out = dict(anchor=anchor, layout=layout, noise=noise.numpy(), crossattn_c=ctx_c.numpy(), crossattn_uc=ctx_uc.numpy(),
               steps=np.int32(STEPS), cfg_scale=np.float32(CFG_SCALE), scale_factor=np.float32(SCALE_FACTOR),
               share_noise_level=np.float32(SHARE_NOISE_LEVEL))

    for use_last_frame, tag in ((True, "last"), (False, "first")):
        frame = anchor
        for k in range(WINDOWS):
            clip = torch.from_numpy(final_cond_zero(frame, use_last_frame))
            with torch.no_grad():
                moments = fs.moments(clip)
                concat = emb(clip)
                assert torch.equal(concat, SCALE_FACTOR * moments[:, :4])
                # the dataset's scaling of the layout (nuscenes_datasets_video.py:551), (t h w c -> t c h w)
                hint = torch.from_numpy(layout[window_frames(k, use_last_frame)].transpose(0, 3, 1, 2).astype(np.float32) / 255.0)
                c = {"crossattn": ctx_c[k], "concat": concat, "cond_feat": hint}
                uc = {"crossattn": ctx_uc, "concat": concat.clone(), "cond_feat": hint}
                randn = noise[k] + concat[-1].unsqueeze(0).expand(T, -1, -1, -1) * SHARE_NOISE_LEVEL          # diffusion.py:242-249
                z = smp(lambda inp, sigma, cc: den(wrapper, inp, sigma, cc), randn, c, uc)
                frames = to_bytes(fs.decode(1.0 / SCALE_FACTOR * z))
            frame = frames[0 if use_last_frame else -1]
            out.update({f"{tag}.moments{k}": moments.numpy(), f"{tag}.concat{k}": concat.numpy(), f"{tag}.z{k}": z.numpy(),
                        f"{tag}.far{k}": frame})
            print(f"{tag} window {k}: |moments| max {moments.abs().max():.3f}  |concat| max {concat.abs().max():.3f}  "
                  f"|z| max {z.abs().max():.3f}  far frame bytes {frame.min()} .. {frame.max()} (mean {frame.mean():.1f})")
    path = GOLDEN / "rollout_tiny.npz"
    np.savez_compressed(path, **out)
    print(f"written {path.relative_to(ROOT)}: {path.stat().st_size} bytes")
    assert path.stat().st_size < 1 << 20


if __name__ == "__main__":
    main()
