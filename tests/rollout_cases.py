"""What tests/test_rollout.py (emulated backend) and tests/test_rollout_gpu.py (MI355X) share: the tiny rollout pipeline at
T = 3 frames, synthetic windows that overlap by one frame, a recorder around the first stage, and the checks against
tests/golden/rollout_tiny.npz with the bounds the suite already holds the two stages to."""
import numpy as np
import torch

import image_boundary_cases as ib
import test_vae as tv
from helpers import GOLDEN, measured, product_network
from panacea_amd import configs, pipeline
from panacea_amd.image import SparseClip
from panacea_amd.nn import model

T = 3
_, _, LH, LW = configs.SHAPES["tiny"]            # the latent
H, W = 2 * LH, 2 * LW                            # frames of the tiny first stage (one Downsample)
G = np.load(GOLDEN / "rollout_tiny.npz")
ENC_MAX, ENC_MEAN = 8e-3, 1e-3                   # tests/test_vae.py, first-stage encoder against vae_enc_tiny.npz: max-abs, mean-abs
Z_TOL = float(np.load(GOLDEN / "sampler_tiny_net.npz")["tol_rel"])       # tests/test_sampler_acceptance.py: max-abs / max|x_ref|


def tiny_encoder(device):
    _, sd, _ = tv._tiny_enc()
    fe = model.FirstStageEncoder(4, tv.TINY)
    fe.load_state_dict(sd, strict=True)
    return fe.to(device)


def tiny_rollout_pipeline(device, enc=None):
    """the tiny network at num_frames = 3 and the tiny first stage, synthetic weights (those of the golden file)"""
    net, _, kw = product_network("tiny", device, kw=configs.with_frames(configs.get("tiny"), T))
    _, sd, _ = tv._tiny()
    dec = model.FirstStageDecoder(4, tv.TINY)
    dec.load_state_dict(sd, strict=True)
    return dict(net=net, dec=dec.to(device), enc=enc if enc is not None else tiny_encoder(device), kw=kw)


def frames_u8(K, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 256, (K, H, W, 3), dtype=np.uint8))


def dense_clip(u8: torch.Tensor, slots, num_frames=T) -> torch.Tensor:
    """the float NCHW clip a SparseClip stands for: zeros, frame j scaled byte / 127.5 - 1 at slots[j]"""
    clip = torch.zeros((num_frames, 3) + tuple(u8.shape[1:3]))
    for j, s in enumerate(slots):
        clip[s] = torch.from_numpy(ib.scaled_nchw(u8[j:j + 1].cpu().numpy(), "image"))[0]
    return clip.to(u8.device)


def window_frames(k, n_windows, anchor):
    first = (n_windows - 1 - k) * (T - 1) if anchor == "last" else k * (T - 1)
    return slice(first, first + T)


def _windows(layout_u8: np.ndarray, ctx_c, ctx_uc, n_windows, anchor, hint, device):
    """(cond, uc) per window from one layout per video frame ((N, 8h, 8w, 19) bytes) and one context per window"""
    out = []
    for k in range(n_windows):
        lay = torch.from_numpy(np.ascontiguousarray(layout_u8[window_frames(k, n_windows, anchor)]))
        if hint == "float":
            lay = torch.from_numpy(ib.scaled_nchw(lay.numpy(), "layout"))
        lay = lay.to(device)
        out.append(({"crossattn": ctx_c[k].to(device), "cond_feat": lay}, {"crossattn": ctx_uc.to(device), "cond_feat": lay}))
    return out


SMALL = (LH // 2, LW // 2)                      # the smallest latent the tiny network takes: 6 views of 4 x 8, 2 x 4 after its Downsample


def rollout_inputs(n_windows, anchor, hint, device="cpu", seed=40, latent=(LH, LW)):
    """synthetic rollout inputs: an anchor frame, `n_windows` windows whose layouts overlap by one frame, the noises"""
    N = T + (n_windows - 1) * (T - 1)
    lh, lw = latent
    rng = np.random.default_rng(seed)
    a = torch.from_numpy(rng.integers(0, 256, (2 * lh, 2 * lw, 3), dtype=np.uint8)).to(device)
    layout = rng.integers(0, 256, (N, lh, lw, 19), dtype=np.uint8).repeat(8, axis=1).repeat(8, axis=2)
    g = torch.Generator().manual_seed(seed)
    kw = configs.get("tiny")
    noise = torch.randn(n_windows, T, 4, lh, lw, generator=g).to(device)
    ctx_c, ctx_uc = torch.randn(n_windows, 1, 77, kw["context_dim"], generator=g), torch.randn(1, 77, kw["context_dim"], generator=g)
    return dict(anchor=a, noise=noise, windows=_windows(layout, ctx_c, ctx_uc, n_windows, anchor, hint, device))


class Recorder:
    """stands in for both first stages of rollout_frames: records every SparseClip encoded with its result, every latent decoded
    (as the sampler left it: times scale_factor) and the frames it became"""

    def __init__(self, dec, enc, scale_factor=pipeline.SCALE_FACTOR):
        self.dec, self.enc, self.scale_factor = dec, enc, scale_factor
        self.clips, self.encoded, self.latents, self.decoded = [], [], [], []

    def encode_sparse_u8(self, clip, **kw):
        z = self.enc.encode_sparse_u8(clip, **kw)
        self.clips.append(clip)
        self.encoded.append(z)
        return z

    def decode_u8(self, z):
        frames = self.dec.decode_u8(z)
        self.latents.append(z * self.scale_factor)
        self.decoded.append(frames)
        return frames


# ---- against the reference's rollout (tests/golden/rollout_tiny.npz) ------------------------------------------------------------
def golden_anchor(tag, k, device):
    """window k's anchor in the reference's rollout: the given frame, then the far-end frame window k - 1 decoded to"""
    return torch.from_numpy(G["anchor"] if k == 0 else G[f"{tag}.far{k - 1}"]).to(device)


def check_moments_and_concat(enc, device, tag, k, where):
    clip = SparseClip(golden_anchor(tag, k, device)[None], [-1 if tag == "last" else 0], T)
    mom = enc.moments_sparse_u8(clip).cpu()
    concat = (float(G["scale_factor"]) * enc.encode_sparse_u8(clip, sample=False)).cpu()
    dm = (mom - torch.from_numpy(G[f"{tag}.moments{k}"])).abs()
    dc = (concat - torch.from_numpy(G[f"{tag}.concat{k}"])).abs()
    print(f"rollout golden, {where}, {tag} window {k}: moments max-abs {dm.max().item():.3e} mean-abs {dm.mean().item():.3e}; "
          f"concat max-abs {dc.max().item():.3e} mean-abs {dc.mean().item():.3e}")
    measured(f"rollout_encode_{where}_{tag}{k}", mom_max=dm.max().item(), mom_mean=dm.mean().item(), concat_max=dc.max().item(),
             concat_mean=dc.mean().item())
    assert mom.shape == dm.shape == (T, 8, LH, LW) and dm.max().item() < ENC_MAX and dm.mean().item() < ENC_MEAN
    assert dc.max().item() < ENC_MAX and dc.mean().item() < ENC_MEAN
    return dm.max().item(), dc.max().item()


def check_window_latent(pipe, device, tag, k, where):
    """window k of the reference's rollout, run as a one-window rollout from the reference's own anchor for it -> z_k"""
    n = int(G["noise"].shape[0])
    c = torch.from_numpy(G["crossattn_c"]).to(device)
    windows = _windows(G["layout"], c, torch.from_numpy(G["crossattn_uc"]), n, tag, "uint8", device)
    rec = Recorder(pipe["dec"], pipe["enc"], float(G["scale_factor"]))
    frames = pipeline.rollout_frames(pipe["net"], rec, rec, golden_anchor(tag, k, device), windows[k:k + 1],
                                     torch.from_numpy(G["noise"][k:k + 1]).to(device), anchor=tag, sample_posterior=False,
                                     share_noise_level=float(G["share_noise_level"]), num_steps=int(G["steps"]),
                                     cfg_scale=float(G["cfg_scale"]), scale_factor=float(G["scale_factor"]))
    ref = torch.from_numpy(G[f"{tag}.z{k}"])
    z = rec.latents[0].float().cpu()
    err = ((z - ref).abs().max() / ref.abs().max()).item()
    far = frames[0 if tag == "last" else -1].cpu().numpy().astype(np.int32)
    byte_diff = np.abs(far - G[f"{tag}.far{k}"].astype(np.int32))
    print(f"rollout golden, {where}, {tag}: z_{k} max-abs / max|z_ref| {err:.3e} (bound {Z_TOL:.1e}); far frame: "
          f"{(byte_diff > 0).mean() * 100:.2f} % of the bytes differ, by at most {byte_diff.max()}")
    measured(f"rollout_z_{where}_{tag}{k}", err_rel=err, bytes_differ=float((byte_diff > 0).mean()), byte_max=int(byte_diff.max()))
    assert z.shape == ref.shape and err <= Z_TOL, (tag, k, err)
    return err
