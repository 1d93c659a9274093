"""tests/emu_edit.py plus the three wrappers region editing adds: `latent_renoise_masked`, `mask_pool_u8` and `u8_select` with
panacea_amd/hip.py's signatures, evaluated by the per-op references of tests/region_edit_ref.py.  Installed as the backend the way
the CPU tests install `emu` (`engine.use_backend(emu_region)`).  `CALLS` is emu_edit's list, so one list holds the launches of a
run in order: emu_edit's (kept frames, sigma is 0 somewhere) entry per `frames_renoise`, and a (name, ...) entry per launch here."""
import torch

import emu
import emu_edit
import region_edit_ref as rref

globals().update({k: v for k, v in vars(emu_edit).items() if not k.startswith("__")})

CALLS = emu_edit.CALLS


def latent_renoise_masked(z, noise, sigma, mask, x, out):
    T = z.shape[0]
    if any(t.shape != z.shape or t.dtype != torch.float32 or not t.is_contiguous() for t in (z, noise, x, out)):
        raise emu.PncError("latent_renoise_masked: z, noise, x and out are contiguous fp32 latents of one shape")
    if sigma.shape != (T,) or sigma.dtype != torch.float32:
        raise emu.PncError("latent_renoise_masked: sigma is a [T] fp32 vector")
    if mask.shape != (T,) + tuple(z.shape[2:]) or mask.dtype != torch.float32 or not mask.is_contiguous():
        raise emu.PncError("latent_renoise_masked: mask is a contiguous fp32 selector of a frame's pixels")
    CALLS.append(("latent_renoise_masked", out is x, bool((sigma == 0).any())))
    C = z.shape[1]
    res = rref.latent_renoise_masked(z.reshape(T, C, -1), noise.reshape(T, C, -1), sigma, mask.reshape(T, -1), x.reshape(T, C, -1).clone())
    out.copy_(res.view(z.shape))


def mask_pool_u8(mask_u8, f, out):
    if mask_u8.dim() != 3 or mask_u8.dtype != torch.uint8 or not mask_u8.is_contiguous():
        raise emu.PncError("mask_pool_u8: mask_u8 is a contiguous (T, H, W) byte mask")
    T, H, W = mask_u8.shape
    if isinstance(f, bool) or not isinstance(f, int) or not 1 <= f <= 16 or H % f or W % f:
        raise emu.PncError("mask_pool_u8: f is an int in 1 .. 16 that divides H and W")
    if out.shape != (T, H // f, W // f) or out.dtype != torch.float32 or not out.is_contiguous():
        raise emu.PncError("mask_pool_u8: out is a contiguous (T, H / f, W / f) fp32 selector")
    CALLS.append(("mask_pool_u8", f))
    out.copy_(rref.mask_pool_u8(mask_u8, f))


def u8_select(src, gen, mask_u8, out):
    if any(t.shape != src.shape or t.dtype != torch.uint8 or not t.is_contiguous() for t in (src, gen, out)):
        raise emu.PncError("u8_select: src, gen and out are contiguous uint8 frames of one shape")
    if src.dim() < 2 or not 1 <= src.shape[-1] <= 4 or out is src:
        raise emu.PncError("u8_select: channels-last frames of 1 .. 4 channels, out is not src")
    if mask_u8.shape != src.shape[:-1] or mask_u8.dtype != torch.uint8 or not mask_u8.is_contiguous():
        raise emu.PncError("u8_select: mask_u8 is the frames' contiguous byte mask")
    CALLS.append(("u8_select", src.shape[-1]))
    C = src.shape[-1]
    out.copy_(rref.u8_select(src.reshape(-1, C), gen.reshape(-1, C).clone(), mask_u8.reshape(-1)).view(src.shape))
