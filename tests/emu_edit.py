"""tests/emu.py plus the one wrapper clip editing adds: `frames_renoise` with panacea_amd/hip.py's signature, evaluated by the
per-op reference of tests/clip_edit_ref.py.  Installed as the backend the way the CPU tests install `emu`
(`engine.use_backend(emu_edit)`); `CALLS` counts the launches, one (kept frames, sigma is 0 somewhere) entry each."""
import torch

import clip_edit_ref as ref
import emu

globals().update({k: v for k, v in vars(emu).items() if not k.startswith("__")})

CALLS = []


def frames_renoise(z, noise, sigma, out, keep=None, x=None):
    planes = [z, noise, out] + ([] if x is None else [x])
    if any(t.shape != z.shape or t.dtype != torch.float32 or not t.is_contiguous() for t in planes):
        raise emu.PncError("frames_renoise: z, noise, out and x are contiguous fp32 latents of one shape")
    if any(t is not None and (t.shape != (z.shape[0],) or t.dtype != torch.float32) for t in (sigma, keep)):
        raise emu.PncError("frames_renoise: sigma and keep are [T] fp32 vectors")
    if keep is not None and x is None:
        raise emu.PncError("frames_renoise: frames that are not kept come from `x`")
    CALLS.append((None if keep is None else tuple(int(k > 0) for k in keep.tolist()), bool((sigma == 0).any())))
    T = z.shape[0]
    res = ref.frames_renoise(z.reshape(T, z.shape[1], -1), noise.reshape(T, z.shape[1], -1), sigma, keep,
                             None if x is None else x.reshape(T, z.shape[1], -1).clone())
    out.copy_(res.view(z.shape))
