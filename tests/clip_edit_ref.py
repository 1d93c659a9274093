"""Per-op fp32 reference of pnc_frames_renoise, written from its comment block in include/panacea_hip.h alone: it imports neither
tests/emu.py nor panacea_amd.sampling.

`frames_renoise` evaluates one launch with torch fp32 CPU tensors, ONE elementwise torch op per rounding, in the header's order: the
product noise * sigma rounded to fp32, then the sum with z.  A frame whose sigma is 0 is z's bits (the noise is not read: -0.0 stays
-0.0, NaN noise is inert), a frame that is not kept is x's bits.  Operands are [T][C][Npix] planes and [T] vectors; `out == x` needs no
case of its own here — a frame that is not touched holds x's bits, which is what a copy of x holds.

`mutant=NAME` is a WRONG kernel, the reference with one deviation (MUTANTS).  tests/test_clip_edit.py shows that each of them leaves
the reference's bits on the case list below, and a failing GPU comparison names the mutant, if any, whose bits the kernel has.

The case list (SHAPES x VARIANTS) is the one tests/test_clip_edit_gpu.py launches."""
import torch

MUTANTS = {
    "fma": "z + noise * sigma contracted into one rounding (float64, then rounded)",
    "keep_nonzero": "a frame kept where keep != 0 instead of keep > 0: negative and NaN selectors keep",
}

# (T, C, Npix): scalar-only frames; whole float4s; more than one frame off a multiple of 1024; Npix % 4 != 0 (planes 1 and 3 of every
# frame start off a 16-byte boundary); 16 frames of three slices; two slices-of-1024 x 24 per frame
SHAPES = [(1, 4, 7), (2, 4, 96), (3, 4, 100), (3, 4, 98), (16, 4, 768), (2, 8, 3072)]
VARIANTS = ["keep_null", "selector", "sigma_zero", "out_is_x", "nan_noise"]
NAN = float("nan")


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def frames_renoise(z, noise, sigma, keep=None, x=None, mutant=None) -> torch.Tensor:
    """-> out [T, C, Npix] fp32.  keep None: every frame is kept (x may be None then)"""
    assert mutant is None or mutant in MUTANTS
    T = z.shape[0]
    out = torch.empty_like(z)
    for t in range(T):
        if keep is None:
            kept = True
        elif mutant == "keep_nonzero":
            kept = bool(keep[t] != 0)
        else:
            kept = bool(keep[t] > 0)                                  # 0.0, -0.0, negative, NaN: not kept
        if not kept:
            out[t] = x[t]
        elif bool(sigma[t] == 0):
            out[t] = z[t]
        elif mutant == "fma":
            out[t] = (noise[t].double() * sigma[t].double() + z[t].double()).float()
        else:
            p = noise[t] * sigma[t]
            out[t] = z[t] + p
    return out


def selector(T: int) -> torch.Tensor:
    """positive, 0.0, -0.0, negative and NaN frames, in turn (a positive subnormal and +inf among the positive ones)"""
    vals = [1.0, 0.0, -0.0, -1.0, NAN, 1e-45, -1e-45, float("inf"), float("-inf"), 0.5]
    return torch.tensor([vals[t % len(vals)] for t in range(T)], dtype=torch.float32)


def case(shape, variant, seed=0):
    """operands of one launch -> dict(z, noise, sigma, keep (or None), x (or None), out_is_x).  Values are drawn so that the FMA
    mutant shows: full 24-bit mantissas in z, noise and sigma."""
    T, C, Npix = shape
    g = torch.Generator().manual_seed(1000 * seed + 31 * T + 7 * C + Npix)
    z, noise, x = (torch.randn(T, C, Npix, generator=g) for _ in range(3))
    sigma = torch.rand(T, generator=g) * 14.0 + 0.03                    # the schedule's range: 0.03 .. 14.6
    z.view(-1)[::5] *= -1.0
    z.view(-1)[3::11] = -0.0                                          # -0.0 + noise * 0 would be +0.0: sigma 0 must copy
    ops = dict(z=z, noise=noise, sigma=sigma, keep=None, x=None, out_is_x=False)
    if variant == "keep_null":
        return ops
    ops["x"] = x
    ops["keep"] = selector(T) if T > 1 else torch.tensor([1.0])
    if variant == "selector":
        if T == 1:
            ops["keep"] = torch.tensor([NAN])
        return ops
    if variant == "sigma_zero":
        sigma[::2] = 0.0
        if T > 2:
            sigma[1] = -0.0
        return ops
    if variant == "out_is_x":
        ops["out_is_x"] = True
        return ops
    assert variant == "nan_noise"
    sigma[::3] = 0.0
    dead = (sigma == 0) | ~(ops["keep"] > 0)                          # frames whose noise must not matter
    noise[dead] = NAN
    if T == 1:
        assert bool(dead[0])
    return ops


def cases():
    for shape in SHAPES:
        for variant in VARIANTS:
            yield shape, variant
