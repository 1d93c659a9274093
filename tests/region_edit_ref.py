"""Per-op references of the three region-editing entries (pnc_latent_renoise_masked, pnc_mask_pool_u8, pnc_u8_select), written from
their comment block in include/panacea_hip.h (section 8) alone: this file imports neither tests/emu.py nor panacea_amd.

`latent_renoise_masked` evaluates one launch with torch fp32 CPU tensors, ONE elementwise torch op per rounding, in the header's
order: the product noise * sigma rounded to fp32, then the sum with z; everything else is a select (torch.where moves bits).  An
element is kept iff its pixel's mask value is > 0; a kept element of a frame whose sigma is 0 is z's bits; an element that is not
kept is x's bits.  Operands are [T][C][Npix] planes, a [T] sigma and a [T][Npix] mask.  `mask_pool_u8` and `u8_select` are byte
references.  `out == x` / `out == gen` need no case of their own here: what is not rewritten holds the bits a copy would hold.

`mutant=NAME` is a WRONG kernel, the reference with one deviation (MUTANTS: name -> (entry, what is wrong)).
tests/test_region_edit.py shows that each of them leaves the reference's bits somewhere on the case lists below, and a failing GPU
comparison names the mutant, if any, whose bits the kernel has.

The case lists (RENOISE_SHAPES x MASKS x VARIANTS, POOL_CASES x POOL_FILLS, SELECT_CASES) are the ones tests/test_region_edit_gpu.py
launches."""
import torch

import clip_edit_ref as cref

NAN = float("nan")
MUTANTS = {
    "fma": ("renoise", "z + noise * sigma contracted into one rounding (float64, then rounded)"),
    "mask_nonzero": ("renoise", "an element kept where mask != 0 instead of mask > 0: negative and NaN selectors keep"),
    "mask_pixel0": ("renoise", "the mask of pixel 0 applied to the whole frame"),
    "mask_by_element": ("renoise", "the mask indexed by the element's index in the frame (c * Npix + p) instead of the pixel p: wrong "
                                   "for every plane but the first"),
    "x_blend": ("renoise", "k * kept + (1 - k) * x instead of a select: NaN in the operand that is not selected comes through"),
    "pool_any": ("pool", "a cell is 1.0 where ANY of its bytes is nonzero"),
    "pool_skip_last_row": ("pool", "the last row of every f x f block is not looked at"),
    "pool_skip_last_col": ("pool", "the last column of every f x f block is not looked at"),
    "select_per_byte": ("select", "the mask taken per byte (mask[i] for byte i of the frames) instead of per pixel"),
}


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


# ---- pnc_latent_renoise_masked -----------------------------------------------------------------------------------------------------
def latent_renoise_masked(z, noise, sigma, mask, x, mutant=None) -> torch.Tensor:
    """-> out [T, C, Npix] fp32"""
    assert mutant is None or MUTANTS[mutant][0] == "renoise"
    T, C, Npix = z.shape
    assert mask.shape == (T, Npix) and sigma.shape == (T,) and noise.shape == z.shape == x.shape
    keep = mask != 0 if mutant == "mask_nonzero" else mask > 0        # 0.0, -0.0, negative, NaN: not kept
    keep = keep[:, None, :].expand(T, C, Npix)
    if mutant == "mask_pixel0":
        keep = keep[:, :, :1].expand(T, C, Npix)
    if mutant == "mask_by_element":
        flat = (mask > 0).reshape(-1)
        idx = (torch.arange(T)[:, None] * Npix + torch.arange(C * Npix)[None, :]) % flat.numel()
        keep = flat[idx].view(T, C, Npix)
    s = sigma[:, None, None]
    if mutant == "fma":
        both = (noise.double() * s.double() + z.double()).float()
    else:
        p = noise * s                                                  # rounded on its own ...
        both = z + p                                                   # ... then the sum
    kept = torch.where(s == 0, z, both)                                # sigma 0 (either sign): z's bits, whatever the noise holds
    if mutant == "x_blend":
        k = keep.to(torch.float32)
        return k * kept + (1.0 - k) * x
    return torch.where(keep, kept, x)


# (T, C, Npix): scalar-only planes; whole float4s; more than one frame off a multiple of 1024; Npix % 4 != 0 (the planes of a frame
# start at different offsets from a 16-byte boundary, the mask row does not); three planes of two slices with one pixel in the
# second; 16 frames; eight planes of three slices
RENOISE_SHAPES = [(1, 4, 7), (2, 4, 96), (3, 4, 100), (3, 4, 98), (2, 3, 1025), (16, 4, 768), (2, 8, 3072)]
MASKS = ["all", "none", "alternate", "band", "last_pixel", "selector"]
VARIANTS = ["plain", "sigma_zero", "out_is_x", "nan_inert"]


def renoise_mask(pattern, T, Npix) -> torch.Tensor:
    """[T][Npix] fp32.  alternate: every other pixel, so every float4 mixes kept and not kept; band: ten columns of a latent 24
    wide (float4s all kept, none kept and mixed); selector: clip_edit_ref.selector's positive, 0.0, -0.0, negative, NaN, subnormal
    and infinite values laid over the pixels, shifted by one per frame"""
    p = torch.arange(Npix)
    if pattern == "all":
        return torch.ones(T, Npix)
    if pattern == "none":
        return torch.zeros(T, Npix)
    if pattern == "alternate":
        return ((p[None, :] + torch.arange(T)[:, None]) % 2 == 0).to(torch.float32)
    if pattern == "band":
        q = (p[None, :] + 2 * torch.arange(T)[:, None]) % 24           # the band moves by two columns per frame
        return ((q >= 4) & (q < 14)).to(torch.float32)
    if pattern == "last_pixel":
        m = torch.zeros(T, Npix)
        m[:, -1] = 1.0
        return m
    assert pattern == "selector"
    vals = cref.selector(Npix + T)
    return torch.stack([vals[t:t + Npix] for t in range(T)])


def renoise_case(shape, pattern, variant, seed=0):
    """operands of one launch -> dict(z, noise, sigma, mask, x, out_is_x).  Full 24-bit mantissas in z, noise and sigma, so that
    the FMA mutant shows; -0.0 in z, so that sigma 0 has to copy."""
    T, C, Npix = shape
    g = torch.Generator().manual_seed(1000 * seed + 31 * T + 7 * C + Npix)
    z, noise, x = (torch.randn(T, C, Npix, generator=g) for _ in range(3))
    sigma = torch.rand(T, generator=g) * 14.0 + 0.03                    # the schedule's range: 0.03 .. 14.6
    z.view(-1)[::5] *= -1.0
    z.view(-1)[3::11] = -0.0
    mask = renoise_mask(pattern, T, Npix)
    ops = dict(z=z, noise=noise, sigma=sigma, mask=mask, x=x, out_is_x=variant == "out_is_x")
    if variant == "sigma_zero":
        sigma[::2] = 0.0
        if T > 2:
            sigma[1] = -0.0
    if variant == "nan_inert":                                          # NaN in every operand that must not be read
        sigma[::3] = 0.0
        keep = (mask > 0)[:, None, :].expand(T, C, Npix)
        noise[~keep | (sigma == 0)[:, None, None].expand(T, C, Npix)] = NAN
        z[~keep] = NAN
        x[keep] = NAN
    return ops


def renoise_cases():
    for shape in RENOISE_SHAPES:
        for pattern in MASKS:
            for variant in VARIANTS:
                yield shape, pattern, variant


# ---- pnc_mask_pool_u8 ----------------------------------------------------------------------------------------------------------------
def mask_pool_u8(mask_u8, f, mutant=None) -> torch.Tensor:
    """(T, H, W) uint8 -> (T, H / f, W / f) fp32: 1.0 iff every byte of the cell's f x f block is nonzero"""
    assert mutant is None or MUTANTS[mutant][0] == "pool"
    T, H, W = mask_u8.shape
    assert 1 <= f <= 16 and H % f == 0 and W % f == 0
    blocks = (mask_u8 != 0).view(T, H // f, f, W // f, f)
    if mutant == "pool_skip_last_row":
        blocks = blocks[:, :, :f - 1]
    if mutant == "pool_skip_last_col":
        blocks = blocks[..., :f - 1]
    if mutant == "pool_any":
        return blocks.any(dim=4).any(dim=2).to(torch.float32)
    return blocks.all(dim=4).all(dim=2).to(torch.float32)


# (T, H, W, f, byte offset of the mask's base): one cell; 8-byte rows; a small factor off the row form; rows from a base 1 byte off
# (no 8-byte reads); f = 1; f = 16
POOL_CASES = [(1, 8, 8, 8, 0), (2, 16, 24, 8, 0), (1, 6, 10, 2, 0), (3, 32, 48, 8, 1), (1, 4, 4, 1, 0), (1, 32, 16, 16, 0)]
POOL_FILLS = ["all255", "hole_tl", "hole_tr", "hole_bl", "hole_br", "hole_centre", "low_values"]


def pool_mask(case, fill) -> torch.Tensor:
    """all255; one zero byte at a corner or the centre of ONE block (the last block of the last frame), everything else 255; the
    values 1 and 128 for "nonzero" with every third block holding one zero byte"""
    T, H, W, f, _ = case
    m = torch.full((T, H, W), 255, dtype=torch.uint8)
    y0, x0 = H - f, W - f
    if fill == "low_values":
        m[:, ::2] = 1
        m[:, 1::2, ::2] = 128
        for k, (y, x) in enumerate((y, x) for y in range(0, H, f) for x in range(0, W, f)):
            if k % 3 == 1:
                m[:, y + (k % f), x + ((k // 3) % f)] = 0
    elif fill != "all255":
        dy, dx = {"hole_tl": (0, 0), "hole_tr": (0, f - 1), "hole_bl": (f - 1, 0), "hole_br": (f - 1, f - 1),
                  "hole_centre": (f // 2, f // 2)}[fill]
        m[T - 1, y0 + dy, x0 + dx] = 0
    return m


# ---- pnc_u8_select -------------------------------------------------------------------------------------------------------------------
def u8_select(src, gen, mask_u8, mutant=None) -> torch.Tensor:
    """src, gen [npix][C] uint8, mask_u8 [npix] -> out [npix][C]: src where the pixel's mask byte is nonzero, gen elsewhere"""
    assert mutant is None or MUTANTS[mutant][0] == "select"
    npix, C = src.shape
    assert gen.shape == src.shape and mask_u8.shape == (npix,)
    if mutant == "select_per_byte":
        take = (mask_u8 != 0)[torch.arange(npix * C) % npix].view(npix, C)
    else:
        take = (mask_u8 != 0)[:, None].expand(npix, C)
    return torch.where(take, src, gen)


# (npix, C): one pixel; a run shorter than a 16-byte chunk; 48 bytes; head, body and tail; more than one workgroup; C = 1 and C = 4
SELECT_CASES = [(1, 3), (15, 3), (16, 3), (231, 3), (4096, 3), (33, 1), (33, 4)]


def select_case(case, seed=0):
    """-> (src, gen, mask): random bytes; the mask holds 0, 1, 128 and 255, about half of the pixels kept, in runs of one to five"""
    npix, C = case
    g = torch.Generator().manual_seed(7 * seed + 13 * npix + C)
    src, gen = (torch.randint(0, 256, (npix, C), generator=g, dtype=torch.uint8) for _ in range(2))
    gen[src == gen] ^= 0x5A                                             # no byte at which a wrong choice would not show
    vals = torch.tensor([0, 1, 0, 128, 0, 255], dtype=torch.uint8)
    runs = torch.randint(1, 6, (npix,), generator=g)
    mask = vals[torch.repeat_interleave(torch.arange(npix) % 6, runs)[:npix]]
    return src, gen, mask
