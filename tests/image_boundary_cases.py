"""Cases and references of the image boundary (pnc_u8_to_tokens_f16 / pnc_tokens_to_u8), shared by tests/test_image_boundary.py
(CPU) and tests/test_image_boundary_gpu.py: the reference's numpy scalings, the reference's quantiser, the byte patterns and
shapes of the kernel tests, and numpy / torch twins of the two wrappers with panacea_amd/hip.py's signatures (a test installs them
on the emulated backend itself: tests/emu.py has no image entries)."""
import functools

import numpy as np
import torch

# nuscenes_datasets_video.py:542-552 on the 256 byte values, written out here (not imported from the product)
BYTES = np.arange(256, dtype=np.uint8)
TABLES = {"layout": BYTES.astype(np.float32) / 255.0, "image": BYTES.astype(np.float32) / 127.5 - 1.0}

# (C, Cpad, F, H, W): 208 pixels of 19 bytes start a pixel at every offset of a 16-byte chunk, a frame of 3952 bytes ends off a
# chunk boundary; 5 x 21 pixels of 19 channels: an odd pixel count and a ragged tail
U8_SHAPES = [(19, 24, 2, 8, 26), (3, 8, 2, 8, 26), (8, 8, 1, 8, 26), (1, 8, 1, 8, 26), (19, 24, 1, 5, 21)]
U8_OFFSETS = (0, 1, 3, 13)
GUARD = 256                     # bytes behind every output that must keep their 0xFF fill
# (M, C, ld): an odd byte count on the contiguous path; a strided matrix; one column
Q_SHAPES = [(1031, 3, 3), (64, 3, 8), (5, 1, 1)]


def frame_bytes(F, H, W, C) -> np.ndarray:
    """(F, H, W, C) uint8: byte (7 p + 13 c) mod 256 at pixel p (counted over all frames) and channel c — every channel sees all
    256 values"""
    p = np.arange(F * H * W, dtype=np.int64).reshape(F, H, W, 1)
    c = np.arange(C, dtype=np.int64).reshape(1, 1, 1, C)
    return ((7 * p + 13 * c) % 256).astype(np.uint8)


def scaled_nchw(u8: np.ndarray, kind: str) -> np.ndarray:
    """the float NCHW tensor the reference's pipeline builds from the bytes: the numpy expression, then channels first"""
    f = u8.astype(np.float32) / 255.0 if kind == "layout" else u8.astype(np.float32) / 127.5 - 1.0
    return np.ascontiguousarray(f.transpose(0, 3, 1, 2))


def quantise(x: np.ndarray) -> np.ndarray:
    """inference.py:189-193 / checkpoint._to_uint8 per element, in float32: clamp, (x + 1) / 2, * 255, truncate; NaN -> 0"""
    x = np.asarray(x, dtype=np.float32)
    t = np.minimum(np.maximum(np.nan_to_num(x, nan=-1.0), np.float32(-1.0)), np.float32(1.0))
    t = (t + np.float32(1.0)) / np.float32(2.0)
    t = t * np.float32(255.0)
    assert t.dtype == np.float32
    return t.astype(np.uint8)


def _order(x: np.ndarray) -> np.ndarray:
    """float32 -> int64 keys whose order is the floats' order"""
    b = x.view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def _unorder(k: np.ndarray) -> np.ndarray:
    return np.where(k < 0, (-k) | 0x80000000, k).astype(np.uint32).view(np.float32)


@functools.lru_cache(maxsize=None)
def thresholds() -> np.ndarray:
    """for every k in 1..255 the smallest float32 x with quantise(x) >= k — the quantiser is monotone, so quantise(x) == k there and
    k - 1 at its predecessor — found by bisection over the ordered float32 bit patterns"""
    lo = np.full(255, _order(np.array([-1.0], np.float32))[0], dtype=np.int64)       # quantise = 0 < k
    hi = np.full(255, _order(np.array([1.0], np.float32))[0], dtype=np.int64)        # quantise = 255 >= k
    k = np.arange(1, 256)
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        ge = quantise(_unorder(mid)) >= k
        hi = np.where(ge, mid, hi)
        lo = np.where(ge, lo, mid)
    return _unorder(hi)


def quantiser_inputs(n: int, seed: int = 0) -> np.ndarray:
    """n float32 inputs: every threshold and its predecessor, the specials, then random values in (-1.5, 1.5); a matrix too small to
    hold them all gets an evenly spaced selection of that list"""
    if n < 1024:
        full = quantiser_inputs(3093, seed)
        return full[np.linspace(0, 540, n).astype(np.int64)]
    th = thresholds()
    one, inf = np.float32(1.0), np.float32(np.inf)
    sp = [one, np.nextafter(one, inf), np.nextafter(one, -inf), -one, np.nextafter(-one, inf), np.nextafter(-one, -inf),
          0.0, -0.0, 3.0, -3.0, np.inf, -np.inf, np.nan]
    fixed = np.concatenate([th, np.nextafter(th, -inf), np.array(sp, dtype=np.float32)])
    assert n >= fixed.size
    rnd = np.random.default_rng(seed).uniform(-1.5, 1.5, n - fixed.size).astype(np.float32)
    return np.concatenate([fixed, rnd])


# ---- twins of the two wrappers (panacea_amd.hip.u8_to_tokens_f16 / tokens_to_u8) for the emulated backend -----------------------
CALLS = []          # names of the twins that ran, in order


def u8_to_tokens_f16(src_u8, lut32, F, Npix, Cch, Cpad, out16, out16_lo=None):
    CALLS.append("u8_to_tokens_f16")
    assert src_u8.dtype == torch.uint8 and src_u8.is_contiguous() and src_u8.numel() == F * Npix * Cch and lut32.numel() == 256
    v = torch.zeros((F * Npix, Cpad), dtype=torch.float32)
    v[:, :Cch] = lut32.float().cpu()[src_u8.reshape(F * Npix, Cch).long().cpu()]
    h = v.half()
    out16.reshape(-1)[: v.numel()].view(v.shape).copy_(h)
    if out16_lo is not None:
        out16_lo.reshape(-1)[: v.numel()].view(v.shape).copy_(((v - h.float()) * 2048.0).half())


def tokens_to_u8(x32, ld, M, Cch, out_u8):
    CALLS.append("tokens_to_u8")
    assert x32.dtype == torch.float32 and out_u8.dtype == torch.uint8 and out_u8.numel() == M * Cch
    x = x32.reshape(-1)[: (M - 1) * ld + Cch].cpu().numpy()
    rows = np.lib.stride_tricks.as_strided(x, shape=(M, Cch), strides=(4 * ld, 4))
    out_u8.reshape(M, Cch).copy_(torch.from_numpy(quantise(rows)))
