"""The 8-bit image boundary of the per-sample path: uint8 channels-last frames enter as the fp16 token
planes the first convs read and leave as the decoder's token matrix quantised on the device — no float image on the host, no
NCHW image on the device.

The reference scales on the CPU, in numpy (sgm/data/nuscenes_video/nuscenes_datasets_video.py:542-552):

    source = source.astype(np.float32) / 255.0            the 19-channel BEV layout          -> table "layout"
    target = target.astype(np.float32) / 127.5 - 1.0      the (conditioning) frames          -> table "image"

`table(kind)` evaluates those very expressions on the 256 byte values, so `table(kind)[b]` IS the float the reference computes for
byte b, bit for bit; pnc_u8_to_tokens_f16 looks it up.  The two kernels are OPTIONAL capabilities of a backend, looked up by name
like AttnBlock looks up `attn_frame`: a backend without them refuses the uint8 paths before anything is launched and serves every
float path as before.
"""
from __future__ import annotations

import operator
from dataclasses import dataclass
from typing import Dict, Tuple

import numpy as np
import torch

from .engine import Act, Operand, Runtime

KINDS = ("layout", "image")
_DEVICE_TABLES: Dict[Tuple[str, str, int], torch.Tensor] = {}


def table(kind: str) -> np.ndarray:
    """the 256 fp32 values byte b scales to, by the reference's numpy expression for `kind`"""
    b = np.arange(256, dtype=np.uint8)
    if kind == "layout":
        return b.astype(np.float32) / 255.0
    if kind == "image":
        return b.astype(np.float32) / 127.5 - 1.0
    raise ValueError(f"unknown table {kind!r}: choose one of {KINDS}")


def device_table(kind: str, device) -> torch.Tensor:
    """`table(kind)` on `device`: one tensor per kind and device, created on first use and kept"""
    device = torch.device(device)
    index = device.index if device.index is not None else (torch.cuda.current_device() if device.type == "cuda" else -1)
    key = (kind, device.type, index)
    if key not in _DEVICE_TABLES:
        _DEVICE_TABLES[key] = torch.from_numpy(table(kind)).to(device)
    return _DEVICE_TABLES[key]


def capability(backend, name: str):
    """the backend's `name` wrapper; NotImplementedError naming it when the backend has none (nothing has been launched then)"""
    fn = getattr(backend, name, None)
    if fn is None:
        raise NotImplementedError(f"this backend has no `{name}`: uint8 frames need the image-boundary kernels "
                                  f"(pnc_{name} of include/panacea_hip.h)")
    return fn


def region_capability(backend, name: str):
    """the backend's `name` wrapper of the region-editing kernels (section 8 of include/panacea_hip.h), by name like `capability`"""
    fn = getattr(backend, name, None)
    if fn is None:
        raise NotImplementedError(f"this backend has no `{name}`: a keep mask needs the region-editing kernels "
                                  f"(pnc_{name} of include/panacea_hip.h)")
    return fn


def keep_mask_u8(mask_u8, T: int, H: int, W: int, what: str = "keep_mask_u8") -> torch.Tensor:
    """`mask_u8` checked as a (T, H, W) uint8 pixel mask (nonzero = this pixel is kept), contiguous"""
    if not isinstance(mask_u8, torch.Tensor) or mask_u8.dtype != torch.uint8 or mask_u8.shape != (T, H, W):
        raise ValueError(f"{what}: a ({T}, {H}, {W}) uint8 mask of the clip's size, got "
                         f"{tuple(mask_u8.shape) if isinstance(mask_u8, torch.Tensor) else type(mask_u8).__name__}"
                         f"{' ' + str(mask_u8.dtype) if isinstance(mask_u8, torch.Tensor) else ''}")
    return mask_u8.detach().contiguous()


def pool_keep_mask(mask_u8: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """a (T, H, W) uint8 pixel mask -> the (T, h, w) fp32 selector of the latent (pnc_mask_pool_u8 at f = H / h = W / w): a latent
    cell is 1.0 only where all of its f x f pixels are kept, so a cell the first stage computed partly from pixels that will be
    regenerated never counts as known"""
    from . import engine as E
    pool = region_capability(E.backend(), "mask_pool_u8")
    if not isinstance(mask_u8, torch.Tensor) or mask_u8.dtype != torch.uint8 or mask_u8.dim() != 3 or 0 in mask_u8.shape:
        raise ValueError(f"pool_keep_mask: a (T, H, W) uint8 mask, got "
                         f"{tuple(mask_u8.shape) if isinstance(mask_u8, torch.Tensor) else type(mask_u8).__name__}")
    T, H, W = mask_u8.shape
    h, w = operator.index(h), operator.index(w)
    if h < 1 or w < 1 or H % h or W % w or H // h != W // w or not 1 <= H // h <= 16:
        raise ValueError(f"pool_keep_mask: a {H} x {W} mask pools to {h} x {w} by one factor in 1 .. 16 only")
    out = torch.empty((T, h, w), dtype=torch.float32, device=mask_u8.device)
    pool(mask_u8.detach().contiguous(), H // h, out)
    return out


def select_u8(src_u8: torch.Tensor, gen_u8: torch.Tensor, mask_u8: torch.Tensor) -> torch.Tensor:
    """(T, H, W, C) uint8 frames: `src_u8` where the pixel's byte of the (T, H, W) `mask_u8` is nonzero, `gen_u8` elsewhere
    (pnc_u8_select), a new tensor"""
    from . import engine as E
    select = region_capability(E.backend(), "u8_select")
    for name, t in (("src_u8", src_u8), ("gen_u8", gen_u8), ("mask_u8", mask_u8)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8:
            raise TypeError(f"select_u8: {name} is a uint8 tensor, got {t.dtype if isinstance(t, torch.Tensor) else type(t).__name__}")
    if src_u8.dim() != 4 or gen_u8.shape != src_u8.shape or mask_u8.shape != src_u8.shape[:3]:
        raise ValueError(f"select_u8: (T, H, W, C) frames twice and their (T, H, W) mask, got {tuple(src_u8.shape)}, "
                         f"{tuple(gen_u8.shape)} and {tuple(mask_u8.shape)}")
    out = torch.empty_like(gen_u8, memory_format=torch.contiguous_format)
    select(src_u8.detach().contiguous(), gen_u8.detach().contiguous(), mask_u8.detach().contiguous(), out)
    return out


def view_mask(T: int, H: int, W: int, views: int, keep_views, device="cpu") -> torch.Tensor:
    """a (T, H, W) uint8 mask of a panorama of `views` camera views side by side: 255 in the column band of every view in
    `keep_views`, 0 elsewhere"""
    views = operator.index(views)
    if views < 1 or W % views:
        raise ValueError(f"view_mask: {W} columns do not split into {views} views")
    keep_views = tuple(operator.index(v) for v in keep_views)
    if any(not 0 <= v < views for v in keep_views):
        raise ValueError(f"view_mask: views {keep_views} outside 0 .. {views - 1}")
    mask = torch.zeros((T, H, W), dtype=torch.uint8)
    band = W // views
    for v in keep_views:
        mask[:, :, v * band:(v + 1) * band] = 255
    return mask.to(device)


def rect_mask(T: int, H: int, W: int, rect, device="cpu") -> torch.Tensor:
    """a (T, H, W) uint8 mask that is 0 inside the rectangle rect = (y0, x0, y1, x1) (rows y0 .. y1 - 1, columns x0 .. x1 - 1 of
    every frame: what is re-rendered) and 255 outside"""
    try:
        y0, x0, y1, x1 = (operator.index(v) for v in rect)
    except (TypeError, ValueError):
        raise ValueError(f"rect_mask: rect is four integers (y0, x0, y1, x1), got {rect!r}") from None
    if not (0 <= y0 < y1 <= H and 0 <= x0 < x1 <= W):
        raise ValueError(f"rect_mask: a non-empty rectangle inside {H} x {W} expected, got {(y0, x0, y1, x1)}")
    mask = torch.full((T, H, W), 255, dtype=torch.uint8)
    mask[:, y0:y1, x0:x1] = 0
    return mask.to(device)


def frames_u8(x: torch.Tensor, what: str) -> torch.Tensor:
    """`x` as contiguous (F, H, W, C) uint8 frames; a (b, t, H, W, C) clip is flattened over its first two dimensions"""
    if x.dtype != torch.uint8:
        raise TypeError(f"{what}: uint8 channels-last frames expected, got {x.dtype}")
    if x.dim() == 5:
        x = x.reshape(-1, *x.shape[2:])
    if x.dim() != 4:
        raise ValueError(f"{what}: uint8 frames are (F, H, W, C) channels-last, got {tuple(x.shape)}")
    return x.detach().contiguous()


@dataclass(frozen=True, eq=False)
class SparseClip:
    """A conditioning clip of `num_frames` frames of which only K are given: `frames_u8` (K, H, W, 3) uint8 channels-last sit at
    `slots` (K distinct indices in [0, num_frames), negative ones counted from the end), every other slot is the blank frame — float
    0.0 after the dataset's scaling, which no byte scales to.  This is `final_cond_zero` (nuscenes_datasets_video.py:559-566) with
    K = 1: the anchor in the last (use_last_frame) or first slot of an all-zero clip.  `slots` is kept as a tuple of non-negative
    indices."""
    frames_u8: torch.Tensor
    slots: Tuple[int, ...]
    num_frames: int

    def __post_init__(self):
        x = self.frames_u8
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"SparseClip: frames_u8 is a uint8 tensor, got {type(x).__name__}")
        if x.dtype != torch.uint8:
            raise TypeError(f"SparseClip: uint8 channels-last frames expected, got {x.dtype}")
        if x.dim() != 4 or 0 in x.shape[1:]:
            raise ValueError(f"SparseClip: frames_u8 is (K, H, W, C) channels-last, got {tuple(x.shape)}")
        T = self.num_frames
        if isinstance(T, bool) or not isinstance(T, int):
            raise TypeError(f"SparseClip: num_frames is an int, got {type(T).__name__}")
        if T < 1:
            raise ValueError(f"SparseClip: num_frames >= 1, got {T}")
        try:
            slots = tuple(operator.index(s) for s in self.slots)
        except TypeError:
            raise TypeError(f"SparseClip: slots are integers, got {self.slots!r}") from None
        if len(slots) != x.shape[0]:
            raise ValueError(f"SparseClip: {x.shape[0]} frames for {len(slots)} slots")
        if any(not -T <= s < T for s in slots):
            raise ValueError(f"SparseClip: slots {slots} outside a clip of {T} frames")
        slots = tuple(s % T for s in slots)
        if len(set(slots)) != len(slots):
            raise ValueError(f"SparseClip: slots {slots} name a frame twice")
        object.__setattr__(self, "frames_u8", x.detach().contiguous())
        object.__setattr__(self, "slots", slots)

    def gather_index(self) -> torch.Tensor:
        """(num_frames,) int64 on the frames' device: for every slot of the clip, the row of [the K given frames, the blank frame]
        that fills it"""
        K = len(self.slots)
        idx = [K] * self.num_frames
        for j, s in enumerate(self.slots):
            idx[s] = j
        return torch.tensor(idx, dtype=torch.int64, device=self.frames_u8.device)


def u8_to_tokens(rt: Runtime, x_u8: torch.Tensor, kind: str, Cpad: int, out: Operand):
    """(F, H, W, C) uint8 -> the fp16 planes `out` ([F*H*W, Cpad]), scaled by table `kind`"""
    convert = capability(rt.be, "u8_to_tokens_f16")
    if out.lo is not None and out.lo.dtype != torch.float16:
        raise NotImplementedError("the image entry writes fp16 lo planes only")
    F, H, W, C = x_u8.shape
    convert(x_u8, device_table(kind, x_u8.device), F, H * W, C, Cpad, *out)


def tokens_to_u8(rt: Runtime, a: Act) -> torch.Tensor:
    """the fp32 token matrix of `a` as (F, H, W, C) uint8 frames on its device"""
    quantise = capability(rt.be, "tokens_to_u8")
    out = rt.empty((a.F, a.H, a.W, a.C), torch.uint8)
    quantise(a.f32, a.f32.shape[1], a.M, a.C, out)
    return out
