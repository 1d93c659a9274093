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
