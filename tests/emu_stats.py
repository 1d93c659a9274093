"""CPU emulation of pnc_operand_stats_f16 (include/panacea_hip.h: the range profile of one contraction operand) for the emu backend of
tests/emu.py, written from the header text with numpy.  tests/test_range_profile.py attaches `operand_stats` to `emu` with
monkeypatch; the GPU tests compare the kernel's records with `record()` word for word (integers: exact equality).

  rec[0..31]  elements per fp16 binade, index = (bits >> 10) & 31 of the hi plane
  rec[32]     max of (bits & 0x7FFF)
  rec[33]     lo elements at the end of their format: e4m3 (byte & 0x7F) >= 0x7E, fp16 non-finite; nothing without a lo plane
  rec[34]     NaN elements of hi
  rec[35]     elements counted
Columns cols .. ld - 1 of a row are padding and never read."""
import numpy as np
import torch

WORDS = 36


def _plane(t: torch.Tensor, rows: int, cols: int, ld: int, np_dtype) -> np.ndarray:
    """the [rows, cols] elements of the plane whose element 0 is t's first one (row stride ld), reinterpreted as np_dtype"""
    flat = torch.as_strided(t, ((rows - 1) * ld + cols,), (1,)) if t.numel() else t.reshape(-1)
    a = flat.detach().cpu().contiguous().numpy().view(np_dtype)
    return np.lib.stride_tricks.as_strided(a, (rows, cols), (ld * a.itemsize, a.itemsize))


def record(hi: torch.Tensor, lo, rows: int, cols: int, ld: int) -> np.ndarray:
    """the 36 words one launch ADDS (word 32: the value the launch maxes in), as int64"""
    if hi.dtype != torch.float16 or rows < 1 or cols < 1 or ld < cols:
        raise ValueError("PNC_EINVAL")
    if cols % 8 or ld % 8:
        raise ValueError("PNC_EALIGN")
    bits = _plane(hi, rows, cols, ld, np.uint16).astype(np.int64)
    a = bits & 0x7FFF
    rec = np.zeros(WORDS, dtype=np.int64)
    rec[:32] = np.bincount((a >> 10).reshape(-1), minlength=32)
    rec[32] = a.max()
    rec[34] = int((a > 0x7C00).sum())
    rec[35] = rows * cols
    if lo is not None:
        if lo.dtype == torch.uint8:
            b = _plane(lo, rows, cols, ld, np.uint8).astype(np.int64)
            rec[33] = int(((b & 0x7F) >= 0x7E).sum())
        elif lo.dtype == torch.float16:
            b = _plane(lo, rows, cols, ld, np.uint16).astype(np.int64)
            rec[33] = int(((b & 0x7C00) == 0x7C00).sum())
        else:
            raise ValueError("PNC_EINVAL")
    return rec


def accumulate(rec: torch.Tensor, add: np.ndarray):
    """what the kernel's atomics do to a record"""
    r = rec.reshape(-1)
    new = r[:WORDS].cpu().numpy() + add
    new[32] = max(int(r[32]), int(add[32]))
    r[:WORDS] = torch.from_numpy(new).to(r.device)


def operand_stats(hi, lo, rows, cols, ld, rec):
    """panacea_amd.hip.operand_stats"""
    assert rec.dtype == torch.int64 and rec.numel() >= WORDS and rec.is_contiguous()
    accumulate(rec, record(hi, lo, rows, cols, ld))
