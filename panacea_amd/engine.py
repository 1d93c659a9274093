"""Execution runtime of the MI355X denoising path: activation handles, weight packing and the
op helpers the module mirrors in `panacea_amd/nn/` are written against.

Data layout.  Activations never leave ONE resident layout: channels-last token
matrices, row m = (frame f, y, x), columns = channels.  The six camera views are a stride along x,
frames a stride along the leading dimension, so intra-view / cross-view / temporal attention, 3x3
convs and temporal convs all address the same buffer — none of the reference's NCHW <-> (b hw c) <->
(bhw t c) copies (attention.py:1069-1134, openaimodel.py:505-515) exist here.  The residual stream is
fp32 (`Act.f32`); every contraction operand is fp16 (`Act.f16`, produced by the norm kernels or by a
GEMM epilogue).

The frame / view shards of the multi-GPU layouts (`FrameShard`, `ViewShard`: who exchanges what over `torch.distributed`) live in
`panacea_amd/shard.py`; this module re-exports the two names and holds the op helpers that call them (`gn_spatial`,
`gn_temporal_sharded`).

The compute backend is `panacea_amd.hip` (ctypes -> libpanacea_hip.so).  `use_backend()` exists so
that the test-suite can run the host logic against a torch emulation of the C-ABI on CPU; product
code never calls it and there is no automatic fallback.
"""
from __future__ import annotations

import contextlib
import dataclasses
import math
import os
from dataclasses import dataclass
from typing import Callable, Dict, List, NamedTuple, Optional

import torch

from . import hip as _hip
from .shard import FrameShard, ViewShard      # noqa: F401 — `engine.FrameShard` / `engine.ViewShard` stay the public names

_BACKEND = _hip


def backend():
    return _BACKEND


@contextlib.contextmanager
def use_backend(be):
    """TESTS ONLY: run the host logic against another implementation of the C-ABI wrappers."""
    global _BACKEND
    old, _BACKEND = _BACKEND, be
    try:
        yield
    finally:
        _BACKEND = old


TEXT_PAD = 80          # 77 text tokens padded to a multiple of 8 rows (zero rows, masked in the kernel)


@dataclass(frozen=True)
class Precision:
    """Which fp16 operand classes are carried as PRECISE (split) pairs hi + lo * 2^-11 (include/panacea_hip.h,
    PncGemmParams.A_lo): the consumer GEMM then runs its K loop twice.  The classes are those of the measured error
    budget (tools/exp/error_budget.py) — share of the eps error variance at full width in brackets:

      stream   [47 %] fp16 copies of the un-normalised fp32 stream: inputs of skip 1x1 convs, zero convs, Down/Upsample
                      convs, the STT / ResBlock outputs handed to them, the skip concat
      gn_stt   [11 %] GroupNorm output feeding proj_in / proj_in_temporal / proj_in_crossview
      ff_out   [10 %] last transformer block's output feeding proj_out*
      stem     [ 8 %] network input tokens (latent | concat) feeding the stem convs
      gn_head  [ 8 %] GroupNorm+SiLU feeding the 4-channel output conv
      gn_res   [ 5 %] GroupNorm+SiLU feeding the ResBlock3D 3x3 convs (the expensive one: doubles the conv3x3 family)
      gnt      [ 3 %] temporal GroupNorm+SiLU feeding the temporal conv1d
      conv_mid [ 2 %] fp16 activations between the layers of the ControlNet hint stem
    LayerNorm outputs, q/k/v, the GEGLU hidden state and the attention output together are < 4 %: never split.

    `lo8`: the lo planes of the classes in LO8_CLASSES are stored as OCP e4m3 bytes (PNC_LO_E4M3) instead of fp16 and their
    consumer GEMMs run the lo K loop on the block-scaled fp8 MFMA against an e4m3 copy of the weights (round 3; half the
    bytes, twice the MFMA rate of the fp16 lo pass).  |lo| <= |v|, so e4m3 resolves the pair to ~2^-15 of v."""
    stream: bool = False
    gn_stt: bool = False
    ff_out: bool = False
    stem: bool = False
    gn_head: bool = False
    gn_res: bool = False
    gnt: bool = False
    conv_mid: bool = False
    lo8: bool = False
    # the classes below are split by `precise-wide` only (every operand of the path, fp16 lo planes): the LayerNorm outputs, the
    # q / k / v of the intra-view, cross-view and temporal attention, the text queries and keys / values, the fp16 context, the
    # GEGLU hidden state and the attention output.  The five attention classes (qkv, q_text, kv_text, ctx, attn_o) go together: the
    # split attention kernels (pnc_attn_views_split_f16 / pnc_attn_temporal_split_f16) read and write all of them.
    ln: bool = False
    qkv: bool = False
    q_text: bool = False
    kv_text: bool = False
    ctx: bool = False
    ff_hidden: bool = False
    attn_o: bool = False
    # `weights`: the packed WEIGHTS are split too, W = fp16(W) + 2^-11 * fp16((W - fp16(W)) * 2^11) (PncGemmParams.W_lo).  Every GEMM
    # adds the A_hi * W_lo products to its lo pass, so an fp32 checkpoint is multiplied at ~22 bits instead of being rounded to fp16
    # first (that rounding alone is 1.3e-3 .. 2.1e-3 of eps on the tiny network).  The plane joins the fp16 lo
    # pass of a split activation: the flag needs every class split and fp16 lo planes.
    # It is a plain class attribute here and a field of the subclass SplitWeights only.  The fields of THIS class are the operand
    # classes and `lo8`; code that enumerates dataclasses.fields(Precision) as "the classes" (tests/test_precise_wide.py does) keeps
    # seeing exactly those, and `weights` splits no activation.  So `precise-full` is a SplitWeights and never equal to a Precision:
    # where both should answer alike, ask is_wide().
    weights = False
    beside = False         # WeightsBeside only: the twin travels next to the launch (gemm(..., w_lo16=)) instead of in PncGemmParams.W_lo

    def __post_init__(self):
        att = (self.qkv, self.q_text, self.kv_text, self.attn_o, self.ctx)
        if any(att) and not all(att):
            raise ValueError("the attention operand classes qkv, q_text, kv_text, ctx and attn_o are split together or not at all")
        if any(att) and self.lo8:
            raise ValueError("the split attention kernels read fp16 lo planes: a policy that splits q / k / v cannot set lo8")
        if self.weights and self.lo8:
            raise ValueError("split weights ride on the fp16 lo pass: a policy with `weights` cannot set lo8 (the e4m3 form of a weight "
                             "lo pass would need an e4m3 copy of every activation's hi plane)")
        if self.weights and not all(getattr(self, c) for c in OPERAND_CLASSES):
            raise ValueError("split weights need every operand class split: each GEMM that receives W_lo must also receive an fp16 A_lo")

    @property
    def name(self) -> str:
        on = [k for k, v in self.__dict__.items() if v and k not in ("lo8", "weights")]
        return ("fp16" if not on else "split(" + ",".join(on) + (")+e4m3-lo" if self.lo8 else ")") + ("+weights" if self.weights else "")
                + ("-beside" if self.beside else ""))

    def lo_dtype(self, cls: str) -> torch.dtype:
        """dtype of the lo plane of operand class `cls` (= its PNC_LO_* format, panacea_amd.hip.lo_fmt)"""
        return torch.uint8 if (self.lo8 and cls in LO8_CLASSES) else torch.float16


@dataclass(frozen=True)
class SplitWeights(Precision):
    """A policy whose weights are split as well (`weights`, see Precision): every operand class split, fp16 lo planes"""
    weights: bool = True


@dataclass(frozen=True)
class WeightsBeside(Precision):
    """`precise-ckpt`: the operand classes and lo-plane formats of `precise` (e4m3 lo planes, `lo8`) + split weights, for fp32
    checkpoints whose activations stay inside `precise`'s range.  The fp16 lo twin of the weights travels BESIDE the launch
    (pnc_gemm_wsplit_f16, `gemm(..., w_lo16=)`), which adds the A_hi * W_lo products ahead of everything `precise` runs: one more fp16
    pass per GEMM, no split attention kernels (attention multiplies activations by activations).  `weights` is True, so the small-M
    linears and the stacked projectors hand over their twins as under `precise-full`; `beside` tells engine.gemm which way the plane
    goes.  The class set is exactly `precise`'s: those are the consumers the entry point serves (every other set would also want
    measurements of its own); single-device like `precise-full`."""
    weights = True
    beside = True

    def __post_init__(self):
        want = {f.name: getattr(PRECISE, f.name) for f in dataclasses.fields(Precision)}
        have = {f.name: getattr(self, f.name) for f in dataclasses.fields(Precision)}
        if have != want:
            raise ValueError("weights beside the launch (`precise-ckpt`) go with exactly the operand classes and e4m3 lo planes of "
                             f"`precise`: {sorted(k for k, v in want.items() if v)}; got {sorted(k for k, v in have.items() if v)}")


OPERAND_CLASSES = ("stream", "gn_stt", "ff_out", "stem", "gn_head", "gn_res", "gnt", "conv_mid",
                   "ln", "qkv", "q_text", "kv_text", "ctx", "ff_hidden", "attn_o")

# classes whose consumers all run the e4m3 lo pass: plain-A GEMMs with K % 16 == 0 and the conv gathers with Cin % 64 == 0.
# Not: `stem` (Cin = 8: a 16-byte chunk of e4m3 would span two taps), `conv_mid` (narrow hint-stem layers), `gn_res` (its
# stride-1 convs run on the halo-tile kernel, whose lo pass reads fp16 planes).
LO8_CLASSES = frozenset({"stream", "gn_stt", "ff_out", "gn_head", "gnt"})


FAST = Precision()
# eps max-abs < 1e-3 at BASELINE config 3: every class except the ResBlock conv inputs (36 ms of conv3x3
# for 5 % of the variance) and the hint stem's inner activations (4 ms for 2 %)
PRECISE = Precision(stream=True, gn_stt=True, ff_out=True, stem=True, gn_head=True, gnt=True, lo8=True)
PRECISE_ALL = Precision(stream=True, gn_stt=True, ff_out=True, stem=True, gn_head=True, gn_res=True, gnt=True, conv_mid=True, lo8=True)
# without the temporal-conv operand: 6 ms cheaper, ~12 % more error — kept for the cost / error table of DESIGN.md §6
PRECISE_LITE = Precision(stream=True, gn_stt=True, ff_out=True, stem=True, gn_head=True, lo8=True)
# round 2's form of `precise`: every lo plane fp16, lo pass on the fp16 MFMA (A/B of the e4m3 lo pass)
PRECISE_F16LO = Precision(stream=True, gn_stt=True, ff_out=True, stem=True, gn_head=True, gnt=True)
# every operand class split, every lo plane fp16: an fp16 lo plane (v - fp16(v)) * 2^11 has the hi plane's range, so the policy holds
# up to |operand| < 65504 (the e4m3 lo planes of `precise` saturate from |v| = 512 on).  Eps 8.5e-6 in the CPU error budget of the
# heavy-tail weight set, where `precise` leaves 2.0e-3.  The target of on_range_exceeded = "escalate".
PRECISE_WIDE = Precision(stream=True, gn_stt=True, ff_out=True, stem=True, gn_head=True, gn_res=True, gnt=True, conv_mid=True,
                         ln=True, qkv=True, q_text=True, kv_text=True, ctx=True, ff_hidden=True, attn_o=True)
# `precise-wide` plus split weights: the policy for fp32 checkpoints, whose weights are not fp16-representable.  Three fp16 passes
# per GEMM instead of two, and an fp16 lo twin of every packed weight (about +4.5 GB at full size).
PRECISE_FULL = SplitWeights(**dataclasses.asdict(PRECISE_WIDE))
# `precise` plus split weights beside the launch: fp32 checkpoints with an ordinary activation range (|v| < 512)
PRECISE_CKPT = WeightsBeside(**dataclasses.asdict(PRECISE))
PRECISIONS = {"fast": FAST, "precise": PRECISE, "precise-all": PRECISE_ALL, "precise-lite": PRECISE_LITE,
              "precise-f16lo": PRECISE_F16LO, "precise-wide": PRECISE_WIDE, "precise-full": PRECISE_FULL,
              "precise-ckpt": PRECISE_CKPT}


def is_wide(p) -> bool:
    """every operand class split with fp16 lo planes, hence the split attention kernels: `precise-wide`, `precise-full` and any policy
    built like them, whatever its class or `weights` flag.  Single-device policies (no frame / view shards)."""
    p = precision(p)
    return not p.lo8 and all(getattr(p, c) for c in OPERAND_CLASSES)


def weights_beside(p) -> bool:
    """the policy hands the weights' lo twins over beside the launch (`precise-ckpt`).  Single-device, like the wide policies."""
    return bool(getattr(precision(p), "beside", False))


def single_device_only(p) -> bool:
    """the policies that frame / view shards and ShardedCFG refuse"""
    return is_wide(p) or weights_beside(p)


def precision(p) -> Precision:
    if isinstance(p, Precision):
        return p
    if p not in PRECISIONS:
        raise ValueError(f"unknown precision {p!r}: choose one of {sorted(PRECISIONS)} or pass an engine.Precision")
    return PRECISIONS[p]


class Operand(NamedTuple):
    """One contraction operand as it travels from its producer to `gemm` (or an attention kernel): the fp16 plane and — when the
    policy splits the operand's class — its lo plane, fp16 or uint8 = e4m3 bytes (Precision.lo_dtype)."""
    hi: torch.Tensor
    lo: Optional[torch.Tensor] = None

    def map(self, fn) -> "Operand":
        """the same view / slice / exchange of both planes"""
        return Operand(fn(self.hi), None if self.lo is None else fn(self.lo))

    def planes(self) -> list:
        return [self.hi] if self.lo is None else [self.hi, self.lo]


class TextKV(NamedTuple):
    """Text keys / values of one cross-attention site (Runtime.text_kv), as flat views whose element 0 is the site's first one.
    Keys are row-major: token r of sample b starts at element (b * TEXT_PAD + r) * ldk.  Values, fp16 policies: channel-major V^T,
    channel c of sample b starts at b * v_gstride + c * ldv (the layout pnc_attn_views_f16 reads); a policy that splits `kv_text`:
    row-major like the keys, ldv = ldk, v_gstride = 0 (the split attention kernels; a transposed store has no lo plane)."""
    k: Operand
    ldk: int
    v: Operand
    ldv: int
    v_gstride: int = 0


@dataclass
class Act:
    """A feature map in the resident layout: [F*H*W, C] tokens, fp32 stream and/or fp16 operand."""
    F: int
    H: int
    W: int
    C: int
    f32: Optional[torch.Tensor] = None
    f16: Optional[Operand] = None
    gn_part: Optional[torch.Tensor] = None     # GroupNorm(32) records of f32 when its producer wrote them (engine.gn_records)

    @property
    def N(self) -> int:
        return self.H * self.W

    @property
    def M(self) -> int:
        return self.F * self.H * self.W

    def need_f16(self, rt: "Runtime") -> Operand:
        """fp16 operand copy of the stream (operand class `stream`)"""
        if self.f16 is None:
            self.f16 = rt.operand((self.M, self.C), "stream")
            rt.be.cast_f16(self.f32, self.M * self.C, *self.f16)
        return self.f16

    def to_nchw(self) -> torch.Tensor:
        t = self.f32 if self.f32 is not None else self.f16.hi.float()
        return t.view(self.F, self.H, self.W, self.C).permute(0, 3, 1, 2).contiguous()


class Runtime:
    """Per-forward execution context.  B samples x T frames; with a FrameShard only T_local = T / G frames of every
    sample live on this rank (F = B * T_local frames in the resident layout); with a ViewShard every map is this rank's
    band of W / G columns."""

    def __init__(self, device: torch.device, B: int, T: int, shard: Optional[FrameShard] = None,
                 vshard: Optional[ViewShard] = None):
        self.be = backend()
        self.device = device
        # a frame shard and a view shard compose (round 4: SURVEY 8e's cfg x view-group x frame-group grid): the rank holds
        # T / G frames of a band of W / V columns; the temporal sites exchange inside the frame group over the band's pixels,
        # the view couplings inside the view group over the rank's frames
        self.shard = shard
        self.vshard = vshard
        G = shard.G if shard is not None else 1
        if T % G:
            raise ValueError(f"{T} frames per sample do not split over {G} frame groups")
        self.B, self.T, self.T_local = B, T, T // G
        self.F = B * self.T_local
        self.emb_all: Optional[torch.Tensor] = None    # frame-sharded runs: SiLU(emb) rows of ALL B*T frames
        self.prec: Precision = FAST                    # operand precision policy of this evaluation
        self.ctx16: Optional[Operand] = None           # [B*TEXT_PAD, context_dim] fp16, zero padded (+ lo plane: operand class `ctx`)
        self.n_text = 77
        self.trace: Optional[Dict[str, torch.Tensor]] = None
        self.text_kv: Dict[int, TextKV] = {}           # per cross-attention site (id of its attn2)
        self.emb_proj: Dict[int, torch.Tensor] = {}    # per ResBlock3D: emb_layers(emb), [F, C] fp32 (nn.openaimodel.EmbProjector)
        self.text_frozen = False                       # text_kv / guided come from StepInvariants (sampler hoisting)
        self.guided: Optional["Act"] = None            # precomputed ControlNet hint-stem output
        self.profile: Optional["RangeProfile"] = None  # UNetModel3D.profile_ranges(): `gemm` observes every A operand; None = off

    def empty(self, shape, dtype, tail_rows: int = 0) -> torch.Tensor:
        """tail_rows: a [rows, C] operand allocated with that many spare rows behind it; the returned [rows, C] view remembers
        the whole allocation (`_pnc_tail`), where a view-band conv puts the neighbours' columns (ViewShard.band_operand)"""
        if not tail_rows:
            return torch.empty(shape, device=self.device, dtype=dtype)
        whole = torch.empty((shape[0] + tail_rows,) + tuple(shape[1:]), device=self.device, dtype=dtype)
        t = whole[:shape[0]]
        t._pnc_tail = whole
        return t

    def band_tail_rows(self, F: int, H: int) -> int:
        """`tail_rows` of a 3x3 conv's operand: room for a view band's two neighbour columns (ViewShard.band_operand)"""
        return 2 * F * H if self.vshard is not None else 0

    def zeros(self, shape, dtype) -> torch.Tensor:
        return torch.zeros(shape, device=self.device, dtype=dtype)

    def lo_plane(self, shape, cls: str, on: bool = True, tail_rows: int = 0) -> Optional[torch.Tensor]:
        """lo plane of an operand of class `cls` (None when the policy does not split that class, or `on` is False); its
        dtype carries the storage format to the kernels"""
        if not (on and getattr(self.prec, cls)):
            return None
        return self.empty(shape, self.prec.lo_dtype(cls), tail_rows)

    def operand(self, shape, cls: Optional[str] = None, tail_rows: int = 0) -> Operand:
        """an uninitialised fp16 operand of class `cls` (None: never split), with its lo plane when the policy splits that class"""
        op = Operand(self.empty(shape, torch.float16, tail_rows), self.lo_plane(shape, cls, tail_rows=tail_rows) if cls else None)
        if self.profile is not None:
            self.profile.note(op.hi, cls)
        return op

    def set_context(self, context: torch.Tensor):
        """context: (B, n_text, D) — tiled over T inside the reference (controlmodel.py:121-122,183-184);
        here every frame of sample b simply reads sample b's keys."""
        B, n, D = context.shape
        if B != self.B:
            raise ValueError(f"context batch {B} != latent batch {self.B} (= frames / num_frames)")
        if n > TEXT_PAD:
            raise ValueError(f"at most {TEXT_PAD} context tokens are supported, got {n}")
        if D % 8:
            raise ValueError("context_dim must be a multiple of 8")
        self.n_text = n
        if self.prec.ctx:
            c32 = torch.zeros((B, TEXT_PAD, D), device=self.device, dtype=torch.float32)
            c32[:, :n] = context.to(device=self.device, dtype=torch.float32)
            self.ctx16 = self.operand((B * TEXT_PAD, D), "ctx")
            self.be.cast_f16(c32, c32.numel(), *self.ctx16)
            return
        c = torch.zeros((B, TEXT_PAD, D), device=self.device, dtype=torch.float16)
        c[:, :n] = context.to(device=self.device, dtype=torch.float16)
        self.ctx16 = Operand(c.view(B * TEXT_PAD, D))
        if self.profile is not None:
            self.profile.note(c, "ctx")


# ----------------------------------------------------------------------------------------------
# range profile (UNetModel3D.profile_ranges): where every GEMM operand of an evaluation sits in fp16's range
# ----------------------------------------------------------------------------------------------
def _f16_from_bits(bits: int) -> float:
    import struct
    return struct.unpack("<e", struct.pack("<H", int(bits) & 0xFFFF))[0]


class RangeProfile:
    """Range statistics of the A operands of every `gemm` of the evaluations it observes, per operand class and per site.

    Owns a device table [slots, 36] of int64 records (pnc_operand_stats_f16, include/panacea_hip.h: binade histogram, maximum,
    lo-plane saturation and NaN counts), zeroed here, and the host map slot -> (operand class, site).  The statistics kernel ADDS to
    a record, so a site that runs in every evaluation, on whichever stream, sums into one slot and nothing synchronises until
    `report()`.  A site is the name of the module that owns the weights within the profiled network (its ControlNet under
    `controlnet.`) plus the weight key; the class is the one the operand was allocated under (Runtime.operand), "unsplit" for
    operands no policy splits.  Remembered per allocation, by storage base pointer, so views and slices resolve; every
    Runtime.operand() overwrites what an earlier allocation at that address left and every evaluation starts from an empty map, so
    a plane that an evaluation did not allocate itself (hoisted StepInvariants) is "unsplit".

    The range monitor (UNetModel3D.lo_clamped) counts the e4m3 QUADS that clamped, process-wide; `lo_saturated` here counts the lo
    ELEMENTS that sit at their format's last code — an upper bound of the clamped elements, per site."""
    WORDS = _hip.STATS_WORDS

    def __init__(self, device, slots: int = 4096):
        self.table = torch.zeros((slots, self.WORDS), dtype=torch.int64, device=device)
        self.sites: List[tuple] = []                  # slot -> (operand class, site)
        self.evaluations = 0
        self.limit: Optional[int] = None              # observe at most that many evaluations (UNetModel3D.profile_ranges)
        self._slot: Dict[tuple, int] = {}
        self._cls: Dict[int, str] = {}                # storage base pointer -> operand class
        self._names: Dict[int, str] = {}              # id(module) -> name within the profiled network

    def bind(self, network: torch.nn.Module):
        """resolve the site names once: named_modules() of the network (its ControlNet is the child `controlnet`)"""
        for name, m in network.named_modules():
            self._names.setdefault(id(m), name)

    def note(self, t: torch.Tensor, cls: Optional[str]):
        """the allocation behind `t` holds an operand of class `cls` (None: an unclassed buffer — forget what lived there before)"""
        ptr = t.untyped_storage().data_ptr()
        if cls is None:
            self._cls.pop(ptr, None)
        else:
            self._cls[ptr] = cls

    def begin_evaluation(self):
        """a new evaluation allocates its operands afresh: drop the classes of the previous one's allocations, whose addresses the
        allocator hands out again (to buffers that never pass through Runtime.operand, too)"""
        self._cls.clear()
        self.evaluations += 1

    def class_of(self, t: torch.Tensor) -> str:
        return self._cls.get(t.untyped_storage().data_ptr(), "unsplit")

    def _site(self, pk, key, site) -> str:
        if key is None or site is not None:
            owner, name = site if site is not None else (None, "stacked")
        else:
            owner, name = getattr(pk, "owner", None), ".".join(str(k) for k in (key if isinstance(key, tuple) else (key,)))
        mod = "" if owner is None else self._names.get(id(owner), type(owner).__name__)
        return f"{mod}.{name}" if mod else name

    def observe(self, rt: Runtime, a: Operand, pk, key, site, kw: dict):
        """one statistics launch over the planes of `a`, on the current stream, ahead of the GEMM that reads them (`kw`: its keywords)"""
        if rt.shard is not None or rt.vshard is not None:
            raise ValueError("the range profile does not run frame- or view-sharded")
        mode = kw.get("a_mode", _hip.A_PLAIN)
        if mode == _hip.A_PLAIN:
            rows, cols = kw["M"], kw["K"]
            ld = kw.get("lda") or cols
        elif mode == _hip.A_CONV3X3:
            # the gather reads every pixel nine times: the profile covers the activation plane once
            c = kw["conv"]
            cols = ld = c["Cin"]
            rows = kw["M"] // (c["Hout"] * c["Wout"]) * c["Hin"] * c["Win"]
        else:
            cols = ld = kw["tconv"]["C"]
            rows = kw["M"]
        k = (self.class_of(a.hi), self._site(pk, key, site))
        slot = self._slot.get(k)
        if slot is None:
            if len(self.sites) >= self.table.shape[0]:
                raise ValueError(f"the range profile holds {self.table.shape[0]} sites; make it with more slots")
            slot = self._slot[k] = len(self.sites)
            self.sites.append(k)
        rt.be.operand_stats(a.hi, a.lo, rows, cols, ld, self.table[slot])

    @staticmethod
    def _stats(words, max_bits: int) -> dict:
        b = [int(v) for v in words[:32]]
        return {"elements": int(words[35]), "max_abs": _f16_from_bits(max_bits), "binades": b, "ge_512": sum(b[24:]),
                "lo_saturated": int(words[33]), "nan": int(words[34]), "inf": b[31] - int(words[34])}

    def report(self) -> dict:
        """-> {"evaluations", "classes": {class: S}, "sites": [{"site", "class", **S}, ...]} with S = {"elements", "max_abs",
        "binades" (32 counts), "ge_512", "lo_saturated", "nan", "inf"}; sites sorted by max_abs, largest first (NaN > Inf > finite).
        One device-to-host copy."""
        n = len(self.sites)
        host = self.table[:n].cpu().tolist() if n else []
        order = sorted(range(n), key=lambda i: (-host[i][32], self.sites[i][1], self.sites[i][0]))
        sites = [{"site": self.sites[i][1], "class": self.sites[i][0], **self._stats(host[i], host[i][32])} for i in order]
        sums: Dict[str, list] = {}
        for (cls, _), w in zip(self.sites, host):
            s = sums.setdefault(cls, [0] * self.WORDS)
            for j in range(self.WORDS):
                s[j] = max(s[j], w[j]) if j == 32 else s[j] + w[j]
        return {"evaluations": self.evaluations, "classes": {c: self._stats(w, w[32]) for c, w in sorted(sums.items())}, "sites": sites}

    def recommend(self, network: torch.nn.Module) -> dict:
        """-> {"policy", "reason", "headroom_binades"}: the cheapest operand policy whose stated range (README, operand policies) holds
        what was observed.  None when an operand is non-finite or at fp16's end: no fp16 policy holds that.  `precise` /
        `precise-ckpt` while no class that `precise` splits reaches |v| = 512 (bins 24..31), `precise-wide` / `precise-full` beyond;
        the second of each pair when the network's weights are not all fp16-representable: checked is `w.half().float() == w` on every
        parameter of `network` with two or more dimensions (the Linear and conv weights every GEMM and small-M linear packs; biases and
        norm parameters stay fp32 on the device and are not looked at), one device synchronisation in all.  `headroom_binades` = 24 - the
        highest occupied binade over those classes: <= 0 is out of range, 1 means the operands already touch [256, 512)."""
        rep = self.report()
        split = [c for c in OPERAND_CLASSES if getattr(PRECISE, c) and c in rep["classes"]]
        top = max((b for c in split for b, cnt in enumerate(rep["classes"][c]["binades"]) if cnt), default=0)
        headroom = 24 - top
        s = rep["sites"][0] if rep["sites"] else None          # (sorted: the worst site first)
        if s is not None and (s["nan"] or s["inf"] or not s["max_abs"] < 65504.0):
            what = "NaN" if s["nan"] else ("Inf" if s["inf"] else "the largest finite fp16 value")
            return {"policy": None, "headroom_binades": headroom,
                    "reason": f"operand class '{s['class']}' at site '{s['site']}' holds {what} (max |v| = {s['max_abs']}): "
                              "no fp16 operand policy can carry it"}
        with torch.no_grad():
            off = [(p.detach().half().float() != p.detach().float()).any() for p in network.parameters() if p.dim() >= 2]
            rounded = not (off and bool(torch.stack(off).any()))
        wtxt = "the GEMM weights are fp16-representable" if rounded else "the GEMM weights are not fp16-representable (an fp32 checkpoint)"
        over = [c for c in split if rep["classes"][c]["ge_512"] > 0]
        if not over:
            return {"policy": "precise" if rounded else "precise-ckpt", "headroom_binades": headroom,
                    "reason": f"every operand class that `precise` splits stays below |v| = 512 ({headroom} binades of headroom); {wtxt}"}
        worst = next(s for s in rep["sites"] if s["class"] in over and s["ge_512"] > 0)
        return {"policy": "precise-wide" if rounded else "precise-full", "headroom_binades": headroom,
                "reason": f"operand class(es) {', '.join(over)} reach |v| >= 512, where an e4m3 lo plane clamps (widest: site "
                          f"'{worst['site']}', max |v| = {worst['max_abs']}); {wtxt}"}


# ----------------------------------------------------------------------------------------------
# weight packing (fp32 checkpoint tensors -> fp16 operand layouts of the kernels)
# ----------------------------------------------------------------------------------------------
def split_lo(w: torch.Tensor, hi16: torch.Tensor) -> torch.Tensor:
    """lo plane of a split weight whose hi plane is `hi16`: fp16((w - hi16) * 2^11), from the fp32 (unrounded) values `w`"""
    return ((w.detach().to(torch.float32) - hi16.to(torch.float32)) * 2048.0).to(torch.float16)


def _cast16(w: torch.Tensor, lo: bool = False) -> torch.Tensor:
    """the fp16 plane of a weight the packers store: fp16(w), or — `lo`, building a lo twin — fp16((w - fp16(w)) * 2^11).
    Elementwise, so every permutation and zero padding the packers apply around it gives the lo plane the layout of its hi plane."""
    w = w.detach()
    hi = w.to(torch.float16)
    return split_lo(w, hi) if lo else hi


def lo_planes(packed):
    """what a lo twin keeps of the result of a `_pack(lo=True)` / `pack(lo=True)`: the fp16 planes, in their places; every other
    tensor (fp32 biases, norm parameters, tables — the hi copies hold them) becomes None; numbers stay"""
    if isinstance(packed, torch.Tensor):
        return packed if packed.dtype == torch.float16 else None
    if isinstance(packed, dict):
        return {k: lo_planes(v) for k, v in packed.items()}
    if isinstance(packed, (list, tuple)):
        return type(packed)(lo_planes(v) for v in packed)
    return packed


# Every fp16 packer takes `lo`: False = the hi plane fp16(w) (the packed weight), True = the lo plane of the same weight in the same
# layout.  The modules' `_pack(lo)` hand it on, so one body describes both planes.
def pk_f16(w: torch.Tensor, lo: bool = False) -> torch.Tensor:
    return _cast16(w, lo).contiguous()


def pk_f32(w: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if w is None else w.detach().to(torch.float32).contiguous()


def pk_linear(w: torch.Tensor, lo: bool = False) -> torch.Tensor:
    """nn.Linear weight [N, K] is already the W[N][K] operand."""
    return pk_f16(w.reshape(w.shape[0], -1), lo)


def pk_lo8(w16: torch.Tensor):
    """e4m3 copy of a packed fp16 weight matrix [N, K] for the lo pass of a precise operand (PncGemmParams.W_lo):
    (bytes uint8 [N, K], E8M0 exponent byte e) with W ~ e4m3 * 2^(e - 127); e puts the tensor maximum in [224, 448]."""
    w = w16.detach().float()
    amax = float(w.abs().max())
    sh = 0 if amax == 0.0 else int(math.floor(math.log2(448.0 / amax)))
    sh = max(-126, min(126, sh))
    q = (w * (2.0 ** sh)).clamp_(-448.0, 448.0).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).contiguous(), 127 - sh


def pk_conv3x3(w: torch.Tensor, cin_pad: Optional[int] = None, lo: bool = False) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> [Cout, 9*Cin_pad].  K order (ky, kx, ci) for narrow inputs; (ci/64, ky, kx, ci%64) when
    Cin_pad % 64 == 0 (see include/panacea_hip.h: the nine taps of a 64-channel slice become adjacent K tiles)."""
    co, ci = w.shape[0], w.shape[1]
    cp = cin_pad or ((ci + 7) // 8 * 8)
    p = torch.zeros((co, 3, 3, cp), device=w.device, dtype=torch.float16)
    p[..., :ci] = _cast16(w.detach().permute(0, 2, 3, 1), lo)
    if cp % 64 == 0:
        p = p.view(co, 9, cp // 64, 64).permute(0, 2, 1, 3)
    return p.reshape(co, 9 * cp).contiguous()


def pk_conv3x3_taps(w: torch.Tensor, lo: bool = False) -> torch.Tensor:
    """[Cout, Cin, 3, 3] -> the linear weight [9*Cout, Cin] whose row (u*3 + v)*Cout + n is W[n, :, u, v]: the nine taps of a 3x3 conv
    as nine column blocks of ONE plain-A GEMM on the conv's source pixels (Upsample at source resolution, pnc_upsample_combine)"""
    return pk_linear(w.detach().permute(2, 3, 0, 1).reshape(9 * w.shape[0], w.shape[1]), lo)


def pk_conv1d(w: torch.Tensor, lo: bool = False) -> torch.Tensor:
    """[Cout, Cin, 3] -> [Cout, 3*Cin] with K ordered (dt, ci); (ci/64, dt, ci%64) when Cin % 64 == 0 (include/panacea_hip.h:
    the three taps of a 64-channel slice become adjacent K tiles)."""
    co, ci = w.shape[0], w.shape[1]
    p = w.detach().permute(0, 2, 1)
    if ci % 64 == 0:
        p = p.reshape(co, 3, ci // 64, 64).permute(0, 2, 1, 3)
    return pk_f16(p.reshape(co, -1), lo)


def pk_geglu(w: torch.Tensor, b: torch.Tensor, lo: bool = False):
    """GEGLU projection [8C, C]: rows [0,4C) are values, [4C,8C) gates (attention.py:97).  Interleave
    32-row blocks (value block j, gate block j) so that the two MFMA column blocks of one wave hold a
    value and its gate at the same accumulator position."""
    n2 = w.shape[0] // 2
    if n2 % 32:
        raise ValueError("GEGLU inner dim must be a multiple of 32")
    wv, wg = w[:n2].view(n2 // 32, 32, -1), w[n2:].view(n2 // 32, 32, -1)
    wi = torch.stack([wv, wg], dim=1).reshape(2 * n2, -1)
    bi = torch.stack([b[:n2].view(-1, 32), b[n2:].view(-1, 32)], dim=1).reshape(-1)
    return pk_f16(wi, lo), pk_f32(bi)


# K order inside every aligned group of 16 on the weight side of the fused chains (include/panacea_hip.h, section 1b): position
# p = 8 g + j of a fragment lane holds K index PERM16[p], so that a C^T accumulator read register by register is the B operand
PERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)


def mfma_a_fragments(w16: torch.Tensor) -> torch.Tensor:
    """[32 R, 16 S] fp16 -> [R, S, 64, 8]: the 1 KB register image (lane l = 32 g + n, 8 halfs) of the A fragment of row block
    R', k-step S' for v_mfma_f32_32x32x16_f16 with the PERM16 K order"""
    R, S = w16.shape[0] // 32, w16.shape[1] // 16
    wp = w16.reshape(R, 32, S, 16)[..., list(PERM16)]
    return wp.reshape(R, 32, S, 2, 8).permute(0, 2, 3, 1, 4).reshape(R, S, 64, 8).contiguous()


class Packed(dict):
    """what Packable.packed() returns: the packed copies, and the way to their lo twins (`lo()`, engine.gemm)"""
    owner = None

    def lo(self) -> dict:
        return self.owner.packed_lo()


class Packable:
    """Mixin for modules that keep kernel-layout copies of their parameters in `self._pk` — and, under a policy that splits the
    weights, the fp16 lo twins of the fp16 ones in `self._pk_lo` (built on first use, dropped together with `_pk`)."""
    _pk: Optional[dict] = None
    _pk_lo: Optional[dict] = None

    def _init_packable(self):
        self._pk = None
        self._pk_lo = None
        self.register_load_state_dict_post_hook(lambda m, _k: m.invalidate_packed())

    def invalidate_packed(self):
        self._pk = None
        self._pk_lo = None

    def _apply(self, fn, *a, **k):          # .to() / .cuda() / .half() move the parameters
        self.invalidate_packed()
        return super()._apply(fn, *a, **k)

    def packed(self) -> dict:
        if self._pk is None:
            with torch.no_grad():
                self._pk = Packed(self._pack())
                self._pk.owner = self
        return self._pk

    def packed_lo(self) -> dict:
        """`_pack(lo=True)`: the LO plane of every fp16 weight, fp16((w - fp16(w)) * 2^11) of the fp32 parameter, under the keys and
        with the permutations and padding of `packed()`; entries that are not fp16 planes are None (engine.lo_planes).  Only a
        policy with `weights` asks for it (engine.gemm, engine.small_linear)."""
        if self._pk_lo is None:
            with torch.no_grad():
                self._pk_lo = lo_planes(self._pack(lo=True))
        return self._pk_lo

    def _pack(self, lo: bool = False) -> dict:                # pragma: no cover
        raise NotImplementedError


def invalidate_all(module: torch.nn.Module):
    """Drop every packed copy below `module` (call after modifying parameters in place)."""
    for m in module.modules():
        if isinstance(m, Packable):
            m.invalidate_packed()


# ----------------------------------------------------------------------------------------------
# op helpers: allocate the output, call the backend
# ----------------------------------------------------------------------------------------------
def _ppc(npix: int) -> int:
    """Pixels per GroupNorm chunk.  <= 128 on the denoiser's grids; image-resolution maps (first-stage decoder:
    256x3072) get larger chunks so that the per-frame chunk count — which every apply block re-combines — stays <= 256."""
    return max(16, min(128, npix // 48), -(-npix // 256))


GN_EPILOGUE_CHUNK = 64      # pixels per record of PncGemmParams.gn_part (the temporal conv's 64-row wave blocks)
GN_FROM_EPILOGUE = True     # False (bench.py --no-gn-epilogue, A/B): every spatial GroupNorm launches its own statistics kernel
EMB_BATCH = os.environ.get("PNC_EMB_BATCH", "1") != "0"      # A/B: "0" = one emb_layers launch per ResBlock3D (rounds 1-4)
TEXTKV_ONE_GEMM = os.environ.get("PNC_TEXTKV_ONE_GEMM", "1") != "0"      # A/B: "0" = text K/V of a network as one GEMM per width
# A/B: "0" = the denoiser's Upsample convs as one 9-tap implicit GEMM at the OUTPUT resolution (rounds 1-6); default: the nine taps as
# a plain-A GEMM on the source pixels + pnc_upsample_combine (nn.openaimodel.Upsample)
UPSAMPLE_SOURCE_RES = os.environ.get("PNC_UPSAMPLE_SOURCE_RES", "1") != "0"
UPSAMPLE_CHUNK_FRAMES = int(os.environ.get("PNC_UPSAMPLE_CHUNK_FRAMES", "0"))      # sweeps / tests: > 0 forces the frames per chunk


def upsample_chunk_frames(F: int, Hin: int, Win: int, Cout: int) -> int:
    """Frames per GEMM + combine round of an Upsample at source resolution: a pure function of the shapes.  The sweep over 1, 2, 4, 8
    and 16 frames (profiles/upsample_source_res.md) shows no chunk size that beats all 16 frames at once by more than the run-to-run
    spread at the two large sites — a P that fits the Infinity Cache speeds the combine up and slows the GEMM down by as much — and
    small chunks lose up to 3x at the small one, so the rule is the whole batch, cut only where P (36 * Cout bytes per source pixel)
    would pass 2 GiB (the 16-frame level 1->0 site holds 1.13 GB)."""
    if UPSAMPLE_CHUNK_FRAMES > 0:
        return min(F, UPSAMPLE_CHUNK_FRAMES)
    return max(1, min(F, (1 << 31) // (36 * Cout * Hin * Win)))


def gn_records(rt: Runtime, F: int, N: int) -> Optional[torch.Tensor]:
    """the record buffer a temporal conv fills for the GroupNorm of its output (`gemm(..., gn_part=)`, then `gn_spatial(..., part=)`)"""
    if not GN_FROM_EPILOGUE:
        return None
    return rt.empty((F * (-(-N // GN_EPILOGUE_CHUNK)) * 32 * 3,), torch.float32)


def gn_spatial(rt: Runtime, x32: torch.Tensor, F: int, N: int, C: int, gamma, beta, eps: float, silu: bool,
               split: Optional[str] = None, tail_rows: int = 0, part: Optional[torch.Tensor] = None):
    """-> Operand.  `split`: the operand class of the output ("gn_stt" | "gn_res" | "gn_head"); its lo plane is None unless the
    policy splits that class (precise operand for the consumer GEMM).  `tail_rows`: Runtime.empty's, for an output that feeds a
    3x3 conv of a view band.  `part`: the statistics records of x32 when its producer wrote them (`gn_records`): no statistics launch."""
    if C % 64:
        raise ValueError(f"GroupNorm(32) kernels need C % 64 == 0, got {C}")
    ppc = _ppc(N)
    y, ylo = out = rt.operand((F * N, C), split, tail_rows)
    if part is None:
        nrec = (N + ppc - 1) // ppc
        part = rt.empty((F * nrec * 32 * 3,), torch.float32)
        # (launching the pair per Infinity-Cache sized panel of frames was measured: slower, profiles/round3/ab_two_wg_and_mall_panels_r3c.txt)
        rt.be.groupnorm_stats(x32, C, F, N, C, ppc, part)
    else:
        nrec = part.numel() // (F * 96)          # the producer's records per frame (GEMM epilogues: 64-pixel chunks; the concat: _ppc(N))
    vs = rt.vshard
    if vs is not None and tail_rows and vs.fused_halo and tail_rows % (2 * F) == 0 and N % (tail_rows // (2 * F)) == 0:
        # GroupNorm -> 3x3 conv of a view band: records + the neighbours' raw edge columns in ONE exchange (ViewShard.stats_and_halo)
        H = tail_rows // (2 * F)
        W = N // H
        x4 = x32.view(F, H, W, C)
        allp, fl, fr = vs.stats_and_halo(part, x4[:, :, 0], x4[:, :, W - 1], F, nrec)
        comb = torch.empty((F * nrec * 96,), device=x32.device, dtype=torch.float32)
        rt.be.groupnorm_combine(allp, vs.G if vs.group is not None else 1, F, nrec, comb)
        rt.be.groupnorm_apply(x32, C, F, N, C, ppc, comb, gamma, beta, eps, silu, y, C, ylo, n_records=nrec)
        # the two received columns, normalised by the same kernel with the same combined records, land in the operand's tail
        # [2][F][H][C] (PncGemmParams.x_halo_off); zeros at the ends of the panorama — the conv's own padding
        for side, raw in ((0, fl), (1, fr)):
            for pl in (y, ylo):
                if pl is None:
                    continue
                t = pl._pnc_tail[F * N + side * F * H: F * N + (side + 1) * F * H]
                if raw is None:
                    t.zero_()
            if raw is not None:
                yt = y._pnc_tail[F * N + side * F * H: F * N + (side + 1) * F * H]
                lt = None if ylo is None else ylo._pnc_tail[F * N + side * F * H: F * N + (side + 1) * F * H]
                rt.be.groupnorm_apply(raw.reshape(F * H, C).contiguous(), C, F, H, C, ppc, comb, gamma, beta, eps, silu, yt, C, lt,
                                      n_records=nrec)
        for pl in out.planes():
            pl._pnc_halo_ready = True
        return out
    if vs is not None:           # statistics of the whole panorama, not of this rank's band of views
        part = vs.combine_stats(part, F, nrec, rt.be)
    rt.be.groupnorm_apply(x32, C, F, N, C, ppc, part, gamma, beta, eps, silu, y, C, ylo, n_records=nrec)
    return out


def gn_temporal(rt: Runtime, x32: torch.Tensor, N: int, C: int, gamma, beta, eps: float) -> Operand:
    """Operand class `gnt`.  x32 holds ALL T frames of N pixels per sample (the resident layout, or the pixel-sharded layout of a
    FrameShard with N = pixels per rank)."""
    y = rt.operand((rt.B * rt.T * N, C), "gnt")
    rt.be.groupnorm_temporal_silu(x32, rt.B, rt.T, N, C, gamma, beta, eps, *y)
    return y


def gn_temporal_sharded(rt: Runtime, sh: "FrameShard", x32: torch.Tensor, N: int, C: int, gamma, beta, eps: float) -> Operand:
    """The temporal GroupNorm + SiLU of a frame-sharded run in the FRAME layout: x32 holds this rank's T_local frames of N pixels per
    sample.  -> the operand in the (T_local + 2)-frame layout of the temporal conv (PncGemmParams.t_halo), halo frames filled."""
    B, Tl = rt.B, rt.T_local
    stats = rt.empty((B * N * 64,), torch.float32)
    rt.be.groupnorm_temporal_part(x32, B, Tl, N, C, gamma, beta, eps, stats, 1, rt.T)
    sh.allreduce_sum(stats)
    y = rt.operand((B * (Tl + 2) * N, C), "gnt")
    rt.be.groupnorm_temporal_part(x32, B, Tl, N, C, gamma, beta, eps, stats, 2, rt.T, y.hi, y.lo, 1)
    sh.halo_frames(y.planes(), B, Tl)
    return y


class TemporalLayout(NamedTuple):
    """Where the T frames of a pixel are when a ResBlock3D temporal site (per pixel: GroupNorm over (C/32, T) + conv1d over T) runs on
    the fp32 stream h [F*N, C] of the frame layout: all that the layouts differ in (nn.openaimodel.ResBlock3D._temporal_site)"""
    emb_all: bool         # the epilogue's per-frame rows are those of ALL B*T frames (rt.emb_all): the batched EmbProjector is not read
    operand: Callable     # (rt, started, N, C, gamma, beta, eps) -> (h in the conv's layout, the conv's normalised Operand)
    tconv: Callable       # (rt, C, N) -> the conv's geometry: B * T * Npix rows, Npix of them per row of the row bias
    start: Callable = lambda rt, h, N: h    # -> h on its way to the conv's layout (`started`): what is enqueued before `operand` runs under the transfer
    # (rt, h in the conv's layout, N) -> h; None: the conv's rows ARE the frame layout's and its epilogue takes the skip path, fp16 output, gn_records
    home: Optional[Callable] = None


# all T frames are this rank's: the site runs on h as it lies
RESIDENT = TemporalLayout(False, lambda rt, h, *gn: (h, gn_temporal(rt, h, *gn)), lambda rt, C, N: dict(C=C, T=rt.T, Npix=N))
# FrameShard(resblock="halo"): h stays; the GroupNorm's sums are added over the frame group, the operand gets ONE frame per neighbour rank
HALO = TemporalLayout(False, lambda rt, h, *gn: (h, gn_temporal_sharded(rt, rt.shard, h, *gn)),
                      lambda rt, C, N: dict(C=C, T=rt.T_local, Npix=N, halo=1))
# FrameShard(resblock="transpose"): h goes to the pixel sharding (all T frames of N / G pixels) and back
TRANSPOSE = TemporalLayout(True, lambda rt, pend, N, *gn: (hp := pend.result(), gn_temporal(rt, hp, N // rt.shard.G, *gn)),
                           lambda rt, C, N: dict(C=C, T=rt.T, Npix=N // rt.shard.G),
                           lambda rt, h, N: rt.shard.to_pixels_start(h, rt.B, N), lambda rt, hp, N: rt.shard.to_frames(hp, rt.B, N))


def temporal_layout(rt: Runtime) -> TemporalLayout:
    return RESIDENT if rt.shard is None else HALO if rt.shard.resblock == "halo" else TRANSPOSE


def layer_norm(rt: Runtime, x32: torch.Tensor, M: int, C: int, gamma, beta) -> Operand:
    """operand class `ln`"""
    y = rt.operand((M, C), "ln")
    rt.be.layernorm(x32, C, M, C, gamma, beta, 1e-5, y.hi, C, y.lo)
    return y


def gemm(rt: Runtime, a: Operand, pk, key, out: Optional[Operand] = None, *, w_lo=None, site=None, **kw):
    """THE launch of a GEMM on an operand: a @ W^T with the epilogue `kw` (the keywords of the backend's `gemm`), fp16 output into
    `out`.  W = pk[key]; `key` may be a path into `pk` (a tuple), and an entry that is a (weight, bias) pair gives both.  What goes
    with the planes of `a` and `out` is decided here and nowhere else:
      a.lo is e4m3   the e4m3 copy of W for the lo pass (pk_lo8), packed on first use and kept in `pk` next to the fp16 weights;
      a.lo is fp16   the fp16 lo twin of W when the policy splits the weights (Packable.packed_lo, built on first use), else nothing;
      no a.lo        nothing.
    Under a policy that hands the twin over BESIDE the launch (`precise-ckpt`, weights_beside) the fp16 lo twin goes along as `w_lo16`
    for every state of a.lo, next to whatever the list above says.
    `key=None`: `pk` is W itself, a stacked matrix that is no Packable's (TextKVProjector, EmbProjector), and `w_lo` its lo twin — used
    under the same conditions as a module's.  `site` = (owning network, fixed name) names such a matrix in a range profile; with a key it
    names the launch of a SECOND packing of a module's weight (Upsample's `w9`) like the launch of the first, (module, "w")).
    With a range profile on (rt.profile, UNetModel3D.profile_ranges) the planes of `a` are observed ahead of the launch, on its stream."""
    w = pk
    if key is not None:
        for k in key if isinstance(key, tuple) else (key,):
            w = w[k]
        if isinstance(w, tuple):
            w, b = w
            if kw.get("bias") is None:
                kw["bias"] = b
    if rt.prec.beside:
        kw["w_lo16"] = _lo_twin(pk, key) if key is not None else w_lo
        if kw["w_lo16"] is None:
            raise ValueError("a stacked weight matrix needs its lo twin (w_lo=) under a policy that splits the weights")
        w_lo = None
    if a.lo is None:
        w_lo = None
    elif a.lo.dtype == torch.uint8:
        k8 = (key, "lo8")
        if k8 not in pk:
            pk[k8] = pk_lo8(w)
        w_lo = pk[k8]
    elif not rt.prec.weights or rt.prec.beside:
        w_lo = None
    elif key is not None:
        w_lo = _lo_twin(pk, key)
    if out is not None:
        kw["out16"] = out.hi
        if out.lo is not None:
            kw["out16_lo"] = out.lo
    if rt.profile is not None:
        rt.profile.observe(rt, a, pk, key, site, kw)
    rt.be.gemm(a.hi, w, a16_lo=a.lo, w_lo=w_lo, **kw)


def _lo_twin(pk: "Packed", key) -> torch.Tensor:
    t = pk.lo()
    for k in key if isinstance(key, tuple) else (key,):
        t = t[k]
    return t[0] if isinstance(t, tuple) else t


def small_linear(rt: Runtime, a32: torch.Tensor, pk: "Packed", wkey, bkey, M: int, N: int, K: int,
                 silu_in=False, silu_out=False) -> torch.Tensor:
    """fp32-activation linear pk[wkey], pk[bkey] for the (frames x 1280) time-embedding path; rows in chunks of 16.  Under a policy
    that splits the weights the kernel joins pk[wkey] with its lo twin in fp32."""
    out = rt.empty((M, N), torch.float32)
    kw = dict(w_lo=_lo_twin(pk, wkey)) if rt.prec.weights else {}
    for m0 in range(0, M, 16):
        mm = min(16, M - m0)
        rt.be.linear_smallm(a32[m0:], K, pk[wkey], pk[bkey], out[m0:], N, mm, N, K, silu_in, silu_out, **kw)
    return out


_FREQS: Dict[tuple, torch.Tensor] = {}


def timestep_freqs(dim: int, device) -> torch.Tensor:
    """exp(-ln(10000) * i / half), tabulated in fp32 on the host exactly like util.py:236-241."""
    key = (dim, str(device))
    if key not in _FREQS:
        half = dim // 2
        f = torch.exp(-math.log(10000.0) * torch.arange(0, half, dtype=torch.float32) / half)
        _FREQS[key] = f.to(device)
    return _FREQS[key]


def temporal_pos_table(T: int, C: int) -> torch.Tensor:
    """The reference's temporal position table as it actually evaluates (attention.py:1140-1159): the
    frequency vector is truncated to int64, leaving col 0 = sin(p), col 1 = cos(p), other even columns
    0 and odd columns 1.  Built once per (T, C) instead of on every forward."""
    p = torch.arange(T, dtype=torch.float32)
    tab = torch.zeros(T, C, dtype=torch.float32)
    tab[:, 1::2] = 1.0
    tab[:, 0] = torch.sin(p)
    tab[:, 1] = torch.cos(p)
    return tab
