"""Execution runtime of the MI355X denoising path: activation handles, weight packing and the
op helpers the module mirrors in `panacea_amd/nn/` are written against.

Data layout.  Activations never leave ONE resident layout: channels-last token
matrices, row m = (frame f, y, x), columns = channels.  The six camera views are a stride along x,
frames a stride along the leading dimension, so intra-view / cross-view / temporal attention, 3x3
convs and temporal convs all address the same buffer — none of the reference's NCHW <-> (b hw c) <->
(bhw t c) copies (attention.py:1069-1134, openaimodel.py:505-515) exist here.  The residual stream is
fp32 (`Act.f32`); every contraction operand is fp16 (`Act.f16`, produced by the norm kernels or by a
GEMM epilogue).

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
from typing import Dict, List, NamedTuple, Optional

import torch

from . import hip as _hip

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


class FrameShard:
    """The T frames of every sample sharded over the G ranks of a process group: rank g of the group
    holds frames [g*T/G, (g+1)*T/G) of each sample — whole panoramic frames, so every spatial op (3x3 convs, spatial
    GroupNorm, intra-/cross-view attention) stays local.  The cross-frame couplings of the path,
        ResBlock3D   temporal GroupNorm + conv1d            (openaimodel.py:505-515, 533-539)
        STT          temporal transformer branch            (attention.py:1106-1134)
    are all POINTWISE PER PIXEL across frames, so they run in the transposed sharding: all T frames of N/G pixels per
    rank.  `to_pixels` / `to_frames` are the two exchanges (one all-to-all each: a rank sends (G-1)/G of its slab and
    receives as much — half the received bytes of all-gathering the slab, and the unmodified kernels run on both sides);
    `gather_rows` all-gathers tiny per-frame rows (the timestep embedding).  RCCL over xGMI on MI355X ("nccl"), gloo in
    the CPU tests; `group=None` with G = 1 is the loop-back used by the single-device GPU test."""

    def __init__(self, G: int, index: int, group=None, resblock: str = "halo"):
        if G < 1 or not (0 <= index < G):
            raise ValueError(f"bad frame shard {index} of {G}")
        if G > 1 and group is None:
            raise ValueError("a frame shard over more than one rank needs its process group")
        if resblock not in ("halo", "transpose"):
            raise ValueError("resblock: 'halo' (statistics all-reduce + neighbour frames, round 4) or 'transpose' (round 2: the "
                             "fp32 stream to the pixel sharding and back)")
        self.G, self.index, self.group, self.resblock = G, index, group, resblock
        self.bytes_sent = 0                       # accounting for bench / DESIGN §9 (this rank, since construction)
        self.exchanges = 0

    def _a2a(self, send: torch.Tensor):
        """-> (recv, work): work is None when the exchange has completed (loop-back), else the handle of the collective running
        on the communicator's own stream — `work.wait()` orders the CURRENT stream behind it"""
        self.exchanges += 1
        self.bytes_sent += send.numel() * send.element_size() * (self.G - 1) // self.G
        if self.group is None:
            return send.clone(), None
        import torch.distributed as dist
        if dist.get_backend(self.group) == "gloo" and send.device.type != "cpu":
            # two processes on one GPU (tests): gloo moves host memory — staged and completed here
            host = send.cpu()
            got = torch.empty_like(host)
            dist.all_to_all_single(got, host, group=self.group)
            return got.to(send.device), None
        recv = torch.empty_like(send)
        return recv, dist.all_to_all_single(recv, send, group=self.group, async_op=True)

    class Pending:
        """An exchange in flight.  Kernels enqueued between `*_start()` and `result()` run UNDER the transfer (RCCL executes
        the collective on its own stream; the compute stream only waits in `result()`): the independent work every ResBlock3D
        site has — the skip 1x1 conv and the `emb_layers` linear — goes there."""

        def __init__(self, recv, work, finish):
            self._recv, self._work, self._finish = recv, work, finish

        def result(self) -> torch.Tensor:
            if self._work is not None:
                self._work.wait()
                self._work = None
            return self._finish(self._recv)

    def to_pixels_start(self, x: torch.Tensor, B: int, N: int) -> "FrameShard.Pending":
        G = self.G
        if N % G:
            raise ValueError(f"{N} pixels per frame do not split over {G} frame groups")
        C = x.shape[-1]
        Tl, Np = x.shape[0] // (B * N), N // G
        send = x.view(B, Tl, G, Np, C).permute(2, 0, 1, 3, 4).contiguous()      # [dest pixel group, b, t_l, p, c]
        recv, work = self._a2a(send)                                            # [src frame group, b, t_l, p, c]
        return FrameShard.Pending(recv, work, lambda r: r.permute(1, 0, 2, 3, 4).contiguous().view(B * G * Tl * Np, C))

    def to_pixels(self, x: torch.Tensor, B: int, N: int) -> torch.Tensor:
        """[B*T_l*N, C] rows (b, t_local, p) -> [B*T*(N/G), C] rows (b, t, p_local)"""
        return self.to_pixels_start(x, B, N).result()

    def to_frames(self, x: torch.Tensor, B: int, N: int) -> torch.Tensor:
        """inverse of to_pixels: [B*T*(N/G), C] -> [B*T_l*N, C]"""
        G = self.G
        C = x.shape[-1]
        Np = N // G
        Tl = x.shape[0] // (B * G * Np)
        send = x.view(B, G, Tl, Np, C).permute(1, 0, 2, 3, 4).contiguous()      # [dest frame group, b, t_l, p, c]
        recv, work = self._a2a(send)                                            # [src pixel group, b, t_l, p, c]
        if work is not None:
            work.wait()
        return recv.permute(1, 2, 0, 3, 4).contiguous().view(B * Tl * N, C)

    # ---- round 6: the planes of ONE operand (fp16 hi + e4m3 / fp16 lo) travel in ONE exchange — row-wise byte concatenation, one
    #      all_to_all instead of one per plane: the STT temporal branch goes from 4 to 2 exchanges per site (92 -> 46 per evaluation)
    @staticmethod
    def _pack_planes(planes):
        keep = [p for p in planes if p is not None]
        rows = keep[0].shape[0]
        return torch.cat([p.contiguous().view(rows, -1).view(torch.uint8) for p in keep], dim=1), [(p.dtype, p.shape[1]) for p in keep]

    @staticmethod
    def _unpack_planes(buf, spec, planes):
        out, o, it = [], 0, iter(spec)
        for p in planes:
            if p is None:
                out.append(None)
                continue
            dt, C = next(it)
            nb = C * torch.empty((), dtype=dt).element_size()
            out.append(buf[:, o:o + nb].contiguous().view(dt).view(buf.shape[0], C))
            o += nb
        return out

    def to_pixels_planes(self, planes, B: int, N: int):
        """`to_pixels` of several planes of one operand (None entries pass through) in one exchange"""
        buf, spec = self._pack_planes(planes)
        return self._unpack_planes(self.to_pixels(buf, B, N), spec, planes)

    def to_frames_planes(self, planes, B: int, N: int):
        buf, spec = self._pack_planes(planes)
        return self._unpack_planes(self.to_frames(buf, B, N), spec, planes)

    # ---- round 4: the ResBlock3D temporal sites WITHOUT moving the fp32 stream.  The temporal GroupNorm only
    #      needs per-(pixel, group) sums over all T frames: every rank reduces its frames, the frame group adds the partial sums
    #      (256 B per pixel, whatever C and T); the k = 3 temporal conv only needs ONE frame of the normalised fp16 operand from
    #      each neighbour rank.  Sent per pixel-channel and site at G = 4: ~5.7 B instead of 12 (fp32 h to the pixel layout and back).
    def allreduce_sum(self, t: torch.Tensor) -> torch.Tensor:
        """in-place sum over the frame group (the temporal GroupNorm's partial sums)"""
        self.exchanges += 1
        if self.group is None:          # loop-back (G = 1 without a process group)
            return t
        import torch.distributed as dist
        host = dist.get_backend(self.group) == "gloo" and t.device.type != "cpu"
        buf = t.cpu() if host else t
        dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
        self.bytes_sent += 2 * t.numel() * t.element_size() * (self.G - 1) // self.G          # ring all-reduce: 2 (G-1)/G of the payload
        if host:
            t.copy_(buf)
        return t

    def halo_frames(self, planes, B: int, Tl: int):
        """planes: tensors of [B, Tl + 2, N, C] (the (T + 2)-frame layout of PncGemmParams.t_halo; hi and lo plane of one operand)
        whose frames 1 .. Tl are this rank's.  Fills frame 0 with the previous rank's last frame and frame Tl + 1 with the next
        rank's first frame — zeros at the two ends of the clip (the conv's own zero padding in time, openaimodel.py:418,469).  One
        all_to_all_single inside the frame group (split sizes name the one or two neighbours; nothing for the other ranks)."""
        G, me = self.G, self.index
        views = [p.view(B, Tl + 2, -1) for p in planes]
        to_prev = [v[:, 1] for v in views]
        to_next = [v[:, Tl] for v in views]
        self.exchanges += 1
        if G == 1:
            for v in views:
                v[:, 0].zero_()
                v[:, Tl + 1].zero_()
            if self.group is None:
                return
        dev = planes[0].device

        def pack(ts):
            return torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in ts])
        bp, bn = pack(to_prev), pack(to_next)
        nb = bp.numel()
        has_prev, has_next = me > 0, me < G - 1
        in_split, out_split = [0] * G, [0] * G
        parts = []
        if has_prev:
            in_split[me - 1] = out_split[me - 1] = nb
            parts.append(bp)                             # (rank me - 1 < me + 1: already ordered by destination)
        if has_next:
            in_split[me + 1] = out_split[me + 1] = nb
            parts.append(bn)
        send = torch.cat(parts) if parts else bp[:0]
        self.bytes_sent += send.numel()
        import torch.distributed as dist
        stage = dist.get_backend(self.group) == "gloo" and dev.type != "cpu"
        if stage:
            send = send.cpu()
        recv = torch.empty(sum(out_split), dtype=torch.uint8, device=send.device)
        dist.all_to_all_single(recv, send, output_split_sizes=out_split, input_split_sizes=in_split, group=self.group)
        if stage:
            recv = recv.to(dev)
        o = 0
        from_prev = recv[o:o + nb] if has_prev else None
        o += nb if has_prev else 0
        from_next = recv[o:o + nb] if has_next else None
        for slot, buf in ((0, from_prev), (Tl + 1, from_next)):
            off = 0
            for v in views:
                n1 = v[:, slot].numel() * v.element_size()
                if buf is None:
                    v[:, slot].zero_()
                else:
                    v[:, slot] = buf[off:off + n1].view(v.dtype).view(v[:, slot].shape)
                off += n1

    def gather_rows(self, x: torch.Tensor, B: int) -> torch.Tensor:
        """[B*T_l, D] per-frame rows -> [B*T, D] (frames of a sample in global order)"""
        G = self.G
        D = x.shape[-1]
        Tl = x.shape[0] // B
        if self.group is None:
            return x.clone()
        import torch.distributed as dist
        host = dist.get_backend(self.group) == "gloo" and x.device.type != "cpu"          # (two processes on one GPU: tests)
        send = x.contiguous().cpu() if host else x.contiguous()
        parts = [torch.empty_like(send) for _ in range(G)]
        dist.all_gather(parts, send, group=self.group)
        return torch.stack([p.view(B, Tl, D) for p in parts], dim=1).reshape(B * G * Tl, D).to(x.device)


class ViewShard:
    """The six camera views of every panoramic frame sharded over the G in {2, 3, 6} ranks of a process group: rank g holds
    views [g*6/G, (g+1)*6/G) — a band of W/G columns of every map, at every level.  Per pixel, per frame and per view work
    (1x1 convs, the temporal GroupNorm / conv1d / attention, LayerNorm, feed-forward, text attention, intra-view attention:
    attention.py:382-489) stays local.  What couples the views:

        3x3 convs (all)              one halo column per side from the neighbour band         `band_operand`
        spatial GroupNorm(32)        per-(frame, group) statistics over the whole panorama     `combine_stats`
        cross-view attention         keys / values of the two neighbouring views (circular:    `halo_views`
                                     attention.py:545-559; view 5 attends view 4 only)

    Neighbour exchanges are point-to-point (one xGMI link per neighbour pair on MI355X); the statistics are one tiny
    all-gather.  With a "gloo" group, device tensors are staged through host memory (the two-process tests on one GPU)."""
    VIEWS = 6

    def __init__(self, G: int, index: int, group=None):
        if G not in (1, 2, 3, 6) or not (0 <= index < G):
            raise ValueError(f"bad view shard {index} of {G}: the six views split over 1 (loop-back), 2, 3 or 6 ranks")
        if G > 1 and group is None:
            raise ValueError("a view shard over more than one rank needs its process group")
        self.G, self.index, self.group = G, index, group
        self.n_local = self.VIEWS // G
        self.first = index * self.n_local              # global index of this rank's first view
        self.bytes_sent = 0
        self.exchanges = 0
        self._host = False
        if group is not None:
            import torch.distributed as dist
            self._host = dist.get_backend(group) == "gloo"

    # -- circular neighbour exchange: every tensor of `to_left` goes to the left neighbour, `to_right` to the right one;
    #    returns (from_left, from_right) = what the neighbours sent towards this rank.
    #    ONE all_to_all_single inside the view group per exchange (round 4): the tensors of a direction travel as one byte
    #    message, the split sizes say who gets what (nothing for a rank that is no neighbour), and nothing depends on message
    #    tags or on the posting order of point-to-point operations — RCCL ignores tags and matches same-peer sends by order,
    #    which is what the first form (batch_isend_irecv with direction tags) silently relied on at G = 2, where both
    #    neighbours are the same peer (VERDICT r3 missing 2).  G = 1 (`group=None`, or a one-rank group): the band is the
    #    whole panorama and its own circular neighbour — the loop-back that drives every exchange site on one device.
    def _exchange(self, to_left, to_right):
        shapes_l = [(t.shape, t.dtype) for t in to_left]
        shapes_r = [(t.shape, t.dtype) for t in to_right]

        def pack(ts):
            return torch.cat([t.contiguous().view(-1).view(torch.uint8) for t in ts])

        def unpack(buf, shapes):
            out, o = [], 0
            for shp, dt in shapes:
                nb = int(torch.Size(shp).numel()) * torch.empty((), dtype=dt).element_size()
                out.append(buf[o:o + nb].view(dt).view(shp))
                o += nb
            return out
        from_left, from_right = self._exchange_bytes(pack(to_left), pack(to_right))
        return unpack(from_left, shapes_r), unpack(from_right, shapes_l)

    def _exchange_bytes(self, bl: torch.Tensor, br: torch.Tensor):
        """bl / br: flat uint8 messages (freshly packed — never aliased by the caller afterwards) for the left / right neighbour ->
        (bytes from the left neighbour = its `br`, bytes from the right neighbour = its `bl`)"""
        dev = bl.device
        nl, nr = bl.numel(), br.numel()
        self.exchanges += 1
        self.bytes_sent += (nl + nr) if self.G > 1 else 0
        G, me = self.G, self.index
        if self.group is None:
            # my left neighbour is me: what arrives from the left is what I sent to the right, and vice versa
            return br, bl
        import torch.distributed as dist
        left, right = (me - 1) % G, (me + 1) % G
        in_split, out_split = [0] * G, [0] * G
        if G == 1:
            send, in_split[0], out_split[0] = torch.cat([bl, br]), nl + nr, nl + nr
        elif G == 2:
            # both neighbours are the one peer: it gets [to_left | to_right] as one message
            send = torch.cat([bl, br])
            in_split[left] = out_split[left] = nl + nr
        else:
            send = torch.cat([bl, br] if left < right else [br, bl])          # ordered by destination rank
            in_split[left], in_split[right] = nl, nr
            out_split[left], out_split[right] = nr, nl                         # the left neighbour sends its to_right batch
        stage = self._host and dev.type != "cpu"
        if stage:
            send = send.cpu()
        recv = torch.empty(sum(out_split), dtype=torch.uint8, device=send.device)
        dist.all_to_all_single(recv, send, output_split_sizes=out_split, input_split_sizes=in_split, group=self.group)
        if stage:
            recv = recv.to(dev)
        if G <= 2:
            # the peer's (or, G = 1, my own) [to_left | to_right]: its to_left batch arrives from the right
            from_right, from_left = recv[:nl], recv[nl:]
        elif left < right:
            from_left, from_right = recv[:nr], recv[nr:]
        else:
            from_right, from_left = recv[:nl], recv[nl:]
        return from_left, from_right

    def band_operand(self, rt, planes, F: int, H: int, W: int, C: int):
        """planes: [F*H*W, C] operand planes of this band (hi and lo plane of one conv operand) -> (planes', x_halo_off): each
        plane in ONE allocation [F*H*W + 2*F*H, C] whose tail holds image column -1 (from the left neighbour: [F][H][C]) and
        column W (from the right neighbour) of every row — zeros at the two ends of the panorama, the conv's own padding — and the
        element offset of that tail, PncGemmParams.x_halo_off.  The 3x3 gathers read the tail instead of padding (no widened copy of
        the band, no window copy of the conv's output).  A plane that came from Runtime.empty(..., tail_rows >= 2*F*H) is used in
        place; any other is copied once into such an allocation."""
        M, tail = F * H * W, 2 * F * H
        if all(getattr(p, "_pnc_halo_ready", False) and getattr(p, "_pnc_tail", None) is not None for p in planes):
            # round 6: the GroupNorm that wrote this operand already exchanged the neighbours' RAW edge columns together with its
            # statistics records (stats_and_halo) and normalised them into the tail: no second exchange in front of the conv
            return [p._pnc_tail for p in planes], M * C
        # the planes' edge columns travel as ONE byte message per direction, row (f, y) = [plane 0's C values | plane 1's | ...]:
        # one gather launch per direction whatever the number of planes
        maps = [p.view(F, H, W, C).view(torch.uint8) for p in planes]
        widths = [m.shape[-1] for m in maps]
        bl = torch.cat([m[:, :, :1] for m in maps], dim=-1).view(-1)
        br = torch.cat([m[:, :, -1:] for m in maps], dim=-1).view(-1)
        fl, fr = self._exchange_bytes(bl, br)
        fl, fr = fl.view(F, H, sum(widths)), fr.view(F, H, sum(widths))
        out, o = [], 0
        for p, wb in zip(planes, widths):
            whole = getattr(p, "_pnc_tail", None)
            if whole is None or whole.shape[0] < M + tail or whole.data_ptr() != p.data_ptr():
                whole = rt.empty((M + tail, C), p.dtype)
                whole[:M] = p
            cols = whole[M:M + tail].view(2, F, H, C)
            if self.index > 0:
                cols[0] = fl[:, :, o:o + wb].view(p.dtype)
            else:
                cols[0].zero_()
            if self.index < self.G - 1:
                cols[1] = fr[:, :, o:o + wb].view(p.dtype)
            else:
                cols[1].zero_()
            out.append(whole)
            o += wb
        return out, M * C

    def combine_stats(self, part: torch.Tensor, F: int, nchunk: int, be=None) -> torch.Tensor:
        """part: the {n, mean, M2} records [F, nchunk, 32, 3] of this band (pnc_groupnorm_stats) -> records of the same shape
        whose Chan combination is the statistics of the whole panorama: slot 0 of every frame holds the combined record, the
        other slots are empty ({0, 0, 0} leaves the combination unchanged), so `pnc_groupnorm_apply` runs unmodified.  The
        records of the G bands are all-gathered (96 floats per frame and chunk) and combined by ONE small kernel
        (`pnc_groupnorm_combine`, fp32 Chan updates in the fixed order (band, chunk) — the same arithmetic the apply kernel
        uses; round 3 did this with ten float64 torch ops per site, 134 sites per step)."""
        be = be or backend()
        mine = part.view(-1)[: F * nchunk * 96]
        if self.group is None:
            allp = mine
        else:
            import torch.distributed as dist
            send = mine.cpu() if self._host and mine.device.type != "cpu" else mine
            allp = torch.empty(self.G * send.numel(), dtype=send.dtype, device=send.device)
            dist.all_gather_into_tensor(allp, send.contiguous(), group=self.group)
            allp = allp.to(part.device)
            self.bytes_sent += send.numel() * 4 * (self.G - 1)
        out = torch.empty_like(mine)
        be.groupnorm_combine(allp, self.G, F, nchunk, out)
        self.exchanges += 1
        return out

    # ---- round 6: GroupNorm -> 3x3 conv of a view band in ONE exchange instead of two.  Rounds 3-5 all-gathered
    #      the statistics records, normalised, and then exchanged the NORMALISED edge columns (band_operand): two exchanges on one
    #      dependency chain at each of the 67 GroupNorm + conv sites of an evaluation.  The neighbour's normalised edge column is a
    #      function of its RAW fp32 column and of the panorama's combined statistics — which this rank holds anyway — so the raw
    #      columns ride with the records and each rank normalises the two columns it received with the same kernel, the same
    #      combined records: the same bits as the neighbour computed (gloo tests: eps equal to the two-exchange form).
    fused_halo = True                 # False: rounds 3-5's two exchanges (A/B, tests)

    def stats_and_halo(self, part: torch.Tensor, col_left: torch.Tensor, col_right: torch.Tensor, F: int, nchunk: int):
        """part: this band's records [F, nchunk, 32, 3]; col_left / col_right: its RAW fp32 edge columns [F, H, C] (image columns 0
        and W - 1) -> (records of all G bands in rank order [G * F * nchunk * 96], the left neighbour's column W - 1 or None at the left
        end of the panorama, the right neighbour's column 0 or None at the right end).  ONE all_to_all_single inside the view group:
        every peer gets the records, the two neighbours one column each on top."""
        G, me = self.G, self.index
        mine = part.reshape(-1)[: F * nchunk * 96].contiguous()
        self.exchanges += 1
        if self.group is None:                       # loop-back: one band = the whole panorama, zeros beyond both ends
            return mine, None, None
        import torch.distributed as dist
        dev = mine.device
        rb = mine.view(torch.uint8)
        cl, cr = col_left.contiguous().view(-1).view(torch.uint8), col_right.contiguous().view(-1).view(torch.uint8)
        nr, nc = rb.numel(), cl.numel()
        parts, in_split, out_split = [], [0] * G, [0] * G
        for p in range(G):
            parts.append(rb)
            in_split[p] = out_split[p] = nr
            if p == me - 1:                          # my left neighbour: my column 0 is its column W
                parts.append(cl)
                in_split[p] += nc
                out_split[p] += nc
            elif p == me + 1:                        # my right neighbour: my column W - 1 is its column -1
                parts.append(cr)
                in_split[p] += nc
                out_split[p] += nc
        send = torch.cat(parts)
        self.bytes_sent += send.numel() - nr
        stage = self._host and dev.type != "cpu"
        if stage:
            send = send.cpu()
        recv = torch.empty(sum(out_split), dtype=torch.uint8, device=send.device)
        dist.all_to_all_single(recv, send, output_split_sizes=out_split, input_split_sizes=in_split, group=self.group)
        if stage:
            recv = recv.to(dev)
        recs, from_left, from_right, o = [], None, None, 0
        for p in range(G):
            recs.append(recv[o:o + nr])
            o += nr
            if p == me - 1:
                from_left = recv[o:o + nc].view(torch.float32).view(col_left.shape)      # its column W - 1
                o += nc
            elif p == me + 1:
                from_right = recv[o:o + nc].view(torch.float32).view(col_right.shape)    # its column 0
                o += nc
        return torch.cat(recs).view(torch.float32), from_left, from_right

    def neighbour_views(self, k4: torch.Tensor, v4: torch.Tensor):
        """k4 [F, H, W_l, C] keys (channels-last), v4 [F, C, H, W_l] values (channel-major) of this band -> the same with one
        view of the left neighbour in front and one of the right neighbour behind (circular), i.e. n_local + 2 views.
        (Round 3-4 form: copies the whole band.  The network uses `halo_views` since round 5.)"""
        Wv = k4.shape[2] // self.n_local
        (kl, vl), (kr, vr) = self._exchange([k4[:, :, :Wv], v4[..., :Wv]], [k4[:, :, -Wv:], v4[..., -Wv:]])
        return torch.cat([kl, k4, kr], dim=2).contiguous(), torch.cat([vl, v4, vr], dim=3).contiguous()

    def halo_views(self, rt, k4: torch.Tensor, v4: torch.Tensor, k_rows: int, k_ld: int, k_col: int):
        """Round 5: the neighbours' edge views WITHOUT touching the band.  k4 [F, H, W_l, C] (a strided view of
        the QKV GEMM's row-major output: rows of k_ld elements, keys at column k_col), v4 [F, C, H, W_l] (its channel-major V^T)
        stay where the GEMM wrote them; the left neighbour's last view and the right neighbour's first view land in view column 0
        of two buffers of the band's own geometry (PncAttnParams.k_halo / vt_halo: same leading dimensions, so the attention
        kernel's tile addresses differ by a wave-uniform offset only; the other columns are never written or read) ->
        ((k_left, k_right), (vt_left, vt_right)).  Copies 2 views per operand instead of n_local + 2."""
        F, H, Wl, C = k4.shape
        Wv = Wl // self.n_local
        (kl, vl), (kr, vr) = self._exchange([k4[:, :, :Wv], v4[..., :Wv]], [k4[:, :, -Wv:], v4[..., -Wv:]])
        kh, vh = [], []
        # the four band-geometry buffers are allocated ONCE per geometry and evaluation (~190 MB per site at level 0 of a
        # 3-view band when allocated per call); only view column 0 is ever written or read, launches on one stream are ordered
        cache = rt.__dict__.setdefault("_halo_bufs", {})
        for side, (kn, vn) in enumerate(((kl, vl), (kr, vr))):
            key = (side, k_rows, k_ld, F, C, H * Wl, k4.dtype)
            if key not in cache:
                cache[key] = (rt.empty((k_rows, k_ld), k4.dtype), rt.empty((F, C, H * Wl), v4.dtype))
            kb, vb = cache[key]
            kb.view(F, H, Wl, k_ld)[:, :, :Wv, k_col:k_col + C] = kn
            vb.view(F, C, H, Wl)[..., :Wv] = vn
            kh.append(kb.view(-1)[k_col:])
            vh.append(vb)
        return tuple(kh), tuple(vh)

    def local_segments(self, segs, halo_ids: bool = False):
        """the per-view key/value view lists of the whole panorama (e.g. INTER_SEGS) -> those of this rank's views, as
        indices into the `neighbour_views` layout (0 = left neighbour, 1 .. n_local = the band, n_local + 1 = right neighbour),
        or — `halo_ids` — as the ids of `halo_views` / PncAttnParams.k_halo: band views 0 .. n_local - 1, left -1, right n_local"""
        out = []
        base = 0 if halo_ids else 1
        for v in range(self.first, self.first + self.n_local):
            row = []
            for u in segs[v]:
                if self.first <= u < self.first + self.n_local:
                    row.append(u - self.first + base)
                elif u == (self.first - 1) % self.VIEWS:
                    row.append(base - 1)
                elif u == (self.first + self.n_local) % self.VIEWS:
                    row.append(self.n_local + base)
                else:
                    raise ValueError(f"view {v} attends view {u}, which is not a neighbour of this rank's band")
            out.append(row)
        return out

    def gather_width(self, x: torch.Tensor) -> torch.Tensor:
        """[..., W_l] bands -> [..., W] (the latent at the end of the schedule, for the first-stage decoder)"""
        if self.group is None:
            return x
        import torch.distributed as dist
        send = x.contiguous().cpu() if self._host and x.device.type != "cpu" else x.contiguous()
        parts = [torch.empty_like(send) for _ in range(self.G)]
        dist.all_gather(parts, send, group=self.group)
        return torch.cat(parts, dim=-1).to(x.device)


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
        if key is None:
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
    under the same conditions as a module's.  `site` = (owning network, fixed name) names such a matrix in a range profile.
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
