"""First-stage decoder — host-side mirror of `sgm/modules/diffusionmodules/model.py` (Decoder, ResnetBlock,
AttnBlock, Upsample, Normalize) plus the `post_quant_conv` of `sgm/models/autoencoder.py:AutoencoderKL` (SURVEY.md
§8 f2).  Same constructor keywords, module tree and state-dict names as the reference, so the `first_stage_model.*`
sub-tree of a checkpoint loads with `strict=False`; all arithmetic runs through the C-ABI kernels of the denoiser:

* resident layout = channels-last tokens `[F*H*W, C]`, fp32 stream + fp16 operands (engine.py);
* `Normalize` (GroupNorm 32, eps 1e-6) + swish (= SiLU, model.py:54-57)  -> pnc_groupnorm_stats/apply (silu flag);
* every 3x3 conv, incl. nearest-2x `Upsample` + conv (model.py:65-77)     -> pnc_gemm_f16 implicit GEMM (upsample flag);
* 1x1 `nin_shortcut`, q / k / v / proj_out                                 -> pnc_gemm_f16, residual adds in its epilogue;
* the single-head d = C attention of the mid block (model.py:374-415)     -> S = Q K^T (fp32) -> pnc_softmax_rows_f16
  -> O = P V against the channel-major V^T the v-projection writes; one frame at a time (12288^2 scores at 256x3072).
  Frames of FUSED_ATTN_MIN_TOKENS tokens or more (default: beyond the row softmax's 16384) -> pnc_attn_frame_f16, one fused
  launch over all frames on the same q / k / V^T, no N x N matrix.

The per-module `forward`s take/return NCHW tensors like the reference; `Decoder.forward` keeps everything resident.

OPERAND POLICY.  `FirstStageDecoder` / `FirstStageEncoder` take `precision=` ("fast", the default: plain fp16 operands and weights;
"precise-wide": every GEMM and attention operand an fp16 pair hi + 2^-11 lo; "precise-full": the weights split as well, for fp32
checkpoints — the reference runs its first stage in fp32).  The policy is an attribute of every module of the tree
(`set_precision`), each Runtime a module creates carries it (`rt.prec`), and the operands follow it: `rt.operand` allocates the lo
planes, `engine.gemm` hands on A_lo / out16_lo and the weights' lo twins.  Under a split policy the mid-block attention is ONE
pnc_attn_frame_split_f16 launch at every N on row-major q / k / v pairs (no V^T: the transposed store has no lo plane).
"""
from __future__ import annotations

import os
from typing import List

import torch
import torch.nn as nn

from .. import engine as E
from .. import image
from ..engine import Act, Operand, Packable, Runtime
from .util import act_from_nchw


SOFTMAX_ROWS_MAX_TOKENS = 16384      # pnc_softmax_rows_f16 keeps a row in registers: the limit of the three-launch attention
FUSED_ATTN_CHANNELS = (128, 256, 512)  # the head dims pnc_attn_frame_f16 is instantiated for


def _fused_attn_min_tokens(default: int = SOFTMAX_ROWS_MAX_TOKENS + 1) -> int:
    """PNC_VAE_FUSED_ATTN_MIN_TOKENS (read once, at import): a frame of that many tokens or more takes the fused attention
    kernel.  Unset: only the frames the three-launch path cannot serve.  0 sends every frame there (measurements, tests)."""
    raw = os.environ.get("PNC_VAE_FUSED_ATTN_MIN_TOKENS")
    if raw is None or raw.strip() == "":
        return default
    try:
        v = int(raw.strip())
    except ValueError:
        raise ValueError(f"PNC_VAE_FUSED_ATTN_MIN_TOKENS must be a non-negative integer, got {raw!r}") from None
    if v < 0:
        raise ValueError(f"PNC_VAE_FUSED_ATTN_MIN_TOKENS must be a non-negative integer, got {raw!r}")
    return v


FUSED_ATTN_MIN_TOKENS = _fused_attn_min_tokens()


def Normalize(in_channels, num_groups=32):
    """model.py:59-62"""
    return torch.nn.GroupNorm(num_groups=num_groups, num_channels=in_channels, eps=1e-6, affine=True)


FIRST_STAGE_PRECISIONS = ("fast", "precise-wide", "precise-full")


def first_stage_precision(p) -> E.Precision:
    """the operand policy of a first stage: one of FIRST_STAGE_PRECISIONS or the matching engine.Precision object"""
    try:
        q = E.precision(p)
    except (ValueError, TypeError):
        q = None
    if not any(q is E.PRECISIONS[n] or (type(q) is type(E.PRECISIONS[n]) and q == E.PRECISIONS[n]) for n in FIRST_STAGE_PRECISIONS):
        raise ValueError(f"first-stage precision {p!r}: choose one of {list(FIRST_STAGE_PRECISIONS)} (or the matching engine.Precision); "
                         "policies with e4m3 lo planes are not measured for the first stage")
    return q


def set_precision(module: nn.Module, p) -> E.Precision:
    """store the operand policy on every module below `module` (their `_run`s read it through the Runtime their entry creates)"""
    q = first_stage_precision(p)
    for m in module.modules():
        m.precision = q
    return q


def _runtime(module: nn.Module, device, F: int) -> Runtime:
    """the Runtime of one run of `module`, carrying the module's operand policy"""
    rt = Runtime(device, F, 1)
    rt.prec = getattr(module, "precision", E.FAST)
    if _split(rt):           # a backend or a width without the split attention kernel is refused before anything is launched
        for m in module.modules():
            if isinstance(m, AttnBlock):
                m.split_kernel(rt)
    return rt


def _split(rt: Runtime) -> bool:
    return E.is_wide(rt.prec)


def _tokens_of_nchw(rt: Runtime, x: torch.Tensor, cpad: int) -> Operand:
    """(F, C, H, W) floats -> the [F*H*W, cpad] token operand a first conv gathers from (operand class `stem`)"""
    F, C, H, W = x.shape
    x16 = rt.operand((F * H * W, cpad), "stem")
    rt.be.nchw_to_tokens_f16(x.detach().to(torch.float32).contiguous(), C, None, 0, F, H * W, cpad, *x16)
    return x16


def _input_operand(rt: Runtime, x16) -> Operand:
    """the token operand handed to a network's `_run` (a bare tensor is an operand without a lo plane)"""
    x16 = x16 if isinstance(x16, Operand) else Operand(x16)
    if _split(rt) and x16.lo is None:
        raise ValueError(f"the operand policy {rt.prec.name} needs the lo plane of the input tokens (an engine.Operand)")
    return x16


def _conv3x3_params(conv: nn.Conv2d, lo: bool = False):
    return E.pk_conv3x3(conv.weight, lo=lo), E.pk_f32(conv.bias)


def _conv1x1_params(conv: nn.Conv2d, lo: bool = False):
    return E.pk_linear(conv.weight, lo), E.pk_f32(conv.bias)


def _gn_params(gn: nn.GroupNorm):
    if gn.num_groups != 32:
        raise NotImplementedError("only GroupNorm(32, C) is on the path")
    return E.pk_f32(gn.weight), E.pk_f32(gn.bias)


def _conv3x3(rt: Runtime, x: Operand, F, Hin, Win, Cin, pk, key, Cout, *, upsample=False, down_br=False, res32=None) -> Act:
    """3x3 conv of the operand `x` (both planes under a split policy) with the weights pk[key] (+ their lo twin: engine.gemm)"""
    if down_br and (Hin % 2 or Win % 2):
        raise NotImplementedError("the stride-2 Downsample needs even image sizes")
    Hout, Wout = (2 * Hin, 2 * Win) if upsample else ((Hin // 2, Win // 2) if down_br else (Hin, Win))
    M = F * Hout * Wout
    o32 = rt.empty((M, Cout), torch.float32)
    E.gemm(rt, x, pk, key, M=M, N=Cout, K=9 * Cin, a_mode=E._hip.A_CONV3X3,
           conv=dict(Cin=Cin, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, stride=2 if down_br else 1,
                     upsample=int(upsample), pad_br=int(down_br)),
           res1=res32, ldr1=Cout, out32=o32, ldc32=Cout, ldc16=Cout)
    return Act(F, Hout, Wout, Cout, f32=o32)


class Upsample(nn.Module, Packable):
    """model.py:65-77: nearest x2, then conv3x3 (folded into the conv's input gather)."""

    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        if not with_conv:
            raise NotImplementedError("Upsample without conv is not on the path (resamp_with_conv=True)")
        self.conv = torch.nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=1, padding=1)
        self._init_packable()

    def _pack(self, lo: bool = False):
        return dict(c=_conv3x3_params(self.conv, lo))

    def _run(self, rt: Runtime, x: Act) -> Act:
        return _conv3x3(rt, x.need_f16(rt), x.F, x.H, x.W, x.C, self.packed(), "c", x.C, upsample=True)

    def forward(self, x):
        rt = _runtime(self, x.device, x.shape[0])
        return self._run(rt, act_from_nchw(rt, x)).to_nchw().to(x.dtype)


class Downsample(nn.Module, Packable):
    """model.py:98-113: F.pad(x, (0, 1, 0, 1)) then conv3x3 stride 2 padding 0 (zero padding bottom / right only)."""

    def __init__(self, in_channels, with_conv):
        super().__init__()
        self.with_conv = with_conv
        if not with_conv:
            raise NotImplementedError("Downsample without conv (avg_pool2d) is not on the path (resamp_with_conv=True)")
        self.conv = torch.nn.Conv2d(in_channels, in_channels, kernel_size=3, stride=2, padding=0)
        self._init_packable()

    def _pack(self, lo: bool = False):
        return dict(c=_conv3x3_params(self.conv, lo))

    def _run(self, rt: Runtime, x: Act) -> Act:
        return _conv3x3(rt, x.need_f16(rt), x.F, x.H, x.W, x.C, self.packed(), "c", x.C, down_br=True)

    def forward(self, x):
        rt = _runtime(self, x.device, x.shape[0])
        return self._run(rt, act_from_nchw(rt, x)).to_nchw().to(x.dtype)


class ResnetBlock(nn.Module, Packable):
    """model.py:139-196 with temb_channels = 0 (the autoencoder has no timestep embedding)."""

    def __init__(self, *, in_channels, out_channels=None, conv_shortcut=False, dropout=0.0, temb_channels=512):
        super().__init__()
        self.in_channels = in_channels
        out_channels = in_channels if out_channels is None else out_channels
        self.out_channels = out_channels
        self.use_conv_shortcut = conv_shortcut
        if temb_channels > 0:
            raise NotImplementedError("ResnetBlock with a timestep embedding is not on the first-stage path")
        if in_channels % 64 or out_channels % 64:
            raise NotImplementedError("GroupNorm(32) kernels need channel counts that are multiples of 64")
        self.norm1, self.conv1 = Normalize(in_channels), _conv(in_channels, out_channels)
        self.norm2, self.conv2 = Normalize(out_channels), _conv(out_channels, out_channels)
        self.dropout = torch.nn.Dropout(dropout)
        if in_channels != out_channels:                              # the checkpoint names the shortcut by its kind
            name, k = ("conv_shortcut", 3) if conv_shortcut else ("nin_shortcut", 1)
            setattr(self, name, _conv(in_channels, out_channels, k))
        self._init_packable()

    def _pack(self, lo: bool = False):
        pk = dict(n1=_gn_params(self.norm1), c1=_conv3x3_params(self.conv1, lo), n2=_gn_params(self.norm2),
                  c2=_conv3x3_params(self.conv2, lo))
        if self.in_channels != self.out_channels:
            pk["sc"] = _conv3x3_params(self.conv_shortcut, lo) if self.use_conv_shortcut else _conv1x1_params(self.nin_shortcut, lo)
        return pk

    def _run(self, rt: Runtime, x: Act) -> Act:
        pk = self.packed()
        Ci, Co = self.in_channels, self.out_channels
        h16 = E.gn_spatial(rt, x.f32, x.F, x.N, Ci, *pk["n1"], 1e-6, True, split="gn_res")
        h = _conv3x3(rt, h16, x.F, x.H, x.W, Ci, pk, "c1", Co)
        h16 = E.gn_spatial(rt, h.f32, x.F, x.N, Co, *pk["n2"], 1e-6, True, split="gn_res")
        skip = x.f32
        if Ci != Co:
            if self.use_conv_shortcut:
                skip = _conv3x3(rt, x.need_f16(rt), x.F, x.H, x.W, Ci, pk, "sc", Co).f32
            else:
                skip = rt.empty((x.M, Co), torch.float32)
                E.gemm(rt, x.need_f16(rt), pk, "sc", M=x.M, N=Co, K=Ci, lda=Ci, out32=skip, ldc32=Co)
        return _conv3x3(rt, h16, x.F, x.H, x.W, Co, pk, "c2", Co, res32=skip)      # x (or shortcut(x)) + h

    def forward(self, x, temb=None):
        assert temb is None
        rt = _runtime(self, x.device, x.shape[0])
        return self._run(rt, act_from_nchw(rt, x)).to_nchw().to(x.dtype)


class AttnBlock(nn.Module, Packable):
    """model.py:374-415 (== MemoryEfficientAttnBlock :417-477): single-head self-attention over the h*w tokens of a frame."""

    def __init__(self, in_channels):
        super().__init__()
        if in_channels % 64:
            raise NotImplementedError("AttnBlock needs a channel count that is a multiple of 64")
        self.in_channels = in_channels
        self.norm = Normalize(in_channels)
        self.q = torch.nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.k = torch.nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.v = torch.nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self.proj_out = torch.nn.Conv2d(in_channels, in_channels, kernel_size=1, stride=1, padding=0)
        self._init_packable()

    def _pack(self, lo: bool = False):
        return dict(n=_gn_params(self.norm), q=_conv1x1_params(self.q, lo), k=_conv1x1_params(self.k, lo),
                    v=_conv1x1_params(self.v, lo), o=_conv1x1_params(self.proj_out, lo))

    def split_kernel(self, rt: Runtime):
        """the backend's `attn_frame_split`, the ONLY attention of a split policy; NotImplementedError naming what is missing"""
        fn = getattr(rt.be, "attn_frame_split", None)
        if fn is None:
            raise NotImplementedError(f"AttnBlock under the operand policy {rt.prec.name}: this backend has no fused attention kernel on "
                                      "split operands (attn_frame_split)")
        if self.in_channels not in FUSED_ATTN_CHANNELS:
            raise NotImplementedError(f"AttnBlock under the operand policy {rt.prec.name}: pnc_attn_frame_split_f16 is built for "
                                      f"{FUSED_ATTN_CHANNELS} channels, not {self.in_channels} channels")
        return fn

    def _run_split(self, rt: Runtime, x: Act) -> Act:
        """q, k, v as row-major pairs -> one attn_frame_split launch over all frames, at every N -> proj_out on the split output"""
        C, N, M, F = self.in_channels, x.N, x.M, x.F
        attn = self.split_kernel(rt)
        pk = self.packed()
        h = E.gn_spatial(rt, x.f32, F, N, C, *pk["n"], 1e-6, False, split="gn_stt")
        q, k, v = (rt.operand((M, C), "qkv") for _ in range(3))
        for key, out in (("q", q), ("k", k), ("v", v)):
            E.gemm(rt, h, pk, key, out, M=M, N=C, K=C, lda=C, ldc16=C)
        o = rt.operand((M, C), "attn_o")
        attn(q.hi, q.lo, C, k.hi, k.lo, C, v.hi, v.lo, C, o.hi, o.lo, C, F=F, N=N, C=C, scale=float(C) ** -0.5)
        out = rt.empty((M, C), torch.float32)
        E.gemm(rt, o, pk, "o", M=M, N=C, K=C, lda=C, res1=x.f32, ldr1=C, out32=out, ldc32=C)
        return Act(F, x.H, x.W, C, f32=out)

    def _run(self, rt: Runtime, x: Act) -> Act:
        C, N, M, F = self.in_channels, x.N, x.M, x.F
        if N % 8:
            raise NotImplementedError(f"AttnBlock over {N} tokens per frame (supported: multiples of 8)")
        if _split(rt):
            return self._run_split(rt, x)
        # The fused kernel is an OPTIONAL capability of the backend, looked up rather than called through the handle: the emulated
        # backend of the tests has no twin of it yet and then behaves as before, refusal of long frames included.
        attn_frame = getattr(rt.be, "attn_frame", None)
        fused_ok = attn_frame is not None and C in FUSED_ATTN_CHANNELS
        if N > SOFTMAX_ROWS_MAX_TOKENS and not fused_ok:
            why = (f"the fused kernel is built for {FUSED_ATTN_CHANNELS} channels, not {C} channels" if attn_frame is not None
                   else "this backend has no fused attention kernel (attn_frame)")
            raise NotImplementedError(f"AttnBlock over {N} tokens per frame: the three-launch path serves up to "
                                      f"{SOFTMAX_ROWS_MAX_TOKENS} tokens and {why}")
        fused = fused_ok and N >= FUSED_ATTN_MIN_TOKENS
        pk = self.packed()
        h16 = E.gn_spatial(rt, x.f32, F, N, C, *pk["n"], 1e-6, False).hi
        q16, k16 = rt.empty((M, C), torch.float16), rt.empty((M, C), torch.float16)
        vt16 = rt.empty((F, C, N), torch.float16)                       # channel-major V^T per frame
        rt.be.gemm(h16, pk["q"][0], M=M, N=C, K=C, lda=C, bias=pk["q"][1], out16=q16, ldc16=C)
        rt.be.gemm(h16, pk["k"][0], M=M, N=C, K=C, lda=C, bias=pk["k"][1], out16=k16, ldc16=C)
        rt.be.gemm(h16, pk["v"][0], M=M, N=C, K=C, lda=C, bias=pk["v"][1], out16t=vt16, ldt=N, t_rows=N,
                   t_gstride=C * N, n_split=0)
        o16 = rt.empty((M, C), torch.float16)
        if fused:
            attn_frame(q16, C, k16, C, vt16, N, C * N, o16, C, F=F, N=N, C=C, scale=float(C) ** -0.5)
        else:
            s32 = rt.empty((N, N), torch.float32)                       # one frame's scores at a time (reused)
            p16 = rt.empty((N, N), torch.float16)
            for f in range(F):
                rt.be.gemm(q16[f * N:], k16[f * N:(f + 1) * N], M=N, N=N, K=C, lda=C, out32=s32, ldc32=N)
                rt.be.softmax_rows(s32, N, N, N, float(C) ** -0.5, p16, N)
                rt.be.gemm(p16, vt16[f], M=N, N=C, K=N, lda=N, out16=o16[f * N:], ldc16=C)
        out = rt.empty((M, C), torch.float32)
        rt.be.gemm(o16, pk["o"][0], M=M, N=C, K=C, lda=C, bias=pk["o"][1], res1=x.f32, ldr1=C, out32=out, ldc32=C)
        return Act(F, x.H, x.W, C, f32=out)

    def forward(self, x, **kwargs):
        rt = _runtime(self, x.device, x.shape[0])
        return self._run(rt, act_from_nchw(rt, x)).to_nchw().to(x.dtype)


def make_attn(in_channels, attn_type="vanilla", attn_kwargs=None, temporal=False):
    """model.py:551-585: "vanilla" and "vanilla-xformers" are the same single-head attention."""
    if attn_type in ("vanilla", "vanilla-xformers") and not temporal:
        assert attn_kwargs is None
        return AttnBlock(in_channels)
    if attn_type == "none":
        return nn.Identity(in_channels)
    raise NotImplementedError(f"attn_type {attn_type!r} is not on the first-stage path")


def _conv(cin: int, cout: int, k: int = 3) -> nn.Conv2d:
    return torch.nn.Conv2d(cin, cout, kernel_size=k, stride=1, padding=k // 2)


def _level_widths(ch: int, ch_mult) -> List[int]:
    return [ch * m for m in ch_mult]


def _stage(widths_in_out, n_blocks: int, with_attn: bool, attn_type: str, dropout: float, resample=None) -> nn.Module:
    """One resolution level of the first-stage networks as the reference names it (`block`, `attn`, optional `upsample` /
    `downsample`; model.py:800-820, 920-945): n_blocks ResnetBlocks from widths_in_out[0] to widths_in_out[1] channels, each
    followed by an AttnBlock where the level's resolution is listed in attn_resolutions.  The state-dict names of a checkpoint
    (`up.2.block.0.conv1.weight`, `down.1.downsample.conv.bias`, ...) are these attribute names."""
    cin, cout = widths_in_out
    level = nn.Module()
    level.block = nn.ModuleList(ResnetBlock(in_channels=cin if i == 0 else cout, out_channels=cout, temb_channels=0, dropout=dropout)
                                for i in range(n_blocks))
    level.attn = nn.ModuleList(make_attn(cout, attn_type=attn_type) for _ in range(n_blocks if with_attn else 0))
    if resample is not None:
        name, module = resample
        setattr(level, name, module)
    return level


def _mid(width: int, attn_type: str, dropout: float) -> nn.Module:
    mid = nn.Module()
    mid.block_1 = ResnetBlock(in_channels=width, out_channels=width, temb_channels=0, dropout=dropout)
    mid.attn_1 = make_attn(width, attn_type=attn_type)
    mid.block_2 = ResnetBlock(in_channels=width, out_channels=width, temb_channels=0, dropout=dropout)
    return mid


class Decoder(nn.Module, Packable):
    """model.py:882-1026.  `forward(z)`: z (F, z_channels, h, w) -> image (F, out_ch, 8h, 8w) for ch_mult of length 4."""

    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0,
                 resamp_with_conv=True, in_channels, resolution, z_channels, give_pre_end=False, tanh_out=False,
                 use_linear_attn=False, attn_type="vanilla", **ignorekwargs):
        super().__init__()
        if use_linear_attn:
            raise NotImplementedError("linear attention is not on the first-stage path")
        widths = _level_widths(ch, ch_mult)
        L = len(widths)
        self.ch, self.temb_ch, self.num_resolutions, self.num_res_blocks = ch, 0, L, num_res_blocks
        self.resolution, self.in_channels, self.z_channels, self.out_ch = resolution, in_channels, z_channels, out_ch
        self.give_pre_end, self.tanh_out = give_pre_end, tanh_out
        # coarse -> fine: the resolution of the k-th level built — the coarsest is floored ONCE and then doubled, as model.py:917-918,
        # 960 do it (curr_res = resolution // 2^(L-1); curr_res *= 2 per level): for a resolution that is no multiple of 2^(L-1) a
        # per-level floor gives another list (100: 12, 25, 50, 100 instead of 12, 24, 48, 96) and with it other AttnBlock placements
        res = [(resolution // 2 ** (L - 1)) * 2 ** k for k in range(L)]
        self.z_shape = (1, z_channels, res[0], res[0])
        self.conv_in = _conv(z_channels, widths[-1])
        self.mid = _mid(widths[-1], attn_type, dropout)
        # levels are built coarse -> fine (that is the order the widths chain in) and stored fine -> coarse like the reference's
        # `self.up.insert(0, up)`: up[i] works at resolution / 2^i and upsamples unless it is the finest
        levels, cin = [None] * L, widths[-1]
        for k, i_level in enumerate(reversed(range(L))):
            up = (("upsample", Upsample(widths[i_level], resamp_with_conv)) if i_level != 0 else None)
            levels[i_level] = _stage((cin, widths[i_level]), num_res_blocks + 1, res[k] in attn_resolutions, attn_type, dropout, up)
            cin = widths[i_level]
        self.up = nn.ModuleList(levels)
        self.norm_out = Normalize(widths[0])
        self.conv_out = _conv(widths[0], out_ch)
        self._init_packable()

    def get_last_layer(self, **kwargs):
        return self.conv_out.weight

    def _pack(self, lo: bool = False):
        zc = (self.z_channels + 7) // 8 * 8
        return dict(cin=(E.pk_conv3x3(self.conv_in.weight, zc, lo), E.pk_f32(self.conv_in.bias)), zc=zc,
                    no=_gn_params(self.norm_out), cout=_conv3x3_params(self.conv_out, lo))

    def _run(self, rt: Runtime, z16, F: int, H: int, W: int) -> Act:
        """z16: [F*H*W, zc] fp16 tokens (channels zero-padded to zc), a tensor or — with its lo plane — an Operand."""
        pk = self.packed()
        z16 = _input_operand(rt, z16)
        h = _conv3x3(rt, z16, F, H, W, pk["zc"], pk, "cin", self.conv_in.out_channels)
        h = self.mid.block_1._run(rt, h)
        if isinstance(self.mid.attn_1, AttnBlock):
            h = self.mid.attn_1._run(rt, h)
        h = self.mid.block_2._run(rt, h)
        for i_level in reversed(range(self.num_resolutions)):
            up = self.up[i_level]
            for i_block in range(self.num_res_blocks + 1):
                h = up.block[i_block]._run(rt, h)
                if len(up.attn) > 0:
                    h = up.attn[i_block]._run(rt, h)
            if i_level != 0:
                h = up.upsample._run(rt, h)
        if self.give_pre_end:
            return h
        h16 = E.gn_spatial(rt, h.f32, h.F, h.N, h.C, *pk["no"], 1e-6, True, split="gn_head")
        return _conv3x3(rt, h16, h.F, h.H, h.W, h.C, pk, "cout", self.out_ch)

    def forward(self, z, **kwargs):
        with torch.no_grad():
            F, C, H, W = z.shape
            rt = _runtime(self, z.device, F)
            z16 = _tokens_of_nchw(rt, z, self.packed()["zc"])
            out = self._run(rt, z16, F, H, W).to_nchw()
            if self.tanh_out:
                out = torch.tanh(out)
        return out.to(z.dtype)


class Encoder(nn.Module, Packable):
    """model.py:763-880.  `forward(x)`: image (F, in_channels, H, W) -> moments (F, 2*z_channels, H/8, W/8)."""

    def __init__(self, *, ch, out_ch, ch_mult=(1, 2, 4, 8), num_res_blocks, attn_resolutions, dropout=0.0,
                 resamp_with_conv=True, in_channels, resolution, z_channels, double_z=True, use_linear_attn=False,
                 attn_type="vanilla", **ignore_kwargs):
        super().__init__()
        if use_linear_attn:
            raise NotImplementedError("linear attention is not on the first-stage path")
        widths = _level_widths(ch, ch_mult)
        L = len(widths)
        self.ch, self.temb_ch, self.num_resolutions, self.num_res_blocks = ch, 0, L, num_res_blocks
        self.resolution, self.in_channels = resolution, in_channels
        self.in_ch_mult = (1,) + tuple(ch_mult)
        self.conv_in = _conv(in_channels, ch)
        chain = [ch] + widths                                        # level i: chain[i] -> chain[i + 1] channels at resolution / 2^i
        self.down = nn.ModuleList(
            _stage((chain[i], chain[i + 1]), num_res_blocks, (resolution // 2 ** i) in attn_resolutions, attn_type, dropout,
                   ("downsample", Downsample(chain[i + 1], resamp_with_conv)) if i != L - 1 else None)
            for i in range(L))
        self.mid = _mid(widths[-1], attn_type, dropout)
        self.norm_out = Normalize(widths[-1])
        self.out_channels = 2 * z_channels if double_z else z_channels
        self.conv_out = _conv(widths[-1], self.out_channels)
        self._init_packable()

    def _pack(self, lo: bool = False):
        ic = (self.in_channels + 7) // 8 * 8
        return dict(cin=(E.pk_conv3x3(self.conv_in.weight, ic, lo), E.pk_f32(self.conv_in.bias)), ic=ic,
                    no=_gn_params(self.norm_out), cout=_conv3x3_params(self.conv_out, lo))

    def _run(self, rt: Runtime, x16, F: int, H: int, W: int) -> Act:
        """x16: [F*H*W, ic] fp16 tokens (channels zero-padded to ic), a tensor or — with its lo plane — an Operand.  Returns the
        moments as an Act (fp32)."""
        pk = self.packed()
        x16 = _input_operand(rt, x16)
        h = _conv3x3(rt, x16, F, H, W, pk["ic"], pk, "cin", self.ch)
        for i_level in range(self.num_resolutions):
            down = self.down[i_level]
            for i_block in range(self.num_res_blocks):
                h = down.block[i_block]._run(rt, h)
                if len(down.attn) > 0:
                    h = down.attn[i_block]._run(rt, h)
            if i_level != self.num_resolutions - 1:
                h = down.downsample._run(rt, h)
        h = self.mid.block_1._run(rt, h)
        if isinstance(self.mid.attn_1, AttnBlock):
            h = self.mid.attn_1._run(rt, h)
        h = self.mid.block_2._run(rt, h)
        h16 = E.gn_spatial(rt, h.f32, h.F, h.N, h.C, *pk["no"], 1e-6, True, split="gn_head")
        return _conv3x3(rt, h16, h.F, h.H, h.W, h.C, pk, "cout", self.out_channels)

    def forward(self, x):
        with torch.no_grad():
            if x.dim() == 5:                                   # (b t c h w) video input (model.py:855-856)
                x = x.reshape(-1, *x.shape[2:])
            F, C, H, W = x.shape
            rt = _runtime(self, x.device, F)
            x16 = _tokens_of_nchw(rt, x, self.packed()["ic"])
            out = self._run(rt, x16, F, H, W).to_nchw()
        return out.to(x.dtype)


class FirstStageEncoder(nn.Module, Packable):
    """The encode half of `AutoencoderKL` (autoencoder.py:333-362): moments = quant_conv(encoder(x)); the posterior is
    DiagonalGaussianDistribution(moments): mean, logvar clamped to [-30, 20], sample = mean + exp(logvar / 2) * eps
    (`AutoencoderKLInferenceWrapper.encode` returns `.sample()`, autoencoder.py:371-373)."""

    def __init__(self, embed_dim: int, ddconfig: dict, *, precision="fast"):
        super().__init__()
        assert ddconfig["double_z"]
        self.encoder = Encoder(**ddconfig)
        self.quant_conv = torch.nn.Conv2d(2 * ddconfig["z_channels"], 2 * embed_dim, 1)
        self.embed_dim = embed_dim
        self._init_packable()
        set_precision(self, precision)                       # (the Encoder's signature mirrors the reference's ddconfig)

    def _pack(self, lo: bool = False):
        return dict(q=_conv1x1_params(self.quant_conv, lo))

    def moments(self, x: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            if x.dim() == 5:
                x = x.reshape(-1, *x.shape[2:])
            F, C, H, W = x.shape
            rt = _runtime(self, x.device, F)
            x16 = _tokens_of_nchw(rt, x, self.encoder.packed()["ic"])
            return self._moments_of_tokens(rt, x16, F, H, W).to(x.dtype)

    def _moments_of_tokens(self, rt: Runtime, x16: Operand, F: int, H: int, W: int) -> torch.Tensor:
        """encoder + quant_conv on the image tokens x16 [F*H*W, ic] -> the moments, NCHW fp32"""
        h = self.encoder._run(rt, x16, F, H, W)
        n = self.quant_conv.out_channels
        m32 = rt.empty((h.M, n), torch.float32)
        E.gemm(rt, h.need_f16(rt), self.packed(), "q", M=h.M, N=n, K=h.C, lda=h.C, out32=m32, ldc32=n)
        return Act(h.F, h.H, h.W, n, f32=m32).to_nchw()

    def moments_u8(self, x_u8: torch.Tensor, table: str = "image") -> torch.Tensor:
        """`moments` of (F, H, W, 3) uint8 channels-last frames, scaled on their way into the token matrix by `table` ("image":
        byte / 127.5 - 1, the dataset's scaling of frames; "layout": byte / 255): the bits of
        `moments(table[x_u8].permute(0, 3, 1, 2))` without a float image anywhere.  Returns fp32."""
        with torch.no_grad():
            x_u8 = image.frames_u8(x_u8, "moments_u8")
            F, H, W, C = x_u8.shape
            if C != self.encoder.in_channels:
                raise ValueError(f"moments_u8: frames of {C} channels for an encoder of {self.encoder.in_channels}")
            image.table(table)                                     # (an unknown kind is refused here)
            rt = _runtime(self, x_u8.device, F)
            image.capability(rt.be, "u8_to_tokens_f16")
            ic = self.encoder.packed()["ic"]
            x16 = rt.operand((F * H * W, ic), "stem")
            image.u8_to_tokens(rt, x_u8, table, ic, x16)
            return self._moments_of_tokens(rt, x16, F, H, W)

    def moments_sparse_u8(self, clip: "image.SparseClip", table: str = "image") -> torch.Tensor:
        """`moments` of the clip `clip` stands for — its K uint8 frames at their slots, float 0.0 frames everywhere else — from ONE
        encoder run over K + 1 frames instead of `num_frames`: the K given frames enter like `moments_u8`'s, the blank frame is an
        all-zero token plane (the bits nchw_to_tokens_f16 writes for a float-zero frame), and since every layer of the encoder acts on
        each frame by itself, the blank frame's moments are those of every blank slot.  K = 0 gives an all-blank clip, K = num_frames
        runs no blank frame.  Returns (num_frames, 2C, h, w) fp32."""
        if not isinstance(clip, image.SparseClip):
            raise TypeError(f"moments_sparse_u8: an image.SparseClip expected, got {type(clip).__name__}")
        with torch.no_grad():
            x_u8 = clip.frames_u8
            K, H, W, C = x_u8.shape
            if C != self.encoder.in_channels:
                raise ValueError(f"moments_sparse_u8: frames of {C} channels for an encoder of {self.encoder.in_channels}")
            image.table(table)                                     # (an unknown kind is refused here)
            F = K + (1 if K < clip.num_frames else 0)
            rt = _runtime(self, x_u8.device, F)
            image.capability(rt.be, "u8_to_tokens_f16")
            ic = self.encoder.packed()["ic"]
            alloc = rt.zeros if F > K else rt.empty              # the blank frame is zero in both planes
            x16 = Operand(alloc((F * H * W, ic), torch.float16), alloc((F * H * W, ic), torch.float16) if _split(rt) else None)
            if K:
                image.u8_to_tokens(rt, x_u8, table, ic, x16.map(lambda t: t[: K * H * W]))
            return self._moments_of_tokens(rt, x16, F, H, W).index_select(0, clip.gather_index())

    def encode(self, x: torch.Tensor, generator=None, sample: bool = True) -> torch.Tensor:
        return self._posterior(self.moments(x), generator, sample)

    def encode_sparse_u8(self, clip: "image.SparseClip", generator=None, sample: bool = True, table: str = "image") -> torch.Tensor:
        """`encode` of a sparse clip (see moments_sparse_u8): the posterior of the full (num_frames, 2C, h, w) moments, so a generator
        state gives the draw that encoding the dense clip gives — one randn of (num_frames, C, h, w)"""
        return self._posterior(self.moments_sparse_u8(clip, table), generator, sample)

    def encode_u8(self, x_u8: torch.Tensor, generator=None, sample: bool = True, table: str = "image") -> torch.Tensor:
        """`encode` of uint8 channels-last frames (see moments_u8): the same posterior, the same draw for the same generator state"""
        return self._posterior(self.moments_u8(x_u8, table), generator, sample)

    @staticmethod
    def _posterior(mom: torch.Tensor, generator, sample: bool) -> torch.Tensor:
        mean, logvar = torch.chunk(mom, 2, dim=1)
        if not sample:
            return mean
        std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
        eps = torch.randn(mean.shape, generator=generator, device=mean.device, dtype=mean.dtype)
        return mean + std * eps

    forward = encode


class FirstStageDecoder(nn.Module, Packable):
    """The decode half of `AutoencoderKL` (autoencoder.py:333-368): `decoder(post_quant_conv(z))`.  Attribute names
    match the reference's, so `load_state_dict(first_stage_sd, strict=False)` fills it (encoder / quant_conv /
    loss keys are reported as unexpected, like any partial load)."""

    def __init__(self, embed_dim: int, ddconfig: dict, *, precision="fast"):
        super().__init__()
        self.decoder = Decoder(**ddconfig)
        self.post_quant_conv = torch.nn.Conv2d(embed_dim, ddconfig["z_channels"], 1)
        self.embed_dim = embed_dim
        self._init_packable()
        set_precision(self, precision)                       # (the Decoder's signature mirrors the reference's ddconfig)

    def _pack(self, lo: bool = False):
        # 1x1 conv embed_dim -> z_channels, both zero-padded to multiples of 8 so that its fp16 output is directly the
        # padded token matrix conv_in gathers from
        ec, zc = (self.embed_dim + 7) // 8 * 8, (self.decoder.z_channels + 7) // 8 * 8
        w = torch.zeros((zc, ec), dtype=torch.float16, device=self.post_quant_conv.weight.device)
        w[: self.decoder.z_channels, : self.embed_dim] = E._cast16(self.post_quant_conv.weight.reshape(
            self.decoder.z_channels, self.embed_dim), lo)
        b = torch.zeros(zc, dtype=torch.float32, device=w.device)
        b[: self.decoder.z_channels] = self.post_quant_conv.bias.detach().float()
        return dict(w=w.contiguous(), b=b, ec=ec, zc=zc)

    def _decode_tokens(self, rt: Runtime, z: torch.Tensor) -> Act:
        """post_quant_conv + decoder on the latent z (F, C, H, W) -> the decoder's output in the resident layout"""
        pk = self.packed()
        F, C, H, W = z.shape
        M = F * H * W
        e16 = _tokens_of_nchw(rt, z, pk["ec"])
        z16 = rt.operand((M, pk["zc"]), "stem")
        E.gemm(rt, e16, pk, "w", z16, M=M, N=pk["zc"], K=pk["ec"], lda=pk["ec"], bias=pk["b"], ldc16=pk["zc"])
        return self.decoder._run(rt, z16, F, H, W)

    def decode(self, z: torch.Tensor) -> torch.Tensor:
        with torch.no_grad():
            out = self._decode_tokens(_runtime(self, z.device, z.shape[0]), z).to_nchw()
        return out.to(z.dtype)

    def decode_u8(self, z: torch.Tensor) -> torch.Tensor:
        """z (F, C, h, w) -> (F, 8h, 8w, 3) uint8 frames on z's device: the decoder's last conv writes an [F*H*W, 3] token matrix,
        which already is H x W x 3, and pnc_tokens_to_u8 quantises it in place of `to_nchw()` + the host's clamp, (x + 1) / 2,
        * 255, truncate (inference.py:189-193).  The bytes of `checkpoint._to_uint8(decode(z)[f])`, frame by frame."""
        if self.decoder.tanh_out or self.decoder.give_pre_end:
            raise NotImplementedError("decode_u8 quantises the output conv's tokens: tanh_out / give_pre_end decoders go through decode()")
        with torch.no_grad():
            rt = _runtime(self, z.device, z.shape[0])
            image.capability(rt.be, "tokens_to_u8")
            return image.tokens_to_u8(rt, self._decode_tokens(rt, z))

    forward = decode
