"""UNetModel3D and its blocks on MI355X — host-side mirror of
`sgm/modules/diffusionmodules/openaimodel.py` (hot part: :79-201 blocks, :356-542 ResBlock3D,
:774-1319 UNetModel3D).

The module tree (and therefore every state-dict key and shape) is the reference's; the forwards run
the gfx950 kernels on channels-last tokens:

  ResBlock3D._forward :499-542   GN+SiLU kernel -> implicit-GEMM conv3x3 -> per-pixel temporal GN+SiLU
                                 -> temporal conv1d GEMM whose epilogue adds the identity, the timestep
                                 embedding row and (second half) the skip path; 4 layout copies of the
                                 reference ("(b t) c h w" <-> "(b h w) c t") do not exist here.
  Downsample :161-201            conv3x3 stride 2 (implicit GEMM, gather does the striding)
  Upsample :106-142              nearest x2 folded into the conv gather (no upsampled tensor is written)
"""
from __future__ import annotations

import contextlib
from typing import Optional

import torch
import torch.nn as nn

from .. import engine as E
from ..engine import Act, Packable, Runtime
from .attention import SpatialTemporalTransformer
from .util import check_num_frames, conv_nd, linear, normalization, timestep_embedding, zero_module


def _as_list(v):
    if isinstance(v, (int, float)) or v is None:
        return v
    return list(v)


class TimestepBlock(nn.Module):
    """openaimodel.py:66-76 — marker for children that take the timestep embedding."""


def conv_params(conv: nn.Conv2d, lo=False):
    """(packed weight, fp32 bias) of a 3x3 or 1x1 conv; `lo`: the weight's lo plane (engine.pk_f16)"""
    k = conv.kernel_size[0]
    if k == 3:
        return E.pk_conv3x3(conv.weight, lo=lo), E.pk_f32(conv.bias)
    if k == 1:
        return E.pk_linear(conv.weight, lo), E.pk_f32(conv.bias)
    raise NotImplementedError(f"conv kernel size {k}")


def run_conv3x3(rt: Runtime, x: E.Operand, F: int, Hin: int, Win: int, Cin_pad: int, pk, key, Cout: int, bias=None,
                stride: int = 1, upsample: bool = False, act_silu: bool = False, out32: bool = True,
                out16: bool = False, split_out: Optional[str] = None) -> Act:
    """3x3 conv (pad 1) as implicit GEMM over the channels-last fp16 image x [F*Hin*Win, Cin_pad] with the weights pk[key]
    (engine.gemm); `split_out`: operand class of the fp16 output.
    On a rank's band of views (engine.ViewShard) the band's columns -1 and Win — the neighbour ranks' edge columns — sit in a tail
    of the operand's own allocation (ViewShard.band_operand) and the gather reads them where the unsharded conv reads the
    neighbouring views (PncGemmParams.x_halo_off): the conv runs over the band as it lies and writes the band's outputs, no widened
    copy of the operand and no window copy of the result."""
    Hout = 2 * Hin if upsample else (Hin - 1) // stride + 1
    Wout = 2 * Win if upsample else (Win - 1) // stride + 1
    conv = dict(Cin=Cin_pad, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, stride=stride, upsample=int(upsample))
    if rt.vshard is not None:
        if stride == 2 and Win % 2:
            raise ValueError(f"a stride-2 conv over a view band needs an even band width, got {Win}")
        planes, conv["x_halo_off"] = rt.vshard.band_operand(rt, x.planes(), F, Hin, Win, Cin_pad)
        x = E.Operand(*planes)
    M = F * Hout * Wout
    o32 = rt.empty((M, Cout), torch.float32) if out32 else None
    o16 = rt.operand((M, Cout), split_out) if out16 else None
    E.gemm(rt, x, pk, key, o16, M=M, N=Cout, K=9 * Cin_pad, a_mode=E._hip.A_CONV3X3, conv=conv, bias=bias,
           act=E._hip.ACT_SILU if act_silu else E._hip.ACT_NONE, out32=o32, ldc32=Cout, ldc16=Cout)
    return Act(F, Hout, Wout, Cout, f32=o32, f16=o16)


class TimestepEmbedSequential(nn.Sequential, TimestepBlock, Packable):
    """openaimodel.py:79-103 — children get (x, emb), (x, context) or (x) according to their type."""

    def __init__(self, *args):
        super().__init__(*args)
        self._init_packable()

    def _pack(self, lo=False):
        return {i: conv_params(m, lo) for i, m in enumerate(self) if isinstance(m, nn.Conv2d)}

    def _run(self, rt: Runtime, x: Act, emb32, want_f16: bool = False) -> Act:
        layers = list(self)
        for i, layer in enumerate(layers):
            nxt = layers[i + 1] if i + 1 < len(layers) else None
            wf = want_f16 if nxt is None else isinstance(nxt, (Upsample, Downsample, nn.Conv2d))
            if isinstance(layer, ResBlock3D):
                # (want_stats: the next layer starts with a spatial GroupNorm of this block's output)
                x = layer._run(rt, x, emb32, want_f16=wf, want_stats=isinstance(nxt, (ResBlock3D, SpatialTemporalTransformer)))
            elif isinstance(layer, SpatialTemporalTransformer):
                x = layer._run(rt, x, want_f16=wf)
            elif isinstance(layer, (Upsample, Downsample)):
                x = layer._run(rt, x, want_f16=wf)
            elif isinstance(layer, nn.Conv2d):
                pk, Co = self.packed(), layer.out_channels           # pk[i] = (weight, bias)
                if layer.kernel_size[0] == 3:
                    x = run_conv3x3(rt, x.need_f16(rt), x.F, x.H, x.W, x.C, pk, i, Co, stride=layer.stride[0], out16=wf,
                                    split_out="stream")
                else:
                    o32 = rt.empty((x.M, Co), torch.float32)
                    o16 = rt.operand((x.M, Co), "stream") if wf else None
                    E.gemm(rt, x.need_f16(rt), pk, i, o16, M=x.M, N=Co, K=x.C, lda=x.C, out32=o32, ldc32=Co, ldc16=Co)
                    x = Act(x.F, x.H, x.W, Co, f32=o32, f16=o16)
            else:
                raise NotImplementedError(f"{type(layer).__name__} inside TimestepEmbedSequential")
        return x


class Upsample(nn.Module, Packable):
    """openaimodel.py:106-142"""

    def __init__(self, channels, use_conv, dims=2, out_channels=None, padding=1, third_up=False):
        super().__init__()
        if dims != 2 or not use_conv or padding != 1:
            raise NotImplementedError("Upsample: only dims=2 with a 3x3 conv is on the Panacea path")
        self.channels, self.out_channels, self.use_conv, self.dims = channels, out_channels or channels, use_conv, dims
        self.conv = conv_nd(dims, self.channels, self.out_channels, 3, padding=padding)
        self._init_packable()

    def _pack(self, lo=False):
        w, b = conv_params(self.conv, lo)
        return dict(w=w, b=b, w9=E.pk_conv3x3_taps(self.conv.weight, lo))      # w: the output-resolution conv (fallback, A/B partner)

    # the conv's operand as a precise pair (class `stream`).  False (bench.py --upsample-plain-operand, an A/B of the error budget):
    # the three Upsample convs of the UNet decoder read the fp16 plane only — their e4m3 lo pass is 1.6 ms of the step
    precise_operand = True

    def _run(self, rt: Runtime, x: Act, want_f16=False) -> Act:
        pk = self.packed()
        x16 = x.need_f16(rt)
        if not self.precise_operand:
            x16 = E.Operand(x16.hi)
        Co = self.out_channels
        # (an OPTIONAL entry of the backend: the torch emulation of the C-ABI the CPU tests run on has none and keeps the conv below)
        combine = getattr(rt.be, "upsample_combine", None)
        if not (E.UPSAMPLE_SOURCE_RES and combine is not None and rt.vshard is None and x.C % 64 == 0 and Co % 4 == 0):
            return run_conv3x3(rt, x16, x.F, x.H, x.W, x.C, pk, "w", Co, pk["b"], upsample=True, out16=want_f16, split_out="stream")
        # Multiply at SOURCE resolution: neighbouring output pixels read the same source pixel through the same tap, so only 9 of the
        # 36 products per source pixel of the output-resolution conv are distinct.  P = x @ w9^T holds them (the hi and lo passes of any
        # `stream` operand, as engine.gemm runs them); pnc_upsample_combine adds each output pixel's nine, in tap order, to the bias.
        # Frames go in chunks (engine.upsample_chunk_frames) over ONE P buffer: the launches of a stream run in order.
        N, Mo = x.N, 4 * x.M
        o32 = rt.empty((Mo, Co), torch.float32)
        o16 = rt.operand((Mo, Co), "stream") if want_f16 else None
        fc = E.upsample_chunk_frames(x.F, x.H, x.W, Co)
        P = rt.empty((fc * N, 9 * Co), torch.float32)
        for f0 in range(0, x.F, fc):
            nf = min(fc, x.F - f0)
            E.gemm(rt, x16.map(lambda t: t[f0 * N:(f0 + nf) * N]), pk, "w9", site=(self, "w"), M=nf * N, N=9 * Co, K=x.C, lda=x.C,
                   out32=P, ldc32=9 * Co)
            outs = [None if t is None else t[4 * f0 * N:] for t in (o32, *(o16 or (None, None)))]
            combine(P, 9 * Co, pk["b"], nf, x.H, x.W, Co, *outs)
        return Act(x.F, 2 * x.H, 2 * x.W, Co, f32=o32, f16=o16)


class Downsample(nn.Module, Packable):
    """openaimodel.py:161-201"""

    def __init__(self, channels, use_conv, dims=2, out_channels=None, padding=1, third_down=False):
        super().__init__()
        if dims != 2 or not use_conv or padding != 1:
            raise NotImplementedError("Downsample: only dims=2 with a strided 3x3 conv is on the Panacea path")
        self.channels, self.out_channels, self.use_conv, self.dims = channels, out_channels or channels, use_conv, dims
        self.op = conv_nd(dims, self.channels, self.out_channels, 3, stride=2, padding=padding)
        self._init_packable()

    def _pack(self, lo=False):
        w, b = conv_params(self.op, lo)
        return dict(w=w, b=b)

    def _run(self, rt: Runtime, x: Act, want_f16=False) -> Act:
        pk = self.packed()
        return run_conv3x3(rt, x.need_f16(rt), x.F, x.H, x.W, x.C, pk, "w", self.out_channels, pk["b"], stride=2, out16=want_f16,
                           split_out="stream")


class ResBlock3D(TimestepBlock, Packable):
    """openaimodel.py:356-542"""

    def __init__(self, channels, emb_channels, dropout, out_channels=None, use_conv=False,
                 use_scale_shift_norm=False, dims=2, use_checkpoint=False, up=False, down=False, kernel_size=3,
                 exchange_temb_dims=False, skip_t_emb=False, temporal_kernel_size=3, alpha=1, num_frames=4):
        super().__init__()
        if up or down or use_scale_shift_norm or exchange_temb_dims or skip_t_emb or use_conv:
            raise NotImplementedError("ResBlock3D: up/down/scale-shift/exchange_temb/skip_t_emb/use_conv are dead "
                                      "paths of the Panacea configuration and are not built")
        if dims != 2 or kernel_size != 3 or temporal_kernel_size != 3:
            raise NotImplementedError("ResBlock3D: dims=2, 3x3 spatial and k=3 temporal kernels only")
        self.num_frames = check_num_frames(num_frames, "ResBlock3D")
        self.channels, self.emb_channels, self.dropout = channels, emb_channels, dropout
        self.out_channels = out_channels or channels
        self.use_conv, self.use_checkpoint, self.use_scale_shift_norm = use_conv, use_checkpoint, use_scale_shift_norm
        self.exchange_temb_dims = exchange_temb_dims
        self.alpha = 1 if alpha == 1 else nn.Parameter(torch.rand(1, requires_grad=True))
        self.temporal_kernel_size = temporal_kernel_size
        self.identity_layer = nn.Identity()
        oc = self.out_channels
        self.in_layers = nn.Sequential(normalization(channels), nn.SiLU(), conv_nd(dims, channels, oc, 3, padding=1))
        self.in_layers_temporal = nn.Sequential(normalization(oc), nn.SiLU(),
                                                zero_module(conv_nd(1, oc, oc, 3, padding=1)))
        self.updown = False
        self.h_upd = self.x_upd = nn.Identity()
        self.skip_t_emb = skip_t_emb
        self.emb_out_channels = oc
        self.emb_layers = nn.Sequential(nn.SiLU(), linear(emb_channels, oc))
        self.out_layers = nn.Sequential(normalization(oc), nn.SiLU(), nn.Dropout(p=dropout),
                                        zero_module(conv_nd(dims, oc, oc, 3, padding=1)))
        self.out_layers_temporal = nn.Sequential(normalization(oc), nn.SiLU(), nn.Dropout(p=dropout),
                                                 zero_module(conv_nd(1, oc, oc, 3, padding=1)))
        self.skip_connection = nn.Identity() if oc == channels else conv_nd(dims, channels, oc, 1)
        self._init_packable()

    def _pack(self, lo=False):
        f32, il, it, ol, ot = E.pk_f32, self.in_layers, self.in_layers_temporal, self.out_layers, self.out_layers_temporal
        pk = dict(
            g1=f32(il[0].weight), b1=f32(il[0].bias), w1=E.pk_conv3x3(il[2].weight, lo=lo), c1=f32(il[2].bias),
            gt1=f32(it[0].weight), bt1=f32(it[0].bias), wt1=E.pk_conv1d(it[2].weight, lo), ct1=f32(it[2].bias),
            we=E.pk_linear(self.emb_layers[1].weight, lo), be=f32(self.emb_layers[1].bias),
            g2=f32(ol[0].weight), b2=f32(ol[0].bias), w2=E.pk_conv3x3(ol[3].weight, lo=lo), c2=f32(ol[3].bias),
            gt2=f32(ot[0].weight), bt2=f32(ot[0].bias), wt2=E.pk_conv1d(ot[3].weight, lo), ct2=f32(ot[3].bias))
        if isinstance(self.skip_connection, nn.Conv2d):
            pk["ws"], pk["bs"] = E.pk_linear(self.skip_connection.weight, lo), f32(self.skip_connection.bias)
        return pk

    def _emb_out(self, rt: Runtime, lay: E.TemporalLayout, emb32: torch.Tensor, pk, Co: int) -> torch.Tensor:
        """emb_layers(emb) of this block, fp32, one row per frame that the layout's conv sees: the network's EmbProjector computed
        it for every block in one launch (same values), or — a block run on its own, or on the rows of all frames — its own launch"""
        emb = rt.emb_all if lay.emb_all else emb32
        out = rt.emb_proj.get(id(self))
        if out is not None and out.shape == (emb.shape[0], Co):
            return out
        return E.small_linear(rt, emb, pk, "we", "be", emb.shape[0], Co, self.emb_channels)

    def _temporal_site(self, rt: Runtime, lay: E.TemporalLayout, sent, F: int, N: int, gamma, beta, w, bias, rows=None, res2=None,
                       o16=None, want_stats: bool = False):
        """One temporal site: h + conv1d_t(SiLU(GN_t(h))) + what the epilogue adds, written over the fp32 stream h [F*N, Co] of the
        frame layout.  `sent` = lay.start(rt, h, N), h on its way to the conv's layout: what the caller enqueued since then runs under
        that transfer.  gamma .. bias: the site's keys in the packed parameters.  Site 1 adds the per-frame `rows` (rowbias); site 2
        adds the skip path `res2` and writes the fp16 operand `o16` of the sum.  -> (h, its GroupNorm records (E.gn_records) or None)"""
        pk, Co = self.packed(), self.out_channels
        tconv = lay.tconv(rt, Co, N)
        at_home = lay.home is None      # the conv's rows are the frame layout's: its epilogue takes the skip path, o16 and the records
        epi = dict(res2=res2, ldr2=Co, ldc16=Co) if at_home else {}      # (away from home the skip path is added after the way back)
        if rows is not None:
            epi = dict(rowbias=rows, rb_rows=tconv["Npix"], rb_mod=rows.shape[0])
        # the normalised operand; the conv GEMM, which adds into the stream in place (res1 = out32 = h); back to the frame layout
        h, t = lay.operand(rt, sent, N, Co, pk[gamma], pk[beta], 1e-5)
        part = E.gn_records(rt, F, N) if want_stats and at_home else None
        E.gemm(rt, t, pk, w, o16 if at_home else None, M=rt.B * tconv["T"] * tconv["Npix"], N=Co, K=3 * Co, a_mode=E._hip.A_CONV1D_T,
               tconv=tconv, bias=pk[bias], res1=h, ldr1=Co, out32=h, ldc32=Co, gn_part=part, **epi)
        if not at_home:
            h = lay.home(rt, h, N)
            if res2 is not None:        # the skip path stayed in the frame layout
                rt.be.add_f32(h, res2, F * N * Co, h, *(o16 or (None, None)))
        return h, part

    def _run(self, rt: Runtime, x: Act, emb32: torch.Tensor, want_f16: bool = False, want_stats: bool = False) -> Act:
        if rt.T != self.num_frames:
            raise ValueError(f"runtime has {rt.T} frames per sample, block was built for {self.num_frames}")
        F, H, W, N, M = x.F, x.H, x.W, x.N, x.M
        pk, Cin, Co = self.packed(), self.channels, self.out_channels
        lay = E.temporal_layout(rt)     # where the T frames of a pixel are: the two temporal sites see all of them
        tail = rt.band_tail_rows(F, H)
        # in_layers: GN + SiLU + conv3x3
        a = E.gn_spatial(rt, x.f32, F, N, Cin, pk["g1"], pk["b1"], 1e-5, True, split="gn_res", tail_rows=tail, part=x.gn_part)
        h = run_conv3x3(rt, a, F, H, W, Cin, pk, "w1", Co, pk["c1"]).f32
        # h = h + conv1d_t(SiLU(GN_t(h))) + emb_layers(emb)[frame]      (:505-531).  h is sent off first: what does not depend on it —
        # emb_layers' rows (emb32 arrives as SiLU(emb), applied ONCE per network evaluation by _time_embedding) and, where h travels
        # (on the communicator's stream), the skip path — is enqueued under the transfer.  want_stats: out_layers' GroupNorm reads the result
        sent = lay.start(rt, h, N)
        rows = self._emb_out(rt, lay, emb32, pk, Co)
        s = self._skip(rt, x, pk) if lay.home is not None else None
        h, part1 = self._temporal_site(rt, lay, sent, F, N, "gt1", "bt1", "wt1", "ct1", rows=rows, want_stats=True)
        # out_layers: GN + SiLU + conv3x3
        a = E.gn_spatial(rt, h, F, N, Co, pk["g2"], pk["b2"], 1e-5, True, split="gn_res", tail_rows=tail, part=part1)
        g = run_conv3x3(rt, a, F, H, W, Co, pk, "w2", Co, pk["c2"]).f32
        s = self._skip(rt, x, pk) if s is None else s
        # return skip(x) + (g + conv1d_t(SiLU(GN_t(g))))                 (:533-542); `want_stats`: for the GroupNorm the next layer starts with
        o16 = rt.operand((M, Co), "stream") if want_f16 else None
        g, part2 = self._temporal_site(rt, lay, lay.start(rt, g, N), F, N, "gt2", "bt2", "wt2", "ct2", res2=s, o16=o16, want_stats=want_stats)
        return Act(F, H, W, Co, f32=g, f16=o16, gn_part=part2)

    def _skip(self, rt: Runtime, x: Act, pk: dict) -> torch.Tensor:
        """skip_connection(x): the 1x1 conv where the channel count changes (openaimodel.py:486), else x itself"""
        if "ws" not in pk:
            return x.f32
        s = rt.empty((x.M, self.out_channels), torch.float32)
        E.gemm(rt, x.need_f16(rt), pk, "ws", M=x.M, N=self.out_channels, K=self.channels, lda=self.channels, bias=pk["bs"], out32=s,
               ldc32=self.out_channels)
        return s

    precision = "precise"      # operand policy of the reference-compatible entry below (the network sets rt.prec itself)

    def forward(self, x, emb):
        from .util import act_from_nchw, runtime_for
        rt = runtime_for(x, self.num_frames)
        rt.prec = E.precision(self.precision)
        semb = torch.nn.functional.silu(emb.to(torch.float32)).contiguous()      # _run takes SiLU(emb)
        return self._run(rt, act_from_nchw(rt, x), semb).to_nchw().to(x.dtype)


class EmbProjector:
    """Batches the `emb_layers` Linear of every ResBlock3D of a network (openaimodel.py:440-447: SiLU -> Linear(time_embed_dim, C),
    added to h per frame at :519-531).  Its input is the network's one SiLU(time embedding): the 22 (UNet) + 11 (ControlNet)
    launches of F <= 16 rows per evaluation — ≈ 27 us each at a few percent of the chip, serialised on their stream — become one
    launch per network (`pnc_linear_smallm_segments`: the blocks' weight rows back to back, one contiguous [F, C] output per
    block; per column the arithmetic of the single launch, bit-identical)."""

    def __init__(self, root):
        self.blocks = [m for m in root.modules() if isinstance(m, ResBlock3D)]
        self._pk = self._sig = self._pk_lo = self._sig_lo = None

    def pack(self, lo=False):
        w = torch.cat([b.emb_layers[1].weight for b in self.blocks], dim=0)
        bias = torch.cat([b.emb_layers[1].bias for b in self.blocks], dim=0)
        seg = [0]
        for b in self.blocks:
            seg.append(seg[-1] + b.out_channels)
        return E.pk_linear(w, lo), E.pk_f32(bias), seg

    def run(self, rt: Runtime, emb32: torch.Tensor):
        if not self.blocks or len(self.blocks) > 64 or any(b.out_channels % 4 for b in self.blocks):
            return
        # the packed copy follows its SOURCE parameters (identity, device and in-place version): loading / moving / editing one
        # ResBlock3D alone drops that block's own packed weights but not this network-level cache
        sig = tuple((id(p), p._version, p.device) for b in self.blocks for p in (b.emb_layers[1].weight, b.emb_layers[1].bias))
        if self._pk is None or self._sig != sig:
            with torch.no_grad():
                self._pk, self._sig = self.pack(), sig
        w, bias, seg = self._pk
        F, K = emb32.shape[0], self.blocks[0].emb_channels
        out = rt.empty((seg[-1] * F,), torch.float32)
        kw = {}
        if rt.prec.weights:                           # the lo twin of the stacked weights follows the same sources
            if self._pk_lo is None or self._sig_lo != sig:
                with torch.no_grad():
                    self._pk_lo, self._sig_lo = self.pack(lo=True)[0], sig
            kw = dict(w_lo=self._pk_lo)
        for m0 in range(0, F, 16):
            rt.be.linear_smallm_segments(emb32[m0:], K, w, bias, out, min(16, F - m0), m0, F, seg[-1], K, seg, **kw)
        for b, s0, s1 in zip(self.blocks, seg[:-1], seg[1:]):
            rt.emb_proj[id(b)] = out[s0 * F:s1 * F].view(F, s1 - s0)


def _capturing(device) -> bool:
    """the current stream of `device` is being captured into a graph"""
    return device.type == "cuda" and torch.cuda.is_current_stream_capturing()


class _OwnBlocks:
    """The blocks a network runs itself (a ControlledUNetModel3D must not walk into its `.controlnet` child)."""

    def __init__(self, net):
        self.net = net

    def modules(self):
        for blk in self.net._own_blocks():
            yield from blk.modules()


class UNetModel3D(nn.Module, Packable):
    """openaimodel.py:774-1319 — same constructor, same module tree, same state dict."""

    def __init__(self, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None, use_checkpoint=False,
                 use_fp16=False, num_heads=-1, num_head_channels=-1, num_heads_upsample=-1,
                 use_scale_shift_norm=False, resblock_updown=False, use_new_attention_order=False,
                 use_spatial_transformer=False, transformer_depth=1, context_dim=None, n_embed=None, legacy=True,
                 disable_self_attentions=None, num_attention_blocks=None, disable_middle_self_attn=False,
                 use_linear_in_transformer=False, spatial_transformer_attn_type="softmax", adm_in_channels=None,
                 use_fairscale_checkpoint=False, offload_to_cpu=False, transformer_depth_middle=None, num_frames=4,
                 alpha=1, temporal_transformer_attn_type=None, spatial_only_attn_type=None, insert_crossview=False):
        super().__init__()
        unsupported = dict(num_classes=num_classes, n_embed=n_embed, resblock_updown=resblock_updown,
                           use_scale_shift_norm=use_scale_shift_norm, disable_self_attentions=disable_self_attentions,
                           num_attention_blocks=num_attention_blocks, disable_middle_self_attn=disable_middle_self_attn,
                           use_fairscale_checkpoint=use_fairscale_checkpoint)
        bad = {k: v for k, v in unsupported.items() if v}
        if bad or dims != 2 or not conv_resample or not use_spatial_transformer or context_dim is None:
            raise NotImplementedError(f"UNetModel3D options outside the Panacea inference configuration: {bad or 'dims/conv_resample/use_spatial_transformer/context_dim'}")
        if num_head_channels == -1:
            raise NotImplementedError("num_head_channels must be set (the attention kernels use head dim 64)")
        self.num_frames = num_frames = check_num_frames(num_frames, type(self).__name__)
        context_dim = _as_list(context_dim)
        attention_resolutions = _as_list(attention_resolutions)
        channel_mult = _as_list(channel_mult)
        self.in_channels, self.model_channels, self.out_channels = in_channels, model_channels, out_channels
        if isinstance(transformer_depth, int):
            transformer_depth = len(channel_mult) * [transformer_depth]
        else:
            transformer_depth = list(transformer_depth)
        transformer_depth_middle = transformer_depth[-1] if transformer_depth_middle is None else transformer_depth_middle
        if isinstance(num_res_blocks, int):
            self.num_res_blocks = len(channel_mult) * [num_res_blocks]
        else:
            if len(num_res_blocks) != len(channel_mult):
                raise ValueError("provide num_res_blocks either as an int or as a per-level list")
            self.num_res_blocks = list(num_res_blocks)
        self.attention_resolutions, self.dropout, self.channel_mult = attention_resolutions, dropout, channel_mult
        self.conv_resample, self.num_classes, self.use_checkpoint = conv_resample, num_classes, use_checkpoint
        self.num_heads, self.num_head_channels, self.num_heads_upsample = num_heads, num_head_channels, num_heads_upsample
        self.predict_codebook_ids = False
        self.alpha = alpha

        time_embed_dim = model_channels * 4
        self.time_embed_dim = time_embed_dim
        self.time_embed = nn.Sequential(linear(model_channels, time_embed_dim), nn.SiLU(),
                                        linear(time_embed_dim, time_embed_dim))

        def res(cin, cout):
            return ResBlock3D(cin, time_embed_dim, dropout, out_channels=cout, dims=dims,
                              use_checkpoint=use_checkpoint, num_frames=num_frames, alpha=alpha)

        def stt(ch, depth):
            return SpatialTemporalTransformer(
                ch, ch // num_head_channels, num_head_channels, depth=depth, context_dim=context_dim,
                use_linear=use_linear_in_transformer, attn_type=spatial_transformer_attn_type,
                use_checkpoint=use_checkpoint, num_frames=num_frames, alpha=alpha,
                temporal_transformer_attn_type=temporal_transformer_attn_type,
                spatial_only_attn_type=spatial_only_attn_type, insert_crossview=insert_crossview)

        self.input_blocks = nn.ModuleList([TimestepEmbedSequential(conv_nd(dims, in_channels, model_channels, 3, padding=1))])
        input_block_chans = [model_channels]
        ch, ds = model_channels, 1
        for level, mult in enumerate(channel_mult):
            for _ in range(self.num_res_blocks[level]):
                layers = [res(ch, mult * model_channels)]
                ch = mult * model_channels
                if ds in attention_resolutions:
                    layers.append(stt(ch, transformer_depth[level]))
                self.input_blocks.append(TimestepEmbedSequential(*layers))
                input_block_chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(TimestepEmbedSequential(Downsample(ch, conv_resample, dims=dims, out_channels=ch)))
                input_block_chans.append(ch)
                ds *= 2
        self.middle_block = TimestepEmbedSequential(res(ch, ch), stt(ch, transformer_depth_middle), res(ch, ch))
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(self.num_res_blocks[level] + 1):
                ich = input_block_chans.pop()
                layers = [res(ch + ich, model_channels * mult)]
                ch = model_channels * mult
                if ds in attention_resolutions:
                    layers.append(stt(ch, transformer_depth[level]))
                if level and i == self.num_res_blocks[level]:
                    layers.append(Upsample(ch, conv_resample, dims=dims, out_channels=ch))
                    ds //= 2
                self.output_blocks.append(TimestepEmbedSequential(*layers))
        self.out = nn.Sequential(normalization(ch), nn.SiLU(),
                                 zero_module(conv_nd(dims, model_channels, out_channels, 3, padding=1)))
        self._init_packable()

    def invalidate_packed(self):
        super().invalidate_packed()
        self.__dict__.pop("_text_proj", None)
        self.__dict__.pop("_emb_proj", None)

    # engine.FrameShard when the frames of every sample are sharded over a process group (panacea_amd.parallel); the
    # batch then carries num_frames / G frames per sample
    frame_shard = None
    view_shard = None          # engine.ViewShard: this rank's batches carry a band of views only

    # Operand precision policy (engine.Precision or "fast" | "precise" | "precise-all").  "precise" carries the operand
    # classes that dominate the eps error as split fp16 pairs and meets the 1e-3 max-abs contract of the boundary
    # (wrappers.py:37-70); "fast" is plain fp16 operands everywhere (2.3e-3 at BASELINE config 3).
    # Not set explicitly, the policy follows the NETWORK: "precise", except where a temporal GroupNorm group holds fewer than
    # 4 values (num_frames * C / 32: the 64-channel single-frame nets, BASELINE config 1) — the normalisation of 2 values
    # amplifies the rounding of its conv3x3 input 4-6x, so those get every class split ("precise-all") and a
    # warning that the configuration sits at 1.0-2.2e-3, above the 1e-3 the wide networks meet.
    @property
    def precision(self):
        p = self.__dict__.get("_precision")
        if p is not None:
            return p
        auto = self.__dict__.get("_auto_precision")
        if auto is None:
            # (a subclass / test net without a ResBlock3D has no temporal GroupNorm to protect: plain `precise`)
            gmin = min(((m.out_channels // 32) * m.num_frames for m in self.modules() if isinstance(m, ResBlock3D)), default=4)
            auto = "precise" if gmin >= 4 else "precise-all"
            if auto != "precise":
                import warnings
                warnings.warn(f"panacea_amd: temporal GroupNorm groups of this network hold {gmin} values (num_frames x C/32); "
                              "operand policy 'precise-all' selected, measured eps max-abs 1.0-2.2e-3 on such networks "
                              "(the 1e-3 contract is met from 4 values per group on: DESIGN.md section 6)", stacklevel=3)
            self.__dict__["_auto_precision"] = auto
        return auto

    @property
    def eps_contract(self) -> dict:
        """The numeric contract of THIS network under its operand policy: the eps max-abs bound against the reference's fp32
        forward that the parity tests gate ("numeric contract per configuration").
        1e-3 (BASELINE.json north_star) wherever a temporal GroupNorm group holds >= 4 values — every configuration of the
        Panacea+ network, T = 1 included; the 64-channel single-frame toy networks (BASELINE config 1 as written) are
        ill-conditioned there — a GroupNorm over TWO values is d / sqrt(d^2 + eps), slope 1/sqrt(eps) = 316 at d = 0 — and are
        stated, and gated, at 2.5e-3 with every operand class split.
        The bound does not depend on the clip length inside the supported range 1 <= num_frames <= 16 (longer clips are refused at
        construction): more frames per temporal group is better conditioned.  Measured on the MI355X against the reference's own
        forward, 64-channel test network: 7.6e-4 at 12 frames, 7.4e-4 at 16 (`precise`; tests/test_long_clips_gpu.py)."""
        gmin = min(((m.out_channels // 32) * m.num_frames for m in self.modules() if isinstance(m, ResBlock3D)), default=4)
        prec = self.precision
        esc = self.__dict__.get("_escalated")
        if E.is_wide(prec):
            # every operand class split with fp16 lo planes: the range of the bound is fp16's own (measured 8.5e-6 eps in the CPU
            # error budget of the heavy-tail weight set)
            out = {"policy": prec, "eps_max_abs": 1e-3 if gmin >= 4 else 2.5e-3, "values_per_temporal_group": gmin,
                   "valid_for": "|operand| < 65504"}
            if E.precision(prec).weights:
                # `precise-full`: the weights of this network are split as well, so the bound holds for fp32 checkpoints — it no longer
                # asks for fp16-representable weights (|w| < 65504 like every operand).  The first-stage VAE and the text tower are
                # outside this network and keep single fp16 weights.
                out["weights"] = "split (fp16 hi + lo planes): fp32 checkpoints, |w| < 65504"
            else:
                out["weights"] = "single fp16: the bound is stated on fp16-representable weights"
            if esc is not None:
                out["escalated_from"], out["trigger_count"] = esc["from"], esc["trigger_count"]
            return out
        if prec in ("fast",):
            return {"policy": prec, "eps_max_abs": None, "note": "plain fp16 operands: measured 2.0-2.6e-3, no stated bound"}
        if gmin >= 4:
            # Range of the bound (round 5, the heavy-tail pin tests/golden/full_cfg3_t500_tail64.npz): an fp16 operand carries 11 bits
            # whatever the policy, and the e4m3 lo plane of a split operand — (v - fp16(v)) * 2^11, clamped at 448 — stops adding to them
            # from |v| = 512 on (include/panacea_hip.h).  With "massive activation" channels that take the residual stream to
            # |v| = 1.8e3 (synth.synth_tensor tail = 64) the measured eps error is 2.3e-3 max / 3.3e-4 mean against the reference's fp32
            # forward: the stream-class convs (skip 1x1, Down / Upsample, zero convs) see those channels at fp16 precision.  Beyond
            # |operand| = 65504 an fp16 path overflows (non-finite eps; the reference's own autocast path does too).
            out = {"policy": prec, "eps_max_abs": 1e-3, "values_per_temporal_group": gmin,
                   "valid_for": "residual stream |v| < 512 (every operand of a split class inside the e4m3 lo plane's range)",
                   "beyond": {"stream_max_abs": 1.8e3, "eps_max_abs_measured": 2.3e-3, "eps_mean_abs_measured": 3.3e-4,
                              "pin": "tests/golden/full_cfg3_t500_tail64.npz"}}
            if E.weights_beside(prec):
                # `precise-ckpt`: `precise` with the weights of this network split (the A_hi * W_lo products of every GEMM, the joined
                # weights of the small-M linears), so the bound holds for fp32 checkpoints inside `precise`'s activation range
                out["weights"] = "split (fp16 hi + lo planes): fp32 checkpoints, |w| < 65504"
                out["note"] = ("the text tower and the first-stage VAE are outside this network and keep single fp16 weights; "
                               "full-size parity on unrounded weights has no golden and is unmeasured (tiny network: 7.3e-4)")
            return out
        return {"policy": prec, "eps_max_abs": 2.5e-3, "values_per_temporal_group": gmin,
                "note": "temporal GroupNorm over fewer than 4 values amplifies its input's rounding (measured 1.0-2.2e-3)"}

    @precision.setter
    def precision(self, value):
        E.precision(value)                                   # validates
        self.__dict__["_precision"] = value
        cn = self._modules.get("controlnet") if hasattr(self, "_modules") else None
        if cn is not None:
            cn.precision = value

    # ---- range monitor (round 6).  `eps_contract` is valid while no split operand leaves the e4m3 lo
    # plane's range (|v| < 512).  The library counts the lo-plane quads that clamped (pnc_range_monitor_collect: every e4m3 pack goes
    # through one helper); one collect per evaluation, read back WITHOUT a device synchronisation (pinned word + event, taken in at the
    # next evaluation or when `lo_clamped` is asked for).  The reference has no counterpart (wrappers.py:37-70 runs fp32 on CPU / an
    # unguarded autocast on CUDA).
    range_monitor = True
    # what happens when an evaluation left the range: "warn" (once per network), "raise", or "escalate" (below).  (fp16 lo planes on the
    # classes of `precise` alone only cut the heavy-tail error by a quarter, 1.3e-2 -> 9.9e-3 on the tiny network: the massive channels
    # amplify the fp16 rounding of the operands `precise` never splits.  "precise-wide" splits those too: 3.9e-5 there.)
    on_range_exceeded = "warn"
    # "escalate": an eager evaluation under an e4m3 policy drains the counters before it starts, reads its own clamp count
    # synchronously after it, and — count > 0 — switches this network (and its ControlNet) to "precise-wide" for good and evaluates
    # the same inputs again; that result is returned.  Costs one device synchronisation per evaluation until it has escalated.
    RANGE_MODES = ("warn", "raise", "escalate")

    @property
    def escalated(self) -> bool:
        """True once an "escalate" evaluation has switched this network to "precise-wide" """
        return self.__dict__.get("_escalated") is not None

    def _range_count_sync(self, device) -> int:
        """the clamp count since the previous collect, read back now (one device synchronisation)"""
        self._range_monitor_poll(wait=True)                  # (asynchronous collects of earlier evaluations first)
        buf = torch.zeros(1, dtype=torch.int32, device=device)
        E.backend().range_monitor_collect(buf)
        return int(buf[0].item())

    def _escalate(self, count: int):
        """switch this network and its ControlNet to "precise-wide" (sticky); packed weights do not depend on the policy, the text
        K/V, lo planes and workspaces of later evaluations are allocated under the new one"""
        self.__dict__["_escalated"] = {"from": self.precision, "trigger_count": count}
        st = self._range_state()
        st["last"], st["evals"], st["total"] = count, st["evals"] + 1, st["total"] + count
        # from `precise-ckpt` the weights stay split: its escalation target is `precise-full`
        self.precision = "precise-full" if E.weights_beside(self.precision) else "precise-wide"

    def _check_unsharded_policy(self):
        """precise-wide and "escalate" are single-device features: the split attention kernels have no halo views and sharded
        evaluations are not re-run"""
        if self.frame_shard is None and self.view_shard is None:
            return
        if self.on_range_exceeded == "escalate" or E.single_device_only(self.precision):
            raise ValueError("the 'precise-wide' operand policy (and 'precise-full', 'precise-ckpt') and on_range_exceeded='escalate' do "
                             "not run frame- or view-sharded")

    def _evaluate(self, once, device):
        """once(collect) runs ONE evaluation under the current policy (collect: enqueue the asynchronous range-monitor collect at its
        end) and returns its output; this wraps it in the escalate protocol (see on_range_exceeded)"""
        if self.on_range_exceeded not in self.RANGE_MODES:
            raise ValueError(f"on_range_exceeded must be one of {self.RANGE_MODES}, got {self.on_range_exceeded!r}")
        self._check_unsharded_policy()
        if self.on_range_exceeded == "escalate" and not self.escalated and _capturing(device):
            # a captured graph replays kernels only: the monitor would never run again (graph.refuse_unescalated says the same
            # before a capture starts when it is given the network; this holds however the graph is built)
            raise ValueError("on_range_exceeded='escalate' is not monitored during graph replay: capture the network after it has "
                             "escalated, or use 'warn' / 'raise'")
        if (self.on_range_exceeded != "escalate" or self.escalated or not self.range_monitor or not E.precision(self.precision).lo8
                or _capturing(device)):
            return once(True)
        self._range_count_sync(device)                       # drain: the count read below belongs to THIS evaluation
        out = once(False)
        n = self._range_count_sync(device)
        if n <= 0:
            st = self._range_state()
            st["last"], st["evals"] = 0, st["evals"] + 1
            return out
        self._escalate(n)
        return once(True)


    # ---- range profile (engine.RangeProfile): opt-in statistics of every GEMM operand, per operand class and per site.  Off (the
    # default) the runtimes carry no profile and engine.gemm launches, allocates and synchronises nothing for it.
    @contextlib.contextmanager
    def profile_ranges(self, slots: int = 4096, evaluations: Optional[int] = None):
        """Context manager -> engine.RangeProfile.  Inside it every evaluation of this network and of its ControlNet — direct calls,
        `denoise`, a sampler's steps, both side streams — adds the range statistics of the A operand of each GEMM to the profile
        (one pnc_operand_stats_f16 launch per operand, on the stream of its GEMM); `report()` / `recommend(network)` read them.
        `evaluations`: observe only the first that many (a sampler run then pays for the statistics in its first steps only).
        Single-device and eager, like `escalate`: refused on a frame- or view-sharded network and while a stream is capturing."""
        cn = self._modules.get("controlnet")
        for net in (self, cn):
            if net is not None and (net.frame_shard is not None or net.view_shard is not None):
                raise ValueError("the range profile does not run frame- or view-sharded")
        device = next(self.parameters()).device
        if _capturing(device):
            raise ValueError("the range profile launches a statistics kernel per operand and reads its table on the host: it cannot "
                             "be started while a stream is capturing")
        if self.__dict__.get("_profile") is not None:
            raise ValueError("this network is being profiled already")
        prof = E.RangeProfile(device, slots)
        prof.limit = evaluations
        prof.bind(self)
        for net in (self, cn):
            if net is not None:
                net.__dict__["_profile"] = prof
        try:
            yield prof
        finally:
            for net in (self, cn):
                if net is not None:
                    net.__dict__.pop("_profile", None)

    def _observed(self, rt: Runtime, evaluation: bool = True) -> Runtime:
        """hand the active range profile (if any) to the runtime of an evaluation"""
        prof = self.__dict__.get("_profile")
        if prof is not None and (prof.limit is None or prof.evaluations < prof.limit):
            if _capturing(rt.device):
                raise ValueError("the range profile does not run while a stream is capturing")
            if rt.shard is not None or rt.vshard is not None:
                raise ValueError("the range profile does not run frame- or view-sharded")
            rt.profile = prof
            if evaluation:
                prof.begin_evaluation()
        return rt

    def _range_state(self) -> dict:
        st = self.__dict__.get("_range_st")
        if st is None:
            st = self.__dict__["_range_st"] = {"pending": [], "last": None, "total": 0, "evals": 0, "warned": False, "slot": 0,
                                                "dev": None, "host": None}
        return st

    def _range_monitor_take(self, n: int):
        st = self._range_state()
        st["last"], st["evals"] = n, st["evals"] + 1
        if n <= 0:
            return
        st["total"] += n
        msg = (f"panacea_amd: {n} e4m3 lo-plane quads saturated in one evaluation — a split operand left |v| < 512, the range the "
               f"eps max-abs {self.eps_contract.get('eps_max_abs')} contract of the '{self.precision}' policy is written for "
               "(UNetModel3D.eps_contract; measured 2.3e-3 with the residual stream at 1.8e3)")
        if self.on_range_exceeded == "raise":
            raise RuntimeError(msg)
        if not st["warned"]:
            import warnings
            st["warned"] = True
            warnings.warn(msg, stacklevel=4)

    def _range_monitor_poll(self, wait: bool = False):
        st = self._range_state()
        while st["pending"]:
            host, idx, ev = st["pending"][0]
            if not (wait or ev.query()):
                break
            if wait:
                ev.synchronize()
            st["pending"].pop(0)
            self._range_monitor_take(int(host[idx]))

    def _range_monitor_collect(self, rt: Runtime):
        """enqueue the collect of this evaluation's clamp count (after the last kernel of the evaluation, on the current stream)"""
        if not self.range_monitor or not rt.prec.lo8:
            return
        if rt.device.type != "cuda":
            buf = torch.zeros(1, dtype=torch.int32, device=rt.device)
            rt.be.range_monitor_collect(buf)
            self._range_monitor_take(int(buf[0]))
            return
        if torch.cuda.is_current_stream_capturing():
            return                                  # (a captured step replays kernels only; the monitor runs in eager evaluations)
        self._range_monitor_poll()
        st = self._range_state()
        if st["dev"] is None or st["dev"].device != rt.device:
            st["dev"] = torch.zeros(64, dtype=torch.int32, device=rt.device)
            st["host"] = torch.zeros(64, dtype=torch.int32).pin_memory()
        if len(st["pending"]) >= 32:
            self._range_monitor_poll(wait=True)
        i = st["slot"] = (st["slot"] + 1) % 64
        st["dev"][i:i + 1].zero_()
        rt.be.range_monitor_collect(st["dev"][i:])
        st["host"][i:i + 1].copy_(st["dev"][i:i + 1], non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        st["pending"].append((st["host"], i, ev))

    @property
    def lo_clamped(self):
        """e4m3 lo-plane quads that saturated in the most recent evaluation (waits for it; None before the first; 0 = inside the
        range of `eps_contract`)"""
        self._range_monitor_poll(wait=True)
        return self._range_state()["last"]

    @property
    def lo_clamped_total(self) -> int:
        self._range_monitor_poll(wait=True)
        return self._range_state()["total"]

    def _project_text(self, rt: Runtime):
        """Text K/V of every cross-attention site of this network, batched (attention.TextKVProjector)."""
        from .attention import TextKVProjector
        if rt.text_frozen:
            return
        tp = self.__dict__.get("_text_proj")
        if tp is None:
            tp = TextKVProjector(_OwnBlocks(self))
            self.__dict__["_text_proj"] = tp
        tp.run(rt)

    def _project_emb(self, rt: Runtime, emb32: torch.Tensor):
        """emb_layers(emb) of every ResBlock3D of this network in one launch (EmbProjector); not in a layout whose temporal sites
        read the rows of ALL frames (rt.emb_all)"""
        if E.temporal_layout(rt).emb_all or not E.EMB_BATCH:
            return
        ep = self.__dict__.get("_emb_proj")
        if ep is None:
            ep = EmbProjector(_OwnBlocks(self))
            self.__dict__["_emb_proj"] = ep
        ep.run(rt, emb32)

    # ---- packed parameters owned by the network itself (time embedding MLP, output head)
    def _pack(self, lo=False):
        te = self.time_embed
        pk = dict(tw0=E.pk_linear(te[0].weight, lo), tb0=E.pk_f32(te[0].bias),
                  tw2=E.pk_linear(te[2].weight, lo), tb2=E.pk_f32(te[2].bias))
        if hasattr(self, "out"):
            pk["og"], pk["ob"] = E.pk_f32(self.out[0].weight), E.pk_f32(self.out[0].bias)
            pk["ow"], pk["oc"] = E.pk_conv3x3(self.out[2].weight, lo=lo), E.pk_f32(self.out[2].bias)
        return pk

    def _time_embedding(self, rt: Runtime, timesteps: torch.Tensor) -> torch.Tensor:
        """timestep_embedding -> Linear -> SiLU -> Linear, all fp32 activations (util.py:224-248, :936-943)."""
        pk = self.packed()
        mc, td = self.model_channels, self.time_embed_dim
        if mc % 8:
            raise NotImplementedError("model_channels must be a multiple of 8")
        t_emb = timestep_embedding(timesteps.to(rt.device), mc)
        h = E.small_linear(rt, t_emb, pk, "tw0", "tb0", rt.F, td, mc, silu_out=True)
        # returns SiLU(emb): every consumer of emb (ResBlock3D.emb_layers, :468-476) starts with nn.SiLU
        emb = E.small_linear(rt, h, pk, "tw2", "tb2", rt.F, td, td, silu_out=True)
        if rt.shard is not None:
            # the temporal sites run on all T frames of a pixel: they index the embedding rows of ALL frames (40 KB)
            rt.emb_all = rt.shard.gather_rows(emb, rt.B)
        return emb

    def _head(self, rt: Runtime, h: Act, tokens: bool = False):
        """self.out: GN + SiLU + conv3x3 -> NCHW fp32 (:1245-1253, controlmodel.py:197-202); `tokens`: the channels-last
        fp32 tokens instead (consumed by the fused sampler-step exit, pnc_cfg_euler_step)."""
        pk = self.packed()
        a = E.gn_spatial(rt, h.f32, h.F, h.N, h.C, pk["og"], pk["ob"], 1e-5, True, split="gn_head", tail_rows=rt.band_tail_rows(h.F, h.H))
        o = run_conv3x3(rt, a, h.F, h.H, h.W, h.C, pk, "ow", self.out_channels, pk["oc"])
        if tokens:
            return o
        out = rt.empty((h.F, self.out_channels, h.H, h.W), torch.float32)
        rt.be.tokens_to_nchw_f32(o.f32, self.out_channels, h.F, h.N, self.out_channels, out)
        return out

    def _stem_tokens(self, rt: Runtime, x: torch.Tensor, concat: Optional[torch.Tensor] = None,
                     scale: Optional[torch.Tensor] = None) -> Act:
        """NCHW network input -> channels-last fp16 tokens (channel count padded to 8).  Fused sampler entry: `x` is the
        latent of ONE CFG half (x.shape[0] divides the batch: both halves read it), scaled per frame by `scale` (c_in of
        DiscreteDenoiser), with `concat` appended on the channel axis (wrappers.py:41) — no torch.cat, no x * c_in pass."""
        Fx, C, H, W = x.shape
        F = Fx if concat is None else concat.shape[0]
        C2 = 0 if concat is None else concat.shape[1]
        cp = (C + C2 + 7) // 8 * 8
        x32 = x.detach().to(torch.float32).contiguous()
        b32 = None if concat is None else concat.detach().to(torch.float32).contiguous()
        t16 = rt.operand((F * H * W, cp), "stem")
        rt.be.nchw_to_tokens_f16(x32, C, b32, C2, F, H * W, cp, *t16, a_scale=scale, a_frames=Fx)
        return Act(F, H, W, cp, f16=t16)

    def _own_blocks(self):
        for name in ("input_blocks", "middle_block", "output_blocks"):
            if hasattr(self, name):
                yield getattr(self, name)

    def _run_unet(self, rt: Runtime, x16: Act, emb32: torch.Tensor, control, tokens: bool = False):
        """controlmodel.py:186-202 / openaimodel.py:1305-1319 on tokens.  `control` is None, the list of ControlNet
        residuals, or a callable returning that list (called after the middle block: the join point when the
        ControlNet runs on a second stream)."""
        self._project_text(rt)
        self._project_emb(rt, emb32)
        hs, h = [], x16
        nb = len(self.input_blocks)
        for i, module in enumerate(self.input_blocks):
            nxt = self.input_blocks[i + 1] if i + 1 < nb else None
            wf = nxt is not None and isinstance(nxt[0], Downsample)
            h = module._run(rt, h, emb32, want_f16=wf)
            hs.append(h)
            if rt.trace is not None:
                rt.trace[f"input_blocks.{i}"] = h.to_nchw()
        h = self.middle_block._run(rt, h, emb32)
        if rt.trace is not None:
            rt.trace["middle_block"] = h.to_nchw()
        if callable(control):
            control = control()
        if control is not None:
            c = control.pop()
            rt.be.add_f32(h.f32, c.f32, h.M * h.C, h.f32, None)                       # h += control.pop()
            h.gn_part = None                                                           # (statistics of the old values)
        for i, module in enumerate(self.output_blocks):
            s = hs.pop()
            c = control.pop() if control is not None else None
            ct = h.C + s.C
            cat32 = rt.empty((h.M, ct), torch.float32)
            cat16 = rt.operand((h.M, ct), "stream")
            # th.cat([h, hs.pop() + control.pop()], dim=1): one pass, fp32 stream + fp16 operand (of the skip 1x1 conv)
            # (round 5: the same pass writes the statistics of the GroupNorm that reads the concat — the first norm of the block's
            # ResBlock3D —: 12 statistics launches and their read of C1 + C2 fp32 channels per step gone)
            part, ppc = None, E._ppc(h.H * h.W)
            if ct % 64 == 0 and E.GN_FROM_EPILOGUE:
                part = rt.empty((h.F * (-(-(h.H * h.W) // ppc)) * 96,), torch.float32)
            rt.be.concat_add(h.f32, h.C, s.f32, None if c is None else c.f32, s.C, h.M, cat32, *cat16,
                             **({} if part is None else dict(gn_part=part, frames=h.F, ppc=ppc)))
            h = module._run(rt, Act(h.F, h.H, h.W, ct, f32=cat32, f16=cat16, gn_part=part), emb32)
            if rt.trace is not None:
                rt.trace[f"output_blocks.{i}"] = h.to_nchw()
        return self._head(rt, h, tokens)

    def forward(self, x, timesteps=None, context=None, y=None, **kwargs):
        """openaimodel.py:1279-1319 — x (B*T, C, h, w), timesteps (B*T,), context (B, 77, D)."""
        assert (y is not None) == (self.num_classes is not None), \
            "must specify y if and only if the model is class-conditional"
        from .util import runtime_for

        def once(collect):
            rt = self._observed(runtime_for(x, self.num_frames, self.frame_shard, self.view_shard))
            rt.prec = E.precision(self.precision)
            rt.set_context(context)
            emb = self._time_embedding(rt, timesteps)
            out = self._run_unet(rt, self._stem_tokens(rt, x), emb, None)
            if collect:
                self._range_monitor_collect(rt)
            return out
        with torch.no_grad():
            out = self._evaluate(once, x.device)
        return out.to(x.dtype)
