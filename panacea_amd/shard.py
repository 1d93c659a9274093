"""The two intra-sample shardings of the denoising path over a `torch.distributed` process group — `FrameShard` (the T frames of a
sample over G ranks) and `ViewShard` (the six camera views over G ranks) — and the one place that talks to the group, `_Link`.

A shard method says WHO GETS WHICH BYTES; the link issues the collective.  Every neighbour / transpose exchange is one
`all_to_all_single` with split sizes (`_Link.exchange`): messages are flat uint8 parts per destination rank, the parts come back per
source rank.  Typed tensors become such parts through `_pack` / `_unpack`.  RCCL over xGMI on MI355X ("nccl"), gloo in the CPU tests;
with a gloo group device tensors are staged through host memory (two processes on one GPU: RCCL refuses two ranks on one device);
`group=None` with G = 1 is the loop-back that drives every exchange site on one device.  This module does not import `engine`.
"""
from __future__ import annotations

import torch
import torch.distributed as dist


def _pack(tensors, by_row: bool = False):
    """typed tensors (None entries are skipped) -> (uint8 message, spec for `_unpack`).  Flat: [tensor 0's bytes | tensor 1's | ...].
    `by_row`: the tensors share dim 0 and the message is [rows, bytes per row], row r = [tensors[0][r]'s bytes | tensors[1][r]'s | ...]
    — it can be cut and permuted along the rows like any of its planes."""
    keep = [t for t in tensors if t is not None]
    rows = keep[0].shape[0] if by_row else 1
    msg = torch.cat([t.contiguous().view(rows, -1).view(torch.uint8) for t in keep], dim=1)
    spec = [None if t is None else (t.dtype, tuple(t.shape[1:] if by_row else t.shape)) for t in tensors]
    return (msg if by_row else msg.view(-1)), spec


def _unpack(msg: torch.Tensor, spec, by_row: bool = False):
    """inverse of `_pack` (None entries come back as None); `by_row`: of a message with any number of rows.  The flat form hands out
    views of the message, so a tensor's byte offset in it must be a multiple of its element size."""
    rows = msg.shape[0] if by_row else 1
    msg, out, o = msg.view(rows, -1), [], 0
    for s in spec:
        if s is None:
            out.append(None)
            continue
        dt, shape = s
        nb = dt.itemsize * int(torch.Size(shape).numel())
        t = msg[:, o:o + nb].contiguous().view(dt)
        out.append(t.view(rows, *shape) if by_row else t.view(shape))
        o += nb
    return out


class Pending:
    """An exchange in flight.  Kernels enqueued between `*_start()` and `result()` run UNDER the transfer (RCCL executes
    the collective on its own stream; the compute stream only waits in `result()`): the independent work every ResBlock3D
    site has — the skip 1x1 conv and the `emb_layers` linear — goes there."""

    def __init__(self, recv, work, finish):
        self._recv, self._work, self._finish = recv, work, finish

    def result(self):
        if self._work is not None:
            self._work.wait()
            self._work = None
        return self._finish(self._recv)


class _Link:
    """Rank `index` of the G ranks of `group`, as a shard sees it: issues the collectives, stages device tensors through host memory
    when the group is gloo, and keeps the accounting for bench / DESIGN §9 (this rank, since construction): `exchanges` counts the
    collectives on an evaluation's dependency chain (the all-gathers that assemble a result at the end of a schedule are not
    counted), `bytes_sent` what they address to other ranks.  `group=None` (G = 1) is the loop-back: counted, nothing moves."""

    def __init__(self, G: int, index: int, group):
        self.G, self.index, self.group = G, index, group
        self.host = group is not None and dist.get_backend(group) == "gloo"
        self.exchanges = 0
        self.bytes_sent = 0

    def _staged(self, t: torch.Tensor) -> torch.Tensor:
        return t.cpu() if self.host and t.device.type != "cpu" else t

    def a2a_start(self, send: torch.Tensor, in_split, out_split, finish=lambda recv: recv) -> Pending:
        """ONE all_to_all_single: `send` is a flat uint8 tensor whose consecutive in_split[r] bytes go to rank r -> Pending of
        finish(recv), recv = out_split[r] bytes from every rank r in rank order.  Only the direct path is in flight on return (`work` is
        the handle of the collective running on the communicator's own stream, `wait()` orders the CURRENT stream behind it); the staged
        one has completed.  Loop-back: `recv` is `send`."""
        self.exchanges += 1
        self.bytes_sent += send.numel() - in_split[self.index]
        if self.group is None:
            return Pending(send, None, finish)
        host = self._staged(send)
        recv = torch.empty(sum(out_split), dtype=torch.uint8, device=host.device)
        work = dist.all_to_all_single(recv, host, output_split_sizes=out_split, input_split_sizes=in_split, group=self.group,
                                      async_op=host is send)
        return Pending(recv, work, finish) if host is send else Pending(recv.to(send.device), None, finish)

    def exchange_start(self, out: dict, sizes_in: dict, device=None) -> Pending:
        """out: {destination rank: [flat uint8 parts]}, sizes_in: {source rank: [bytes of each part expected from it]} (ranks that
        get / send nothing are left out) -> Pending of {source rank: [parts]}.  Nothing depends on message tags or on the posting
        order of point-to-point operations (RCCL ignores tags and matches same-peer sends by order): two parts for one peer are one
        message.  Loop-back: the caller's own parts for this rank come back, themselves.  `device`: needed when `out` is empty."""
        G = self.G
        if self.group is None:
            self.exchanges += 1
            return Pending({self.index: list(out.get(self.index, ()))}, None, lambda got: got)
        parts = [p for r in range(G) for p in out.get(r, ())]
        send = torch.cat(parts) if parts else torch.empty(0, dtype=torch.uint8, device=device)

        def split(recv):
            got, o = {}, 0
            for r in sorted(sizes_in):
                got[r] = []
                for n in sizes_in[r]:
                    got[r].append(recv[o:o + n])
                    o += n
            return got
        return self.a2a_start(send, [sum(p.numel() for p in out.get(r, ())) for r in range(G)],
                              [sum(sizes_in.get(r, ())) for r in range(G)], split)

    def exchange(self, out: dict, sizes_in: dict, device=None) -> dict:
        return self.exchange_start(out, sizes_in, device).result()

    def all_reduce(self, t: torch.Tensor) -> torch.Tensor:
        """in-place sum over the group; counted as a ring all-reduce: 2 (G-1)/G of the payload"""
        self.exchanges += 1
        if self.group is not None:
            buf = self._staged(t)
            dist.all_reduce(buf, op=dist.ReduceOp.SUM, group=self.group)
            self.bytes_sent += 2 * t.numel() * t.element_size() * (self.G - 1) // self.G
            if buf is not t:
                t.copy_(buf)
        return t

    def all_gather_flat(self, t: torch.Tensor) -> torch.Tensor:
        """flat `t` of every rank in rank order, [G * numel], where the collective ran (host memory when staged); counted"""
        self.exchanges += 1
        if self.group is None:
            return t
        send = self._staged(t).contiguous()
        got = torch.empty(self.G * send.numel(), dtype=send.dtype, device=send.device)
        dist.all_gather_into_tensor(got, send, group=self.group)
        self.bytes_sent += send.numel() * send.element_size() * (self.G - 1)
        return got

    def all_gather(self, t: torch.Tensor) -> list:
        """`t` of every rank, where the collective ran; assembles a result outside an evaluation's exchange sites: not counted"""
        send = self._staged(t.contiguous())
        parts = [torch.empty_like(send) for _ in range(self.G)]
        dist.all_gather(parts, send, group=self.group)
        return parts


class _Sharded:
    """what both shards share: validation aside, the link and its counters"""

    def __init__(self, G: int, index: int, group):
        self.G, self.index, self.group = G, index, group
        self._link = _Link(G, index, group)

    exchanges = property(lambda self: self._link.exchanges)
    bytes_sent = property(lambda self: self._link.bytes_sent)


class FrameShard(_Sharded):
    """The T frames of every sample sharded over the G ranks of a process group: rank g of the group
    holds frames [g*T/G, (g+1)*T/G) of each sample — whole panoramic frames, so every spatial op (3x3 convs, spatial
    GroupNorm, intra-/cross-view attention) stays local.  The cross-frame couplings of the path,
        ResBlock3D   temporal GroupNorm + conv1d            (openaimodel.py:505-515, 533-539)
        STT          temporal transformer branch            (attention.py:1106-1134)
    are all POINTWISE PER PIXEL across frames, so they run in the transposed sharding: all T frames of N/G pixels per
    rank.  `to_pixels` / `to_frames` are the two exchanges (one all-to-all each: a rank sends (G-1)/G of its slab and
    receives as much — half the received bytes of all-gathering the slab, and the unmodified kernels run on both sides);
    `gather_rows` all-gathers tiny per-frame rows (the timestep embedding)."""
    Pending = Pending

    def __init__(self, G: int, index: int, group=None, resblock: str = "halo"):
        if G < 1 or not (0 <= index < G):
            raise ValueError(f"bad frame shard {index} of {G}")
        if G > 1 and group is None:
            raise ValueError("a frame shard over more than one rank needs its process group")
        if resblock not in ("halo", "transpose"):
            raise ValueError("resblock: 'halo' (statistics all-reduce + neighbour frames, round 4) or 'transpose' (round 2: the "
                             "fp32 stream to the pixel sharding and back)")
        super().__init__(G, index, group)
        self.resblock = resblock

    def _chunks_start(self, send: torch.Tensor, finish) -> Pending:
        """equal chunks: send[r] goes to rank r -> Pending of finish(recv), recv[r] = what rank r addressed to this rank"""
        if self.group is None:
            send = send.clone()          # G = 1: the caller's permute can alias its input, and `finish` its output
        n = send[0].numel() * send.element_size()
        return self._link.a2a_start(send.view(-1).view(torch.uint8), [n] * self.G, [n] * self.G,
                                    lambda recv: finish(recv.view(send.dtype).view(send.shape)))

    def to_pixels_start(self, x: torch.Tensor, B: int, N: int) -> Pending:
        G = self.G
        if N % G:
            raise ValueError(f"{N} pixels per frame do not split over {G} frame groups")
        C = x.shape[-1]
        Tl, Np = x.shape[0] // (B * N), N // G
        send = x.view(B, Tl, G, Np, C).permute(2, 0, 1, 3, 4).contiguous()      # [dest pixel group, b, t_l, p, c]
        return self._chunks_start(send, lambda r: r.permute(1, 0, 2, 3, 4).contiguous().view(B * G * Tl * Np, C))   # r: [src frame group, ...]

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
        return self._chunks_start(send, lambda r: r.permute(1, 2, 0, 3, 4).contiguous().view(B * Tl * N, C)).result()   # r: [src pixel group, ...]

    # the planes of ONE operand (fp16 hi + e4m3 / fp16 lo) travel in ONE exchange — row-wise byte concatenation, one all_to_all instead
    # of one per plane: the STT temporal branch goes from 4 to 2 exchanges per site (92 -> 46 per evaluation)
    def to_pixels_planes(self, planes, B: int, N: int):
        """`to_pixels` of several planes of one operand (None entries pass through) in one exchange"""
        buf, spec = _pack(planes, by_row=True)
        return _unpack(self.to_pixels(buf, B, N), spec, by_row=True)

    def to_frames_planes(self, planes, B: int, N: int):
        buf, spec = _pack(planes, by_row=True)
        return _unpack(self.to_frames(buf, B, N), spec, by_row=True)

    # the ResBlock3D temporal sites WITHOUT moving the fp32 stream.  The temporal GroupNorm only needs
    # per-(pixel, group) sums over all T frames: every rank reduces its frames, the frame group adds the partial sums (256 B per pixel,
    # whatever C and T); the k = 3 temporal conv only needs ONE frame of the normalised fp16 operand from each neighbour rank.  Sent
    # per pixel-channel and site at G = 4: ~5.7 B instead of 12 (fp32 h to the pixel layout and back).
    def allreduce_sum(self, t: torch.Tensor) -> torch.Tensor:
        """in-place sum over the frame group (the temporal GroupNorm's partial sums)"""
        return self._link.all_reduce(t)

    def halo_frames(self, planes, B: int, Tl: int):
        """planes: tensors of [B, Tl + 2, N, C] (the (T + 2)-frame layout of PncGemmParams.t_halo; hi and lo plane of one operand)
        whose frames 1 .. Tl are this rank's.  Fills frame 0 with the previous rank's last frame and frame Tl + 1 with the next
        rank's first frame — zeros at the two ends of the clip (the conv's own zero padding in time, openaimodel.py:418,469).  One
        exchange inside the frame group: the planes' frame for the one or two neighbours, nothing for the other ranks."""
        G, me = self.G, self.index
        views = [p.view(B, Tl + 2, -1) for p in planes]
        out, sizes, spec = {}, {}, None
        for dest, frame in ((me - 1, 1), (me + 1, Tl)):
            if 0 <= dest < G:
                msg, spec = _pack([v[:, frame] for v in views])
                out[dest], sizes[dest] = [msg], [msg.numel()]        # what the neighbour sends has the size of what it gets
        got = self._link.exchange(out, sizes, planes[0].device)
        for src, slot in ((me - 1, 0), (me + 1, Tl + 1)):
            for v, t in zip(views, _unpack(got[src][0], spec) if src in sizes else [None] * len(views)):
                if t is None:
                    v[:, slot].zero_()
                else:
                    v[:, slot] = t

    def gather_rows(self, x: torch.Tensor, B: int) -> torch.Tensor:
        """[B*T_l, D] per-frame rows -> [B*T, D] (frames of a sample in global order)"""
        if self.group is None:
            return x.clone()
        D = x.shape[-1]
        Tl = x.shape[0] // B
        parts = self._link.all_gather(x)
        return torch.stack([p.view(B, Tl, D) for p in parts], dim=1).reshape(B * self.G * Tl, D).to(x.device)


class ViewShard(_Sharded):
    """The six camera views of every panoramic frame sharded over the G in {2, 3, 6} ranks of a process group: rank g holds
    views [g*6/G, (g+1)*6/G) — a band of W/G columns of every map, at every level.  Per pixel, per frame and per view work
    (1x1 convs, the temporal GroupNorm / conv1d / attention, LayerNorm, feed-forward, text attention, intra-view attention:
    attention.py:382-489) stays local.  What couples the views:

        3x3 convs (all)              one halo column per side from the neighbour band         `band_operand`
        spatial GroupNorm(32)        per-(frame, group) statistics over the whole panorama     `combine_stats`
        cross-view attention         keys / values of the two neighbouring views (circular:    `halo_views`
                                     attention.py:545-559; view 5 attends view 4 only)

    Neighbour exchanges address the two neighbours only (one xGMI link per neighbour pair on MI355X); the statistics are one tiny
    all-gather."""
    VIEWS = 6

    def __init__(self, G: int, index: int, group=None):
        if G not in (1, 2, 3, 6) or not (0 <= index < G):
            raise ValueError(f"bad view shard {index} of {G}: the six views split over 1 (loop-back), 2, 3 or 6 ranks")
        if G > 1 and group is None:
            raise ValueError("a view shard over more than one rank needs its process group")
        super().__init__(G, index, group)
        self.n_local = self.VIEWS // G
        self.first = index * self.n_local              # global index of this rank's first view

    def _exchange(self, to_left, to_right):
        """circular neighbour exchange: every tensor of `to_left` goes to the left neighbour, `to_right` to the right one ->
        (from_left, from_right) = what the neighbours sent towards this rank.  The tensors of a direction travel as one byte message."""
        bl, spec_l = _pack(to_left)
        br, spec_r = _pack(to_right)
        from_left, from_right = self._exchange_bytes(bl, br)
        return _unpack(from_left, spec_r), _unpack(from_right, spec_l)

    def _exchange_bytes(self, bl: torch.Tensor, br: torch.Tensor):
        """bl / br: flat uint8 messages (freshly packed — never aliased by the caller afterwards) for the left / right neighbour ->
        (bytes from the left neighbour = its `br`, bytes from the right neighbour = its `bl`).  At G = 2, and at G = 1 (`group=None`
        or a one-rank group: the band is the whole panorama and its own circular neighbour), both neighbours are ONE peer: it gets
        [to_left | to_right] as one message, and of a peer's message the first part is what it sent as my right neighbour."""
        left, right = (self.index - 1) % self.G, (self.index + 1) % self.G
        out, sizes = {}, {}
        out.setdefault(left, []).append(bl)
        out.setdefault(right, []).append(br)
        sizes.setdefault(right, []).append(bl.numel())     # the right neighbour's to_left batch
        sizes.setdefault(left, []).append(br.numel())      # the left neighbour's to_right batch
        got = self._link.exchange(out, sizes)
        return got[left][-1], got[right][0]

    def band_operand(self, rt, planes, F: int, H: int, W: int, C: int):
        """planes: [F*H*W, C] operand planes of this band (hi and lo plane of one conv operand) -> (planes', x_halo_off): each
        plane in ONE allocation [F*H*W + 2*F*H, C] whose tail holds image column -1 (from the left neighbour: [F][H][C]) and
        column W (from the right neighbour) of every row — zeros at the two ends of the panorama, the conv's own padding — and the
        element offset of that tail, PncGemmParams.x_halo_off.  The 3x3 gathers read the tail instead of padding (no widened copy of
        the band, no window copy of the conv's output).  A plane that came from Runtime.empty(..., tail_rows >= 2*F*H) is used in
        place; any other is copied once into such an allocation."""
        M, tail = F * H * W, 2 * F * H
        if all(getattr(p, "_pnc_halo_ready", False) and getattr(p, "_pnc_tail", None) is not None for p in planes):
            # the GroupNorm that wrote this operand already exchanged the neighbours' RAW edge columns together with its
            # statistics records (stats_and_halo) and normalised them into the tail: no second exchange in front of the conv
            return [p._pnc_tail for p in planes], M * C
        # the planes' edge columns travel as ONE byte message per direction, row (f, y) = [plane 0's C values | plane 1's | ...]:
        # one gather launch per direction whatever the number of planes (gathered straight from the strided columns, not by `_pack`)
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

    def combine_stats(self, part: torch.Tensor, F: int, nchunk: int, be) -> torch.Tensor:
        """part: the {n, mean, M2} records [F, nchunk, 32, 3] of this band (pnc_groupnorm_stats) -> records of the same shape
        whose Chan combination is the statistics of the whole panorama: slot 0 of every frame holds the combined record, the
        other slots are empty ({0, 0, 0} leaves the combination unchanged), so `pnc_groupnorm_apply` runs unmodified.  The
        records of the G bands are all-gathered (96 floats per frame and chunk) and combined by ONE small kernel of the backend `be`
        (`pnc_groupnorm_combine`, fp32 Chan updates in the fixed order (band, chunk) — the same arithmetic the apply kernel uses)."""
        mine = part.view(-1)[: F * nchunk * 96]
        allp = self._link.all_gather_flat(mine).to(part.device)
        out = torch.empty_like(mine)
        be.groupnorm_combine(allp, self.G, F, nchunk, out)
        return out

    # GroupNorm -> 3x3 conv of a view band in ONE exchange instead of two.  All-gathering the statistics
    # records, normalising, and then exchanging the NORMALISED edge columns (band_operand) is two exchanges on one dependency chain
    # at each of the 67 GroupNorm + conv sites of an evaluation.  The neighbour's normalised edge column is a function of its RAW
    # fp32 column and of the panorama's combined statistics — which this rank holds anyway — so the raw columns ride with the
    # records and each rank normalises the two columns it received with the same kernel, the same combined records: the same bits
    # as the neighbour computed (gloo tests: eps equal to the two-exchange form).
    fused_halo = True                 # False: the two exchanges (A/B, tests)

    def stats_and_halo(self, part: torch.Tensor, col_left: torch.Tensor, col_right: torch.Tensor, F: int, nchunk: int):
        """part: this band's records [F, nchunk, 32, 3]; col_left / col_right: its RAW fp32 edge columns [F, H, C] (image columns 0
        and W - 1) -> (records of all G bands in rank order [G * F * nchunk * 96], the left neighbour's column W - 1 or None at the left
        end of the panorama, the right neighbour's column 0 or None at the right end).  ONE exchange inside the view group:
        every rank gets the records, the two neighbours one column each on top."""
        G, me = self.G, self.index
        recs = part.reshape(-1)[: F * nchunk * 96].contiguous().view(torch.uint8)
        out, sizes = {r: [recs] for r in range(G)}, {r: [recs.numel()] for r in range(G)}
        # my column 0 is the left neighbour's column W, my column W - 1 the right neighbour's column -1; no wrap: zeros beyond both ends
        for r, col in ((me - 1, col_left), (me + 1, col_right)):
            if 0 <= r < G:
                out[r].append(col.contiguous().view(-1).view(torch.uint8))
                sizes[r].append(col.numel() * col.element_size())
        got = self._link.exchange(out, sizes)
        from_left = got[me - 1][1].view(col_left.dtype).view(col_left.shape) if me > 0 else None            # its column W - 1
        from_right = got[me + 1][1].view(col_right.dtype).view(col_right.shape) if me < G - 1 else None     # its column 0
        allrec = got[0][0] if G == 1 else torch.cat([got[r][0] for r in range(G)])
        return allrec.view(part.dtype), from_left, from_right

    def neighbour_views(self, k4: torch.Tensor, v4: torch.Tensor):
        """k4 [F, H, W_l, C] keys (channels-last), v4 [F, C, H, W_l] values (channel-major) of this band -> the same with one
        view of the left neighbour in front and one of the right neighbour behind (circular), i.e. n_local + 2 views.
        (Copies the whole band: the network uses `halo_views`; the tests pin `local_segments` with this form.)"""
        Wv = k4.shape[2] // self.n_local
        (kl, vl), (kr, vr) = self._exchange([k4[:, :, :Wv], v4[..., :Wv]], [k4[:, :, -Wv:], v4[..., -Wv:]])
        return torch.cat([kl, k4, kr], dim=2).contiguous(), torch.cat([vl, v4, vr], dim=3).contiguous()

    def halo_views(self, rt, k4: torch.Tensor, v4: torch.Tensor, k_rows: int, k_ld: int, k_col: int):
        """The neighbours' edge views WITHOUT touching the band.  k4 [F, H, W_l, C] (a strided view of
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
        return torch.cat(self._link.all_gather(x), dim=-1).to(x.device)
