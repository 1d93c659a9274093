"""CPU emulation of the split-operand attention entry points (include/panacea_hip.h: pnc_attn_views_split_f16,
pnc_attn_temporal_split_f16) for the emu backend of tests/emu.py.  tests/test_precise_wide.py attaches them to `emu` with
monkeypatch; tests/test_precise_wide_gpu.py holds the HIP kernels to the float64 form (`exact=True`) on the MI355X.

Default form: the kernels' arithmetic in fp32 — S = Qh.Kh + 2^-11 (Qh.Kl + Ql.Kh), fp32 softmax, P split into an fp16 pair,
O = Ph.Vh + 2^-11 (Ph.Vl + Pl.Vh) — written as hi + fp16 lo planes.  `exact=True`: float64 attention of the operand values
hi + lo * 2^-11 (no term dropped), returned instead of written."""
import torch

import emu

S = 1.0 / emu.LO_SCALE


def _rows_views(groups, H, W, views):
    """row index [groups, views, H * W / views] of every query (the resident layout: row = (g * H + y) * W + x)"""
    Wv = W // views
    g = torch.arange(groups).view(-1, 1, 1)
    v = torch.arange(views).view(1, -1, 1)
    i = torch.arange(H * Wv).view(1, 1, -1)
    return g * H * W + (i // Wv) * W + v * Wv + i % Wv


def _kv_rows(kg, u, kvW, kvWv, kv_rows, kv_valid):
    j = torch.arange(kv_valid)
    return kg * kv_rows + (j // kvWv) * kvW + u * kvWv + j % kvWv


def _attend(qh, ql, kh, kl, vh, vl, scale, exact):
    """[..., nq, 64] queries, [..., nk, 64] keys / values (hi, lo) -> [..., nq, 64] output (float64 when exact, else fp32)"""
    if exact:
        d = torch.float64
        q, k, v = (a.to(d) + b.to(d) * S for a, b in ((qh, ql), (kh, kl), (vh, vl)))
        return torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1) @ v
    f = torch.float32
    qh, ql, kh, kl, vh, vl = (t.to(f) for t in (qh, ql, kh, kl, vh, vl))
    s = qh @ kh.transpose(-1, -2) + (qh @ kl.transpose(-1, -2) + ql @ kh.transpose(-1, -2)) * S
    p = torch.softmax(s * scale, dim=-1)
    ph = p.half().float()
    pl = ((p - ph) * emu.LO_SCALE).half().float()
    return ph @ vh + (ph @ vl + pl @ vh) * S


def _write(o, o_lo, rows, ldo, Cc, val):
    """val [..., heads, nq, 64] at the query rows `rows` [..., nq]"""
    val = val.float()
    heads = val.shape[-3]
    flat = val.movedim(-3, -2).reshape(-1, heads * 64)          # [..., nq, heads*64]
    r = rows.reshape(-1)
    hi = emu.r16(flat, "attn_split")
    Om, Ol = emu._mat(o, int(r.max()) + 1, Cc, ldo), emu._mat(o_lo, int(r.max()) + 1, Cc, ldo)
    Om[r] = hi
    Ol[r] = emu._lo(flat, hi)


def attn_views_split(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, *, groups, heads, H, W, views, kvH, kvW, kv_views,
                     kv_rows_per_group, q_per_kv, kv_valid, segs, scale, exact=False):
    Cc = heads * 64
    kvWv = kvW // kv_views
    n_kvg = (groups + q_per_kv - 1) // q_per_kv
    qrows = _rows_views(groups, H, W, views)                            # [g, views, nq]
    nrows_q = groups * H * W
    nrows_kv = n_kvg * kv_rows_per_group

    def heads_of(t, ld, rows, n):
        return emu._mat(t, n, Cc, ld)[rows].view(*rows.shape, heads, 64).movedim(-2, -3)     # [..., heads, n, 64]
    out = []
    for vw in range(views):
        qr = qrows[:, vw]
        qh, ql = heads_of(q, ldq, qr, nrows_q), heads_of(q_lo, ldq, qr, nrows_q)
        kr = torch.stack([torch.cat([_kv_rows(g // q_per_kv, u, kvW, kvWv, kv_rows_per_group, kv_valid) for u in segs[vw]])
                          for g in range(groups)])                       # [g, nk]
        kh, kl = heads_of(k, ldk, kr, nrows_kv), heads_of(k_lo, ldk, kr, nrows_kv)
        vh, vl = heads_of(v, ldv, kr, nrows_kv), heads_of(v_lo, ldv, kr, nrows_kv)
        out.append(_attend(qh, ql, kh, kl, vh, vl, scale, exact))       # [g, heads, nq, 64]
    if exact:
        return torch.stack(out, 1), qrows                               # [g, views, heads, nq, 64], rows
    for vw in range(views):
        _write(o, o_lo, qrows[:, vw], ldo, Cc, out[vw])


def attn_temporal_split(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, *, B, T, Npix, heads, scale, exact=False):
    Cc = heads * 64
    M = B * T * Npix
    rows = (torch.arange(B).view(-1, 1, 1) * T * Npix + torch.arange(Npix).view(1, -1, 1)
            + torch.arange(T).view(1, 1, -1) * Npix)                     # [B, Npix, T]

    def g(t, ld):
        return emu._mat(t, M, Cc, ld)[rows].view(B, Npix, T, heads, 64).movedim(-2, -3)      # [B, Npix, heads, T, 64]
    val = _attend(g(q, ldq), g(q_lo, ldq), g(k, ldk), g(k_lo, ldk), g(v, ldv), g(v_lo, ldv), scale, exact)
    if exact:
        return val, rows
    _write(o, o_lo, rows, ldo, Cc, val)
