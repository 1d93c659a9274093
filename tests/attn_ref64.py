"""Float64 softmax attention for the geometries of include/panacea_hip.h, indexed from the header's words alone.

Nothing here comes from tests/emu.py: every operand element is fetched from the FLAT storage of its buffer at the address the header
spells out, one gather per (group, view, head), so a convention shared by the kernels and the emulation (strided views, reshapes of a
token grid) cannot hide in both.  Only the elements the contract names are touched: a buffer may hold NaN everywhere else.

    q row of (group g, y, x)        m = (g*H + y)*W + x, head h at columns h*64 .. h*64 + 63           q[m*ldq + h*64 + d]
    K row of (kv group kvg, ky, kx) r = kvg*kv_rows_per_group + ky*kvW + kx                            k[r*ldk + h*64 + d]
    V^T of the same key             token = ky*kvW + kx                     vt[kvg*vt_gstride + (h*64 + d)*ldvt + token]
    query view v of a group         columns v*W/views .. of the H x W grid, queries numbered row by row inside the view
    its keys                        the first kv_valid keys (numbered the same way) of each kv view seg[v][0 .. nseg[v]) of
                                    kv group g / q_per_kv, concatenated; causal: key j of a view only for j <= query index i
    temporal                        row of (b, t, pixel p) m = (b*T + t)*Npix + p; the T frames of one pixel attend each other

Operands are taken as they are (fp16, or float64 values of split operands); the result is float64.
"""
import torch


def _flat(t):
    return t.detach().cpu().reshape(-1)


def _softmax_pv(Q, K, V, scale, keep=None):
    S = (Q @ K.transpose(-1, -2)) * scale
    if keep is not None:
        S = S.masked_fill(~keep, float("-inf"))
    S = S - S.max(dim=-1, keepdim=True).values
    P = torch.exp(S)
    return (P / P.sum(dim=-1, keepdim=True)) @ V


def attn_views(q, ldq, k, ldk, vt, ldvt, vt_gstride, *, groups, heads, H, W, views, kvH, kvW, kv_views, kv_rows_per_group,
               q_per_kv, kv_valid, segs, scale, causal=False):
    """-> float64 [groups*H*W, heads*64], row m = (g*H + y)*W + x (the layout of o with ldo = heads*64)"""
    qf, kf, vf = _flat(q), _flat(k), _flat(vt)
    Wv, kvWv = W // views, kvW // kv_views
    assert Wv * views == W and kvWv * kv_views == kvW and 1 <= kv_valid <= kvH * kvWv
    d = torch.arange(64)
    qi = torch.arange(H * Wv)                                   # view-local query index
    kj = torch.arange(kv_valid)                                 # view-local key index
    out = torch.full((groups * H * W, heads * 64), float("nan"), dtype=torch.float64)
    for g in range(groups):
        kvg = g // q_per_kv
        for v in range(views):
            qrow = (g * H + qi // Wv) * W + v * Wv + qi % Wv
            tok = torch.cat([(kj // kvWv) * kvW + u * kvWv + kj % kvWv for u in segs[v]])
            krow = kvg * kv_rows_per_group + tok
            keep = None
            if causal:
                keep = kj.repeat(len(segs[v]))[None, :] <= qi[:, None]
            for h in range(heads):
                col = h * 64 + d
                Q = qf[qrow[:, None] * ldq + col[None, :]].double()
                K = kf[krow[:, None] * ldk + col[None, :]].double()
                V = vf[kvg * vt_gstride + col[None, :] * ldvt + tok[:, None]].double()
                out[qrow[:, None], col[None, :]] = _softmax_pv(Q, K, V, scale, keep)
    return out


def attn_temporal(q, ldq, k, ldk, v, ldv, *, B, T, Npix, heads, scale):
    """-> float64 [B*T*Npix, heads*64], row m = (b*T + t)*Npix + p"""
    qf, kf, vf = _flat(q), _flat(k), _flat(v)
    col = torch.arange(heads * 64).view(heads, 1, 64)
    t = torch.arange(T)
    out = torch.full((B * T * Npix, heads * 64), float("nan"), dtype=torch.float64)
    for b in range(B):
        for p in range(Npix):
            row = ((b * T + t) * Npix + p).view(1, T, 1)
            Q, K, V = (f[row * ld + col].double() for f, ld in ((qf, ldq), (kf, ldk), (vf, ldv)))      # [heads, T, 64]
            out[row, col] = _softmax_pv(Q, K, V, scale)
    return out
