"""Operand builders of the attention edge cases (tests/test_attn_edges_gpu.py on the MI355X, tests/test_attn_ref64.py on the CPU).

Every builder returns CPU fp16 buffers that are LARGER than the launch may read, the excess filled with NaN, and the keyword
geometry of hip.attn_views / emu.attn_views / attn_ref64.attn_views.  `pad` names what the keys kv_valid .. Nkv - 1 of a view hold —
the region PncAttnParams.kv_valid says is read, must be finite and must not matter: "zero" or "garbage" (finite values of
alternating sign up to +-60000).  Bounds: the project's own (tests/test_kernels_gpu.py)."""
import torch

NAN = float("nan")
UNIT = (3e-3, 2e-3)          # atol, rtol of test_attn_views_self / test_attn_temporal: unit-scale data
SHARP = (5e-3, 2e-3)         # test_attn_views_sharp_softmax
EXCESS = 8                   # NaN rows behind q / o / K, and 8 * 8 NaN elements behind V^T
INTRA = [[0], [1], [2], [3], [4], [5]]
CROSS = [[5, 1], [0, 2], [1, 3], [2, 4], [3, 5], [4]]


def rnd16(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).half()


def garbage(n):
    """n finite fp16 values of alternating sign, magnitudes spread over 1 .. 60000"""
    i = torch.arange(n, dtype=torch.int64)
    mag = (i * 7919) % 60000 + 1
    return (mag * (1 - 2 * (i % 2))).double().half()


def _fill(dst, mask, pad):
    """dst[mask] = zeros or garbage"""
    n = int(mask.sum())
    dst[mask] = garbage(n) if pad == "garbage" else torch.zeros(n, dtype=torch.float16)


def nan_tail(body, rows):
    """[body rows | `rows` rows of NaN] as one allocation; -> (whole, view of the body)"""
    whole = torch.full((body.shape[0] + rows,) + tuple(body.shape[1:]), NAN, dtype=torch.float16)
    whole[: body.shape[0]] = body
    return whole


def text_case(B, T, H, W, heads, rows, kv_valid, *, pad="zero", sharp=1.0, seed=0):
    """Cross-attention against few keys shared by the T frames of a sample: G = B * T groups of H x W queries, B kv groups of `rows`
    key rows (kvH = 1, kvW = rows), ldvt = rows rounded up to a multiple of 8, kv_rows_per_group = ldvt.  K rows rows .. ldvt - 1 of
    every group and V^T columns rows .. ldvt - 1 lie BEHIND the key buffer: NaN.  -> (buffers, geometry)"""
    C, G, N = heads * 64, B * T, H * W
    ldvt = (rows + 7) // 8 * 8
    q = rnd16(G * N, C, seed=seed + 3) * sharp
    k = torch.full((B, ldvt, C), NAN, dtype=torch.float16)
    vt = torch.full((B, C, ldvt), NAN, dtype=torch.float16)
    k[:, :kv_valid] = rnd16(B, kv_valid, C, seed=seed + 4)
    vt[:, :, :kv_valid] = rnd16(B, C, kv_valid, seed=seed + 6)
    padk = torch.zeros(B, ldvt, C, dtype=torch.bool)
    padk[:, kv_valid:rows] = True
    padv = torch.zeros(B, C, ldvt, dtype=torch.bool)
    padv[:, :, kv_valid:rows] = True
    _fill(k, padk, pad)
    _fill(vt, padv, pad)
    buf = dict(q=nan_tail(q, EXCESS), k=nan_tail(k.view(B * ldvt, C), EXCESS), vt=nan_tail(vt.view(-1, 8), EXCESS), M=G * N, C=C)
    geo = dict(groups=G, heads=heads, H=H, W=W, views=1, kvH=1, kvW=rows, kv_views=1, kv_rows_per_group=ldvt, q_per_kv=T,
               kv_valid=kv_valid, segs=[[0]], scale=0.125)
    lds = dict(ldq=C, ldk=C, ldvt=ldvt, vt_gstride=C * ldvt, ldo=C)
    return buf, lds, geo


def causal_case(G, L, Lp, heads, *, pad="zero", seed=50):
    """The text tower's launch: a prompt = a group of one view with Lp rows, L valid keys, causal; q and k are column blocks of one
    [G * Lp, 2 C] projection buffer.  Padding = the K columns of rows L .. Lp - 1 and V^T columns L .. Lp - 1."""
    C = heads * 64
    qk = rnd16(G, Lp, 2 * C, seed=seed + 1)
    vt = rnd16(G, C, Lp, seed=seed + 2)
    padk = torch.zeros(G, Lp, 2 * C, dtype=torch.bool)
    padk[:, L:, C:] = True
    padv = torch.zeros(G, C, Lp, dtype=torch.bool)
    padv[:, :, L:] = True
    _fill(qk, padk, pad)
    _fill(vt, padv, pad)
    buf = dict(qk=nan_tail(qk.view(G * Lp, 2 * C), EXCESS), vt=nan_tail(vt.view(-1, 8), EXCESS), M=G * Lp, C=C)
    geo = dict(groups=G, heads=heads, H=1, W=Lp, views=1, kvH=1, kvW=Lp, kv_views=1, kv_rows_per_group=Lp, q_per_kv=1, kv_valid=L,
               segs=[[0]], scale=0.125, causal=True)
    lds = dict(ldq=2 * C, ldk=2 * C, ldvt=Lp, vt_gstride=C * Lp, ldo=C)
    return buf, lds, geo


def cross_case(G, H, Wv, heads, kv_valid, *, pad="zero", seed=70):
    """Cross-view attention, six views of H rows x Wv columns, two key segments per view (one for view 5), self-attention geometry;
    only the first kv_valid keys of a view (numbered row by row inside the view) exist: the others are the padding."""
    C, W = heads * 64, 6 * Wv
    N = H * W
    q = rnd16(G * N, C, seed=seed + 1)
    k = rnd16(G, H, W, C, seed=seed + 2)
    vt = rnd16(G, C, H, W, seed=seed + 3)
    y, x = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    padded = (y * Wv + x % Wv) >= kv_valid                       # [H, W]
    _fill(k, padded.view(1, H, W, 1).expand(G, H, W, C), pad)
    _fill(vt, padded.view(1, 1, H, W).expand(G, C, H, W), pad)
    buf = dict(q=nan_tail(q, EXCESS), k=nan_tail(k.view(G * N, C), EXCESS), vt=nan_tail(vt.view(-1, 8), EXCESS), M=G * N, C=C)
    geo = dict(groups=G, heads=heads, H=H, W=W, views=6, kvH=H, kvW=W, kv_views=6, kv_rows_per_group=N, q_per_kv=1,
               kv_valid=kv_valid, segs=CROSS, scale=0.125)
    lds = dict(ldq=C, ldk=C, ldvt=N, vt_gstride=C * N, ldo=C)
    return buf, lds, geo


def operands(buf, lds):
    """-> the nine positional arguments in front of `o` of hip.attn_views / attn_ref64.attn_views: q, ldq, k, ldk, vt, ldvt, vt_gstride"""
    if "qk" in buf:
        qk = buf["qk"]
        return qk, lds["ldq"], qk.reshape(-1)[buf["C"]:], lds["ldk"], buf["vt"], lds["ldvt"], lds["vt_gstride"]
    return buf["q"], lds["ldq"], buf["k"], lds["ldk"], buf["vt"], lds["ldvt"], lds["vt_gstride"]


def excess_error(got, ref, bound):
    """-> (max |got - ref|, max over elements of |got - ref| - (atol + rtol |ref|)): the second is <= 0 inside the bound"""
    atol, rtol = bound
    err = (got.double() - ref).abs()
    return err.max().item(), (err - (atol + rtol * ref.abs())).max().item()
