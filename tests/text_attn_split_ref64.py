"""Float64 reference, derived error bound and test operands of pnc_attn_text_split_f16, from the words of include/panacea_hip.h
section 6c alone.

Nothing here comes from tests/emu.py or from the kernel: every operand element is fetched from the FLAT storage of its buffer at the
address the header spells out, and only the named elements are touched — key and value rows >= kv_valid are never read.

    row of (prompt g, token i) of q / k / v / o, either plane      g*Lp + i, element c of head h at  buf[(g*Lp + i)*ld + 64h + c]
    the value of a pair                                            x = x_hi + 2^-11 x_lo
    query i attends key j                                          iff  j <= i  and  j < kv_valid
    reference                                                      o = softmax(scale * q k^T over the attended keys) v  on the VALUES

`value`, `split`, `embed`, `named_mask` and `excess` are those of tests/frame_attn_split_ref64.py (a prompt's rows are a frame's, the
tower's width 64*heads the frame's C).  `bound` is that file's bound applied per row to the row's attended keys, at C = 64, without
the per-tile rescale term: the header states a two-pass softmax (no running maximum, no rescale)."""
import torch

from frame_attn_ref64 import _flat
from frame_attn_split_ref64 import LO, U, case as frame_case, embed, excess, named_mask, split, value      # noqa: F401

D = 64                       # head dim
MUTATIONS = ("q_lo", "k_lo", "v_lo", "pl", "o_lo", "diag_plus", "diag_minus", "no_kv_valid")
# (Lp, kv_valid) of the tests: every edge of the 16-key and 16-query tiles, a one-key row, the product's shape, the largest accepted one
SHAPES = ((8, 1), (8, 8), (16, 9), (24, 17), (32, 31), (80, 77), (96, 96))


def gather(buf, ld, *, groups, heads, Lp, rows):
    """-> the named elements of the first `rows` token rows of every prompt, as float64 [groups, heads, rows, 64]"""
    r = (torch.arange(groups)[:, None] * Lp + torch.arange(rows)[None, :]).reshape(-1)
    idx = (r * ld)[:, None] + torch.arange(D * heads)[None, :]
    return _flat(buf)[idx].double().reshape(groups, rows, heads, D).permute(0, 2, 1, 3)


def attended(Lp, kv_valid, mutate=None):
    """bool [Lp, nk]: query i attends key j.  nk = kv_valid keys, or Lp under the mutation that ignores kv_valid."""
    nk = Lp if mutate == "no_kv_valid" else kv_valid
    i, j = torch.arange(Lp)[:, None], torch.arange(nk)[None, :]
    if mutate == "diag_plus":
        return j <= i + 1
    if mutate == "diag_minus":
        return j < i
    return j <= i


def applies(mutate, Lp, kv_valid):
    """whether the wrong kernel `mutate` computes another function than the right one at this shape.  With one valid key every row's
    softmax is the single probability 1 whatever the scores: q_lo, k_lo and Pl cannot matter, and no row has a key behind its diagonal
    to attend by mistake.  A kernel that ignores kv_valid is right when kv_valid = Lp.  v_lo, o_lo and the forgotten diagonal (row 0
    is left with no key) are wrong at every shape."""
    if mutate in ("q_lo", "k_lo", "pl", "diag_plus"):
        return kv_valid >= 2
    if mutate == "no_kv_valid":
        return kv_valid < Lp
    return True


def bound(Qh, Ql, Kh, Kl, Vh, Vl, scale, x, Pn, O, att):
    """|kernel's pair value - reference| a correct kernel may show, per element of one head of one prompt.  u = 2^-24.  The terms are
    those of frame_attn_split_ref64.bound (its docstring derives each one), per row over the row's attended keys `att`, n of them:

    1. scores, fp32 accumulation over C = 64 channels in any order, the hi.hi and the cross sums kept apart and met once:
           dS = 2 u ((C + 8) |Qh||Kh| + (2 C + 8) 2^-11 (|Qh||Kl| + |Ql||Kh|))
    2. the dropped lo.lo products:  2^-22 |Ql||Kl|.
    3. x = scale * S in the exp2 domain and the subtraction of the row's maximum:
           dx = scale (dS + lo.lo) + 4 u |x| + 2 u (|x| + max_j |x|)          (max over the attended keys)
    4. p = exp2(..) off by dx relatively + 4 u (v_exp_f32), carried as an fp16 pair (2^-22 p; half a subnormal step 2^-25 for a p below
       2^-14):  eps = dx + 4 u + 2^-22;  o moves by  sum_j Pn_j eps_j (|v_j| + |o|).
    5. the dropped Pl.Vl product:  2^-22 sum_j Pn_j |Vl_j|.
    6. fp32 accumulation over the n attended keys (any order; the masked keys of a visited tile add exact zeros) and 8 roundings for
       the meeting of the sums, the normalisation and its reciprocal; the row sum is n + 8 additions of positive terms.  TWO passes:
       no rescale of the accumulators, so the per-tile term of the frame kernel's bound is absent.
           2 u ((n + 8) Pn|Vh| + (2 n + 8) 2^-11 (Pn|Vl| + Pn|Vh|))  +  2 u (n + 8) |o|  +  6 u |o|
    7. second order: everything above times (1 + 4 max eps).
    8. the output pair against the computed value: + 2^-22 (|o| + b) + 2^-36."""
    C = Qh.shape[-1]
    n = att.sum(dim=-1, keepdim=True).double()
    aQh, aQl, aKh, aKl, aVh, aVl = (t.abs() for t in (Qh, Ql, Kh, Kl, Vh, Vl))
    dS = 2 * U * ((C + 8) * (aQh @ aKh.t()) + (2 * C + 8) * LO * (aQh @ aKl.t() + aQl @ aKh.t()))
    lolo = LO * LO * (aQl @ aKl.t())
    ax = torch.where(att, x.abs(), torch.zeros_like(x))
    dx = scale * (dS + lolo) + 4 * U * ax + 2 * U * (ax + ax.max(dim=-1, keepdim=True).values)
    eps = dx + 4 * U + 2.0 ** -22
    Vabs = aVh + LO * aVl
    Pe = Pn * eps                                                # Pn is 0 at the keys a row does not attend
    b = Pe @ Vabs + O.abs() * Pe.sum(dim=-1, keepdim=True)
    b = b + 2.0 ** -25 * (((Pn < 2.0 ** -14) & att).double() @ Vabs)
    b = b + LO * LO * (Pn @ aVl)
    b = b + 2 * U * ((n + 8) * (Pn @ aVh) + (2 * n + 8) * LO * (Pn @ aVl + Pn @ aVh))
    b = b + (2 * U * (n + 8) + 6 * U) * O.abs()
    b = b * (1.0 + 4.0 * eps[att].max().item())
    return b + 2.0 ** -22 * (O.abs() + b) + 2.0 ** -36


def attn_text_split(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, *, groups, heads, Lp, kv_valid, scale, mutate=None, with_bound=True):
    """-> (float64 [groups, Lp, 64*heads] reference of the pair value of o — the layout of o with ldo = 64*heads —, the bound of the same
    shape or None).  `mutate`: what one of the wrong kernels of MUTATIONS would deliver — no bound then.  (`no_kv_valid` reads the key
    and value rows behind kv_valid: only on buffers that hold numbers there.)"""
    assert mutate is None or mutate in MUTATIONS
    geo = dict(groups=groups, heads=heads, Lp=Lp)
    att = attended(Lp, kv_valid, mutate)
    nk = att.shape[1]
    Qh, Ql = gather(q, ldq, rows=Lp, **geo), gather(q_lo, ldq, rows=Lp, **geo)
    Kh, Kl = gather(k, ldk, rows=nk, **geo), gather(k_lo, ldk, rows=nk, **geo)
    Vh, Vl = gather(v, ldv, rows=nk, **geo), gather(v_lo, ldv, rows=nk, **geo)
    if mutate == "q_lo":
        Ql = torch.zeros_like(Ql)
    if mutate == "k_lo":
        Kl = torch.zeros_like(Kl)
    if mutate == "v_lo":
        Vl = torch.zeros_like(Vl)
    out = torch.empty((groups, heads, Lp, D), dtype=torch.float64)
    bnd = torch.empty_like(out) if with_bound and mutate is None else None
    some = att.any(dim=-1, keepdim=True)                         # (the forgotten diagonal leaves row 0 without a key: it delivers 0)
    for g in range(groups):
        for h in range(heads):
            x = ((Qh[g, h] + LO * Ql[g, h]) @ (Kh[g, h] + LO * Kl[g, h]).t()) * scale
            xm = torch.where(att, x, torch.full_like(x, -float("inf")))
            m = torch.where(some, xm.max(dim=-1, keepdim=True).values, torch.zeros_like(x[:, :1]))
            P = torch.where(att, torch.exp(x - m), torch.zeros_like(x))
            l = torch.where(some, P.sum(dim=-1, keepdim=True), torch.ones_like(m))
            Vv = Vh[g, h] + LO * Vl[g, h]
            o = ((P.float().half().double() if mutate == "pl" else P) @ Vv) / l
            if mutate == "o_lo":
                o = o.float().half().double()
            out[g, h] = o
            if bnd is not None:
                bnd[g, h] = bound(Qh[g, h], Ql[g, h], Kh[g, h], Kl[g, h], Vh[g, h], Vl[g, h], scale, x, P / l, o, att)
    fold = lambda t: t.permute(0, 2, 1, 3).reshape(groups, Lp, D * heads)      # noqa: E731
    return fold(out), None if bnd is None else fold(bnd)


def case(kind, *, groups, heads, Lp, seed=0):
    """-> (dict of the six [groups, Lp, 64*heads] fp16 planes q, q_lo, k, k_lo, v, v_lo, scale): the STRUCTURED operands of
    frame_attn_split_ref64.case at C = 64, one of its frames per (prompt, head) — every term a wrong kernel could lose adds up
    coherently over its contraction while the bound stays that of small scores (x0 = scale C a b = 1/8).  kind: "unit" or "zero_lo"."""
    planes, scale = frame_case(kind, F=groups * heads, N=Lp, C=D, seed=seed)
    fold = lambda t: t.reshape(groups, heads, Lp, D).permute(0, 2, 1, 3).reshape(groups, Lp, D * heads).contiguous()      # noqa: E731
    return {n: fold(t) for n, t in planes.items()}, scale


def qkv_buffer(planes, which):
    """the planes as column blocks of ONE [groups*Lp, 3W] buffer (what the QKV GEMM writes; ld = 3W) -> (flat buffer, the three flat views
    whose element 0 is the first element of q / k / v).  which: "" for the hi planes, "_lo" for the lo planes."""
    g, Lp, W = planes["q"].shape
    buf = torch.cat([planes[n + which].reshape(g * Lp, W) for n in ("q", "k", "v")], dim=1).contiguous().reshape(-1)
    return buf, (buf, buf[W:], buf[2 * W:])
