"""Float64 reference, derived error bound and test operands of pnc_attn_frame_split_f16, from the words of include/panacea_hip.h
section 6b alone.

Nothing here comes from tests/emu.py or from the kernel: every operand element is fetched from the FLAT storage of its buffer at the
address the header spells out (helpers of tests/frame_attn_ref64.py), and only the named elements are touched.

    row of (frame f, token i) of q / k / v / o, either plane      f*N + i, element c < C at  buf[(f*N + i)*ld + c]
    the value of a pair                                            x = x_hi + 2^-11 x_lo
    reference                                                      o = softmax(scale * q k^T) v  on the VALUES, all products kept

`attn_frame_split` returns that reference and `bound`, the error a correct kernel may show against it (docstring of `bound`).  `mutate`
turns the reference into one of the wrong kernels the bound has to catch (tests/test_frame_attn_split.py).  `case` builds the operands
of the tests: structured so that every plane of every operand moves the result by more than the bound allows."""
import torch

from frame_attn_ref64 import _flat

U = 2.0 ** -24               # unit roundoff of fp32
LO = 2.0 ** -11              # weight of a lo plane
MUTATIONS = ("q_lo", "k_lo", "v_lo", "pl", "o_lo")


def gather(buf, ld, *, F, N, C):
    """-> the named elements of a plane as float64 [F, N, C]"""
    idx = (torch.arange(F * N) * ld)[:, None] + torch.arange(C)[None, :]
    return _flat(buf)[idx].double().reshape(F, N, C)


def value(hi, lo):
    """the float64 value of an fp16 pair"""
    return hi.double() + LO * lo.double()


def split(x):
    """float64 / float32 values -> (hi, lo) fp16 planes as the library splits them (fp32 arithmetic)"""
    x = x.float()
    hi = x.half()
    return hi, ((x - hi.float()) * 2048.0).half()


def bound(Qh, Ql, Kh, Kl, Vh, Vl, scale, x, Pn, O):
    """|kernel's pair value - reference| a correct kernel may show, per element of one frame.  u = 2^-24.  Nothing is fitted to a kernel.

    1. scores, fp32 accumulation over C.  fp16 x fp16 products are exact in fp32 and the 2^-11 weights exact scalings; a sum of n fp32
       terms in ANY order is off by at most 2 n u sum|terms| (the form of tests/gemm_ref64.py: it covers the MFMA's internal order, the
       meeting of the four channel slices and a truncating adder).  The hi.hi products are C terms, the two cross products 2 C terms
       2^-11 times smaller, plus 8 additions for the slices and the meeting of the two sums:
           dS = 2 u ((C + 8) |Qh||Kh| + (2 C + 8) 2^-11 (|Qh||Kl| + |Ql||Kh|))
    2. the dropped lo.lo products, from the planes themselves:  2^-22 |Ql||Kl|.
    3. x = scale * S in the exp2 domain and the subtraction of the running maximum m (any m up to the row's maximum; a shift of
       the whole row cancels, only its roundings stay): two rounded products 4 u |x|, the difference u (|x| + max_j |x|), doubled.
           dx = scale (dS + lo.lo) + 4 u |x| + 2 u (|x| + max_j |x|)
    4. a probability p = exp2(..) is off by dx relatively (first order) + 4 u for v_exp_f32 (1 ulp) and is then carried as an fp16
       pair: hi within 2^-11 p, the residual exact in fp32, its fp16 rounding 2^-11 of it -> 2^-22 p; a p below fp16's normal range
       (< 2^-14 of the row's scale, whose sum is >= 1) is off by up to half a subnormal step 2^-25 instead.
           eps = dx + 4 u + 2^-22
       o = sum_j p_j v_j / sum_j p_j moves by  sum_j Pn_j eps_j (|v_j| + |o|)  to first order (Pn the normalised probabilities).
    5. the dropped Pl.Vl product:  2^-22 sum_j Pn_j |Vl_j|    (|Pl| <= p).
    6. fp32 accumulation over N: N products of Ph.Vh, 2 N cross products 2^-11 times smaller, one rounding per rescale (at most one per
       32-key tile) and 8 for the meeting of the sums, the normalisation and its reciprocal; the row sum is N + 8 additions of
       positive terms, a relative error of the whole row:
           2 u ((N + N / 32 + 8) Pn|Vh| + (2 N + N / 32 + 8) 2^-11 (Pn|Vl| + Pn|Vh|))  +  2 u (N + 8) |o|  +  6 u |o|
    7. second order: everything above times (1 + 4 max eps).
    8. the output pair against the computed value: + 2^-22 (|o| + b) + 2^-36   (tests/gemm_ref64.py, out16 + out16_lo)."""
    C, N = Qh.shape[-1], Kh.shape[0]
    aQh, aQl, aKh, aKl, aVh, aVl = (t.abs() for t in (Qh, Ql, Kh, Kl, Vh, Vl))
    dS = 2 * U * ((C + 8) * (aQh @ aKh.t()) + (2 * C + 8) * LO * (aQh @ aKl.t() + aQl @ aKh.t()))
    lolo = LO * LO * (aQl @ aKl.t())
    ax = x.abs()
    dx = scale * (dS + lolo) + 4 * U * ax + 2 * U * (ax + ax.max(dim=-1, keepdim=True).values)
    eps = dx + 4 * U + 2.0 ** -22
    Vabs = aVh + LO * aVl
    Pe = Pn * eps
    b = Pe @ Vabs + O.abs() * Pe.sum(dim=-1, keepdim=True)
    b = b + 2.0 ** -25 * ((Pn < 2.0 ** -14).double() @ Vabs)
    b = b + LO * LO * (Pn @ aVl)
    nt = N / 32.0
    b = b + 2 * U * ((N + nt + 8) * (Pn @ aVh) + (2 * N + nt + 8) * LO * (Pn @ aVl + Pn @ aVh))
    b = b + (2 * U * (N + 8) + 6 * U) * O.abs()
    b = b * (1.0 + 4.0 * eps.max().item())
    return b + 2.0 ** -22 * (O.abs() + b) + 2.0 ** -36


def attn_frame_split(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, *, F, N, C, scale, mutate=None, with_bound=True):
    """-> (float64 [F, N, C] reference of the pair value of o, the bound of the same shape or None).  `mutate`: what a kernel would
    deliver that ignores q_lo / k_lo / v_lo, drops Pl (P carried as a single fp16), or writes o_lo as zero — no bound then."""
    assert mutate is None or mutate in MUTATIONS
    geo = dict(F=F, N=N, C=C)
    Qh, Ql = gather(q, ldq, **geo), gather(q_lo, ldq, **geo)
    Kh, Kl = gather(k, ldk, **geo), gather(k_lo, ldk, **geo)
    Vh, Vl = gather(v, ldv, **geo), gather(v_lo, ldv, **geo)
    if mutate == "q_lo":
        Ql = torch.zeros_like(Ql)
    if mutate == "k_lo":
        Kl = torch.zeros_like(Kl)
    if mutate == "v_lo":
        Vl = torch.zeros_like(Vl)
    out = torch.empty((F, N, C), dtype=torch.float64)
    bnd = torch.empty((F, N, C), dtype=torch.float64) if with_bound and mutate is None else None
    for f in range(F):
        x = ((Qh[f] + LO * Ql[f]) @ (Kh[f] + LO * Kl[f]).t()) * scale
        P = torch.exp(x - x.max(dim=-1, keepdim=True).values)
        l = P.sum(dim=-1, keepdim=True)
        Vv = Vh[f] + LO * Vl[f]
        if mutate == "pl":
            out[f] = (P.float().half().double() @ Vv) / l
        else:
            out[f] = (P / l) @ Vv
        if mutate == "o_lo":
            out[f] = out[f].float().half().double()
        if bnd is not None:
            bnd[f] = bound(Qh[f], Ql[f], Kh[f], Kl[f], Vh[f], Vl[f], scale, x, P / l, out[f])
    return out, bnd


def embed(plane, ld, fill=float("nan")):
    """[F, N, C] fp16 -> a flat buffer whose named elements are `plane` with leading dimension ld; everything else holds `fill`, and
    the buffer ENDS right behind the last named element"""
    F, N, C = plane.shape
    buf = torch.full(((F * N - 1) * ld + C,), fill, dtype=torch.float16)
    idx = (torch.arange(F * N) * ld)[:, None] + torch.arange(C)[None, :]
    buf[idx.reshape(-1)] = plane.reshape(-1)
    return buf


def named_mask(ld, *, F, N, C):
    """bool mask over embed()'s buffer: True at the named elements"""
    m = torch.zeros(((F * N - 1) * ld + C,), dtype=torch.bool)
    m[((torch.arange(F * N) * ld)[:, None] + torch.arange(C)[None, :]).reshape(-1)] = True
    return m


def excess(got, ref, bnd):
    """-> (max |got - ref|, max over elements of |got - ref| - bound): the second is <= 0 inside the bound"""
    err = (got.double() - ref).abs()
    return err.max().item(), (err - bnd).max().item()


def case(kind, *, F, N, C, seed=0):
    """-> (dict of the six [F, N, C] fp16 planes q, q_lo, k, k_lo, v, v_lo, scale).

    A worst-case fp32 bound over C = 512 channels is wider than what a lo plane of random data moves, so the operands are STRUCTURED:
    every term a wrong kernel could lose adds up coherently over its contraction while the bound stays that of small scores.
      t_c, e_c = +-1 per channel; h_i = +-1 per query, g_j, g'_j = +-1 per key in two different patterns
      Qh = h_i t_c a,  Ql = 0.9 t_c a,  Kh = g_j t_c b,  Kl = 0.9 g'_j t_c b   (a = b = 1/8, powers of two: the residual of a value just
          off a power of two reaches |hi| itself)
          -> scale * S = x0 (h_i g_j + 2^-11 0.9 (g_j + h_i g'_j)):  q_lo moves the keys of g_j = +1 against the others, k_lo those of g'_j
      Vh = g_j w1_c + g'_j w2_c + v0_c,  Vl = 0.45 e_c |Vh|:  w1 / w2 carry the two shifts into o, v_lo adds up over the keys; a quarter
          of the channels holds v0 = 1 instead, an o of about 1 whose fp16 residual (o_lo) is far above the bound
      x0 = scale C a b = sqrt(C) / 64 (0.18 / 0.25 / 0.35): the probabilities of a row take two values, 1 and exp(-2 x0), the second
          with one fp16 residual for all its keys — Pl adds up over them.
    The lo planes and V carry a few percent of noise.  kind: "unit" (scale = C^-0.5), "spike" (one key late in the last tile with 64
    times the magnitude: rows with h_i g_j = +1 see their maximum rise by 64 x0 log2(e) > 16 in the last tile — the deferred rescale
    must run — the others see a vanishing probability), "large" (|q| = |k| = 256, lo planes up to 230, scale = C^-0.5 2^-22 for the
    same x0), "zero_lo" ("unit" with all lo planes 0)."""
    assert kind in ("unit", "spike", "large", "zero_lo")
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * C + 31 * N + F)

    def sign(*shape):
        return (torch.randint(0, 2, shape, generator=g) * 2 - 1).double()

    def noise(*shape, amp=0.03):
        return 1.0 + amp * (2.0 * torch.rand(*shape, generator=g, dtype=torch.float64) - 1.0)

    i = torch.arange(N)
    t_c, e_c = sign(C), sign(C)
    h_i = (1 - 2 * (i % 2)).double()
    g_j = (1 - 2 * ((i // 1 + i // 2) % 2)).double()           # + - - + + - - + ...
    g2_j = (1 - 2 * ((i // 2 + i // 4) % 2)).double()          # + + - - - - + + ...
    a = b = 256.0 if kind == "large" else 2.0 ** -3
    scale = float(C) ** -0.5 * (2.0 ** -22 if kind == "large" else 1.0)      # x0 = scale C a b = sqrt(C) / 64: 0.18, 0.25, 0.35
    chan = torch.arange(C)
    w1 = torch.where(chan % 4 == 1, 1.0, 0.0).double() + torch.where(chan % 4 == 3, 0.5, 0.0).double()
    w2 = torch.where(chan % 4 == 2, 1.0, 0.0).double() + torch.where(chan % 4 == 3, 0.5, 0.0).double()
    v0 = torch.where(chan % 4 == 0, 1.0, 0.0).double()
    out = {}
    planes = {n: [] for n in ("q", "q_lo", "k", "k_lo", "v", "v_lo")}
    for f in range(F):
        Qh = (h_i[:, None] * t_c[None, :] * a).expand(N, C)
        Ql = 0.9 * a * t_c[None, :] * noise(N, C)
        kb = torch.full((N, C), b, dtype=torch.float64)
        if kind == "spike":
            kb[N - 3] = kb[N - 3] * 64.0
        Kh = g_j[:, None] * t_c[None, :] * kb
        Kl = 0.9 * g2_j[:, None] * t_c[None, :] * kb * noise(N, C)
        Vh = (g_j[:, None] * w1[None, :] + g2_j[:, None] * w2[None, :] + v0[None, :]) * noise(N, C)
        Vl = 0.45 * e_c[None, :] * Vh.half().double().abs() * noise(N, C)
        for n, t in (("q", Qh), ("q_lo", Ql), ("k", Kh), ("k_lo", Kl), ("v", Vh), ("v_lo", Vl)):
            planes[n].append(t.float().half())
    out = {n: torch.stack(ts) for n, ts in planes.items()}
    if kind == "zero_lo":
        for n in ("q_lo", "k_lo", "v_lo"):
            out[n] = torch.zeros_like(out[n])
    assert all(torch.isfinite(t.float()).all() for t in out.values())
    return out, scale
