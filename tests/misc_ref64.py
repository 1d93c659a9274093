"""Float64 references of sections 4 and 5 of include/panacea_hip.h — the small-M linears, the timestep embeddings, the layout helpers,
the elementwise passes and pnc_softmax_rows_f16 — indexed from the flat storage of the buffers a launch reads by the formulae of the
header.  Independent of tests/emu.py: tests/test_misc_ref64.py holds the emulation to these, tests/test_misc_edges_gpu.py the kernels.

Every function takes the CPU tensors of a launch (views inside the poisoned allocations of tests/misc_edge_cases.py; only the
elements the header names are ever gathered, so the poison never enters) and returns {output name: Expect}.  An Expect names the
flat indices a launch WRITES in that output, the float64 value of each, and either
    exact   the tensor of the output's dtype the launch has to reproduce bit for bit (fp32 sums, layout moves, the fp16 hi plane of
            a cast, lo planes: the formats define these results, there is nothing to allow), or
    floor + allow   what a correct kernel may be off by: `floor` is the output FORMAT's share (half an fp16 step), `allow` the
            arithmetic's.  A kernel is held to floor + allow, the emulation to floor + allow / 2.
Where floor + allow is 0 and the value is 0 (a masked probability, the zero column of an odd embedding) the output is +0, bits too.

Nothing below was fitted to an output of the code under test: every allowance is derived next to its function.  u = 2^-24, the unit
roundoff of fp32 (half an ulp, relative); "one ulp" of an approximate instruction is 2 u relative."""
import math

import torch

U = 2.0 ** -24
L_SILU = 1.1                      # max |d/dx x sigmoid(x)| = 1.0998
LOG2E = 1.44269504088896340736


class Expect:
    def __init__(self, idx, v, exact=None, floor=None, allow=None):
        self.idx, self.v, self.exact, self.floor, self.allow = idx, v, exact, floor, allow

    def bound(self, share=1.0):
        return self.floor + share * self.allow


def _flat64(t):
    return t.reshape(-1).double()


def _f32(x):
    """a Python number as the fp32 value a C `float` argument carries"""
    return float(torch.tensor(x, dtype=torch.float64).float())


def silu(x):
    return x * torch.sigmoid(x)


def silu_err(x):
    """|silu_f(x) - x sigmoid(x)| of the kernels' silu_f(v) = v * rcp(1 + __expf(-v)) (csrc/common.h), per evaluation:
        (8 + 2 |x|) u |x sigmoid(x)|
    __expf(-v) is exp2(-v * log2 e): the rounded product moves the exponent by |v| log2(e) u, i.e. the power by |v| u relatively, and
    the rounded constant log2 e does so once more: 2 |x| u.  v_exp_f32 and v_rcp_f32 are one-ulp instructions (AMD's CDNA ISA
    guides state 1 ULP for both): 2 u each; the addition 1 + e: u; the relative error of e reaches the quotient 1 / (1 + e) times
    e / (1 + e) < 1.  That is (5 + 2 |x|) u on the sigmoid — an ABSOLUTE error of |x| (5 + 2 |x|) u sigmoid(x) on the product, which is
    (5 + 2 |x|) u |f| — plus one fp32 ulp (2 u) for the final product, plus u for the conversion of the result's operand: 8 u.  The
    same figure as gemm_ref64.bound uses for the GEMM epilogue's SiLU."""
    return (8.0 + 2.0 * x.abs()) * U * silu(x).abs()


# ------------------------------------------------------------------------------------------------------------------ small-M linears
def _linear(a32, lda, w16, w_lo, bias, M, N, K, silu_in, silu_out):
    """-> (v, allow) float64 [M, N] of out[m][n] = sum_k f(a[m * lda + k]) w[n * K + k] + bias[n], w = W + 2^-11 W_lo joined in float64.

    allow, with mag = sum_k |f(a)| |w|:
      gamma_K mag            K fp32 FMAs and the additions of the wave reduction, in ANY order: every product passes through at most
                             K roundings, gamma_K = K u / (1 - K u) (Higham, Accuracy and Stability, section 3.1)
      + u mag                with W_lo: the fp32 join fmaf(W_lo, 2^-11, W) rounds a weight that needs up to 22 bits
      + sum_k |w| silu_err(a)   with silu_in: every f(a) is off by silu_err
      + u (mag + |bias|)     the bias addition (none for a NULL bias: + 0.0f is exact)
    and with silu_out, pre = the value above:  L_SILU allow + silu_err(pre)  (Lipschitz, then the evaluation itself)."""
    m, k = torch.arange(M).view(M, 1), torch.arange(K).view(1, K)
    n = torch.arange(N).view(N, 1)
    A = _flat64(a32)[m * lda + k]
    W = _flat64(w16)[n * K + k]
    if w_lo is not None:
        W = W + _flat64(w_lo)[n * K + k] * 2.0 ** -11
    fa = silu(A) if silu_in else A
    v = fa @ W.t()
    mag = fa.abs() @ W.abs().t()
    allow = K * U / (1.0 - K * U) * mag
    if w_lo is not None:
        allow = allow + U * mag
    if silu_in:
        allow = allow + silu_err(A) @ W.abs().t()
    if bias is not None:
        b = _flat64(bias)[:N].view(1, N)
        v = v + b
        allow = allow + U * (mag + b.abs())
    if silu_out:
        allow = L_SILU * allow + silu_err(v)
        v = silu(v)
    return v, allow


def linear_smallm(a32, lda, w16, bias, ldo, M, N, K, silu_in=False, silu_out=False, w_lo=None):
    """pnc_linear_smallm / pnc_linear_smallm_split: out[m * ldo + n]"""
    v, allow = _linear(a32, lda, w16, w_lo, bias, M, N, K, silu_in, silu_out)
    idx = torch.arange(M).view(M, 1) * ldo + torch.arange(N).view(1, N)
    return {"out32": Expect(idx, v, floor=torch.zeros_like(v), allow=allow)}


def linear_smallm_segments(a32, lda, w16, bias, M, m0, Mtot, N, K, seg_start, silu_in=False, silu_out=False, w_lo=None):
    """pnc_linear_smallm_segments[_split]: out[seg_start[s] * Mtot + (m0 + m) * width_s + (n - seg_start[s])]"""
    v, allow = _linear(a32, lda, w16, w_lo, bias, M, N, K, silu_in, silu_out)
    idx = torch.empty(M, N, dtype=torch.int64)
    m = torch.arange(M).view(M, 1)
    for s0, s1 in zip(seg_start[:-1], seg_start[1:]):
        idx[:, s0:s1] = s0 * Mtot + (m0 + m) * (s1 - s0) + torch.arange(s1 - s0).view(1, -1)
    return {"out32": Expect(idx, v, floor=torch.zeros_like(v), allow=allow)}


# ---------------------------------------------------------------------------------------------------------------------- embeddings
EMB_ULPS = 4


def timestep_embedding(t, F, dim, freqs):
    """pnc_timestep_embedding (int64 t) / pnc_timestep_embedding_f32 (fp32 t): out[f * dim + j] = cos(arg), out[f * dim + dim / 2 + j] =
    sin(arg), arg = float32(float32(t[f]) * freqs[j]) — the reference project's fp32 product — with cos and sin of that fp32 argument in
    float64; the last column of an odd dim is 0.

    allow = EMB_ULPS 2^-24 = 2^-22, absolute.  The argument is exact (one fp32 product, reproduced here), so only cosf / sinf err.
    The device functions are OCML's, which implements the accuracy table of the OpenCL specification (7.4, relative error as ULP):
    sin and cos <= 4 ulp over the whole range, large arguments included.  |cos|, |sin| <= 1, where an fp32 ulp is at most 2^-24."""
    half = dim // 2
    tf = t.reshape(-1)[:F].float().double()                       # int64 -> fp32: round to nearest even, as the kernel's (float)t
    arg = (tf.view(F, 1) * _flat64(freqs)[:half].view(1, half)).float().double()     # the fp64 product of two fp32 is exact: ONE rounding
    v = torch.zeros(F, dim, dtype=torch.float64)
    v[:, :half], v[:, half:2 * half] = torch.cos(arg), torch.sin(arg)
    allow = torch.full_like(v, EMB_ULPS * U)
    allow[:, 2 * half:] = 0.0
    idx = torch.arange(F).view(F, 1) * dim + torch.arange(dim).view(1, dim)
    return {"out32": Expect(idx, v, floor=torch.zeros_like(v), allow=allow)}


# -------------------------------------------------------------------------------------------------------------------------- layout
def lo_f16(v32, hi):
    """the fp16 lo plane fp16((v - hi) * 2048): v - hi and the scaling are exact in fp32 (and in float64), ONE rounding"""
    return ((v32.double() - hi.double()) * 2048.0).half()


def lo_e4m3(v32, hi):
    """-> (the e4m3 bytes of the residual clamped to +-448, the mask of elements whose residual clamped)"""
    r = ((v32.double() - hi.double()) * 2048.0).float()            # exact
    return r.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8), r.abs() > 448.0


def clamped_quads(over):
    """what the range monitor counts: aligned groups of four consecutive elements of which at least one clamped"""
    return int(over.reshape(-1, 4).any(dim=1).sum())


def _lo_expect(idx, v32, hi, lo):
    """the Expect of a lo plane in format `lo` ("f16" / "e4m3") + the clamped-quad count (0 for fp16)"""
    if lo == "f16":
        return Expect(idx, v32.double(), exact=lo_f16(v32, hi)), 0
    q, over = lo_e4m3(v32, hi)
    return Expect(idx, v32.double(), exact=q), clamped_quads(over)


def nchw_to_tokens_f16(a32, C1, a_scale, a_frames, b32, C2, F, Npix, Cpad, with_lo):
    """pnc_nchw_to_tokens_f16: out[(f * Npix + p) * Cpad + c] = c < C1 ? a[((f % a_frames) * C1 + c) * Npix + p] * a_scale[f]
    : c < C1 + C2 ? b[(f * C2 + c - C1) * Npix + p] : 0.  The value is the fp32 product (the header defines it so): formed in
    float64, where it is exact, and rounded once.  hi = fp16(v), lo = fp16((v - hi) * 2048): both exact."""
    f, p = torch.arange(F).view(F, 1, 1), torch.arange(Npix).view(1, Npix, 1)
    v = torch.zeros(F, Npix, Cpad, dtype=torch.float64)
    c = torch.arange(C1).view(1, 1, C1)
    av = _flat64(a32)[((f % a_frames) * C1 + c) * Npix + p]
    if a_scale is not None:
        av = av * _flat64(a_scale)[:F].view(F, 1, 1)
    v[:, :, :C1] = av
    if C2:
        c = torch.arange(C2).view(1, 1, C2)
        v[:, :, C1:C1 + C2] = _flat64(b32)[(f * C2 + c) * Npix + p]
    v32 = v.float()
    hi = v32.half()
    idx = ((f * Npix + p) * Cpad + torch.arange(Cpad).view(1, 1, Cpad))
    out = {"out16": Expect(idx, v32.double(), exact=hi)}
    if with_lo:
        out["out16_lo"] = Expect(idx, v32.double(), exact=lo_f16(v32, hi))
    return out


def tokens_to_nchw_f32(x32, ld, F, Npix, C):
    """pnc_tokens_to_nchw_f32: out[(f * C + c) * Npix + p] = x[(f * Npix + p) * ld + c], a move: exact"""
    f, c, p = torch.arange(F).view(F, 1, 1), torch.arange(C).view(1, C, 1), torch.arange(Npix).view(1, 1, Npix)
    v = x32.reshape(-1)[(f * Npix + p) * ld + c]
    return {"out32": Expect((f * C + c) * Npix + p, v.double(), exact=v.clone())}


# --------------------------------------------------------------------------------------------------------------------- elementwise
def _sum32(x, a):
    """the fp32 sum of two fp32 tensors: their float64 sum is exact unless the exponents lie more than 29 binades apart, where the small
    addend is far below half an fp32 ulp of the large one and no tie is near — rounding it to fp32 is the correctly rounded sum"""
    return (x.double() + a.double()).float()


def _cast_expects(v32, want32, want16, lo):
    """outputs of a pass that writes the fp32 value, its fp16 cast and a lo plane at the same flat indices -> ({name: Expect}, clamped)"""
    idx = torch.arange(v32.numel()).view(v32.shape)
    out, clamped = {}, 0
    if want32:
        out["out32"] = Expect(idx, v32.double(), exact=v32)
    if want16:
        hi = v32.half()
        out["out16"] = Expect(idx, v32.double(), exact=hi)
        if lo is not None:
            out["out16_lo"], clamped = _lo_expect(idx, v32, hi, lo)
    return out, clamped


def concat_add(a32, C1, s32, c32, C2, M, want32=True, want16=True, lo=None):
    """pnc_concat_add: out[m * (C1 + C2) + ch] = ch < C1 ? a[m * C1 + ch] : s[m * C2 + ch - C1] + c[m * C2 + ch - C1] (c NULL: s alone)
    -> ({name: Expect}, clamped quads of an e4m3 lo plane)"""
    a = a32.reshape(-1)[: M * C1].view(M, C1)
    s = s32.reshape(-1)[: M * C2].view(M, C2)
    if c32 is not None:
        s = _sum32(s, c32.reshape(-1)[: M * C2].view(M, C2))
    return _cast_expects(torch.cat([a, s], dim=1).contiguous(), want32, want16, lo)


def add_f32(x32, a32, n, want32=True, want16=True, lo=None):
    """pnc_add_f32 (a32 None + want32 False: pnc_cast_f16): y[i] = x[i] + a[i] -> ({name: Expect}, clamped quads)"""
    x = x32.reshape(-1)[:n]
    return _cast_expects(x.clone() if a32 is None else _sum32(x, a32.reshape(-1)[:n]), want32, want16, lo)


# ------------------------------------------------------------------------------------------------------------------------- softmax
def floor_f16(p):
    """half an fp16 step at p (the subnormal spacing 2^-24 below 2^-14: 2^-25): never more than 2^-11 p in the normal range"""
    e = torch.floor(torch.log2(p.clamp_min(2.0 ** -14)))
    return 0.5 * torch.exp2(e - 10.0)


def softmax_rows(s32, lds, M, N, scale, causal, n_valid, ldp):
    """pnc_softmax_rows_f16: p[m * ldp + j] = softmax_j(scale * s[m * lds + j]) over the VISIBLE columns j < n_valid (<= 0: N), and with
    `causal` j <= m.  The masks are predicates: a masked column is exactly 0, takes no part in the sum, and its score is never looked at.
    `scale` is the fp32 value the C argument carries.  Every column j < N of every row is written.

    floor = half an fp16 step at p.  allow = p (E_j + sum_i p_i E_i + (N + 5) u), with d_j = |s_j - max s| scale log2(e) and
      E_j = ln 2 (3 d_j u + u^2 |max s| sc) + 2 u
    The kernel forms exp2(fma(s_j, sc, -off)), sc = fl(scale log2 e), off = fl(max sc).  fma = (s_j - max) sc + (max sc - off): the
    second term is the SAME for every column and cancels in the normalisation.  sc carries two roundings (the product and the fp32
    constant): the exponent moves by 2 u d_j; the fma's own rounding is u times its result, d_j + u |max| sc at most: 3 d_j u +
    u^2 |max| sc in the exp2 domain, times ln 2 as a relative error of the power; v_exp_f32 is a one-ulp instruction: 2 u.
    The row sum inherits the p-weighted mean of the E_i, and adds N u for N fp32 additions in any order ((N - 1) u to first order);
    the reciprocal one ulp (2 u), the final product u, and 2 u of slack for the second-order terms."""
    sc = _f32(scale)
    m, j = torch.arange(M).view(M, 1), torch.arange(N).view(1, N)
    nv = n_valid if n_valid > 0 else N
    vis = (j < nv) & ((j <= m) if causal else torch.ones(M, N, dtype=torch.bool))
    S = torch.where(vis, _flat64(s32)[m * lds + j], torch.zeros((), dtype=torch.float64))      # a masked score is never a value
    mx = torch.where(vis, S, torch.full((), -math.inf, dtype=torch.float64)).amax(dim=1, keepdim=True)
    e = torch.where(vis, torch.exp(sc * (S - mx)), torch.zeros((), dtype=torch.float64))
    p = e / e.sum(dim=1, keepdim=True)
    d = (S - mx).abs() * sc * LOG2E
    E = torch.where(vis, math.log(2.0) * (3.0 * d * U + U * U * mx.abs() * sc * LOG2E) + 2.0 * U, torch.zeros((), dtype=torch.float64))
    allow = p * (E + (p * E).sum(dim=1, keepdim=True) + (N + 5) * U)
    floor = torch.where(vis, floor_f16(p), torch.zeros((), dtype=torch.float64))
    ex = Expect(m * ldp + j, p, floor=floor, allow=allow)
    ex.vis = vis
    return {"p16": ex}
