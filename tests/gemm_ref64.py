"""float64 reference of the MFMA GEMM family (pnc_gemm_f16 / pnc_gemm_wsplit_f16), written from section 1 of include/panacea_hip.h
alone: it does not import tests/emu.py and uses no torch convolution, padding or interpolation.  Every operand element is fetched
from the FLAT storage of its buffer at the address the header spells out, and only the elements the contract names are fetched —
everything else of a buffer may hold NaN (tests/gemm_edge_cases.py makes sure it does).

    gather_index / gather_a   the A operand of every gather mode as an [M, K] matrix in W's K order
    gemm                      contraction + epilogue of one launch -> float64 expectations, the `mag` of the same passes with every
                              factor replaced by its absolute value, and for every output buffer the flat indices it is written at
    bound                     the error a correct fp32-accumulating kernel may show against `gemm`, derived term by term (docstring)

    monitor_expect / monitor_bracket / silu_tail   the exact statements over the operand range (bound, points 6 and 7)
    model_outputs             the output planes and the monitor count of a kernel with an exact accumulator, and of five wrong writers

`ln_*` and `gn_part` are out of scope (tests/test_norm_offsets_gpu.py holds them to float64): `gemm` rejects them.
`mutate` (tests/test_gemm_ref64.py, tests/test_gemm_range_ref64.py only) turns the reference into one of the wrong kernels the bound
has to catch."""
import math

import torch

A_PLAIN, A_CONV3X3, A_CONV1D_T = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
S = 2.0 ** -11              # weight of a lo plane
U = 2.0 ** -24              # unit roundoff of fp32
MUTANTS = ("acc16", "drop_last_chunk", "halo_zero", "ignore_pad_br", "rb_mod_m", "geglu_halves", "frame_neighbour")
# wrong kernels over the operand RANGE (tests/test_gemm_range_ref64.py): the first four misread an operand and change `gemm`'s value,
# the others miswrite an output plane or miscount and change `model_outputs`
# The fp16 MFMA of the MI355X takes an fp16-SUBNORMAL factor exactly but unnormalised: its product is aligned in the adder as if the
# factor were 2^-14 and truncated there (bound, point 8).  True: `mag` counts such a factor as 2^-14.
MFMA_UNNORMALISED_SUBNORMALS = True
RANGE_MUTANTS_IN = ("wexp_ignored", "wexp_off_by_one", "e4m3_fnuz", "flush16_in")
RANGE_MUTANTS_OUT = ("flush16_out", "lo_sat_240", "lo_unclamped", "hi_rtz", "monitor_per_element")


# ----------------------------------------------------------------------------------------------------------------- the A operand
def _k_order(K, C, taps):
    """k -> (tap, channel) for the two K orders of the conv gathers: (tap, ci), or (ci/64, tap, ci%64) when C % 64 == 0"""
    k = torch.arange(K, dtype=torch.int64)
    if C % 64 == 0:
        cc, r = k // (64 * taps), k % (64 * taps)
        return r // 64, cc * 64 + r % 64
    return k // C, k % C


def gather_index(*, M, K, lda=0, a_mode=A_PLAIN, conv=None, tconv=None, mutate=None):
    """-> (idx int64 [M, K], ok bool [M, K]): element (m, k) of gatherA is A_flat[idx] where ok, an exact 0 elsewhere (a tap outside
    the image / the clip: never fetched)."""
    m = torch.arange(M, dtype=torch.int64).view(M, 1)
    if a_mode == A_PLAIN:
        return m * lda + torch.arange(K, dtype=torch.int64).view(1, K), torch.ones(M, K, dtype=torch.bool)
    if a_mode == A_CONV3X3:
        C, Hin, Win, Hout, Wout = (conv[n] for n in ("Cin", "Hin", "Win", "Hout", "Wout"))
        stride, up, pad_br, xh = conv.get("stride", 1), int(conv.get("upsample", 0)), int(conv.get("pad_br", 0)), int(conv.get("x_halo_off", 0))
        assert K == 9 * C and M % (Hout * Wout) == 0
        F = M // (Hout * Wout)
        tap, ci = _k_order(K, C, 9)
        ky, kx = (tap // 3).view(1, K), (tap % 3).view(1, K)
        f, oy, ox = m // (Hout * Wout), (m // Wout) % Hout, m % Wout          # row m = (f * Hout + oy) * Wout + ox
        # the image the taps walk: the input, or its nearest x2 upsampling; one zero row / column on every side (pad 1), or on the
        # bottom / right only (conv_pad_br: F.pad(x, (0, 1, 0, 1)) + padding 0)
        Hv, Wv = (2 * Hin, 2 * Win) if up else (Hin, Win)
        pad = 0 if (pad_br and mutate != "ignore_pad_br") else 1
        vy, vx = oy * stride + ky - pad, ox * stride + kx - pad
        iy, ix = (vy // 2, vx // 2) if up else (vy, vx)                        # floor: column -1 stays -1, column Wv becomes Win
        rows_in, cols_in = (vy >= 0) & (vy < Hv), (vx >= 0) & (vx < Wv)
        idx = ((f * Hin + iy) * Win + ix) * C + ci.view(1, K)
        ok = rows_in & cols_in
        if mutate == "frame_neighbour":            # a row above / below the frame read from the neighbouring frame's storage
            fy = f * Hin + iy
            ok = cols_in & (fy >= 0) & (fy < F * Hin)
        if xh and mutate != "halo_zero":           # columns -1 / Win of a band: block [2][F][Hin][C] at A + x_halo_off
            left, right = rows_in & (vx == -1), rows_in & (vx == Wv)
            hidx = xh + ((torch.where(left, 0, 1) * F + f) * Hin + iy) * C + ci.view(1, K)
            idx = torch.where(left | right, hidx, idx)
            ok = ok | left | right
        return idx, ok
    C, T, Npix, halo = tconv["C"], tconv["T"], tconv["Npix"], int(tconv.get("halo", 0))
    assert K == 3 * C and M % (T * Npix) == 0
    tap, ci = _k_order(K, C, 3)
    b, t, p = m // (T * Npix), (m // Npix) % T, m % Npix                      # row m = (b * T + t) * Npix + p
    tt = t + tap.view(1, K) - 1
    if halo:                                       # T + 2 frames per sample, frame t at slot t + 1, no tap padded
        return ((b * (T + 2) + tt + 1) * Npix + p) * C + ci.view(1, K), torch.ones(M, K, dtype=torch.bool)
    idx = ((b * T + tt) * Npix + p) * C + ci.view(1, K)
    ok = (tt >= 0) & (tt < T)
    if mutate == "frame_neighbour":                # the last frame of the previous sample / the first of the next
        ok = (b * T + tt >= 0) & (b * T + tt < (M // Npix))
    return idx, ok


def _values(plane):
    """flat float64 values of an operand plane: fp16 / fp32 as they are, uint8 = OCP e4m3 bytes"""
    flat = plane.reshape(-1)
    return (flat.view(torch.float8_e4m3fn).float() if flat.dtype == torch.uint8 else flat).double()


_plane_values = _values


def _fetch(flat, idx, ok):
    out = torch.zeros(idx.shape, dtype=torch.float64)
    out[ok] = flat[idx[ok]]
    return out


def gather_a(plane, **geo):
    """float64 [M, K] gatherA of one plane (A, or A_lo in either format) in W's K order"""
    idx, ok = gather_index(**geo)
    return _fetch(_values(plane), idx, ok)


def _w(plane, N, K, ld, values=None):
    n, k = torch.arange(N, dtype=torch.int64).view(N, 1), torch.arange(K, dtype=torch.int64).view(1, K)
    return (values or _values)(plane)[n * ld + k]


# ------------------------------------------------------------------------------------------------------------------- the launch
def _phi(x):
    return 0.5 * (1.0 + torch.erf(x * math.sqrt(0.5)))


def gemm(a16, w16, *, M, N, K, lda=0, a_mode=A_PLAIN, conv=None, tconv=None, bias=None, rowbias=None, rb_rows=0, rb_mod=0,
         res1=None, ldr1=0, res2=None, ldr2=0, out32=None, ldc32=0, out16=None, ldc16=0, out16t=None, ldt=0, t_rows=0, t_gstride=0,
         n_split=0, act=ACT_NONE, geglu=False, a16_lo=None, out16_lo=None, w_ld=0, w_lo=None, w_lo16=None, ln_out16=None,
         gn_part=None, mutate=None, **unsupported):
    """The launch hip.gemm(a16, w16, **same keywords) describes, in float64.  Output tensors are only looked at for `is None`.
    -> dict: v [M, No] the epilogue's value per (m, n) (No = N / 2 under GEGLU), `outs` = {buffer name: (flat indices [M, n], columns
    n of v they receive)} for out32 / out16 / out16_lo / out16t, and the fields `bound` reads."""
    if ln_out16 is not None or gn_part is not None or unsupported:
        raise ValueError(f"out of scope for this reference: ln_* / gn_part / {sorted(unsupported)}")
    assert mutate is None or mutate in MUTANTS + RANGE_MUTANTS_IN
    geo = dict(M=M, K=K, lda=lda, a_mode=a_mode, conv=conv, tconv=tconv, mutate=mutate)

    def _values(plane):                                                  # (shadows the module's: every plane of the launch)
        x = _plane_values(plane)
        if mutate == "flush16_in" and plane.dtype == torch.float16:      # fp16-subnormal operand elements read as 0
            x = torch.where(x.abs() < 2.0 ** -14, torch.zeros_like(x), x)
        if mutate == "e4m3_fnuz" and plane.dtype == torch.uint8:         # exponent bias 8 (MI300's format) instead of OCP's 7
            x = x * 0.5
        return x
    idx, ok = gather_index(**geo)
    if mutate == "drop_last_chunk":
        ok = ok.clone()
        ok[:, K - 8:] = False
    ldw = w_ld or K
    Ah, Wh = _fetch(_values(a16), idx, ok), _w(w16, N, K, ldw, _values)
    passes = [(Ah, Wh, 1.0)]                                   # (A factor, W factor, weight) of every K pass of the launch
    e4m3 = a16_lo is not None and a16_lo.dtype == torch.uint8
    if e4m3:                                                   # e4m3(A_lo) . e4m3(W_lo) 2^(w_lo_exp - 127), weighted 2^-11
        w8, w_exp = w_lo
        w_exp = 116 if mutate == "wexp_ignored" else int(w_exp) + 1 if mutate == "wexp_off_by_one" else int(w_exp)
        passes.append((_fetch(_values(a16_lo), idx, ok), _w(w8, N, K, w8.shape[-1], _values) * 2.0 ** (w_exp - 127), S))
    elif a16_lo is not None:
        passes.append((_fetch(_values(a16_lo), idx, ok), Wh, S))
    wl16 = w_lo16 if w_lo16 is not None else (w_lo if torch.is_tensor(w_lo) else None)
    if wl16 is not None:                                       # split weights: A_hi . W_lo, weighted 2^-11 (A_lo . W_lo is dropped)
        assert wl16.dtype == torch.float16 and (w_lo16 is not None or (a16_lo is not None and not e4m3))
        passes.append((Ah, _w(wl16, N, K, ldw, _values), S))
    acc = sum(s * (a @ w.t()) for a, w, s in passes)

    def aligned(x, i):                                         # |x| as the MFMA's adder aligns it (bound, point 8); pass 1 of an
        on = MFMA_UNNORMALISED_SUBNORMALS and not (e4m3 and i == 1)      # e4m3 pair holds no fp16 plane
        return torch.where((x != 0) & (x.abs() < 2.0 ** -14), 2.0 ** -14, x.abs()) if on else x.abs()
    mag = sum(s * (aligned(a, i) @ aligned(w, i).t()) for i, (a, w, s) in enumerate(passes))
    if mutate == "acc16":
        acc = acc.half().double()
    m = torch.arange(M, dtype=torch.int64)
    pre, amag, n_add = acc, mag, 0
    if bias is not None:
        b = _values(bias)[:N]
        pre, amag, n_add = pre + b, amag + b.abs(), n_add + 1
    if rowbias is not None:
        ridx = (m % rb_mod) if mutate == "rb_mod_m" else (m // rb_rows) % rb_mod
        rb = _values(rowbias)[ridx.view(M, 1) * N + torch.arange(N).view(1, N)]
        pre, amag, n_add = pre + rb, amag + rb.abs(), n_add + 1
    r = dict(K_passes=len(passes) * K, pre=pre, pre_mag=amag, pre_adds=n_add, act=act, geglu=bool(geglu))
    if geglu:
        if mutate == "geglu_halves":
            val, gate = pre[:, : N // 2], pre[:, N // 2:]
            r["val_mag"], r["gate_mag"] = amag[:, : N // 2], amag[:, N // 2:]
        else:                                                  # 64 columns = 32 of `value` followed by the 32 of their `gate`
            blk = pre.view(M, N // 64, 2, 32)
            val, gate = blk[:, :, 0].reshape(M, N // 2), blk[:, :, 1].reshape(M, N // 2)
            bm = amag.view(M, N // 64, 2, 32)
            r["val_mag"], r["gate_mag"] = bm[:, :, 0].reshape(M, N // 2), bm[:, :, 1].reshape(M, N // 2)
        r["val"], r["gate"] = val, gate
        v = val * gate * _phi(gate)
        No = N // 2
    else:
        v = pre * torch.sigmoid(pre) if act == ACT_SILU else pre * _phi(pre) if act == ACT_GELU else pre
        No = N
    r["f"] = v
    cols = torch.arange(No, dtype=torch.int64).view(1, No)
    res_mag, res_adds = torch.zeros(M, No, dtype=torch.float64), 0
    for res, ld in ((res1, ldr1), (res2, ldr2)):
        if res is not None:
            x = _values(res)[m.view(M, 1) * ld + cols]
            v, res_mag, res_adds = v + x, res_mag + x.abs(), res_adds + 1
    r.update(v=v, res_mag=res_mag, res_adds=res_adds)
    ns = n_split if out16t is not None else No
    outs = {}
    row = m.view(M, 1)
    if out32 is not None:
        outs["out32"] = (row * ldc32 + cols[:, :ns], slice(0, ns))
    if out16 is not None:
        outs["out16"] = (row * ldc16 + cols[:, :ns], slice(0, ns))
        if out16_lo is not None:
            outs["out16_lo"] = outs["out16"]
    if out16t is not None:
        outs["out16t"] = ((row // t_rows) * t_gstride + (cols[:, ns:] - ns) * ldt + row % t_rows, slice(ns, No))
    r["outs"] = outs
    r["out_lo_e4m3"] = out16_lo is not None and out16_lo.dtype == torch.uint8
    return r


# -------------------------------------------------------------------------------------------------------------------- the bound
L_SILU, L_GELU = 1.1, 1.13        # max |d/dx x sigmoid(x)| = 1.0998, max |d/dx x Phi(x)| = 1.1290
PHI_TAB = 1.8e-6                  # gemm_kernel.h, gelu_tab_f: linear interpolation of Phi in steps of 1/128, h^2 / 8 max |Phi''|


def bound(r, name="out32"):
    """|kernel - reference| a correct kernel may show at every (m, n) of the columns buffer `name` receives.  u = 2^-24.  Nothing here
    is fitted to a kernel's output; tests/test_gemm_ref64.py shows honest fp32 (tests/emu.py on the CPU) inside it and an fp16-staged
    accumulator outside.

    1. accumulation + additions.  The fp16 x fp16 and e4m3 x e4m3 products are exact in fp32, the 2^-11 weights exact scalings.  A sum
       of n fp32 terms in ANY order with round-to-nearest additions is off by at most (n - 1) u sum|terms| (1 + O(n u)); a truncating
       adder doubles the per-addition error.  With n = K_passes products (K per pass of the launch) + E added streams:
           b_lin = 2 (K_passes + E) u (mag + |bias| + |rowbias| + |res1| + |res2|)
       — the issue's formula; it does not depend on the summation order (split-K, the MFMA's internal tree) nor on the rounding mode.
    2. activations see pre = acc + bias + rowbias with b_pre = 2 (K_passes + E_pre) u (mag + |bias| + |rowbias|):
       SiLU  f = x sigmoid(x), silu_f = v * rcp(1 + __expf(-v)):  L_SILU b_pre  (Lipschitz)  +  (8 + 2 |x|) u |f|: __expf is
             exp2(v log2 e) — the rounded product moves the exponent by |v| u log2 e, i.e. the result by |v| u relatively, once for the
             product and once for the constant — then exp2, the addition, the reciprocal and the product, each within one ulp = 2 u.
       GELU  f = x Phi(x), 0.5 v (1 + erff(v / sqrt 2)):  L_GELU b_pre  +  |x| (4 + |x|) 2 u + 4 u |f|: erff within 4 ulp of a value
             <= 1 (the sum 1 + erf cancels for x < 0, so the term is absolute, times 0.5 |x|; with the additions' own ulp), the
             argument's rounding |x| u times max erf' / sqrt 2 < 1, two roundings of the products.
       GEGLU out = value * gate * Phi_tab(gate):  |value| (L_GELU b_gate + |gate| (PHI_TAB + 4 u)) + |gate Phi(gate)| b_value + 4 u |out|
             — the table's documented interpolation error on Phi, its fma / conversion roundings, the two products.
       The residuals are then added to a value that is off by b_act:  b = b_act + 2 E_res u (|f| + b_act + |res1| + |res2|).
    3. out16 / out16t:  + 2^-11 (|ref| + b) for the rounding of the computed value to fp16, + 2^-25 (half a subnormal step).
    4. out16 + 2^-11 out16_lo against the value:  b + 2^-22 (|ref| + b) + 2^-36 for an fp16 lo plane (the residual r = (v - hi) 2^11 is
       exact in fp32, |r| <= |v|, its fp16 rounding 2^-11 |r|, half a subnormal step 2^-25, all times 2^-11);  b + 2^-15 (|ref| + b) +
       2^-21 for e4m3 (3 mantissa bits: 2^-4 |r|; half its subnormal step 2^-10; times 2^-11).  The e4m3 term is the bound of the
       elements with |ref| + b < 512: the kernel's own value is then below 512, |r| <= 256 and nothing clamps.  From there on the
       residual may clamp at +-448 and the pair is held to what the header promises, "degrades gracefully": a clamp moves 2^-11 lo
       towards 0 by less than |v - hi|, and an unclamped r (a multiple of 2^-3 there: exact down to e4m3's subnormal step) is
       rounded by at most 2^-4 |r|, so |v - (hi + 2^-11 lo)| <= |v - hi|, the fp16 rounding error of point 3, and the bound is
       the out16 bound plus b.  Which of the two applies is decided by the reference, never by the output.

    Over the operand range (tests/gemm_edge_cases.py RANGE_CASES; every |v| < 65504, nothing fitted):
    5. `wide-rows` (operands from 2^-24 to 2^13, weights times 2^g) needs no new term: the planes ARE the operands, fp16-subnormal
       elements are exact fp16 values, every product of two planes is exact in fp32 (|product| >= 2^-58, far above fp32's
       subnormals), the block scale 2^(w_lo_exp - 127) and the 2^-11 are exact, and b_lin is relative to `mag`.
    6. `graded-cols` (outputs from 2^-24 to 2^15): points 1 to 4 hold at any magnitude below 65504 because points 3 and 4 carry the
       half steps 2^-25 / 2^-36 of fp16's subnormals.  In the tails of the activations the Lipschitz term L b_pre dominates; SiLU
       at pre < -88: __expf(-v) overflows to +Inf, its reciprocal is +0 and v * 0 = -0, or, where the sum stays finite, |f| <
       88 e^-88 < 2^-120 (`silu_tail`).
    7. a launch that writes out32 next to an e4m3 out16_lo states its planes as functions of its OWN fp32 value (`exact_planes`):
       out16 = fp16(out32) bit for bit, the lo byte = e4m3(clamp((out32 - out16) 2^11, +-448)) as a value (-0 = +0), no byte 0x7F /
       0xFF; out32 itself is held to float64 by b.  With it the range monitor's count follows from out32 (`monitor_expect`), in the
       unit of the writer: store_h8 (every fast epilogue) and the split-K reduce pack ALIGNED QUADS of columns 4 q .. 4 q + 3 and
       count a quad once; the generic epilogue packs one element per call and counts ELEMENTS (include/panacea_hip.h says so).
       Without out32 the count is bracketed (`monitor_bracket`): |r|(v) = 2^11 dist(v, fp16 grid) is 2^11-Lipschitz in v, so the
       kernel's |r| is within 2^11 b of the reference's.
    8. fp16-subnormal factors (MFMA_UNNORMALISED_SUBNORMALS; found by `wide-rows` on the MI355X, the header says so now).  The fp16
       MFMA multiplies a subnormal factor exactly, nothing is flushed, but the adder aligns the product as if the factor were
       2^-14: rows of A at 2^-24 .. 2^-15 showed the SAME absolute truncation per product, about 2^-14 |w| 2^-25, towards -Inf,
       independent of the row's binade and proportional to the weights' scale — up to 2^10 times the 2 u |a w| of point 1, which
       assumes a truncation relative to the product.  So `mag` counts a non-zero fp16 factor below 2^-14 as 2^-14: the error of a
       truncating adder (point 1) relative to what the adder aligns.  Unit-scale data has such factors at a rate of 1e-4 to 1e-3
       and changes by parts in 1e6; a flushed subnormal row is still outside (tests/test_gemm_range_ref64.py)."""
    b, ref = _b(r)[:, r["outs"][name][1]], r["v"][:, r["outs"][name][1]].abs()
    if name in ("out16", "out16t"):
        return b + 2.0 ** -11 * (ref + b) + 2.0 ** -25
    if name == "out16_lo" and r["out_lo_e4m3"]:
        return torch.where(ref + b < 512.0, b + 2.0 ** -15 * (ref + b) + 2.0 ** -21, 2.0 * b + 2.0 ** -11 * (ref + b) + 2.0 ** -25)
    if name == "out16_lo":
        return b + 2.0 ** -22 * (ref + b) + 2.0 ** -36
    return b


def _b_pre(r):
    return 2.0 * (r["K_passes"] + r["pre_adds"]) * U * r["pre_mag"]


def _b(r):
    """points 1 and 2 of `bound` at every (m, n) of the epilogue's value"""
    kp = r["K_passes"]
    if not r["geglu"] and r["act"] == ACT_NONE:
        b = 2.0 * (kp + r["pre_adds"] + r["res_adds"]) * U * (r["pre_mag"] + r["res_mag"])
    else:
        f = r["f"].abs()
        if r["geglu"]:
            bv, bg = (2.0 * (kp + r["pre_adds"]) * U * r[n] for n in ("val_mag", "gate_mag"))
            val, gate = r["val"].abs(), r["gate"].abs()
            b_act = val * (L_GELU * bg + gate * (PHI_TAB + 4 * U)) + gate * _phi(r["gate"]) * bv + 4 * U * f
        else:
            b_pre = 2.0 * (kp + r["pre_adds"]) * U * r["pre_mag"]
            x = r["pre"].abs()
            b_act = L_SILU * b_pre + (8 + 2 * x) * U * f if r["act"] == ACT_SILU else L_GELU * b_pre + x * (4 + x) * 2 * U + 4 * U * f
        b = b_act + 2.0 * r["res_adds"] * U * (f + b_act + r["res_mag"])
    return b


# ------------------------------------------------------------------------------------- planes and monitor over the range (point 7)
def _e4m3(r32):
    """(OCP e4m3 bytes of an fp32 residual clamped to +-448, the mask of the elements that clamped)"""
    return r32.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8), r32.abs() > 448.0


def _count(over, unit):
    """what the range monitor adds for the [M, n] mask of clamped elements: aligned quads of columns, or elements"""
    assert unit in ("quads", "elements")
    if unit == "elements":
        return int(over.sum())
    M, n = over.shape
    assert n % 4 == 0
    return int(over.view(M, n // 4, 4).any(dim=2).sum())


def monitor_expect(out32, out16, unit):
    """the count a launch implies by its own out32 / out16 (both [M, n], as written): residuals beyond +-448, in the writer's unit"""
    return _count(((out32.double() - out16.double()) * 2048.0).abs() > 448.0, unit)


def monitor_bracket(r, unit, slack=1.0):
    """(lower, upper) for the count of a launch that writes an e4m3 out16_lo and no out32: the reference's |r| reduced / increased by
    2^11 (b + 2^-24 |ref|) (the second term: the reference's own rounding to fp32 ahead of the fp16 grid).  slack = 0: what the
    float64 value itself clamps, twice"""
    cols = r["outs"]["out16_lo"][1]
    ref = r["v"][:, cols]
    slack = slack * 2048.0 * (_b(r)[:, cols] + U * ref.abs())
    res = ((ref - ref.float().half().double()) * 2048.0).abs()
    return _count(res - slack > 448.0, unit), _count(res + slack > 448.0, unit)


def silu_tail(r):
    """mask [M, No] of the elements whose pre-activation is below -88 whatever a correct kernel's rounding (pre + b_pre < -88), for a
    SiLU launch with nothing added behind the activation; None for every other launch"""
    if r["geglu"] or r["act"] != ACT_SILU or r["res_adds"]:
        return None
    return r["pre"] + _b_pre(r) < -88.0


def _rtz16(v32):
    """fp32 -> fp16 by truncation"""
    h = v32.half()
    bits = h.view(torch.int16)
    return torch.where(h.float().abs() > v32.abs(), bits - 1, bits).view(torch.float16)      # sign-magnitude: one step towards 0


def model_outputs(r, kw, unit="quads", mutate=None):
    """Writes what a kernel with an exact accumulator would: out32 = fp32(v), out16 / out16t = fp16(out32), out16_lo from the two,
    into the output tensors of `kw` at the indices of `r`.  -> the range monitor's count.  `mutate`: one of RANGE_MUTANTS_OUT."""
    assert mutate is None or mutate in RANGE_MUTANTS_OUT
    count = 0
    for name, (idx, cols) in r["outs"].items():
        if name == "out16_lo":
            continue
        v32 = r["v"][:, cols].float()
        if name == "out32":
            kw[name].reshape(-1)[idx] = v32
            continue
        hi = _rtz16(v32) if mutate == "hi_rtz" else v32.half()
        if mutate == "flush16_out":
            hi = torch.where(hi.abs() < 2.0 ** -14, torch.zeros_like(hi), hi)
        kw[name].reshape(-1)[idx] = hi
        if name == "out16" and "out16_lo" in r["outs"]:
            res = (v32 - hi.float()) * 2048.0
            if not r["out_lo_e4m3"]:
                kw["out16_lo"].reshape(-1)[idx] = res.half()
                continue
            q, over = _e4m3(res.clamp(-240.0, 240.0) if mutate == "lo_sat_240" else res)
            if mutate == "lo_unclamped":                      # the conversion's own answer to a value beyond 448: the NaN code
                q = torch.where(over, torch.where(res < 0, 0xFF, 0x7F).to(torch.uint8), q)
            kw["out16_lo"].reshape(-1)[idx] = q
            count = _count(over, "elements" if mutate == "monitor_per_element" else unit)
    return count
