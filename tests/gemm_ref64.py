"""float64 reference of the MFMA GEMM family (pnc_gemm_f16 / pnc_gemm_wsplit_f16), written from section 1 of include/panacea_hip.h
alone: it does not import tests/emu.py and uses no torch convolution, padding or interpolation.  Every operand element is fetched
from the FLAT storage of its buffer at the address the header spells out, and only the elements the contract names are fetched —
everything else of a buffer may hold NaN (tests/gemm_edge_cases.py makes sure it does).

    gather_index / gather_a   the A operand of every gather mode as an [M, K] matrix in W's K order
    gemm                      contraction + epilogue of one launch -> float64 expectations, the `mag` of the same passes with every
                              factor replaced by its absolute value, and for every output buffer the flat indices it is written at
    bound                     the error a correct fp32-accumulating kernel may show against `gemm`, derived term by term (docstring)

`ln_*` and `gn_part` are out of scope (tests/test_norm_offsets_gpu.py holds them to float64): `gemm` rejects them.
`mutate` (tests/test_gemm_ref64.py only) turns the reference into one of the wrong kernels the bound has to catch."""
import math

import torch

A_PLAIN, A_CONV3X3, A_CONV1D_T = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
S = 2.0 ** -11              # weight of a lo plane
U = 2.0 ** -24              # unit roundoff of fp32
MUTANTS = ("acc16", "drop_last_chunk", "halo_zero", "ignore_pad_br", "rb_mod_m", "geglu_halves", "frame_neighbour")


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


def _fetch(flat, idx, ok):
    out = torch.zeros(idx.shape, dtype=torch.float64)
    out[ok] = flat[idx[ok]]
    return out


def gather_a(plane, **geo):
    """float64 [M, K] gatherA of one plane (A, or A_lo in either format) in W's K order"""
    idx, ok = gather_index(**geo)
    return _fetch(_values(plane), idx, ok)


def _w(plane, N, K, ld):
    n, k = torch.arange(N, dtype=torch.int64).view(N, 1), torch.arange(K, dtype=torch.int64).view(1, K)
    return _values(plane)[n * ld + k]


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
    assert mutate is None or mutate in MUTANTS
    geo = dict(M=M, K=K, lda=lda, a_mode=a_mode, conv=conv, tconv=tconv, mutate=mutate)
    idx, ok = gather_index(**geo)
    if mutate == "drop_last_chunk":
        ok = ok.clone()
        ok[:, K - 8:] = False
    ldw = w_ld or K
    Ah, Wh = _fetch(_values(a16), idx, ok), _w(w16, N, K, ldw)
    passes = [(Ah, Wh, 1.0)]                                   # (A factor, W factor, weight) of every K pass of the launch
    e4m3 = a16_lo is not None and a16_lo.dtype == torch.uint8
    if e4m3:                                                   # e4m3(A_lo) . e4m3(W_lo) 2^(w_lo_exp - 127), weighted 2^-11
        w8, w_exp = w_lo
        passes.append((_fetch(_values(a16_lo), idx, ok), _w(w8, N, K, w8.shape[-1]) * 2.0 ** (int(w_exp) - 127), S))
    elif a16_lo is not None:
        passes.append((_fetch(_values(a16_lo), idx, ok), Wh, S))
    wl16 = w_lo16 if w_lo16 is not None else (w_lo if torch.is_tensor(w_lo) else None)
    if wl16 is not None:                                       # split weights: A_hi . W_lo, weighted 2^-11 (A_lo . W_lo is dropped)
        assert wl16.dtype == torch.float16 and (w_lo16 is not None or (a16_lo is not None and not e4m3))
        passes.append((Ah, _w(wl16, N, K, ldw), S))
    acc = sum(s * (a @ w.t()) for a, w, s in passes)
    mag = sum(s * (a.abs() @ w.abs().t()) for a, w, s in passes)
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
       2^-21 for e4m3 (3 mantissa bits: 2^-4 |r|; half its subnormal step 2^-10; times 2^-11).  Valid below the clamp, |v| < 512."""
    cols = r["outs"][name][1]
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
    b, ref = b[:, cols], r["v"][:, cols].abs()
    if name in ("out16", "out16t"):
        return b + 2.0 ** -11 * (ref + b) + 2.0 ** -25
    if name == "out16_lo":
        return b + (2.0 ** -15 * (ref + b) + 2.0 ** -21 if r["out_lo_e4m3"] else 2.0 ** -22 * (ref + b) + 2.0 ** -36)
    return b
