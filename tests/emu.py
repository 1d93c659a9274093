"""Plain-torch emulation of every wrapper of panacea_amd.hip that the product calls on its backend: same names, same parameters
(names, order, keyword-only split, defaults — tests/test_emu_surface.py holds the two signatures together), results written into
the caller's output tensors.  One module is the whole backend: `engine.use_backend(emu)` and nothing else.  The sections follow
the order of hip.py: GEMM, attention, norms, small-M linears, embeddings and layout, sampler exits, elementwise, statistics.

TEST INFRASTRUCTURE ONLY.  Two uses:
  * `-m gpu` kernel tests: HIP kernel vs this emulation on the same device tensors;
  * `-m "not gpu"` host-logic tests: the engine (weight packing, layouts, quirks, graph order) runs
    on CPU against this module injected in place of `panacea_amd.hip`, and is compared with the oracle.
The product never imports it: `panacea_amd.hip` has no fallback and raises without the HIP library.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as TF

A_PLAIN, A_CONV3X3, A_CONV1D_T = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_GELU = 0, 1, 2
SAMPLER_HEUN1, SAMPLER_HEUN2, SAMPLER_EULER_A, SAMPLER_DPM2S_1, SAMPLER_DPM2S_2, SAMPLER_DPM2M, SAMPLER_LMS = range(7)   # PNC_SAMPLER_*


class PncError(RuntimeError):
    pass


def _r16_default(v: torch.Tensor, site: str) -> torch.Tensor:
    return v.half()


# every fp16 rounding of an activation goes through this hook: r16(value_fp32, producing_entry_point).  The default is
# the kernels' rounding; tools/exp/error_budget.py swaps it to measure what each operand class contributes.
r16 = _r16_default
STRICT_DTYPES = True
LO_SCALE = 2048.0


def _lo(v: torch.Tensor, hi: torch.Tensor, like: torch.Tensor = None) -> torch.Tensor:
    """lo plane of a precise (split) operand, exactly like the kernels: fp16((v - hi) * 2^11), or — when the destination `like`
    is a uint8 tensor (PNC_LO_E4M3) — the OCP e4m3 byte of the same residual clamped to +-448"""
    r = (v.float() - hi.float()) * LO_SCALE
    if like is not None and like.dtype == torch.uint8:
        global _LO_CLAMPED
        _LO_CLAMPED += int((r.abs() > 448.0).reshape(-1, 4).any(dim=1).sum()) if r.numel() % 4 == 0 else int((r.abs() > 448.0).sum())
        return r.clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8)
    return r.half()


_LO_CLAMPED = 0      # e4m3 lo-plane quads that clamped since the last range_monitor_collect (the kernels' per-quad count)


def _lo_value(lo: torch.Tensor) -> torch.Tensor:
    """fp32 value of a lo plane in either storage format"""
    return lo.view(torch.float8_e4m3fn).float() if lo.dtype == torch.uint8 else lo.float()


def _join(hi: torch.Tensor, lo) -> torch.Tensor:
    return hi.float() if lo is None else hi.float() + _lo_value(lo) / LO_SCALE


# ---- MX block-scaled fp8 lo plane (the format of the NEXT round's lo pass; nothing in the library
# produces or consumes it yet — this is the reference the producers / the scaled-MFMA lo pass will be checked against).
# A block is 32 consecutive channels of one row; its scale is one E8M0 byte (2^(byte - 127)); elements are OCP e4m3 bytes.
MX_BLOCK = 32


def mx8_quant(r: torch.Tensor):
    """fp32 [..., C] (C % 32 == 0) -> (e4m3 bytes uint8 [..., C], E8M0 scale bytes uint8 [..., C / 32]).  The scale puts the block
    maximum in [128, 256) (e4m3 tops out at 448: no saturation, at most one binade of head room lost); an all-zero block gets
    scale byte 0 and zero elements."""
    shp = r.shape
    b = r.float().reshape(-1, shp[-1] // MX_BLOCK, MX_BLOCK)
    amax = b.abs().amax(dim=-1, keepdim=True)
    e = torch.where(amax > 0, torch.floor(torch.log2(amax.clamp_min(1e-38))) - 7.0, torch.full_like(amax, -127.0)).clamp(-127.0, 127.0)
    q = (b / torch.exp2(e)).to(torch.float8_e4m3fn)
    return q.view(torch.uint8).reshape(shp), (e + 127.0).to(torch.uint8).reshape(*shp[:-1], shp[-1] // MX_BLOCK)


def mx8_dequant(q: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    shp = q.shape
    v = q.view(torch.float8_e4m3fn).float().reshape(-1, shp[-1] // MX_BLOCK, MX_BLOCK)
    return (v * torch.exp2(scale.float().reshape(-1, shp[-1] // MX_BLOCK, 1) - 127.0)).reshape(shp)


def _lo_mx8(v: torch.Tensor, hi: torch.Tensor):
    """MX fp8 lo plane of a split operand: (v - hi) * 2^11, block-scaled"""
    return mx8_quant((v.float() - hi.float()) * LO_SCALE)


def _mat(t: torch.Tensor, rows: int, cols: int, ld: int) -> torch.Tensor:
    """[rows, cols] strided view (row stride ld) of the flat storage of t."""
    return torch.as_strided(t.reshape(-1), (rows, cols), (ld, 1))


def load():
    return None


ACC_HOOK = None


def _contract(a16, Wm, M, N, K, lda, a_mode, conv, tconv):
    """gatherA[M, K] @ Wm[N, K]^T in fp32: the contraction of every GEMM mode (Wm already a float [N, K] matrix)"""
    if a_mode == A_PLAIN:
        A = _mat(a16, M, K, lda).float()
        acc = A @ Wm.t()
    elif a_mode == A_CONV3X3:
        Cin, Hin, Win, Hout, Wout = conv["Cin"], conv["Hin"], conv["Win"], conv["Hout"], conv["Wout"]
        stride, up = conv.get("stride", 1), conv.get("upsample", 0)
        Fr = M // (Hout * Wout)
        x = a16.reshape(-1)[: Fr * Hin * Win * Cin].view(Fr, Hin, Win, Cin).permute(0, 3, 1, 2).float()
        xh = int(conv.get("x_halo_off", 0))      # PncGemmParams.x_halo_off: columns -1 and Win of a view band, [2][Fr][Hin][Cin]
        if xh:
            cols = a16.reshape(-1)[xh: xh + 2 * Fr * Hin * Cin].view(2, Fr, Hin, Cin).permute(0, 1, 3, 2).float()
            x = torch.cat([cols[0][..., None], x, cols[1][..., None]], dim=3)
        if up:
            x = TF.interpolate(x, scale_factor=2, mode="nearest")
            if xh:
                x = x[..., 1:-1]
        if Cin % 64 == 0:     # K order (ci/64, ky, kx, ci%64)
            w = Wm.view(N, Cin // 64, 3, 3, 64).permute(0, 1, 4, 2, 3).reshape(N, Cin, 3, 3)
        else:                 # K order (ky, kx, ci)
            w = Wm.view(N, 3, 3, Cin).permute(0, 3, 1, 2)
        if conv.get("pad_br", 0):
            y = TF.conv2d(TF.pad(x, (0, 1, 0, 1)), w, stride=stride, padding=0)
        elif xh:
            y = TF.conv2d(TF.pad(x, (0, 0, 1, 1)), w, stride=stride, padding=0)
        else:
            y = TF.conv2d(x, w, stride=stride, padding=1)
        assert y.shape[2] == Hout and y.shape[3] == Wout, (y.shape, Hout, Wout)
        acc = y.permute(0, 2, 3, 1).reshape(M, N)
    else:
        Cc, T, Npix = tconv["C"], tconv["T"], tconv["Npix"]
        B = M // (T * Npix)
        halo = int(tconv.get("halo", 0))       # PncGemmParams.t_halo: A holds T + 2 frames per sample, no temporal padding
        Ta = T + 2 * halo
        x = a16.reshape(-1)[: B * Ta * Npix * Cc].view(B, Ta, Npix, Cc).permute(0, 2, 3, 1).reshape(B * Npix, Cc, Ta).float()
        if Cc % 64 == 0:      # K order (ci/64, dt, ci%64)
            w = Wm.view(N, Cc // 64, 3, 64).permute(0, 1, 3, 2).reshape(N, Cc, 3)
        else:                 # K order (dt, ci)
            w = Wm.view(N, 3, Cc).permute(0, 2, 1)
        y = TF.conv1d(x, w, padding=0 if halo else 1)        # [B*Npix, N, T]
        acc = y.view(B, Npix, N, T).permute(0, 3, 1, 2).reshape(M, N)
    return acc


# ---- GEMM (pnc_gemm_f16 / pnc_gemm_wsplit_f16; the kernels are held to float64 by tests/test_gemm_edges_gpu.py) ----------------
# Split operands: A W ~= A_hi W_hi + 2^-11 (A_lo W_hi + A_hi W_lo), the 2^-22 A_lo W_lo term dropped.  An fp16 A_lo is joined to
# A_hi in fp32 ahead of the contraction; an e4m3 A_lo runs its own pass against the e4m3 copy of the weights (`w_lo` = the (bytes,
# exponent) pair of engine.pk_lo8).  The fp16 lo plane of the WEIGHTS arrives as `w_lo` (PncGemmParams.W_lo, `precise-full`: next
# to an fp16 A_lo only) or as `w_lo16` (beside the parameter block, pnc_gemm_wsplit_f16, `precise-ckpt`: next to every A_lo — none,
# e4m3, or fp16, which the library forwards to the three-part launch).  The sum is linear in W, so 2^-11 A_hi W_lo is one more
# contraction added to the fp32 accumulator ahead of the epilogue.
def gemm(a16, w16, *, M, N, K, lda=0, a_mode=A_PLAIN, conv=None, tconv=None, bias=None, rowbias=None, rb_rows=0, rb_mod=0,
         res1=None, ldr1=0, res2=None, ldr2=0, out32=None, ldc32=0, out16=None, ldc16=0, out16t=None, ldt=0, t_rows=0,
         t_gstride=0, n_split=0, act=ACT_NONE, geglu=False, a16_lo=None, out16_lo=None, w_ld=0, w_lo=None, w_lo16=None,
         ln_gamma=None, ln_beta=None, ln_out16=None, ldln=0, ln_eps=1e-5, ln_in_library=False, gn_part=None):
    f16 = torch.float16
    if w_lo16 is not None:
        if w_lo16.dtype != f16 or w_lo16.shape != w16.shape:
            raise PncError("w_lo16: the fp16 lo plane of the weights in w16's layout")
        if a16_lo is not None and a16_lo.dtype == f16:
            if w_lo is not None:
                raise PncError("an fp16 A_lo is forwarded with W_lo = W_lo16: W_lo must be NULL (PNC_EINVAL)")
            w_lo, w_lo16 = w_lo16, None
    if isinstance(w_lo, torch.Tensor):                  # else None, or the (bytes, exponent) pair of an e4m3 lo pass
        if a16_lo is None:
            raise PncError("W_lo without A_lo (PNC_EINVAL)")
        if a16_lo.dtype != f16 or w_lo.dtype != f16:
            raise PncError("split weights go with fp16 lo planes")
        w_lo, w_lo16 = None, w_lo
    assert (not STRICT_DTYPES) or (a16.dtype == f16 and w16.dtype == f16)
    assert K % 8 == 0
    Wm = _mat(w16, N, K, w_ld or K).float()
    acc_w = None                                        # 2^-11 A_hi W_lo, from the hi plane of A
    if w_lo16 is not None:
        acc_w = _contract(a16, _mat(w_lo16, N, K, w_ld or K).float(), M, N, K, lda, a_mode, conv, tconv) / LO_SCALE
    acc_lo = None
    if a16_lo is not None and a16_lo.dtype == torch.uint8:
        # e4m3 lo plane: its pass runs against the e4m3 copy of the weights (engine.pk_lo8), products weighted 2^-11
        if w_lo is None:
            raise PncError("an e4m3 lo plane needs the e4m3 copy of the weights (w_lo)")
        cin = lda if a_mode == A_PLAIN else (conv["Cin"] if a_mode == A_CONV3X3 else tconv["C"])
        if K % 16 or cin % (16 if a_mode == A_PLAIN else 64):      # the library's PNC_EALIGN
            raise PncError("e4m3 lo pass: K % 16 == 0 and lda % 16 == 0 (plain) / Cin % 64 == 0 (conv gathers)")
        Wl = _mat(w_lo[0], N, K, w_lo[0].shape[-1]).view(torch.float8_e4m3fn).float() * (2.0 ** (int(w_lo[1]) - 127))
        acc_lo = _contract(_lo_value(a16_lo.reshape(-1)[: a16.numel()]).reshape(a16.shape), Wl, M, N, K, lda, a_mode, conv, tconv) / LO_SCALE
    elif a16_lo is not None:     # fp16 lo plane: A = hi + lo * 2^-11 (the kernel sums the two planes' products in fp32)
        a16 = _join(a16.reshape(-1), a16_lo.reshape(-1)[: a16.numel()])
    acc = _contract(a16, Wm, M, N, K, lda, a_mode, conv, tconv)
    if acc_lo is not None:
        acc = acc + acc_lo
    if ACC_HOOK is not None:     # numerics experiments (tools/exp/error_budget.py): e.g. the weight side of an MX lo pass
        acc = ACC_HOOK(acc, a16, Wm, dict(M=M, N=N, K=K, lda=lda, a_mode=a_mode, conv=conv, tconv=tconv))
    if acc_w is not None:
        acc = acc + acc_w
    v = acc
    if bias is not None:
        v = v + bias.reshape(-1)[:N].float()
    if geglu:
        assert N % 64 == 0
        vb = v.view(M, N // 64, 2, 32)
        v = (vb[:, :, 0, :] * TF.gelu(vb[:, :, 1, :])).reshape(M, N // 2)
        if out32 is not None:
            _mat(out32, M, N // 2, ldc32).copy_(v)
        if out16 is not None:
            h = r16(v, 'gemm.geglu')
            _mat(out16, M, N // 2, ldc16).copy_(h)
            if out16_lo is not None:
                _mat(out16_lo, M, N // 2, ldc16).copy_(_lo(v, h, out16_lo))
        return
    if rowbias is not None:
        idx = (torch.arange(M, device=v.device) // rb_rows) % rb_mod
        v = v + rowbias.reshape(-1)[: rb_mod * N].view(rb_mod, N).float()[idx]
    if act == ACT_SILU:
        v = TF.silu(v)
    if act == ACT_GELU:
        v = TF.gelu(v)
    if res1 is not None:
        v = v + _mat(res1, M, N, ldr1)
    if res2 is not None:
        v = v + _mat(res2, M, N, ldr2)
    ns = n_split if out16t is not None else N
    if out32 is not None:
        _mat(out32, M, ns, ldc32).copy_(v[:, :ns])
    if out16 is not None:
        h = r16(v[:, :ns], 'gemm.out16')
        _mat(out16, M, ns, ldc16).copy_(h)
        if out16_lo is not None:
            _mat(out16_lo, M, ns, ldc16).copy_(_lo(v[:, :ns], h, out16_lo))
    if ln_out16 is not None:
        assert out32 is not None and out16t is None
        layernorm(out32, ldc32, M, N, ln_gamma, ln_beta, ln_eps, ln_out16, ldln)
    if gn_part is not None:      # PncGemmParams.gn_part: the records pnc_groupnorm_stats writes for 64-pixel chunks
        assert a_mode == A_CONV1D_T and out32 is not None and N % 64 == 0
        groupnorm_stats(out32, ldc32, M // tconv["Npix"], tconv["Npix"], N, 64, gn_part)
    if out16t is not None:
        G = M // t_rows
        assert G * t_rows == M
        dst = torch.as_strided(out16t.reshape(-1), (G, N - ns, t_rows), (t_gstride, ldt, 1))
        dst.copy_(r16(v[:, ns:], 'gemm.out16t').view(G, t_rows, N - ns).permute(0, 2, 1))


# ---- attention (pnc_attn_views_f16, pnc_softmax_rows_f16, pnc_attn_temporal_f16) ------------------------------------------------
PERM16 = (0, 1, 2, 3, 8, 9, 10, 11, 4, 5, 6, 7, 12, 13, 14, 15)


def _unfrag(fr: torch.Tensor) -> torch.Tensor:
    """inverse of engine.mfma_a_fragments: [R, S, 64, 8] -> [32 R, 16 S]"""
    R, S = fr.shape[0], fr.shape[1]
    wp = fr.reshape(R, S, 2, 32, 8).permute(0, 3, 1, 2, 4).reshape(R, 32, S, 16)
    inv = [PERM16.index(k) for k in range(16)]
    return wp[..., inv].reshape(R * 32, S * 16)


def attn_views(q, ldq, k, ldk, vt, ldvt, vt_gstride, o, ldo, *, groups, heads, H, W, views, kvH, kvW,
               kv_views, kv_rows_per_group, q_per_kv, kv_valid, segs, scale, causal=False, k_halo=None, vt_halo=None):
    Cc = heads * 64
    Wv, kvWv = W // views, kvW // kv_views
    Q = _mat(q, groups * H * W, Cc, ldq).float().view(groups, H, W, heads, 64)
    n_kvg = (groups + q_per_kv - 1) // q_per_kv

    def kv_maps(kb, vb):
        Ka = _mat(kb, n_kvg * kv_rows_per_group, Cc, ldk).float().view(n_kvg, kv_rows_per_group, heads, 64)
        Ka = Ka[:, : kvH * kvW].reshape(n_kvg, kvH, kvW, heads, 64)
        Va = torch.as_strided(vb.reshape(-1), (n_kvg, Cc, kvH * kvW), (vt_gstride, ldvt, 1)).float()
        return Ka, Va.view(n_kvg, heads, 64, kvH, kvW)
    Kband, Vband = kv_maps(k, vt)
    # PncAttnParams.k_halo: view id -1 / kv_views = view column 0 of a buffer laid out like the band's
    halos = None if k_halo is None else [kv_maps(k_halo[i], vt_halo[i]) for i in range(2)]
    O = _mat(o, groups * H * W, Cc, ldo).view(groups, H, W, Cc)
    gidx = torch.arange(groups, device=q.device) // q_per_kv
    for v in range(views):
        qv = Q[:, :, v * Wv:(v + 1) * Wv].reshape(groups, H * Wv, heads, 64).permute(0, 2, 1, 3)
        ks, vs = [], []
        for u in segs[v]:
            Kall, Vall = Kband, Vband
            if u == -1 or u == kv_views:
                Kall, Vall = halos[0 if u < 0 else 1]
                u = 0
            kk = Kall[:, :, u * kvWv:(u + 1) * kvWv].reshape(n_kvg, kvH * kvWv, heads, 64)[:, :kv_valid]
            vv = Vall[:, :, :, :, u * kvWv:(u + 1) * kvWv].reshape(n_kvg, heads, 64, kvH * kvWv)[..., :kv_valid]
            ks.append(kk.permute(0, 2, 1, 3))          # [g, heads, keys, 64]
            vs.append(vv.permute(0, 1, 3, 2))
        kc = torch.cat(ks, dim=2)[gidx]
        vc = torch.cat(vs, dim=2)[gidx]
        s = torch.einsum("ghqd,ghkd->ghqk", qv, kc) * scale
        if causal:          # view-local key index <= view-local query index, in every key segment
            nk = min(kv_valid, kvH * kvWv)
            kidx = torch.arange(nk, device=s.device).repeat(len(segs[v]))
            qidx = torch.arange(H * Wv, device=s.device)
            s = s.masked_fill(kidx[None, :] > qidx[:, None], float("-inf"))
        pr = torch.softmax(s, dim=-1)
        ov = torch.einsum("ghqk,ghkd->ghqd", pr, vc)   # [g, heads, q, 64]
        ov = ov.permute(0, 2, 1, 3).reshape(groups, H, Wv, Cc)
        O[:, :, v * Wv:(v + 1) * Wv] = r16(ov, 'attn_views')


# ---- split-operand attention (pnc_attn_views_split_f16, pnc_attn_temporal_split_f16; CPU tensors only) -------------------------
# The kernels' arithmetic in fp32 — S = Qh.Kh + 2^-11 (Qh.Kl + Ql.Kh), fp32 softmax, P split into an fp16 pair,
# O = Ph.Vh + 2^-11 (Ph.Vl + Pl.Vh) — written as hi + fp16 lo planes.  The `_exact` forms: float64 attention of the operand values
# hi + lo * 2^-11 (no term dropped), returned with the query rows instead of written; tests/test_precise_wide_gpu.py holds the HIP
# kernels to them on the MI355X.
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
    S = 1.0 / LO_SCALE
    if exact:
        d = torch.float64
        q, k, v = (a.to(d) + b.to(d) * S for a, b in ((qh, ql), (kh, kl), (vh, vl)))
        return torch.softmax((q @ k.transpose(-1, -2)) * scale, dim=-1) @ v
    qh, ql, kh, kl, vh, vl = (t.float() for t in (qh, ql, kh, kl, vh, vl))
    s = qh @ kh.transpose(-1, -2) + (qh @ kl.transpose(-1, -2) + ql @ kh.transpose(-1, -2)) * S
    p = torch.softmax(s * scale, dim=-1)
    ph = p.half().float()
    pl = ((p - ph) * LO_SCALE).half().float()
    return ph @ vh + (ph @ vl + pl @ vh) * S


def _write_split(o, o_lo, rows, ldo, Cc, val):
    """val [..., heads, nq, 64] at the query rows `rows` [..., nq]"""
    val = val.float()
    heads = val.shape[-3]
    flat = val.movedim(-3, -2).reshape(-1, heads * 64)          # [..., nq, heads*64]
    r = rows.reshape(-1)
    hi = r16(flat, "attn_split")
    _mat(o, int(r.max()) + 1, Cc, ldo)[r] = hi
    _mat(o_lo, int(r.max()) + 1, Cc, ldo)[r] = _lo(flat, hi)


def _views_split(exact, q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, *, groups, heads, H, W, views, kvH, kvW, kv_views, kv_rows_per_group,
                 q_per_kv, kv_valid, segs, scale):
    """-> ([g, heads, nq, 64] per view, query rows [g, views, nq])"""
    Cc = heads * 64
    kvWv = kvW // kv_views
    n_kvg = (groups + q_per_kv - 1) // q_per_kv
    qrows = _rows_views(groups, H, W, views)
    nrows_q, nrows_kv = groups * H * W, n_kvg * kv_rows_per_group

    def heads_of(t, ld, rows, n):
        return _mat(t, n, Cc, ld)[rows].view(*rows.shape, heads, 64).movedim(-2, -3)     # [..., heads, n, 64]
    out = []
    for vw in range(views):
        qr = qrows[:, vw]
        qh, ql = heads_of(q, ldq, qr, nrows_q), heads_of(q_lo, ldq, qr, nrows_q)
        kr = torch.stack([torch.cat([_kv_rows(g // q_per_kv, u, kvW, kvWv, kv_rows_per_group, kv_valid) for u in segs[vw]])
                          for g in range(groups)])                       # [g, nk]
        kh, kl = heads_of(k, ldk, kr, nrows_kv), heads_of(k_lo, ldk, kr, nrows_kv)
        vh, vl = heads_of(v, ldv, kr, nrows_kv), heads_of(v_lo, ldv, kr, nrows_kv)
        out.append(_attend(qh, ql, kh, kl, vh, vl, scale, exact))
    return out, qrows


def attn_views_split(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, *, groups, heads, H, W, views, kvH, kvW, kv_views,
                     kv_rows_per_group, q_per_kv, kv_valid, segs, scale):
    out, qrows = _views_split(False, q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, groups=groups, heads=heads, H=H, W=W, views=views,
                              kvH=kvH, kvW=kvW, kv_views=kv_views, kv_rows_per_group=kv_rows_per_group, q_per_kv=q_per_kv,
                              kv_valid=kv_valid, segs=segs, scale=scale)
    for vw in range(views):
        _write_split(o, o_lo, qrows[:, vw], ldo, heads * 64, out[vw])


def attn_views_split_exact(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, **geo):
    """-> (float64 [g, views, heads, nq, 64], query rows [g, views, nq]); `geo`: the keywords of attn_views_split"""
    out, qrows = _views_split(True, q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, **geo)
    return torch.stack(out, 1), qrows


def _temporal_split(exact, q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, *, B, T, Npix, heads, scale):
    """-> ([B, Npix, heads, T, 64], rows [B, Npix, T])"""
    Cc, M = heads * 64, B * T * Npix
    rows = (torch.arange(B).view(-1, 1, 1) * T * Npix + torch.arange(Npix).view(1, -1, 1)
            + torch.arange(T).view(1, 1, -1) * Npix)

    def g(t, ld):
        return _mat(t, M, Cc, ld)[rows].view(B, Npix, T, heads, 64).movedim(-2, -3)
    return _attend(g(q, ldq), g(q_lo, ldq), g(k, ldk), g(k_lo, ldk), g(v, ldv), g(v_lo, ldv), scale, exact), rows


def attn_temporal_split(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, o, o_lo, ldo, *, B, T, Npix, heads, scale):
    val, rows = _temporal_split(False, q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, B=B, T=T, Npix=Npix, heads=heads, scale=scale)
    _write_split(o, o_lo, rows, ldo, heads * 64, val)


def attn_temporal_split_exact(q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, *, B, T, Npix, heads, scale):
    """-> (float64 [B, Npix, heads, T, 64], rows [B, Npix, T])"""
    return _temporal_split(True, q, q_lo, ldq, k, k_lo, ldk, v, v_lo, ldv, B=B, T=T, Npix=Npix, heads=heads, scale=scale)


def softmax_rows(s32, lds, M, N, scale, p16, ldp, causal=False, n_valid=0):
    """The masks are predicates (a masked score is never a value: it may be NaN), and the row maximum is subtracted BEFORE the scaling,
    as the kernel's fma(s, sc, -max * sc) does in effect: scale * s rounded on its own loses |scale * s| 2^-24 of every exponent, which on
    scores with a large common offset (+1e4) is more than half the allowance of tests/misc_ref64.py, softmax_rows."""
    S = _mat(s32, M, N, lds).float()
    col, row = torch.arange(N, device=S.device)[None, :], torch.arange(M, device=S.device)[:, None]
    keep = col < (n_valid if n_valid > 0 else N)
    if causal:
        keep = keep & (col <= row)
    mx = S.masked_fill(~keep, float("-inf")).amax(dim=-1, keepdim=True)
    pr = torch.softmax(((S - mx) * scale).masked_fill(~keep, float("-inf")), dim=-1)
    _mat(p16, M, N, ldp).copy_(r16(pr, 'softmax_rows'))


def attn_temporal(q, ldq, k, ldk, v, ldv, o, ldo, *, B, T, Npix, heads, scale):
    Cc = heads * 64
    M = B * T * Npix

    def g(t, ld):
        return _mat(t, M, Cc, ld).float().view(B, T, Npix, heads, 64).permute(0, 2, 3, 1, 4)  # b p h t d
    s = torch.einsum("bphtd,bphsd->bphts", g(q, ldq), g(k, ldk)) * scale
    pr = torch.softmax(s, dim=-1)
    ov = torch.einsum("bphts,bphsd->bphtd", pr, g(v, ldv))
    _mat(o, M, Cc, ldo).copy_(r16(ov.permute(0, 3, 1, 2, 4).reshape(M, Cc), 'attn_temporal'))


# ---- norms (pnc_groupnorm_*, pnc_layernorm) ------------------------------------------------------------------------------------
def groupnorm_stats(x32, ldx, F, Npix, Cch, ppc, partial):
    nchunk = (Npix + ppc - 1) // ppc
    X = _mat(x32, F * Npix, Cch, ldx).view(F, Npix, 32, Cch // 32)
    P = partial.reshape(-1)[: F * nchunk * 32 * 3].view(F, nchunk, 32, 3)
    for c in range(nchunk):
        xs = X[:, c * ppc:(c + 1) * ppc].permute(0, 2, 1, 3).reshape(F, 32, -1)
        n = xs.shape[-1]
        mean = xs.mean(-1)
        P[:, c, :, 0] = n
        P[:, c, :, 1] = mean
        P[:, c, :, 2] = ((xs - mean[..., None]) ** 2).sum(-1)


def groupnorm_combine(parts_in, parts, F, nchunk, out):
    P = parts_in.reshape(-1)[: parts * F * nchunk * 96].view(parts, F, nchunk, 32, 3).double()
    P = P.permute(1, 0, 2, 3, 4).reshape(F, parts * nchunk, 32, 3)
    n = P[..., 0].sum(1)
    mean = (P[..., 0] * P[..., 1]).sum(1) / n
    m2 = (P[..., 2] + P[..., 0] * (P[..., 1] - mean[:, None]) ** 2).sum(1)
    O = out.reshape(-1)[: F * nchunk * 96].view(F, nchunk, 32, 3)
    O.zero_()
    O[:, 0] = torch.stack([n, mean, m2], dim=-1).to(O.dtype)


def groupnorm_apply(x32, ldx, F, Npix, Cch, ppc, partial, gamma, beta, eps, silu, y16, ldy, y16_lo=None, n_records=0):
    nchunk = n_records or (Npix + ppc - 1) // ppc
    P = partial.reshape(-1)[: F * nchunk * 32 * 3].view(F, nchunk, 32, 3).double()
    n = P[..., 0].sum(1)
    mean = (P[..., 0] * P[..., 1]).sum(1) / n
    m2 = (P[..., 2] + P[..., 0] * (P[..., 1] - mean[:, None]) ** 2).sum(1)
    rstd = 1.0 / torch.sqrt(m2 / n + eps)
    X = _mat(x32, F * Npix, Cch, ldx).view(F, Npix, 32, Cch // 32)
    y = (X - mean.float()[:, None, :, None]) * rstd.float()[:, None, :, None]
    y = y.reshape(F * Npix, Cch) * gamma.reshape(-1)[:Cch] + beta.reshape(-1)[:Cch]
    if silu:
        y = TF.silu(y)
    h = r16(y, 'groupnorm_apply')
    _mat(y16, F * Npix, Cch, ldy).copy_(h)
    if y16_lo is not None:
        _mat(y16_lo, F * Npix, Cch, ldy).copy_(_lo(y, h, y16_lo))


def groupnorm_temporal_part(x32, B, T, Npix, Cch, gamma, beta, eps, stats, mode, T_total, y16=None, y16_lo=None, t_pad=0):
    X = x32.reshape(-1)[: B * T * Npix * Cch].view(B, T, Npix, 32, Cch // 32).float()
    S = stats.reshape(-1)[: B * Npix * 64].view(B, Npix, 32, 2)
    if mode == 1:
        S[..., 0] = X.sum(dim=(1, 4))
        S[..., 1] = (X * X).sum(dim=(1, 4))
        return
    n = float((Cch // 32) * T_total)
    mean = S[..., 0].double() / n
    var = (S[..., 1].double() / n - mean * mean).clamp_min(0.0)
    rstd = (1.0 / torch.sqrt(var + eps)).float()
    y = (X - mean.float()[:, None, :, :, None]) * rstd[:, None, :, :, None]
    y = TF.silu(y.reshape(B, T, Npix, Cch) * gamma.reshape(-1)[:Cch] + beta.reshape(-1)[:Cch])
    h = r16(y, 'groupnorm_temporal')
    Y = y16.reshape(-1)[: B * (T + 2 * t_pad) * Npix * Cch].view(B, T + 2 * t_pad, Npix, Cch)
    Y[:, t_pad:t_pad + T] = h
    if y16_lo is not None:
        L = y16_lo.reshape(-1)[: B * (T + 2 * t_pad) * Npix * Cch].view(B, T + 2 * t_pad, Npix, Cch)
        L[:, t_pad:t_pad + T] = _lo(y, h, y16_lo)


def groupnorm_temporal_silu(x32, B, T, Npix, Cch, gamma, beta, eps, y16, y16_lo=None):
    X = x32.reshape(-1)[: B * T * Npix * Cch].view(B, T, Npix, Cch).permute(0, 2, 3, 1).reshape(B * Npix, Cch, T)
    y = TF.silu(TF.group_norm(X, 32, gamma.reshape(-1)[:Cch], beta.reshape(-1)[:Cch], eps))
    y = y.view(B, Npix, Cch, T).permute(0, 3, 1, 2).reshape(-1)
    h = r16(y, 'groupnorm_temporal')
    y16.reshape(-1)[: y.numel()].copy_(h)
    if y16_lo is not None:
        y16_lo.reshape(-1)[: y.numel()].copy_(_lo(y, h, y16_lo))


def layernorm(x32, ldx, M, Cch, gamma, beta, eps, y16, ldy, y16_lo=None):
    X = _mat(x32, M, Cch, ldx)
    y = TF.layer_norm(X, (Cch,), gamma.reshape(-1)[:Cch], beta.reshape(-1)[:Cch], eps)
    h = r16(y, 'layernorm')
    _mat(y16, M, Cch, ldy).copy_(h)
    if y16_lo is not None:
        _mat(y16_lo, M, Cch, ldy).copy_(_lo(y, h, y16_lo))


# ---- small-M linears (pnc_linear_smallm[_split], pnc_linear_smallm_segments[_split]) --------------------------------------------
# `w_lo`: the fp16 lo plane of split weights; the kernels join w = W + 2^-11 W_lo in fp32, so does `_join`.
def _smallm(a32, lda, w16, w_lo, bias, M, N, K, silu_in, silu_out):
    A = _mat(a32, M, K, lda)
    if silu_in:
        A = TF.silu(A)
    y = A @ _join(w16, w_lo).reshape(-1)[: N * K].view(N, K).t()
    if bias is not None:
        y = y + bias.reshape(-1)[:N]
    return TF.silu(y) if silu_out else y


def linear_smallm(a32, lda, w16, bias, out32, ldo, M, N, K, silu_in=False, silu_out=False, w_lo=None):
    _mat(out32, M, N, ldo).copy_(_smallm(a32, lda, w16, w_lo, bias, M, N, K, silu_in, silu_out))


def linear_smallm_segments(a32, lda, w16, bias, out32, M, m0, Mtot, N, K, seg_start, silu_in=False, silu_out=False, w_lo=None):
    y = _smallm(a32, lda, w16, w_lo, bias, M, N, K, silu_in, silu_out)
    flat = out32.reshape(-1)
    for s0, s1 in zip(seg_start[:-1], seg_start[1:]):
        flat[s0 * Mtot:s1 * Mtot].view(Mtot, s1 - s0)[m0:m0 + M].copy_(y[:, s0:s1])


# ---- embeddings and layout -----------------------------------------------------------------------------------------------------
def timestep_embedding(t_i64, F, dim, freqs, out32):
    args = t_i64.reshape(-1)[:F, None].float() * freqs.reshape(-1)[None, : dim // 2]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    o = out32.reshape(-1)[: F * dim].view(F, dim)
    o[:, : 2 * (dim // 2)].copy_(emb)
    o[:, 2 * (dim // 2):] = 0.0                     # the zero column of an odd dim, which the kernel writes


def timestep_embedding_f32(t_f32, F, dim, freqs, out32):
    """float timesteps (a continuous c_noise) as given: the int64 emulation's arithmetic after its `.float()`"""
    assert t_f32.dtype == torch.float32
    timestep_embedding(t_f32, F, dim, freqs, out32)


def nchw_to_tokens_f16(a32, C1, b32, C2, F, Npix, Cpad, out16, out16_lo=None, a_scale=None, a_frames=0):
    v = torch.zeros((F, Npix, Cpad), dtype=torch.float32, device=a32.device)
    af = a_frames or F
    a = a32.reshape(af, C1, Npix).float().repeat(F // af, 1, 1)
    if a_scale is not None:
        a = a * a_scale.reshape(F, 1, 1).float()
    v[:, :, :C1] = a.permute(0, 2, 1)
    if C2:
        v[:, :, C1:C1 + C2] = b32.reshape(F, C2, Npix).permute(0, 2, 1)
    h = r16(v, 'nchw_to_tokens')
    out16.reshape(-1)[: F * Npix * Cpad].view(F, Npix, Cpad).copy_(h)
    if out16_lo is not None:
        out16_lo.reshape(-1)[: F * Npix * Cpad].view(F, Npix, Cpad).copy_(_lo(v, h))


# ---- sampler exits (pnc_cfg_euler_step[_skip], pnc_cfg_sampler_step[_skip]) -----------------------------------------------------
# The reference's torch ops in the reference's order (denoiser.py:22-28, guiders.py:25-29, sampling.py:85-365) on channels-last eps
# tokens.  The HIP kernel is held to these BITS on the MI355X, per mode, entry, selector and aliased launch, in poisoned allocations
# (tests/test_sampler_exit_gpu.py against the per-op reference tests/sampler_exit_ref.py, which tests/test_sampler_exit_ref.py ties
# to this emulation bit for bit); the trajectories of tests/test_samplers_gpu.py / tests/test_denoisers_gpu.py sit on top of that.
def _denoised(eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, c_skip):
    """(X [T, C, Npix], guided D).  `c_skip` None: the eps path, D_h = E_h * c_out + X; else D_h = E_h * c_out + X * c_skip
    (denoiser.py:28) with both products and the sum rounded on their own.  Then CFG."""
    E = _mat(eps_tok, (2 if cfg else 1) * T * Npix, Cch, ld).view(-1, T, Npix, Cch).permute(0, 1, 3, 2)   # [halves, T, C, Npix]
    X = x.reshape(T, Cch, Npix)
    if c_skip is None:
        D = E * c_out.reshape(T, 1, 1) + X
    else:
        D = E * c_out.reshape(T, 1, 1) + X * c_skip.reshape(T, 1, 1)
    return X, (D[0] + scale * (D[1] - D[0]) if cfg else D[0])


def cfg_euler_step(eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, sigma, sigma_next, x_next, c_skip=None):
    """as the library: HEUN1 with v = {sigma, sigma_next} into x_next, no d kept"""
    _exit_step(SAMPLER_HEUN1, eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, [sigma, sigma_next], x_next, c_skip=c_skip)


def cfg_sampler_step(mode, eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, v, out, out_aux=None, x0=None, aux=None, hist=(),
                     noise=None, s_noise=1.0, c_skip=None):
    """`v` = the mode's per-frame [T] vectors in header order, `hist` = previous LMS d planes newest first"""
    if mode == SAMPLER_HEUN1 and out_aux is None:                   # PNC_EINVAL: only the Euler entries leave it out
        raise ValueError("HEUN1 without out_aux")
    _exit_step(mode, eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, v, out, out_aux, x0, aux, hist, noise, s_noise, c_skip)


def _exit_step(mode, eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, v, out, out_aux=None, x0=None, aux=None, hist=(), noise=None,
               s_noise=1.0, c_skip=None):
    """the one update behind both entries (the library's launch function)"""
    X, D = _denoised(eps_tok, ld, T, Npix, Cch, cfg, scale, x, c_out, c_skip)
    v = [t.reshape(T, 1, 1) for t in v]
    plane = lambda t: t.reshape(T, Cch, Npix)                       # noqa: E731
    if mode == SAMPLER_HEUN1:
        d = (X - D) / v[0]
        y = X + (v[1] - v[0]) * d
        if out_aux is not None:                                     # None: the Euler exit
            plane(out_aux).copy_(d)
    elif mode == SAMPLER_HEUN2:
        d_new = (X - D) / v[1]
        d_prime = (plane(aux) + d_new) / 2.0
        y = torch.where(v[1] > 0.0, plane(x0) + d_prime * (v[1] - v[0]), X)
    elif mode in (SAMPLER_EULER_A, SAMPLER_DPM2S_1):
        xe = X + (v[1] - v[0]) * ((X - D) / v[0])
        if mode == SAMPLER_DPM2S_1:
            y = v[2] * X - v[3] * D
            plane(out_aux).copy_(xe)
        else:
            y = torch.where(v[3] > 0.0, xe + plane(noise) * s_noise * v[2], xe)
    elif mode == SAMPLER_DPM2S_2:
        xs = torch.where(v[2] > 0.0, v[0] * plane(x0) - v[1] * D, plane(aux))
        y = torch.where(v[4] > 0.0, xs + plane(noise) * s_noise * v[3], xs)
    elif mode == SAMPLER_DPM2M:
        y = v[0] * X - v[1] * D
        if aux is not None:
            y = torch.where(v[4] > 0.0, v[0] * X - v[1] * (v[2] * D - v[3] * plane(aux)), y)
        plane(out_aux).copy_(D)
    elif mode == SAMPLER_LMS:
        d = (X - D) / v[0]
        acc = 0 + v[1] * d
        for k, h in enumerate(hist):
            acc = acc + v[2 + k] * plane(h)
        y = X + acc
        plane(out_aux).copy_(d)
    else:
        raise ValueError(f"mode {mode}")
    plane(out).copy_(y)


# ---- elementwise ---------------------------------------------------------------------------------------------------------------
def tokens_to_nchw_f32(x32, ld, F, Npix, Cch, out32):
    X = _mat(x32, F * Npix, Cch, ld).view(F, Npix, Cch)
    out32.reshape(-1)[: F * Cch * Npix].view(F, Cch, Npix).copy_(X.permute(0, 2, 1))


def concat_add(a32, C1, s32, c32, C2, M, out32, out16, out16_lo=None, gn_part=None, frames=0, ppc=64):
    a = a32.reshape(-1)[: M * C1].view(M, C1)
    s = s32.reshape(-1)[: M * C2].view(M, C2)
    if c32 is not None:
        s = s + c32.reshape(-1)[: M * C2].view(M, C2)
    y = torch.cat([a, s], dim=1)
    if out32 is not None:
        out32.reshape(-1)[: y.numel()].copy_(y.reshape(-1))
    if out16 is not None:
        h = r16(y.reshape(-1), 'concat_add')
        out16.reshape(-1)[: y.numel()].copy_(h)
        if out16_lo is not None:
            out16_lo.reshape(-1)[: y.numel()].copy_(_lo(y.reshape(-1), h, out16_lo))
    if gn_part is not None:       # pnc_concat_add_stats: the records pnc_groupnorm_stats writes for 64-pixel chunks
        assert frames >= 1 and M % frames == 0 and (C1 + C2) % 64 == 0
        groupnorm_stats(y.contiguous(), C1 + C2, frames, M // frames, C1 + C2, ppc, gn_part)


def add_f32(x32, a32, n, y32, y16, y16_lo=None):
    y = x32.reshape(-1)[:n]
    if a32 is not None:
        y = y + a32.reshape(-1)[:n]
    if y16 is not None:
        h = r16(y, 'add_f32')
        y16.reshape(-1)[:n].copy_(h)
        if y16_lo is not None:
            y16_lo.reshape(-1)[:n].copy_(_lo(y, h, y16_lo))
    if y32 is not None and (a32 is not None or y32.data_ptr() != x32.data_ptr()):
        y32.reshape(-1)[:n].copy_(y)


def range_monitor_collect(out_i32: torch.Tensor):
    """pnc_range_monitor_collect: adds the clamped-quad count since the previous call to out_i32[0] and resets it"""
    global _LO_CLAMPED
    out_i32[0] += _LO_CLAMPED
    _LO_CLAMPED = 0


# ---- operand range profile (pnc_operand_stats_f16), written from the header text with numpy ------------------------------------
# The GPU tests (tests/test_range_profile_gpu.py) compare the kernel's records with `record()` word for word (integers: exact).
#   rec[0..31]  elements per fp16 binade, index = (bits >> 10) & 31 of the hi plane
#   rec[32]     max of (bits & 0x7FFF)
#   rec[33]     lo elements at the end of their format: e4m3 (byte & 0x7F) >= 0x7E, fp16 non-finite; nothing without a lo plane
#   rec[34]     NaN elements of hi
#   rec[35]     elements counted
# Columns cols .. ld - 1 of a row are padding and never read.
STATS_WORDS = 36


def _plane(t: torch.Tensor, rows: int, cols: int, ld: int, np_dtype) -> np.ndarray:
    """the [rows, cols] elements of the plane whose element 0 is t's first one (row stride ld), reinterpreted as np_dtype"""
    flat = torch.as_strided(t, ((rows - 1) * ld + cols,), (1,)) if t.numel() else t.reshape(-1)
    a = flat.detach().cpu().contiguous().numpy().view(np_dtype)
    return np.lib.stride_tricks.as_strided(a, (rows, cols), (ld * a.itemsize, a.itemsize))


def record(hi: torch.Tensor, lo, rows: int, cols: int, ld: int) -> np.ndarray:
    """the 36 words one launch ADDS (word 32: the value the launch maxes in), as int64"""
    if hi.dtype != torch.float16 or rows < 1 or cols < 1 or ld < cols:
        raise ValueError("PNC_EINVAL")
    if cols % 8 or ld % 8:
        raise ValueError("PNC_EALIGN")
    bits = _plane(hi, rows, cols, ld, np.uint16).astype(np.int64)
    a = bits & 0x7FFF
    rec = np.zeros(STATS_WORDS, dtype=np.int64)
    rec[:32] = np.bincount((a >> 10).reshape(-1), minlength=32)
    rec[32] = a.max()
    rec[34] = int((a > 0x7C00).sum())
    rec[35] = rows * cols
    if lo is not None:
        if lo.dtype == torch.uint8:
            b = _plane(lo, rows, cols, ld, np.uint8).astype(np.int64)
            rec[33] = int(((b & 0x7F) >= 0x7E).sum())
        elif lo.dtype == torch.float16:
            b = _plane(lo, rows, cols, ld, np.uint16).astype(np.int64)
            rec[33] = int(((b & 0x7C00) == 0x7C00).sum())
        else:
            raise ValueError("PNC_EINVAL")
    return rec


def accumulate(rec: torch.Tensor, add: np.ndarray):
    """what the kernel's atomics do to a record"""
    r = rec.reshape(-1)
    new = r[:STATS_WORDS].cpu().numpy() + add
    new[32] = max(int(r[32]), int(add[32]))
    r[:STATS_WORDS] = torch.from_numpy(new).to(r.device)


def operand_stats(hi, lo, rows, cols, ld, rec):
    assert rec.dtype == torch.int64 and rec.numel() >= STATS_WORDS and rec.is_contiguous()
    accumulate(rec, record(hi, lo, rows, cols, ld))


def cast_f16(x32, n, y16, y16_lo=None):
    add_f32(x32, None, n, None, y16, y16_lo)
