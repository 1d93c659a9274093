"""Split weights on the MI355X (PncGemmParams.W_lo next to an fp16 A_lo; the `precise-full` operand policy).

Kernel level: pnc_gemm_f16 with all four planes fp16 at |a|, |w| up to ~1e3 against the float64 value of
(A_hi + 2^-11 A_lo) (W_hi + 2^-11 W_lo), on the smallest shapes that reach each code path.  The tolerance is not a fixed number:
on each shape the EXISTING path (the same launch with W_lo = NULL) is measured against the float64 value of
(A_hi + 2^-11 A_lo) W_hi, and the new launch may err by at most twice that plus the analytic size of the dropped term,
2^-22 sum |a_lo| |w_lo|.  Both figures are printed and appended to the measurement log (helpers.measured).

End to end: the `tiny` network on weights that are not fp16-representable against tests/golden/tiny_w32.npz."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from helpers import cond, err_stats, golden, manifest, measured, product_network, step_inputs
from panacea_amd import hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
S = 1.0 / 2048.0


def _split(v64):
    hi = v64.half()
    return hi, ((v64 - hi.double()) * 2048.0).half()


def _planes(shape, gen, mag=300.0):
    """fp16 (hi, lo) planes of randn * mag: |v| up to ~1e3, |lo| up to 512"""
    return _split(torch.randn(*shape, generator=gen, dtype=torch.float64) * mag)


def _contract64(A, W, M, N, K, a_mode, conv, tconv):
    """float64 gatherA[M, K] @ W[N, K]^T in the K orders of include/panacea_hip.h (A: the flat plane, W: [N, K])"""
    if a_mode == hip.A_PLAIN:
        return A.reshape(M, K) @ W.t()
    if a_mode == hip.A_CONV3X3:
        Cin, Hin, Win, Hout, Wout = conv["Cin"], conv["Hin"], conv["Win"], conv["Hout"], conv["Wout"]
        Fr = M // (Hout * Wout)
        x = A.reshape(Fr, Hin, Win, Cin).permute(0, 3, 1, 2)
        if conv.get("upsample", 0):
            x = TF.interpolate(x, scale_factor=2, mode="nearest")
        if Cin % 64 == 0:
            w = W.view(N, Cin // 64, 3, 3, 64).permute(0, 1, 4, 2, 3).reshape(N, Cin, 3, 3)
        else:
            w = W.view(N, 3, 3, Cin).permute(0, 3, 1, 2)
        y = TF.conv2d(x, w, stride=conv.get("stride", 1), padding=1)
        assert y.shape[2:] == (Hout, Wout)
        return y.permute(0, 2, 3, 1).reshape(M, N)
    Cc, T, Npix = tconv["C"], tconv["T"], tconv["Npix"]
    halo = int(tconv.get("halo", 0))
    B, Ta = M // (T * Npix), T + 2 * halo
    x = A.reshape(B, Ta, Npix, Cc).permute(0, 2, 3, 1).reshape(B * Npix, Cc, Ta)
    w = W.view(N, Cc // 64, 3, 64).permute(0, 1, 3, 2).reshape(N, Cc, 3) if Cc % 64 == 0 else W.view(N, 3, Cc).permute(0, 2, 1)
    y = TF.conv1d(x, w, padding=0 if halo else 1)
    return y.view(B, Npix, N, T).permute(0, 3, 1, 2).reshape(M, N)


def _launch(ah, al, wh, wl, M, N, K, **kw):
    out = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float32)
    hip.gemm(ah, wh, M=M, N=N, K=K, a16_lo=al, w_lo=wl, out32=out, ldc32=N, **kw)
    torch.cuda.synchronize()
    return out


def _case(name, a_shape, M, N, K, seed=0, **kw):
    """-> (old launch, new launch) after the checks every shape gets: the float64 bound and the all-zero W_lo identity"""
    g = torch.Generator().manual_seed(seed)
    ah, al = _planes(a_shape, g)
    wh, wl = _planes((N, K), g)
    a_mode, conv, tconv = kw.get("a_mode", hip.A_PLAIN), kw.get("conv"), kw.get("tconv")
    a64 = ah.double() + al.double() * S
    ref_old = _contract64(a64, wh.double(), M, N, K, a_mode, conv, tconv)
    ref_new = _contract64(a64, wh.double() + wl.double() * S, M, N, K, a_mode, conv, tconv)
    dropped = (_contract64(al.double().abs(), wl.double().abs(), M, N, K, a_mode, conv, tconv) * S * S).max().item()
    d = [t.to(DEV) for t in (ah, al, wh, wl)]
    if a_mode == hip.A_PLAIN:
        kw.setdefault("lda", K)
    old = _launch(d[0], d[1], d[2], None, M, N, K, **kw)
    new = _launch(d[0], d[1], d[2], d[3], M, N, K, **kw)
    zero = _launch(d[0], d[1], d[2], torch.zeros_like(d[3]), M, N, K, **kw)
    e_old = (old.double().cpu() - ref_old).abs().max().item()
    e_new = (new.double().cpu() - ref_new).abs().max().item()
    term = (ref_new - ref_old).abs().max().item()
    print(f"{name}: existing path {e_old:.3e}  with W_lo {e_new:.3e}  (dropped term <= {dropped:.3e}; the W_lo term itself {term:.3e}; "
          f"|C| max {ref_new.abs().max().item():.3e})")
    measured("precise_full_kernel", case=name.replace(" ", "_"), existing=e_old, with_wlo=e_new, dropped=dropped, wlo_term=term)
    assert torch.isfinite(new).all()
    assert term > 10 * (2 * e_old + dropped), "the operands do not make a mishandled W_lo visible"
    assert e_new <= 2 * e_old + dropped, (name, e_new, e_old, dropped)
    assert torch.equal(zero, old), "an all-zero W_lo plane must not change a bit"
    return old, new


def test_plain_ragged_everything():
    _case("plain M200 N72 K136", (200, 136), 200, 72, 136)


def test_plain_single_k_tile():
    _case("plain K64", (200, 64), 200, 72, 64, seed=1)        # the lo pass is exactly two tiles


def _k_slices(M, N, K):
    """K slices the library runs for this problem: its workspace request in units of M x N floats (0 -> one slice)"""
    import ctypes
    p = hip.GemmParams()
    p.struct_bytes = ctypes.sizeof(hip.GemmParams)
    p.M, p.N, p.K = M, N, K
    return max(1, hip.load().pnc_gemm_workspace_floats(ctypes.byref(p)) // (M * N))


@pytest.mark.parametrize("N", [64, 256])
def test_plain_at_the_split_k_threshold(N):
    """K = 3584 = 56 K tiles (4 slices from there on).  N = 64 is the shape as specified — the library splits only where N % 256 == 0, so
    that launch runs unsplit either way and the comparison is bitwise; N = 256 is the smallest shape that does split: its slices sum
    the same products in another order, so both launches are held to the float64 bound (in _case).  The split decision itself is
    read from the library."""
    M, K = 64, 3584
    assert _k_slices(M, N, K) == (1 if N == 64 else 4)
    old, new = _case(f"plain split-K N{N}", (M, K), M, N, K, seed=2)
    prev = hip.set_option(hip.OPT_GEMM_TILE, 4)                # a forced tile (256x256, the split launch's own) disables split K
    try:
        old1, new1 = _case(f"plain unsplit N{N}", (M, K), M, N, K, seed=2)
    finally:
        hip.set_option(hip.OPT_GEMM_TILE, prev)
    if N == 64:
        assert torch.equal(new, new1) and torch.equal(old, old1)


@pytest.mark.parametrize("Cin", [64, 8])
@pytest.mark.parametrize("mode", ["stride1", "stride2", "upsample"])
def test_conv3x3_gather(Cin, mode):
    F, Hin, Win, N = 2, 8, 12, 72
    stride, up = (2 if mode == "stride2" else 1), mode == "upsample"
    Hout, Wout = (2 * Hin, 2 * Win) if up else ((Hin - 1) // stride + 1, (Win - 1) // stride + 1)
    M, K = F * Hout * Wout, 9 * Cin
    _case(f"conv3x3 Cin{Cin} {mode}", (F * Hin * Win, Cin), M, N, K, seed=3, a_mode=hip.A_CONV3X3,
          conv=dict(Cin=Cin, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, stride=stride, upsample=int(up)))


def test_stencil_tile_kernel():
    """one frame of 16 x 32 pixels = two 16x16 spatial tiles, N = 264 = one full 256-column tile + a ragged one of 8 columns, C = 64;
    the tile kernel (PNC_OPT_STENCIL_TILES = 2: wherever the shape allows) must give the per-tap kernel's bits"""
    F, H, W, C, N = 1, 16, 32, 64, 264
    M, K = F * H * W, 9 * C
    kw = dict(a_mode=hip.A_CONV3X3, conv=dict(Cin=C, Hin=H, Win=W, Hout=H, Wout=W, stride=1, upsample=0))
    prev = hip.set_option(hip.OPT_STENCIL_TILES, 2)
    try:
        old_t, new_t = _case("stencil tile", (M, C), M, N, K, seed=4, **kw)
        hip.set_option(hip.OPT_STENCIL_TILES, 0)
        old_g, new_g = _case("per-tap, same shape", (M, C), M, N, K, seed=4, **kw)
    finally:
        hip.set_option(hip.OPT_STENCIL_TILES, prev)
    assert torch.equal(old_t, old_g) and torch.equal(new_t, new_g)


@pytest.mark.parametrize("T", [3, 8])
@pytest.mark.parametrize("halo", [0, 1])
def test_conv1d_temporal(T, halo):
    B, Npix, C, N = 2, 32, 64, 64
    M, K = B * T * Npix, 3 * C
    _case(f"conv1d T{T} halo{halo}", (B * (T + 2 * halo) * Npix, C), M, N, K, seed=5, a_mode=hip.A_CONV1D_T,
          tconv=dict(C=C, T=T, Npix=Npix, halo=halo))


def test_refusals():
    g = torch.Generator().manual_seed(6)
    M, N, K = 64, 64, 64
    ah, al = (t.to(DEV) for t in _planes((M, K), g))
    wh, wl = (t.to(DEV) for t in _planes((N, K), g))
    out = torch.empty((M, N), device=DEV, dtype=torch.float32)
    with pytest.raises(hip.PncError, match="PNC_EINVAL"):          # W_lo without A_lo
        hip.gemm(ah, wh, M=M, N=N, K=K, lda=K, w_lo=wl, out32=out, ldc32=N)
    off = torch.empty(N * K + 8, device=DEV, dtype=torch.float16)[4:4 + N * K].view(N, K)      # 8 bytes off a 16-byte boundary
    with pytest.raises(hip.PncError, match="PNC_EALIGN"):
        hip.gemm(ah, wh, M=M, N=N, K=K, lda=K, a16_lo=al, w_lo=off, out32=out, ldc32=N)
    # next to an e4m3 A_lo, W_lo keeps its e4m3 meaning: the binding refuses an fp16 plane in its place (what the library does with a
    # real e4m3 pair on a shape of the tile kernel: test_e4m3_pair_on_a_tile_shape_runs_the_per_tap_kernel)
    with pytest.raises(hip.PncError):
        hip.gemm(ah, wh, M=M, N=N, K=K, lda=K, a16_lo=torch.zeros((M, K), device=DEV, dtype=torch.uint8), w_lo=wl, out32=out, ldc32=N)
    assert hip.ABI_VERSION == 8


def test_e4m3_pair_on_a_tile_shape_runs_the_per_tap_kernel():
    """Next to an e4m3 A_lo, W_lo keeps its e4m3 meaning, and the halo-tile kernel — which has no e4m3 pass — is not selected even
    where the shape allows it and PNC_OPT_STENCIL_TILES = 2 asks for it: the launch gives the per-tap kernel's bits, and they are
    the e4m3 pair's product.  Bound: the worst case of an fp32 sum of K terms, K 2^-24 max sum |a| |w| (the products themselves are
    exact in fp32)."""
    from panacea_amd import engine as E
    g = torch.Generator().manual_seed(7)
    F, H, W, C, N = 1, 16, 32, 64, 264
    M, K = F * H * W, 9 * C
    a64 = torch.randn(M, C, generator=g, dtype=torch.float64)
    ah = a64.half()
    al8 = ((a64 - ah.double()) * 2048.0).float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
    wh = (torch.randn(N, K, generator=g, dtype=torch.float64) / K ** 0.5).half()
    w8, e8 = E.pk_lo8(wh)
    conv = dict(Cin=C, Hin=H, Win=W, Hout=H, Wout=W, stride=1, upsample=0)
    w8_64 = w8.view(torch.float8_e4m3fn).double() * 2.0 ** (e8 - 127)
    ref = (_contract64(ah.double(), wh.double(), M, N, K, hip.A_CONV3X3, conv, None)
           + _contract64(al8.double(), w8_64, M, N, K, hip.A_CONV3X3, conv, None) * S)
    bound = K * 2.0 ** -24 * _contract64(ah.double().abs() + al8.double().abs() * S, wh.double().abs(), M, N, K, hip.A_CONV3X3, conv,
                                         None).max().item()
    d = dict(a=ah.to(DEV), al=al8.view(torch.uint8).to(DEV), w=wh.to(DEV), w8=w8.to(DEV))
    outs = []
    prev = hip.set_option(hip.OPT_STENCIL_TILES, 2)
    try:
        for opt in (2, 0):
            hip.set_option(hip.OPT_STENCIL_TILES, opt)
            outs.append(_launch(d["a"], d["al"], d["w"], (d["w8"], e8), M, N, K, a_mode=hip.A_CONV3X3, conv=conv))
    finally:
        hip.set_option(hip.OPT_STENCIL_TILES, prev)
    err = (outs[0].double().cpu() - ref).abs().max().item()
    print(f"e4m3 pair on a tile shape: {err:.3e} against float64 (bound {bound:.3e})")
    measured("precise_full_kernel", case="e4m3_pair_tile_shape", err=err, bound=bound)
    assert torch.equal(outs[0], outs[1])
    assert err <= bound


def test_small_m_linears_join_the_pair_in_fp32():
    g = torch.Generator().manual_seed(8)
    M, N, K = 16, 72, 320
    a = torch.randn(M, K, generator=g)
    w64 = torch.randn(N, K, generator=g, dtype=torch.float64) / K ** 0.5
    wh, wl = _split(w64)
    bias = torch.randn(N, generator=g)
    ref = a.double() @ (wh.double() + wl.double() * S).t() + bias.double()
    d = [t.to(DEV) for t in (a, wh, wl, bias)]
    o_new, o_old, o_seg = (torch.empty((M, N), device=DEV) for _ in range(3))
    hip.linear_smallm(d[0], K, d[1], d[3], o_new, N, M, N, K, w_lo=d[2])
    hip.linear_smallm(d[0], K, d[1], d[3], o_old, N, M, N, K)
    hip.linear_smallm_segments(d[0], K, d[1], d[3], o_seg, M, 0, M, N, K, [0, 32, N], w_lo=d[2])
    torch.cuda.synchronize()
    e_new = (o_new.double().cpu() - ref).abs().max().item()
    e_old = (o_old.double().cpu() - ref).abs().max().item()
    print(f"linear_smallm: pair {e_new:.3e}  single fp16 weights {e_old:.3e}")
    # fp32 accumulation of K = 320 products with sum |a w| ~ 11: K^1/2 * 2^-24 * 11 ~ 1e-5 at the outside; single fp16 weights err
    # by 2^-12 per product, ~1e-4
    assert e_new <= 1e-5 and e_old >= 10 * e_new
    seg = torch.cat([o_seg.view(-1)[:M * 32].view(M, 32), o_seg.view(-1)[M * 32:].view(M, N - 32)], dim=1)
    assert torch.equal(seg, o_new)


# ---- end to end: the tiny network on weights that are not fp16-representable
def _tiny_w32(prec):
    w, _, kw = product_network("tiny", "cpu")
    w.diffusion_model.load_state_dict(synth.synth_state_dict(manifest("tiny"), round_fp16=False), strict=True)
    w = w.to(DEV)
    w.diffusion_model.precision = prec
    return w, kw, step_inputs("tiny", kw, DEV)


def test_tiny_network_on_unrounded_weights():
    ref = golden("tiny_w32")["eps"]
    errs = {}
    for p in ("precise-wide", "precise-full"):
        w, kw, inp = _tiny_w32(p)
        eps = w(inp["x"], inp["t"], cond(inp))
        torch.cuda.synchronize()
        errs[p] = err_stats(eps, ref)
        measured("precise_full_tiny_w32", prec=p, max_abs=errs[p]["max_abs"], mean_abs=errs[p]["mean_abs"])
    print("tiny, unrounded weights vs tiny_w32:", errs)
    assert errs["precise-full"]["max_abs"] <= 1e-3, errs
    assert errs["precise-wide"]["max_abs"] >= 2 * errs["precise-full"]["max_abs"], errs
    assert "libpanacea_hip.so" in open("/proc/self/maps").read()


def test_representable_weights_give_the_precise_wide_bits():
    """fp16-representable weights: every W_lo plane is zero and `precise-full` is `precise-wide` bit for bit"""
    w, _, kw = product_network("tiny", DEV)
    inp = step_inputs("tiny", kw, DEV)
    m = w.diffusion_model
    m.precision = "precise-wide"
    wide = w(inp["x"], inp["t"], cond(inp))
    m.precision = "precise-full"
    full = w(inp["x"], inp["t"], cond(inp))
    torch.cuda.synchronize()
    assert all(not bool(t.any()) for mod in m.modules() if getattr(mod, "_pk_lo", None)
               for t in mod._pk_lo.values() if isinstance(t, torch.Tensor) and t.dtype == torch.float16)
    assert torch.equal(full, wide)


def test_plain_hoisted_and_graphed_steps_are_bit_identical():
    from panacea_amd import sampling as Smp
    from panacea_amd.graph import GraphedStep
    w, kw, inp = _tiny_w32("precise-full")
    T = kw["num_frames"]
    c = {"crossattn": inp["crossattn"][1:2], "concat": inp["concat"][T:], "cond_feat": inp["cond_feat"][T:]}
    uc = {"crossattn": inp["crossattn"][0:1], "concat": inp["concat"][:T], "cond_feat": inp["cond_feat"][:T]}
    den = Smp.DiscreteDenoiser().to(DEV)
    smp = Smp.EulerEDMSampler(3, guider=Smp.VanillaCFG(5.0), device=DEV)
    sig = smp.sigmas()
    s_in = inp["x"].new_ones([T])
    x0 = inp["x"][T:] * 14.6
    bd = Smp.BoundDenoiser(den, w)
    with torch.no_grad():
        step = lambda xi, s0, s1: smp.sampler_step(s0, s1, lambda a, b, cc: den(w, a, b, cc), xi, c, uc)   # noqa: E731
        e0 = step(x0, s_in * sig[0], s_in * sig[1])
        e1 = step(e0, s_in * sig[1], s_in * sig[2])
        c2, u2 = Smp.hoist_invariants(w, smp.guider, c, uc)
        assert smp._fusable(bd, x0, c2)
        fstep = lambda xi, s0, s1: smp.sampler_step(s0, s1, bd, xi, c2, u2)   # noqa: E731      (fused + hoisted)
        f0 = fstep(x0, s_in * sig[0], s_in * sig[1])
        f1 = fstep(f0, s_in * sig[1], s_in * sig[2])
        gr = GraphedStep(fstep, x0, s_in * sig[0], s_in * sig[1])
        g0 = gr(x0, s_in * sig[0], s_in * sig[1]).clone()
        g1 = gr(g0, s_in * sig[1], s_in * sig[2]).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(e1).all() and (e1 - e0).abs().max().item() > 1e-3
    assert torch.equal(f0, e0) and torch.equal(f1, e1)
    assert torch.equal(g0, e0) and torch.equal(g1, e1)
