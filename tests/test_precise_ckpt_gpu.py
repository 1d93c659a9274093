"""Split weights BESIDE the launch on the MI355X (pnc_gemm_wsplit_f16; the `precise-ckpt` operand policy).

Kernel level, one test per kernel form on the smallest shapes that reach each code path: the launch against the float64 product of
the planes actually passed,
    A_hi W_hi + 2^-11 (A_lo8 W_8 [with an e4m3 A_lo: the e4m3 copy of W the lo pass reads] + A_hi W_lo16).
The tolerance is not a fixed number: on each shape the EXISTING launch (pnc_gemm_f16, no weight plane) is measured against the float64
value of its own operands, and the new launch may err by at most twice that.  No term is dropped against this reference (the A_lo W_lo
product does not exist in it), so nothing is added to the bound.  With W_lo16 all zero every launch must give the existing launch's
bits.  Both figures are printed and appended to the measurement log (helpers.measured).

End to end: the `tiny` network on weights that are not fp16-representable against tests/golden/tiny_w32.npz."""
import ctypes

import pytest
import torch
import torch.nn.functional as TF

from helpers import cond, err_stats, golden, manifest, measured, product_network, step_inputs
from panacea_amd import engine as E, hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
S = 1.0 / 2048.0


def _split(v64):
    hi = v64.half()
    return hi, ((v64 - hi.double()) * 2048.0).half()


def _contract64(A, W, M, N, K, a_mode, conv, tconv):
    """float64 gatherA[M, K] @ W[N, K]^T in the K orders of include/panacea_hip.h (A: the flat plane, W: [N, K]), on A's device"""
    if a_mode == hip.A_PLAIN:
        return A.reshape(M, K) @ W.t()
    if a_mode == hip.A_CONV3X3:
        Cin, Hin, Win, Hout, Wout = conv["Cin"], conv["Hin"], conv["Win"], conv["Hout"], conv["Wout"]
        Fr = M // (Hout * Wout)
        x = A.reshape(Fr, Hin, Win, Cin).permute(0, 3, 1, 2)
        if conv.get("upsample", 0):
            x = TF.interpolate(x, scale_factor=2, mode="nearest")
        w = W.view(N, Cin // 64, 3, 3, 64).permute(0, 1, 4, 2, 3).reshape(N, Cin, 3, 3)       # (Cin % 64 == 0 here)
        y = TF.conv2d(x, w, stride=conv.get("stride", 1), padding=1)
        assert y.shape[2:] == (Hout, Wout)
        return y.permute(0, 2, 3, 1).reshape(M, N)
    Cc, T, Npix = tconv["C"], tconv["T"], tconv["Npix"]
    halo = int(tconv.get("halo", 0))
    B, Ta = M // (T * Npix), T + 2 * halo
    x = A.reshape(B, Ta, Npix, Cc).permute(0, 2, 3, 1).reshape(B * Npix, Cc, Ta)
    w = W.view(N, Cc // 64, 3, 64).permute(0, 1, 3, 2).reshape(N, Cc, 3)
    y = TF.conv1d(x, w, padding=0 if halo else 1)
    return y.view(B, Npix, N, T).permute(0, 3, 1, 2).reshape(M, N)


def _geglu64(c):
    """value * gelu_erf(gate) on interleaved 32-column blocks (include/panacea_hip.h), float64"""
    M, N = c.shape
    c = c.view(M, N // 64, 2, 32)
    v, g = c[:, :, 0], c[:, :, 1]
    return (v * 0.5 * g * (1.0 + torch.erf(g * 0.70710678118654752440))).reshape(M, N // 2)


def _case(name, a_shape, M, N, K, seed=0, a8=False, geglu=False, ref_dev="cpu", **kw):
    """-> (existing launch, launch with the plane) after the checks every form gets: the float64 bound and the all-zero identity.
    a8: A carries an e4m3 lo plane (values of order 1: inside its range); otherwise |a|, |w| up to ~1e3 as in test_precise_full_gpu."""
    g = torch.Generator().manual_seed(seed)
    mag = 1.0 if (a8 or geglu) else 300.0
    a64 = torch.randn(*a_shape, generator=g, dtype=torch.float64) * mag
    ah = a64.half()
    wh, wl = _split(torch.randn(N, K, generator=g, dtype=torch.float64) * (mag if not geglu else K ** -0.5))
    if geglu:
        # the fp16 output rounds at 2^-11 of a value, the lo twin of a real weight moves it by 2^-12: a plane of the twin's format but
        # 5 % of the weights' size makes a mishandled plane visible all the same (the planes are operands like any other)
        wl = (torch.randn(N, K, generator=g, dtype=torch.float64) * (0.05 * 2048.0 * K ** -0.5)).half()
    a_mode, conv, tconv = kw.get("a_mode", hip.A_PLAIN), kw.get("conv"), kw.get("tconv")
    r = torch.device(ref_dev)
    c64 = lambda A, W: _contract64(A.to(r).double(), W.to(r).double(), M, N, K, a_mode, conv, tconv)      # noqa: E731
    ref_old = c64(ah, wh)
    al = w8 = None
    if a8:
        al8 = ((a64 - ah.double()) * 2048.0).float().clamp(-448.0, 448.0).to(torch.float8_e4m3fn)
        w8b, e8 = E.pk_lo8(wh)
        ref_old = ref_old + c64(al8.float(), w8b.view(torch.float8_e4m3fn).double() * 2.0 ** (e8 - 127)) * S
        al, w8 = al8.view(torch.uint8).to(DEV), (w8b.to(DEV), e8)
    ref_new = ref_old + c64(ah, wl) * S
    if geglu:
        ref_old, ref_new = _geglu64(ref_old), _geglu64(ref_new)
    d = [t.to(DEV) for t in (ah, wh, wl)]
    if a_mode == hip.A_PLAIN:
        kw.setdefault("lda", K)

    def launch(plane):
        if geglu:
            out = torch.full((M, N // 2), float("nan"), device=DEV, dtype=torch.float16)
            okw = dict(out16=out, ldc16=N // 2, geglu=True)
        else:
            out = torch.full((M, N), float("nan"), device=DEV, dtype=torch.float32)
            okw = dict(out32=out, ldc32=N)
        hip.gemm(d[0], d[1], M=M, N=N, K=K, a16_lo=al, w_lo=w8, w_lo16=plane, **okw, **kw)
        torch.cuda.synchronize()
        return out
    old, new, zero = launch(None), launch(d[2]), launch(torch.zeros_like(d[2]))
    e_old = (old.to(r).double() - ref_old).abs().max().item()
    e_new = (new.to(r).double() - ref_new).abs().max().item()
    term = (ref_new - ref_old).abs().max().item()
    print(f"{name}: existing launch {e_old:.3e}  with W_lo16 {e_new:.3e}  (the W_lo16 term itself {term:.3e}; "
          f"|C| max {ref_new.abs().max().item():.3e})")
    measured("precise_ckpt_kernel", case=name.replace(" ", "_"), existing=e_old, with_wlo16=e_new, wlo_term=term)
    assert torch.isfinite(new).all()
    assert term > 10 * 2 * e_old, "the operands do not make a mishandled W_lo16 visible"
    assert e_new <= 2 * e_old, (name, e_new, e_old)
    assert torch.equal(zero, old), "an all-zero W_lo16 plane must not change a bit"
    return old, new


def test_plain_ragged_everything():
    _case("plain M200 N72 K136", (200, 136), 200, 72, 136)


def test_plain_single_k_tile():
    _case("plain K64", (200, 64), 200, 72, 64, seed=1)


def _k_slices(M, N, K):
    p = hip.GemmParams()
    p.struct_bytes = ctypes.sizeof(hip.GemmParams)
    p.M, p.N, p.K = M, N, K
    return max(1, hip.load().pnc_gemm_workspace_floats(ctypes.byref(p)) // (M * N))


@pytest.mark.parametrize("N", [64, 256])
def test_plain_at_the_split_k_threshold(N):
    """K = 3584 = 56 K tiles (4 slices from there on).  N = 64 is the shape as specified: the library splits only where N % 256 == 0, so
    it runs unsplit; N = 256 is the smallest shape that does split — every slice runs its own K range in the weight part too."""
    M, K = 64, 3584
    assert _k_slices(M, N, K) == (1 if N == 64 else 4)
    _case(f"plain split-K threshold N{N}", (M, K), M, N, K, seed=2)


@pytest.mark.parametrize("N", [72, 320])
def test_plain_with_an_e4m3_a_lo(N):
    """K = 320 = 2.5 e4m3 tiles, 5 fp16 tiles: weight part, scaling, e4m3 lo tiles, hi pass (N = 320: the 256x320 geometry)"""
    _case(f"plain e4m3 A_lo K320 N{N}", (200, 320), 200, N, 320, seed=3, a8=True)


@pytest.mark.parametrize("a8", [False, True])
@pytest.mark.parametrize("mode", ["stride1", "stride2", "upsample"])
def test_conv3x3_gather(mode, a8):
    F, Hin, Win, Cin, N = 2, 8, 16, 64, 72
    stride, up = (2 if mode == "stride2" else 1), mode == "upsample"
    Hout, Wout = (2 * Hin, 2 * Win) if up else ((Hin - 1) // stride + 1, (Win - 1) // stride + 1)
    M, K = F * Hout * Wout, 9 * Cin
    _case(f"conv3x3 {mode} a8={int(a8)}", (F * Hin * Win, Cin), M, N, K, seed=4, a8=a8, a_mode=hip.A_CONV3X3,
          conv=dict(Cin=Cin, Hin=Hin, Win=Win, Hout=Hout, Wout=Wout, stride=stride, upsample=int(up)))


@pytest.mark.parametrize("T", [3, 8])
@pytest.mark.parametrize("halo", [0, 1])
def test_conv1d_temporal(T, halo):
    B, Npix, C, N = 2, 32, 64, 64
    M, K = B * T * Npix, 3 * C
    _case(f"conv1d T{T} halo{halo}", (B * (T + 2 * halo) * Npix, C), M, N, K, seed=5, a8=(T == 8), a_mode=hip.A_CONV1D_T,
          tconv=dict(C=C, T=T, Npix=Npix, halo=halo))


def test_stencil_tile_kernel():
    """one frame of 16 x 32 pixels = two 16x16 spatial tiles, N = 264 = one full 256-column tile + a ragged one of 8 columns, C = 64;
    the tile kernel (PNC_OPT_STENCIL_TILES = 2: wherever the shape allows) must give the per-tap kernel's bits"""
    F, H, W, C, N = 1, 16, 32, 64, 264
    M, K = F * H * W, 9 * C
    kw = dict(a_mode=hip.A_CONV3X3, conv=dict(Cin=C, Hin=H, Win=W, Hout=H, Wout=W, stride=1, upsample=0))
    prev = hip.set_option(hip.OPT_STENCIL_TILES, 2)
    try:
        old_t, new_t = _case("stencil tile", (M, C), M, N, K, seed=6, **kw)
        hip.set_option(hip.OPT_STENCIL_TILES, 0)
        old_g, new_g = _case("per-tap, same shape", (M, C), M, N, K, seed=6, **kw)
    finally:
        hip.set_option(hip.OPT_STENCIL_TILES, prev)
    assert torch.equal(old_t, old_g) and torch.equal(new_t, new_g)


@pytest.mark.parametrize("a8", [False, True])
def test_smallest_shape_of_the_persistent_plain_kernel(a8):
    """131072 x 320 x 64 = 512 full 256x320 tiles: pnc_gemm_f16 runs the persistent plain-A kernel, which has no weight part — the launch
    with the plane runs one tile per workgroup on the same tiles and must give the persistent kernel's bits for a zero plane"""
    M, N, K = 131072, 320, 64
    _case(f"persistent plain a8={int(a8)}", (M, K), M, N, K, seed=7, a8=a8, ref_dev="cuda")


@pytest.mark.parametrize("K", [64, 128])
def test_smallest_shape_of_the_persistent_geglu_kernel(K):
    """32768 x 1024 = 512 full 256x256 tiles.  The persistent GEGLU kernel has the weight part: K = 64 is one K tile per part; K = 128
    makes the launch with the plane four virtual K tiles, where its staggered schedule starts (PNC_OPT_GEMM_STAGGER = 4) while the
    existing launch's two tiles run the plain loop — the zero plane must give the same bits all the same"""
    M, N = 32768, 1024
    _case(f"persistent GEGLU K{K}", (M, K), M, N, K, seed=8, geglu=True, ref_dev="cuda")


def test_refusals_and_the_forwarded_fp16_a_lo():
    g = torch.Generator().manual_seed(9)
    M, N, K = 64, 64, 64
    ah, al = (t.to(DEV) for t in _split(torch.randn(M, K, generator=g, dtype=torch.float64) * 300))
    wh, wl = (t.to(DEV) for t in _split(torch.randn(N, K, generator=g, dtype=torch.float64) * 300))
    out = torch.empty((M, N), device=DEV, dtype=torch.float32)
    off = torch.empty(N * K + 8, device=DEV, dtype=torch.float16)[4:4 + N * K].view(N, K)      # 8 bytes off a 16-byte boundary
    with pytest.raises(hip.PncError, match="PNC_EALIGN"):
        hip.gemm(ah, wh, M=M, N=N, K=K, lda=K, w_lo16=off, out32=out, ldc32=N)
    p, lib, _ws = hip._gemm_params(ah, wh, M=M, N=N, K=K, lda=K, out32=out, ldc32=N)
    assert lib.pnc_gemm_wsplit_f16(ctypes.byref(p), None, hip._stream()) == -1                 # PNC_EINVAL: a NULL plane
    with pytest.raises(hip.PncError):                        # the binding: a plane of another layout
        hip.gemm(ah, wh, M=M, N=N, K=K, lda=K, w_lo16=wl[:32], out32=out, ldc32=N)
    # an fp16 A_lo is forwarded to the three-part launch of pnc_gemm_f16 (W_lo = the plane): its bits; W_lo next to it is refused
    fwd, three = torch.empty_like(out), torch.empty_like(out)
    hip.gemm(ah, wh, M=M, N=N, K=K, lda=K, a16_lo=al, w_lo16=wl, out32=fwd, ldc32=N)
    hip.gemm(ah, wh, M=M, N=N, K=K, lda=K, a16_lo=al, w_lo=wl, out32=three, ldc32=N)
    torch.cuda.synchronize()
    assert torch.equal(fwd, three)
    with pytest.raises(hip.PncError, match="PNC_EINVAL"):
        hip.gemm(ah, wh, M=M, N=N, K=K, lda=K, a16_lo=al, w_lo=wl, w_lo16=wl, out32=out, ldc32=N)
    assert hip.ABI_VERSION == 8 and hip.load().pnc_abi_version() == 8


# ---- end to end: the tiny network
def _tiny_w32(prec):
    w, _, kw = product_network("tiny", "cpu")
    w.diffusion_model.load_state_dict(synth.synth_state_dict(manifest("tiny"), round_fp16=False), strict=True)
    w = w.to(DEV)
    w.diffusion_model.precision = prec
    return w, kw, step_inputs("tiny", kw, DEV)


def test_tiny_network_on_unrounded_weights():
    ref = golden("tiny_w32")["eps"]
    errs = {}
    for p in ("precise", "precise-ckpt"):
        w, kw, inp = _tiny_w32(p)
        eps = w(inp["x"], inp["t"], cond(inp))
        torch.cuda.synchronize()
        errs[p] = err_stats(eps, ref)
        measured("precise_ckpt_tiny_w32", prec=p, max_abs=errs[p]["max_abs"], mean_abs=errs[p]["mean_abs"])
    print("tiny, unrounded weights vs tiny_w32:", errs)
    assert errs["precise-ckpt"]["max_abs"] <= 1e-3, errs
    assert "libpanacea_hip.so" in open("/proc/self/maps").read()


def test_representable_weights_give_the_precise_bits():
    """fp16-representable weights: every lo twin is zero and `precise-ckpt` is `precise` bit for bit — through the kernels with the
    weight part, the stencil-tile kernel's and the one-tile-per-workgroup stand-ins of the persistent kernels included"""
    w, _, kw = product_network("tiny", DEV)
    inp = step_inputs("tiny", kw, DEV)
    m = w.diffusion_model
    m.precision = "precise"
    base = w(inp["x"], inp["t"], cond(inp))
    m.precision = "precise-ckpt"
    ckpt = w(inp["x"], inp["t"], cond(inp))
    torch.cuda.synchronize()
    twins = [t for mod in m.modules() if getattr(mod, "_pk_lo", None)
             for t in mod._pk_lo.values() if isinstance(t, torch.Tensor) and t.dtype == torch.float16]
    assert twins and all(not bool(t.any()) for t in twins)
    assert torch.equal(ckpt, base)


def test_plain_hoisted_and_graphed_steps_are_bit_identical():
    from panacea_amd import sampling as Smp
    from panacea_amd.graph import GraphedStep
    w, kw, inp = _tiny_w32("precise-ckpt")
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
