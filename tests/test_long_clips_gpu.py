"""Clips of 9 to 16 frames on the MI355X.

Kernel parity of the three entry points that take the frame count — pnc_attn_temporal_f16 (attn_temporal_wide_kernel, the MFMA
kernel of 9 <= T <= 16), pnc_groupnorm_temporal_silu and pnc_groupnorm_temporal_part (gn_temporal_kernel<9..16>: one work item per
thread) — against the torch emulation (tests/emu.py), with the tolerances of tests/test_kernels_gpu.py::test_attn_temporal (3e-3),
test_groupnorm_temporal (4e-3) and test_groupnorm_temporal_in_parts (2e-3; lo planes 2e-4 / 1e-4; statistics rtol 1e-5, atol 1e-4).

Network parity at 12 and 16 frames against the reference's own forward (tests/golden/tiny_t12.npz / tiny_t16.npz) with the bounds of
tests/test_model_gpu.py, the full-width network at 16 frames against the oracle at the 1e-3 / 2e-4 contract, and one fused + hoisted
sampler step at 16 frames replayed from a captured graph."""
import numpy as np
import pytest
import torch

import emu
from helpers import cond, err_stats, golden, measured, oracle_cfg, product_network, step_inputs
from panacea_amd import configs, hip

pytestmark = pytest.mark.gpu
DEV = "cuda"
NORTH_STAR = 1e-3                                                    # tests/test_model_gpu.py
TOL = {"precise": (NORTH_STAR, 2e-4), "fast": (3e-3, 5e-4)}         # its ("tiny", policy) bounds
BLOCK_TOL = {"precise": 9e-4, "fast": 1.1e-3}                        # its BLOCK_TOL[("tiny", policy)]


def rnd(*shape, scale=1.0, dtype=torch.float32, seed=None):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed if seed is not None else (hash(shape) & 0xFFFF) + 17)
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(DEV)


def check(name, got, ref, atol, rtol=2e-3):
    got, ref = got.float(), ref.float()
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = (got - ref).abs()
    tol = atol + rtol * ref.abs()
    print(f"{name}: max|err| {err.max().item():.3e} (ref max {ref.abs().max().item():.3e})")
    if (err - tol).max().item() > 0:
        idx = torch.nonzero(err > tol)
        first = idx[0].tolist()
        raise AssertionError(f"{name}: {idx.shape[0]}/{err.numel()} elements off; max|err|={err.max().item():.4e}; first bad index "
                             f"{first}: got {got[tuple(first)].item():.5f} ref {ref[tuple(first)].item():.5f}")


# ------------------------------------------------------------------------------------------ kernels
# Npix = 33 / 50 / 7 with 1 / 5 / 20 heads: B * Npix * heads work items are not a multiple of the 4 waves of a workgroup for
# (1, 33, 1), (1, 7, 5) and the last workgroup of a launch is partly empty
@pytest.mark.parametrize("heads", [1, 5, 20])
@pytest.mark.parametrize("B,T,Npix", [(2, 9, 50), (1, 12, 33), (1, 15, 7), (2, 16, 96)])
def test_attn_temporal_nine_to_sixteen_frames(B, T, Npix, heads):
    C, M = heads * 64, B * T * Npix
    qkv = rnd(M, 3 * C, dtype=torch.float16, seed=21 + T)
    oh = torch.zeros(M, C, device=DEV, dtype=torch.float16)
    oe = torch.zeros_like(oh)
    flat = qkv.reshape(-1)
    hip.attn_temporal(qkv, 3 * C, qkv[:, C:], 3 * C, qkv[:, 2 * C:], 3 * C, oh, C, B=B, T=T, Npix=Npix, heads=heads, scale=0.125)
    emu.attn_temporal(flat, 3 * C, flat[C:], 3 * C, flat[2 * C:], 3 * C, oe, C, B=B, T=T, Npix=Npix, heads=heads, scale=0.125)
    torch.cuda.synchronize()
    check(f"attn_temporal T={T} heads={heads}", oh, oe, 3e-3)


def test_attn_temporal_identity_probabilities_asymmetric_values():
    """Exact data: q = k = one-hot rows scaled so that every query attends to its own frame alone (the other scores are 48 below),
    v = distinct integers per (frame, channel).  The output must be v itself, bit for bit: a transposed or permuted fragment map of
    either MFMA, or a wrong channel order of the 16-byte stores, cannot pass."""
    B, T, Npix, heads = 1, 13, 5, 2
    C, M = heads * 64, B * T * Npix
    q = torch.zeros(B, T, Npix, heads, 64)
    for t in range(T):
        q[:, t, :, :, (5 * t + 3) % 64] = 20.0
    q = q.reshape(M, C).to(torch.float16).to(DEV)
    v = ((torch.arange(M * C).view(M, C) * 7 + torch.arange(M).view(M, 1) * 3) % 1021).to(torch.float16).to(DEV)
    o = torch.zeros(M, C, device=DEV, dtype=torch.float16)
    hip.attn_temporal(q, C, q, C, v, C, o, C, B=B, T=T, Npix=Npix, heads=heads, scale=0.125)
    torch.cuda.synchronize()
    assert torch.equal(o, v)


def test_attn_temporal_reads_nothing_behind_the_last_frame():
    """T = 9: the MFMA tile has 7 empty rows.  The allocation continues behind the last valid row and is NaN-filled there: the output
    must be finite and the same bits as on a clean buffer (rows t >= T are neither read nor allowed to reach P x V)."""
    B, T, Npix, heads = 1, 9, 40, 5
    C, M = heads * 64, B * T * Npix
    pad = 8 * Npix                                                  # where frames 9 .. 16 of the pixel rows would be
    qkv = rnd(M, 3 * C, dtype=torch.float16, seed=33)
    big = torch.full((M + pad, 3 * C), float("nan"), device=DEV, dtype=torch.float16)
    big[:M] = qkv
    outs = []
    for buf in (qkv, big):
        o = torch.full((M + pad, C), 7.0, device=DEV, dtype=torch.float16)
        hip.attn_temporal(buf, 3 * C, buf[:, C:], 3 * C, buf[:, 2 * C:], 3 * C, o, C, B=B, T=T, Npix=Npix, heads=heads, scale=0.125)
        torch.cuda.synchronize()
        assert (o[M:] == 7.0).all()                                 # nothing written behind the last frame either
        outs.append(o[:M])
    assert torch.isfinite(outs[1]).all() and torch.equal(outs[0], outs[1])
    oe = torch.zeros(M, C, device=DEV, dtype=torch.float16)
    flat = qkv.reshape(-1)
    emu.attn_temporal(flat, 3 * C, flat[C:], 3 * C, flat[2 * C:], 3 * C, oe, C, B=B, T=T, Npix=Npix, heads=heads, scale=0.125)
    check("attn_temporal T=9 (NaN behind the last row)", outs[1], oe, 3e-3)


@pytest.mark.parametrize("lo", [None, "f16", "e4m3"])
@pytest.mark.parametrize("B,T,Npix,C", [(2, 9, 50, 64), (1, 12, 77, 320), (1, 16, 33, 640), (1, 16, 40, 1280), (2, 12, 21, 1280),
                                        (1, 9, 19, 640), (2, 16, 96, 320)])
def test_groupnorm_temporal_nine_to_sixteen_frames(B, T, Npix, C, lo):
    x = rnd(B * T * Npix, C, seed=40 + T) * 1.3 - 0.4
    gamma, beta = rnd(C, seed=41) * 0.5 + 1, rnd(C, seed=42) * 0.3
    yh = torch.zeros(B * T * Npix, C, device=DEV, dtype=torch.float16)
    ye = torch.zeros_like(yh)
    mk = {None: lambda: None, "f16": lambda: torch.zeros_like(yh), "e4m3": lambda: torch.zeros(B * T * Npix, C, device=DEV, dtype=torch.uint8)}[lo]
    lh, le = mk(), mk()
    hip.groupnorm_temporal_silu(x, B, T, Npix, C, gamma, beta, 1e-5, yh, lh)
    emu.groupnorm_temporal_silu(x, B, T, Npix, C, gamma, beta, 1e-5, ye, le)
    torch.cuda.synchronize()
    check(f"gn_temporal T={T} C={C}", yh, ye, 4e-3)
    if lo is not None:
        dec = (lambda t: t.view(torch.float8_e4m3fn).float()) if lo == "e4m3" else (lambda t: t.float())
        check(f"gn_temporal T={T} C={C} hi + lo ({lo})", yh.float() + dec(lh) / 2048.0, ye.float() + dec(le) / 2048.0, 2e-4, 1e-4)


@pytest.mark.parametrize("lo8", [False, True])
@pytest.mark.parametrize("B,T,Tl,Npix,C", [(2, 16, 16, 50, 64), (1, 16, 8, 77, 320), (1, 16, 16, 33, 640), (2, 16, 16, 21, 1280), (1, 16, 8, 19, 1280),
                                           (1, 12, 12, 40, 320), (1, 9, 9, 19, 1280)])
def test_groupnorm_temporal_in_parts_up_to_sixteen_frames(B, T, Tl, Npix, C, lo8):
    """modes 1 and 2 of pnc_groupnorm_temporal_part with T_total up to 16: all frames on one rank (Tl = T: the widened kernel, the
    G = 1 frame shard) and 16 frames on two ranks of 8 (the T <= 8 kernel with T_total = 16); t_pad = 1 and 0."""
    x = rnd(B * T * Npix, C, seed=71) * 1.3 - 0.4
    gamma, beta = rnd(C, seed=72) * 0.5 + 1, rnd(C, seed=73) * 0.3
    ref = torch.zeros(B * T * Npix, C, device=DEV, dtype=torch.float16)
    ref_lo = torch.zeros(B * T * Npix, C, device=DEV, dtype=torch.uint8 if lo8 else torch.float16)
    emu.groupnorm_temporal_silu(x, B, T, Npix, C, gamma, beta, 1e-5, ref, ref_lo)
    dec = (lambda t: t.view(torch.float8_e4m3fn).float()) if lo8 else (lambda t: t.float())
    G = T // Tl
    xv = x.view(B, T, Npix, C)
    parts = [xv[:, g * Tl:(g + 1) * Tl].contiguous() for g in range(G)]
    stats = [torch.zeros(B * Npix * 64, device=DEV) for _ in range(G)]
    for g in range(G):
        hip.groupnorm_temporal_part(parts[g], B, Tl, Npix, C, gamma, beta, 1e-5, stats[g], 1, T)
    es = torch.zeros_like(stats[0])
    emu.groupnorm_temporal_part(parts[0], B, Tl, Npix, C, gamma, beta, 1e-5, es, 1, T)
    torch.cuda.synchronize()
    assert torch.allclose(stats[0], es, rtol=1e-5, atol=1e-4)
    total = torch.stack(stats).sum(0)
    for g in range(G):
        for t_pad in (1, 0):
            y = torch.full((B, Tl + 2 * t_pad, Npix, C), 9.0, device=DEV, dtype=torch.float16)
            ylo = torch.zeros(B, Tl + 2 * t_pad, Npix, C, device=DEV, dtype=torch.uint8 if lo8 else torch.float16)
            hip.groupnorm_temporal_part(parts[g], B, Tl, Npix, C, gamma, beta, 1e-5, total, 2, T, y, ylo, t_pad)
            torch.cuda.synchronize()
            if t_pad:
                assert (y[:, 0] == 9.0).all() and (y[:, -1] == 9.0).all()      # the halo slots are the exchange's, not the kernel's
            sl = slice(t_pad, t_pad + Tl)
            want = ref.view(B, T, Npix, C)[:, g * Tl:(g + 1) * Tl]
            check(f"gn_temporal_part[{g}] T={T} Tl={Tl} t_pad={t_pad}", y[:, sl], want, 2e-3)
            rec = y[:, sl].float() + dec(ylo[:, sl]) / 2048.0
            rr = want.float() + dec(ref_lo.view(B, T, Npix, C)[:, g * Tl:(g + 1) * Tl]) / 2048.0
            check(f"gn_temporal_part_lo[{g}] T={T} Tl={Tl} t_pad={t_pad}", rec, rr, 2e-4, 1e-4)


# ------------------------------------------------------------------------------------------ network
def _tiny(T, prec):
    kw = configs.with_frames(configs.get("tiny"), T)
    w, sd, _ = product_network("tiny", DEV, kw=kw)
    w.diffusion_model.precision = prec
    return w, sd, kw, step_inputs("tiny", kw, DEV, shape=(2, T, 8, 96))


@pytest.mark.parametrize("T", [12, 16])
@pytest.mark.parametrize("prec", ["precise", "fast"])
def test_hip_path_matches_reference_golden_at_12_and_16_frames(T, prec):
    w, _, kw, inp = _tiny(T, prec)
    gold = golden(f"tiny_t{T}")
    trace = {}
    eps = w(inp["x"], inp["t"], cond(inp), trace=trace)
    torch.cuda.synchronize()
    st = err_stats(eps, gold["eps"])
    print(f"tiny, T={T}, {prec}:", st)
    measured("long_clip_tiny", T=T, prec=prec, max_abs=st["max_abs"], mean_abs=st["mean_abs"])
    assert eps.is_cuda and eps.dtype == torch.float32
    assert st["max_abs"] <= TOL[prec][0] and st["mean_abs"] <= TOL[prec][1], st
    worst, checked = 0.0, 0
    for k in gold.files:
        key = k[6:] if k.startswith("block.") else k
        if key in trace and k != "eps" and not k.startswith("stride."):
            ref = gold[k]
            got = trace[key].reshape(-1)[::int(gold["stride." + k])].cpu().numpy()
            rel = np.abs(got - ref).max() / max(1.0, np.abs(ref).max())
            worst = max(worst, rel)
            checked += 1
            assert rel <= BLOCK_TOL[prec], (k, rel)
    assert checked >= 15
    measured("long_clip_block_trace", T=T, prec=prec, worst_rel=float(worst))


def test_hip_path_precise_wide_at_16_frames():
    w, _, kw, inp = _tiny(16, "precise-wide")
    eps = w(inp["x"], inp["t"], cond(inp))
    torch.cuda.synchronize()
    st = err_stats(eps, golden("tiny_t16")["eps"])
    print("tiny, T=16, precise-wide:", st)
    measured("long_clip_tiny", T=16, prec="precise-wide", max_abs=st["max_abs"], mean_abs=st["mean_abs"])
    assert st["max_abs"] <= NORTH_STAR, st


def test_frame_shard_loop_back_with_all_16_frames_local():
    """engine.FrameShard(1, 0): G = 1, local T = 16 — the ResBlock3D temporal sites run modes 1 and 2 of the widened part kernel
    and the halo-frame temporal conv.  Other roundings of the statistics than the fused kernel: eps differs like two `precise`
    evaluations do (the bound of tests/test_model_gpu.py::test_frame_shard_code_path_single_device)."""
    from panacea_amd import engine as E, parallel
    w, _, kw, inp = _tiny(16, "precise")
    ref = w(inp["x"], inp["t"], cond(inp))
    sh = E.FrameShard(1, 0, None)
    parallel.apply_frame_shard(w, sh)
    got = w(inp["x"], inp["t"], cond(inp))
    torch.cuda.synchronize()
    d = (got - ref).abs()
    print(f"T=16 frame loop-back vs unsharded: max {d.max().item():.3e} mean {d.mean().item():.3e}; {sh.exchanges} exchanges")
    assert sh.exchanges >= 20 and d.max().item() <= 1.2e-3 and d.mean().item() <= 2e-4
    st = err_stats(got, golden("tiny_t16")["eps"])
    assert st["max_abs"] <= NORTH_STAR and st["mean_abs"] <= 2e-4, st


def test_full_network_16_frames_small_panorama_vs_oracle():
    """Every tensor of the Panacea+ stage-2 network at its real width (C = 320 .. 1280, 5 .. 20 heads) at 16 frames; the
    small-panorama shape of tests/test_model_gpu.py::test_full_network_small_panorama_vs_oracle (B = 1, latent 16x192), policy
    `precise`, against the CPU oracle on the same synthetic weights and inputs: the 1e-3 / 2e-4 contract."""
    from oracle import panacea_oracle as po
    kw = configs.with_frames(configs.get("full"), 16)
    w, sd, _ = product_network("full", "cpu", kw=kw)
    inp = step_inputs("full", kw, "cpu", shape=(1, 16, 16, 192))
    ref = po.wrapper_forward(sd, oracle_cfg(kw), inp["x"], inp["t"], cond(inp))
    w = w.to(DEV)
    g = {k: v.to(DEV) for k, v in inp.items()}
    assert w.diffusion_model.precision == "precise"
    eps = w(g["x"], g["t"], cond(g))
    torch.cuda.synchronize()
    st = err_stats(eps, ref)
    print("full network, T=16, 16x192:", st)
    measured("long_clip_full", T=16, max_abs=st["max_abs"], mean_abs=st["mean_abs"])
    assert st["ref_max"] > 1.0
    assert st["max_abs"] <= NORTH_STAR and st["mean_abs"] <= 2e-4, st
    assert w.diffusion_model.lo_clamped == 0


def test_fused_hoisted_step_at_16_frames_replays_from_a_graph():
    """One fused + hoisted Euler / CFG step at 16 frames, captured with panacea_amd.graph and replayed: the eager step's bits."""
    from panacea_amd import sampling as S
    from panacea_amd.graph import GraphedStep
    T = 16
    w, _, kw, inp = _tiny(T, "precise")
    c = {"crossattn": inp["crossattn"][1:2], "concat": inp["concat"][T:], "cond_feat": inp["cond_feat"][T:]}
    uc = {"crossattn": inp["crossattn"][0:1], "concat": inp["concat"][:T], "cond_feat": inp["cond_feat"][:T]}
    smp = S.EulerEDMSampler(3, guider=S.VanillaCFG(5.0), device=DEV)
    sig = smp.sigmas()
    x0 = inp["x"][T:] * 14.6
    s_in = x0.new_ones([T])
    bd = S.BoundDenoiser(S.DiscreteDenoiser().to(DEV), w)
    with torch.no_grad():
        c2, u2 = S.hoist_invariants(w, smp.guider, c, uc)
        assert smp._fusable(bd, x0, c2)
        step = lambda xi, s0, s1: smp.sampler_step(s0, s1, bd, xi, c2, u2)   # noqa: E731
        e0 = step(x0, s_in * sig[0], s_in * sig[1])
        e1 = step(e0, s_in * sig[1], s_in * sig[2])
        g = GraphedStep(step, x0, s_in * sig[0], s_in * sig[1])
        g0 = g(x0, s_in * sig[0], s_in * sig[1]).clone()
        g1 = g(g0, s_in * sig[1], s_in * sig[2]).clone()
    torch.cuda.synchronize()
    assert torch.isfinite(e1).all() and (e1 - e0).abs().max().item() > 1e-3
    assert torch.equal(g0, e0) and torch.equal(g1, e1)
