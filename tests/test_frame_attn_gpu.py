"""pnc_attn_frame_f16 (include/panacea_hip.h section 6) on the MI355X against the float64 reference of tests/frame_attn_ref64.py,
and the first stage with the fused path forced and by default.

Bounds: the project's own attention bounds (tests/test_attn_edges_gpu.py) — unit-scale data atol 3e-3 + rtol 2e-3 |ref|, sharp rows
5e-3.  The kernel works on 64-query x 32-key tiles: the sizes below hold N equal to either tile, either tile + 8, the smallest legal
N = 8, several frames with N no multiple of the query tile, and one N beyond the row softmax's 16384.  Every buffer is at least as
large as its named elements; what is not named holds zeros in one run and NaN in the other, and the two must agree to the bit."""
import functools
import json

import numpy as np
import pytest
import torch

import attn_edge_cases as cases
import frame_attn_ref64 as ref64
from helpers import measured
from panacea_amd import hip, synth
from panacea_amd.nn import model
from test_vae import FULL, GOLDEN, TINY

pytestmark = pytest.mark.gpu
DEV = "cuda"
QT, KT = 64, 32              # the kernel's query and key tiles
TAIL = 8                     # spare rows behind q / k / o, and 8 * 8 spare elements behind V^T


def _padded(q, k, v, fill):
    """q, k, v: [F, N, C] fp16 on the CPU -> device buffers with ldq = C + 8, ldk = C + 16, ldvt = N + 8, vt_fstride = C * ldvt + 8 and
    TAIL rows behind the last frame; everything that is not a named element holds `fill`"""
    F, N, C = q.shape
    ldq, ldk, ldvt = C + 8, C + 16, N + 8
    fstride = C * ldvt + 8
    qb = torch.full((F * N + TAIL, ldq), fill, dtype=torch.float16)
    kb = torch.full((F * N + TAIL, ldk), fill, dtype=torch.float16)
    vb = torch.full((F * fstride + 8 * TAIL,), fill, dtype=torch.float16)
    qb[:F * N, :C], kb[:F * N, :C] = q.reshape(F * N, C), k.reshape(F * N, C)
    for f in range(F):
        vb[f * fstride:f * fstride + C * ldvt].view(C, ldvt)[:, :N] = v[f].t()
    return (qb.to(DEV), ldq, kb.to(DEV), ldk, vb.to(DEV), ldvt, fstride), dict(F=F, N=N, C=C, scale=float(C) ** -0.5)


def _launch(ops, geo):
    """-> the named rows of o [F * N, C] on the CPU; o starts as NaN and everything but its named elements must stay so"""
    F, N, C = geo["F"], geo["N"], geo["C"]
    ldo = C + 8
    o = torch.full((F * N + TAIL, ldo), cases.NAN, device=DEV, dtype=torch.float16)
    hip.attn_frame(*ops, o, ldo, **geo)
    torch.cuda.synchronize()
    assert torch.isnan(o[:, C:]).all(), "the padding of o's rows was written"
    assert torch.isnan(o[F * N:]).all(), "rows behind the last frame were written"
    return o[:F * N, :C].cpu()


def _within(tag, got, ref, bound):
    finite = bool(torch.isfinite(got.float()).all())
    err, over = cases.excess_error(got, ref, bound) if finite else (float("nan"), float("nan"))
    print(f"{tag}: attn_frame_kernel vs float64 max|err| {err:.3e} (|ref| max {ref.abs().max().item():.2f}), over the bound by {over:.3e}")
    measured("frame_attn " + tag.replace(" ", "_"), kernel="attn_frame_kernel", max_err=err, over_bound=over, atol=bound[0], rtol=bound[1])
    assert finite, f"{tag}: non-finite output ({int((~torch.isfinite(got.float())).sum())} of {got.numel()} elements)"
    assert over <= 0, f"{tag}: max|err| {err:.4e} exceeds atol {bound[0]} + rtol {bound[1]} |ref| by {over:.3e}"


def _zero_and_nan_padding(tag, q, k, v, bound):
    """the case with zeroed and with NaN padding, the latter twice: the same bits all three times, inside `bound` of float64"""
    F, N, C = q.shape
    ref = ref64.attn_frame(q, C, k, C, v.transpose(1, 2).contiguous(), N, C * N, F=F, N=N, C=C, scale=float(C) ** -0.5).reshape(F * N, C)
    assert torch.isfinite(ref).all()
    ops0, geo = _padded(q, k, v, 0.0)
    opsn, _ = _padded(q, k, v, cases.NAN)
    zero, nan1, nan2 = _launch(ops0, geo), _launch(opsn, geo), _launch(opsn, geo)
    _within(tag, nan1, ref, bound)
    assert torch.equal(zero.view(torch.int16), nan1.view(torch.int16)), f"{tag}: the content of the padding reaches the result"
    assert torch.equal(nan1.view(torch.int16), nan2.view(torch.int16)), f"{tag}: two runs differ"


# ------------------------------------------------------------------------------------------ 6. the kernel against float64
SIZES = [(1, 8), (3, 40), (2, 136), (1, 264),                  # the smallest legal N; partial tiles; several frames off the query tile
         (1, KT), (2, QT), (1, QT + 8)]                        # (KT + 8 = 40 is above) N equal to either tile, and the query tile + 8


@pytest.mark.parametrize("F,N", SIZES)
@pytest.mark.parametrize("C", [128, 256, 512])
def test_kernel_vs_float64_padded_strides(C, F, N):
    g = torch.Generator().manual_seed(1000 * C + N)
    q, k, v = (torch.randn(F, N, C, generator=g).half() for _ in range(3))
    _zero_and_nan_padding(f"unit C{C} F{F} N{N}", q, k, v, cases.UNIT)


# ------------------------------------------------------------------------------------------ 7. sharp and flat rows
def test_sharp_rows_dominant_key_in_the_first_and_in_the_last_tile():
    """One dominant key per row, its scaled score at least 40 above every other: for the even rows it lies in the LAST key tile
    (keys 256 .. 263: the accumulated O is rescaled by exp(-40) or less at the very end), for the odd rows in the first."""
    F, N, C = 1, 264, 512
    g = torch.Generator().manual_seed(77)
    k = torch.randn(F, N, C, generator=g).half()
    v = torch.randn(F, N, C, generator=g).half()
    i = torch.arange(N)
    target = torch.where(i % 2 == 0, 256 + (i // 2) % 8, (i // 2) % KT)
    q = (3.0 * k[0, target].float()).half()[None]
    s = (q[0].double() @ k[0].double().t()) * float(C) ** -0.5
    top = s.gather(1, target[:, None])[:, 0]
    rest = s.scatter(1, target[:, None], float("-inf")).max(dim=1).values
    assert (top - rest).min() >= 40.0, (top - rest).min()
    _zero_and_nan_padding("sharp C512 N264", q, k, v, cases.SHARP)


def test_flat_rows_equal_scores():
    """every key of a frame is the same row: all scores of a query are equal (and not zero), P = 1 / N"""
    F, N, C = 1, 264, 512
    g = torch.Generator().manual_seed(78)
    q = torch.randn(F, N, C, generator=g).half()
    k = torch.randn(F, 1, C, generator=g).half().expand(F, N, C).contiguous()
    v = torch.randn(F, N, C, generator=g).half()
    _zero_and_nan_padding("flat C512 N264", q, k, v, cases.UNIT)


# ------------------------------------------------------------------------------------------ 8. above the row softmax's limit
N_LONG = 16392               # an 8 x 2049 frame: 256 query tiles and one of 8 rows; 512 key tiles and one of 8 keys


def test_kernel_above_16384_tokens_sampled_rows_vs_float64():
    F, N, C = 1, N_LONG, 128
    g = torch.Generator().manual_seed(79)
    q, k, v = (torch.randn(F, N, C, generator=g).half() for _ in range(3))
    rows = torch.cat([torch.arange(16), 8192 + torch.arange(24), torch.arange(16384, N)])       # first tile, middle, last (partial) tile
    assert rows.numel() == 48
    ref = ref64.attn_frame(q, C, k, C, v.transpose(1, 2).contiguous(), N, C * N, F=F, N=N, C=C, scale=float(C) ** -0.5, rows=rows)[0]
    ops, geo = _padded(q, k, v, cases.NAN)
    got = _launch(ops, geo)
    assert torch.isfinite(got.float()).all()
    _within(f"long C{C} N{N} 48 rows", got[rows], ref, cases.UNIT)


def test_attn_block_above_16384_tokens_runs_without_an_n_by_n_buffer():
    """AttnBlock(128) on one 8 x 2049 frame: refused with NotImplementedError before the fused kernel.  The block's own tensors are
    about 50 MB; the N x N fp32 scores alone would be 1.07 GB."""
    C = 128
    torch.manual_seed(3)
    blk = model.AttnBlock(C).to(DEV)
    x = torch.randn(1, C, 8, 2049, generator=torch.Generator().manual_seed(4)).to(DEV)
    calls = []
    real = hip.attn_frame
    try:
        hip.attn_frame = lambda *a, **kw: (calls.append(kw["N"]), real(*a, **kw))[1]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        with torch.no_grad():
            out = blk(x)
        torch.cuda.synchronize()
        growth = torch.cuda.max_memory_allocated() - before
    finally:
        hip.attn_frame = real
    print(f"AttnBlock(128) over {N_LONG} tokens: peak memory growth {growth / 2 ** 20:.1f} MiB")
    measured("frame_attn block_long", growth_bytes=int(growth))
    assert calls == [N_LONG]
    assert out.shape == x.shape and torch.isfinite(out).all()
    assert growth < 256 * 2 ** 20, growth


# ------------------------------------------------------------------------------------------ 9 / 10. the first stage, forced and by default
@functools.lru_cache(maxsize=None)
def _tiny_stage(kind):
    name = "vae_tiny" if kind == "dec" else "vae_enc_tiny"
    man = json.loads((GOLDEN / f"manifest_{name}.json").read_text())
    net = (model.FirstStageDecoder if kind == "dec" else model.FirstStageEncoder)(4, TINY)
    net.load_state_dict(synth.synth_state_dict(man), strict=True)
    return net.to(DEV), np.load(GOLDEN / f"{name}.npz")


@functools.lru_cache(maxsize=None)
def _full_decoder():
    """-> (the full-width decoder on the GPU, 2 frames of a 16 x 48 latent, the oracle's image): test_vae.py's full-size case"""
    from oracle import vae_oracle as vo
    fs = model.FirstStageDecoder(4, FULL)
    sd = synth.synth_state_dict({k: list(v.shape) for k, v in fs.state_dict().items()})
    fs.load_state_dict(sd, strict=True)
    z = torch.randn(2, 4, 16, 48, generator=torch.Generator().manual_seed(3)) * 2.0
    return fs.to(DEV), z, vo.decode(sd, vo.VaeConfig(), z)


class _count_fused:
    """counts the launches of hip.attn_frame for the length of a `with` block (AttnBlock looks the wrapper up at every call)"""

    def __enter__(self):
        self.calls, self.real = [], hip.attn_frame
        hip.attn_frame = lambda *a, **kw: (self.calls.append((kw["F"], kw["N"], kw["C"])), self.real(*a, **kw))[1]
        return self.calls

    def __exit__(self, *exc):
        hip.attn_frame = self.real


def test_first_stage_with_the_fused_path_forced(monkeypatch):
    """the goldens and bounds of tests/test_vae.py (tiny decoder and encoder: max 8e-3, mean 1e-3; full-width decoder against the
    oracle: max 2e-2, mean 2e-3), every mid-block attention on the fused kernel"""
    monkeypatch.setattr(model, "FUSED_ATTN_MIN_TOKENS", 0)
    fs, g = _tiny_stage("dec")
    with _count_fused() as calls:
        img = fs.decode(torch.from_numpy(g["z"]).to(DEV))
        again = fs.decode(torch.from_numpy(g["z"]).to(DEV))
    d = (img.cpu() - torch.from_numpy(g["img"])).abs()
    print("fused: vae tiny decoder vs reference:", d.max().item(), d.mean().item())
    measured("frame_attn vae_tiny_dec", max_err=d.max().item(), mean_err=d.mean().item())
    assert calls == [(2, 8 * 48, 128)] * 2
    assert d.max().item() < 8e-3 and d.mean().item() < 1e-3
    assert torch.equal(img, again)
    fe, ge = _tiny_stage("enc")
    with _count_fused() as calls:
        mom = fe.moments(torch.from_numpy(ge["x"]).to(DEV))
    d = (mom.cpu() - torch.from_numpy(ge["moments"])).abs()
    print("fused: vae tiny encoder vs reference:", d.max().item(), d.mean().item())
    measured("frame_attn vae_tiny_enc", max_err=d.max().item(), mean_err=d.mean().item())
    assert calls == [(2, 8 * 48, 128)]
    assert d.max().item() < 8e-3 and d.mean().item() < 1e-3
    fd, z, ref = _full_decoder()
    with _count_fused() as calls:
        img = fd.decode(z.to(DEV))
    d = (img.cpu() - ref).abs()
    print("fused: vae full-width, 16x48 latent vs oracle:", d.max().item(), d.mean().item(), "ref max", ref.abs().max().item())
    measured("frame_attn vae_full_dec", max_err=d.max().item(), mean_err=d.mean().item())
    assert calls == [(2, 16 * 48, 512)]
    assert d.max().item() < 2e-2 and d.mean().item() < 2e-3


def test_default_dispatch_makes_no_fused_launch():
    assert model.FUSED_ATTN_MIN_TOKENS == 16385
    fs, g = _tiny_stage("dec")
    fd, z, ref = _full_decoder()
    with _count_fused() as calls:
        img = fs.decode(torch.from_numpy(g["z"]).to(DEV))
        big = fd.decode(z.to(DEV))
        torch.cuda.synchronize()
    assert calls == []
    assert torch.isfinite(img).all() and torch.isfinite(big).all()
