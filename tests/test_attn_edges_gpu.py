"""Attention kernels against a float64 reference at ragged key counts and poisoned padding (MI355X).

Reference: tests/attn_ref64.py — float64 softmax attention indexed from the header's formulae, independent of tests/emu.py
(tests/test_attn_ref64.py holds the emulation to it within half of the bounds used here).  Bounds: the project's own — unit-scale
data atol 3e-3 + rtol 2e-3 (test_attn_views_self, test_attn_temporal), sharp rows 5e-3 (test_attn_views_sharp_softmax), split
kernels SPLIT_BOUND of tests/test_precise_wide_gpu.py.  Every buffer is allocated larger than the launch may read and the excess
holds NaN; outputs start as NaN and the rows behind the last query must stay so.

  1. ragged key buffers (65 / 77 / 90 rows, NaN behind every V^T row): the dispatcher must keep attn_text_kernel away
  2. attn_text_kernel against float64 where pnc_attn_uses_text_kernel says it runs, forced and unforced
  3. PncAttnParams.kv_valid: finite garbage in the keys kv_valid .. Nkv - 1 changes no output bit
  4. pnc_attn_temporal_split_f16 at 9 .. 16 frames
"""
import pytest
import torch

import attn_edge_cases as cases
import attn_ref64
from helpers import measured
from panacea_amd import hip
from test_precise_wide_gpu import S as LO_UNIT, SPLIT_BOUND, _operands, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"


class _options:
    """library options for the length of a `with` block (None = leave the option alone)"""

    def __init__(self, **opts):
        self.opts = [(getattr(hip, "OPT_" + n.upper()), v) for n, v in opts.items() if v is not None]
        self.prev = []

    def __enter__(self):
        try:
            for o, v in self.opts:
                self.prev.append((o, hip.set_option(o, v)))
        except BaseException:
            self.__exit__()
            raise

    def __exit__(self, *exc):
        for o, v in reversed(self.prev):
            hip.set_option(o, v)
        self.prev = []


def _option(o):
    """the current value of a library option"""
    v = hip.set_option(o, 0)
    hip.set_option(o, v)
    return v


def _to_dev(buf):
    return dict(buf, **{n: t.to(DEV) for n, t in buf.items() if torch.is_tensor(t)})


def _launch(buf, lds, geo, **opts):
    """-> (fp16 output rows on the CPU, did the text kernel run); checks that nothing was written behind the last query row"""
    o = torch.full((buf["M"] + cases.EXCESS, buf["C"]), cases.NAN, device=DEV, dtype=torch.float16)
    ops = cases.operands(buf, lds)
    with _options(**opts):
        text = hip.attn_uses_text_kernel(*ops, o, lds["ldo"], **geo)
        hip.attn_views(*ops, o, lds["ldo"], **geo)
        torch.cuda.synchronize()
    assert torch.isnan(o[buf["M"]:]).all(), "rows behind the last query were written"
    return o[: buf["M"]].cpu(), text


def _within(tag, got, ref, bound, kernel):
    finite = bool(torch.isfinite(got.float()).all())
    err, over = cases.excess_error(got, ref, bound) if finite else (float("nan"), float("nan"))
    print(f"{tag}: {kernel} vs float64 max|err| {err:.3e} (|ref| max {ref.abs().max().item():.2f}), over the bound by {over:.3e}")
    measured("attn_edges " + tag.replace(" ", "_"), kernel=kernel, max_err=err, over_bound=over, atol=bound[0], rtol=bound[1])
    assert finite, f"{tag}: non-finite output ({int((~torch.isfinite(got.float())).sum())} of {got.numel()} elements)"
    assert over <= 0, f"{tag}: max|err| {err:.4e} exceeds atol {bound[0]} + rtol {bound[1]} |ref| by {over:.3e}"


_REF = {}


def _ref_views(key, buf, lds, geo):
    """the float64 reference of a case, computed once from the CPU buffers and shared"""
    if key not in _REF:
        _REF[key] = attn_ref64.attn_views(*cases.operands(buf, lds), **geo)
        assert torch.isfinite(_REF[key]).all()
    return _REF[key]


# ------------------------------------------------------------------------------------------ 1. ragged key buffers
# (1, 1, 8, 96, 12): 6 query tiles x 3 head groups = 18 >= 16 — the default dispatcher sent it to attn_text_kernel before the guard
@pytest.mark.parametrize("Nkv", [65, 77, 90])
@pytest.mark.parametrize("B,T,H,W,heads", [(1, 1, 8, 96, 12), (1, 2, 4, 48, 2)])
def test_ragged_key_buffer_stays_off_the_text_kernel(B, T, H, W, heads, Nkv):
    """kvW = kv_valid = Nkv, ldvt = Nkv rounded up to 8; V^T columns Nkv .. ldvt - 1 and the K rows from Nkv on hold NaN.  A kernel
    that stages V^T in 8-key chunks guarded per chunk multiplies P = 0 by that NaN: attn_text_kernel, which the dispatcher chose for
    the 8 x 96 x 12-head grid unforced (and anywhere under variant 43) until attn_text_dispatch asked for kvH * kvW % 8 == 0."""
    key = ("ragged", B, T, H, W, heads, Nkv)
    buf, lds, geo = cases.text_case(B, T, H, W, heads, Nkv, Nkv, seed=11)
    assert lds["ldvt"] % 8 == 0 and lds["ldvt"] > Nkv and lds["vt_gstride"] == buf["C"] * lds["ldvt"]
    ref = _ref_views(key, buf, lds, geo)
    dbuf = _to_dev(buf)
    outs = {}
    for variant in (0, 43, 42, 41):
        outs[variant], text = _launch(dbuf, lds, geo, attn_variant=variant)
        assert not text, f"variant {variant}: the text kernel would run on a {Nkv}-row key buffer"
        _within(f"ragged {H}x{W}x{heads} Nkv={Nkv} v{variant}", outs[variant], ref, cases.UNIT, "attn_views_kernel")
    # 43 without the text kernel is the 4-wave x 1-block workgroup (41); 0 resolves by view size: 42 from 256 queries on, else 41
    assert torch.equal(outs[43], outs[41])
    assert torch.equal(outs[0], outs[42 if H * W >= 256 else 41])


# ------------------------------------------------------------------------------------------ 2. the text kernel where it runs
@pytest.mark.parametrize("B,T,H,W,heads,rows,kv_valid,sharp,variant", [
    (2, 2, 4, 48, 5, 80, 65, 1.0, 43),
    (1, 3, 13, 31, 7, 80, 77, 1.0, 43),           # 403 queries: the last 128-query tile is ragged; 7 heads = 5 + 2
    (1, 2, 4, 48, 12, 96, 96, 1.0, 43),
    (2, 1, 8, 24, 7, 96, 80, 6.0, 43),            # sharp rows
    (1, 1, 4, 48, 5, 80, 80, 1.0, 43),
    (1, 1, 8, 96, 12, 80, 77, 1.0, 0),            # the 768-query, 12-head grid: dispatched without being forced
    (1, 2, 8, 96, 12, 96, 65, 1.0, 0),
])
def test_text_kernel_vs_float64_where_it_runs(B, T, H, W, heads, rows, kv_valid, sharp, variant):
    buf, lds, geo = cases.text_case(B, T, H, W, heads, rows, kv_valid, sharp=sharp, seed=13)
    ref = _ref_views(("text", B, T, H, W, heads, rows, kv_valid, sharp), buf, lds, geo)
    dbuf = _to_dev(buf)
    ops = cases.operands(dbuf, lds)
    o = torch.empty((buf["M"], buf["C"]), device=DEV, dtype=torch.float16)
    with _options(attn_variant=variant):
        # the ways out of the text kernel, each for the same parameters otherwise
        assert not hip.attn_uses_text_kernel(*ops, o, lds["ldo"], **dict(geo, causal=True))
        assert not hip.attn_uses_text_kernel(*ops, o, lds["ldo"], **dict(geo, kv_valid=64))
        with _options(attn_dma=_option(hip.OPT_ATTN_DMA) | 4):
            assert not hip.attn_uses_text_kernel(*ops, o, lds["ldo"], **geo)
        assert hip.attn_uses_text_kernel(*ops, o, lds["ldo"], **geo)
    got, text = _launch(dbuf, lds, geo, attn_variant=variant)
    assert text, "pnc_attn_uses_text_kernel == 0 right before the launch"
    _within(f"text {H}x{W}x{heads} {kv_valid}of{rows} q*{sharp:g} v{variant}", got, ref, cases.SHARP if sharp > 1 else cases.UNIT,
            "attn_text_kernel")


# ------------------------------------------------------------------------------------------ 3. padding content does not matter
def _zero_vs_garbage(tag, key, build, bound, kernel, expect_text=None, **opts):
    """the same operands with zeroed and with garbage padding: same bits, and within the bound of the float64 reference"""
    outs = []
    for pad in ("zero", "garbage"):
        buf, lds, geo = build(pad)
        if pad == "zero":
            ref = _ref_views(key, buf, lds, geo)
        got, text = _launch(_to_dev(buf), lds, geo, **opts)
        if expect_text is not None:
            assert text == expect_text, (tag, text)
        outs.append(got)
    _within(tag, outs[1], ref, bound, kernel)
    diff = outs[0] != outs[1]
    assert not diff.any(), f"{tag}: {int(diff.sum())} outputs change with the content of the padding keys"


@pytest.mark.parametrize("rows,kv_valid,variant", [(80, 77, 43), (80, 77, 42), (80, 77, 41), (96, 90, 43)])
def test_padding_content_text_keys(rows, kv_valid, variant):
    _zero_vs_garbage(f"padding text {kv_valid}of{rows} v{variant}", ("padding text", rows, kv_valid), lambda pad: cases.text_case(2, 2, 4, 48, 7, rows, kv_valid, pad=pad, seed=15),
                     cases.UNIT, "attn_text_kernel" if variant == 43 else "attn_views_kernel", expect_text=variant == 43, attn_variant=variant)


@pytest.mark.parametrize("G,L,Lp,heads,sum_trigger", [(2, 77, 80, 3, None), (1, 33, 200, 2, None), (1, 33, 200, 2, 0)])
def test_padding_content_causal_tower(G, L, Lp, heads, sum_trigger):
    """L = 33 of Lp = 200: three of the four key tiles are padding throughout — with the sum-triggered running maximum at its default
    (the optimistic path sees a row sum of 0) and off (the row maximum of an all-masked tile)"""
    _zero_vs_garbage(f"padding causal {L}of{Lp} sumtrig={sum_trigger}", ("padding causal", G, L, Lp, heads), lambda pad: cases.causal_case(G, L, Lp, heads, pad=pad), cases.UNIT,
                     "attn_views_kernel", expect_text=False, attn_sum_trigger=sum_trigger)


def test_padding_content_cross_view_two_segments():
    """views of 5 rows x 10 columns, 37 of their 50 keys valid, two key segments: the gather path, one partly masked tile per segment"""
    _zero_vs_garbage("padding cross 5x10 37of50", "padding cross", lambda pad: cases.cross_case(2, 5, 10, 2, 37, pad=pad), cases.UNIT, "attn_views_kernel",
                     expect_text=False)


# ------------------------------------------------------------------------------------------ 4. split temporal kernel, 9 .. 16 frames
def _temporal_split(planes, B, T, Npix, heads, rows_alloc):
    """planes: six [rows_alloc, C] device tensors (q, q_lo, k, k_lo, v, v_lo) -> the two output planes [rows_alloc, C], prefilled with 7"""
    C = heads * 64
    o, olo = (torch.full((rows_alloc, C), 7.0, device=DEV, dtype=torch.float16) for _ in range(2))
    qh, ql, kh, kl, vh, vl = planes
    hip.attn_temporal_split(qh, ql, C, kh, kl, C, vh, vl, C, o, olo, C, B=B, T=T, Npix=Npix, heads=heads, scale=0.125)
    torch.cuda.synchronize()
    return o, olo


@pytest.mark.parametrize("B,T,Npix,heads", [(2, 9, 21, 2), (1, 13, 7, 5), (1, 15, 33, 1), (2, 16, 10, 2)])
def test_temporal_split_kernel_nine_to_sixteen_frames_vs_float64(B, T, Npix, heads):
    """hi + lo / 2048 against float64 attention of the split values (operands as test_temporal_split_kernel_vs_float64 builds them)
    under its bound.  T = 9: the launch again inside an allocation that goes on for 8 * Npix rows of NaN in all six operand planes —
    the same bits, finite, and both output planes unwritten behind the last frame."""
    g = torch.Generator().manual_seed(7 + T)
    C, M = heads * 64, B * T * Npix
    planes = [t for mag in (2e-3, 1e3, 1e3) for t in _operands(M, C, g, mag)]
    joined = [planes[i].double().cpu() + planes[i + 1].double().cpu() * LO_UNIT for i in (0, 2, 4)]
    ref = attn_ref64.attn_temporal(joined[0], C, joined[1], C, joined[2], C, B=B, T=T, Npix=Npix, heads=heads, scale=0.125)
    o, olo = _temporal_split(planes, B, T, Npix, heads, M)
    got = o.double().cpu() + olo.double().cpu() * LO_UNIT
    assert torch.isfinite(got).all()
    err = _rel(got, ref)
    print(f"temporal split B{B} T{T} Npix{Npix} heads{heads}: {err:.2e}")
    measured(f"attn_edges temporal_split_B{B}_T{T}_Npix{Npix}_h{heads}", kernel="attn_temporal_split_kernel", rel_err=err, bound=SPLIT_BOUND)
    assert err < SPLIT_BOUND, err
    if T == 9:
        pad = 8 * Npix                                              # where frames 9 .. 16 of the last sample's pixels would be
        big = []
        for t in planes:
            b = torch.full((M + pad, C), cases.NAN, device=DEV, dtype=torch.float16)
            b[:M] = t
            big.append(b)
        o2, olo2 = _temporal_split(big, B, T, Npix, heads, M + pad)
        assert (o2[M:] == 7.0).all() and (olo2[M:] == 7.0).all()
        assert torch.isfinite(o2[:M]).all() and torch.isfinite(olo2[:M]).all()
        assert torch.equal(o2[:M], o) and torch.equal(olo2[:M], olo)


def test_temporal_split_identity_probabilities_asymmetric_values():
    """test_attn_temporal_identity_probabilities_asymmetric_values for the split kernel at T = 13: a one-hot q = k makes every query
    attend its own frame alone (the other scores are 50 below: their probabilities round to 0 in both planes), v = distinct integers
    per (frame, channel).  The hi plane must be v itself and the lo plane zero: a permuted fragment map of either MFMA cannot pass."""
    B, T, Npix, heads = 1, 13, 5, 2
    C, M = heads * 64, B * T * Npix
    q = torch.zeros(B, T, Npix, heads, 64)
    for t in range(T):
        q[:, t, :, :, (5 * t + 3) % 64] = 20.0
    q = q.reshape(M, C).to(torch.float16).to(DEV)
    v = ((torch.arange(M * C).view(M, C) * 7 + torch.arange(M).view(M, 1) * 3) % 1021).to(torch.float16).to(DEV)
    z = torch.zeros_like(q)
    o, olo = _temporal_split([q, z, q, z, v, z], B, T, Npix, heads, M)
    assert torch.equal(o, v)
    assert not olo.any()
