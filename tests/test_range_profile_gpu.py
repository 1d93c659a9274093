"""pnc_operand_stats_f16 and the operand range profile on the MI355X.  Every figure is an integer count: the kernel's records are
compared with numpy's (tests/emu.py, written from the header text) word for word, no tolerance.

Kernel shapes: the smallest at which the kernel can go wrong — one chunk, less than a wave, ragged multiples of the 8-element chunk,
a leading dimension wider than the row (NaN-filled padding in both planes), and 4099 x 72 = 36 891 chunks: more than one workgroup,
several strides of the grid, a ragged tail in the last wave."""
import warnings

import numpy as np
import pytest
import torch

import emu
from helpers import cond, manifest, product_network, step_inputs
from panacea_amd import engine as E, hip, synth

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SHAPES = [(1, 8, 8), (3, 64, 64), (37, 320, 320), (33, 64, 192), (4099, 72, 72)]


def launch(hi, lo, rows, cols, ld, rec=None):
    rec = torch.zeros(36, dtype=torch.int64, device=DEV) if rec is None else rec
    hip.operand_stats(hi, lo, rows, cols, ld, rec)
    torch.cuda.synchronize()
    return rec


def padded(values: torch.Tensor, rows, cols, ld, poison: bool):
    """[rows, cols] values inside an allocation of rows * ld + 64 elements; everything else NaN (fp16) / 0xFF = the e4m3 NaN code
    (uint8) when `poison`, else zero.  -> the device tensor whose element 0 is the plane's first one"""
    if values.dtype == torch.float16:
        fill = float("nan") if poison else 0.0
    else:
        fill = 0xFF if poison else 0
    buf = torch.full((rows * ld + 64,), fill, dtype=values.dtype)
    torch.as_strided(buf, (rows, cols), (ld, 1)).copy_(values)
    return buf.to(DEV)


def spread_values(rows, cols, seed):
    """random values times powers of two that span the binades, subnormals and a few overflows to Inf included"""
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(rows, cols, generator=g) * torch.exp2(torch.randint(-26, 15, (rows, cols), generator=g).float())
    return v.to(torch.float16)


def lo_plane(kind, rows, cols, seed):
    g = torch.Generator().manual_seed(1000 + seed)
    if kind == "none":
        return None
    if kind == "f16":
        lo = (torch.randn(rows, cols, generator=g) * 300).to(torch.float16)
        flat = lo.view(-1)
        flat[::7] = float("inf")
        flat[3::11] = float("nan")
        flat[5::13] = -float("inf")
        return lo
    lo = torch.randint(0, 256, (rows, cols), generator=g, dtype=torch.int32).to(torch.uint8)
    return lo


def test_every_fp16_bit_pattern_once():
    g = torch.Generator().manual_seed(0)
    bits = torch.arange(65536, dtype=torch.int32)[torch.randperm(65536, generator=g)]
    hi = torch.from_numpy(bits.numpy().astype(np.uint16).view(np.int16)).view(torch.float16).view(1024, 64)
    want = emu.record(hi, None, 1024, 64, 64)
    assert (want[:32] == 2048).all() and want[32] == 0x7FFF and want[34] == 2046 and want[33] == 0 and want[35] == 65536
    got = launch(hi.to(DEV), None, 1024, 64, 64).cpu().numpy()
    assert np.array_equal(got, want), (got, want)


@pytest.mark.parametrize("kind", ["none", "f16", "e4m3"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_shapes_and_poisoned_padding(shape, kind):
    rows, cols, ld = shape
    hi = spread_values(rows, cols, seed=rows)
    lo = lo_plane(kind, rows, cols, seed=rows)
    want = emu.record(hi, lo, rows, cols, cols)
    assert want[:32].sum() == rows * cols == want[35]
    recs = []
    for poison in (False, True):
        d_hi = padded(hi, rows, cols, ld, poison)
        d_lo = None if lo is None else padded(lo, rows, cols, ld, poison)
        recs.append(launch(d_hi, d_lo, rows, cols, ld).cpu().numpy())
    assert np.array_equal(recs[0], want), (shape, kind, recs[0], want)
    assert np.array_equal(recs[1], want), (shape, kind, "poisoned padding was read", recs[1], want)


def test_lo_planes_with_known_counts():
    rows, cols = 37, 320
    hi = spread_values(rows, cols, seed=5)
    base = emu.record(hi, None, rows, cols, cols)
    assert np.array_equal(launch(hi.to(DEV), None, rows, cols, cols).cpu().numpy(), base) and base[33] == 0
    # e4m3: 0x7E / 0xFE (+-448), 0x7F / 0xFF (the NaN code) count; 0x7D (416) does not
    lo8 = torch.full((rows * cols,), 0x38, dtype=torch.uint8)
    for code, n, start in ((0x7E, 11, 0), (0xFE, 7, 100), (0x7F, 5, 200), (0xFF, 2, 250), (0x7D, 13, 300), (0xFD, 3, 400)):
        lo8[start:start + 3 * n:3] = code
    got = launch(hi.to(DEV), lo8.view(rows, cols).to(DEV), rows, cols, cols).cpu().numpy()
    assert got[33] == 11 + 7 + 5 + 2 and np.array_equal(np.delete(got, 33), np.delete(base, 33))
    # fp16 lo: Inf and NaN count, the largest finite value does not
    lo16 = torch.full((rows * cols,), 1.5, dtype=torch.float16)
    lo16[10:10 + 9] = float("inf")
    lo16[1000:1000 + 4] = -float("inf")
    lo16[5000:5000 + 6] = float("nan")
    lo16[7000:7000 + 17] = 65504.0
    got = launch(hi.to(DEV), lo16.view(rows, cols).to(DEV), rows, cols, cols).cpu().numpy()
    assert got[33] == 9 + 4 + 6 and np.array_equal(np.delete(got, 33), np.delete(base, 33))


def test_accumulation_into_one_record_of_a_table():
    SENT = -0x0123456789ABCDEF
    table = torch.full((3, 40), SENT, dtype=torch.int64)
    table[1, :36] = 0
    table = table.to(DEV)
    a = (torch.randn(33, 64, generator=torch.Generator().manual_seed(1)) * 3).to(torch.float16)            # max in binade ~16
    b = (torch.randn(3, 64, generator=torch.Generator().manual_seed(2)) * 3000).to(torch.float16)          # a larger maximum
    lo_b = torch.full((3, 64), 0x7E, dtype=torch.uint8)
    ra, rb = emu.record(a, None, 33, 64, 64), emu.record(b, lo_b, 3, 64, 64)
    assert rb[32] > ra[32]
    launch(b.to(DEV), lo_b.to(DEV), 3, 64, 64, table[1])
    launch(a.to(DEV), None, 33, 64, 64, table[1])               # the smaller maximum second: word 32 must keep the larger one
    got = table.cpu().numpy()
    want = ra + rb
    want[32] = max(ra[32], rb[32])
    assert np.array_equal(got[1, :36], want)
    assert (got[0] == SENT).all() and (got[2] == SENT).all() and (got[1, 36:] == SENT).all()


# ---- the network
def _ctx_record(inp):
    c = inp["crossattn"].cpu()
    pad = torch.zeros((c.shape[0], E.TEXT_PAD, c.shape[2]), dtype=torch.float16)
    pad[:, :c.shape[1]] = c.to(torch.float16)
    return emu.record(pad.view(-1, c.shape[2]), None, c.shape[0] * E.TEXT_PAD, c.shape[2], c.shape[2])


def _words(S):
    w = np.zeros(36, dtype=np.int64)
    w[:32] = S["binades"]
    w[32] = int(np.array(S["max_abs"], dtype=np.float16).view(np.uint16)) & 0x7FFF
    w[33], w[34], w[35] = S["lo_saturated"], S["nan"], S["elements"]
    return w


def _emulated_site_classes():
    from test_range_profile import stats_emu
    w, _, kw = product_network("tiny")
    inp = step_inputs("tiny", kw)
    m = w.diffusion_model
    m.precision = "precise"
    with stats_emu(), m.profile_ranges() as prof:
        w(inp["x"], inp["t"], cond(inp))
    return {s["site"]: s["class"] for s in prof.report()["sites"]}


def test_tiny_network_profile_changes_no_bit_and_reports_every_split_class():
    w, _, kw = product_network("tiny", DEV)
    inp = step_inputs("tiny", kw, DEV)
    m = w.diffusion_model
    m.precision = "precise"
    off = w(inp["x"], inp["t"], cond(inp))
    with m.profile_ranges() as prof:
        on = w(inp["x"], inp["t"], cond(inp))
    again = w(inp["x"], inp["t"], cond(inp))
    torch.cuda.synchronize()
    assert torch.equal(on, off) and torch.equal(again, off)
    assert "libpanacea_hip.so" in open("/proc/self/maps").read()
    rep, rec = prof.report(), prof.recommend(m)
    print(rec)
    print({c: (S["elements"], S["max_abs"], S["ge_512"], S["lo_saturated"]) for c, S in rep["classes"].items()})
    assert rep["evaluations"] == 1 and len(rep["sites"]) > 100
    # one slot per site: no operand was filed under a class left behind by an earlier allocation at its address — the sites and their
    # classes are those of the same evaluation on the emulated C-ABI (tests/test_range_profile.py holds them to the launches)
    assert len({s["site"] for s in rep["sites"]}) == len(rep["sites"])
    assert {s["site"]: s["class"] for s in rep["sites"]} == _emulated_site_classes()
    occurring = {"stream", "gn_stt", "ff_out", "stem", "gn_head", "gnt"}
    assert occurring == {c for c in E.OPERAND_CLASSES if getattr(E.PRECISE, c)}
    for c in occurring:
        assert rep["classes"][c]["elements"] > 0, c
    for s in rep["sites"]:
        assert sum(s["binades"]) == s["elements"], s["site"]
    one = _ctx_record(inp)
    n_sites = sum(s["class"] == "ctx" for s in rep["sites"])
    want = one * n_sites
    want[32] = one[32]
    assert n_sites == 2 and np.array_equal(_words(rep["classes"]["ctx"]), want)
    assert rec["policy"] == "precise" and rec["headroom_binades"] >= 1


def test_heavy_tail_weights_are_reported_and_precise_wide_recommended():
    w, _, kw = product_network("tiny", "cpu")
    w.diffusion_model.load_state_dict(synth.synth_state_dict(manifest("tiny"), tail=64.0), strict=True)
    w = w.to(DEV)
    inp = step_inputs("tiny", kw, DEV)
    m = w.diffusion_model
    m.precision = "precise"
    with warnings.catch_warnings(), m.profile_ranges() as prof:
        warnings.simplefilter("ignore")
        w(inp["x"], inp["t"], cond(inp))
        clamped = m.lo_clamped
    rep, rec = prof.report(), prof.recommend(m)
    sat = sum(S["lo_saturated"] for S in rep["classes"].values())
    print(rec, "lo_clamped", clamped, "lo_saturated", sat, "stream ge_512", rep["classes"]["stream"]["ge_512"])
    assert clamped > 0
    if clamped > 0:
        assert sat > 0
    assert rep["classes"]["stream"]["ge_512"] > 0
    assert rec["policy"] == "precise-wide" and rec["headroom_binades"] <= 0


def test_profile_refuses_while_capturing():
    w, _, kw = product_network("tiny", DEV)
    m = w.diffusion_model
    buf = torch.zeros(8, device=DEV)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        buf.add_(1.0)
        with pytest.raises(ValueError, match="capturing"):
            with m.profile_ranges():
                pass
    torch.cuda.synchronize()
    assert m.__dict__.get("_profile") is None
