"""The operand range profile (UNetModel3D.profile_ranges -> engine.RangeProfile) on the CPU: the host logic over the emulated C-ABI
(tests/emu.py) on the `tiny` network.  Counts are integers: every comparison is exact.

The independent side of the comparisons is a wrapper around emu.gemm that keeps a copy of the A operand of every launch of one
evaluation, resolves the launch's site from the WEIGHT pointer (the packed dicts of the network's modules, walked after the run) and
computes the statistics with torch integer ops — neither engine.RangeProfile's site naming nor emu.record's numpy."""
import contextlib
import ctypes
import math
import warnings

import pytest
import torch

import emu
from helpers import cond, golden, manifest, product_network, step_inputs
from panacea_amd import engine as E, hip, synth


@contextlib.contextmanager
def stats_emu(operand_stats=None, gemm=None):
    """the emu backend, optionally with a spy in the place of `operand_stats` and / or `gemm`"""
    old = (emu.operand_stats, emu.gemm)
    emu.operand_stats, emu.gemm = operand_stats or old[0], gemm or old[1]
    try:
        with E.use_backend(emu), torch.no_grad():
            yield
    finally:
        emu.operand_stats, emu.gemm = old


def _never(*a, **k):
    raise AssertionError("operand_stats was called with the range profile off")


def torch_stats(hi, lo, rows, cols, ld):
    """the 36 words of one operand, with torch integer ops"""
    bits = emu._mat(hi, rows, cols, ld).contiguous().view(torch.int16).to(torch.int64) & 0x7FFF
    w = torch.zeros(36, dtype=torch.int64)
    w[:32] = torch.bincount((bits >> 10).reshape(-1), minlength=32)
    w[32] = bits.max()
    w[34] = (bits > 0x7C00).sum()
    w[35] = rows * cols
    if lo is not None and lo.dtype == torch.uint8:
        w[33] = ((emu._mat(lo, rows, cols, ld).to(torch.int64) & 0x7F) >= 0x7E).sum()
    elif lo is not None:
        lb = emu._mat(lo, rows, cols, ld).contiguous().view(torch.int16).to(torch.int64)
        w[33] = ((lb & 0x7C00) == 0x7C00).sum()
    return w


def add_words(a, b):
    out = a + b
    out[32] = max(int(a[32]), int(b[32]))
    return out


def as_words(S):
    """a report entry S -> the 36 words it was made from (max_abs back to its bit pattern)"""
    w = torch.zeros(36, dtype=torch.int64)
    w[:32] = torch.tensor(S["binades"])
    m = S["max_abs"]
    w[32] = 0x7E00 if math.isnan(m) else int(torch.tensor(m, dtype=torch.float16).view(torch.int16))
    w[33], w[34], w[35] = S["lo_saturated"], S["nan"], S["elements"]
    assert S["ge_512"] == sum(S["binades"][24:]) and S["inf"] == S["binades"][31] - S["nan"]
    return w


class Capture:
    """wraps emu.gemm: the words of the A operand of every launch, keyed by the weight tensor's pointer"""

    def __init__(self):
        self.inner = emu.gemm
        self.words = {}           # weight data_ptr -> summed words
        self.lo_dtype = {}        # weight data_ptr -> set of lo-plane dtypes seen (None: no lo plane)

    def __call__(self, a16, w16, **kw):
        mode = kw.get("a_mode", emu.A_PLAIN)
        if mode == emu.A_PLAIN:
            rows, cols, ld = kw["M"], kw["K"], kw["lda"]
        elif mode == emu.A_CONV3X3:
            c = kw["conv"]
            cols = ld = c["Cin"]
            rows = kw["M"] // (c["Hout"] * c["Wout"]) * c["Hin"] * c["Win"]
        else:
            cols = ld = kw["tconv"]["C"]
            rows = kw["M"]
        lo = kw.get("a16_lo")
        w = torch_stats(a16, lo, rows, cols, ld)
        p = w16.data_ptr()
        self.words[p] = add_words(self.words[p], w) if p in self.words else w
        self.lo_dtype.setdefault(p, set()).add(None if lo is None else lo.dtype)
        return self.inner(a16, w16, **kw)


def weight_sites(net):
    """weight data_ptr -> site name, from the packed dicts of the network's modules (and the stacked text K/V matrices)"""
    out = {}

    def walk(mod, v, path):
        if isinstance(v, torch.Tensor):
            if v.dtype == torch.float16:
                out[v.data_ptr()] = ".".join(x for x in (mod, *map(str, path)) if x)
        elif isinstance(v, tuple) and v and isinstance(v[0], torch.Tensor):
            walk(mod, v[0], path)                          # a (weight, bias) entry: the key names the pair
        elif isinstance(v, dict):
            for k, x in v.items():
                if not (isinstance(k, tuple) and k[-1] == "lo8"):
                    walk(mod, x, path + (k,))
        elif isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                walk(mod, x, path + (i,))
    for name, m in net.named_modules():
        if isinstance(m, E.Packable) and m._pk is not None:
            walk(name, m._pk, ())
        tp = m.__dict__.get("_text_proj")
        if tp is not None and tp._pk is not None:
            out[tp._pk[0].data_ptr()] = ".".join(x for x in (name, "text_kv") if x)
    return out


def ctx_words(inp):
    c = inp["crossattn"]
    pad = torch.zeros((c.shape[0], E.TEXT_PAD, c.shape[2]), dtype=torch.float16)
    pad[:, :c.shape[1]] = c.to(torch.float16)
    return torch_stats(pad.view(-1, c.shape[2]), None, c.shape[0] * E.TEXT_PAD, c.shape[2], c.shape[2])


@pytest.fixture(scope="module")
def precise_run():
    """`tiny` under `precise`: one evaluation with the profile off (operand_stats raises), one with it on and every A operand captured"""
    w, _, kw = product_network("tiny")
    inp = step_inputs("tiny", kw)
    m = w.diffusion_model
    m.precision = "precise"
    with stats_emu(operand_stats=_never):
        eps_off = w(inp["x"], inp["t"], cond(inp))
    cap = Capture()
    with stats_emu(gemm=cap):
        with m.profile_ranges() as prof:
            eps_on = w(inp["x"], inp["t"], cond(inp))
        rep = prof.report()
        rec = prof.recommend(m)
    return dict(w=w, m=m, inp=inp, eps_off=eps_off, eps_on=eps_on, cap=cap, rep=rep, rec=rec, sites=weight_sites(m))


def test_profile_off_launches_nothing_and_profile_on_changes_no_bit(precise_run):
    r = precise_run
    assert torch.equal(r["eps_off"], r["eps_on"])
    assert r["rep"]["evaluations"] == 1
    assert r["m"].__dict__.get("_profile") is None and r["m"].controlnet.__dict__.get("_profile") is None


def test_report_equals_independent_statistics_per_site_and_class(precise_run):
    r = precise_run
    cap, rep, sites = r["cap"], r["rep"], r["sites"]
    assert len(cap.words) > 100 and set(cap.words) <= set(sites)
    want = {sites[p]: w for p, w in cap.words.items()}
    assert len(want) == len(cap.words)                                   # distinct (module, key) launches have distinct names
    assert len(rep["sites"]) == len(want)                                # ... and each is one site of the report
    got = {s["site"]: s for s in rep["sites"]}
    assert set(got) == set(want)
    by_class = {}
    for name, s in got.items():
        assert torch.equal(as_words(s), want[name]), name
        by_class[s["class"]] = add_words(by_class[s["class"]], want[name]) if s["class"] in by_class else want[name]
    assert set(by_class) == set(rep["classes"])
    for c, wsum in by_class.items():
        assert torch.equal(as_words(rep["classes"][c]), wsum), c
    mx = [as_words(s)[32].item() for s in rep["sites"]]
    assert mx == sorted(mx, reverse=True)                                # widest site first
    assert any(n.startswith("controlnet.") for n in got) and "text_kv" in got and "controlnet.text_kv" in got


def test_ctx_class_is_the_padded_fp16_context(precise_run):
    r = precise_run
    n_sites = sum(s["class"] == "ctx" for s in r["rep"]["sites"])
    assert n_sites == 2                                                  # the text K/V GEMM of the UNet and of its ControlNet
    one = ctx_words(r["inp"])
    want = one * n_sites
    want[32] = one[32]
    assert torch.equal(as_words(r["rep"]["classes"]["ctx"]), want)


def test_classes_follow_the_lo_planes(precise_run):
    r = precise_run
    cls = {s["site"]: s["class"] for s in r["rep"]["sites"]}
    seen8 = 0
    for p, dts in r["cap"].lo_dtype.items():
        c = cls[r["sites"][p]]
        if torch.uint8 in dts:
            assert c in E.LO8_CLASSES, (r["sites"][p], c)
            seen8 += 1
        if c == "unsplit":
            assert dts == {None}, r["sites"][p]
        if dts != {None}:
            assert getattr(E.PRECISE, c), (r["sites"][p], c)            # a lo plane only under a class the policy splits
    assert seen8 > 20
    occurring = {c for c in E.OPERAND_CLASSES if getattr(E.PRECISE, c)} & set(r["rep"]["classes"])
    assert {"stream", "gn_stt", "ff_out", "stem", "gn_head", "gnt"} <= occurring
    assert all(r["rep"]["classes"][c]["elements"] > 0 for c in occurring)


def test_fast_reports_the_same_classes_without_lo_planes(precise_run):
    r = precise_run
    w, m, inp = r["w"], r["m"], r["inp"]
    m.precision = "fast"
    try:
        with stats_emu(), m.profile_ranges() as prof:
            w(inp["x"], inp["t"], cond(inp))
        rep = prof.report()
    finally:
        m.precision = "precise"
    assert set(rep["classes"]) == set(r["rep"]["classes"])
    assert {s["site"]: s["class"] for s in rep["sites"]} == {s["site"]: s["class"] for s in r["rep"]["sites"]}
    assert all(S["lo_saturated"] == 0 for S in rep["classes"].values())


def test_recommends_precise_on_fp16_weights(precise_run):
    rec = precise_run["rec"]
    print(rec)
    assert rec["policy"] == "precise" and rec["headroom_binades"] >= 1


def test_recommends_precise_ckpt_on_unrounded_weights():
    """the weights behind tests/golden/tiny_w32.npz: the synthetic set of the fixture's `salt` without its fp16 rounding
    (tools/gen_golden_w32.py).  That these ARE the fixture's weights is checked on its eps: the recommended policy, run on them through
    the emulation of its entry points, holds its own 1e-3 contract against the reference's fp32 forward stored there."""
    gold = golden("tiny_w32")
    w, _, kw = product_network("tiny")
    m = w.diffusion_model
    m.load_state_dict(synth.synth_state_dict(manifest("tiny"), salt=int(gold["salt"]), round_fp16=False), strict=True)
    m.precision = "precise"
    inp = step_inputs("tiny", kw)
    with stats_emu(), m.profile_ranges() as prof:
        w(inp["x"], inp["t"], cond(inp))
    rec = prof.recommend(m)
    print(rec)
    assert rec["policy"] == "precise-ckpt" and rec["headroom_binades"] >= 1
    m.precision = rec["policy"]
    with stats_emu():
        eps = w(inp["x"], inp["t"], cond(inp))
    err = (eps - torch.from_numpy(gold["eps"])).abs().max().item()
    print("eps max-abs vs tiny_w32 under the recommended policy:", err)
    assert err <= m.eps_contract["eps_max_abs"] == 1e-3


def test_recommends_precise_wide_on_the_heavy_tail_weights():
    w, _, kw = product_network("tiny")
    m = w.diffusion_model
    m.load_state_dict(synth.synth_state_dict(manifest("tiny"), tail=64.0), strict=True)
    m.precision = "precise"
    inp = step_inputs("tiny", kw)
    with stats_emu(), warnings.catch_warnings(), m.profile_ranges() as prof:
        warnings.simplefilter("ignore")
        w(inp["x"], inp["t"], cond(inp))
        clamped = m.lo_clamped
    rep, rec = prof.report(), prof.recommend(m)
    print(rec, clamped, rep["classes"]["stream"]["ge_512"], rep["classes"]["stream"]["lo_saturated"])
    assert clamped > 0 and rep["classes"]["stream"]["ge_512"] > 0
    assert sum(S["lo_saturated"] for S in rep["classes"].values()) > 0
    assert rec["policy"] == "precise-wide" and rec["headroom_binades"] <= 0 and "stream" in rec["reason"]


def test_nan_in_the_latent_leaves_no_policy():
    w, _, kw = product_network("tiny")
    m = w.diffusion_model
    m.precision = "precise"
    inp = step_inputs("tiny", kw)
    x = inp["x"].clone()
    x[0, 0, 0, 0] = float("nan")
    with stats_emu(), warnings.catch_warnings(), m.profile_ranges() as prof:
        warnings.simplefilter("ignore")
        w(x, inp["t"], cond(inp))
    rep, rec = prof.report(), prof.recommend(m)
    print(rec)
    assert rec["policy"] is None
    assert math.isnan(rep["sites"][0]["max_abs"]) and rep["sites"][0]["nan"] > 0
    assert any(s["nan"] > 0 and f"'{s['site']}'" in rec["reason"] for s in rep["sites"])
    assert rep["classes"]["stem"]["nan"] > 0


def test_sharded_networks_refuse_the_profile():
    w, _, kw = product_network("tiny")
    m = w.diffusion_model
    for attr, shard in (("frame_shard", E.FrameShard(1, 0)), ("view_shard", E.ViewShard(1, 0))):
        setattr(m, attr, shard)
        with pytest.raises(ValueError, match="sharded"):
            with m.profile_ranges():
                pass
        setattr(m, attr, None)
    m.controlnet.view_shard = E.ViewShard(1, 0)
    with pytest.raises(ValueError, match="sharded"):
        with m.profile_ranges():
            pass
    m.controlnet.view_shard = None
    # a shard set after the profile was started: the evaluation refuses
    inp = step_inputs("tiny", kw)
    with stats_emu(), m.profile_ranges():
        m.frame_shard = m.controlnet.frame_shard = E.FrameShard(1, 0)
        with pytest.raises(ValueError, match="sharded"):
            w(inp["x"], inp["t"], cond(inp))
    assert m.__dict__.get("_profile") is None


def test_entry_point_checks_its_arguments_before_any_launch():
    """no device needed: every refusal below returns before a launch.  ABI version 8, header symbols = the binding's."""
    lib = hip.load()
    assert lib.pnc_abi_version() == 8 == hip.ABI_VERSION
    assert set(hip.header_symbols()) == set(hip._SIGNATURES) and "pnc_operand_stats_f16" in hip._SIGNATURES
    buf = (ctypes.c_char * 256)()
    a16 = (ctypes.addressof(buf) + 15) & ~15
    ok, rec = ctypes.c_void_p(a16), ctypes.c_void_p(a16 + 64)
    f = lib.pnc_operand_stats_f16
    EINVAL, EALIGN = -1, -2
    for args, want in (
            ((None, None, hip.LO_F16, 1, 8, 8, rec), EINVAL),                       # NULL hi
            ((ok, None, hip.LO_F16, 1, 8, 8, None), EINVAL),                        # NULL rec
            ((ok, None, hip.LO_F16, 0, 8, 8, rec), EINVAL),                         # rows < 1
            ((ok, None, hip.LO_F16, 1, 0, 8, rec), EINVAL),                         # cols < 1
            ((ok, None, hip.LO_F16, 1, 16, 8, rec), EINVAL),                        # ld < cols
            ((ok, ok, 7, 1, 8, 8, rec), EINVAL),                                    # unknown lo_fmt with a lo plane
            ((ok, None, hip.LO_F16, 1, 12, 16, rec), EALIGN),                       # cols % 8
            ((ok, None, hip.LO_F16, 1, 8, 12, rec), EALIGN),                        # ld % 8
            ((ctypes.c_void_p(a16 + 8), None, hip.LO_F16, 1, 8, 8, rec), EALIGN),   # hi not 16-byte aligned
            ((ok, ctypes.c_void_p(a16 + 8), hip.LO_F16, 1, 8, 8, rec), EALIGN),     # fp16 lo: 8 elements = 16 bytes
            ((ok, ctypes.c_void_p(a16 + 4), hip.LO_E4M3, 1, 8, 8, rec), EALIGN),    # e4m3 lo: 8 elements = 8 bytes
            ((ok, None, hip.LO_F16, 1, 8, 8, ctypes.c_void_p(a16 + 68)), EALIGN),   # rec not 8-byte aligned
    ):
        assert f(*args, None) == want, args


def test_profile_refuses_while_a_stream_is_capturing(monkeypatch):
    from panacea_amd.nn import openaimodel
    w, _, kw = product_network("tiny")
    m = w.diffusion_model
    inp = step_inputs("tiny", kw)
    with stats_emu(), m.profile_ranges():
        monkeypatch.setattr(openaimodel, "_capturing", lambda device: True)      # a capture that starts inside the context
        with pytest.raises(ValueError, match="capturing"):
            w(inp["x"], inp["t"], cond(inp))
    with pytest.raises(ValueError, match="capturing"):
        with m.profile_ranges():
            pass
    assert m.__dict__.get("_profile") is None


def test_evaluation_limit_and_hoisted_invariants(precise_run):
    """`evaluations=1`: the second evaluation of the context launches no statistics; both give the unprofiled bits, hoisted or not"""
    r = precise_run
    w, m, inp = r["w"], r["m"], r["inp"]
    x = torch.cat([inp["x"], inp["concat"]], dim=1)
    calls = []

    real = emu.operand_stats

    def counting(*a):
        calls.append(1)
        return real(*a)
    with stats_emu(operand_stats=counting), m.profile_ranges(evaluations=1) as prof:
        inv = m.prepare(inp["crossattn"], inp["cond_feat"])
        n_prepare = len(calls)
        e1 = m.denoise(x, inp["t"], inp["crossattn"], inp["cond_feat"], invariants=inv)
        n_first = len(calls)
        e2 = m.denoise(x, inp["t"], inp["crossattn"], inp["cond_feat"], invariants=inv)
    assert n_prepare > 0 and n_first > n_prepare and len(calls) == n_first
    assert torch.equal(e1, r["eps_off"]) and torch.equal(e2, r["eps_off"])
    rep = prof.report()
    assert rep["evaluations"] == 1 and rep["classes"]["ctx"]["elements"] == r["rep"]["classes"]["ctx"]["elements"]
