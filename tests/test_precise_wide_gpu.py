"""The `precise-wide` operand policy on the MI355X: the split-operand attention kernels (pnc_attn_views_split_f16,
pnc_attn_temporal_split_f16) against float64 attention of the split values, next to the fp16 kernels on the same inputs, and the
policy / the "escalate" mode at full size on the golden weight sets."""
import pytest
import torch

import emu
from panacea_amd import hip
from panacea_amd.nn.attention import INTER_SEGS, INTRA_SEGS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
S = 1.0 / 2048.0

# measured on the MI355X (max |O - O_ref| / max |O_ref|, operands at |v| ~ 1e3): split kernels 2.0e-7 .. 4.8e-7, fp16 kernels on the
# hi planes of the same inputs 5.9e-4 .. 9.8e-4
SPLIT_BOUND = 4e-6
F16_FLOOR = 5e-5


def _split(v64):
    hi = v64.half()
    lo = ((v64 - hi.double()) * 2048.0).half()
    return hi, lo


def _operands(rows, C, gen, mag, nan_rows=None):
    v = torch.randn(rows, C, generator=gen, dtype=torch.float64) * mag
    hi, lo = _split(v)
    if nan_rows is not None:
        hi[nan_rows] = float("nan")
        lo[nan_rows] = float("nan")
    return hi.to(DEV), lo.to(DEV)


def _rel(got, ref):
    return float((got - ref).abs().max() / ref.abs().max())


def _views_case(groups, heads, H, W, views, segs, kv=None, q_per_kv=1, seed=0):
    """-> (split error, fp16-kernel error).  kv = None: self-attention geometry (keys laid out like the queries); kv = "text":
    80-row key blocks per sample, 77 valid, NaN in the padding"""
    g = torch.Generator().manual_seed(seed)
    C = heads * 64
    M = groups * H * W
    qh, ql = _operands(M, C, g, 2e-3)                      # scores O(1) against keys at |v| ~ 1e3
    if kv == "text":
        nkvg = groups // q_per_kv
        kvH, kvW, kv_views, kv_rows, kv_valid = 1, 80, 1, 80, 77
        pad = torch.cat([torch.arange(77, 80) + 80 * b for b in range(nkvg)])
        kh, kl = _operands(nkvg * 80, C, g, 1e3, pad)
        vh, vl = _operands(nkvg * 80, C, g, 1e3, pad)
    else:
        kvH, kvW, kv_views, kv_rows, kv_valid = H, W, views, H * W, H * (W // views)
        kh, kl = _operands(M, C, g, 1e3)
        vh, vl = _operands(M, C, g, 1e3)
    geo = dict(groups=groups, heads=heads, H=H, W=W, views=views, kvH=kvH, kvW=kvW, kv_views=kv_views, kv_rows_per_group=kv_rows,
               q_per_kv=q_per_kv, kv_valid=kv_valid, segs=segs, scale=0.125)
    o, olo = torch.full((M, C), float("nan"), device=DEV, dtype=torch.float16), torch.empty((M, C), device=DEV, dtype=torch.float16)
    hip.attn_views_split(qh, ql, C, kh, kl, C, vh, vl, C, o, olo, C, **geo)
    torch.cuda.synchronize()
    ref, rows = emu.attn_views_split_exact(*(t.cpu() for t in (qh, ql)), C, *(t.cpu() for t in (kh, kl)), C,
                                           *(t.cpu() for t in (vh, vl)), C, **geo)
    ref = ref.movedim(-3, -2).reshape(-1, C)                # [g * views * nq, C] in the order of rows
    r = rows.reshape(-1).to(DEV)
    got = o[r].double().cpu() + olo[r].double().cpu() * S
    # the fp16 kernel on the hi planes (V^T channel-major, its layout)
    nkv = kh.shape[0] // kv_rows
    vt = torch.nan_to_num(vh).view(nkv, kv_rows, C).transpose(1, 2).contiguous()          # (its padding rows: zeros)
    o16 = torch.empty((M, C), device=DEV, dtype=torch.float16)
    hip.attn_views(qh, C, torch.nan_to_num(kh), C, vt, kv_rows, C * kv_rows, o16, C, **geo)
    torch.cuda.synchronize()
    return _rel(got, ref), _rel(o16[r].double().cpu(), ref)


@pytest.mark.parametrize("name,groups,heads,H,W,views,segs", [
    ("intra", 2, 2, 4, 48, 6, INTRA_SEGS),
    ("intra-ragged", 1, 3, 3, 30, 6, INTRA_SEGS),          # 15 queries / keys per view: partial tiles
    ("cross", 2, 2, 4, 48, 6, INTER_SEGS),                 # view 5 attends view 4 only (one kv segment)
    ("plain", 3, 1, 6, 20, 1, [[0]]),
])
def test_views_split_kernel_vs_float64(name, groups, heads, H, W, views, segs):
    err, err16 = _views_case(groups, heads, H, W, views, segs)
    print(f"{name}: split {err:.2e}  fp16 kernel {err16:.2e}")
    assert err < SPLIT_BOUND, err
    assert err16 > F16_FLOOR and err16 > 20 * err, (err, err16)


def test_views_split_kernel_text_keys_vs_float64():
    # 2 samples x 4 frames of queries, 77 text keys padded to 80 rows, NaN in the padding of K and V (hi and lo)
    err, err16 = _views_case(8, 2, 2, 40, 1, [[0]], kv="text", q_per_kv=4, seed=3)
    print(f"text: split {err:.2e}  fp16 kernel {err16:.2e}")
    assert err < SPLIT_BOUND, err
    assert err16 > F16_FLOOR and err16 > 20 * err, (err, err16)


@pytest.mark.parametrize("B,T,Npix,heads", [(2, 8, 40, 2), (1, 4, 33, 1)])
def test_temporal_split_kernel_vs_float64(B, T, Npix, heads):
    g = torch.Generator().manual_seed(7)
    C = heads * 64
    M = B * T * Npix
    qh, ql = _operands(M, C, g, 2e-3)
    kh, kl = _operands(M, C, g, 1e3)
    vh, vl = _operands(M, C, g, 1e3)
    o, olo = torch.empty((M, C), device=DEV, dtype=torch.float16), torch.empty((M, C), device=DEV, dtype=torch.float16)
    hip.attn_temporal_split(qh, ql, C, kh, kl, C, vh, vl, C, o, olo, C, B=B, T=T, Npix=Npix, heads=heads, scale=0.125)
    o16 = torch.empty((M, C), device=DEV, dtype=torch.float16)
    hip.attn_temporal(qh, C, kh, C, vh, C, o16, C, B=B, T=T, Npix=Npix, heads=heads, scale=0.125)
    torch.cuda.synchronize()
    ref, rows = emu.attn_temporal_split_exact(*(t.cpu() for t in (qh, ql)), C, *(t.cpu() for t in (kh, kl)), C,
                                              *(t.cpu() for t in (vh, vl)), C, B=B, T=T, Npix=Npix, heads=heads, scale=0.125)
    ref = ref.movedim(-3, -2).reshape(-1, C)
    r = rows.reshape(-1).to(DEV)
    err = _rel(o[r].double().cpu() + olo[r].double().cpu() * S, ref)
    err16 = _rel(o16[r].double().cpu(), ref)
    print(f"temporal B{B} T{T}: split {err:.2e}  fp16 kernel {err16:.2e}")
    assert err < SPLIT_BOUND, err
    assert err16 > F16_FLOOR and err16 > 20 * err, (err, err16)


def test_split_kernels_match_the_emulation():
    """the fp32 form of tests/emu.py (what the CPU tests run) against the kernel: the same arithmetic up to fp32 ordering"""
    g = torch.Generator().manual_seed(11)
    heads, C, groups, H, W = 2, 128, 2, 4, 48
    M = groups * H * W
    ops = [_operands(M, C, g, m) for m in (2e-3, 1e3, 1e3)]
    geo = dict(groups=groups, heads=heads, H=H, W=W, views=6, kvH=H, kvW=W, kv_views=6, kv_rows_per_group=H * W, q_per_kv=1,
               kv_valid=H * 8, segs=INTER_SEGS, scale=0.125)
    outs = []
    for dev in (DEV, torch.device("cpu")):
        o, olo = torch.zeros((M, C), device=dev, dtype=torch.float16), torch.zeros((M, C), device=dev, dtype=torch.float16)
        (qh, ql), (kh, kl), (vh, vl) = [(a.to(dev), b.to(dev)) for a, b in ops]
        (hip.attn_views_split if dev.type == "cuda" else emu.attn_views_split)(qh, ql, C, kh, kl, C, vh, vl, C, o, olo, C, **geo)
        outs.append(o.double().cpu() + olo.double().cpu() * S)
    assert _rel(outs[0], outs[1]) < SPLIT_BOUND


# ---- full size (BASELINE config 3: 2 x 8 frames of 32 x 384, 256 x 3072 hint) against the reference's own forward
@pytest.fixture(scope="module")
def full_net():
    from helpers import product_network
    w, _, kw = product_network("full", "cpu")
    return w.to(DEV), kw


def _reset(m):
    """back to the default policy and mode (the module fixture's network is shared)"""
    for net in (m, m.controlnet):
        net.__dict__.pop("_precision", None)
        net.__dict__.pop("_escalated", None)
    m.on_range_exceeded = "warn"


def test_full_size_heavy_tail_pin_wide_and_escalate(full_net):
    """tests/golden/full_cfg3_t500_tail64.npz: residual stream at |v| = 1.8e3, where `precise` measures 2.3e-3"""
    import numpy as np
    from helpers import GOLDEN, cond, err_stats, manifest
    from panacea_amd import synth
    w, kw = full_net
    m = w.diffusion_model
    gp = np.load(GOLDEN / "full_cfg3_t500_tail64.npz")
    assert float(gp["weight_tail"]) == 64.0 and int(gp["t_index"]) == 500
    try:
        m.load_state_dict(synth.synth_state_dict(manifest("full"), salt=0, tail=64.0), strict=True)
        gi = {k: v.to(DEV) for k, v in synth.synth_inputs(2, 8, 32, 384, context_dim=kw["context_dim"], t_index=500).items()}
        m.precision = "precise-wide"
        eps_w = w(gi["x"], gi["t"], cond(gi))
        st = err_stats(eps_w.reshape(-1)[::7], gp["eps_s7"])
        print("tail64 pin, precise-wide:", st)
        assert st["max_abs"] <= 1e-3, st
        _reset(m)
        m.on_range_exceeded = "escalate"
        eps_e = w(gi["x"], gi["t"], cond(gi))
        c = m.eps_contract
        st_e = err_stats(eps_e.reshape(-1)[::7], gp["eps_s7"])
        print("tail64 pin, precise + escalate:", st_e, c)
        assert m.escalated and c["escalated_from"] == "precise" and c["trigger_count"] > 0
        assert st_e["max_abs"] <= 1e-3, st_e
        assert torch.equal(eps_e, eps_w)
    finally:
        _reset(m)
        m.load_state_dict(synth.synth_state_dict(manifest("full")), strict=True)


def test_full_size_cfg3_wide_and_escalate_without_trigger(full_net):
    import numpy as np
    from helpers import GOLDEN, cond, err_stats, step_inputs
    w, kw = full_net
    m = w.diffusion_model
    inp = step_inputs("full", kw, DEV)
    try:
        warn = w(inp["x"], inp["t"], cond(inp))
        m.on_range_exceeded = "escalate"
        esc = w(inp["x"], inp["t"], cond(inp))
        assert not m.escalated and m.lo_clamped == 0
        assert torch.equal(esc, warn)
        _reset(m)
        m.precision = "precise-wide"
        eps = w(inp["x"], inp["t"], cond(inp))
        st = err_stats(eps, np.load(GOLDEN / "full_cfg3.npz")["eps"])
        print("config 3, precise-wide, whole tensor:", st)
        assert st["max_abs"] <= 1e-3, st
    finally:
        _reset(m)


def test_fused_hoisted_schedule_escalating_mid_schedule_matches_wide_from_that_step():
    """Tiny network, heavy-tail weights, 4-step fused + hoisted Euler / CFG schedule (the CFG pair shares ONE hoisted invariants
    object).  The range monitor is switched on after step K - 1, so "escalate" triggers at step K: that step's tokens must come from
    the re-run evaluation and the hoisted invariants must be rebuilt at once.  Reference: the same schedule stepped by hand, under
    `precise` up to step K - 1 and from step K on under `precise-wide` with invariants prepared fresh under that policy."""
    from helpers import manifest, product_network
    from panacea_amd import sampling as Smp, synth
    from test_samplers_gpu import GT, _tiny_inputs
    K, steps, scale = 2, 4, float(GT["cfg_scale"])
    w, _, kw = product_network("tiny", "cpu")
    w.diffusion_model.load_state_dict(synth.synth_state_dict(manifest("tiny"), tail=64.0), strict=True)
    w = w.to(DEV)
    m = w.diffusion_model
    x0, c, uc = _tiny_inputs(kw)
    bd = Smp.BoundDenoiser(Smp.DiscreteDenoiser().to(DEV), w)

    # escalate run
    m.on_range_exceeded, m.range_monitor = "escalate", False
    xs, seen = [], []

    def rec(i, x):
        xs.append(x.detach().clone())
        seen.append(m.escalated)
        if i == K - 1:
            m.range_monitor = True
    smp = Smp.EulerEDMSampler(steps, guider=Smp.VanillaCFG(scale), device=DEV)
    assert smp._fusable(bd, x0, c)
    with torch.no_grad():
        smp(bd, x0.clone(), c, uc, network=w, callback=rec)
    torch.cuda.synchronize()
    assert seen == [False] * K + [True] * (steps - K), seen            # escalated AT step K, not before, not later
    esc = m.eps_contract
    assert esc["escalated_from"] == "precise" and esc["trigger_count"] > 0, esc

    # reference: precise for steps 0 .. K-1, precise-wide (fresh invariants) from step K on
    _reset(m)
    m.range_monitor = False
    smp = Smp.EulerEDMSampler(steps, guider=Smp.VanillaCFG(scale), device=DEV)
    sig = smp.sigmas()
    s_in = x0.new_ones([x0.shape[0]])
    ref = []
    with torch.no_grad():
        x = x0.clone() * torch.sqrt(1.0 + sig[0] ** 2.0)
        cp, up = Smp.hoist_invariants(w, smp.guider, c, uc)
        for i in range(steps):
            if i == K:
                m.precision = "precise-wide"
                cp, up = Smp.hoist_invariants(w, smp.guider, c, uc)
            x = smp.sampler_step(s_in * sig[i], s_in * sig[i + 1], bd, x, cp, up)
            ref.append(x.detach().clone())
    torch.cuda.synchronize()
    m.range_monitor = True
    _reset(m)
    m._range_count_sync(torch.device(DEV))       # drain the counts the unmonitored steps left in the library for later tests
    for i, (a, b) in enumerate(zip(xs, ref)):
        assert torch.equal(a, b), (i, (a - b).abs().max().item())
