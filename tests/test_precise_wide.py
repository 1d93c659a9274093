"""The `precise-wide` operand policy and on_range_exceeded = "escalate" on CPU: the host logic against the emulated C-ABI
(tests/emu.py) and the reference oracle."""
import dataclasses

import pytest
import torch

import emu
from helpers import cond, manifest, oracle_cfg, product_network, step_inputs
from panacea_amd import engine as E, synth

CLASSES = [f.name for f in dataclasses.fields(E.Precision) if f.name != "lo8"]


@pytest.fixture
def wide_emu():
    with E.use_backend(emu):
        yield


def test_policy_splits_every_class_with_fp16_lo_planes():
    p = E.precision("precise-wide")
    assert p is E.PRECISE_WIDE and not p.lo8
    for c in CLASSES:
        assert getattr(p, c), c
        assert p.lo_dtype(c) == torch.float16, c
    # the existing policies split none of the new classes
    for name in ("fast", "precise", "precise-all", "precise-lite", "precise-f16lo"):
        for c in ("ln", "qkv", "q_text", "kv_text", "ctx", "ff_hidden", "attn_o"):
            assert not getattr(E.precision(name), c), (name, c)
    with pytest.raises(ValueError):
        E.Precision(qkv=True)                    # the attention classes go together


def _tail_case():
    from oracle import panacea_oracle as po
    w, _, kw = product_network("tiny")
    inp = step_inputs("tiny", kw)
    sd_t = synth.synth_state_dict(manifest("tiny"), tail=64.0)
    w.diffusion_model.load_state_dict(sd_t, strict=True)
    ref = po.wrapper_forward(sd_t, oracle_cfg(kw), inp["x"], inp["t"], cond(inp))
    return w, inp, ref


# tiny network, heavy-tail weights (synth tail = 64), emulated C-ABI against the fp32 oracle: `precise` 1.3e-2,
# `precise-wide` 3.9e-5 (measured)
WIDE_TAIL_BOUND = 1e-4


def test_wide_policy_on_heavy_tail_weights(wide_emu):
    w, inp, ref = _tail_case()
    m = w.diffusion_model
    errs = {}
    for p in ("precise", "precise-wide"):
        m.precision = p
        with torch.no_grad():
            errs[p] = (w(inp["x"], inp["t"], cond(inp)) - ref).abs().max().item()
    print(errs)
    assert errs["precise-wide"] <= WIDE_TAIL_BOUND, errs
    assert errs["precise"] >= 10 * errs["precise-wide"], errs
    c = m.eps_contract
    assert c["policy"] == "precise-wide" and c["eps_max_abs"] == 1e-3 and c["valid_for"] == "|operand| < 65504"


def test_escalate_switches_once_and_returns_the_wide_evaluation(wide_emu):
    w, inp, ref = _tail_case()
    m = w.diffusion_model
    m.precision = "precise-wide"
    with torch.no_grad():
        direct = w(inp["x"], inp["t"], cond(inp))
    m.__dict__.pop("_precision")
    m.controlnet.__dict__.pop("_precision", None)
    assert m.precision == "precise" and not m.escalated
    m.on_range_exceeded = "escalate"
    with torch.no_grad():
        e1 = w(inp["x"], inp["t"], cond(inp))
    assert m.escalated and m.precision == "precise-wide" and m.controlnet.precision == "precise-wide"
    assert torch.equal(e1, direct)
    c = m.eps_contract
    assert c["escalated_from"] == "precise" and c["trigger_count"] > 0 and c["policy"] == "precise-wide"
    n = c["trigger_count"]
    with torch.no_grad():
        e2 = w(inp["x"], inp["t"], cond(inp))
    assert torch.equal(e2, direct) and m.eps_contract["trigger_count"] == n          # sticky, no second escalation
    assert (e1 - ref).abs().max().item() <= WIDE_TAIL_BOUND


def test_escalate_on_ordinary_weights_is_warn_bit_for_bit(wide_emu):
    w, _, kw = product_network("tiny")
    inp = step_inputs("tiny", kw)
    m = w.diffusion_model
    with torch.no_grad():
        warn = w(inp["x"], inp["t"], cond(inp))
        m.on_range_exceeded = "escalate"
        esc = w(inp["x"], inp["t"], cond(inp))
    assert not m.escalated and m.lo_clamped == 0
    assert torch.equal(warn, esc)


def test_escalate_rebuilds_the_hoisted_invariants(wide_emu):
    w, inp, _ = _tail_case()
    m = w.diffusion_model
    x = torch.cat([inp["x"], inp["concat"]], dim=1)
    ctx, hint = inp["crossattn"], inp["cond_feat"]
    m.precision = "precise-wide"
    with torch.no_grad():
        inv_w = m.prepare(ctx, hint)
        direct = m.denoise(x, inp["t"], ctx, hint, invariants=inv_w)
    m.__dict__.pop("_precision")
    m.controlnet.__dict__.pop("_precision", None)
    m.on_range_exceeded = "escalate"
    with torch.no_grad():
        inv = m.prepare(ctx, hint)
        assert inv.prec == E.PRECISE and inv.ctx16.lo is None
        got = m.denoise(x, inp["t"], ctx, hint, invariants=inv)
    assert m.escalated
    assert inv.prec == E.PRECISE_WIDE and inv.ctx16.lo is not None           # rebuilt in place under the new policy
    assert torch.equal(got, direct)


def test_graph_capture_refuses_an_unescalated_escalate_network():
    from panacea_amd import graph
    w, _, _ = product_network("tiny")
    w.diffusion_model.on_range_exceeded = "escalate"
    x = torch.zeros(1)
    with pytest.raises(ValueError, match="escalate"):
        graph.GraphedStep(lambda a, b, c: a, x, x, x, network=w)
    with pytest.raises(ValueError, match="escalate"):
        graph.GraphedSchedule(None, None, x, {}, network=w)
    w.diffusion_model.__dict__["_escalated"] = {"from": "precise", "trigger_count": 1}
    graph.refuse_unescalated(w)                  # an escalated network may be captured


@pytest.mark.parametrize("what", ["precise-wide", "escalate"])
def test_sharded_setups_refuse_wide_and_escalate(what):
    from panacea_amd import parallel, sampling
    w, _, kw = product_network("tiny")
    m = w.diffusion_model
    if what == "escalate":
        m.on_range_exceeded = "escalate"
    else:
        m.precision = "precise-wide"
    with pytest.raises(ValueError, match="sharded"):
        parallel.apply_frame_shard(w, E.FrameShard(1, 0))
    with pytest.raises(ValueError, match="sharded"):
        parallel.apply_view_shard(w, E.ViewShard(1, 0))

    class Half:                                  # the CFG half of parallel.ShardedCFG
        half = 0
    with pytest.raises(ValueError, match="sharded"):
        sampling.hoist_invariants(w, Half(), {}, {})
    m.frame_shard = E.FrameShard(1, 0)           # set directly: the evaluation refuses
    inp = step_inputs("tiny", kw)
    with pytest.raises(ValueError, match="sharded"), E.use_backend(emu), torch.no_grad():
        w(inp["x"], inp["t"], cond(inp))


def test_capture_of_an_unescalated_escalate_network_refuses_however_the_graph_is_built(wide_emu, monkeypatch):
    """GraphedStep without `network=`: the evaluation itself refuses while its stream is being captured"""
    from panacea_amd.nn import openaimodel
    w, _, kw = product_network("tiny")
    inp = step_inputs("tiny", kw)
    m = w.diffusion_model
    m.on_range_exceeded = "escalate"
    monkeypatch.setattr(openaimodel, "_capturing", lambda device: True)
    with pytest.raises(ValueError, match="graph replay"), torch.no_grad():
        w(inp["x"], inp["t"], cond(inp))
    m.__dict__["_escalated"] = {"from": "precise", "trigger_count": 1}
    m.precision = "precise-wide"
    with torch.no_grad():
        w(inp["x"], inp["t"], cond(inp))                  # escalated: may be captured


@pytest.mark.parametrize("what", ["precise-wide", "escalate"])
def test_sharded_cfg_refuses_without_hoisting(what):
    from panacea_amd import sampling
    w, _, kw = product_network("tiny")
    m = w.diffusion_model
    if what == "escalate":
        m.on_range_exceeded = "escalate"
    else:
        m.precision = "precise-wide"

    class HalfCFG(sampling.VanillaCFG):                   # the `half` of parallel.ShardedCFG (no process group needed here)
        half = 0
    smp = sampling.EulerEDMSampler(2, guider=HalfCFG(5.0), device="cpu")
    bd = sampling.BoundDenoiser(sampling.DiscreteDenoiser(), w)
    with pytest.raises(ValueError, match="sharded"):
        smp.denoise(torch.zeros(1), bd, torch.ones(1), {}, {})


def test_invariants_keep_their_sources_only_where_the_policy_can_change(wide_emu):
    w, _, kw = product_network("tiny")
    inp = step_inputs("tiny", kw)
    m = w.diffusion_model
    with torch.no_grad():
        inv = m.prepare(inp["crossattn"], inp["cond_feat"])
    assert inv._sources is None                           # "warn": no reference to the (large) hint
    with pytest.raises(ValueError, match="cannot be rebuilt"):
        inv.rebuild(m)
    m.on_range_exceeded = "escalate"
    with torch.no_grad():
        inv = m.prepare(inp["crossattn"], inp["cond_feat"])
    assert inv._sources is not None
