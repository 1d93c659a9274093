"""The `precise-ckpt` operand policy (`precise`'s operand classes and e4m3 lo planes + split weights beside the launch,
pnc_gemm_wsplit_f16) on CPU: the host logic against the emulated C-ABI (tests/emu.py) and
tests/golden/tiny_w32.npz — the reference's own fp32 forward of the `tiny` network on weights that are NOT fp16-representable."""
import dataclasses

import pytest
import torch

import emu
from helpers import cond, golden, manifest, product_network, step_inputs
from panacea_amd import engine as E, synth

OTHER_POLICIES = ("fast", "precise", "precise-all", "precise-lite", "precise-f16lo", "precise-wide", "precise-full")


@pytest.fixture
def ckpt_emu():
    with E.use_backend(emu):
        yield


def _w32_network():
    """the tiny product network on the unrounded synthetic weights + its step inputs"""
    w, _, kw = product_network("tiny")
    sd = synth.synth_state_dict(manifest("tiny"), round_fp16=False)
    w.diffusion_model.load_state_dict(sd, strict=True)
    return w, kw, step_inputs("tiny", kw)


def _twins(net):
    out = [m for m in net.modules() if isinstance(m, E.Packable) and m._pk_lo is not None]
    for m in net.modules():
        for name in ("_text_proj", "_emb_proj"):
            pr = m.__dict__.get(name)
            if pr is not None and getattr(pr, "_pk_lo", None) is not None:
                out.append(pr)
    return out


def test_precise_ckpt_holds_the_contract_on_unrounded_weights(ckpt_emu):
    w, _, inp = _w32_network()
    ref = torch.from_numpy(golden("tiny_w32")["eps"])
    m = w.diffusion_model
    errs = {}
    for p in ("precise", "precise-ckpt"):
        m.precision = p
        with torch.no_grad():
            errs[p] = (w(inp["x"], inp["t"], cond(inp)) - ref).abs().max().item()
    print("eps max-abs vs tiny_w32 (emulated C-ABI, unrounded weights):", errs)
    assert errs["precise-ckpt"] <= 1e-3, errs
    assert errs["precise"] >= 2 * errs["precise-ckpt"], errs
    c = m.eps_contract
    assert c["policy"] == "precise-ckpt" and c["eps_max_abs"] == 1e-3 and "|v| < 512" in c["valid_for"]
    assert c["weights"].startswith("split") and "text tower" in c["note"] and "VAE" in c["note"]
    m.precision = "precise"
    assert "weights" not in m.eps_contract                     # `precise` states what it stated


def test_policy_definition_and_refusals():
    p = E.precision("precise-ckpt")
    assert p is E.PRECISE_CKPT and type(p) is E.WeightsBeside and p.weights and p.beside and p.lo8
    assert not isinstance(p, E.SplitWeights) and p != E.PRECISE and not E.is_wide(p) and not E.is_wide("precise-ckpt")
    assert E.weights_beside(p) and E.single_device_only(p)
    # the operand classes and lo-plane formats are exactly `precise`'s
    assert dataclasses.asdict(p) == dataclasses.asdict(E.PRECISE)
    assert all(p.lo_dtype(c) == E.PRECISE.lo_dtype(c) for c in E.OPERAND_CLASSES)
    for name in OTHER_POLICIES:
        assert not E.weights_beside(name) and not E.precision(name).beside, name
    assert E.single_device_only("precise-wide") and E.single_device_only("precise-full") and not E.single_device_only("precise")
    # partial or foreign class sets are refused
    for other in (E.PRECISE_F16LO, E.PRECISE_ALL, E.PRECISE_LITE, E.PRECISE_WIDE, E.FAST):
        with pytest.raises(ValueError, match="exactly the operand classes"):
            E.WeightsBeside(**dataclasses.asdict(other))
    with pytest.raises(ValueError, match="exactly the operand classes"):
        dataclasses.replace(p, gnt=False)
    with pytest.raises(ValueError, match="exactly the operand classes"):
        dataclasses.replace(p, lo8=False)
    with pytest.raises(ValueError):
        E.WeightsBeside()


def test_sharded_setups_refuse_precise_ckpt():
    from panacea_amd import parallel, sampling
    w, _, kw = product_network("tiny")
    m = w.diffusion_model
    m.precision = "precise-ckpt"
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


def test_escalate_targets():
    w, _, _ = product_network("tiny")
    m = w.diffusion_model
    m.precision = "precise-ckpt"
    m._escalate(1)
    assert m.precision == "precise-full" and E.precision(m.precision).weights and m.escalated
    assert m.eps_contract["escalated_from"] == "precise-ckpt" and m.eps_contract["weights"].startswith("split")
    w, _, _ = product_network("tiny")
    m = w.diffusion_model
    m.precision = "precise"
    m._escalate(1)
    assert m.precision == "precise-wide" and not E.precision(m.precision).weights


def test_every_weight_consumer_receives_its_twin_and_no_other_policy_allocates_one(ckpt_emu, monkeypatch):
    w, _, inp = _w32_network()
    m = w.diffusion_model
    calls = {"gemm": 0, "gemm_lo": 0, "gemm_a8": 0, "gemm_a16": 0, "gemm_a0": 0, "small": 0, "small_lo": 0}

    def is_twin(t, w16):
        return isinstance(t, torch.Tensor) and t.dtype == torch.float16 and t.shape == w16.shape

    def count_gemm(fn):
        def wrapped(a16, w16, **k):
            if w16.dtype == torch.float16:
                calls["gemm"] += 1
                calls["gemm_lo"] += int(is_twin(k.get("w_lo16"), w16))
                a_lo = k.get("a16_lo")
                calls["gemm_a0" if a_lo is None else ("gemm_a8" if a_lo.dtype == torch.uint8 else "gemm_a16")] += 1
                if k.get("w_lo16") is not None:              # `w_lo` keeps its e4m3 meaning and nothing else
                    assert (a_lo is not None and a_lo.dtype == torch.uint8) == (k.get("w_lo") is not None)
                    assert k.get("w_lo") is None or isinstance(k["w_lo"], tuple)
            return fn(a16, w16, **k)
        monkeypatch.setattr(emu, "gemm", wrapped)

    def count_small(name, fn):
        def wrapped(*a, **k):
            calls["small"] += 1
            calls["small_lo"] += int(is_twin(k.get("w_lo"), a[2]))
            return fn(*a, **k)
        monkeypatch.setattr(emu, name, wrapped)
    count_gemm(emu.gemm)
    count_small("linear_smallm", emu.linear_smallm)
    count_small("linear_smallm_segments", emu.linear_smallm_segments)
    for p in ("fast", "precise", "precise-all", "precise-lite", "precise-f16lo", "precise-wide"):
        m.precision = p
        with torch.no_grad():
            w(inp["x"], inp["t"], cond(inp))
        assert calls["gemm_lo"] == 0 and calls["small_lo"] == 0 and not _twins(m), p
    for k in calls:
        calls[k] = 0
    m.precision = "precise-ckpt"
    with torch.no_grad():
        w(inp["x"], inp["t"], cond(inp))
    print(calls)
    assert calls["gemm"] > 100 and calls["gemm_lo"] == calls["gemm"], calls
    assert calls["gemm_a0"] > 0 and calls["gemm_a8"] > 0 and calls["gemm_a16"] > 0, calls       # every state of a.lo occurs
    assert calls["small"] > 0 and calls["small_lo"] == calls["small"], calls
    assert _twins(m)


def test_hoisted_invariants_run_under_precise_ckpt(ckpt_emu):
    w, _, inp = _w32_network()
    m = w.diffusion_model
    m.precision = "precise-ckpt"
    x = torch.cat([inp["x"], inp["concat"]], dim=1)
    ctx, hint = inp["crossattn"], inp["cond_feat"]
    with torch.no_grad():
        plain = m.denoise(x, inp["t"], ctx, hint)
        inv = m.prepare(ctx, hint)
        assert inv.prec == E.PRECISE_CKPT
        hoisted = m.denoise(x, inp["t"], ctx, hint, invariants=inv)
    assert torch.equal(plain, hoisted)


def test_zero_twins_give_the_bits_of_precise(ckpt_emu):
    """fp16-representable weights have all-zero lo twins: the policy then computes what `precise` computes, bit for bit"""
    w, _, kw = product_network("tiny")
    inp = step_inputs("tiny", kw)
    m = w.diffusion_model
    out = {}
    for p in ("precise", "precise-ckpt"):
        m.precision = p
        with torch.no_grad():
            out[p] = w(inp["x"], inp["t"], cond(inp))
    assert torch.equal(out["precise"], out["precise-ckpt"])
