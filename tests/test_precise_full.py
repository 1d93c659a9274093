"""The `precise-full` operand policy (precise-wide + split weights, PncGemmParams.W_lo) on CPU: the host logic against the emulated
C-ABI (tests/emu.py), the oracle and tests/golden/tiny_w32.npz — the reference's own fp32
forward of the `tiny` network on weights that are NOT fp16-representable (tools/gen_golden_w32.py)."""
import dataclasses

import numpy as np
import pytest
import torch

import emu
from helpers import cond, golden, manifest, oracle_cfg, product_network, step_inputs
from panacea_amd import engine as E, synth

OLD_POLICIES = ("fast", "precise", "precise-all", "precise-lite", "precise-f16lo", "precise-wide")


@pytest.fixture
def full_emu():
    with E.use_backend(emu):
        yield


def _w32_network():
    """the tiny product network on the unrounded synthetic weights + its step inputs"""
    w, _, kw = product_network("tiny")
    sd = synth.synth_state_dict(manifest("tiny"), round_fp16=False)
    w.diffusion_model.load_state_dict(sd, strict=True)
    return w, sd, kw, step_inputs("tiny", kw)


def _twins(net):
    """every lo twin allocated below `net`: Packable._pk_lo and the two projector caches"""
    out = [m for m in net.modules() if isinstance(m, E.Packable) and m._pk_lo is not None]
    for m in net.modules():
        for name in ("_text_proj", "_emb_proj"):
            pr = m.__dict__.get(name)
            if pr is not None and getattr(pr, "_pk_lo", None) is not None:
                out.append(pr)
    return out


def test_unrounded_weights_are_not_fp16_representable_and_default_is_unchanged():
    man = manifest("tiny")
    a, b = synth.synth_state_dict(man), synth.synth_state_dict(man, round_fp16=False)
    k = "input_blocks.1.0.in_layers.2.weight"
    assert torch.equal(a[k], a[k].half().float()) and a[k].dtype == torch.float32
    assert b[k].dtype == torch.float32 and not torch.equal(b[k], b[k].half().float())
    assert torch.equal(b[k].half().float(), a[k])                  # the same stream, one rounding apart
    assert torch.equal(synth.synth_tensor(k, man[k]), a[k])


def test_oracle_on_unrounded_weights_matches_the_reference_golden():
    _, sd, kw, inp = _w32_network()
    eps = __import__("oracle.panacea_oracle", fromlist=["x"]).wrapper_forward(sd, oracle_cfg(kw), inp["x"], inp["t"], cond(inp))
    d = np.abs(eps.numpy() - golden("tiny_w32")["eps"]).max()
    print(f"oracle vs tiny_w32: {d:.3e}")
    assert d <= 2e-5


def test_precise_full_holds_the_contract_on_unrounded_weights(full_emu):
    w, _, _, inp = _w32_network()
    ref = torch.from_numpy(golden("tiny_w32")["eps"])
    m = w.diffusion_model
    errs = {}
    for p in ("precise-wide", "precise-full"):
        m.precision = p
        with torch.no_grad():
            errs[p] = (w(inp["x"], inp["t"], cond(inp)) - ref).abs().max().item()
    print("eps max-abs vs tiny_w32 (emulated C-ABI, unrounded weights):", errs)
    assert errs["precise-full"] <= 1e-3, errs
    assert errs["precise-wide"] >= 2 * errs["precise-full"], errs
    c = m.eps_contract
    assert c["policy"] == "precise-full" and c["eps_max_abs"] == 1e-3 and c["valid_for"] == "|operand| < 65504"
    assert c["weights"].startswith("split")


def test_policy_definition_and_refusals():
    p = E.precision("precise-full")
    assert p is E.PRECISE_FULL and p.weights and not p.lo8
    assert E.Precision(**{k: v for k, v in dataclasses.asdict(p).items() if k != "weights"}) == E.PRECISE_WIDE and p != E.PRECISE_WIDE
    for name in OLD_POLICIES:
        assert not E.precision(name).weights, name
    assert E.PRECISIONS["precise"] is E.PRECISE
    with pytest.raises(ValueError, match="lo8"):
        E.SplitWeights(**dataclasses.asdict(E.PRECISE_ALL))        # lo8
    with pytest.raises(ValueError, match="every operand class"):
        E.SplitWeights(**dataclasses.asdict(E.PRECISE_F16LO))      # partial splits
    with pytest.raises(ValueError, match="every operand class"):
        dataclasses.replace(E.PRECISE_FULL, ff_hidden=False)
    with pytest.raises(ValueError):
        E.SplitWeights()
    assert not dataclasses.replace(E.PRECISE_FULL, weights=False).weights      # = precise-wide's behaviour
    # ... and the shards refuse it like precise-wide: what they ask is structural (every class split, fp16 lo planes)
    assert E.is_wide(dataclasses.replace(E.PRECISE_FULL, weights=False)) and E.is_wide("precise-wide") and E.is_wide(p)
    assert not any(E.is_wide(n) for n in OLD_POLICIES if n != "precise-wide")


def test_sharded_setups_refuse_precise_full():
    from panacea_amd import parallel, sampling
    w, _, kw = product_network("tiny")
    m = w.diffusion_model
    m.precision = "precise-full"
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


def test_escalate_still_targets_precise_wide():
    w, _, _ = product_network("tiny")
    m = w.diffusion_model
    m._escalate(1)
    assert m.precision == "precise-wide" and not E.precision(m.precision).weights


def test_lo_twins_have_the_layout_of_their_hi_planes_and_follow_the_parameters():
    from panacea_amd.nn.openaimodel import ResBlock3D
    from panacea_amd.nn.attention import FeedForward
    w, _, _, _ = _w32_network()
    net = w.diffusion_model
    rb = next(m for m in net.modules() if isinstance(m, ResBlock3D))
    ff = next(m for m in net.modules() if isinstance(m, FeedForward))
    stem = net.input_blocks[0]
    assert not _twins(net)
    for mod, keys in ((rb, ("w1", "wt1", "we", "w2", "wt2")), (ff, ("w1", "w2"))):
        hi, lo = mod.packed(), mod.packed().lo()
        assert lo is mod.packed_lo()                               # built once
        for k in keys:
            assert lo[k].dtype == torch.float16 and lo[k].shape == hi[k].shape and lo[k].abs().max() > 0, k
    # the pair carries the fp32 parameter to ~2^-22: conv3x3 (ci/64 slices, taps), conv1d taps, the GEGLU interleave
    def joined(mod, k):
        return mod.packed()[k].double() + mod.packed_lo()[k].double() / 2048.0
    w32 = rb.in_layers[2].weight.detach()
    co, ci = w32.shape[:2]
    p = w32.permute(0, 2, 3, 1).reshape(co, 9, ci // 64, 64).permute(0, 2, 1, 3).reshape(co, 9 * ci).double()
    assert (joined(rb, "w1") - p).abs().max() <= p.abs().max() * 2.0 ** -21
    w1 = ff.net[0].proj.weight.detach().double()
    n2 = w1.shape[0] // 2
    gi = torch.stack([w1[:n2].view(n2 // 32, 32, -1), w1[n2:].view(n2 // 32, 32, -1)], dim=1).reshape(2 * n2, -1)
    assert (joined(ff, "w1") - gi).abs().max() <= gi.abs().max() * 2.0 ** -21
    # the stem conv: Cin = 8 stays (ky, kx, ci) with its zero padding -> zero lo entries where the hi plane is padded
    hi_s, lo_s = stem.packed()[0][0], stem.packed().lo()[0][0]
    assert lo_s.shape == hi_s.shape and torch.equal(lo_s[hi_s == 0], torch.zeros_like(lo_s[hi_s == 0]))
    # a modified parameter: the twin is rebuilt with the hi copy (engine.invalidate_all); load_state_dict drops both
    before = rb.packed_lo()["w1"].clone()
    with torch.no_grad():
        rb.in_layers[2].weight.mul_(1.0 + 2.0 ** -9)
    E.invalidate_all(net)
    assert rb._pk_lo is None and rb._pk is None
    assert not torch.equal(rb.packed_lo()["w1"], before)
    rb.packed()
    net.to(torch.float64)
    assert (rb._pk_lo is None) == (rb._pk is None)                 # .to(): whatever happens to the hi copies happens to the twins
    net.to(torch.float32)
    rb.packed_lo()
    net.load_state_dict(net.state_dict())
    assert rb._pk_lo is None


def test_control_scales_are_folded_before_the_split():
    w, _, _, _ = _w32_network()
    cn = w.diffusion_model.controlnet
    cn.control_scales = 0.75
    cn.invalidate_packed()
    hi, lo = cn.packed()["zero"], cn.packed_lo()["zero"]
    for z, (h, _), (l, _) in zip(list(cn.zero_convs) + [cn.middle_block_out], hi, lo):
        w32 = z[0].weight.detach().double().reshape(h.shape) * 0.75
        assert (h.double() + l.double() / 2048.0 - w32).abs().max() <= w32.abs().max() * 2.0 ** -21


def test_every_weight_consumer_receives_its_lo_plane_and_no_other_policy_allocates_one(full_emu, monkeypatch):
    w, _, _, inp = _w32_network()
    m = w.diffusion_model
    calls = {"gemm": 0, "gemm_lo": 0, "small": 0, "small_lo": 0}

    def counting(name, fn, key):
        def wrapped(*a, **k):
            w16 = a[1] if name == "gemm" else a[2]
            if w16.dtype == torch.float16:
                calls[key] += 1
                calls[key + "_lo"] += int(isinstance(k.get("w_lo"), torch.Tensor) and k["w_lo"].dtype == torch.float16
                                          and k["w_lo"].shape == w16.shape)
            return fn(*a, **k)
        monkeypatch.setattr(emu, name, wrapped)
    counting("gemm", emu.gemm, "gemm")
    counting("linear_smallm", emu.linear_smallm, "small")
    counting("linear_smallm_segments", emu.linear_smallm_segments, "small")
    for p in OLD_POLICIES:
        m.precision = p
        with torch.no_grad():
            w(inp["x"], inp["t"], cond(inp))
        assert calls["gemm_lo"] == 0 and calls["small_lo"] == 0 and not _twins(m), p
    for k in calls:
        calls[k] = 0
    m.precision = "precise-full"
    with torch.no_grad():
        w(inp["x"], inp["t"], cond(inp))
    print(calls)
    assert calls["gemm"] > 100 and calls["gemm_lo"] == calls["gemm"], calls
    assert calls["small"] > 0 and calls["small_lo"] == calls["small"], calls
    assert _twins(m)


def test_hoisted_invariants_run_under_precise_full(full_emu):
    w, _, _, inp = _w32_network()
    m = w.diffusion_model
    m.precision = "precise-full"
    x = torch.cat([inp["x"], inp["concat"]], dim=1)
    ctx, hint = inp["crossattn"], inp["cond_feat"]
    with torch.no_grad():
        plain = m.denoise(x, inp["t"], ctx, hint)
        inv = m.prepare(ctx, hint)
        assert inv.prec == E.PRECISE_FULL and inv.ctx16.lo is not None
        hoisted = m.denoise(x, inp["t"], ctx, hint, invariants=inv)
    assert torch.equal(plain, hoisted)
