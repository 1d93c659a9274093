"""The text tower's operand policies (`precision=` of conditioner.FrozenOpenCLIPEmbedder) on the emulated backend: tests/emu.py plus
`attn_text_split` evaluated in float64 from the header's formulae (tests/emu_text_tower.py).

Fixture and bound: tests/text_tower_w32.py — towers of width 128 with 3 and with 24 layers on unrounded fp32 weights, 2 prompts of 77
tokens, truth = the float64 restatement, bound 16 e32 with e32 the fp32 oracle's own distance from truth.  On the emulation
`precise-full` is also held to half of the bound: more would mean an operand still travels single-plane
(tests/test_first_stage_precision.py argues the same).

The same fixture goes through the library in tests/test_text_tower_precision_gpu.py."""
import pytest
import torch

import emu
import emu_text_tower as ett
import text_tower_w32 as fx
from oracle import clip_oracle
from panacea_amd import conditioner as C
from panacea_amd import engine as E


def _run(emb, be=None, tok=None):
    with E.use_backend(be or ett.Backend()):
        return emb(fx.tokens() if tok is None else tok)


@pytest.mark.parametrize("dims", [fx.SMALL, fx.DEEP])
def test_float64_restatement_agrees_with_the_fp32_oracle(dims):
    f = fx.fixture(dims)
    assert f["truth"].dtype == torch.float64 and f["truth"].shape == (2, 77, dims[0])
    # e32 itself is the distance; what is held here is that it IS an fp32 rounding distance and not a different function: a few
    # 1e-6 at |out| of a few units.  16 e32 of a fixed fp32 yardstick: 2^-24 * 4 (|out|) * sqrt(layers * 12 roundings per block)
    yard = 2.0 ** -24 * f["truth"].abs().max().item() * (12 * dims[1]) ** 0.5
    print(f"tower {dims}: e32 {f['e32']:.3e}, yardstick {yard:.3e}, |out| {f['truth'].abs().max().item():.2f}")
    assert 0 < f["e32"] <= 16 * yard
    # and on another evaluation of the oracle (the last layer included) the two agree as closely
    sd, tok = fx.weights(*dims), fx.tokens()
    last = clip_oracle.text_tower(sd, tok, heads=dims[2], layer="last")
    assert (last.double() - fx.truth(sd, tok, dims[2], layer="last")).abs().max().item() <= 16 * f["e32"]


@pytest.mark.parametrize("dims", [fx.SMALL, fx.DEEP])
def test_precise_full_within_16_e32_of_truth_fast_and_wide_outside(dims):
    f = fx.fixture(dims)
    bound = fx.FACTOR * f["e32"]
    errs = {p: fx.err(_run(fx.tower(dims, p)), f["truth"]) for p in C.TEXT_TOWER_PRECISIONS}
    print(dims, "e32", f["e32"], {p: f"{e:.3e} = {e / f['e32']:.1f} e32" for p, e in errs.items()})
    assert errs["precise-full"] <= bound, errs
    assert errs["precise-full"] <= 0.5 * bound, errs
    assert errs["fast"] >= 10.0 * bound, errs
    assert errs["precise-wide"] > bound, errs                    # the weight planes are in use: without them the weights' rounding stays


def test_wide_and_full_differ_on_unrounded_weights_and_agree_on_fp16_ones():
    wide, full = (_run(fx.tower(fx.SMALL, p)) for p in ("precise-wide", "precise-full"))
    assert not torch.equal(wide, full)
    wide, full = (_run(fx.tower(fx.SMALL, p, rounded=True)) for p in (E.PRECISE_WIDE, E.PRECISE_FULL))
    assert torch.equal(wide, full)                               # all-zero lo twins add exact zeros
    f = fx.fixture(fx.SMALL, rounded=True)
    assert fx.err(full, f["truth"]) <= fx.FACTOR * f["e32"]


def test_default_omitted_keyword_and_fast_give_the_same_bits():
    a = _run(fx.tower(fx.SMALL), be=emu)                         # the plain emulation: no capability is asked for
    b = _run(fx.tower(fx.SMALL, "fast"), be=emu)
    c = _run(fx.tower(fx.SMALL, E.FAST))
    assert torch.equal(a, b) and torch.equal(a, c)
    assert fx.tower(fx.SMALL).precision is E.FAST
    be = ett.Backend()
    _run(fx.tower(fx.SMALL), be)
    assert be.split_calls == []                                  # `fast` keeps its single-plane launches


def test_one_split_launch_per_block_on_column_blocks_of_the_qkv_buffer():
    be = ett.Backend()
    views = []
    be.attn_views = lambda *a, **kw: views.append(1) or emu.attn_views(*a, **kw)
    _run(fx.tower(fx.SMALL, "precise-full"), be)
    W = 128
    assert be.split_calls == [dict(groups=2, heads=2, Lp=80, kv_valid=77, scale=64 ** -0.5, lds=(3 * W, 3 * W, 3 * W, W))] * 2
    assert views == []                                           # (3 layers, penultimate: two blocks run)


class _Counting:
    calls = 0

    def __getattr__(self, name):
        fn = getattr(emu, name)
        if not callable(fn):
            return fn

        def wrapped(*a, **kw):
            _Counting.calls += 1
            return fn(*a, **kw)
        return wrapped


def test_refusals():
    dims = dict(arch="custom", width=128, layers=2, heads=2, vocab_size=100)
    for bad in ("precise", "precise-ckpt", "precise-all", "precise-f16lo", "nonsense", E.PRECISE, E.PRECISE_CKPT, None, 3, 1.5):
        with pytest.raises(ValueError) as e:
            C.FrozenOpenCLIPEmbedder(**dims, precision=bad)
        assert all(n in str(e.value) for n in C.TEXT_TOWER_PRECISIONS), str(e.value)
        with pytest.raises(ValueError):
            C.FrozenOpenCLIPEmbedder(**dims).set_precision(bad)
    assert C.TEXT_TOWER_PRECISIONS == ("fast", "precise-wide", "precise-full")
    with pytest.raises(TypeError):                               # keyword-only
        C.FrozenOpenCLIPEmbedder("custom", "v", "cpu", 77, True, "last", None, 128, 2, 2, 100, "precise-full")
    for p in C.TEXT_TOWER_PRECISIONS:
        assert C.FrozenOpenCLIPEmbedder(**dims, precision=p).precision is E.PRECISIONS[p]
        assert C.FrozenOpenCLIPEmbedder(**dims, precision=E.PRECISIONS[p]).precision is E.PRECISIONS[p]
    # the mirror takes the YAML's params
    emb = C.instantiate_from_config(dict(target="panacea_amd.conditioner.FrozenOpenCLIPEmbedder", params=dict(dims, precision="precise-full")))
    assert emb.precision is E.PRECISE_FULL
    # a backend without the capability: refused before anything is launched
    for p in ("precise-wide", "precise-full"):
        emb = fx.tower(fx.SMALL, p)
        emb.packed()
        _Counting.calls = 0
        with E.use_backend(_Counting()):
            with pytest.raises(NotImplementedError, match="attn_text_split"):
                emb(fx.tokens())
        assert _Counting.calls == 0
    assert not hasattr(emu, "attn_text_split") and not hasattr(ett.Backend(with_split=False), "attn_text_split")
    with E.use_backend(ett.Backend(with_split=False)):
        with pytest.raises(NotImplementedError, match="attn_text_split"):
            fx.tower(fx.SMALL, "precise-full")(fx.tokens())
    # prompts longer than the kernel's 96 rows
    long = C.FrozenOpenCLIPEmbedder(**dims, max_length=100, precision="precise-wide")
    long.allow_random_init = True
    with E.use_backend(ett.Backend()):
        with pytest.raises(NotImplementedError, match="96"):
            long(torch.zeros(1, 100, dtype=torch.long))


def test_set_precision_is_followed_by_the_next_encode():
    emb = fx.tower(fx.SMALL)
    be = ett.Backend()
    fast = _run(emb, be)
    assert emb.set_precision("precise-full") is E.PRECISE_FULL
    full = _run(emb, be)
    assert len(be.split_calls) == 2 and not torch.equal(fast, full)
    assert torch.equal(full, _run(fx.tower(fx.SMALL, "precise-full")))
    emb.set_precision(E.FAST)
    assert torch.equal(_run(emb, be), fast) and len(be.split_calls) == 2


def test_load_state_dict_after_an_encode_rebuilds_the_lo_twins():
    emb = fx.tower(fx.SMALL, "precise-full")
    a = _run(emb)
    twin = emb.packed_lo()["blocks"][0]["wqkv"]
    assert twin.dtype == torch.float16 and bool(twin.ne(0).any()) and emb.packed_lo()["blocks"][0]["g1"] is None
    w = emb.model.transformer.resblocks[0].attn.in_proj_weight.detach()
    assert torch.equal(twin, E.split_lo(w, w.half()))
    sd = {k: v.clone() for k, v in emb.state_dict().items()}
    sd["model.transformer.resblocks.0.attn.in_proj_weight"] *= 1.0 + 2.0 ** -13      # moves (almost) only the lo plane
    emb.load_state_dict(sd)
    assert emb._pk is None and emb._pk_lo is None
    b = _run(emb)
    assert not torch.equal(a, b) and not torch.equal(emb.packed_lo()["blocks"][0]["wqkv"], twin)
    want = fx.truth(sd, fx.tokens(), 2)
    assert fx.err(b, want) <= fx.FACTOR * fx.fixture(fx.SMALL)["e32"]          # the output follows the new weights ...
    assert fx.err(a, want) > fx.FACTOR * fx.fixture(fx.SMALL)["e32"]           # ... which the old output does not
