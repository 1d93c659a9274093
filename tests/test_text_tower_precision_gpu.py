"""The text tower's operand policies on the MI355X: the towers and the bound of tests/text_tower_w32.py (unrounded fp32 weights,
truth = the float64 restatement, 16 e32) through the library — pnc_attn_text_split_f16 in every block, split operands and split
weights in every GEMM — and one case at the product's size (ViT-H/14 text side, penultimate layer)."""
from pathlib import Path

import pytest
import torch

import text_tower_w32 as fx
from helpers import measured
from oracle import clip_oracle
from panacea_amd import conditioner as C
from panacea_amd import hip

pytestmark = pytest.mark.gpu
DEV = "cuda"


class _count_split:
    def __enter__(self):
        self.calls, self.real = [], hip.attn_text_split
        hip.attn_text_split = lambda *a, **kw: (self.calls.append((kw["groups"], kw["heads"], kw["Lp"], kw["kv_valid"])), self.real(*a, **kw))[1]
        return self.calls

    def __exit__(self, *exc):
        hip.attn_text_split = self.real


def _run(dims, precision=None, rounded=False):
    out = fx.tower(dims, precision, rounded, device=DEV)(fx.tokens().to(DEV))
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("dims", [fx.SMALL, fx.DEEP])
def test_three_policies_against_truth(dims):
    f = fx.fixture(dims)
    bound = fx.FACTOR * f["e32"]
    with _count_split() as calls:
        errs = {p: fx.err(_run(dims, p), f["truth"]) for p in C.TEXT_TOWER_PRECISIONS}
    tag = "x".join(str(d) for d in dims)
    print(f"text tower {tag}: e32 {f['e32']:.3e}, bound {bound:.3e};", {p: f"{e:.3e} = {e / f['e32']:.1f} e32" for p, e in errs.items()})
    measured(f"text_tower_precision {tag}", e32=f["e32"], **{p.replace("-", "_"): e for p, e in errs.items()})
    assert calls == [(2, dims[2], 80, 77)] * (2 * (dims[1] - 1))       # one split launch per block and split policy, none under `fast`
    assert "libpanacea_hip.so" in Path("/proc/self/maps").read_text()
    assert errs["precise-full"] <= bound, errs
    assert errs["fast"] >= 10.0 * bound, errs
    assert errs["precise-wide"] > bound, errs                    # the weight planes are in use
    full = _run(dims, "precise-full")
    assert torch.equal(full, _run(dims, "precise-full"))


def test_wide_equals_full_on_rounded_weights_and_fast_is_the_omitted_keyword():
    wide, full = (_run(fx.SMALL, p, rounded=True) for p in ("precise-wide", "precise-full"))
    assert torch.equal(wide, full)                               # all-zero lo twins add exact zeros
    f = fx.fixture(fx.SMALL, rounded=True)
    e = fx.err(full, f["truth"])
    print(f"text tower, fp16-rounded weights: precise-full {e:.3e} = {e / f['e32']:.1f} e32")
    measured("text_tower_precision 128x3x2 rounded", e32=f["e32"], precise_full=e)
    assert e <= fx.FACTOR * f["e32"]
    assert not torch.equal(_run(fx.SMALL, "precise-wide"), _run(fx.SMALL, "precise-full"))
    with _count_split() as calls:
        a, b = _run(fx.SMALL), _run(fx.SMALL, "fast")
    assert torch.equal(a, b) and calls == []


def test_vit_h14_penultimate_one_prompt_precise_full_against_truth():
    """the product's size: width 1024, 24 blocks of which 23 run, 16 heads; ONE prompt of 77 tokens, unrounded weights; e32 from
    clip_oracle at the same size"""
    dims = (1024, 24, 16)
    f = fx.fixture(dims, prompts=1)
    emb = fx.tower(dims, "precise-full", device=DEV, arch="ViT-H-14")
    assert emb.layer == "penultimate" and emb.heads == 16 and len(emb.model.transformer.resblocks) == 24
    with _count_split() as calls:
        out = emb(f["tokens"].to(DEV))
        torch.cuda.synchronize()
    e = fx.err(out, f["truth"])
    print(f"text tower ViT-H/14 penultimate, 1 prompt: e32 {f['e32']:.3e}, precise-full {e:.3e} = {e / f['e32']:.1f} e32, "
          f"|out| {f['truth'].abs().max().item():.2f}")
    measured("text_tower_precision vit_h14", e32=f["e32"], precise_full=e)
    assert calls == [(1, 16, 80, 77)] * 23
    assert out.shape == (1, 77, 1024) and e <= fx.FACTOR * f["e32"]
