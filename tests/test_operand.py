"""engine.Operand and engine.gemm, the one place that decides a16_lo / w_lo / out16_lo of a GEMM (CPU, a recording stub as the backend):
the exact call the helper makes on a 16 x 64 operand against a 64 x 64 packed weight, per form of the lo plane and of the key."""
from pathlib import Path

import pytest
import torch
from torch import nn

from panacea_amd import engine as E

M, N, K = 16, 64, 64


class Stub:
    def __init__(self):
        self.calls = []

    def gemm(self, *a, **kw):
        self.calls.append((a, kw))


class Lin(nn.Module, E.Packable):
    """a packed weight under a plain key, as a (weight, bias) entry and at the end of a path"""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.fc = nn.Linear(K, N)
        self._init_packable()

    def _pack(self, lo=False):
        w, b = E.pk_linear(self.fc.weight, lo), E.pk_f32(self.fc.bias)
        return dict(w=w, b=b, pair=(w, b), nest=[(w, b)])


@pytest.fixture
def env():
    be = Stub()
    with E.use_backend(be):
        rt = E.Runtime(torch.device("cpu"), 1, 1)
    return be, rt, Lin().packed()


def _one(be):
    assert len(be.calls) == 1
    return be.calls.pop()


def test_no_lo_plane(env):
    be, rt, pk = env
    a, o32 = torch.zeros(M, K, dtype=torch.float16), torch.zeros(M, N)
    for prec in (E.FAST, E.PRECISE, E.PRECISE_FULL):
        rt.prec = prec
        E.gemm(rt, E.Operand(a), pk, "w", M=M, N=N, K=K, lda=K, bias=pk["b"], out32=o32, ldc32=N)
        args, kw = _one(be)
        assert args[0] is a and args[1] is pk["w"] and len(args) == 2
        assert set(kw) == {"a16_lo", "w_lo", "M", "N", "K", "lda", "bias", "out32", "ldc32"}
        assert kw["a16_lo"] is None and kw["w_lo"] is None and kw["bias"] is pk["b"] and kw["out32"] is o32
    assert pk.owner._pk_lo is None and not any(isinstance(k, tuple) for k in pk)      # no twin, no e4m3 copy was built


def test_fp16_lo_plane_under_precise_wide_has_no_weight_plane(env):
    be, rt, pk = env
    rt.prec = E.PRECISE_WIDE
    a = rt.operand((M, K), "ln")
    assert a.lo.dtype == torch.float16
    E.gemm(rt, a, pk, "w", M=M, N=N, K=K, lda=K)
    args, kw = _one(be)
    assert args == (a.hi, pk["w"]) and set(kw) == {"a16_lo", "w_lo", "M", "N", "K", "lda"}
    assert kw["a16_lo"] is a.lo and kw["w_lo"] is None and pk.owner._pk_lo is None


@pytest.mark.parametrize("key", ["w", "pair", ("nest", 0)])
def test_fp16_lo_plane_under_precise_full_gets_the_lo_twin(env, key):
    be, rt, pk = env
    rt.prec = E.PRECISE_FULL
    a = rt.operand((M, K), "ln")
    E.gemm(rt, a, pk, key, M=M, N=N, K=K, lda=K)
    args, kw = _one(be)
    hi, lo = pk, pk.lo()
    for k in key if isinstance(key, tuple) else (key,):
        hi, lo = hi[k], lo[k]
    entry = isinstance(hi, tuple)
    assert args[0] is a.hi and args[1] is (hi[0] if entry else hi)
    assert set(kw) == {"a16_lo", "w_lo", "M", "N", "K", "lda"} | ({"bias"} if entry else set())
    assert kw["a16_lo"] is a.lo and kw["w_lo"] is (lo[0] if entry else lo)
    assert kw["w_lo"].dtype == torch.float16 and kw["w_lo"].shape == args[1].shape
    if entry:
        assert kw["bias"] is hi[1]
    if key == "w":
        assert kw["w_lo"] is pk.lo()[key]


def test_explicit_twin_of_a_stacked_weight(env):
    be, rt, pk = env
    w, twin = pk["w"], pk.lo()["w"]
    for prec, want in ((E.PRECISE_FULL, twin), (E.PRECISE_WIDE, None)):
        rt.prec = prec
        a = rt.operand((M, K), "ctx")
        E.gemm(rt, a, w, None, w_lo=twin, M=M, N=N, K=K, lda=K)
        args, kw = _one(be)
        assert args == (a.hi, w) and kw["a16_lo"] is a.lo and kw["w_lo"] is want


def test_e4m3_lo_plane_gets_the_e4m3_weights_packed_once(env):
    be, rt, pk = env
    rt.prec = E.PRECISE
    a = rt.operand((M, K), "stream")
    assert a.lo.dtype == torch.uint8
    E.gemm(rt, a, pk, "w", M=M, N=N, K=K, lda=K)
    args, kw = _one(be)
    assert args == (a.hi, pk["w"]) and set(kw) == {"a16_lo", "w_lo", "M", "N", "K", "lda"} and kw["a16_lo"] is a.lo
    q, e = first = kw["w_lo"]
    assert q.dtype == torch.uint8 and q.shape == (N, K) and isinstance(e, int)
    want = E.pk_lo8(pk["w"])
    assert torch.equal(q, want[0]) and e == want[1]
    E.gemm(rt, a, pk, "w", M=M, N=N, K=K, lda=K)
    assert _one(be)[1]["w_lo"] is first


def test_output_operand(env):
    be, rt, pk = env
    a = torch.zeros(M, K, dtype=torch.float16)
    for prec, cls in ((E.PRECISE, "stream"), (E.PRECISE_WIDE, "stream"), (E.PRECISE, "gn_res"), (E.FAST, "stream")):
        rt.prec = prec
        out = rt.operand((M, N), cls)
        E.gemm(rt, E.Operand(a), pk, "w", out, M=M, N=N, K=K, lda=K, ldc16=N)
        _, kw = _one(be)
        assert kw["out16"] is out.hi and out.hi.dtype == torch.float16 and out.hi.shape == (M, N)
        if getattr(prec, cls):
            assert set(kw) == {"a16_lo", "w_lo", "M", "N", "K", "lda", "ldc16", "out16", "out16_lo"}
            assert kw["out16_lo"] is out.lo and out.lo.dtype == prec.lo_dtype(cls) and out.lo.shape == (M, N)
        else:
            assert set(kw) == {"a16_lo", "w_lo", "M", "N", "K", "lda", "ldc16", "out16"} and out.lo is None


def test_operand_is_immutable_and_maps_both_planes():
    hi, lo = torch.arange(8.0).half(), torch.arange(8.0).half() + 8
    op = E.Operand(hi, lo)
    with pytest.raises(AttributeError):
        op.lo = None
    t = op.map(lambda p: p[2:])
    assert t.hi.data_ptr() == hi[2:].data_ptr() and t.lo.data_ptr() == lo[2:].data_ptr()
    assert E.Operand(hi).map(lambda p: p[2:]).lo is None and E.Operand(hi).planes() == [hi] and op.planes() == [hi, lo]


def test_no_nn_module_decides_a_weight_plane():
    """`w_lo=` appears under panacea_amd/nn/ only in the two projectors that stack their own weights and build their own twin"""
    root = Path(E.__file__).resolve().parent / "nn"
    allowed = {"attention.py": "class TextKVProjector", "openaimodel.py": "class EmbProjector"}
    for f in sorted(root.glob("*.py")):
        src = f.read_text()
        lines = src.splitlines()
        for i, line in enumerate(lines):
            if "w_lo=" not in line:
                continue
            owner = [l for l in lines[:i] if l.startswith(("class ", "def "))][-1]
            assert f.name in allowed and owner.startswith(allowed[f.name]), f"{f.name}:{i + 1}: {line.strip()}"
