"""tests/emu.py is the whole backend: every wrapper the product calls on its backend exists there with panacea_amd/hip.py's
signature, `gemm` refuses what the library refuses, and no lo plane of the weights is accepted and ignored."""
import inspect
import re
from pathlib import Path

import pytest
import torch

import emu
import gemm_ref64 as ref64
from panacea_amd import hip

PKG = Path(hip.__file__).resolve().parent


def backend_calls():
    """every name the product calls through `.be.`, `backend().` or `be.`, from the source text of panacea_amd/**/*.py"""
    names = set()
    for f in PKG.rglob("*.py"):
        names |= set(re.findall(r"(?:\.be|backend\(\)|\bbe)\.([A-Za-z_]\w*)\s*\(", f.read_text()))
    return sorted(names)


def test_the_scan_finds_the_backend_surface():
    names = backend_calls()
    assert len(names) >= 25 and {"gemm", "attn_views_split", "cfg_sampler_step", "timestep_embedding_f32", "operand_stats"} <= set(names)


@pytest.mark.parametrize("name", backend_calls())
def test_signature_is_the_product_wrappers(name):
    assert hasattr(emu, name), f"tests/emu.py has no `{name}`"
    want = [(p.name, p.kind, p.default) for p in inspect.signature(getattr(hip, name)).parameters.values()]
    got = [(p.name, p.kind, p.default) for p in inspect.signature(getattr(emu, name)).parameters.values()]
    assert got == want


# ---- gemm: refusals and the weight planes ---------------------------------------------------------------------------------------
M, N, K = 8, 8, 16


def _launch(**extra):
    """a plain-A GEMM on fixed operands -> its fp32 output; `extra`: lo planes by name"""
    g = torch.Generator().manual_seed(3)
    a32, w32 = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g)
    a, w = a32.half(), w32.half()
    planes = dict(a_lo=((a32 - a.float()) * 2048.0).half(), w_lo=((w32 - w.float()) * 2048.0).half(),
                  a_lo8=torch.zeros(M, K, dtype=torch.uint8))
    assert planes["w_lo"].abs().max() > 0
    out = torch.zeros(M, N)
    kw = {k: (planes[v] if isinstance(v, str) else v) for k, v in extra.items()}
    emu.gemm(a, w, M=M, N=N, K=K, lda=K, out32=out, ldc32=N, **kw)
    return out, dict(a16=a, w16=w, M=M, N=N, K=K, lda=K, out32=True, ldc32=N, **kw)


@pytest.mark.parametrize("extra", [
    dict(w_lo="w_lo"),                                              # fp16 w_lo without a16_lo
    dict(a16_lo="a_lo", w_lo=torch.zeros(N, K)),                    # split weights with a non-fp16 plane
    dict(a16_lo="a_lo8", w_lo="w_lo"),                              # ... or next to a non-fp16 A_lo
    dict(w_lo16=torch.zeros(N, K)),                                 # w_lo16 of another dtype than w16
    dict(w_lo16=torch.zeros(N, K + 8, dtype=torch.float16)),        # ... of another shape
    dict(a16_lo="a_lo", w_lo="w_lo", w_lo16="w_lo"),                # fp16 a16_lo with both w_lo and w_lo16
    dict(a16_lo="a_lo8"),                                           # an e4m3 a16_lo without its pair
    dict(a16_lo="a_lo8", w_lo16="w_lo"),                            # ... also beside the struct
], ids=["wlo-no-alo", "wlo-f32", "wlo-alo8", "wlo16-dtype", "wlo16-shape", "wlo-and-wlo16", "alo8-no-pair", "alo8-wlo16-no-pair"])
def test_gemm_refuses_what_the_library_refuses(extra):
    with pytest.raises(emu.PncError):
        _launch(**extra)


@pytest.mark.parametrize("how", ["w_lo", "w_lo16"])
def test_a_weight_lo_plane_is_never_ignored(how):
    """an fp16 plane of the weights next to an fp16 A_lo moves the output by 2^-11 A_hi W_lo.  Bound: each of the two launches is
    within gemm_ref64.bound of its own float64 value (K = 16 fp32 products per pass), so their difference is within the sum of the
    two bounds of the float64 term."""
    base, kw0 = _launch(a16_lo="a_lo")
    got, kw1 = _launch(a16_lo="a_lo", **{how: "w_lo"})
    assert not torch.equal(got, base)
    r0, r1 = ref64.gemm(**kw0), ref64.gemm(**kw1)
    term = 2.0 ** -11 * kw1["a16"].double() @ kw1[how].double().t()
    assert torch.equal(r1["v"] - r0["v"], term) or (r1["v"] - r0["v"] - term).abs().max() < 1e-15
    err = ((got.double() - base.double()) - term).abs()
    tol = ref64.bound(r0) + ref64.bound(r1)
    print(f"{how}: |term| max {term.abs().max():.3e}, err / bound max {(err / tol).max():.3g}")
    assert (err <= tol).all()
    assert (term.abs() > tol).any()             # the check bites: a launch that drops the plane is outside the bound
