"""Clips of 9 to 16 frames on the CPU: the product's host path over the torch emulation of the C-ABI (tests/emu.py, generic in T)
against the reference's own forward at 12 and 16 frames (tests/golden/tiny_t12.npz / tiny_t16.npz, tools/gen_golden_frames.py),
the construction-time limit of 16 frames, the state dict (the frame count adds no tensors) and the unchanged C-ABI (version 8).

The bounds are the `tiny` bounds of tests/test_engine_emu.py: more frames per temporal GroupNorm group is better conditioned, not
worse.  Block samples are held to 2e-3 of max(1, max|ref|) like there; the fixtures sample every tensor at its own `stride.<key>`."""
import ctypes
import subprocess

import numpy as np
import pytest
import torch

import emu
from helpers import cond, err_stats, golden, manifest, product_network, step_inputs
from panacea_amd import build_network, configs, engine as E, hip

TOL = {"precise": (1e-3, 2e-4), "fast": (3e-3, 5e-4)}          # tests/test_engine_emu.py, ("tiny", policy)
BLOCK_REL = 2e-3
SHAPE = (2, 8, 96)                                              # CFG batch, latent rows, latent columns (6 views of 16)


@pytest.mark.parametrize("T", [12, 16])
@pytest.mark.parametrize("prec", ["precise", "fast"])
def test_emulated_host_path_matches_reference_golden(T, prec):
    kw = configs.with_frames(configs.get("tiny"), T)
    w, _, _ = product_network("tiny", kw=kw)
    w.diffusion_model.precision = prec
    inp = step_inputs("tiny", kw, shape=(SHAPE[0], T, SHAPE[1], SHAPE[2]))
    gold = golden(f"tiny_t{T}")
    trace = {}
    with E.use_backend(emu), torch.no_grad():
        eps = w(inp["x"], inp["t"], cond(inp), trace=trace)
    st = err_stats(eps, gold["eps"])
    print(f"tiny, T={T}, {prec} (emulated):", st)
    assert eps.dtype == torch.float32 and eps.shape == inp["x"].shape == (2 * T, 4, 8, 96)
    assert st["max_abs"] <= TOL[prec][0] and st["mean_abs"] <= TOL[prec][1], st
    checked = 0
    for k in gold.files:
        key = k[6:] if k.startswith("block.") else k
        if key in trace and k != "eps" and not k.startswith("stride."):
            ref = gold[k]
            got = trace[key].reshape(-1)[::int(gold["stride." + k])].numpy()
            assert got.shape == ref.shape, k
            assert np.abs(got - ref).max() <= BLOCK_REL * max(1.0, np.abs(ref).max()), k
            checked += 1
    assert checked >= 15


def test_seventeen_frames_are_refused_at_construction():
    """The kernels hold at most 16 frames of a pixel: a longer clip is refused when the module is built, with the limit in the
    message — never with a PNC_EINVAL from the middle of the first evaluation."""
    from panacea_amd.nn.attention import SpatialTemporalTransformer
    from panacea_amd.nn.controlmodel import ControlNet3D
    from panacea_amd.nn.openaimodel import ResBlock3D, UNetModel3D
    kw = configs.with_frames(configs.get("tiny"), 17)
    with pytest.raises(NotImplementedError, match="16"):
        build_network(kw)
    with pytest.raises(NotImplementedError, match="16"):
        UNetModel3D(out_channels=4, **kw)
    with pytest.raises(NotImplementedError, match="16"):
        ControlNet3D(hint_channels=19, control_scales=1.0, **kw)
    with pytest.raises(NotImplementedError, match="16"):
        ResBlock3D(64, 256, 0.0, out_channels=64, num_frames=17)
    with pytest.raises(NotImplementedError, match="16"):
        SpatialTemporalTransformer(64, 1, 64, depth=1, context_dim=64, use_linear=True, num_frames=17)
    with pytest.raises(NotImplementedError, match="16"):
        ResBlock3D(64, 256, 0.0, out_channels=64, num_frames=0)
    for T in (1, 9, 16):                                        # the whole supported range builds
        ResBlock3D(64, 256, 0.0, out_channels=64, num_frames=T)
        SpatialTemporalTransformer(64, 1, 64, depth=1, context_dim=64, use_linear=True, num_frames=T)


def test_frame_count_adds_no_tensors():
    """The temporal position table is computed, not stored: the state dict at 16 frames is the one of manifest_tiny.json."""
    w = build_network(configs.with_frames(configs.get("tiny"), 16))
    assert {k: list(v.shape) for k, v in w.diffusion_model.state_dict().items()} == manifest("tiny")


def test_abi_is_unchanged(tmp_path):
    """No struct and no entry point changed: the header compiles as C, its layout is the ctypes mirror's, the version stays 8,
    and the three widened entry points validate their arguments before any launch (no device needed)."""
    fields = {"PncGemmParams": [f[0] for f in hip.GemmParams._fields_], "PncAttnParams": [f[0] for f in hip.AttnParams._fields_]}
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{hip.HEADER}"', 'int main(void) {']
    for st, fs in fields.items():
        src.append(f'printf("{st} %zu\\n", sizeof({st}));')
        src += [f'printf("{st}.{f} %zu\\n", offsetof({st}, {f}));' for f in fs]
    src.append('printf("abi %d\\n", PNC_ABI_VERSION); return 0; }')
    c = tmp_path / "layout.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", str(c), "-o", str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    for st, cls in (("PncGemmParams", hip.GemmParams), ("PncAttnParams", hip.AttnParams)):
        assert int(got[st]) == ctypes.sizeof(cls), st
        for f in fields[st]:
            assert int(got[f"{st}.{f}"]) == getattr(cls, f).offset, (st, f)
    assert int(got["abi"]) == hip.ABI_VERSION == 8
    lib = hip.load()
    assert lib.pnc_abi_version() == 8 and set(hip.header_symbols()) == set(hip._SIGNATURES)
    # frame counts outside 1..16 are PNC_EINVAL (-1) on valid-looking pointers; 16 frames pass the range check and stop at the
    # alignment check (PNC_EALIGN = -2) — nothing is launched either way
    buf = (ctypes.c_char * 64)()
    a = ctypes.addressof(buf)
    a16 = (a + 15) & ~15
    odd = ctypes.c_void_p(a16 + 2)
    ok = ctypes.c_void_p(a16)
    for T, want in ((17, -1), (0, -1), (16, -2), (9, -2)):
        assert lib.pnc_attn_temporal_f16(odd, 64, odd, 64, odd, 64, odd, 64, 1, T, 1, 1, 0.125, None) == want, T
        assert lib.pnc_groupnorm_temporal_silu(odd, 1, T, 1, 64, ok, ok, 1e-5, ok, None, hip.LO_F16, None) == want, T
        assert lib.pnc_groupnorm_temporal_part(odd, 1, T, 1, 64, ok, ok, 1e-5, ok, 1, 16, None, None, hip.LO_F16, 0, None) == want, T
