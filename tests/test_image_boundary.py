"""The image boundary without a GPU: the two entries in the header, the binding and the library (ABI 8, refusals before any launch),
the scaling tables against the reference's numpy expressions, the host routing of uint8 frames on the emulated backend (with numpy
twins of the two wrappers installed here; without them every new path refuses before it launches anything and every old path runs),
and the writers on uint8 frames."""
import ctypes
import re
import types

import numpy as np
import pytest
import torch

import emu
import image_boundary_cases as ib
import test_vae as tv
from panacea_amd import checkpoint as ck, engine as E, hip, image, pipeline
from panacea_amd.conditioner import VAEEmbedder
from panacea_amd.nn import model

NEW = {"pnc_u8_to_tokens_f16": 9, "pnc_tokens_to_u8": 6}


def test_header_binding_and_library_agree_on_the_two_entries():
    syms = hip.header_symbols()
    assert set(syms) == set(hip._SIGNATURES)
    txt = re.sub(r"/\*.*?\*/", "", hip.HEADER.read_text(), flags=re.S)
    assert re.search(r"#define\s+PNC_ABI_VERSION\s+8\b", txt) and hip.ABI_VERSION == 8
    lib = hip.load()
    assert lib.pnc_abi_version() == 8
    for name, nargs in NEW.items():
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", txt)
        assert decl, name
        assert len(decl.group(1).split(",")) == nargs == len(hip._SIGNATURES[name][1])
        assert hip._SIGNATURES[name][0] is ctypes.c_int and getattr(lib, name).argtypes == hip._SIGNATURES[name][1]
    assert hip._SIGNATURES["pnc_tokens_to_u8"][1][2] is ctypes.c_int64              # M
    assert "image.hip" in __import__("panacea_amd.build", fromlist=["SOURCES"]).SOURCES


EINVAL, EALIGN = -1, -2


def test_every_refusal_returns_its_code_before_any_launch():
    """host addresses: a call that got past the checks would launch on them; every case here is refused first"""
    lib = hip.load()
    buf = ctypes.create_string_buffer(4096)
    a = (ctypes.addressof(buf) + 63) // 64 * 64
    src, lut, o, ol = a + 1, a + 1024, a + 2048, a + 3072

    def u8(src=src, lut=lut, F=1, Npix=4, C=3, Cpad=8, out=o, out_lo=ol):
        return lib.pnc_u8_to_tokens_f16(src, lut, F, Npix, C, Cpad, out, out_lo, None)
    for kw, want in [(dict(Cpad=12), EINVAL), (dict(Cpad=0, C=3), EINVAL), (dict(C=9, Cpad=8), EINVAL), (dict(C=0), EINVAL),
                     (dict(C=-1), EINVAL), (dict(src=None), EINVAL), (dict(lut=None), EINVAL), (dict(out=None), EINVAL),
                     (dict(F=0), EINVAL), (dict(Npix=0), EINVAL), (dict(out=o + 8), EALIGN), (dict(out_lo=ol + 2), EALIGN),
                     (dict(out=o + 8, out_lo=None), EALIGN)]:
        assert u8(**kw) == want, kw

    def q(x=a, ld=3, M=4, C=3, out=o):
        return lib.pnc_tokens_to_u8(x, ld, M, C, out, None)
    for kw, want in [(dict(C=0), EINVAL), (dict(C=9, ld=9), EINVAL), (dict(ld=2), EINVAL), (dict(M=0), EINVAL), (dict(x=None), EINVAL),
                     (dict(out=None), EINVAL), (dict(out=o + 2), EALIGN), (dict(out=o + 1), EALIGN), (dict(x=a + 2), EALIGN)]:
        assert q(**kw) == want, kw


def test_tables_are_the_references_numpy_expressions():
    for kind in ("layout", "image"):
        t = image.table(kind)
        assert t.dtype == np.float32 and t.shape == (256,) and np.array_equal(t.view(np.uint32), ib.TABLES[kind].view(np.uint32))
        # ... and elementwise on an image, as the dataset applies them
        u8 = ib.frame_bytes(1, 4, 16, 4)
        assert np.array_equal(t[u8].transpose(0, 3, 1, 2), ib.scaled_nchw(u8, kind))
        d = image.device_table(kind, "cpu")
        assert d is image.device_table(kind, torch.device("cpu")) and np.array_equal(d.numpy(), t)
    assert image.table("image")[0] == -1.0 and image.table("image")[255] == 1.0 and image.table("layout")[255] == 1.0
    with pytest.raises(ValueError):
        image.table("other")


def test_the_quantiser_reference_is_to_uint8():
    """image_boundary_cases.quantise (the GPU tests' reference) is checkpoint._to_uint8 on finite inputs, thresholds included"""
    x = ib.quantiser_inputs(1024)
    fin = np.isfinite(x)
    img = torch.from_numpy(x[fin]).reshape(1, 1, -1)
    assert np.array_equal(ck._to_uint8(img).reshape(-1), ib.quantise(x[fin]))
    th = ib.thresholds()
    assert np.array_equal(ib.quantise(th), np.arange(1, 256)) and np.array_equal(ib.quantise(np.nextafter(th, np.float32(-np.inf))), np.arange(255))
    assert ib.quantise(np.array([np.nan, np.inf, -np.inf, 1.0, -1.0], np.float32)).tolist() == [0, 255, 0, 255, 0]


# ---- host routing on the emulated backend ---------------------------------------------------------------------------------------
@pytest.fixture
def twins(monkeypatch):
    monkeypatch.setattr(emu, "u8_to_tokens_f16", ib.u8_to_tokens_f16, raising=False)
    monkeypatch.setattr(emu, "tokens_to_u8", ib.tokens_to_u8, raising=False)
    del ib.CALLS[:]
    return ib.CALLS


def _layout_u8(like: torch.Tensor) -> torch.Tensor:
    """a uint8 channels-last layout with the frame count, channels and resolution of the float NCHW hint `like`"""
    T, C, H, W = like.shape
    return torch.from_numpy(np.random.default_rng(5).integers(0, 256, (T, H, W, C), dtype=np.uint8))


@pytest.fixture(scope="module")
def tiny():
    w, fs, c, uc, noise = tv._tiny_pipeline("cpu")
    u8 = _layout_u8(c["cond_feat"])
    f32 = torch.from_numpy(ib.scaled_nchw(u8.numpy(), "layout"))
    cf, ucf = dict(c, cond_feat=f32), dict(uc, cond_feat=f32)
    with E.use_backend(emu):
        frames = pipeline.sample_frames(w, fs, cf, ucf, noise, num_steps=2)
    return dict(w=w, fs=fs, c=c, uc=uc, noise=noise, u8=u8, f32=f32, cf=cf, ucf=ucf, frames=frames)


def test_sample_frames_uint8_is_to_uint8_of_the_float_run(tiny, twins):
    t = tiny
    cu, ucu = dict(t["c"], cond_feat=t["u8"]), dict(t["uc"], cond_feat=t["u8"])
    with E.use_backend(emu):
        got = pipeline.sample_frames(t["w"], t["fs"], cu, ucu, t["noise"], num_steps=2, output="uint8")
        got_nohoist = pipeline.sample_frames(t["w"], t["fs"], cu, ucu, t["noise"], num_steps=2, output="uint8", hoist=False)
    F, _, H, W = t["frames"].shape
    assert got.dtype == torch.uint8 and got.shape == (F, H, W, 3) and torch.equal(got, got_nohoist)
    want = np.stack([ck._to_uint8(f) for f in t["frames"]])
    assert np.array_equal(got.numpy(), want)
    assert "u8_to_tokens_f16" in twins and twins[-1] == "tokens_to_u8"
    with pytest.raises(ValueError):
        pipeline.sample_frames(t["w"], t["fs"], cu, ucu, t["noise"], num_steps=2, output="jpeg")


def test_uint8_hint_gives_the_eps_of_the_float_hint(tiny, twins):
    from helpers import step_inputs
    from panacea_amd import configs
    t = tiny
    w = t["w"]
    inp = step_inputs("tiny", configs.get("tiny"), "cpu")
    F = inp["x"].shape[0]
    f32, u8 = t["f32"].repeat(F // t["f32"].shape[0], 1, 1, 1), t["u8"].repeat(F // t["u8"].shape[0], 1, 1, 1)
    for prec in ("precise", "fast"):
        w.diffusion_model.precision = prec
        try:
            with E.use_backend(emu):
                a = w(inp["x"], inp["t"], dict(concat=inp["concat"], crossattn=inp["crossattn"], cond_feat=f32))
                b = w(inp["x"], inp["t"], dict(concat=inp["concat"], crossattn=inp["crossattn"], cond_feat=u8))
                inv = w.diffusion_model.prepare(inp["crossattn"], u8)
                c = w(inp["x"], inp["t"], dict(concat=inp["concat"], crossattn=inp["crossattn"], cond_feat=u8, _invariants=inv))
        finally:
            w.diffusion_model.precision = "precise"
        assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c), prec
    assert twins.count("u8_to_tokens_f16") == 4
    # the checks of the float hint apply unchanged: frame count, resolution
    with E.use_backend(emu), pytest.raises(ValueError):
        w.diffusion_model.prepare(inp["crossattn"], u8[:3])
    with E.use_backend(emu), pytest.raises(ValueError):
        w(inp["x"], inp["t"], dict(concat=inp["concat"], crossattn=inp["crossattn"], cond_feat=u8[:, ::2].contiguous()))


def _tiny_encoder():
    _, sd, g = tv._tiny_enc()
    fe = model.FirstStageEncoder(4, tv.TINY)
    fe.load_state_dict(sd, strict=True)
    return fe, g


def test_encoder_and_embedder_route_uint8_frames(twins):
    fe, g = _tiny_encoder()
    F, _, H, W = g["x"].shape
    u8 = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (F, H, W, 3), dtype=np.uint8))
    x = torch.from_numpy(ib.scaled_nchw(u8.numpy(), "image"))
    with E.use_backend(emu):
        assert torch.equal(fe.moments_u8(u8), fe.moments(x))
        assert torch.equal(fe.moments_u8(u8, table="layout"), fe.moments(torch.from_numpy(ib.scaled_nchw(u8.numpy(), "layout"))))
        z = fe.encode(x, generator=torch.Generator().manual_seed(4))
        assert torch.equal(fe.encode_u8(u8, generator=torch.Generator().manual_seed(4)), z)
        assert torch.equal(fe.encode_u8(u8, sample=False), fe.encode(x, sample=False))
        emb = VAEEmbedder()
        emb.first_stage_model, emb.disable_first_stage_autocast, emb.scale_factor = fe, True, 0.18215
        torch.manual_seed(7)
        want = emb(x)
        torch.manual_seed(7)
        assert torch.equal(emb(u8), want)
        emb.down_blur_factor = 2
        with pytest.raises(NotImplementedError):
            emb(u8)
        emb.down_blur_factor = 1
        plain = VAEEmbedder()                                    # a first stage that only encodes float frames
        plain.first_stage_model, plain.disable_first_stage_autocast, plain.scale_factor = torch.nn.Identity(), True, 0.18215
        plain.first_stage_model.encode = fe.encode
        with pytest.raises(TypeError, match="encode_u8"):
            plain(u8)
        with pytest.raises(ValueError):
            fe.moments_u8(u8, table="other")
        with pytest.raises(TypeError):
            fe.moments_u8(x)


def _counting_backend():
    """the emulated backend as it is (no image entries), every call counted"""
    calls = []

    def counted(name, fn):
        def run(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return run
    names = [n for n in dir(emu) if not n.startswith("_") and isinstance(getattr(emu, n), types.FunctionType)]
    be = types.SimpleNamespace(**{n: counted(n, getattr(emu, n)) for n in names})
    assert not hasattr(be, "u8_to_tokens_f16") and not hasattr(be, "tokens_to_u8") and hasattr(be, "gemm")
    return be, calls


def test_without_the_capability_every_new_path_refuses_before_any_launch_and_old_paths_run(tiny):
    t = tiny
    w, fs = t["w"], t["fs"]
    be, calls = _counting_backend()
    cu, ucu = dict(t["c"], cond_feat=t["u8"]), dict(t["uc"], cond_feat=t["u8"])
    fe, g = _tiny_encoder()
    img_u8 = torch.zeros((1, 16, 96, 3), dtype=torch.uint8)
    z = torch.from_numpy(tv._tiny()[2]["z"])
    from helpers import step_inputs
    from panacea_amd import configs
    inp = step_inputs("tiny", configs.get("tiny"), "cpu")
    u8_all = t["u8"].repeat(inp["x"].shape[0] // t["u8"].shape[0], 1, 1, 1)
    emb = VAEEmbedder()
    emb.first_stage_model, emb.disable_first_stage_autocast, emb.scale_factor = fe, True, 0.18215
    new_paths = {
        "tokens_to_u8": [lambda: fs.decode_u8(z),
                         lambda: pipeline.sample_frames(w, fs, t["cf"], t["ucf"], t["noise"], num_steps=2, output="uint8")],
        "u8_to_tokens_f16": [lambda: fe.moments_u8(img_u8), lambda: fe.encode_u8(img_u8), lambda: emb(img_u8),
                             lambda: w.diffusion_model.prepare(inp["crossattn"], u8_all),
                             lambda: w(inp["x"], inp["t"], dict(concat=inp["concat"], crossattn=inp["crossattn"], cond_feat=u8_all)),
                             lambda: w.diffusion_model.controlnet(torch.cat((inp["x"], inp["concat"]), 1), u8_all, inp["t"], inp["crossattn"]),
                             lambda: pipeline.sample_frames(w, fs, cu, ucu, t["noise"], num_steps=2)],
    }
    with E.use_backend(be):
        for name, paths in new_paths.items():
            for i, path in enumerate(paths):
                with pytest.raises(NotImplementedError, match=name):
                    path()
                assert calls == [], (name, i, calls[:3])
        # every old path still runs
        frames = pipeline.sample_frames(w, fs, t["cf"], t["ucf"], t["noise"], num_steps=2)
        assert torch.equal(frames, t["frames"]) and len(calls) > 100
        assert torch.equal(fs.decode(z), fs.decode(z))
        assert fe.encode(torch.from_numpy(g["x"]), sample=False).shape[1] == 4
    dec = model.FirstStageDecoder(4, dict(tv.TINY, tanh_out=True))
    with pytest.raises(NotImplementedError, match="tanh_out"):
        dec.decode_u8(z)


def test_writers_give_the_float_inputs_files_for_uint8_frames(tiny, tmp_path):
    frames = tiny["frames"]
    u8 = torch.from_numpy(np.stack([ck._to_uint8(f) for f in frames]))
    vw = frames.shape[-1] // 6
    names = [f"v{i}" for i in range(6)]
    pa = ck.save_view_frames(frames, str(tmp_path / "f"), names, view_width=vw)
    pb = ck.save_view_frames(u8, str(tmp_path / "u"), names, view_width=vw)
    assert len(pa) == len(pb) == 6 * frames.shape[0]
    for a, b in zip(pa, pb):
        assert a.replace(str(tmp_path / "f"), "") == b.replace(str(tmp_path / "u"), "")
        assert open(a, "rb").read() == open(b, "rb").read()
    ga = ck.save_gif(frames[:, :, ::2, ::2], str(tmp_path / "a.gif"))
    gb = ck.save_gif(u8[:, ::2, ::2], str(tmp_path / "b.gif"))
    assert open(ga, "rb").read() == open(gb, "rb").read()
    with pytest.raises(ValueError):
        ck.save_view_frames(u8.permute(0, 3, 1, 2), str(tmp_path / "x"), names, view_width=vw)
