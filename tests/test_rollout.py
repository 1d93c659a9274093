"""Videos past one clip, without a GPU (emulated backend, the numpy twins of the two image-boundary wrappers installed here as
tests/test_image_boundary.py installs them): image.SparseClip, the sparse first-stage encode against the dense float
`final_cond_zero` clip, pipeline.rollout_frames against the composition written out below, every refusal before a backend call, and
the reference's own two-window rollout (tests/golden/rollout_tiny.npz, tools/gen_golden_rollout.py).

Bounds are the ones the suite already holds these stages to: the first-stage encoder's against vae_enc_tiny.npz
(tests/test_vae.py: max-abs < 8e-3, mean-abs < 1e-3) and the sampler trajectory's (tests/test_sampler_acceptance.py: `tol_rel` of
sampler_tiny_net.npz, max-abs relative to max|x| of the reference latent)."""
import types

import pytest
import torch

import emu
import image_boundary_cases as ib
import rollout_cases as rc
from panacea_amd import engine as E, pipeline, sampling
from panacea_amd.conditioner import GeneralConditioner, VAEEmbedder
from panacea_amd.image import SparseClip

T, H, W = rc.T, rc.H, rc.W


@pytest.fixture(scope="module")
def twins():
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(emu, "u8_to_tokens_f16", ib.u8_to_tokens_f16, raising=False)
        mp.setattr(emu, "tokens_to_u8", ib.tokens_to_u8, raising=False)
        yield ib.CALLS


@pytest.fixture(scope="module")
def enc():
    return rc.tiny_encoder("cpu")


@pytest.fixture(scope="module")
def pipe(enc):
    return rc.tiny_rollout_pipeline("cpu", enc)


def _counting_backend():
    """the emulated backend as it stands (with the twins when they are installed), every call counted"""
    calls = []

    def counted(name, fn):
        def run(*a, **k):
            calls.append(name)
            return fn(*a, **k)
        return run
    names = [n for n in dir(emu) if not n.startswith("_") and isinstance(getattr(emu, n), types.FunctionType)]
    return types.SimpleNamespace(**{n: counted(n, getattr(emu, n)) for n in names}), calls


# ---- SparseClip -----------------------------------------------------------------------------------------------------------------
def test_sparse_clip_validates_at_construction():
    f = torch.zeros((2, 4, 6, 3), dtype=torch.uint8)
    c = SparseClip(f, [-1, 0], 4)
    assert c.slots == (3, 0) and c.num_frames == 4 and c.gather_index().tolist() == [1, 2, 2, 0]
    assert SparseClip(f[:0], [], 2).gather_index().tolist() == [0, 0]
    assert SparseClip(f.permute(0, 2, 1, 3), (0, 1), 2).frames_u8.is_contiguous()
    with pytest.raises(Exception):                            # frozen
        c.num_frames = 5
    for bad, exc in [((f.float(), [0, 1], 4), TypeError), ((f.numpy(), [0, 1], 4), TypeError), ((f, [0, 1.5], 4), TypeError),
                     ((f, [0, 1], 4.0), TypeError), ((f[0], [0], 4), ValueError), ((f, [0], 4), ValueError), ((f, [0, 4], 4), ValueError),
                     ((f, [0, -5], 4), ValueError), ((f, [1, -3], 4), ValueError), ((f, [0, 1], 0), ValueError),
                     ((f, [0, 0], 1), ValueError), ((f[:, :0], [0, 1], 4), ValueError)]:
        with pytest.raises(exc):
            SparseClip(*bad)


# ---- the sparse encode ----------------------------------------------------------------------------------------------------------
CLIPS = [(0, []), (1, [0]), (1, [1]), (1, [T - 1]), (1, [-1]), (2, [0, -1]), (2, [-2, 0]), (T, [2, 0, 1])]


@pytest.mark.parametrize("K,slots", CLIPS, ids=[f"K{k}-{'_'.join(map(str, s)) or 'none'}" for k, s in CLIPS])
def test_sparse_moments_and_encode_are_the_dense_float_clips(enc, twins, K, slots):
    u8 = rc.frames_u8(K, seed=3 + K)
    clip, dense = SparseClip(u8, slots, T), rc.dense_clip(u8, slots)
    with E.use_backend(emu):
        want = enc.moments(dense)
        got = enc.moments_sparse_u8(clip)
        assert got.shape == (T, 8, H // 2, W // 2) and got.dtype == torch.float32 and torch.equal(got, want)
        torch.manual_seed(11)
        z = enc.encode(dense)
        torch.manual_seed(11)
        assert torch.equal(enc.encode_sparse_u8(clip), z) and not torch.equal(z, want[:, :4])
        gen = torch.Generator().manual_seed(5)
        assert torch.equal(enc.encode_sparse_u8(clip, generator=gen), enc.encode(dense, generator=torch.Generator().manual_seed(5)))
        assert torch.equal(enc.encode_sparse_u8(clip, sample=False), want[:, :4])


def test_embedder_takes_a_sparse_clip_and_tensors_as_before(enc, twins):
    u8 = rc.frames_u8(1, seed=8)
    clip, dense = SparseClip(u8, [-1], T), rc.dense_clip(u8, [-1])
    emb = VAEEmbedder()
    emb.first_stage_model, emb.disable_first_stage_autocast, emb.scale_factor = enc, True, 0.18215
    with E.use_backend(emu):
        torch.manual_seed(7)
        want = emb(dense)
        torch.manual_seed(7)
        assert torch.equal(want, 0.18215 * enc.encode(dense))                               # tensors: float frames ...
        torch.manual_seed(7)
        assert torch.equal(emb(clip), want)
        full = rc.frames_u8(T, seed=9)
        torch.manual_seed(7)
        got_u8 = emb(full)                                                                  # ... and bytes, as before
        torch.manual_seed(7)
        assert torch.equal(got_u8, 0.18215 * enc.encode_u8(full))
        # through the conditioner's routing, under the key the YAML gives the embedder
        cond = GeneralConditioner([{"target": "panacea_amd.conditioner.VAEEmbedder", "input_key": "final_cond_zero"}])
        e = cond.embedders[0]
        e.first_stage_model, e.disable_first_stage_autocast, e.scale_factor = enc, True, 0.18215
        torch.manual_seed(7)
        assert torch.equal(cond({"final_cond_zero": clip})["concat"], want)
        torch.manual_seed(7)
        assert torch.equal(cond({"final_cond_zero": dense[None]})["concat"], want)
    emb.down_blur_factor = 2
    with pytest.raises(NotImplementedError, match="down_blur_factor"):
        emb(clip)
    plain = VAEEmbedder()                                        # a first stage that only encodes tensors
    plain.first_stage_model, plain.disable_first_stage_autocast, plain.scale_factor = torch.nn.Identity(), True, 0.18215
    plain.first_stage_model.encode, plain.first_stage_model.encode_u8 = enc.encode, enc.encode_u8
    with pytest.raises(TypeError, match="encode_sparse_u8"):
        plain(clip)
    with pytest.raises(TypeError):
        enc.moments_sparse_u8(u8)
    with pytest.raises(ValueError):
        enc.moments_sparse_u8(clip, table="other")
    with pytest.raises(ValueError):
        enc.moments_sparse_u8(SparseClip(torch.zeros((1, H, W, 4), dtype=torch.uint8), [0], T))


@pytest.mark.parametrize("K", [0, 1, 2, T])
def test_the_sparse_path_runs_the_encoder_over_k_plus_one_frames(enc, twins, K):
    """every 3x3 conv of the encoder is a gemm launch whose M is frames x output pixels: K + 1 frames for a sparse clip (K when no
    slot is blank), T for the dense one, in the same number of launches"""
    def frames_of(run):
        be, calls = _counting_backend()
        gemm, fr = be.gemm, []

        def counted_gemm(*a, **k):
            if k.get("conv"):
                fr.append(k["M"] / (k["conv"]["Hout"] * k["conv"]["Wout"]))
            return gemm(*a, **k)
        be.gemm = counted_gemm
        with E.use_backend(be):
            run()
        return fr, calls
    u8 = rc.frames_u8(K, seed=1)
    slots = list(range(K))
    fs, cs = frames_of(lambda: enc.moments_sparse_u8(SparseClip(u8, slots, T)))
    fd, cd = frames_of(lambda: enc.moments(rc.dense_clip(u8, slots)))
    assert set(fs) == {min(K + 1, T)} and set(fd) == {T} and len(fs) == len(fd) > 4
    assert cs.count("u8_to_tokens_f16") == (1 if K else 0) and "nchw_to_tokens_f16" not in cs and cd.count("nchw_to_tokens_f16") == 1
    # one encoder run, not one per frame: no more launches than the dense clip's (the mid-block attention launches per frame)
    assert len(cs) <= len(cd) and (len(cs) < len(cd)) == (K + 1 < T)


# ---- the rollout ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs(pipe, twins):
    """rollout_frames results of this module, one per argument set; at the smallest latent the tiny network takes (a window costs
    about a second on the emulation at the golden file's size)"""
    cache = {}

    def run(anchor, hint, W_=3, **kw):
        key = (anchor, hint, W_, tuple(sorted(kw.items())))
        if key not in cache:
            inp = rc.rollout_inputs(W_, anchor, hint, latent=rc.SMALL)
            rec = rc.Recorder(pipe["dec"], pipe["enc"])
            if "seed" in kw:
                kw = dict(kw, generator=torch.Generator().manual_seed(kw.pop("seed")))
            with E.use_backend(emu):
                out = pipeline.rollout_frames(pipe["net"], rec, rec, inp["anchor"], inp["windows"], inp["noise"], anchor=anchor,
                                              num_steps=2, **kw)
            cache[key] = dict(out=out, rec=rec, inp=inp)
        return cache[key]
    return run


def _manual(pipe, inp, anchor, sample, generator=None, hoist=True):
    """the rollout composed by hand from sample_frames(output="uint8") and encode_sparse_u8 -> (the video, every window's frames)"""
    slot, far = (T - 1, 0) if anchor == "last" else (0, T - 1)
    frame, wins = inp["anchor"], []
    for k, (c, uc) in enumerate(inp["windows"]):
        clip = SparseClip(frame[None], [slot], T)
        cc = pipeline.SCALE_FACTOR * pipe["enc"].encode_sparse_u8(clip, generator=generator, sample=sample)
        ucc = pipeline.SCALE_FACTOR * pipe["enc"].encode_sparse_u8(clip, generator=generator, sample=sample)
        x0 = sampling.share_noise_init(inp["noise"][k], cc, 0.07)
        wins.append(pipeline.sample_frames(pipe["net"], pipe["dec"], dict(c, concat=cc), dict(uc, concat=ucc), x0, num_steps=2,
                                           hoist=hoist, output="uint8"))
        frame = wins[-1][far]
    if anchor == "last":
        video = torch.cat([w[:-1] for w in wins[:0:-1]] + [wins[0]])
    else:
        video = torch.cat([wins[0]] + [w[1:] for w in wins[1:]])
    return video, wins


@pytest.mark.parametrize("anchor,hint", [("last", "uint8"), ("first", "float")])
def test_rollout_is_the_manual_composition_and_hands_the_far_frame_over(pipe, runs, anchor, hint):
    r = runs(anchor, hint, sample_posterior=False)
    out, rec, inp = r["out"], r["rec"], r["inp"]
    Wn = len(inp["windows"])
    N = T + (Wn - 1) * (T - 1)
    assert out.shape == (N,) + tuple(inp["anchor"].shape) and out.dtype == torch.uint8 and N == 7
    with E.use_backend(emu):
        video, wins = _manual(pipe, inp, anchor, sample=False)
    assert torch.equal(out, video)
    assert len(rec.decoded) == Wn and all(torch.equal(a, b) for a, b in zip(rec.decoded, wins))
    # two encodes per window, each of the window's anchor in its slot; window k + 1's anchor is window k's far-end frame, and that
    # frame is in the video where the two windows meet
    slot, far = (T - 1, 0) if anchor == "last" else (0, T - 1)
    assert len(rec.clips) == 2 * Wn and all(c.slots == (slot,) and c.num_frames == T for c in rec.clips)
    assert torch.equal(rec.clips[0].frames_u8[0], inp["anchor"])
    for k in range(Wn - 1):
        junction = rec.decoded[k][far]
        assert torch.equal(rec.clips[2 * k + 2].frames_u8[0], junction) and torch.equal(rec.clips[2 * k + 3].frames_u8[0], junction)
        at = (Wn - 1 - k) * (T - 1) if anchor == "last" else (k + 1) * (T - 1)
        assert torch.equal(out[at], junction)
    # the windows in the video: all of window 0, the others without their anchor slot
    for k in range(Wn):
        first = (Wn - 1 - k) * (T - 1) if anchor == "last" else k * (T - 1)
        keep = slice(None) if k == 0 else slice(0, T - 1) if anchor == "last" else slice(1, T)
        assert torch.equal(out[first:first + T][keep], rec.decoded[k][keep])
    assert inp["windows"][0][0]["cond_feat"].dtype == (torch.uint8 if hint == "uint8" else torch.float32)


def test_rollout_draws_twice_per_window_c_before_uc(pipe, runs):
    r = runs("last", "uint8", seed=31)
    with E.use_backend(emu):
        video, _ = _manual(pipe, r["inp"], "last", sample=True, generator=torch.Generator().manual_seed(31))
        assert torch.equal(r["out"], video)
        # the recorded concats are the draws of ONE stream, in the order c_0, uc_0, c_1, ...: replay them
        gen = torch.Generator().manual_seed(31)
        for clip, z in zip(r["rec"].clips, r["rec"].encoded):
            assert torch.equal(pipe["enc"].encode_sparse_u8(clip, generator=gen), z)
    rec = r["rec"]
    assert len(rec.encoded) == 6 and not torch.equal(rec.encoded[0], rec.encoded[1])
    assert not torch.equal(r["out"], runs("last", "uint8", sample_posterior=False)["out"])


def test_rollout_hoisted_is_unhoisted_and_one_window_is_sample_frames(pipe, runs):
    a = runs("first", "float", sample_posterior=False)
    b = runs("first", "float", sample_posterior=False, hoist=False)
    assert torch.equal(a["out"], b["out"])
    inp = a["inp"]
    (c, uc), noise = inp["windows"][0], inp["noise"][0]
    with E.use_backend(emu):
        one = pipeline.rollout_frames(pipe["net"], pipe["dec"], pipe["enc"], inp["anchor"], inp["windows"][:1], inp["noise"][:1],
                                      anchor="first", sample_posterior=False, num_steps=2)
        concat = pipeline.SCALE_FACTOR * pipe["enc"].encode_sparse_u8(SparseClip(inp["anchor"][None], [0], T), sample=False)
        want = pipeline.sample_frames(pipe["net"], pipe["dec"], dict(c, concat=concat), dict(uc, concat=concat),
                                      sampling.share_noise_init(noise, concat, 0.07), num_steps=2, output="uint8")
    assert one.shape == (T,) + tuple(inp["anchor"].shape) and torch.equal(one, want) and torch.equal(one, a["rec"].decoded[0])


def test_every_refusal_comes_before_the_first_backend_call(pipe, enc, twins):
    net, dec = pipe["net"], pipe["dec"]
    inp = rc.rollout_inputs(2, "last", "uint8")
    a, wins, noise = inp["anchor"], inp["windows"], inp["noise"]
    no_dec, no_enc = types.SimpleNamespace(decode=dec.decode), types.SimpleNamespace(encode=enc.encode, encode_u8=enc.encode_u8)

    def roll(net=net, dec=dec, enc=enc, a=a, wins=wins, noise=noise, **kw):
        return pipeline.rollout_frames(net, dec, enc, a, wins, noise, num_steps=2, **kw)
    be, calls = _counting_backend()
    assert hasattr(be, "u8_to_tokens_f16") and hasattr(be, "tokens_to_u8")
    with_concat = [(dict(wins[0][0], concat=torch.zeros(T, 4, H // 2, W // 2)), wins[0][1]), wins[1]]
    with_uc_concat = [wins[0], (wins[1][0], dict(wins[1][1], concat=torch.zeros(T, 4, H // 2, W // 2)))]
    cases = [(dict(dec=no_dec), TypeError, "decode_u8"), (dict(enc=no_enc), TypeError, "encode_sparse_u8"),
             (dict(noise=noise[:, :2]), ValueError, "num_frames"), (dict(noise=noise[0]), ValueError, "noise"),
             (dict(noise=noise[:1]), ValueError, "noise"), (dict(wins=[], noise=noise[:0]), ValueError, "noise"),
             (dict(a=a.float()), ValueError, "anchor_u8"), (dict(a=a[None]), ValueError, "anchor_u8"),
             (dict(a=a[:, :-1].contiguous()), ValueError, "anchor_u8"), (dict(a=a[:-2].contiguous()), ValueError, "anchor_u8"),
             (dict(a=a.numpy()), ValueError, "anchor_u8"),
             (dict(wins=with_concat), ValueError, "concat"), (dict(wins=with_uc_concat), ValueError, "concat"),
             (dict(wins=[wins[0], wins[1][0]]), ValueError, "pair"), (dict(anchor="middle"), ValueError, "anchor")]
    with E.use_backend(be):
        for kw, exc, match in cases:
            with pytest.raises(exc, match=match):
                roll(**kw)
            assert calls == [], (kw.keys(), calls[:3])
        for where in ("diffusion_model", "controlnet"):
            for attr in ("frame_shard", "view_shard"):
                m = net.diffusion_model if where == "diffusion_model" else net.diffusion_model.controlnet
                setattr(m, attr, object())
                try:
                    with pytest.raises(NotImplementedError, match="one device"):
                        roll()
                finally:
                    delattr(m, attr)
                assert getattr(m, attr) is None and calls == []
    # the emulated backend as it is committed, without the twins: the capability is refused by name
    with pytest.MonkeyPatch.context() as mp:
        mp.delattr(emu, "u8_to_tokens_f16")
        mp.delattr(emu, "tokens_to_u8")
        bare, calls = _counting_backend()
        assert not hasattr(bare, "u8_to_tokens_f16") and not hasattr(bare, "tokens_to_u8") and hasattr(bare, "gemm")
        clip = SparseClip(a[None], [-1], T)
        emb = VAEEmbedder()
        emb.first_stage_model, emb.disable_first_stage_autocast, emb.scale_factor = enc, True, 0.18215
        with E.use_backend(bare):
            for path in (roll, lambda: enc.moments_sparse_u8(clip), lambda: enc.encode_sparse_u8(clip), lambda: emb(clip),
                         lambda: enc.moments_sparse_u8(SparseClip(a[None][:0], [], T))):
                with pytest.raises(NotImplementedError, match="tokens_to_u8" if path is roll else "u8_to_tokens_f16"):
                    path()
                assert calls == []
            mp.setattr(bare, "tokens_to_u8", ib.tokens_to_u8, raising=False)
            with pytest.raises(NotImplementedError, match="u8_to_tokens_f16"):
                roll()
            assert calls == []


# ---- the reference's rollout ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["last", "first"])
@pytest.mark.parametrize("k", [0, 1])
def test_sparse_moments_and_concat_against_the_reference(enc, twins, tag, k):
    """the dense `final_cond_zero` clip through the reference's Encoder + quant_conv and its VAEEmbedder (posterior mean): window 0's
    anchor and window 1's, which is the far-end frame the reference generated"""
    with E.use_backend(emu):
        rc.check_moments_and_concat(enc, "cpu", tag, k, "emu")


@pytest.mark.parametrize("tag", ["last", "first"])
def test_second_window_latent_against_the_reference(pipe, twins, tag):
    """z_1 of the reference's rollout, from the reference's own window-0 far frame as anchor"""
    with E.use_backend(emu):
        rc.check_window_latent(pipe, "cpu", tag, 1, "emu")
