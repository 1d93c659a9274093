"""Launch trace of the host logic on CPU: which backend wrappers the `tiny` network and the samplers call, in what order, with which
arguments.

    python tools/launch_trace.py [--dump DIR] [case ...]

The backend is a recording proxy over the torch emulation of the C-ABI (tests/emu.py, the whole backend in one module).  Per call it
records the wrapper name and every argument under its parameter name — the emulation's signature, which tests/test_emu_surface.py
holds equal to panacea_amd/hip.py's — defaults filled in (an omitted optional argument and an explicit None are the same launch):
scalars and keywords as they are, tensors as shape, dtype and storage offset (never addresses: allocation order may change) — so
`w_lo` shows as None, an fp16 tensor or a (bytes, exponent) pair.  Per case it prints the launch count, a digest of the trace and a
digest of the output bytes; two trees that print the same table enqueue the same launches on the same bits.  `--dump DIR` writes the
full traces for diffing.

Network cases: every entry of engine.PRECISIONS on the wrapper network (`precise-wide` / `precise-full` on weights that are not
fp16-representable, so that a dropped weight plane changes the bits too); `precise` under the loop-back view shard and both loop-back
frame shards; SpatialTemporalTransformer.forward and ResBlock3D.forward on their own under `precise` and `precise-full`.

Sampler cases (`sampler/...`): the fused device loop of every sampler, 3 steps at CFG scale 2 around the closed-form network of
tests/sampler_cases.py, which here also embeds the c_noise it is handed through the backend; LinearMultistepSampler at order 3 (its
history is read), noise from a seeded generator, EulerEDMSampler and DPMPP2MSampler once more under VScaling with a float c_noise
(`c_skip`, pnc_timestep_embedding_f32), and EulerEDMSampler without a guider.  Their output digest is the final latent.
"""
import hashlib
import inspect
import sys
import types
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import emu  # noqa: E402
from helpers import cond, manifest, product_network, step_inputs  # noqa: E402
from sampler_cases import FakeTokenNetwork, fake_inputs  # noqa: E402
from panacea_amd import engine as E, parallel, sampling as S, synth  # noqa: E402
from panacea_amd.nn.attention import SpatialTemporalTransformer  # noqa: E402
from panacea_amd.nn.openaimodel import ResBlock3D  # noqa: E402
from panacea_amd.nn.util import timestep_embedding  # noqa: E402


def describe(v):
    if isinstance(v, torch.Tensor):
        return f"T{tuple(v.shape)}:{str(v.dtype)[6:]}@{v.storage_offset()}"
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(describe(x) for x in v) + "]"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}={describe(x)}" for k, x in sorted(v.items())) + "}"
    return repr(v)


class Recorder(types.ModuleType):
    """tests/emu.py as a backend for engine.use_backend; every call of a wrapper appends one line to `lines`"""

    def __init__(self):
        super().__init__("launch_trace_backend")
        self.lines = []

    def __getattr__(self, name):
        fn = getattr(emu, name)
        if not callable(fn) or isinstance(fn, type):
            return fn

        sig = inspect.signature(fn)      # = the product wrapper's signature: an omitted optional argument = its default

        def call(*a, **k):
            bound = sig.bind(*a, **k)
            bound.apply_defaults()
            self.lines.append(f"{name}(" + ", ".join(f"{n}={describe(x)}" for n, x in bound.arguments.items()) + ")")
            return fn(*a, **k)
        return call


def network(w32: bool):
    w, _, kw = product_network("tiny")
    if w32:
        w.diffusion_model.load_state_dict(synth.synth_state_dict(manifest("tiny"), round_fp16=False), strict=True)
    return w, step_inputs("tiny", kw)


def cases():
    for p in E.PRECISIONS:
        def whole(p=p):
            w, inp = network(p in ("precise-wide", "precise-full", "precise-ckpt"))
            w.diffusion_model.precision = p
            return w(inp["x"], inp["t"], cond(inp))
        yield p, whole
    shards = (("view", parallel.apply_view_shard, lambda: E.ViewShard(1, 0)),
              ("frame-halo", parallel.apply_frame_shard, lambda: E.FrameShard(1, 0, resblock="halo")),
              ("frame-transpose", parallel.apply_frame_shard, lambda: E.FrameShard(1, 0, resblock="transpose")))
    for tag, apply, make in shards:
        def sharded(apply=apply, make=make):
            w, inp = network(False)
            w.diffusion_model.precision = "precise"
            apply(w, make())
            return w(inp["x"], inp["t"], cond(inp))
        yield "precise/" + tag, sharded
    for cls in (SpatialTemporalTransformer, ResBlock3D):
        for p in ("precise", "precise-full"):
            def alone(cls=cls, p=p):
                w, inp = network(p == "precise-full")
                mod = next(m for m in w.diffusion_model.modules() if isinstance(m, cls))
                mod.precision = p
                B, T, h, wd = inp["x"].shape[0] // mod.num_frames, mod.num_frames, *inp["x"].shape[2:]
                g = torch.Generator().manual_seed(7)
                x = torch.randn(B * T, mod.in_channels if cls is SpatialTemporalTransformer else mod.channels, h, wd, generator=g)
                if cls is ResBlock3D:
                    return mod(x, torch.randn(B * T, mod.emb_channels, generator=g))
                ctx = inp["crossattn"]
                return mod(x, ctx[:, None].expand(B, T, *ctx.shape[1:]).reshape(B * T, *ctx.shape[1:]))
            yield f"{cls.__name__}/{p}", alone
    yield from sampler_cases()


class EmbeddingNetwork(FakeTokenNetwork):
    """the closed-form stand-in network, with the product's embedding of the c_noise it is handed (a backend launch: int64 table
    indices or floats) folded into its eps tokens"""

    def denoise_tokens(self, x, c_in, c_noise, ctx, concat, cond_feat, invariants=None):
        eps = super().denoise_tokens(x, c_in, c_noise, ctx, concat, cond_feat, invariants)
        eps.f32 += 1e-3 * timestep_embedding(c_noise, 64).mean(dim=1).repeat_interleave(eps.N)[:, None]
        return eps


def sampler_cases():
    v_float = lambda: S.DiscreteDenoiser(quantize_c_noise=False, scaling=S.VScaling())      # noqa: E731
    runs = [(cls, S.DiscreteDenoiser, 2.0, cls) for cls in ("EulerEDMSampler", "HeunEDMSampler", "EulerAncestralSampler",
                                                             "DPMPP2SAncestralSampler", "DPMPP2MSampler", "LinearMultistepSampler")]
    runs += [(cls, v_float, 2.0, cls + "/v-float") for cls in ("EulerEDMSampler", "DPMPP2MSampler")]
    runs.append(("EulerEDMSampler", S.DiscreteDenoiser, None, "EulerEDMSampler/no-guider"))
    for cls, denoiser, scale, tag in runs:
        def fused(cls=cls, denoiser=denoiser, scale=scale):
            kw = {"order": 3} if cls == "LinearMultistepSampler" else {}
            smp = getattr(S, cls)(3, guider=None if scale is None else S.VanillaCFG(scale), device="cpu", **kw)
            g = torch.Generator().manual_seed(11)
            smp.noise_sampler = lambda x: torch.randn(x.shape, generator=g)
            bd = S.BoundDenoiser(denoiser(), EmbeddingNetwork())
            x0, c, uc = fake_inputs()
            assert smp._fusable_network(bd, c)
            sig, sig_f = smp.sigmas(), smp.host_sigmas()
            x = x0 * torch.sqrt(1.0 + sig[0] ** 2.0)
            state = smp._state(x)
            for form, sv, draw in smp._steps(sig, sig_f, x.new_ones([x.shape[0]])):       # the device loop, as on the GPU
                if draw:
                    sv["noise"] = smp.noise_sampler(x)
                x = smp._device_step(form, sv, x, bd, c, uc, state)
            return x
        yield "sampler/" + tag, fused


def main(argv):
    torch.set_num_threads(8)       # the emulation's fp32 sums depend on the partitioning: pinned, the output digest is reproducible
    dump = None
    if "--dump" in argv:
        i = argv.index("--dump")
        dump = Path(argv[i + 1])
        dump.mkdir(parents=True, exist_ok=True)
        del argv[i:i + 2]
    print("| case | launches | trace digest | output digest |\n|---|---|---|---|")
    for name, run in cases():
        if argv and name not in argv:
            continue
        rec = Recorder()
        with E.use_backend(rec), torch.no_grad():
            out = run()
        text = "\n".join(rec.lines) + "\n"
        dig = hashlib.sha256(text.encode()).hexdigest()[:16]
        odig = hashlib.sha256(out.detach().contiguous().numpy().tobytes()).hexdigest()[:16]
        print(f"| {name} | {len(rec.lines)} | {dig} | {odig} |", flush=True)
        if dump is not None:
            (dump / (name.replace("/", "_") + ".txt")).write_text(text)


if __name__ == "__main__":
    main(sys.argv[1:])
