"""Launch trace of the host logic on CPU: which backend wrappers the `tiny` network calls, in what order, with which arguments.

    python tools/launch_trace.py [--dump DIR] [case ...]

The backend is a recording proxy over the torch emulation of the C-ABI (tests/emu.py with the split attention of tests/emu_wide.py and
the split weights of tests/emu_weights.py attached).  Per call it records the wrapper name and every argument under the name it
has in panacea_amd/hip.py, defaults filled in (an omitted optional argument and an explicit None are the same launch): scalars and
keywords as they are, tensors as shape, dtype and storage offset (never addresses: allocation order may change) — so `w_lo` shows
as None, an fp16 tensor or a (bytes, exponent) pair.  Per case it prints the launch count, a digest of the trace and a digest of the output bytes; two trees
that print the same table enqueue the same launches on the same bits.  `--dump DIR` writes the full traces for diffing.

Cases: every entry of engine.PRECISIONS on the wrapper network (`precise-wide` / `precise-full` on weights that are not
fp16-representable, so that a dropped weight plane changes the bits too); `precise` under the loop-back view shard and both loop-back
frame shards; SpatialTemporalTransformer.forward and ResBlock3D.forward on their own under `precise` and `precise-full`.
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
import emu_ckpt  # noqa: E402
import emu_weights  # noqa: E402
import emu_wide  # noqa: E402
from helpers import cond, manifest, product_network, step_inputs  # noqa: E402
from panacea_amd import engine as E, hip, parallel, synth  # noqa: E402
from panacea_amd.nn.attention import SpatialTemporalTransformer  # noqa: E402
from panacea_amd.nn.openaimodel import ResBlock3D  # noqa: E402

OVERLAY = dict(attn_views_split=emu_wide.attn_views_split, attn_temporal_split=emu_wide.attn_temporal_split, gemm=emu_ckpt.gemm,
               linear_smallm=emu_weights.linear_smallm, linear_smallm_segments=emu_weights.linear_smallm_segments)


def describe(v):
    if isinstance(v, torch.Tensor):
        return f"T{tuple(v.shape)}:{str(v.dtype)[6:]}@{v.storage_offset()}"
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(describe(x) for x in v) + "]"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}={describe(x)}" for k, x in sorted(v.items())) + "}"
    return repr(v)


class Recorder(types.ModuleType):
    """tests/emu.py + OVERLAY as a backend for engine.use_backend; every call of a wrapper appends one line to `lines`"""

    def __init__(self):
        super().__init__("launch_trace_backend")
        self.lines = []

    def __getattr__(self, name):
        fn = OVERLAY.get(name) or getattr(emu, name)
        if not callable(fn) or isinstance(fn, type):
            return fn

        sig = inspect.signature(getattr(hip, name))      # the product wrapper's signature: an omitted optional argument = its default

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
