"""Timings and errors of the text tower's operand policies (profiles/text_tower_precise.md).

    python tools/exp/text_tower_precise_timing.py [--rounds 7] [--reps 4] [--skip-errors] [--skip-timing]

One MI355X.  Device events around --reps back-to-back runs after a warm-up, in --rounds interleaved rounds (every variant once per
round, in turn); median and minimum over the rounds, one process (the method of profiles/long_clips.md).

  1. us of pnc_attn_text_split_f16 against the single-plane causal launch (pnc_attn_views_f16 with `causal`) at the product's shape:
     2 prompts x 16 heads, Lp = 80, 77 valid keys.
  2. ms per ViT-H/14 encode (penultimate layer) of 2 prompts of 77 tokens under `fast`, `precise-wide`, `precise-full`; synthetic
     unrounded weights, vocabulary cut to 500 rows (the gather does not depend on it).
  3. max|tower - float64 truth| of the towers 128 / 3 / 2 and 256 / 8 / 4 (width / layers / heads) on fp16-rounded and on unrounded
     weights, under the three policies, in units of e32 (tests/text_tower_w32.py).
  4. how far the eps of the `tiny` network moves (fp32 CPU oracle) when its context comes from a 64 / 3 / 1 tower under each policy
     instead of from the float64 truth.
"""
import argparse
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

from frame_attn_timing import interleaved  # noqa: E402
import text_tower_w32 as fx  # noqa: E402
from panacea_amd import conditioner as C  # noqa: E402
from panacea_amd import hip  # noqa: E402

DEV = "cuda"


def pair(*shape, seed):
    x = torch.randn(*shape, generator=torch.Generator().manual_seed(seed))
    hi = x.half()
    return hi.to(DEV), ((x - hi.float()) * 2048.0).half().to(DEV)


def kernels(rounds, reps):
    B, H, L, Lp = 2, 16, 77, 80
    W, M, scale = 64 * H, B * Lp, 64 ** -0.5
    print(f"## causal attention of one block, {B} prompts x {H} heads, Lp = {Lp}, {L} valid keys (us per launch: median / min over "
          f"{rounds} rounds of {reps} launches)")
    qkv, qkv_lo = pair(M, 3 * W, seed=1)
    qk = qkv[:, : 2 * W].contiguous()
    vt = torch.zeros(B, W, Lp, device=DEV, dtype=torch.float16)
    vt[:, :, :L] = qkv[:, 2 * W:].reshape(B, Lp, W)[:, :L].transpose(1, 2)
    o1, o, ol = (torch.zeros(M, W, device=DEV, dtype=torch.float16) for _ in range(3))
    f, fl = qkv.view(-1), qkv_lo.view(-1)
    res = interleaved({
        "pnc_attn_views_f16 (causal)": lambda: hip.attn_views(qk, 2 * W, qk.view(-1)[W:], 2 * W, vt, Lp, W * Lp, o1, W, groups=B, heads=H, H=1,
                                                              W=Lp, views=1, kvH=1, kvW=Lp, kv_views=1, kv_rows_per_group=Lp, q_per_kv=1,
                                                              kv_valid=L, segs=[[0]], scale=scale, causal=True),
        "pnc_attn_text_split_f16": lambda: hip.attn_text_split(f, fl, 3 * W, f[W:], fl[W:], 3 * W, f[2 * W:], fl[2 * W:], 3 * W, o, ol, W,
                                                               groups=B, heads=H, Lp=Lp, kv_valid=L, scale=scale)}, rounds, reps)
    for name, (med, mn) in res.items():
        print(f"  {name:<30} {med:8.1f} / {mn:8.1f} us")
    d = (o.float() - o1.float()).view(B, Lp, W)[:, :L].abs().max().item()
    print(f"  max |o_hi - single| over the real rows = {d:.3e}; finite: {bool(torch.isfinite(o).all() and torch.isfinite(ol).all())}")


def encodes(rounds, reps):
    dims = (1024, 24, 16)
    print(f"## ViT-H/14 text tower, penultimate layer, 2 prompts of 77 tokens (ms per encode: median / min over {rounds} rounds of {reps})")
    sd = fx.weights(*dims)
    tok = fx.tokens(2).to(DEV)
    towers = {}
    for p in C.TEXT_TOWER_PRECISIONS:
        emb = C.FrozenOpenCLIPEmbedder(arch="ViT-H-14", layer="penultimate", vocab_size=fx.VOCAB, precision=p)
        emb.load_state_dict(sd, strict=True)
        towers[p] = emb.to(DEV)
    res = interleaved({p: (lambda e=e: e(tok)) for p, e in towers.items()}, rounds, reps)
    base = res["fast"][0]
    for p, (med, mn) in res.items():
        print(f"  {p:<14} {med / 1e3:8.2f} / {mn / 1e3:8.2f} ms   {med / base:5.2f} x fast")


def errors():
    print("## max|tower - float64 truth| in e32 (e32 = max|fp32 oracle - truth|), 2 prompts of 77 tokens")
    for dims in ((128, 3, 2), (256, 8, 4)):
        for rounded in (True, False):
            f = fx.fixture(dims, rounded)
            row = []
            for p in C.TEXT_TOWER_PRECISIONS:
                out = fx.tower(dims, p, rounded, device=DEV)(f["tokens"].to(DEV))
                torch.cuda.synchronize()
                e = fx.err(out, f["truth"])
                row.append(f"{p} {e:.3e} = {e / f['e32']:.1f} e32")
            print(f"  {dims[0]} / {dims[1]} / {dims[2]}  {'fp16-representable' if rounded else 'unrounded fp32':<19} e32 {f['e32']:.3e}   " + "   ".join(row))


def eps_shift():
    """how far the `tiny` network's eps (the fp32 CPU oracle, so nothing but the context differs) moves when its `crossattn` context
    comes from the tower under each policy instead of from the float64 truth; tower: width 64 = tiny's context_dim, one head, 3 layers"""
    import json
    from oracle import panacea_oracle as po
    from panacea_amd import configs, synth
    kw = configs.get("tiny")
    sd = synth.synth_state_dict(json.loads((ROOT / "tests" / "golden" / "manifest_tiny.json").read_text()))
    B, T, h, w = configs.SHAPES["tiny"]
    inp = synth.synth_inputs(B, T, h, w, context_dim=kw["context_dim"])
    cfg = po.OracleConfig(num_frames=T, model_channels=kw["model_channels"], num_head_channels=kw["num_head_channels"],
                          spatial_only_attn_type=kw["spatial_only_attn_type"], insert_crossview=kw["insert_crossview"])
    dims = (kw["context_dim"], 3, 1)
    nb = inp["crossattn"].shape[0]
    print(f"## eps of the `tiny` network (CPU oracle) with the context of a {dims[0]} / {dims[1]} / {dims[2]} tower on the MI355X instead of truth; "
          f"{nb} prompts")

    def eps(ctx):
        c = dict(concat=inp["concat"], crossattn=ctx.float().cpu(), cond_feat=inp["cond_feat"])
        return po.wrapper_forward(sd, cfg, inp["x"], inp["t"], c)

    for rounded in (True, False):
        f = fx.fixture(dims, rounded, nb)
        base = eps(f["truth"])
        row = []
        for p in C.TEXT_TOWER_PRECISIONS:
            out = fx.tower(dims, p, rounded, device=DEV)(f["tokens"].to(DEV))
            torch.cuda.synchronize()
            d = (eps(out) - base).abs().max().item()
            row.append(f"{p} context err {fx.err(out, f['truth']):.3e} -> eps moves {d:.3e}")
        print(f"  {'fp16-representable' if rounded else 'unrounded fp32':<19} |eps| max {base.abs().max().item():.2f}   " + "   ".join(row))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--skip-errors", action="store_true")
    ap.add_argument("--skip-timing", action="store_true")
    a = ap.parse_args()
    print(f"build digest {hip.build_digest()[:16]}; {torch.cuda.get_device_name(0)}")
    if not a.skip_timing:
        kernels(a.rounds, a.reps)
        encodes(a.rounds, a.reps)
    if not a.skip_errors:
        errors()
        eps_shift()
