#!/usr/bin/env python
"""End-to-end demo of everything this package owns, with SYNTHETIC weights (no checkpoint, no dataset offline):
conditioning tensors -> N sampler/CFG steps (Euler by default, `--sampler` picks another) of the ControlNet-UNet (step invariants hoisted) -> first-stage decode ->
per-view JPEGs + panorama GIF.  With `--ckpt <engine checkpoint>` the reference's weights are loaded instead
(`model.diffusion_model.*` into the denoiser, `first_stage_model.*` into the decoder).

    python tools/sample.py --steps 5 --out gpurun_out/sample
    python tools/sample.py --sampler dpmpp2m --steps 15
    python tools/sample.py --prediction v --steps 5       (a v-prediction checkpoint; `edm` = EDMScaling + the continuous Denoiser)
    python tools/sample.py --prediction edm --discretization edm --sampler heun --steps 18
    python tools/sample.py --frames 16 --steps 5          (clips of 1 .. 16 frames; the default 8 is the released FrameLength)
    python tools/sample.py --u8 --steps 5                 (uint8 channels-last BEV layout in, uint8 frames out: panacea_amd.image)
    python tools/sample.py --windows 4 --steps 5          (a video of 8 + 3 * 7 = 29 frames: windows chained on an anchor frame,
                                                           pipeline.rollout_frames; `--anchor first` rolls forward in time)
    python tools/sample.py --edit --strength 0.6 --keep 0,7    (clip editing, pipeline.edit_frames: a first sample is decoded to uint8
                                                           frames, then re-rendered under the swapped prompt from 60 % of the
                                                           schedule on, frames 0 and 7 kept as they are)
    python tools/sample.py --edit --keep-views 0,3             (region editing: camera views 0 and 3 of every frame stay the recorded
                                                           pixels, the other four are generated next to them)
    python tools/sample.py --edit --edit-rect 64,1024,192,1536 (only rows 64 .. 191, columns 1024 .. 1535 are re-rendered; with
                                                           --keep-views the kept sets are united)
"""
import argparse, json, sys, time
from pathlib import Path
import torch
ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from panacea_amd import build_network, checkpoint, configs, engine, image, pipeline, sampling, synth   # noqa: E402
from panacea_amd.nn import model                                               # noqa: E402

VAE = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
           num_res_blocks=2, attn_resolutions=[], dropout=0.0)
SAMPLERS = {"euler": "EulerEDMSampler", "heun": "HeunEDMSampler", "euler_a": "EulerAncestralSampler",
            "dpmpp2s_a": "DPMPP2SAncestralSampler", "dpmpp2m": "DPMPP2MSampler", "lms": "LinearMultistepSampler"}
P = "sgm.modules.diffusionmodules."
VIEWS = 6        # camera views side by side in a frame
DISCRETIZATIONS = {"ddpm": "LegacyDDPMDiscretization", "edm": "EDMDiscretization"}


def denoiser_config(prediction: str) -> dict:
    """the reference-style denoiser_config of a parameterisation: eps / v = DiscreteDenoiser on the DDPM table with EpsScaling /
    VScaling (what an SD eps or v checkpoint was trained under), edm = the continuous Denoiser with EDMScaling"""
    if prediction == "edm":
        return {"target": P + "denoiser.Denoiser", "params": {"scaling_config": {"target": P + "denoiser_scaling.EDMScaling"}}}
    scaling = {"eps": "EpsScaling", "v": "VScaling"}[prediction]
    return {"target": P + "denoiser.DiscreteDenoiser",
            "params": {"num_idx": 1000, "scaling_config": {"target": P + "denoiser_scaling." + scaling},
                       "discretization_config": {"target": P + "discretizer.LegacyDDPMDiscretization"}}}


def print_range_profile(prof, network, path=""):
    """the class table, the ten widest sites and the recommendation of an engine.RangeProfile; `path`: the report as JSON"""
    rep, rec = prof.report(), prof.recommend(network)

    def row(name, S):
        top = max((b for b, n in enumerate(S["binades"]) if n), default=0)
        return (f"{name[:58]:58s} {S['elements']:>13d} {S['max_abs']:>10.4g} {top:>4d} {S['ge_512']:>11d} {S['lo_saturated']:>11d} "
                f"{S['nan']:>6d} {S['inf']:>6d}")
    head = f"{'':58s} {'elements':>13s} {'max |v|':>10s} {'bin':>4s} {'>= 512':>11s} {'lo at end':>11s} {'NaN':>6s} {'Inf':>6s}"
    print(f"operand ranges over {rep['evaluations']} evaluation(s), policy {network.precision} (bin: highest occupied fp16 binade; 24 = [512, 1024))")
    print(head)
    for c, S in rep["classes"].items():
        print(row(c, S))
    print("the ten widest sites")
    for s in rep["sites"][:10]:
        print(row(f"{s['class']}: {s['site']}", s))
    print(f"recommended operand policy: {rec['policy']} (headroom {rec['headroom_binades']} binades) - {rec['reason']}")
    if path:
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        Path(path).write_text(json.dumps({"recommendation": rec, **rep}, indent=1))
        print("wrote", path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=25)
    ap.add_argument("--out", default="gpurun_out/sample")
    ap.add_argument("--ckpt", default=None)
    ap.add_argument("--seed", type=int, default=3407)
    ap.add_argument("--sampler", choices=sorted(SAMPLERS), default="euler")
    ap.add_argument("--cfg-scale", type=float, default=5.0)
    ap.add_argument("--prediction", choices=["eps", "v", "edm"], default="eps", help="denoiser parameterisation")
    ap.add_argument("--discretization", choices=sorted(DISCRETIZATIONS), default="ddpm", help="the sampler's sigma schedule")
    ap.add_argument("--frames", type=int, default=8, choices=range(1, 17), metavar="1..16", help="frames per clip (num_frames)")
    ap.add_argument("--precision", choices=sorted(engine.PRECISIONS), default=None,
                    help="operand policy of the denoiser (default: the network's own, `precise`); `precise-ckpt` splits the weights too — "
                         "the policy for fp32 checkpoints with an ordinary activation range (|v| < 512); `precise-full` splits every "
                         "operand and the weights (|v| < 65504, at 3-4x the time)")
    ap.add_argument("--first-stage-precision", choices=list(model.FIRST_STAGE_PRECISIONS), default="fast",
                    help="operand policy of the first-stage decoder and encoder: `precise-wide` carries every GEMM and attention operand as "
                         "an fp16 pair, `precise-full` splits the weights too (fp32 checkpoints: the reference runs its first stage in fp32)")
    ap.add_argument("--range-profile", nargs="?", const="", default=None, metavar="FILE",
                    help="profile the operand ranges of the first two evaluations of the run under the chosen policy "
                         "(UNetModel3D.profile_ranges): prints the class table, the ten widest sites and the recommended operand "
                         "policy; FILE: also write the report as JSON")
    ap.add_argument("--u8", action="store_true",
                    help="the image boundary on the device: the synthetic BEV layout enters as uint8 channels-last bytes (scaled / 255 in "
                         "the hint stem's entry kernel) and the frames leave the decoder as uint8 (T, H, W, 3)")
    ap.add_argument("--windows", type=int, default=0, metavar="N",
                    help="roll out N windows of --frames frames chained by conditioning (pipeline.rollout_frames): a synthetic anchor "
                         "frame, then each window anchored on the far-end frame of the one before; T + (N - 1)(T - 1) uint8 frames")
    ap.add_argument("--anchor", choices=["last", "first"], default="last",
                    help="--windows: the anchor's slot in the conditioning clip (last = the reference's --use_last_frame: the video "
                         "grows backwards in time; first: forwards)")
    ap.add_argument("--edit", action="store_true",
                    help="clip editing (pipeline.edit_frames) on a synthetic clip: a first sample is decoded to uint8 frames, then edited "
                         "under the other prompt; the timing printed is the edit's")
    ap.add_argument("--strength", type=float, default=0.6,
                    help="--edit: the share of the schedule that runs, in (0, 1]: the clip is noised to the level of step "
                         "floor((1 - strength) * steps) and sampled from there")
    ap.add_argument("--keep", default="", metavar="SLOTS", help="--edit: comma-separated frame slots kept as they are, e.g. 0,7")
    ap.add_argument("--keep-views", default="", metavar="VIEWS",
                    help=f"--edit: comma-separated camera views (0 .. {VIEWS - 1}, column bands of the panorama) whose recorded pixels are kept")
    ap.add_argument("--edit-rect", default="", metavar="Y0,X0,Y1,X1",
                    help="--edit: only the pixels of rows Y0 .. Y1-1, columns X0 .. X1-1 are re-rendered, everything outside is kept; "
                         "with --keep-views the kept sets are united")
    a = ap.parse_args()
    if a.windows < 0:
        ap.error("--windows takes N >= 1")
    if a.edit and a.windows:
        ap.error("--edit and --windows are two different runs")
    try:
        keep = tuple(int(s) for s in a.keep.split(",") if s.strip())
    except ValueError:
        ap.error("--keep takes comma-separated frame slots")
    if keep and not a.edit:
        ap.error("--keep belongs to --edit")
    try:
        keep_views = tuple(int(s) for s in a.keep_views.split(",") if s.strip())
    except ValueError:
        ap.error("--keep-views takes comma-separated camera views")
    if any(not 0 <= v < VIEWS for v in keep_views):
        ap.error(f"--keep-views takes camera views in 0 .. {VIEWS - 1}")
    rect = None
    if a.edit_rect:
        try:
            rect = tuple(int(s) for s in a.edit_rect.split(","))
        except ValueError:
            ap.error("--edit-rect takes four integers Y0,X0,Y1,X1")
        if len(rect) != 4 or not (0 <= rect[0] < rect[2] and 0 <= rect[1] < rect[3]):
            ap.error("--edit-rect takes four integers Y0,X0,Y1,X1 with 0 <= Y0 < Y1 and 0 <= X0 < X1")
    if (keep_views or rect) and not a.edit:
        ap.error("--keep-views and --edit-rect belong to --edit")
    dev = torch.device("cuda", 0)
    kw = configs.with_frames(configs.get("full"), a.frames)
    net = build_network(kw)
    fs = model.FirstStageDecoder(4, VAE, precision=a.first_stage_precision)
    if a.ckpt:
        print(checkpoint.load_denoiser(net, a.ckpt))
        sd = checkpoint.denoiser_state_dict(checkpoint.read_state_dict(a.ckpt), "first_stage_model.")
        print(fs.load_state_dict(sd, strict=False))
    else:
        man = json.loads((ROOT / "tests/golden/manifest_full.json").read_text())
        net.diffusion_model.load_state_dict(synth.synth_state_dict(man), strict=True)
        fs.load_state_dict(synth.synth_state_dict({k: list(v.shape) for k, v in fs.state_dict().items()}), strict=True)
    net, fs = net.to(dev), fs.to(dev)
    if a.precision:
        net.diffusion_model.precision = a.precision
    _, _, h, w = configs.SHAPES["full"]
    T = a.frames
    g = {k: v.to(dev) for k, v in synth.synth_inputs(2, T, h, w, context_dim=kw["context_dim"]).items()}
    cond = {"crossattn": g["crossattn"][1:2], "concat": g["concat"][T:], "cond_feat": g["cond_feat"][T:]}
    uc = {"crossattn": g["crossattn"][0:1], "concat": g["concat"][:T], "cond_feat": g["cond_feat"][:T]}
    if a.u8:       # the layout as the dataset holds it: H x W x C bytes, one tensor shared by the two CFG halves
        layout = (g["cond_feat"][T:] * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        cond["cond_feat"] = uc["cond_feat"] = layout
    noise = torch.randn(T, 4, h, w, generator=torch.Generator().manual_seed(a.seed)).to(dev)
    if a.edit:     # the synthetic clip: a first sample, decoded to bytes (not part of the edit's timing)
        clip = pipeline.sample_frames(net, fs, cond, uc, noise, num_steps=a.steps, denoiser=denoiser_config(a.prediction), output="uint8")
        enc = first_stage_encoder(a, dev)
        cond, uc = dict(cond, crossattn=g["crossattn"][0:1]), dict(uc, crossattn=g["crossattn"][1:2])       # "another prompt"
        noise = torch.randn(T, 4, h, w, generator=torch.Generator().manual_seed(a.seed + 1)).to(dev)
        keep_mask = None               # the pixels kept: the union of the kept views and of everything outside the rectangle
        if keep_views:
            keep_mask = image.view_mask(*clip.shape[:3], VIEWS, keep_views, dev)
        if rect:
            outside = image.rect_mask(*clip.shape[:3], rect, dev)
            keep_mask = outside if keep_mask is None else torch.maximum(keep_mask, outside)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    smp = sampling.from_config({"target": P + "sampling." + SAMPLERS[a.sampler],
                                "params": {"num_steps": a.steps,
                                           "discretization_config": {"target": P + "discretizer." + DISCRETIZATIONS[a.discretization]},
                                           "guider_config": {"target": P + "guiders.VanillaCFG", "params": {"scale": a.cfg_scale}}}},
                               device=dev)
    import contextlib
    profiling = net.diffusion_model.profile_ranges(evaluations=2) if a.range_profile is not None else contextlib.nullcontext()
    with profiling as prof:
        if a.windows:
            frames = rollout(a, net, fs, smp, g, dev)
        elif a.edit:
            frames = pipeline.edit_frames(net, fs, enc, clip, cond, uc, noise, strength=a.strength, keep=keep, num_steps=a.steps,
                                          sampler=smp, denoiser=denoiser_config(a.prediction),
                                          generator=torch.Generator(device=dev).manual_seed(a.seed), keep_mask_u8=keep_mask)
        else:
            frames = pipeline.sample_frames(net, fs, cond, uc, noise, num_steps=a.steps, sampler=smp,
                                            denoiser=denoiser_config(a.prediction), output="uint8" if a.u8 else "float")
    torch.cuda.synchronize(); dt = time.perf_counter() - t0
    u8 = frames.dtype == torch.uint8
    what = f"{a.sampler} ({a.prediction}-prediction, {a.discretization} schedule): {a.steps} steps + decode of {T} frames {tuple(frames.shape)}"
    if a.windows:
        what = (f"{a.sampler} ({a.prediction}-prediction, {a.discretization} schedule): {a.windows} windows of {T} frames, anchor {a.anchor}, "
                f"{a.steps} steps each, {tuple(frames.shape)}")
    if a.edit:
        start = pipeline.edit_start_step(a.strength, a.steps)
        what = (f"{a.sampler} ({a.prediction}-prediction, {a.discretization} schedule): edit of {T} frames at strength {a.strength} (steps "
                f"{start} .. {a.steps - 1} of {a.steps}), kept {kept_summary(keep, keep_views, rect, keep_mask)}, encode + decode, "
                f"{tuple(frames.shape)}")
    if u8:
        print(f"{what}: {dt:.2f} s (uint8, range {frames.min().item()} .. {frames.max().item()})")
    else:
        print(f"{what}: {dt:.2f} s "
              f"(range {frames.min().item():.2f} .. {frames.max().item():.2f}, finite={bool(torch.isfinite(frames).all())})")
    if prof is not None:
        print_range_profile(prof, net.diffusion_model, a.range_profile)
    out = Path(a.out); out.mkdir(parents=True, exist_ok=True)
    width = frames.shape[2] if u8 else frames.shape[-1]
    checkpoint.save_view_frames(frames, str(out), [f"scene__{v}__000" for v in range(6)], view_width=width // 6)
    checkpoint.save_gif(frames[:, ::4, ::4] if u8 else frames[:, :, ::4, ::4], str(out / "panorama_quarter.gif"))
    print("wrote", out)


def kept_summary(keep, keep_views, rect, keep_mask):
    """what an edit kept, for the printed line: frame slots, camera views, the outside of the rectangle, the share of pixels"""
    parts = ([f"frames {keep}"] if keep else []) + ([f"views {keep_views}"] if keep_views else [])
    if rect:
        parts.append(f"everything outside rows {rect[0]} .. {rect[2] - 1}, columns {rect[1]} .. {rect[3] - 1}")
    if keep_mask is not None:
        parts.append(f"{100.0 * (keep_mask != 0).float().mean().item():.1f} % of the pixels as recorded")
    return ", ".join(parts) or "none"


def first_stage_encoder(a, dev):
    """the first-stage encoder with synthetic weights, or the checkpoint's `first_stage_model.*` like the decoder"""
    enc = model.FirstStageEncoder(4, VAE, precision=a.first_stage_precision)
    if a.ckpt:
        print(enc.load_state_dict(checkpoint.denoiser_state_dict(checkpoint.read_state_dict(a.ckpt), "first_stage_model."), strict=False))
    else:
        enc.load_state_dict(synth.synth_state_dict({k: list(v.shape) for k, v in enc.state_dict().items()}), strict=True)
    return enc.to(dev)


def rollout(a, net, fs, smp, g, dev):
    """--windows: a synthetic anchor frame and one (cond, uc) pair per window -> the video's uint8 frames.  Window k reads the layouts
    of the video frames it covers (one synthetic layout per video frame, so neighbouring windows share the layout of the frame where
    they meet); the first-stage encoder gets synthetic weights, or the checkpoint's `first_stage_model.*` like the decoder."""
    T, W = a.frames, a.windows
    N = T + (W - 1) * (T - 1)
    enc = first_stage_encoder(a, dev)
    _, _, h, w = configs.SHAPES["full"]
    hint = g["cond_feat"][T:]                                                   # T synthetic layouts, cycled over the N video frames
    layout = torch.stack([hint[i % T] for i in range(N)])
    if a.u8:
        layout = (layout * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    windows = []
    for k in range(W):
        first = (W - 1 - k) * (T - 1) if a.anchor == "last" else k * (T - 1)
        lay = layout[first:first + T].contiguous()
        windows.append(({"crossattn": g["crossattn"][1:2], "cond_feat": lay}, {"crossattn": g["crossattn"][0:1], "cond_feat": lay}))
    gen = torch.Generator().manual_seed(a.seed)
    noise = torch.randn(W, T, 4, h, w, generator=gen).to(dev)
    anchor = torch.randint(0, 256, (8 * h, 8 * w, 3), generator=gen, dtype=torch.uint8).to(dev)
    return pipeline.rollout_frames(net, fs, enc, anchor, windows, noise, anchor=a.anchor, num_steps=a.steps, sampler=smp,
                                   denoiser=denoiser_config(a.prediction))


if __name__ == "__main__":
    main()
