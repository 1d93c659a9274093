"""panacea_amd/shard.py with DEVICE tensors on the MI355X, one rank: the byte exchange without a group, through a one-rank gloo
group (the host-staging path: the result is back on the device) and through a one-rank "nccl" (= RCCL) group; and the frame
transposes through RCCL, where `Pending.result()` really waits on a work handle.  tests/test_shard_link.py has the worlds > 1."""
import os
import sys
from pathlib import Path

import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent


def _worker(rank, port, out):
    sys.path.insert(0, str(ROOT))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1", LOCAL_RANK="0")
    import torch.distributed as dist
    from panacea_amd import shard
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    rccl, gloo = dist.new_group([0]), dist.new_group([0], backend="gloo")
    dev = torch.device("cuda", 0)
    sizes = [0, 16, 40]
    want = [((torch.arange(n) * 5 + 3 * n) % 251).to(torch.uint8) for n in sizes]
    bad = []
    for tag, group in (("none", None), ("gloo", gloo), ("rccl", rccl)):
        link = shard._Link(1, 0, group)
        if link.host != (tag == "gloo"):
            bad.append(f"{tag}: host {link.host}")
        parts = [w.to(dev) for w in want]
        got = link.exchange({0: parts}, {0: sizes}, dev)[0]
        torch.cuda.synchronize()
        if len(got) != 3 or any(g.device != dev or g.dtype != torch.uint8 or not torch.equal(g.cpu(), w) for g, w in zip(got, want)):
            bad.append(f"{tag}: parts differ")
        if tag == "none" and not all(g is p for g, p in zip(got, parts)):
            bad.append("none: the loop-back copied")
        if (link.exchanges, link.bytes_sent) != (1, 0):
            bad.append(f"{tag}: counters {(link.exchanges, link.bytes_sent)}")
    # the frame transposes: through RCCL the same bits as the loop-back (which the CPU tests hold to the global tensor)
    B, Tl, N, C = 2, 2, 6, 8
    x = torch.randn(B * Tl * N, C, device=dev, generator=torch.Generator(dev).manual_seed(1)).half()
    sh0, sh = shard.FrameShard(1, 0, None), shard.FrameShard(1, 0, rccl)
    pend = sh.to_pixels_start(x, B, N)
    if not isinstance(pend, shard.FrameShard.Pending) or pend._work is None:
        bad.append("to_pixels_start through RCCL holds no work handle")
    px, px0 = pend.result(), sh0.to_pixels_start(x, B, N).result()
    fr, fr0 = sh.to_frames(px, B, N), sh0.to_frames(px0, B, N)
    torch.cuda.synchronize()
    if not (torch.equal(px, px0) and torch.equal(fr, fr0) and torch.equal(fr, x) and px.shape == (B * Tl * N, C)):
        bad.append("frame transposes through RCCL differ from the loop-back")
    if (sh.exchanges, sh.bytes_sent, sh0.exchanges, sh0.bytes_sent) != (2, 0, 2, 0):
        bad.append(f"frame counters {(sh.exchanges, sh.bytes_sent, sh0.exchanges, sh0.bytes_sent)}")
    open(out, "w").write("ok" if not bad else "; ".join(bad))
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_link_and_frame_transposes_on_device_tensors(tmp_path):
    out = tmp_path / "link.txt"
    mp.spawn(_worker, args=(29800 + (os.getpid() % 150), str(out)), nprocs=1, join=True)
    assert out.read_text() == "ok", out.read_text()
