"""panacea_amd/shard.py on its own, on CPU: the byte exchange every neighbour / transpose exchange of FrameShard and ViewShard is
written on (`_Link.exchange`: one all_to_all_single with split sizes), its staged collectives and its accounting, over gloo worlds of
1, 2 and 3 ranks and without a group; and the packing of typed tensors into byte messages (`_pack` / `_unpack`).  Every result is
compared bit for bit with what a table of the messages of ALL ranks says it must be."""
import os
import sys
import tempfile
from pathlib import Path

import pytest
import torch
import torch.multiprocessing as mp

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def parts_of(s: int, d: int):
    """the global table: the flat uint8 parts rank s addresses to rank d.  One part, two parts (one message: the G = 2 ring) or none
    at all, of 0, 16, 40 or 3 bytes — unequal per destination, and the table is not symmetric in (s, d)."""
    out = []
    for k in range((1, 2, 0)[(s + d) % 3]):
        n = (0, 16, 40, 3)[(2 * s + d + 3 * k) % 4]
        out.append(((torch.arange(n) * 7 + 31 * s + 17 * d + 5 * k) % 251).to(torch.uint8))
    return out


def check_exchange(link, me: int, world: int):
    """one exchange of the table's row `me`; -> the bytes it must have counted"""
    out = {d: parts_of(me, d) for d in range(world) if parts_of(me, d)}
    sizes_in = {s: [p.numel() for p in parts_of(s, me)] for s in range(world) if parts_of(s, me)}
    n0, b0 = link.exchanges, link.bytes_sent
    got = link.exchange(out, sizes_in, torch.device("cpu"))
    for s in range(world):
        want = parts_of(s, me)
        have = got.get(s, [])
        assert len(have) == len(want), (me, s, len(have), len(want))
        for h, w in zip(have, want):
            assert h.dtype == torch.uint8 and torch.equal(h, w), (me, s)
    to_others = sum(p.numel() for d in range(world) if d != me for p in parts_of(me, d))
    assert link.exchanges == n0 + 1 and link.bytes_sent == b0 + to_others, (link.exchanges, link.bytes_sent, to_others)
    return out


def test_the_table_holds_the_cases():
    """what the worlds below exercise: a zero-length part, a rank that sends nothing to a peer, two parts for one destination"""
    for world in (2, 3):
        flat = [(s, d, parts_of(s, d)) for s in range(world) for d in range(world)]
        assert any(p.numel() == 0 for _, _, ps in flat for p in ps)
        assert any(s != d and not ps for s, d, ps in flat) or world == 2
        assert any(s != d and len(ps) == 2 for s, d, ps in flat)
    assert not parts_of(0, 2) and [p.numel() for p in parts_of(0, 1)] == [16, 0]
    assert [sum(p.numel() for p in parts_of(2, d)) for d in range(3)] == [0, 16, 56]          # unequal per destination


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    torch.set_num_threads(1)
    import torch.distributed as dist
    from panacea_amd import shard
    dist.init_process_group("gloo", rank=rank, world_size=world)
    group = dist.new_group(list(range(world)))
    link = shard._Link(world, rank, group)
    assert link.host and (link.exchanges, link.bytes_sent) == (0, 0)
    check_exchange(link, rank, world)
    check_exchange(link, rank, world)                       # the counters add up
    # the asynchronous form hands back FrameShard.Pending; its result is the same dictionary
    pend = link.exchange_start({rank: parts_of(rank, rank)} if parts_of(rank, rank) else {},
                               {rank: [p.numel() for p in parts_of(rank, rank)]} if parts_of(rank, rank) else {}, torch.device("cpu"))
    assert isinstance(pend, shard.FrameShard.Pending)
    got = pend.result()
    assert all(torch.equal(h, w) for h, w in zip(got.get(rank, []), parts_of(rank, rank)))
    # the ring on the same primitive: (from_left, from_right) = (the left neighbour's to_right, the right neighbour's to_left), also
    # where both neighbours are one peer (G = 2) or this rank itself (the one-rank group).  Unequal sizes per direction.
    def ring_msg(r, direction):
        return ((torch.arange(24 if direction else 10) * 3 + 11 * r + 100 * direction) % 251).to(torch.uint8)
    vs = shard.ViewShard(world, rank, group)
    fl, fr = vs._exchange_bytes(ring_msg(rank, 0), ring_msg(rank, 1))
    assert torch.equal(fl, ring_msg((rank - 1) % world, 1)) and torch.equal(fr, ring_msg((rank + 1) % world, 0))
    assert (vs.exchanges, vs.bytes_sent) == (1, 34 if world > 1 else 0)
    a, b = torch.full((3, 5), float(rank)), torch.full((2, 7), rank + 0.5).half()
    (l1, l2), (r1, r2) = vs._exchange([a, b], [a + 10, b + 10])
    lf, rt = float((rank - 1) % world), float((rank + 1) % world)
    assert torch.equal(l1, torch.full((3, 5), lf + 10)) and torch.equal(l2, torch.full((2, 7), lf + 10.5).half())
    assert torch.equal(r1, torch.full((3, 5), rt)) and torch.equal(r2, torch.full((2, 7), rt + 0.5).half())
    # the staged collectives and their closed-form accounting
    n0, b0 = link.exchanges, link.bytes_sent
    t = torch.arange(6, dtype=torch.float32) + rank
    assert link.all_reduce(t) is t and torch.equal(t, world * torch.arange(6, dtype=torch.float32) + sum(range(world)))
    assert (link.exchanges, link.bytes_sent) == (n0 + 1, b0 + 2 * 24 * (world - 1) // world)
    flat = link.all_gather_flat(torch.arange(5, dtype=torch.float32) + 10 * rank)
    assert torch.equal(flat, torch.cat([torch.arange(5, dtype=torch.float32) + 10 * r for r in range(world)]))
    assert (link.exchanges, link.bytes_sent) == (n0 + 2, b0 + 2 * 24 * (world - 1) // world + 5 * 4 * (world - 1))
    parts = link.all_gather(torch.full((2, 3), rank, dtype=torch.int32))
    assert [int(p[0, 0]) for p in parts] == list(range(world)) and all(p.shape == (2, 3) for p in parts)
    assert (link.exchanges, link.bytes_sent) == (n0 + 2, b0 + 2 * 24 * (world - 1) // world + 5 * 4 * (world - 1))      # not counted
    (Path(out_dir) / f"ok{rank}").write_text("ok")
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(120)
@pytest.mark.parametrize("world", [1, 2, 3])
def test_link_over_gloo(world):
    """worlds 2 and 3, and a one-rank group (everything is addressed to this rank: the collective runs, nothing counts as sent)"""
    port = 29500 + ((os.getpid() * 3 + world * 29 + 1201) % 2000)
    with tempfile.TemporaryDirectory() as d:
        mp.spawn(_worker, args=(world, port, d), nprocs=world, join=True)
        assert all((Path(d) / f"ok{r}").read_text() == "ok" for r in range(world))


def test_link_without_a_group_is_the_loop_back():
    from panacea_amd import shard
    link = shard._Link(1, 0, None)
    assert not link.host
    check_exchange(link, 0, 1)
    parts = [torch.arange(n, dtype=torch.uint8) for n in (0, 16, 40)]
    got = link.exchange({0: parts}, {0: [0, 16, 40]})
    assert len(got[0]) == 3 and all(h is w for h, w in zip(got[0], parts))          # the caller's parts themselves: no copy
    assert link.exchange({}, {}) == {0: []} and link.bytes_sent == 0
    bl, br = torch.arange(10, dtype=torch.uint8), torch.arange(24, dtype=torch.uint8)
    vs = shard.ViewShard(1, 0, None)
    fl, fr = vs._exchange_bytes(bl, br)
    assert fl is br and fr is bl and (vs.exchanges, vs.bytes_sent) == (1, 0)
    t = torch.arange(6, dtype=torch.float32)
    assert link.all_reduce(t) is t and link.all_gather_flat(t) is t and link.bytes_sent == 0 and link.exchanges == 5


def test_pack_round_trips_flat_and_by_row():
    from panacea_amd import shard
    g = torch.Generator().manual_seed(3)
    R = 4
    h = torch.randn(R, 4, generator=g).half()
    u = torch.randint(0, 256, (R, 3), generator=g, dtype=torch.uint8)
    f = torch.randn(R, 2, generator=g)
    planes = [h, None, u, f]

    def raw(t):
        return t.contiguous().view(-1).view(torch.uint8)
    msg, spec = shard._pack(planes)
    assert msg.dtype == torch.uint8 and torch.equal(msg, torch.cat([raw(h), raw(u), raw(f)]))
    back = shard._unpack(msg, spec)
    assert back[1] is None and all(b.dtype == p.dtype and torch.equal(b, p) for b, p in zip(back, planes) if p is not None)
    rows, spec = shard._pack(planes, by_row=True)
    assert rows.shape == (R, 4 * 2 + 3 + 2 * 4)
    for r in range(R):
        assert torch.equal(rows[r], torch.cat([raw(h[r]), raw(u[r]), raw(f[r])]))
    perm = torch.tensor([2, 0, 3, 1, 1])                  # the message is cut and permuted along its rows like any of its planes
    back = shard._unpack(rows[perm].contiguous(), spec, by_row=True)
    assert back[1] is None and all(b.dtype == p.dtype and torch.equal(b, p[perm]) for b, p in zip(back, planes) if p is not None)
