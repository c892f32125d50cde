"""world_size=2 (gloo, CPU): ``dist.allreduce_totals`` sums the ranks' episode totals, leaves the local table alone, and is the
identity without a process group."""
import os
import tempfile

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from embodied_clip_amd.dist import allreduce_totals


def _rendezvous():
    """File-store rendezvous: no TCP port to race for."""
    fd, path = tempfile.mkstemp(prefix="ec_nav_gloo_")
    os.close(fd)
    os.unlink(path)
    return path


def _table(rank):
    """[(1 + 3), 10] float64 with sums that round differently in fp32 and fp64, different on each rank."""
    g = torch.Generator().manual_seed(100 + rank)
    t = torch.rand((4, 10), dtype=torch.float64, generator=g) * 1e3 + 1.0 / 3.0
    t[:, 0] = torch.tensor([7.0, 2.0, 3.0, 2.0]) * (rank + 1)
    return t


def _worker(rank, world, path, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["GLOO_SOCKET_IFNAME"] = "lo"
    dist.init_process_group("gloo", init_method=f"file://{path}", rank=rank, world_size=world)
    try:
        torch.set_num_threads(1)
        from embodied_clip_amd.episodes import info_from_nav_totals
        local = _table(rank)
        keep = local.clone()
        out = allreduce_totals(local)
        assert out.data_ptr() != local.data_ptr() and torch.equal(local, keep)        # a new tensor; the local table is unchanged
        assert out.dtype == torch.float64 and out.device.type == "cpu"
        again = allreduce_totals(local, group=dist.group.WORLD)
        assert torch.equal(out, again)
        q.put((rank, out.tolist(), info_from_nav_totals(out[0])))      # (plain floats: nothing the reader needs dies with this process)
    finally:
        dist.destroy_process_group()


@pytest.mark.timeout(180)
def test_two_ranks_sum_their_totals():
    world, path = 2, _rendezvous()
    ctx = mp.get_context("spawn")
    q = ctx.SimpleQueue()
    procs = [ctx.Process(target=_worker, args=(r, world, path, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:                                       # (a result is a few hundred bytes: put() never waits for the reader)
        p.join(120)
        assert p.exitcode == 0, p.exitcode                # a child that failed is reported here, before anything waits on the queue
    got = dict((r, (torch.tensor(t, dtype=torch.float64), info)) for r, t, info in (q.get() for _ in range(world)))
    want = _table(0) + _table(1)                          # one fp64 addition per entry: exact to compare with
    assert torch.equal(got[0][0], want) and torch.equal(got[1][0], want)
    assert got[0][1] == got[1][1] and got[0][1]["episodes"] == 21


def test_identity_without_a_process_group():
    assert not dist.is_initialized()
    t = _table(0)
    keep = t.clone()
    out = allreduce_totals(t)
    assert torch.equal(out, t) and torch.equal(t, keep) and out.data_ptr() != t.data_ptr()
    out += 1
    assert torch.equal(t, keep)
