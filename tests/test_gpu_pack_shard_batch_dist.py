"""SpiralPack batches on trial-sharded servers beyond the emulated ranks: two real rank processes on one GPU with the gloo all-gather on device
tensors, each running spiral_amd.dist.answer_pack_batch_sharded; the root's responses equal a one-process answer_batch."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu
CHILD_LIMIT_S = 240  # each child's own time limit (a healthy one takes a few seconds)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q, B=2):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch

    torch.cuda.is_available()  # torch initialises HIP first
    import torch.distributed as dist

    import spiral_amd as sa
    from oracle import pyoracle as O
    from spiral_amd import dist as sdist
    from spiral_amd.pack import answer_batch

    dist.init_process_group("gloo", rank=rank, world_size=world)
    nu1, nu2, out_n, kw = 4, 2, 2, dict(t_gsw=4)
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    clients = [O.PackClient(po, out_n, seed=60 + b) for b in range(B)]  # the same keys and queries on every rank
    pps = [c.pub_params() for c in clients]
    cuts = sdist.pack_trial_cuts(world, s.trials)
    own = sa.PackServer(pg, out_n, 0, cuts[rank], cuts[rank + 1])
    own.gen_db(12)
    servers = [own] + [own.create_shard_lane() for _ in range(B - 1)]
    for sv, pp in zip(servers, pps):
        sv.set_pub_params(*pp)
    bufs = sdist.pack_batch_buffers(servers, cuts)
    total = s.dim0 * s.num_per
    ok = True
    for idxs in ([3, total - 1], [9, 9]):
        qs = [c.query(i) for c, i in zip(clients, idxs)]
        bufs, out = sdist.answer_pack_batch_sharded(servers, qs, None, bufs)
        ok &= (out is None) == (rank != 0)
        if rank == 0:
            ref = sa.PackServer(pg, out_n)
            ref.gen_db(12)
            refs = [ref] + [ref.create_lane() for _ in range(B - 1)]
            for sv, pp in zip(refs, pps):
                sv.set_pub_params(*pp)
            want, _ = answer_batch(refs, qs)
            for b in range(B):
                ok &= bool(np.array_equal(out[b][0], want[b][0]))
                ok &= bool(np.array_equal(clients[b].decode(out[b][0]), O.pack_db_item(po, out_n, 12, idxs[b])))
            for sv in reversed(refs):
                sv.close()
    for sv in reversed(servers):
        sv.close()
    if rank == 0:
        q.put(ok)
    dist.destroy_process_group()


def test_two_rank_processes_answer_pack_batches():
    """answer_pack_batch_sharded with B = 2 clients at (4, 2, 2) on two rank processes (both on cuda:0, gloo): fold_trials_batch, one all-gather,
    pack_gathered_batch on the root; every client's response == a one-process answer_batch's and decodes to its item"""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=CHILD_LIMIT_S)
    late = [p.pid for p in procs if p.is_alive()]
    for p in procs:
        if p.is_alive():
            p.kill()
            p.join()
    assert not late, f"rank processes {late} ran into their time limit"
    assert [p.exitcode for p in procs] == [0, 0]
    assert q.get(timeout=5) is True
