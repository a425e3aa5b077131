"""A column-sharded batch beyond the emulated ranks: two real rank processes on one GPU with gloo collectives on device tensors running
spiral_amd.dist.answer_batch_column_sharded -- run_column_batch, ONE all-gather, fold_root_batch on the root."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q, B=4, nu=(5, 5)):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    import torch

    torch.cuda.is_available()  # torch initialises HIP first
    import torch.distributed as dist

    import spiral_amd as sa
    from oracle import pyoracle as O
    from spiral_amd import dist as sdist
    from spiral_amd import server as SV

    dist.init_process_group("gloo", rank=rank, world_size=world)
    kw = dict(t_gsw=4)
    po, pg = O.make_params(*nu, **kw), sa.make_params(*nu, **kw)
    s = O.shape_of(po)
    clients = [O.Client(po, seed=60 + b) for b in range(B)]  # the same keys and queries on every rank
    pps = [c.pub_params() for c in clients]
    own = sa.Server(pg, 0, col_rank=rank, col_ranks=world)
    own.gen_db(12)
    servers = [own] + [sa.Server(pg, 0, share_db_of=own) for _ in range(B - 1)]
    for b, srv in enumerate(servers):
        srv.set_pub_params(*pps[b])
    own.use_graphs(True)
    bufs = sdist.column_batch_buffers(servers, world)
    ok = sorted(bufs) == ["cts", "gathered_cts", "responses"]
    total = s.dim0 * s.num_per
    for idxs in ([3, total - 1, 100, 7], [0, 9, total // 2, 11]):  # (item 0 and the last; 9 and 11, 3 and 7: one column residue)
        qs = [c.query(i) for c, i in zip(clients, idxs)]
        for srv, qy in zip(servers, qs):
            srv.set_query(qy)
        assert sdist.answer_batch_column_sharded(servers, None, bufs) is bufs
        if rank == 0:
            ref = sa.Server(pg, 0)
            ref.gen_db(12)
            resp = bufs["responses"].cpu().numpy().view(np.uint64).reshape(B, -1)
            for b in range(B):
                ref.set_pub_params(*pps[b])
                ref.set_query(qs[b])
                ref.run_query()
                ref.sync()
                exp = ref.read(SV.BUF_RESPONSE)
                ok &= bool(np.array_equal(servers[b].read(SV.BUF_FINAL), ref.read(SV.BUF_FINAL)))
                ok &= bool(np.array_equal(servers[b].read(SV.BUF_RESPONSE), exp)) and bool(np.array_equal(resp[b], exp.reshape(-1)))
                ok &= bool(np.array_equal(clients[b].decode(exp), O.db_item(po, 12, idxs[b])))
            ref.close()
    for srv in reversed(servers):
        srv.close()
    if rank == 0:
        q.put(ok)
    dist.destroy_process_group()


def test_two_rank_processes_answer_column_sharded_batches():
    """answer_batch_column_sharded with B = 4 clients on two rank processes (both on cuda:0, gloo): one all-gather of the folded ciphertexts per batch
    and no other collective; on the root every client's final ciphertext and response == its single answer, for two rounds"""
    import torch.multiprocessing as mp

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=300)
    for p in procs:  # (a rank still running after its wait is ended, and fails the test below)
        if p.is_alive():
            p.kill()
            p.join()
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert q.get(timeout=5) is True
