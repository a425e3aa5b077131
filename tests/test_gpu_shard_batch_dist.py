"""Batches of a sharded answer beyond the emulated ranks: 2 and 4 real rank processes on one GPU with gloo collectives on device tensors running
spiral_amd.dist.answer_batch_sharded, and configs[2] (2^24 x 256 B) at full size as four emulated shards."""
import os
import socket
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 2048

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
    j0, j1 = sdist.shard_range(rank, world, s.dim0)
    own = sa.Server(pg, 0, j0, j1)
    own.gen_db(12)
    servers = [own] + [sa.Server(pg, 0, share_db_of=own) for _ in range(B - 1)]
    for b, srv in enumerate(servers):
        srv.set_fold_ranks(world)
        srv.set_expand_shard(rank, world)
        srv.set_pub_params(*pps[b])
    own.use_graphs(True)
    bufs = sdist.batch_buffers(servers, world, world, True)
    ok = True
    total = s.dim0 * s.num_per
    for r, idxs in enumerate(([3, total - 1, 100, 7], [9, 9, total // 2, 1])):
        qs = [c.query(i) for c, i in zip(clients, idxs)]
        for srv, qy in zip(servers, qs):
            srv.set_query(qy)
        sdist.answer_batch_sharded(servers, None, bufs, sharded_expansion=True)
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


@pytest.mark.parametrize("world", [2, 4])
def test_real_rank_processes_answer_batches(world):
    """answer_batch_sharded with B = 4 clients and a sharded expansion on `world` rank processes (every rank on cuda:0, gloo): one all-gather of the
    GSW bits, one reduce-scatter, one all-gather of the folded ciphertexts per batch; every client's response == its single answer"""
    import torch.multiprocessing as mp

    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=600)
    assert all(p.exitcode == 0 for p in procs), [p.exitcode for p in procs]
    assert q.get(timeout=5) is True


def test_config3_full_size_four_shards_four_clients():
    """configs[2] (2^24 x 256 B, nu1 = 9, nu2 = 10) as G = 4 emulated shards with B = 4 clients: every lane's final ciphertext bit-identical to
    run_query_batch on the unsharded database"""
    import torch

    torch.cuda.is_available()
    import spiral_amd as sa
    from oracle import pyoracle as O
    from spiral_amd import dist as sdist
    from spiral_amd import server as SV

    kw = dict(t_gsw=10, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=22, p_db=256)
    po, pg = O.make_params(9, 10, **kw), sa.make_params(9, 10, **kw)
    s = O.shape_of(po)
    G, B = 4, 4
    clients = [O.Client(po, seed=900 + b) for b in range(B)]
    pps = [c.pub_params() for c in clients]
    idxs = [0, 123457, s.dim0 * s.num_per - 1, 4242]  # (a record of the 2^19 holds several 256-byte items)
    qs = [c.query(i) for c, i in zip(clients, idxs)]
    dev = torch.device("cuda", 0)
    # the reference: run_query_batch on the unsharded database
    ref = sa.Server(pg, 0)
    ref.gen_db(21)
    rl = [ref] + [sa.Server(pg, 0, share_db_of=ref) for _ in range(B - 1)]
    for b, srv in enumerate(rl):
        srv.set_pub_params(*pps[b])
        srv.set_query(qs[b])
    sa.run_query_batch(rl)
    ref.sync()
    exp = [srv.read(SV.BUF_FINAL).copy() for srv in rl]
    for srv in reversed(rl):
        srv.close()
    del ref, rl
    torch.cuda.empty_cache()
    accs, lanes = [], []
    try:
        for g in range(G):
            own = sa.Server(pg, 0, g * s.dim0 // G, (g + 1) * s.dim0 // G)
            own.gen_db(21)
            srvs = [own] + [sa.Server(pg, 0, share_db_of=own) for _ in range(B - 1)]
            for b, srv in enumerate(srvs):
                srv.set_fold_ranks(G)
                srv.set_pub_params(*pps[b])
                srv.set_query(qs[b])
            acc = torch.zeros(sdist.batch_acc_words(s, B), dtype=torch.int64, device=dev)
            sa.run_pre_sweep_batch(srvs, acc.data_ptr())
            own.sync()
            accs.append(acc)
            lanes.append(srvs)
        torch.cuda.synchronize()
        for g in range(1, G):  # the reduce ...
            accs[0] += accs[g]
            accs[g] = None
        n = sdist.batch_chunk_words(s, B, G)
        cts = []
        for g in range(G):  # ... and the scatter, then the local folds
            ct = torch.zeros(sdist.batch_ct_words(B), dtype=torch.int64, device=dev)
            chunk = accs[0][g * n:(g + 1) * n].clone()
            torch.cuda.synchronize()
            sa.fold_local_batch(lanes[g], chunk.data_ptr(), ct.data_ptr())
            lanes[g][0].sync()
            cts.append(ct)
        gathered = torch.cat(cts)
        torch.cuda.synchronize()
        sa.fold_root_batch(lanes[0], gathered.data_ptr())
        lanes[0][0].sync()
        for b in range(B):
            assert np.array_equal(lanes[0][b].read(SV.BUF_FINAL), exp[b]), f"client {b}: final ciphertext differs from run_query_batch's"
    finally:
        for srvs in lanes:
            for srv in reversed(srvs):
                srv.close()
