"""Batches of a sharded answer (run_pre_sweep_batch ... fold_root_batch) with the ranks emulated in one process: G owner servers on their j-shards of one
device, each with B - 1 lanes; the reduce-scatter is a torch sum and slice, the all-gathers are cats.  Every client's final ciphertext and response must
be bit-identical to its own run_query on an unsharded server with the same database, and decode to the oracle's item."""
import ctypes as C

import numpy as np
import pytest

N = 2048

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


class Ranks:
    """G emulated ranks of one batch: owners[g] on j-shard g, lanes[g] = [owner, its lanes]; fixed device buffers (as a deployment keeps them)"""

    def __init__(self, sa, O, nu1, nu2, kw, G, B, sharded, fold1, graphs, db_seed, clients):
        import torch

        from spiral_amd import dist as sdist

        self.sa, self.O, self.G, self.B, self.sharded, self.fold1 = sa, O, G, B, sharded, fold1
        self.po, self.pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
        self.s = O.shape_of(self.po)
        self.clients, self.pps = clients, [c.pub_params() for c in clients]
        self.db_seed = db_seed
        dev = torch.device("cuda", 0)
        FG = 1 if fold1 else G
        self.lanes = []
        for g in range(G):
            own = sa.Server(self.pg, 0, g * self.s.dim0 // G, (g + 1) * self.s.dim0 // G)
            own.gen_db(db_seed)
            srvs = [own] + [sa.Server(self.pg, 0, share_db_of=own) for _ in range(B - 1)]
            for b, srv in enumerate(srvs):
                srv.set_fold_ranks(FG)
                if sharded:
                    srv.set_expand_shard(g, G)
                srv.set_pub_params(*self.pps[b])
            if graphs and B > 1 and nu1 >= 8:
                # (a batch on the matrix-core geometry converts the image to limb planes the first time, which drops the graphs captured on the
                # packed form: converted up front, the first batch's captures are the only ones)
                own.set_db_format(sa.server.DB_LIMBS)
            own.use_graphs(graphs)
            self.lanes.append(srvs)
        z = lambda w: torch.zeros(w, dtype=torch.int64, device=dev)
        self.acc = [z(sdist.batch_acc_words(self.s, B)) for _ in range(G)]
        self.chunk = [z(sdist.batch_chunk_words(self.s, B, FG)) for _ in range(G)]
        self.cts = [z(sdist.batch_ct_words(B)) for _ in range(G)]
        self.gathered = z(sdist.batch_gathered_ct_words(B, FG))
        self.resp = z(sdist.batch_ct_words(B))
        self.wire_bytes = sa.lib().spiral_gpu_response_wire_bytes(C.byref(self.pg), 2)
        self.wire = torch.zeros(B * self.wire_bytes, dtype=torch.uint8, device=dev)
        if sharded:
            w = self.lanes[0][0].gsw_bits_words()
            self.bits = [z(sdist.batch_bits_words(w, B)) for _ in range(G)]
            self.gbits = z(G * sdist.batch_bits_words(w, B))

    def outputs(self):
        return [self.resp, self.wire] + self.acc + self.chunk + self.cts + [self.gathered] + (self.bits + [self.gbits] if self.sharded else [])

    def sync(self):
        import torch

        for srvs in self.lanes:
            srvs[0].sync()
        torch.cuda.synchronize()

    def answer(self, queries):
        import torch

        SV = self.sa.server
        G, B = self.G, self.B
        for g in range(G):
            for b in range(B):
                self.lanes[g][b].set_query(queries[b])
        if self.sharded:
            for g in range(G):
                SV.run_expand_pack_batch(self.lanes[g], self.bits[g].data_ptr())
            self.sync()
            self.gbits.copy_(torch.cat(self.bits))  # the all-gather: [rank][lane][words]
            self.sync()
            for g in range(G):
                SV.run_unpack_convert_sweep_batch(self.lanes[g], self.gbits.data_ptr(), self.acc[g].data_ptr())
        else:
            for g in range(G):
                SV.run_pre_sweep_batch(self.lanes[g], self.acc[g].data_ptr())
        self.sync()
        total = torch.stack(self.acc).sum(0)  # the reduce
        if self.fold1:  # root fold: everything on rank 0
            self.chunk[0].copy_(total)
            self.sync()
            SV.fold_local_batch(self.lanes[0], self.chunk[0].data_ptr(), self.cts[0].data_ptr())
            SV.fold_root_batch(self.lanes[0], self.cts[0].data_ptr(), self.resp.data_ptr(), self.wire.data_ptr())
        else:
            n = self.chunk[0].numel()
            for g in range(G):  # the scatter
                self.chunk[g].copy_(total[g * n:(g + 1) * n])
            self.sync()
            for g in range(G):
                SV.fold_local_batch(self.lanes[g], self.chunk[g].data_ptr(), self.cts[g].data_ptr())
            self.sync()
            self.gathered.copy_(torch.cat(self.cts))  # the all-gather: [rank][lane][CT]
            self.sync()
            SV.fold_root_batch(self.lanes[0], self.gathered.data_ptr(), self.resp.data_ptr(), self.wire.data_ptr())
        self.sync()

    def close(self):
        for srvs in self.lanes:
            for srv in reversed(srvs):
                srv.close()


def single_answers(sa, pg, db_seed, pps, queries):
    """each client's run_query on an unsharded server of the same database: (final, response, wire) per client"""
    from spiral_amd import server as SV

    ref = sa.Server(pg, 0)
    ref.gen_db(db_seed)
    out = []
    for pp, q in zip(pps, queries):
        ref.set_pub_params(*pp)
        ref.set_query(q)
        ref.run_query()
        ref.sync()
        out.append((ref.read(SV.BUF_FINAL).copy(), ref.read(SV.BUF_RESPONSE).copy(), ref.read_response_wire()))
    ref.close()
    return out


def check_batch(R, exp, idxs, what):
    from spiral_amd import server as SV

    resp = R.resp.cpu().numpy().view(np.uint64).reshape(R.B, -1)
    wire = R.wire.cpu().numpy().reshape(R.B, -1)
    for b in range(R.B):
        fin, rsp, wr = exp[b]
        root = R.lanes[0][b]
        assert np.array_equal(root.read(SV.BUF_FINAL), fin), f"{what}: client {b} final ciphertext"
        assert np.array_equal(root.read(SV.BUF_RESPONSE), rsp), f"{what}: client {b} response"
        assert np.array_equal(resp[b], rsp.reshape(-1)), f"{what}: client {b} response output"
        assert np.array_equal(wire[b], np.frombuffer(bytes(wr), dtype=np.uint8)), f"{what}: client {b} wire output"
        assert np.array_equal(bytes(root.read_response_wire()), bytes(wr)), f"{what}: client {b} read_response_wire"
        assert np.array_equal(R.clients[b].decode(rsp), R.O.db_item(R.po, R.db_seed, idxs[b])), f"{what}: client {b} decodes to its item"


# (nu1, nu2, kw): (4, 4) has 32 output columns -- one sweep per client and a strided copy; (5, 5) the vector-ALU passes of two; (8, 6) at G <= 4
# has shards of >= 64 first-dimension entries and 64 ciphertexts per slot: the matrix cores
VEC1, VEC2, MFMA = (4, 4, dict(t_gsw=4)), (5, 5, dict(t_gsw=4)), (8, 6, dict(t_gsw=4))
CASES = [
    # geometry, G, B, sharded expansion, fold ranks 1, graphs
    (VEC1, 2, 3, False, False, False),
    (VEC1, 4, 2, True, False, True),
    (VEC1, 2, 1, False, True, False),
    (VEC2, 2, 3, False, False, True),
    (VEC2, 4, 8, True, True, False),
    (VEC2, 1, 2, False, False, False),
    (VEC2, 4, 3, False, False, False),
    (MFMA, 4, 8, True, False, True),
    (MFMA, 2, 3, False, True, True),
    (MFMA, 1, 3, False, False, False),
    (MFMA, 2, 1, True, False, False),
]


@pytest.mark.parametrize("geo,G,B,sharded,fold1,graphs", CASES, ids=[f"nu{g[0]}-{g[1]}-G{G}-B{B}{'-xs' if s else ''}{'-root' if f else ''}{'-graphs' if gr else ''}"
                                                                   for g, G, B, s, f, gr in CASES])
def test_batch_matches_single_queries(sa, oracle, geo, G, B, sharded, fold1, graphs):
    from spiral_amd import ops

    O = oracle
    nu1, nu2, kw = geo
    clients = [O.Client(O.make_params(nu1, nu2, **kw), seed=100 + 7 * b + G) for b in range(B)]
    R = Ranks(sa, O, nu1, nu2, kw, G, B, sharded, fold1, graphs, 41 + G, clients)
    rng = np.random.default_rng(G * 10 + B)
    rounds = 3 if graphs else 1
    try:
        caps = None
        for r in range(rounds):
            idxs = [int(i) for i in rng.integers(0, R.s.dim0 * R.s.num_per, size=B)]
            qs = [c.query(i) for c, i in zip(clients, idxs)]
            R.answer(qs)
            check_batch(R, single_answers(sa, R.pg, R.db_seed, R.pps, qs), idxs, f"G={G} B={B} round {r}")
            if graphs:
                if r == 0:
                    caps = ops.get_option("graph_captures")
                else:
                    assert ops.get_option("graph_captures") == caps, "a replayed batch captured again"
    finally:
        R.close()


def test_update_between_replayed_batches_and_limb_image(sa, oracle):
    """update_db_items between two replayed batches (matrix-core geometry, the image in limb-plane form): the answers follow the update, nothing is
    captured again"""
    from spiral_amd import ops
    from spiral_amd import server as SV

    O = oracle
    nu1, nu2, kw = MFMA
    G, B = 2, 4
    clients = [O.Client(O.make_params(nu1, nu2, **kw), seed=300 + b) for b in range(B)]
    R = Ranks(sa, O, nu1, nu2, kw, G, B, False, False, True, 5, clients)
    try:
        for g in range(G):
            R.lanes[g][0].set_db_format(SV.DB_LIMBS)
        idxs = [3, 77, 1000, 4095]
        qs = [c.query(i) for c, i in zip(clients, idxs)]
        R.answer(qs)
        check_batch(R, single_answers(sa, R.pg, R.db_seed, R.pps, qs), idxs, "before the update")
        caps = ops.get_option("graph_captures")
        # new plaintexts for two of the queried items, on every shard and on the reference
        rng = np.random.default_rng(9)
        items = rng.integers(0, R.po.p_db, size=(2, 2, 2, N), dtype=np.uint64)
        ids = [77, 4095]
        for g in range(G):
            R.lanes[g][0].update_db_items(O.pack_items(items, 64), 64, ids)
        R.answer(qs)
        assert ops.get_option("graph_captures") == caps, "update_db_items forced a capture"
        ref = sa.Server(R.pg, 0)
        ref.gen_db(R.db_seed)
        ref.update_db_items(O.pack_items(items, 64), 64, ids)
        for b in range(B):
            ref.set_pub_params(*R.pps[b])
            ref.set_query(qs[b])
            ref.run_query()
            ref.sync()
            assert np.array_equal(R.lanes[0][b].read(SV.BUF_FINAL), ref.read(SV.BUF_FINAL)), f"client {b} after the update"
            exp = items[ids.index(idxs[b])] if idxs[b] in ids else O.db_item(R.po, R.db_seed, idxs[b])
            assert np.array_equal(clients[b].decode(R.lanes[0][b].read(SV.BUF_RESPONSE)), exp), f"client {b} decodes to the updated item"
        ref.close()
    finally:
        R.close()


def test_failures_write_nothing(sa, oracle):
    """a mismatched lane, a lane with another fold-rank count, n = 9, a null buffer: refused before anything is launched, every output unchanged"""
    import torch

    from spiral_amd import server as SV

    O = oracle
    nu1, nu2, kw = VEC1
    G, B = 2, 3
    clients = [O.Client(O.make_params(nu1, nu2, **kw), seed=500 + b) for b in range(B)]
    R = Ranks(sa, O, nu1, nu2, kw, G, B, False, False, False, 8, clients)
    other = sa.Server(R.pg, 0, 0, R.s.dim0 // G)  # another image on the same shard
    other.gen_db(8)
    other.set_fold_ranks(G)
    other.set_pub_params(*R.pps[0])
    try:
        qs = [c.query(5) for c in clients]
        R.answer(qs)
        for t in R.outputs():
            t.view(torch.uint8).fill_(0xA5) if t.dtype != torch.uint8 else t.fill_(0xA5)
        torch.cuda.synchronize()
        before = [t.clone() for t in R.outputs()]
        L0 = R.lanes[0]
        other.set_query(qs[0])
        for b in range(B):
            L0[b].set_query(qs[b])
        acc, chunk, cts, gath = (R.acc[0].data_ptr(), R.chunk[0].data_ptr(), R.cts[0].data_ptr(), R.gathered.data_ptr())
        with pytest.raises(RuntimeError, match="does not sweep server 0's database image"):
            SV.run_pre_sweep_batch(L0[:2] + [other], acc)
        L0[2].set_fold_ranks(1)
        with pytest.raises(RuntimeError, match="fold ranks"):
            SV.run_pre_sweep_batch(L0, acc)
        with pytest.raises(RuntimeError, match="fold ranks"):
            SV.fold_local_batch(L0, chunk, cts)
        with pytest.raises(RuntimeError, match="fold ranks"):
            SV.fold_root_batch(L0, gath, R.resp.data_ptr(), R.wire.data_ptr())
        L0[2].set_fold_ranks(G)
        with pytest.raises(RuntimeError, match="at most 8 clients"):
            SV.run_pre_sweep_batch(L0 * 3, acc)
        with pytest.raises(RuntimeError, match="listed twice"):
            SV.run_pre_sweep_batch([L0[0], L0[1], L0[1]], acc)
        with pytest.raises(RuntimeError, match="null"):
            SV.run_pre_sweep_batch(L0, 0)
        with pytest.raises(RuntimeError, match="null"):
            SV.fold_local_batch(L0, chunk, 0)
        with pytest.raises(RuntimeError, match="null"):
            SV.fold_root_batch(L0, 0, R.resp.data_ptr())
        with pytest.raises(RuntimeError, match="expansion is sharded"):
            L0s = R.lanes[1]
            for srv in L0s:
                srv.set_expand_shard(1, G)
            SV.run_pre_sweep_batch(L0s, R.acc[1].data_ptr())
        R.sync()
        for t, t0 in zip(R.outputs(), before):
            assert torch.equal(t, t0), "a refused call wrote an output"
    finally:
        other.close()
        R.close()
