"""Column shards (create_column_shard, run_column_batch) with the ranks emulated in one process: G column-shard owners on one device, each with B - 1
lanes; the all-gather is a torch.cat.  The images: G shards reading into one buffer reassemble, byte for byte, what an unsharded server of the same
content reads, after every loader and in both image forms.  The answers: every client's final ciphertext, response and wire form are bit-identical to
its own run_query on an unsharded server, and decode to the oracle's item."""
import ctypes as C

import numpy as np
import pytest

N = 2048
KW = dict(t_gsw=4)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def sa():
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


def assert_bytes(got, exp, what):
    assert got.dtype == np.uint8 and got.shape == exp.shape, f"{what}: {got.dtype} {got.shape} for {exp.shape}"
    if not (got == exp).all():
        bad = np.flatnonzero(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} bytes differ, first at byte {bad[0]}")


def shards_of(sa, pg, G):
    return [sa.Server(pg, col_rank=g, col_ranks=G) for g in range(G)]


def read_all(shards, bits, total, item_bytes):
    """every shard's read_db_items into ONE buffer (poisoned first: a byte nobody writes shows)"""
    out = np.full(total * item_bytes, 0xA5, dtype=np.uint8)
    for srv in shards:
        srv.read_db_items(bits, out=out)
    return out


def close_all(*servers):
    for srv in servers:
        srv.close()


# ---- the image ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu1,nu2,G", [(4, 4, 2), (4, 4, 4), (5, 5, 4)])
def test_shards_reassemble_the_database_after_every_loader(sa, oracle, nu1, nu2, G):
    """gen_db, load_db_items in two calls cut at items that are no multiples of G, load_db of the oracle's reference layout: each time the G shards'
    read_db_items into one buffer == the unsharded server's; a shard alone writes its own items and no other byte"""
    O = oracle
    po, pg = O.make_params(nu1, nu2, **KW), sa.make_params(nu1, nu2, **KW)
    s = O.shape_of(po)
    total, ib = s.dim0 * s.num_per, sa.db_items_bytes(pg, 8, 1)
    ref, shards = sa.Server(pg), shards_of(sa, pg, G)
    try:
        ref.gen_db(31)
        want = ref.read_db_items(8)
        for srv in shards:
            srv.gen_db(31)
        assert_bytes(read_all(shards, 8, total, ib), want, "after gen_db")
        # one shard alone: its items ii = g (mod G), i.e. i = g (mod G), and nothing else
        g = G - 1
        alone = np.full(total * ib, 0xA5, dtype=np.uint8)
        shards[g].read_db_items(8, out=alone)
        alone = alone.reshape(total, ib)
        mine = np.arange(total) % G == g
        assert_bytes(alone[mine], want.reshape(total, ib)[mine], "a shard's own items")
        assert (alone[~mine] == 0xA5).all(), "a shard wrote another shard's bytes"
        ids = [0, total - 1, g, g + G, 3 * s.num_per + 1, total - 1]  # (any order, a duplicate, ids of other shards)
        at = np.full(len(ids) * ib, 0xA5, dtype=np.uint8)
        shards[g].read_db_items_at(8, ids, out=at)
        for k, i in enumerate(ids):
            got = at[k * ib:(k + 1) * ib]
            assert (got == want[i * ib:(i + 1) * ib]).all() if i % G == g else (got == 0xA5).all(), f"read_db_items_at, id {i}"
        # load_db_items: another database, in two calls whose boundaries are no multiples of G
        ref.gen_db(77)
        want2 = ref.read_db_items(8)
        assert not np.array_equal(want, want2)
        cut = total // 2 + 1
        assert cut % G and (total - 3) % G
        for srv in shards:
            srv.load_db_items(want2[:cut * ib], 8, 0, cut)
            srv.load_db_items(want2[cut * ib:], 8, cut, total - cut)
        assert_bytes(read_all(shards, 8, total, ib), want2, "after load_db_items in two calls")
        # a run in the middle, from an odd item to an odd item: only its items change
        lo, hi = 3, total - 3
        for srv in shards:
            srv.load_db_items(want[lo * ib:hi * ib], 8, lo, hi - lo)
        mixed = np.concatenate([want2[:lo * ib], want[lo * ib:hi * ib], want2[hi * ib:]])
        assert_bytes(read_all(shards, 8, total, ib), mixed, "after a partial load_db_items")
        # load_db: the oracle's reference-layout database
        db = O.gen_db(po, 5)
        ref.load_db(db)
        for srv in shards:
            srv.load_db(db)
        assert_bytes(read_all(shards, 8, total, ib), ref.read_db_items(8), "after load_db")
        for srv in shards:
            assert srv.db_format() == sa.server.DB_PACKED and srv.db_device_bytes() * G == ref.db_device_bytes()
            for call in (lambda: srv.read_db_item(0), lambda: srv.read_db_slots(0), lambda: srv.read_db_columns(0)):
                with pytest.raises(sa.SpiralGpuError, match="column shard"):
                    call()
    finally:
        close_all(ref, *shards)


@pytest.mark.parametrize("nu1,nu2,G,narrow", [(7, 7, 2, 0), (8, 6, 4, 1)], ids=["wide-L64", "narrow-L16"])
def test_shards_reassemble_from_limb_planes(sa, oracle, opts, nu1, nu2, G, narrow):
    """the same from the limb-plane form: 64 columns per shard (the wide form) and 16 (a narrow form, option sweep_narrow)"""
    SV = sa.server
    opts(sweep_narrow=narrow)
    pg = sa.make_params(nu1, nu2, **KW)
    s = sa.get_shape(pg)
    total, ib = s.dim0 * s.num_per, sa.db_items_bytes(pg, 8, 1)
    assert sa.column_shard_has_limb_form(pg, G)
    ref, shards = sa.Server(pg), shards_of(sa, pg, G)
    try:
        ref.gen_db(13)
        want = ref.read_db_items(8)
        for srv in shards:
            srv.gen_db(13)
            srv.set_db_format(SV.DB_LIMBS)
            assert srv.db_format() == SV.DB_LIMBS
        assert_bytes(read_all(shards, 8, total, ib), want, "limb planes after gen_db")
        # an update in this form, ids of every residue mod G, then the read again
        ids = [0, 1, G + 1, total - 1, total - 2, 5 * s.num_per + 2, 5 * s.num_per + 3]
        items = want.reshape(total, ib)[[(i * 7 + 3) % total for i in ids]].copy()
        ref.update_db_items(items, 8, ids)
        for srv in shards:
            srv.update_db_items(items, 8, ids)
            assert srv.db_format() == SV.DB_LIMBS
        assert_bytes(read_all(shards, 8, total, ib), ref.read_db_items(8), "limb planes after update_db_items")
    finally:
        close_all(ref, *shards)


def test_update_changes_exactly_the_holders_items(sa, oracle):
    """update_db_items with ids of every residue mod G, given to every shard: each changes the ids it holds and nothing else"""
    nu1, nu2, G = 5, 5, 4
    pg = sa.make_params(nu1, nu2, **KW)
    s = sa.get_shape(pg)
    total, ib = s.dim0 * s.num_per, sa.db_items_bytes(pg, 8, 1)
    shards = shards_of(sa, pg, G)
    try:
        for srv in shards:
            srv.gen_db(3)
        before = read_all(shards, 8, total, ib).reshape(total, ib)
        ids = [0, 1, 2, 3, 4 + 1, total - 1, total - 2, 9 * s.num_per + 6, 9 * s.num_per + 7, 17 * s.num_per + 31]
        assert {i % G for i in ids} == set(range(G))
        rng = np.random.default_rng(1)
        items = rng.integers(0, 256, size=(len(ids), ib), dtype=np.uint8)
        for g, srv in enumerate(shards):
            srv.update_db_items(items, 8, ids)
            one = np.full(total * ib, 0xA5, dtype=np.uint8)
            srv.read_db_items(8, out=one)
            one = one.reshape(total, ib)
            for i in range(g, total, G):
                exp = items[ids.index(i)] if i in ids else before[i]
                assert (one[i] == exp).all(), f"shard {g}, item {i}"
        after = read_all(shards, 8, total, ib).reshape(total, ib)
        changed = np.flatnonzero((after != before).any(axis=1))
        assert sorted(changed.tolist()) == sorted(ids)
        assert_bytes(after[ids], items, "the updated items")
    finally:
        close_all(*shards)


# ---- the answers ----------------------------------------------------------------------------------------------------------------------------
class ColRanks:
    """G emulated ranks: owners[g] = column shard g of G, lanes[g] = [owner, its lanes]; fixed device buffers (as a deployment keeps them)"""

    def __init__(self, sa, O, nu1, nu2, G, B, graphs, db_seed, clients):
        import torch

        from spiral_amd import dist as sdist

        self.sa, self.O, self.G, self.B = sa, O, G, B
        self.po, self.pg = O.make_params(nu1, nu2, **KW), sa.make_params(nu1, nu2, **KW)
        self.s = O.shape_of(self.po)
        self.clients, self.pps, self.db_seed = clients, [c.pub_params() for c in clients], db_seed
        self.lanes = []
        for g in range(G):
            own = sa.Server(self.pg, col_rank=g, col_ranks=G)
            own.gen_db(db_seed)
            srvs = [own] + [sa.Server(self.pg, share_db_of=own) for _ in range(B - 1)]
            assert all((x.col_rank, x.col_ranks) == (g, G) for x in srvs)
            for b, srv in enumerate(srvs):
                srv.set_pub_params(*self.pps[b])
            own.use_graphs(graphs)
            self.lanes.append(srvs)
        self.bufs = [sdist.column_batch_buffers(self.lanes[g], G) for g in range(G)]
        assert all(sorted(b) == ["cts", "gathered_cts", "responses"] for b in self.bufs)
        self.cts = [b["cts"] for b in self.bufs]
        self.gathered, self.resp = self.bufs[0]["gathered_cts"], self.bufs[0]["responses"]
        self.wire_bytes = sa.lib().spiral_gpu_response_wire_bytes(C.byref(self.pg), 2)
        self.wire = torch.zeros(B * self.wire_bytes, dtype=torch.uint8, device=self.resp.device)
        self.ref = sa.Server(self.pg)
        self.ref.gen_db(db_seed)

    def outputs(self):
        return [self.resp, self.wire, self.gathered] + self.cts

    def sync(self):
        import torch

        for srvs in self.lanes:
            srvs[0].sync()
        torch.cuda.synchronize()

    def answer(self, queries):
        """one step; returns the matrix-core sweeps the G run_column_batch calls made"""
        import torch

        sa = self.sa
        for g in range(self.G):
            for b in range(self.B):
                self.lanes[g][b].set_query(queries[b])
        m0 = sa.get_option("mfma_sweeps")
        for g in range(self.G):
            sa.run_column_batch(self.lanes[g], self.cts[g].data_ptr())
        self.sync()
        sweeps = sa.get_option("mfma_sweeps") - m0
        self.gathered.copy_(torch.cat(self.cts))  # the all-gather: [rank][lane][CT]
        self.sync()
        sa.fold_root_batch(self.lanes[0], self.gathered.data_ptr(), self.resp.data_ptr(), self.wire.data_ptr())
        self.sync()
        return sweeps

    def singles(self, queries):
        """each client's own run_query on the unsharded server: (final, response, wire)"""
        SV = self.sa.server
        out = []
        for pp, q in zip(self.pps, queries):
            self.ref.set_pub_params(*pp)
            self.ref.set_query(q)
            self.ref.run_query()
            self.ref.sync()
            out.append((self.ref.read(SV.BUF_FINAL).copy(), self.ref.read(SV.BUF_RESPONSE).copy(), self.ref.read_response_wire()))
        return out

    def check(self, exp, items, what):
        SV = self.sa.server
        resp = self.resp.cpu().numpy().view(np.uint64).reshape(self.B, -1)
        wire = self.wire.cpu().numpy().reshape(self.B, -1)
        wires = SV.read_response_wire_batch(self.lanes[0])
        for b in range(self.B):
            fin, rsp, wr = exp[b]
            root = self.lanes[0][b]
            assert np.array_equal(root.read(SV.BUF_FINAL), fin), f"{what}: client {b} final ciphertext"
            assert np.array_equal(root.read(SV.BUF_RESPONSE), rsp), f"{what}: client {b} response"
            assert np.array_equal(resp[b], rsp.reshape(-1)), f"{what}: client {b} response output"
            assert np.array_equal(wire[b], np.frombuffer(bytes(wr), dtype=np.uint8)), f"{what}: client {b} wire output"
            assert bytes(root.read_response_wire()) == bytes(wr) == bytes(wires[b]), f"{what}: client {b} read_response_wire"
            assert np.array_equal(self.clients[b].decode(rsp), items[b]), f"{what}: client {b} decodes to its item"

    def close(self):
        self.ref.close()
        for srvs in self.lanes:
            for srv in reversed(srvs):
                srv.close()


def query_pool(total, G, rng):
    """item 0, the last item, two items of one column residue mod G, then a draw"""
    return [0, total - 1, 5, 5 + 3 * G] + [int(i) for i in rng.integers(0, total, size=12)]


# geometry, G, B, graphs, option sweep_narrow, the pass runs on the matrix cores
CASES = [
    ((4, 4), 2, 3, False, 0, False),
    ((4, 4), 4, 2, True, 0, False),
    ((4, 4), 1, 2, False, 0, False),
    ((5, 5), 4, 8, False, 0, False),
    ((5, 5), 2, 1, True, 0, False),
    ((7, 7), 2, 8, True, 0, True),    # 64 columns per shard: the wide form, default options
    ((8, 6), 4, 3, True, 1, True),    # 16 columns: a narrow form
    ((8, 6), 8, 2, False, 1, True),   # 8 columns
    ((8, 6), 2, 3, False, 0, False),  # 32 columns without the option: the vector-ALU passes on the same image geometry
]


@pytest.mark.parametrize("geo,G,B,graphs,narrow,mfma", CASES, ids=[f"nu{g[0]}-{g[1]}-G{G}-B{B}{'-graphs' if gr else ''}{'-narrow' if nw else ''}" for g, G, B, gr, nw, _ in CASES])
def test_batch_matches_single_queries(sa, oracle, opts, geo, G, B, graphs, narrow, mfma):
    O = oracle
    nu1, nu2 = geo
    opts(sweep_narrow=narrow)
    clients = [O.Client(O.make_params(nu1, nu2, **KW), seed=100 + 7 * b + G) for b in range(B)]
    R = ColRanks(sa, O, nu1, nu2, G, B, graphs, 41 + G, clients)
    assert sa.column_shard_has_limb_form(R.pg, G) is mfma
    total = R.s.dim0 * R.s.num_per
    pool = query_pool(total, G, np.random.default_rng(G * 10 + B))
    try:
        caps = None
        for r in range(3 if graphs else 2):
            idxs = [pool[(2 * r + b) % len(pool)] for b in range(B)]
            qs = [c.query(i) for c, i in zip(clients, idxs)]
            sweeps = R.answer(qs)
            assert sweeps == (G if mfma and B >= 2 else 0), f"round {r}: {sweeps} matrix-core sweeps for {G} ranks"
            R.check(R.singles(qs), [O.db_item(R.po, R.db_seed, i) for i in idxs], f"G={G} B={B} round {r}")
            if graphs:
                if r == 0:
                    caps = sa.get_option("graph_captures")
                else:
                    assert sa.get_option("graph_captures") == caps, "a replayed step captured again"
        if mfma and B >= 2:
            assert all(srvs[0].db_format() == sa.server.DB_LIMBS for srvs in R.lanes)
    finally:
        R.close()


def test_update_between_replayed_steps_on_limb_planes(sa, oracle):
    """update_db_items between two replayed steps, the image in limb planes: the answers follow the update, nothing is captured again"""
    O = oracle
    nu1, nu2, G, B = 7, 7, 2, 4
    clients = [O.Client(O.make_params(nu1, nu2, **KW), seed=300 + b) for b in range(B)]
    R = ColRanks(sa, O, nu1, nu2, G, B, True, 5, clients)
    try:
        total = R.s.dim0 * R.s.num_per
        idxs = [3, 78, 1000, total - 1]
        qs = [c.query(i) for c, i in zip(clients, idxs)]
        R.answer(qs)
        assert all(srvs[0].db_format() == sa.server.DB_LIMBS for srvs in R.lanes)
        R.check(R.singles(qs), [O.db_item(R.po, R.db_seed, i) for i in idxs], "before the update")
        caps = sa.get_option("graph_captures")
        rng = np.random.default_rng(9)
        items = rng.integers(0, R.po.p_db, size=(2, 2, 2, N), dtype=np.uint64)
        ids = [78, total - 1]  # one on each shard
        assert {i % G for i in ids} == {0, 1}
        for srvs in R.lanes:
            srvs[0].update_db_items(O.pack_items(items, 64), 64, ids)
        R.ref.update_db_items(O.pack_items(items, 64), 64, ids)
        assert R.answer(qs) == G
        assert sa.get_option("graph_captures") == caps, "update_db_items forced a capture"
        want = [items[ids.index(i)] if i in ids else O.db_item(R.po, R.db_seed, i) for i in idxs]
        R.check(R.singles(qs), want, "after the update")
    finally:
        R.close()


def hip_runtime():
    """the HIP runtime this process already has loaded (torch's, which the library shares)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def test_refusals_write_nothing(sa, oracle):
    """a j-shard lane in the call, a column shard of another rank or rank count, n = 9, a null output, a lane without a query, a call during capture:
    refused before anything is launched, every output unchanged; and every call that has no meaning on a column shard fails by name and leaves the
    servers usable"""
    import torch

    O = oracle
    SV = sa.server
    nu1, nu2, G, B = 4, 4, 2, 3
    clients = [O.Client(O.make_params(nu1, nu2, **KW), seed=500 + b) for b in range(B)]
    R = ColRanks(sa, O, nu1, nu2, G, B, False, 8, clients)
    extra = []
    try:
        total = R.s.dim0 * R.s.num_per
        idxs = [5, total - 1, 0]
        qs = [c.query(i) for c, i in zip(clients, idxs)]
        R.answer(qs)
        for t in R.outputs():
            t.view(torch.uint8).fill_(0xA5)
        torch.cuda.synchronize()
        before = [t.clone() for t in R.outputs()]
        L0, out = R.lanes[0], R.cts[0].data_ptr()

        def other(**kw):
            srv = sa.Server(R.pg, **kw)
            extra.append(srv)
            srv.gen_db(8)
            srv.set_pub_params(*R.pps[2])
            srv.set_query(qs[2])
            return srv

        jshard = other(j_begin=0, j_end=R.s.dim0 // 2)
        with pytest.raises(sa.SpiralGpuError, match="run_column_batch: server 2 is not a column shard"):
            sa.run_column_batch(L0[:2] + [jshard], out)
        with pytest.raises(sa.SpiralGpuError, match="another rank or rank count"):
            sa.run_column_batch(L0[:2] + [R.lanes[1][2]], out)
        with pytest.raises(sa.SpiralGpuError, match="another rank or rank count"):
            sa.run_column_batch(L0[:2] + [other(col_rank=0, col_ranks=4)], out)
        with pytest.raises(sa.SpiralGpuError, match="does not sweep server 0's database image"):
            sa.run_column_batch(L0[:2] + [other(col_rank=0, col_ranks=2)], out)
        with pytest.raises(sa.SpiralGpuError, match="at most 8 clients"):
            sa.run_column_batch(L0 * 3, out)
        with pytest.raises(sa.SpiralGpuError, match="null output"):
            sa.run_column_batch(L0, 0)
        fresh = sa.Server(R.pg, share_db_of=L0[0])
        extra.append(fresh)
        fresh.set_pub_params(*R.pps[2])
        with pytest.raises(sa.SpiralGpuError, match="needs its query"):
            sa.run_column_batch(L0[:2] + [fresh], out)
        # a column shard mixed into the j-shard's and the unsharded calls
        with pytest.raises(sa.SpiralGpuError, match="column shard"):
            SV.run_pre_sweep_batch([jshard, L0[0]], out)
        # during capture
        hip = hip_runtime()
        st = C.c_void_p()
        assert hip.hipStreamCreate(C.byref(st)) == 0
        L0[1].set_stream(st.value)
        assert hip.hipStreamBeginCapture(st, 2) == 0  # (hipStreamCaptureModeRelaxed)
        try:
            with pytest.raises(sa.SpiralGpuError, match="capturing"):
                sa.run_column_batch(L0, out)
        finally:
            g = C.c_void_p()
            assert hip.hipStreamEndCapture(st, C.byref(g)) == 0
            if g.value:
                hip.hipGraphDestroy(g)
        L0[1].set_stream(0)
        hip.hipStreamDestroy(st)
        # the calls that refuse a column shard, each by name
        S = L0[0]
        acc = torch.zeros(16, dtype=torch.int64, device=R.resp.device).data_ptr()
        refused = {
            "run_query": S.run_query, "answer": lambda: S.answer(qs[0]), "run_query_batch": lambda: sa.run_query_batch(L0),
            "run_query_instances": lambda: S.run_query_instances([S], acc), "run_query_batch_instances": lambda: sa.run_query_batch_instances(L0, [S], acc),
            "run_pre_sweep": S.run_pre_sweep, "run_pre_sweep_batch": lambda: SV.run_pre_sweep_batch(L0, acc),
            "run_expand_pack": lambda: S.run_expand_pack(acc), "run_expand_pack_batch": lambda: SV.run_expand_pack_batch(L0, acc),
            "run_unpack_convert_sweep": lambda: S.run_unpack_convert_sweep(acc), "run_unpack_convert_sweep_batch": lambda: SV.run_unpack_convert_sweep_batch(L0, acc, acc),
            "fold_local": lambda: S.fold_local(acc, acc), "fold_local_batch": lambda: SV.fold_local_batch(L0, acc, acc),
            "set_expand_shard": lambda: S.set_expand_shard(0, 2), "set_sweep_stages": lambda: S.set_sweep_stages(2),
        }
        for name, call in refused.items():
            with pytest.raises(sa.SpiralGpuError, match=f"{name}: .*column shard"):
                call()
        with pytest.raises(sa.SpiralGpuError, match="fixed"):
            S.set_fold_ranks(4)
        S.set_fold_ranks(G)  # (its own count is no change)
        R.sync()
        for t, t0 in zip(R.outputs(), before):
            assert torch.equal(t, t0), "a refused call wrote an output"
        # ... and the servers answer afterwards
        R.answer(qs)
        R.check(R.singles(qs), [O.db_item(R.po, R.db_seed, i) for i in idxs], "after the refusals")
    finally:
        close_all(*extra)
        R.close()
