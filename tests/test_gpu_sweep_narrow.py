"""The narrow base forms of the batch's shared pass (csrc/sweep_mfma.hip, the W forms: workgroups of 4, 2, 1 waves per slot at 32, 16, 8 ciphertexts
per slot), taken only under option "sweep_narrow" = 1.  Every comparison is word for word: against each lane's own run_query on the PACKED image with
the option off (the vector-ALU sweep), and against the oracle for the first and the last lane.  nu1 = 6 has one piece of 128 terms per prime, nu1 = 7
two (the prime boundary, the run-ahead across work items); nu2 = 5, 4, 3 are the three widths; the batch sizes hit NT = 1, 2, 3, 4 and 6 tiles."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2048
WORDS = 6 * N
KW = dict(t_gsw=4)


@pytest.fixture(scope="module")
def sa():
    # torch first: it ships its own HIP runtime and the two must not be initialised in the opposite order
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


@pytest.fixture(scope="module")
def SV(sa):
    from spiral_amd import server

    return server


def assert_eq(got, exp, what):
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[:5].tolist()}")


def captures(sa):
    return sa.get_option("graph_captures")


class World:
    """an owner with database `db_seed` and B - 1 lanes, lane b with client b's keys and a query for its own index"""

    def __init__(self, sa, O, nu1, nu2, B, db_seed, j_begin=0, j_end=0, clients=None, fold_ranks=1):
        self.sa, self.O, self.B, self.db_seed = sa, O, B, db_seed
        self.po, self.pg = O.make_params(nu1, nu2, **KW), sa.make_params(nu1, nu2, **KW)
        self.total = 1 << (nu1 + nu2)
        self.owner = sa.Server(self.pg, 0, j_begin, j_end)
        self.owner.gen_db(db_seed)
        self.lanes = [self.owner] + [sa.Server(self.pg, share_db_of=self.owner) for _ in range(B - 1)]
        self.clients = clients or [O.Client(self.po, seed=900 + 31 * b + nu1 + nu2) for b in range(B)]
        self.pps = [cl.pub_params() for cl in self.clients]
        for srv, pp in zip(self.lanes, self.pps):
            srv.set_pub_params(*pp)
            if fold_ranks > 1:
                srv.set_fold_ranks(fold_ranks)
        self.idx = [(5 + 997 * b) % self.total for b in range(B)]
        self.idx[-1] = self.total - 1 - (B > 1)  # the last lane asks for the far end of the database
        self.queries = [cl.query(i) for cl, i in zip(self.clients, self.idx)]

    def set_queries(self):
        for srv, q in zip(self.lanes, self.queries):
            srv.set_query(q)

    def read(self):
        SV = self.sa.server
        for srv in self.lanes:
            srv.sync()
        return [(srv.read(SV.BUF_FINAL).copy(), srv.read(SV.BUF_RESPONSE).copy()) for srv in self.lanes]

    def singles(self):
        """every lane's own run_query"""
        self.set_queries()
        for srv in self.lanes:
            srv.run_query()
        return self.read()

    def batch(self):
        self.set_queries()
        self.sa.run_query_batch(self.lanes)
        return self.read()

    def close(self):
        for srv in reversed(self.lanes):
            srv.close()


def check_lanes(got, want, what):
    assert len(got) == len(want)
    for b, ((fin, resp), (wfin, wresp)) in enumerate(zip(got, want)):
        assert_eq(fin, wfin, f"{what}: lane {b} FINAL")
        assert_eq(resp, wresp, f"{what}: lane {b} RESPONSE")


# (nu1, nu2, B): B = 8, 5, 3, 8, 2, 8, 1 -> NT = 6, 4, 3, 6, 2, 6, 1 tiles
PARITY = [(6, 5, 8), (7, 5, 5), (6, 4, 3), (7, 4, 8), (6, 3, 2), (7, 3, 8), (7, 3, 1)]


@pytest.mark.parametrize("nu1,nu2,B", PARITY)
def test_parity(sa, SV, oracle, opts, nu1, nu2, B):
    """1. the shared pass, the one-query instance on the converted image, the image's read-back in both forms, and a replayed batch.  B = 1: a batch
    of one lane is that lane's run_query and converts nothing, so the image is converted by set_db_format and the batch is the NT = 1 instance"""
    O = oracle
    opts(sweep_narrow=0)
    w = World(sa, O, nu1, nu2, B, 77)
    try:
        owner = w.owner
        want = w.singles()
        assert owner.db_format() == SV.DB_PACKED
        db = O.gen_db(w.po, 77)
        for b in sorted({0, B - 1}):
            assert_eq(want[b][0], O.answer(w.po, w.queries[b], *w.pps[b], db), f"lane {b}: the reference run_query against the oracle")
        del db
        items = [0, w.total - 1, (w.total // 2 + 3) % w.total]
        want_items = [owner.read_db_item(i) for i in items]
        want_slots = owner.read_db_slots(0, 2)
        if B > 1:  # (with the option off a batch leaves the image alone and answers the same)
            check_lanes(w.batch(), want, "option off")
            assert owner.db_format() == SV.DB_PACKED

        opts(sweep_narrow=1)
        got = w.batch()
        if B == 1:
            assert owner.db_format() == SV.DB_PACKED, "a batch of one is a single query: it converts nothing"
            check_lanes(got, want, "option on, a batch of one on the packed image")
            owner.set_db_format(SV.DB_LIMBS)
            got = w.batch()
        assert owner.db_format() == SV.DB_LIMBS, "the batch converts the image under the option"
        check_lanes(got, want, f"({nu1},{nu2}) B={B}: the shared pass")
        check_lanes(w.singles(), want, "a single run_query on the LIMBS image")
        for i, wi in zip(items, want_items):
            assert_eq(owner.read_db_item(i), wi, f"read_db_item({i}) in LIMBS form")
        assert_eq(owner.read_db_slots(0, 2), want_slots, "read_db_slots(0, 2) in LIMBS form")

        for srv in w.lanes:
            srv.use_graphs(True)
        first = w.batch()
        c0 = captures(sa)
        second = w.batch()
        assert captures(sa) == c0, "the second batch is a replay"
        check_lanes(first, want, "the capturing batch")
        check_lanes(second, want, "the replayed batch")
        for srv in w.lanes:
            srv.use_graphs(False)

        owner.set_db_format(SV.DB_PACKED)
        assert owner.db_format() == SV.DB_PACKED
        for i, wi in zip(items, want_items):
            assert_eq(owner.read_db_item(i), wi, f"read_db_item({i}) converted back")
        assert_eq(owner.read_db_slots(0, 2), want_slots, "read_db_slots(0, 2) converted back")
    finally:
        w.close()


def test_option_semantics(sa, SV, oracle, opts):
    """2. the option decides whether an image TAKES the form, never what works on an image that is in it"""
    opts(sweep_narrow=0)
    w = World(sa, oracle, 6, 4, 3, 78)
    try:
        owner = w.owner
        want = w.singles()
        check_lanes(w.batch(), want, "option off")
        assert owner.db_format() == SV.DB_PACKED, "option off: a batch leaves the image packed"
        with pytest.raises(sa.SpiralGpuError, match="sweep_narrow"):
            owner.set_db_format(SV.DB_LIMBS)
        assert owner.db_format() == SV.DB_PACKED
        check_lanes(w.batch(), want, "after the refused conversion")

        sa.set_option("sweep_narrow", 1)
        owner.set_db_format(SV.DB_LIMBS)
        assert owner.db_format() == SV.DB_LIMBS
        check_lanes(w.batch(), want, "option on, converted by set_db_format")

        sa.set_option("sweep_narrow", 0)  # switched off while the image is in the form: nothing is stranded
        check_lanes(w.batch(), want, "option off again, image still LIMBS: batch")
        assert owner.db_format() == SV.DB_LIMBS
        check_lanes(w.singles(), want, "option off again, image still LIMBS: single queries")
        owner.set_db_format(SV.DB_PACKED)
        assert owner.db_format() == SV.DB_PACKED
        check_lanes(w.batch(), want, "converted back")
        assert owner.db_format() == SV.DB_PACKED
        with pytest.raises(sa.SpiralGpuError, match="sweep_narrow"):
            owner.set_db_format(SV.DB_LIMBS)
    finally:
        w.close()


def test_update_in_limb_form(sa, SV, oracle, opts):
    """3. update_db_items on the converted image: item 0, the last item, two neighbours in one slot and a few more"""
    O = oracle
    opts(sweep_narrow=1)
    w = World(sa, O, 6, 4, 3, 79)
    fresh = None
    try:
        owner, np_ = w.owner, 16
        ids = [0, w.total - 1, 5 * np_ + 3, 5 * np_ + 4, 37 * np_ + 15, (37 ^ 32) * np_ + 15, 63 * np_]
        assert len(set(ids)) == len(ids)
        pts = [O.db_item(w.po, 99, i) for i in ids]
        w.idx = [0, 5 * np_ + 4, w.total - 1]  # updated items, so the answers depend on the update
        w.queries = [cl.query(i) for cl, i in zip(w.clients, w.idx)]
        w.batch()
        assert owner.db_format() == SV.DB_LIMBS
        owner.update_db_items(O.pack_items(np.stack(pts), 8), 8, ids)
        assert owner.db_format() == SV.DB_LIMBS, "the image keeps its form"
        got = w.batch()

        sa.set_option("sweep_narrow", 0)
        fresh = sa.Server(w.pg)
        all_pts = [pts[ids.index(i)] if i in ids else O.db_item(w.po, 79, i) for i in range(w.total)]
        fresh.load_db_items(O.pack_items(np.stack(all_pts), 8), 8)
        want = []
        for pp, q in zip(w.pps, w.queries):
            fresh.set_pub_params(*pp)
            fresh.set_query(q)
            fresh.run_query()
            fresh.sync()
            want.append((fresh.read(SV.BUF_FINAL).copy(), fresh.read(SV.BUF_RESPONSE).copy()))
        assert fresh.db_format() == SV.DB_PACKED
        check_lanes(got, want, "batch after the update")
        for i in ids + [1, 5 * np_ + 2, 5 * np_ + 5, w.total - 2]:
            assert_eq(owner.read_db_item(i), fresh.read_db_item(i), f"read_db_item({i})")
        assert_eq(owner.read_db_slots(0, 4), fresh.read_db_slots(0, 4), "read_db_slots(0, 4)")
    finally:
        if fresh is not None:
            fresh.close()
        w.close()


def test_sharded_batch(sa, SV, oracle, opts):
    """4. two emulated ranks on the shards [0, 64) and [64, 128) of nu1 = 7, three clients: run_pre_sweep_batch's rank-major accumulators (the GS
    instances) with the option on equal those with it off"""
    import torch

    from spiral_amd import dist as sdist

    O = oracle
    G, B = 2, 3
    clients = [O.Client(O.make_params(7, 4, **KW), seed=640 + b) for b in range(B)]
    ranks = [World(sa, O, 7, 4, B, 80, 64 * g, 64 * (g + 1), clients=clients, fold_ranks=G) for g in range(G)]
    try:
        for r in ranks[1:]:
            r.queries = ranks[0].queries  # a client sends every rank the same query
        s = sa.get_shape(ranks[0].pg)
        acc = [torch.zeros(sdist.batch_acc_words(s, B), dtype=torch.int64, device="cuda") for _ in range(G)]

        def sweep():
            out = []
            for g, r in enumerate(ranks):
                acc[g].zero_()
                torch.cuda.synchronize()
                r.set_queries()
                SV.run_pre_sweep_batch(r.lanes, acc[g].data_ptr())
                for srv in r.lanes:
                    srv.sync()
                torch.cuda.synchronize()
                out.append(acc[g].cpu().numpy().view(np.uint64).copy())
            return out

        opts(sweep_narrow=0)
        want = sweep()
        assert all(r.owner.db_format() == SV.DB_PACKED for r in ranks)
        assert all(a.any() for a in want)
        sa.set_option("sweep_narrow", 1)
        got = sweep()
        assert all(r.owner.db_format() == SV.DB_LIMBS for r in ranks), "each rank's batch converts its shard"
        for g in range(G):
            assert_eq(got[g], want[g], f"rank {g}: rank-major accumulators")
    finally:
        for r in ranks:
            r.close()


def test_item_batch(sa, SV, oracle, opts):
    """5. three clients against an item of two database instances (run_query_batch_instances): one shared pass per instance"""
    import torch

    O = oracle
    B, F = 3, 2
    w = World(sa, O, 6, 5, B, 81)
    inst = [w.owner, sa.Server(w.pg)]
    inst[1].gen_db(82)
    wb = sa.lib().spiral_gpu_response_wire_bytes(C.byref(w.pg), 2)
    try:
        def run():
            resp = torch.zeros(B * F * WORDS, dtype=torch.int64, device="cuda")
            fin = torch.zeros(B * F * WORDS, dtype=torch.int64, device="cuda")
            wire = torch.zeros(B * F * wb, dtype=torch.uint8, device="cuda")
            w.set_queries()
            sa.run_query_batch_instances(w.lanes, inst, resp.data_ptr(), fin.data_ptr(), wire.data_ptr())
            for srv in w.lanes:
                srv.sync()
            torch.cuda.synchronize()
            return [t.cpu().numpy().copy() for t in (resp, fin, wire)]

        opts(sweep_narrow=0)
        want = run()
        assert all(sv.db_format() == SV.DB_PACKED for sv in inst)
        assert want[0].any() and want[2].any()
        sa.set_option("sweep_narrow", 1)
        got = run()
        assert all(sv.db_format() == SV.DB_LIMBS for sv in inst), "the item batch converts every instance image"
        for name, g, x in zip(("responses", "folded ciphertexts", "wire forms"), got, want):
            assert_eq(g, x, f"item batch: {name}")
    finally:
        inst[1].close()
        w.close()


@pytest.mark.parametrize("nu2", [4, 3])
def test_stage_api(sa, SV, oracle, opts, nu2):
    """6. first_dim_batch and the primitive multiplyQueriesByDatabase: the same accumulators with the option on and off (the primitive decides its
    sweep by the option; its results cannot tell)"""
    O = oracle
    B = 3
    w = World(sa, O, 6, nu2, B, 83)
    try:
        def stage():
            w.set_queries()
            for srv in w.lanes:
                srv.run_pre()
            sa.first_dim_batch(w.lanes)
            for srv in w.lanes:
                srv.sync()
            return [srv.read(SV.BUF_ACC).copy() for srv in w.lanes]

        opts(sweep_narrow=0)
        want = stage()
        assert w.owner.db_format() == SV.DB_PACKED
        sa.set_option("sweep_narrow", 1)
        got = stage()
        assert w.owner.db_format() == SV.DB_LIMBS
        for b in range(B):
            assert_eq(got[b], want[b], f"first_dim_batch: lane {b} accumulators")

        dim0, num_per = 64, 1 << nu2
        rng = np.random.default_rng(60 + nu2)
        res = [O.reorient_ciphertexts(np.stack([rng.integers(0, m, size=(dim0, 3, 2, N), dtype=np.uint64) for m in (O.P, O.B)], axis=-2)) for _ in range(B)]
        db = O.fill_db_random(9, dim0 * num_per * 4 * N)
        on = sa.multiplyQueriesByDatabase(res, db, dim0, num_per)
        sa.set_option("sweep_narrow", 0)
        off = sa.multiplyQueriesByDatabase(res, db, dim0, num_per)
        assert_eq(on, off, "multiplyQueriesByDatabase: option on against off")
        for b in (0, B - 1):
            assert_eq(on[b], O.multiply_query_by_database(res[b], db, dim0, num_per), f"multiplyQueriesByDatabase: query {b} against the oracle")
    finally:
        w.close()
