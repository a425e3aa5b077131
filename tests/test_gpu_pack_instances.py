"""SpiralPack items of several database instances (include/spiral_gpu.h, spiral_gpu_pack_server_answer_batch_instances): B clients -- an owner and
its lanes -- fetch an item of F plaintexts each, F pack servers holding one database each.  Slot (q, k) must be bit-identical to client q's own
answer against instance k, and to the oracle's pack_answer on instance k's database, whatever the group size, the image forms or the query form."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2048
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# test_gpu_pack_batch.py's geometries (nu1, nu2, out_n, params): the matrix-core pass covers the first two
COVERED = (7, 7, 1, {})
DIRECT = (7, 7, 2, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1))
UNCOVERED = (6, 2, 2, {})
WIDE = (3, 2, 12, dict(t_gsw=3, t_conv=56, t_exp=56, qprime_bits=31, p_db=524288, direct_upload=1))  # n = 12, t_conv = 56, p = 2^19


@pytest.fixture(scope="module")
def sa():
    import torch  # (first: it ships its own HIP runtime)

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0
    return spiral_amd


@pytest.fixture(scope="module")
def P(sa):
    from spiral_amd import pack as _  # noqa: F401

    return sys.modules["spiral_amd.pack"]


@pytest.fixture
def group(sa):
    """sets option pack_item_group for one test and restores automatic grouping afterwards"""
    L = sa.lib()
    yield lambda g: L.spiral_gpu_set_option(b"pack_item_group", g) == 0 or pytest.fail("set_option")
    L.spiral_gpu_set_option(b"pack_item_group", 0)


def assert_eq(got, exp, what):
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[:5].tolist()}")


def seed_of(k):
    return 300 + 11 * k


class Item:
    """F instances (instance k: gen_db(seed_of(k)); instance 0 is the owner) and B clients (the owner and B - 1 of its lanes), each client with its own
    public parameters and a query for its own index"""

    def __init__(self, sa, O, geom, B, F, salt=0):
        nu1, nu2, out_n, kw = geom
        self.O, self.out_n = O, out_n
        self.po, self.pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
        self.s = O.pack_shape_of(self.po, out_n)
        self.instances = []
        for k in range(F):
            srv = sa.PackServer(self.pg, out_n)
            srv.gen_db(seed_of(k))
            self.instances.append(srv)
        owner = self.instances[0]
        self.servers = [owner] + [owner.create_lane() for _ in range(B - 1)]
        self.clients, self.idx, self.queries = [], [], []
        total = self.s.dim0 * self.s.num_per
        for q, srv in enumerate(self.servers):
            cl = O.PackClient(self.po, out_n, seed=50 + 13 * q + salt)
            cl.pp = cl.pub_params()
            srv.set_pub_params(*cl.pp)
            self.clients.append(cl)
            self.idx.append((salt + 5 + 7919 * q) % total if q else total - 1)
            self.queries.append(cl.query(self.idx[-1]))

    def close(self):
        for srv in self.servers[1:] + self.instances:
            srv.close()


@pytest.mark.parametrize("geom,F", [(COVERED, 2), (UNCOVERED, 5), (DIRECT, 3), (WIDE, 2)], ids=["covered", "uncovered", "direct", "n12"])
def test_one_client_matches_oracle(sa, P, oracle_mt, geom, F):
    O = oracle_mt
    it = Item(sa, O, geom, 1, F)
    resp, wire = P.answer_instances(it.servers[0], it.instances, it.queries[0], wire=True)
    assert resp.shape == (F, it.out_n + 1, it.out_n, N) and resp.dtype == np.uint64 and wire.shape[0] == F
    for k in range(F):
        exp, _ = O.pack_answer(it.po, it.out_n, it.queries[0], *it.clients[0].pp, O.pack_gen_db(it.po, it.out_n, seed_of(k)))
        assert_eq(resp[k], exp, f"instance {k}: response vs the oracle")
        assert_eq(it.clients[0].decode(resp[k]), O.pack_db_item(it.po, it.out_n, seed_of(k), it.idx[0]), f"instance {k}: decoded plaintext")
    it.close()


def test_slots_equal_single_answers(sa, P, oracle):
    """each slot's response and wire form == that instance's own answer + read_response_wire with the client's public parameters; B = F = 1 == answer"""
    it = Item(sa, oracle, UNCOVERED, 1, 3)
    q = it.queries[0]
    resp, wire = P.answer_instances(it.servers[0], it.instances, q, wire=True)
    one = P.answer_instances(it.servers[0], it.instances[:1], q)
    for k, inst in enumerate(it.instances):
        inst.set_pub_params(*it.clients[0].pp)
        r, _, _ = inst.answer(q)
        assert_eq(resp[k], r, f"instance {k}: response vs its own answer")
        assert_eq(wire[k], inst.read_response_wire(), f"instance {k}: wire form vs its own answer's")
        if k == 0:
            assert_eq(one[0], r, "B = F = 1 vs answer")
    it.close()


@pytest.mark.parametrize("geom", [COVERED, UNCOVERED], ids=["covered", "uncovered"])
@pytest.mark.parametrize("B,F", [(2, 2), (3, 3), (8, 2), (2, 3), (3, 2), (8, 3)])
def test_batches_equal_one_client_calls(sa, P, oracle, geom, B, F):
    it = Item(sa, oracle, geom, B, F, salt=B + F)
    covered = geom is COVERED
    if covered:  # mixed forms going in: instance 1 in limb planes, the others packed
        it.instances[1].set_db_format(P.DB_LIMBS)
    resp, wire = P.answer_batch_instances(it.servers, it.instances, it.queries, wire=True)
    assert resp.shape[:2] == (B, F) and wire.shape[:2] == (B, F)
    for inst in it.instances:
        assert inst.db_format() == (P.DB_LIMBS if covered else P.DB_PACKED)
    for q in range(B):
        one, w1 = P.answer_instances(it.servers[q], it.instances, it.queries[q], wire=True)
        assert_eq(resp[q], one, f"client {q}: batch vs its own item call")
        assert_eq(wire[q], w1, f"client {q}: wire forms")
        for k in range(F):
            assert_eq(it.clients[q].decode(resp[q, k]), oracle.pack_db_item(it.po, it.out_n, seed_of(k), it.idx[q]), f"client {q}, instance {k}: decoded")
    it.close()


def test_mixed_forms_one_client(sa, P, oracle):
    """B = 1 sweeps each instance in the form it is in: one limb-plane instance between packed ones"""
    it = Item(sa, oracle, COVERED, 1, 3)
    want = P.answer_instances(it.servers[0], it.instances, it.queries[0])
    it.instances[1].set_db_format(P.DB_LIMBS)
    got = P.answer_instances(it.servers[0], it.instances, it.queries[0])
    assert [i.db_format() for i in it.instances] == [P.DB_PACKED, P.DB_LIMBS, P.DB_PACKED]
    assert_eq(got, want, "mixed forms vs all packed")
    it.close()


@pytest.mark.parametrize("geom,B", [(COVERED, 2), (UNCOVERED, 1)], ids=["covered-B2", "uncovered-B1"])
def test_grouping_is_invisible(sa, P, oracle, group, geom, B):
    it = Item(sa, oracle, geom, B, 5)
    outs = {}
    for g in (1, 2, 3, 0):
        group(g)
        outs[g] = P.answer_batch_instances(it.servers, it.instances, it.queries, wire=True)
    for g in (2, 3, 0):
        assert_eq(outs[g][0], outs[1][0], f"pack_item_group {g}: responses vs groups of one")
        assert_eq(outs[g][1], outs[1][1], f"pack_item_group {g}: wire forms vs groups of one")
    it.close()


def wire_of(sa, O, q):
    return sa.raw_to_wire(O.from_ntt(np.ascontiguousarray(q).reshape(-1, 2, N)).reshape(-1, N))


@pytest.mark.parametrize("geom", [COVERED, UNCOVERED], ids=["covered", "uncovered"])
def test_wire_input_equals_raw_input(sa, P, oracle, geom):
    it = Item(sa, oracle, geom, 2, 3)
    stats = {}
    raw = P.answer_batch_instances(it.servers, it.instances, it.queries, wire=True, stats=stats)
    assert stats["total_us"] > 0
    qw = [wire_of(sa, oracle, q) for q in it.queries]
    got = P.answer_batch_instances_wire(it.servers, it.instances, qw, wire=True)
    assert_eq(got[0], raw[0], "responses")
    assert_eq(got[1], raw[1], "wire forms")
    one = P.answer_instances_wire(it.servers[1], it.instances, qw[1])
    assert_eq(one, raw[0][1], "one client from its wire form")
    it.close()


def test_updates_are_seen(sa, P, oracle):
    """update_db_items on instance 1 (on its own stream, no synchronisation) between two item calls: slot 1 decodes the new item, the others are unchanged"""
    O = oracle
    it = Item(sa, O, UNCOVERED, 2, 3)
    before = P.answer_batch_instances(it.servers, it.instances, it.queries)
    new = {q: O.pack_db_item(it.po, it.out_n, 999, it.idx[q]).reshape(it.s.trials, N) for q in range(2)}
    for t in range(it.s.trials):
        pts = np.stack([new[q][t] for q in range(2)])
        it.instances[1].update_db_items(t, O.pack_items(pts, 8), 8, it.idx)
    after = P.answer_batch_instances(it.servers, it.instances, it.queries)
    for q in range(2):
        assert_eq(it.clients[q].decode(after[q, 1]).reshape(it.s.trials, N), new[q], f"client {q}: the updated item")
        for k in (0, 2):
            assert_eq(after[q, k], before[q, k], f"client {q}, instance {k}: unchanged")
    it.close()


def test_argument_checks_with_real_handles(sa, P, oracle):
    O = oracle
    it = Item(sa, O, UNCOVERED, 2, 2)
    L = sa.lib()
    from spiral_amd._lib import U64P

    qs = [np.ascontiguousarray(q) for q in it.queries]
    n = it.out_n

    def refused(servers, instances, match, bytes_each=None):
        resp = np.full((len(servers), len(instances), n + 1, n, N), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
        wb = L.spiral_gpu_response_wire_bytes(C.byref(it.pg), n)
        wire = np.full((len(servers), len(instances), wb), 0x5A, dtype=np.uint8)
        hs = (C.c_void_p * len(servers))(*[s.h for s in servers])
        ins = (C.c_void_p * len(instances))(*[s.h for s in instances])
        if bytes_each is None:
            qp = (U64P * len(servers))(*[qs[i % 2].ctypes.data_as(U64P) for i in range(len(servers))])
            rc = L.spiral_gpu_pack_server_answer_batch_instances(hs, len(servers), ins, len(instances), qp, resp.ctypes.data_as(U64P), wire.ctypes.data, None)
        else:
            w = np.zeros(bytes_each, dtype=np.uint8)
            wp = (C.c_void_p * len(servers))(*([w.ctypes.data] * len(servers)))
            rc = L.spiral_gpu_pack_server_answer_batch_instances_wire(hs, len(servers), ins, len(instances), wp, bytes_each, resp.ctypes.data_as(U64P),
                                                                     wire.ctypes.data, None)
        assert rc != 0, match
        msg = L.spiral_gpu_last_error().decode()
        assert match in msg, msg
        assert (resp == 0xA5A5A5A5A5A5A5A5).all() and (wire == 0x5A).all(), f"{match}: an output was written"

    S = it.servers
    other_n = sa.PackServer(sa.make_params(6, 2), 1)
    other_n.gen_db(1)
    other_p = sa.PackServer(sa.make_params(6, 2, t_gsw=4), 2)
    other_p.gen_db(1)
    refused(S, [it.instances[1], other_n], "other parameters")
    refused(S, [other_p], "other parameters")
    sharded = sa.PackServer(it.pg, n, trial0=0, trial1=2)
    sharded.gen_db(1)
    refused(S, [it.instances[1], sharded], "trial-sharded")
    empty = sa.PackServer(it.pg, n)
    refused(S, [empty], "no database")
    bare = S[0].create_lane()
    refused([S[0], bare], it.instances, "public parameters")
    refused([S[0], S[0]], it.instances, "twice")
    foreign = it.instances[1].create_lane()
    foreign.set_pub_params(*it.clients[1].pp)
    refused([S[0], foreign], it.instances, "database image")
    want = L.spiral_gpu_pack_query_wire_bytes(C.byref(it.pg), n)
    refused(S, it.instances, "bytes per query", bytes_each=want - 7)
    # the clients' own image need not hold a database: a client of an image-less owner answers against the instances
    lone = sa.PackServer(it.pg, n)
    lone.set_pub_params(*it.clients[0].pp)
    got = P.answer_instances(lone, it.instances, it.queries[0])
    assert_eq(got, P.answer_instances(S[0], it.instances, it.queries[0]), "a client whose own image is empty")
    for srv in (other_n, other_p, sharded, empty, bare, foreign, lone):
        srv.close()
    it.close()


@pytest.mark.parametrize("args,env", [
    (["6", "2", "77", "a", "--high-rate", "--instances", "3"], {}),
    (["7", "7", "300", "a", "--high-rate", "--direct-upload", "--instances", "4"], {"OUTN": "2", "TGSW": "5", "TEXP": "2", "QPBITS": "19"}),
])
def test_cli_high_rate_instances(sa, args, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([os.path.join(ROOT, "spiral_amd", "spiral")] + args, capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    F = int(args[-1])
    assert "Is correct? : 1" in r.stdout
    assert f"Item of {F} plaintexts, Is correct?: " + " ".join(["1"] * F) in r.stdout, r.stdout[-2000:]
    assert f"Item of {F} plaintexts (one query, {F} database instances), device (GPU·us): " in r.stdout
