"""set_query_batch and read_response_wire_batch (include/spiral_gpu.h, spiral_amd/server.py): the queries of all lanes of a batch through one
lane-aware launch (csrc/query_ingest.hip), their responses through one read.  The expected value is always a TWIN server fed by the per-server
setter (set_query_wire / set_query_seeded) with the same message: the resident query, the folded ciphertext, the response and its wire form must
equal the twin's word for word.  Every lane has its own client, index and seed, so a kernel that reads another lane's message or seed shows."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2048
POLY = 7 * N

COMPRESSED = (4, 3, dict(t_gsw=4))                                         # 2 wire / 1 seeded polynomial per lane: the host-checked path
DIRECT = (5, 2, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1))  # 84 wire / 42 seeded polynomials per lane: the chunked path
COVERED = (6, 6, dict(t_gsw=8))                                            # batches sweep on the matrix cores
GEOMS = {"compressed": COMPRESSED, "direct": DIRECT, "covered": COVERED}
FORMS = ["wire", "seeded"]


@pytest.fixture(scope="module")
def sa():
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
    """one geometry: an owner with its database and seven lanes, lane b holding client b's keys, a twin server, and the clients' query messages in
    both forms with the twin's state for each -- computed once and shared by the tests of the module"""

    def __init__(self, sa, SV, O, geom, db_seed=77):
        nu1, nu2, kw = geom
        self.sa, self.SV, self.O, self.db_seed = sa, SV, O, db_seed
        self.po, self.pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
        self.total = 1 << (nu1 + nu2)
        self.owner = sa.Server(self.pg)
        self.owner.gen_db(db_seed)
        self.lanes = [self.owner] + [sa.Server(self.pg, share_db_of=self.owner) for _ in range(7)]
        self.twin = sa.Server(self.pg)
        self.twin.gen_db(db_seed)
        self.rng = np.random.default_rng(2000 + nu1 * 16 + nu2)
        self.clients = [O.Client(self.po, seed=500 + 13 * c) for c in range(8)]
        self.pp = [cl.pub_params() for cl in self.clients]
        for b in range(8):
            self.lanes[b].set_pub_params(*self.pp[b])
        self.queries, self.msgs, self.states, self.twin_client = {}, {}, {}, None

    def index(self, c, salt=0):
        return (11 + 953 * c + 137 * salt) % self.total

    def query(self, c, salt):
        """client c's query ciphertexts for index(c, salt), [ciphertext][row][residue][N]: drawn once (every call of the oracle client's query()
        draws fresh randomness), so both message forms and the oracle's answer speak of the same ciphertexts"""
        if (c, salt) not in self.queries:
            self.queries[(c, salt)] = self.clients[c].query(self.index(c, salt)).reshape(-1, 2, 2, N)
        return self.queries[(c, salt)]

    def msg(self, c, salt, form):
        """client c's query for index(c, salt) as a message: the wire form of its ciphertexts, or a seed of its own and row 1 of each"""
        if (c, salt, form) not in self.msgs:
            sa, O = self.sa, self.O
            q = self.query(c, salt)
            if form == "wire":
                m = sa.raw_to_wire(O.from_ntt(np.ascontiguousarray(q.reshape(-1, 2, N))).reshape(-1, N))
            else:
                seed = self.rng.integers(0, 256, size=32, dtype=np.uint8)
                m = np.concatenate([seed, sa.raw_to_wire(O.from_ntt(np.ascontiguousarray(q[:, 1])).reshape(-1, N))])
            self.msgs[(c, salt, form)] = m
        return self.msgs[(c, salt, form)]

    def read(self, srv, ran=True):
        SV = self.SV
        srv.sync()
        st = {"query": srv.read(SV.BUF_QUERY)}
        if ran:
            st.update(final=srv.read(SV.BUF_FINAL), response=srv.read(SV.BUF_RESPONSE), wire=srv.read_response_wire())
        return st

    def expected(self, c, salt, form):
        """the twin's state after its own setter of the same message and run_query with client c's keys"""
        if (c, salt, form) not in self.states:
            if self.twin_client != c:
                self.twin.set_pub_params(*self.pp[c])
                self.twin_client = c
            (self.twin.set_query_wire if form == "wire" else self.twin.set_query_seeded)(self.msg(c, salt, form))
            self.twin.run_query()
            self.states[(c, salt, form)] = self.read(self.twin)
        return self.states[(c, salt, form)]

    def check(self, srv, c, salt, form, what, ran=True):
        got, exp = self.read(srv, ran), self.expected(c, salt, form)
        for name in got:
            assert_eq(got[name], exp[name], f"{what}: {name}")

    def by_address(self):
        """the lanes in ascending order of their arena's device address"""
        return sorted(self.lanes, key=lambda s: s.acc()[0])


_worlds = {}


@pytest.fixture(scope="module")
def world(sa, SV, oracle):
    def get(name):
        if name not in _worlds:
            _worlds[name] = World(sa, SV, oracle, GEOMS[name])
        return _worlds[name]

    yield get
    for w in _worlds.values():
        for s in w.lanes[::-1] + [w.twin]:
            s.close()
    _worlds.clear()


@pytest.mark.parametrize("n", [1, 3, 8])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("geom", list(GEOMS))
def test_equals_per_server_setter(sa, world, geom, form, n):
    """1. every lane's resident query equals the twin's after its own setter, and the batch's folded ciphertexts and responses the twin's run_query
    (n = 8: the last arm of the lane select chain)"""
    w = world(geom)
    lanes = w.lanes[:n]
    msgs = [w.msg(b, 0, form) for b in range(n)]
    assert msgs[0].size == (sa.query_wire_bytes if form == "wire" else sa.query_seeded_bytes)(w.pg)
    if geom == "direct":
        assert (msgs[0].size - (32 if form == "seeded" else 0)) // POLY == (84 if form == "wire" else 42)
    sa.set_query_batch(lanes, msgs, form=form)
    for b in range(n):
        w.check(lanes[b], b, 0, form, f"{geom} {form} n={n} lane {b} after set_query_batch", ran=False)
    sa.run_query_batch(lanes)
    for b in range(n):
        w.check(lanes[b], b, 0, form, f"{geom} {form} n={n} lane {b} after the batch")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("geom", ["compressed", "direct"])
def test_server_order_is_kept(sa, world, geom, form):
    """2. the servers in an order neither ascending nor descending in arena address, the owner (which anchors nothing here) left out: message b is
    in server b"""
    w = world(geom)
    s = [x for x in w.by_address() if x is not w.owner]
    servers = [s[2], s[0], s[3], s[1]]
    addr = [x.acc()[0] for x in servers]
    assert addr != sorted(addr) and addr != sorted(addr, reverse=True)
    cs = [w.lanes.index(x) for x in servers]
    sa.set_query_batch(servers, [w.msg(c, 1, form) for c in cs], form=form)
    sa.run_query_batch(servers)
    for x, c in zip(servers, cs):
        w.check(x, c, 1, form, f"{geom} {form}: the lane of client {c}")


@pytest.mark.parametrize("chunk", [5, 1])
@pytest.mark.parametrize("form", FORMS)
def test_chunked_passes(sa, world, opts, form, chunk):
    """3. the direct-upload message in passes of 5 polynomials per lane (84 = 16 x 5 + 4, seeded 42 = 8 x 5 + 2) and of 1: the default's results"""
    w = world("direct")
    assert sa.get_option("query_batch_chunk") == 4096 // 8
    opts(query_batch_chunk=chunk)
    lanes = w.lanes[:3]
    sa.set_query_batch(lanes, [w.msg(b, 2, form) for b in range(3)], form=form)
    sa.run_query_batch(lanes)
    for b in range(3):
        w.check(lanes[b], b, 2, form, f"chunk {chunk}, {form}, lane {b}")
    with pytest.raises(sa.SpiralGpuError, match="out of range"):
        sa.set_option("query_batch_chunk", 0)


@pytest.mark.parametrize("form", FORMS)
def test_back_to_back_calls_reuse_the_ring(sa, world, form):
    """4. three unsynchronised calls on lane sets {0, 1}, {0, 2}, {0, 3} behind batches still in flight, lane 0's message different each time: the
    third call refills the pinned slot of the first.  Lane 0 ends with the third message, lanes 1 to 3 with their own"""
    w = world("compressed")
    lanes = w.lanes[:4]
    sa.set_query_batch(lanes, [w.msg(b, 0, form) for b in range(4)], form=form)
    for _ in range(10):  # work in flight in front of the ingests
        sa.run_query_batch(lanes)
    for k in (1, 2, 3):
        sa.set_query_batch([lanes[0], lanes[k]], [w.msg(0, 2 + k, form), w.msg(k, 1, form)], form=form)
    sa.run_query_batch(lanes)
    w.check(lanes[0], 0, 5, form, "lane 0 holds the third message")
    for k in (1, 2, 3):
        w.check(lanes[k], k, 1, form, f"lane {k} holds its own")


@pytest.mark.parametrize("form", FORMS)
def test_graphs_replay_the_new_queries(sa, world, form):
    """5. with use_graphs on, a batch captured on one set of queries replays set_query_batch's new ones without a re-capture"""
    w = world("covered")
    lanes = w.lanes[:3]
    w.owner.use_graphs(True)
    try:
        sa.set_query_batch(lanes, [w.msg(b, 0, form) for b in range(3)], form=form)
        for _ in range(2):  # capture, first replay
            sa.run_query_batch(lanes)
        w.check(lanes[2], 2, 0, form, "before the new queries")
        n0 = captures(sa)
        sa.set_query_batch(lanes, [w.msg(b, 1, form) for b in range(3)], form=form)
        sa.run_query_batch(lanes)
        for b in range(3):
            w.check(lanes[b], b, 1, form, f"replay on the new queries, lane {b}")
        assert captures(sa) == n0, "set_query_batch forced a re-capture"
    finally:
        w.owner.use_graphs(False)


def above_q(sa, msg, form, coeff):
    """msg with raw coefficient `coeff` of the wire part set to Q + 1"""
    bad = msg.copy()
    at = (32 if form == "seeded" else 0) + 7 * coeff
    bad[at:at + 7] = np.frombuffer(int(sa.Q + 1).to_bytes(7, "little"), dtype=np.uint8)
    return bad


@pytest.mark.parametrize("form", FORMS)
def test_host_found_coefficient_changes_nothing(sa, world, form):
    """6a. one coefficient above Q in lane 2's message, and the last coefficient of the last lane: the call names server and coefficient, every
    lane keeps its query and the batch reproduces the previous responses"""
    w = world("compressed")
    lanes = w.lanes[:4]
    good = [w.msg(b, 1, form) for b in range(4)]
    sa.set_query_batch(lanes, good, form=form)
    sa.run_query_batch(lanes)
    ncoeff = (good[0].size - (32 if form == "seeded" else 0)) // 7
    for lane, k in ((2, 777), (3, ncoeff - 1)):
        msgs = [w.msg(b, 2, form) for b in range(4)]
        msgs[lane] = above_q(sa, msgs[lane], form, k)
        with pytest.raises(sa.SpiralGpuError, match=rf"set_query_batch: server {lane}: coefficient {k} \(polynomial {k // N}, index {k % N}\) is above Q"):
            sa.set_query_batch(lanes, msgs, form=form)
        for b in range(4):
            w.check(lanes[b], b, 1, form, f"bad coefficient in lane {lane}: lane {b} unchanged")
        sa.run_query_batch(lanes)
        for b in range(4):
            w.check(lanes[b], b, 1, form, f"bad coefficient in lane {lane}: lane {b} answered again")


@pytest.mark.parametrize("form", FORMS)
def test_device_found_coefficient_drops_every_query(sa, world, form):
    """6b. direct upload: the device finds the coefficient; the call names server and coefficient, every lane of it is left without a query, and
    a good call restores service"""
    w = world("direct")
    lanes = w.lanes[:3]
    sa.set_query_batch(lanes, [w.msg(b, 0, form) for b in range(3)], form=form)
    msgs = [w.msg(b, 1, form) for b in range(3)]
    k = 40 * N + 2047
    msgs[1] = above_q(sa, msgs[1], form, k)
    with pytest.raises(sa.SpiralGpuError, match=rf"set_query_batch: server 1: coefficient {k} \(polynomial 40, index 2047\) is above Q"):
        sa.set_query_batch(lanes, msgs, form=form)
    with pytest.raises(sa.SpiralGpuError, match="needs its query and public parameters set first"):
        sa.run_query_batch(lanes)
    for b in range(3):
        with pytest.raises(sa.SpiralGpuError, match="must be set first"):
            lanes[b].run_query()
    sa.set_query_batch(lanes, [w.msg(b, 1, form) for b in range(3)], form=form)
    sa.run_query_batch(lanes)
    for b in range(3):
        w.check(lanes[b], b, 1, form, f"after a good call, lane {b}")


def test_refused_calls_change_nothing(sa, world):
    """6c. a wrong message size, the NTT form, a null entry, nine servers, a duplicate server, a server with another image: refused by name, with
    every lane as it was"""
    w = world("compressed")
    lanes = w.lanes[:3]
    good = [w.msg(b, 1, "wire") for b in range(3)]
    sa.set_query_batch(lanes, good, form="wire")
    sa.run_query_batch(lanes)
    new = [w.msg(b, 2, "wire") for b in range(3)]
    other = sa.Server(w.pg)
    other.gen_db(w.db_seed)
    extra = sa.Server(w.pg, share_db_of=w.owner)
    nine = w.lanes + [extra]
    cases = [
        (lanes, [m[:-7] for m in new], "wire", rf"{new[0].size - 7} bytes per message, the wire form of this query takes {new[0].size}"),
        (lanes, [w.msg(b, 2, "seeded") for b in range(3)], "wire", "bytes per message, the wire form"),
        (lanes, new, "seeded", "bytes per message, the seeded form"),
        (lanes, new, "ntt", "the NTT form is not taken"),
        (lanes, [new[0], None, new[2]], "wire", "null message 1"),
        (nine, [new[0]] * 9, "wire", "at most 8 clients"),
        ([lanes[0], lanes[1], lanes[0]], new, "wire", "server 2 listed twice"),
        ([lanes[0], other, lanes[2]], new, "wire", "server 1 does not sweep server 0's database image"),
    ]
    for k, (servers, msgs, form, err) in enumerate(cases):
        with pytest.raises(sa.SpiralGpuError, match=err):
            sa.set_query_batch(servers, msgs, form=form)
        for b in range(3):
            w.check(lanes[b], b, 1, "wire", f"case {k}: lane {b} unchanged")
    sa.run_query_batch(lanes)
    for b in range(3):
        w.check(lanes[b], b, 1, "wire", f"after the refused calls: lane {b} answered again")
    L = sa.lib()
    hs = (C.c_void_p * 3)(*[s.h for s in lanes])
    assert L.spiral_gpu_server_set_query_batch(hs, 3, 1, None, good[0].size) != 0 and "null message list" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_server_set_query_batch(hs, 3, 7, None, good[0].size) != 0 and "unknown message form 7" in L.spiral_gpu_last_error().decode()
    for s in (extra, other):
        s.close()


def test_batched_read_equals_per_lane_reads(sa, world):
    """7. after a batch of 8, lane b's slice of the one read equals its own read_response_wire; a capacity one byte short is refused"""
    w = world("covered")
    lanes = w.lanes
    sa.set_query_batch(lanes, [w.msg(b, 0, "wire") for b in range(8)], form="wire")
    sa.run_query_batch(lanes)
    out = sa.read_response_wire_batch(lanes)
    nb = sa.lib().spiral_gpu_response_wire_bytes(C.byref(w.pg), 2)
    assert out.shape == (8, nb) and out.dtype == np.uint8
    for b in range(8):
        assert_eq(out[b], lanes[b].read_response_wire(), f"lane {b}: its own read")
        assert_eq(out[b], w.expected(b, 0, "wire")["wire"], f"lane {b}: the twin's")
    assert_eq(sa.read_response_wire_batch([lanes[5]])[0], out[5], "a batch of one")
    L = sa.lib()
    hs = (C.c_void_p * 8)(*[s.h for s in lanes])
    buf = np.zeros(8 * nb, dtype=np.uint8)
    assert L.spiral_gpu_server_read_response_wire_batch(hs, 8, buf.ctypes.data_as(C.c_void_p), 8 * nb - 1) != 0
    assert f"response buffer of {8 * nb - 1} bytes, the wire forms of 8 lanes need {8 * nb}" in L.spiral_gpu_last_error().decode()
    assert not buf.any(), "a refused read wrote"
    assert L.spiral_gpu_server_read_response_wire_batch(hs, 8, None, 8 * nb) != 0 and "null output" in L.spiral_gpu_last_error().decode()


def test_oracle_end_to_end_from_a_key_store(sa, world):
    """8. n = 8, keys bound from a FULL store, queries through set_query_batch, responses through read_response_wire_batch and response_from_wire.
    Seeded form: the oracle's client keeps its secret key to itself and draws row 0 itself, so a seeded message of its query is no encryption it
    can decode; the responses are compared with the ORACLE's answer on those ciphertexts (row 0 the seed's expansion) instead, for the first and the
    last lane.  Wire form: every client decodes its own item with the oracle's client.  (./spiral's own client makes valid seeded encryptions:
    tests/test_cli_query_batch.py decodes those.)"""
    w = world("covered")
    O, lanes = w.O, w.lanes
    store = sa.KeyStore(w.pg, 8, form="full")
    for c in range(8):
        store.put(c, *w.pp[c])
    slots = [(b + 3) % 8 for b in range(8)]  # lane b serves client slots[b]
    sa.bind_keys(lanes, store, slots)
    sa.set_query_batch(lanes, [w.msg(c, 3, "seeded") for c in slots], form="seeded")
    sa.run_query_batch(lanes)
    out = sa.read_response_wire_batch(lanes)
    db = O.gen_db(w.po, w.db_seed)
    for b in (0, 7):
        c = slots[b]
        m = w.msg(c, 3, "seeded")
        q = w.query(c, 3).copy()
        q[:, 0] = sa.seed_expand(m[:32].tobytes(), 1, 0, q.shape[0]).reshape(-1, 2, N)
        resp = O.stage_rescale(w.po, O.answer(w.po, q, *w.pp[c], db))
        assert_eq(sa.response_from_wire(w.pg, out[b]).reshape(resp.shape), resp, f"seeded, lane {b} serving client {c}: the oracle's response")
    sa.set_query_batch(lanes, [w.msg(c, 3, "wire") for c in slots], form="wire")
    sa.run_query_batch(lanes)
    out = sa.read_response_wire_batch(lanes)
    for b, c in enumerate(slots):
        pt = w.clients[c].decode(sa.response_from_wire(w.pg, out[b]))
        assert_eq(pt, O.db_item(w.po, w.db_seed, w.index(c, 3)), f"wire, lane {b}: client {c} decodes its own item")
    for b in range(8):  # (the lanes' own keys again, for the tests that follow)
        lanes[b].set_pub_params(*w.pp[b])
    store.close()
