"""The key store (include/spiral_gpu.h spiral_gpu_key_store_*, spiral_amd/keys.py) and bind_keys: client keys resident on the device in the device
layout, bound to the lanes of a batch by one launch (csrc/keys.hip).  The expected value is always a TWIN server whose keys were set by
set_pub_params with the same matrices (row 0 of every matrix the seed's expansion): the expanded query, the GSW keys, the folded ciphertext and the
response after a bind must equal the twin's word for word -- the conversion and the fold read every polynomial of every key, so a wrong word in any
of the four key buffers shows.  One case is also checked against the oracle's answer."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2048
POLY_BYTES = 8 * N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")
KEY_BIND_BLOCKS = 256  # csrc/keys.hip kKeyBindBlocks: workgroups per lane, one polynomial each per pass

COMPRESSED = (4, 3, dict(t_gsw=4))
DIRECT = (5, 2, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1))  # no W_exp_left / W_exp_right: two absent parts
COVERED = (6, 6, dict(t_gsw=8))                                            # batches sweep on the matrix cores
GEOMS = {"compressed": COMPRESSED, "direct": DIRECT, "covered": COVERED}
PACK = (6, 2, 2, {})  # test_gpu_pack_lanes.py G_UNCOVERED


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


@pytest.fixture(scope="module")
def P(sa):
    from spiral_amd import pack as _  # noqa: F401

    return sys.modules["spiral_amd.pack"]


def assert_eq(got, exp, what):
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[:5].tolist()}")


def binds(sa):
    return sa.get_option("key_binds")


def seeded(sa, O, seed, domain, mats):
    """the client's half: mats = (NTT-form array, rows, cols) in message order (an absent matrix: fewer than 2N words).  Returns the seeded message
    and the arrays with row 0 of every matrix replaced by the seed's expansion (what the server must end up holding)"""
    k, sent, out = 0, [], []
    for m, r, c in mats:
        a = np.array(m, dtype=np.uint64, copy=True)
        out.append(a)
        if a.size < 2 * N:
            continue
        v = a.reshape(-1, r, c, 2, N)
        nm = v.shape[0]
        v[:, 0] = sa.seed_expand(seed, domain, k, nm * c).reshape(nm, c, 2, N)
        k += nm * c
        sent.append(v[:, 1:].reshape(-1, 2, N))
    raw = O.from_ntt(np.ascontiguousarray(np.concatenate(sent))).reshape(-1, N)
    return np.concatenate([np.frombuffer(seed, dtype=np.uint8), sa.raw_to_wire(raw)]), out


def wire_of(sa, O, *mats):
    raws = [O.from_ntt(np.ascontiguousarray(m).reshape(-1, 2, N)).reshape(-1, N) for m in mats if np.asarray(m).size >= 2 * N]
    return sa.raw_to_wire(np.concatenate(raws))


class World:
    """one geometry: an owner with its database and two lanes, a twin server, and clients made on demand -- client c's seeded and wire messages and
    its matrices with row 0 replaced (pp), all three the same keys; computed once and shared by the tests of the module"""

    def __init__(self, sa, SV, O, geom, db_seed=77):
        nu1, nu2, kw = geom
        self.sa, self.SV, self.O, self.db_seed = sa, SV, O, db_seed
        self.po, self.pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
        self.total = 1 << (nu1 + nu2)
        self.owner = sa.Server(self.pg)
        self.owner.gen_db(db_seed)
        self.lanes = [self.owner] + [sa.Server(self.pg, share_db_of=self.owner) for _ in range(2)]
        self.twin = sa.Server(self.pg)
        self.twin.gen_db(db_seed)
        self.rng = np.random.default_rng(1000 + nu1 * 16 + nu2)
        self.clients, self.answers = {}, {}

    def client(self, c):
        if c not in self.clients:
            sa, O, pg = self.sa, self.O, self.pg
            cl = O.Client(self.po, seed=300 + 17 * c)
            seed = self.rng.integers(0, 256, size=32, dtype=np.uint8).tobytes()
            pp = cl.pub_params()
            cl.seeded_msg, pp2 = seeded(sa, O, seed, 2, [(pp[0], 2, pg.t_exp), (pp[1], 2, pg.t_exp_right), (pp[2], 3, 2 * pg.t_conv), (pp[3], 3, 2 * pg.t_conv)])
            cl.pp = tuple(pp2)
            cl.wire_msg = wire_of(sa, O, *cl.pp)
            cl.queries = {}
            self.clients[c] = cl
        return self.clients[c]

    def index(self, c, salt=0):
        return (7 + 977 * c + 131 * salt) % self.total

    def query(self, c, salt=0):
        cl = self.client(c)
        if salt not in cl.queries:
            cl.queries[salt] = cl.query(self.index(c, salt))
        return cl.queries[salt]

    def state(self, srv):
        SV = self.SV
        srv.sync()
        return {n: srv.read(b) for n, b in (("expanded", SV.BUF_EXPANDED), ("gsw", SV.BUF_GSW), ("final", SV.BUF_FINAL), ("response", SV.BUF_RESPONSE))}

    def expected(self, c, salt=0):
        """the twin's state after set_pub_params of client c's matrices and its query: client c's own single answer"""
        if (c, salt) not in self.answers:
            self.twin.set_pub_params(*self.client(c).pp)
            self.twin.set_query(self.query(c, salt))
            self.twin.run_query()
            self.answers[(c, salt)] = self.state(self.twin)
        return self.answers[(c, salt)]

    def check(self, srv, c, salt, what):
        got, exp = self.state(srv), self.expected(c, salt)
        for name in exp:
            assert_eq(got[name], exp[name], f"{what}: {name}")

    def fill(self, store, cs, form="seeded"):
        for slot, c in enumerate(cs):
            put(store, slot, self.client(c), form)


def put(store, slot, cl, form):
    if form == "ntt":
        store.put(slot, *cl.pp)
    elif form == "wire":
        store.put_wire(slot, cl.wire_msg)
    else:
        store.put_seeded(slot, cl.seeded_msg)


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


def fresh_lane(sa, w):
    """a lane that has never had public parameters"""
    return sa.Server(w.pg, share_db_of=w.owner)


@pytest.mark.parametrize("geom", list(GEOMS))
def test_full_slots_every_put_form(sa, world, geom):
    """a FULL slot filled from the NTT form, the wire form and the seeded form of the same keys, bound to a server without public parameters, answered"""
    w = world(geom)
    cl = w.client(0)
    store = sa.KeyStore(w.pg, 3, form="full")
    assert store.slot_bytes() == sum(np.asarray(m).size // (2 * N) for m in cl.pp) * POLY_BYTES
    for slot, form in enumerate(("ntt", "wire", "seeded")):
        assert not store.has(slot)
        put(store, slot, cl, form)
        assert store.has(slot)
        lane = fresh_lane(sa, w)
        with pytest.raises(sa.SpiralGpuError, match="must be set first"):
            lane.run_query()
        sa.bind_keys([lane], store, [slot])
        lane.set_query(w.query(0))
        lane.run_query()
        w.check(lane, 0, 0, f"FULL slot put from the {form} form")
        lane.close()
    if geom == "compressed":  # ... and the oracle's answer on those keys
        O = w.O
        fin = O.answer(w.po, w.query(0), *cl.pp, O.gen_db(w.po, w.db_seed))
        assert_eq(w.expected(0)["final"], fin, "twin vs oracle: final ciphertext")
        assert_eq(w.expected(0)["response"], O.stage_rescale(w.po, fin), "twin vs oracle: response")
    store.close()


@pytest.mark.parametrize("geom", list(GEOMS))
def test_compact_slots(sa, world, geom):
    """a COMPACT slot takes the seeded form only; bound, row 0 regenerated on the device, it answers as the twin"""
    from spiral_amd import keys

    w = world(geom)
    cl = w.client(1)
    store = sa.KeyStore(w.pg, 2, form="compact")
    polys = sum(np.asarray(m).size // (2 * N) for m in cl.pp)
    sent = (cl.seeded_msg.size - 32) // (7 * N)
    assert store.slot_bytes() == keys.slot_bytes(w.pg, 0, "compact") == 256 + sent * POLY_BYTES and sent < polys
    with pytest.raises(sa.SpiralGpuError, match="compact store.*seeded form only"):
        store.put(0, *cl.pp)
    with pytest.raises(sa.SpiralGpuError, match="compact store.*seeded form only"):
        store.put_wire(0, cl.wire_msg)
    assert not store.has(0)
    with pytest.raises(sa.SpiralGpuError, match=f"{cl.seeded_msg.size - 7} bytes, the seeded form of these public parameters takes {cl.seeded_msg.size}"):
        store.put_seeded(1, cl.seeded_msg[:-7])
    assert not store.has(1)
    store.put_seeded(1, cl.seeded_msg)
    lane = fresh_lane(sa, w)
    sa.bind_keys([lane], store, [1])
    lane.set_query(w.query(1))
    lane.run_query()
    w.check(lane, 1, 0, "COMPACT slot")
    lane.close()
    store.close()


@pytest.mark.parametrize("form", ["full", "compact"])
def test_three_lanes_two_slot_sets_and_memo(sa, world, form):
    """three lanes, six clients: the batch with slots (0, 1, 2), (3, 4, 5), then (2, 0, 0) -- a duplicate slot and a lane swap.  Every lane equals
    its client's own single answer each time; key_binds grows by exactly the lanes whose binding changed"""
    w = world("covered")
    store = sa.KeyStore(w.pg, 6, form=form)
    w.fill(store, range(6))
    lanes = w.lanes
    lanes[0].set_pub_params(*w.client(5).pp)  # (forgets what an earlier test bound: every lane of the first bind is copied)
    for k, (slots, changed) in enumerate([((0, 1, 2), 3), ((3, 4, 5), 3), ((2, 0, 0), 3), ((2, 0, 0), 0), ((2, 1, 0), 1), ((2, 1, 0), 0)]):
        n0 = binds(sa)
        sa.bind_keys(lanes, store, slots)
        assert binds(sa) - n0 == changed, f"bind {k} of slots {slots}"
        for b, c in enumerate(slots):
            lanes[b].set_query(w.query(c, salt=k))
        sa.run_query_batch(lanes)
        for b, c in enumerate(slots):
            w.check(lanes[b], c, k, f"bind {k}, lane {b} serving client {c}")
    # set_pub_params forgets the memo: the same slots again copy that lane, and only it
    lanes[1].set_pub_params(*w.client(4).pp)
    n0 = binds(sa)
    sa.bind_keys(lanes, store, (2, 1, 0))
    assert binds(sa) - n0 == 1
    for b, c in enumerate((2, 1, 0)):
        lanes[b].set_query(w.query(c))
    sa.run_query_batch(lanes)
    for b, c in enumerate((2, 1, 0)):
        w.check(lanes[b], c, 0, f"after set_pub_params on lane 1: lane {b}")
    store.close()


@pytest.mark.parametrize("form", ["full", "compact"])
def test_graphs_replay_with_new_keys(sa, world, form):
    """with use_graphs on, a re-bind drops no capture (graph_captures does not grow) and the replay answers with the new keys"""
    w = world("covered")
    store = sa.KeyStore(w.pg, 4, form=form)
    w.fill(store, range(4))
    lanes = w.lanes[:2]
    w.owner.use_graphs(True)
    try:
        sa.bind_keys(lanes, store, (0, 1))
        for _ in range(2):  # capture, first replay
            for b, c in enumerate((0, 1)):
                lanes[b].set_query(w.query(c))
            sa.run_query_batch(lanes)
        w.check(lanes[1], 1, 0, "before the re-bind")
        n0 = sa.get_option("graph_captures")
        sa.bind_keys(lanes, store, (2, 3))
        for b, c in enumerate((2, 3)):
            lanes[b].set_query(w.query(c))
        sa.run_query_batch(lanes)
        for b, c in enumerate((2, 3)):
            w.check(lanes[b], c, 0, f"replay after the re-bind, lane {b}")
        assert sa.get_option("graph_captures") == n0, "a re-bind forced a re-capture"
    finally:
        w.owner.use_graphs(False)
    store.close()


def test_put_drop_and_ordering(sa, world):
    """a bind is a copy: a put of other keys to the slot leaves the bound lane's answers unchanged until it is re-bound (the put's new generation
    makes the re-bind copy); drop, then bind, fails; a failing put leaves the slot empty"""
    w = world("compressed")
    store = sa.KeyStore(w.pg, 2, form="full")
    w.fill(store, [0, 1])
    lane = w.lanes[1]
    sa.bind_keys([lane], store, [0])
    store.put_seeded(0, w.client(2).seeded_msg)  # (waits for the bind in flight, then overwrites the slot)
    lane.set_query(w.query(0))
    lane.run_query()
    w.check(lane, 0, 0, "after a put to the bound slot")
    n0 = binds(sa)
    sa.bind_keys([lane], store, [0])
    assert binds(sa) - n0 == 1, "the slot's content changed: the re-bind copies"
    lane.set_query(w.query(2))
    lane.run_query()
    w.check(lane, 2, 0, "re-bound after the put")
    store.drop(0)
    assert not store.has(0) and store.has(1)
    with pytest.raises(sa.SpiralGpuError, match=r"slot 0 \(lane 0\) is empty"):
        sa.bind_keys([lane], store, [0])
    lane.run_query()
    w.check(lane, 2, 0, "after the refused bind of a dropped slot")
    bad = w.client(1).wire_msg.copy()
    bad[-7:] = 0xFF
    with pytest.raises(sa.SpiralGpuError, match="is above Q"):
        store.put_wire(1, bad)
    assert not store.has(1), "a failing put leaves the slot empty"
    with pytest.raises(sa.SpiralGpuError, match="outside the store of 2 slots"):
        store.put_seeded(2, w.client(1).seeded_msg)
    with pytest.raises(sa.SpiralGpuError, match="outside the store of 2 slots"):
        sa.bind_keys([lane], store, [2])
    store.close()


def test_put_waits_for_binds_on_every_stream(sa, world):
    """two lane groups with owners of their own -- each on its own stream -- bind from one store; a put then waits for BOTH binds, not only the
    last one launched: the first group's bind, queued behind work in flight on its stream, still reads the slot's earlier content"""
    w = world("covered")
    store = sa.KeyStore(w.pg, 2, form="full")
    w.fill(store, [0, 1])
    first, second = w.lanes[1], sa.Server(w.pg)
    second.gen_db(w.db_seed)
    first.set_pub_params(*w.client(3).pp)
    first.set_query(w.query(3))
    for _ in range(20):  # work in flight in front of the first group's bind
        first.run_query()
    sa.bind_keys([first], store, [0])
    sa.bind_keys([second], store, [1])
    store.put_seeded(0, w.client(2).seeded_msg)
    for srv, c in ((first, 0), (second, 1)):
        srv.set_query(w.query(c))
        srv.run_query()
        w.check(srv, c, 0, f"bound before the put, client {c}")
    second.close()
    store.close()


def test_failing_bind_leaves_state_intact(sa, world):
    """every check comes before the launch: after a failing bind -- an empty slot among valid ones, a server of other parameters, a duplicate
    server, n = 9, a SpiralPack store on base servers -- every lane answers as before, with the batch before it still in flight on the streams"""
    w = world("covered")
    store = sa.KeyStore(w.pg, 4, form="full")
    w.fill(store, [0, 1, 2])  # (slot 3 stays empty)
    lanes = w.lanes
    sa.bind_keys(lanes, store, (0, 1, 2))
    other = sa.Server(sa.make_params(*COMPRESSED[:2], **COMPRESSED[2]))
    pack_store = sa.KeyStore(w.pg, 1, out_n=2, form="full")
    nine = lanes + [fresh_lane(sa, w) for _ in range(6)]
    cases = [
        (lanes, store, (0, 3, 2), r"slot 3 \(lane 1\) is empty"),
        ([lanes[0], other, lanes[2]], store, (0, 1, 2), "server 1 differs from server 0"),
        ([lanes[0], lanes[1], lanes[0]], store, (0, 1, 2), "server 2 listed twice"),
        (nine, store, (0,) * 9, "at most 8 clients"),
        (lanes, pack_store, (0, 0, 0), "other parameters"),
    ]
    for k, (servers, st, slots, msg) in enumerate(cases):
        for b in range(3):
            lanes[b].set_query(w.query(b, salt=k))
        sa.run_query_batch(lanes)  # not synchronised: the failing call meets streams with work in flight
        n0 = binds(sa)
        with pytest.raises(sa.SpiralGpuError, match=msg):
            sa.bind_keys(servers, st, slots)
        assert binds(sa) == n0
        for b in range(3):
            w.check(lanes[b], b, k, f"case {k}: the batch in flight, lane {b}")
        sa.run_query_batch(lanes)  # the keys, have_pp and the memos are what they were
        for b in range(3):
            w.check(lanes[b], b, k, f"case {k}: answered again, lane {b}")
        n0 = binds(sa)
        sa.bind_keys(lanes, store, (0, 1, 2))
        assert binds(sa) == n0, f"case {k}: the memos survived the failing call"
    for s in nine[3:] + [other]:
        s.close()
    pack_store.close()
    store.close()


@pytest.mark.parametrize("form", ["full", "compact"])
def test_ragged_sizes(sa, world, form):
    """the compressed geometry has 688 key polynomials: more than one pass of the launch's KEY_BIND_BLOCKS workgroups per lane and no multiple of it
    (the last pass is ragged), parts that begin at polynomials 80 and 640 (no multiple of it either), and the W_exp matrices have rows = 2 (a compact
    slot's run of rows 1.. is one row of cols); the direct geometry has fewer polynomials than workgroups and two absent parts.  From a store of
    capacity 1, into two lanes at once"""
    for geom in ("compressed", "direct"):
        w = world(geom)
        cl = w.client(3)
        polys = [np.asarray(m).size // (2 * N) for m in cl.pp]
        if geom == "compressed":
            assert sum(polys) > KEY_BIND_BLOCKS and sum(polys) % KEY_BIND_BLOCKS and polys[0] % KEY_BIND_BLOCKS and (polys[0] + polys[1]) % KEY_BIND_BLOCKS
            assert polys[0] == w.sa.get_shape(w.pg).n_left * 2 * w.pg.t_exp
        else:
            assert polys[0] == polys[1] == 0 and 0 < sum(polys) < KEY_BIND_BLOCKS
        store = sa.KeyStore(w.pg, 1, form=form)
        put(store, 0, cl, "seeded")
        lanes = w.lanes[1:]
        for lane in lanes:
            lane.set_pub_params(*w.client(0).pp)
        sa.bind_keys(lanes, store, (0, 0))
        for lane in lanes:
            lane.set_query(w.query(3))
        sa.run_query_batch(lanes)
        for b, lane in enumerate(lanes):
            w.check(lane, 3, 0, f"{geom}, capacity 1, lane {b}")
        store.close()


@pytest.mark.parametrize("form", ["full", "compact"])
def test_pack_bind_keys(sa, P, oracle, form):
    """SpiralPack: two lanes, three clients in a store for out_n; after each bind a lane's answer_batch response and packed ciphertext equal those of
    a twin whose keys were set by set_pub_params_seeded of the same message"""
    O = oracle
    nu1, nu2, out_n, kw = PACK
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    rng = np.random.default_rng(606)
    owner = sa.PackServer(pg, out_n)
    owner.gen_db(41)
    lanes = [owner, owner.create_lane()]
    twin = sa.PackServer(pg, out_n)
    twin.gen_db(41)
    clients, msgs, wires = [O.PackClient(po, out_n, seed=100 + 17 * c) for c in range(3)], [], []
    for c in clients:
        wl, wr, v, vw = c.pub_params()
        seed = rng.integers(0, 256, size=32, dtype=np.uint8).tobytes()
        pm, pp2 = seeded(sa, O, seed, 4, [(wl, 2, pg.t_exp), (wr, 2, pg.t_exp_right), (v, 2, 2 * pg.t_conv), (vw, out_n + 1, pg.t_conv)])
        msgs.append(pm), wires.append(wire_of(sa, O, *pp2))
    store = sa.KeyStore(pg, 3, out_n=out_n, form=form)
    assert store.slot_bytes() == (wires[0].size // (7 * N) if form == "full" else (msgs[0].size - 32) // (7 * N)) * POLY_BYTES + (256 if form == "compact" else 0)
    for slot in range(3):
        if form == "full" and slot == 1:
            store.put_wire(slot, wires[slot])
        else:
            store.put_seeded(slot, msgs[slot])
    total = s.dim0 * s.num_per
    with pytest.raises(sa.SpiralGpuError, match="no public parameters"):
        P.answer_batch(lanes, [clients[0].query(1), clients[1].query(2)])
    base_store = sa.KeyStore(pg, 1, form="full")
    with pytest.raises(sa.SpiralGpuError, match="other parameters"):
        P.bind_keys(lanes, base_store, (0, 0))
    base_store.close()
    for k, (slots, changed) in enumerate([((0, 1), 2), ((2, 0), 2), ((2, 0), 0), ((2, 2), 1)]):
        n0 = binds(sa)
        P.bind_keys(lanes, store, slots)
        assert binds(sa) - n0 == changed, f"bind {k}"
        qs = [clients[c].query((1 + 7919 * c + 31 * k) % total) for c in slots]
        out, _ = P.answer_batch(lanes, qs, want_packed=True)
        for b, c in enumerate(slots):
            twin.set_pub_params_seeded(msgs[c])
            resp, packed, _ = twin.answer(qs[b])
            assert_eq(out[b][0], resp, f"bind {k}, lane {b} serving client {c}: response")
            assert_eq(out[b][1], packed, f"bind {k}, lane {b} serving client {c}: packed ciphertext")
    store.close()
    for srv in lanes[::-1] + [twin]:
        srv.close()


@pytest.mark.parametrize("extra", [[], ["compact"]], ids=["full", "compact"])
def test_cli_key_store(sa, extra):
    """./spiral --batch 3 --key-store [compact]: every client decodes its own item in both rounds of the rotated slot assignment"""
    r = subprocess.run([BIN, "4", "3", "40", "a", "--seed", "5", "--batch", "3", "--key-store"] + extra, capture_output=True, text=True,
                       env=dict(os.environ, TGSW="4"), timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rounds = re.findall(r"Key store round (\d), client (\d) on lane (\d), Is correct\?: (\d)", r.stdout)
    assert len(rounds) == 6 and all(ok == "1" for *_, ok in rounds), r.stdout
    assert {(int(rd), int(c), int(b)) for rd, c, b, _ in rounds} == {(rd, (b + rd) % 3, b) for rd in range(2) for b in range(3)}
    assert f"({'compact' if extra else 'full'} slots)" in r.stdout
