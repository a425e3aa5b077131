"""The SpiralPack record store on the device (include/spiral_gpu.h "Records", SpiralPack: PackServer.load_records, update_records, read_records,
read_records_at; Client(out_n).record_queries / decode_records).  Expected plaintexts come from the oracle's pack_db_item, expected bytes from the numpy
restatement of the layout and of the bit-level splice (tests/pack_records_restated.py); nothing expected comes from the code under test."""
import sys

import numpy as np
import pytest

import pack_records_restated as PR

pytestmark = pytest.mark.gpu
N = 2048


@pytest.fixture(scope="module")
def sa():
    # torch first: it ships its own HIP runtime and the two must not be initialised in the opposite order
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


@pytest.fixture(scope="module")
def P(sa):
    return sys.modules["spiral_amd.pack"]


def assert_eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp) if got.shape == exp.shape else []
        raise AssertionError(f"{what}: shapes {got.shape} / {exp.shape}, {len(bad)} of {got.size} differ, first at {bad[:5].tolist() if len(bad) else '-'}")


def both(sa, O, nu1, nu2, **kw):
    return O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)


def lay_of(po, out_n, S):
    return PR.layout(int(po.p_db), int(po.nu1), int(po.nu2), out_n, S)


def load_width(po):
    """the coefficient width at which read_db_items / load_db_items see every value below p_db: w, or w + 1 for a p_db that is no power of two"""
    w = int(po.p_db).bit_length() - 1
    return w if (1 << w) == int(po.p_db) else w + 1


class Model:
    """the items a record database should hold: item -> [trials][2048] coefficients, from `base` until an update replaces them"""

    def __init__(self, po, out_n, base):
        self.po, self.out_n, self.w, self.base, self.items = po, out_n, int(po.p_db).bit_length() - 1, base, {}

    def get(self, item):
        return self.items[item] if item in self.items else self.base(item)

    def update(self, S, ids, recs, instance=0):
        lay = lay_of(self.po, self.out_n, S)
        for r, rec in zip(ids, np.asarray(recs).reshape(len(ids), S)):
            item, off, nb, first = PR.place(lay, S, int(r), instance)
            self.items[item] = PR.splice(self.get(item), self.w, off, rec[first:first + nb])

    def records(self, S, ids, instance=0):
        """[n][S]: the bytes instance `instance` holds of each record; the other bytes 0xEE (what the tests prefill their buffers with)"""
        lay = lay_of(self.po, self.out_n, S)
        out = np.full((len(ids), S), 0xEE, dtype=np.uint8)
        for k, r in enumerate(ids):
            item, off, nb, first = PR.place(lay, S, int(r), instance)
            out[k, first:first + nb] = PR.cut(self.get(item), self.w, off, nb)
        return out

    def trial_streams(self, before, t, bits):
        """trial t's item stream: `before` [total][256 bits] with the replaced items' polynomial t"""
        want = before.copy()
        for i, pt in self.items.items():
            want[i] = PR.stream_of(pt[t], bits)
        return want


def oracle_model(O, po, out_n, seed):
    trials = out_n * out_n
    return Model(po, out_n, lambda i: O.pack_db_item(po, out_n, seed, i).reshape(trials, N))


def crafted_ids(lay, S, s):
    """the first and the last record; every record that touches trial 1's polynomial of item a (the polynomial is covered whole, its neighbours in part;
    at S = 3000, w = 8 record 0 of the item straddles the boundary of trials 0 and 1); where the first dimension has partner rows j / j + 64, a record in
    each item of a pair of one column and in a lone member of another pair; records in trials 2k and 2k + 1 of one item and one in the last trial"""
    pi, np_, trials = lay.per_item, s.num_per, s.trials
    pb = 256 * lay.coeff_bits
    rec = lambda item, k: item * pi + k % pi
    at = lambda item, t: rec(item, min(pi - 1, (t * pb + pb // 2) // S))  # a record of `item` with bytes in trial t's polynomial
    a = 5 * np_ + 2 % np_
    ids = {0, lay.capacity - 1, rec(a + 1, 3)}
    if trials > 1:
        ids |= {rec(a, k) for k in range(pi) if k * S < 2 * pb and (k + 1) * S > pb}
    if s.dim0 >= 128:
        ids |= {rec(10 * np_ + 3, 7), rec(74 * np_ + 3, 30), rec(33 * np_ + 5 % np_, 1)}
    b = 7 * np_ + 1
    k2 = 2 * ((trials - 1) // 2) - 2 if trials > 2 else 0
    ids |= {at(b, k2), at(b, min(k2 + 1, trials - 1)), at(b + np_, trials - 1)}
    ids = sorted(ids)
    ids.reverse()  # (the call's order is not the image's)
    return ids


def fixed_query(sa, pg, out_n, servers, idx):
    """one device client's public parameters on every server and one query for item idx (existing calls only)"""
    cl = sa.Client(pg, bytes([41] * 32), out_n=out_n)
    pp = cl.pub_params("seeded")
    for sv in servers:
        sv.set_pub_params_seeded(pp)
    q = cl.query(idx, "seeded")
    cl.close()
    return q


CASES = [  # name, (nu1, nu2, out_n, parameters), form, option pack_pair_blocks, record sizes
    ("422-packed", (4, 2, 2, {}), "packed", 0, (256, 3000, 1)),
    ("742-packed", (7, 4, 2, {}), "packed", 0, (256, 3000)),
    ("742-limbs", (7, 4, 2, {}), "limbs", 0, (256, 3000)),
    ("733-packed", (7, 3, 3, {}), "packed", 0, (256, 3000)),
    ("733-pairs", (7, 3, 3, {}), "limbs", 1, (256, 3000)),
    ("422-w5", (4, 2, 2, dict(p_db=32)), "packed", 0, (99,)),
    ("742-w5-limbs", (7, 4, 2, dict(p_db=32)), "limbs", 0, (99,)),
]


@pytest.mark.parametrize("name,geom,form,pairs,sizes", CASES, ids=[c[0] for c in CASES])
def test_update_and_read_in_every_form(sa, P, oracle, opts, name, geom, form, pairs, sizes):
    """1: crafted id sets of each record size into the trial images in the form they are in.  Every trial's read_db_items equals the model (no bit
    outside the ranges changed); the form is unchanged; read_records / read_records_at return the restated ranges, on the owner and on a lane; limb
    planes converted back are a fresh load of the model's streams, bit for bit and in the answer to one query."""
    O = oracle
    opts(pack_pair_blocks=pairs)
    nu1, nu2, out_n, kw = geom
    po, pg = both(sa, O, nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    total, trials, w = s.dim0 * s.num_per, s.trials, int(po.p_db).bit_length() - 1
    srv = sa.PackServer(pg, out_n)
    srv.gen_db(21)  # every coefficient is below p_db = 2^w: a record database
    fmt = P.DB_PACKED if form == "packed" else P.DB_LIMBS
    if form == "limbs":
        assert P.has_limb_form(pg, out_n)
        srv.set_db_format(P.DB_LIMBS)
    lane = srv.create_lane()
    model = oracle_model(O, po, out_n, 21)
    before = [srv.read_db_items(t, w).reshape(total, -1) for t in range(trials)]
    rng = np.random.default_rng(7)
    for S in sizes:
        lay = lay_of(po, out_n, S)
        ids = crafted_ids(lay, S, s)
        recs = rng.integers(0, 256, size=(len(ids), S), dtype=np.uint8)
        srv.update_records(recs, S, ids)
        model.update(S, ids, recs)
        assert srv.db_format() == fmt, "the image keeps its form"
        probe = ids + [min(i + 1, lay.capacity - 1) for i in ids[:6]] + [max(i - 1, 0) for i in ids[:6]] + ids[:2]
        assert_eq(srv.read_records_at(S, probe), model.records(S, probe), f"{name} S={S}: read_records_at")
        assert_eq(lane.read_records_at(S, probe[::-1]), model.records(S, probe[::-1]), f"{name} S={S}: read_records_at on a lane")
        first = max(0, min(lay.capacity - 1, 6 * lay.per_item - 3))
        n = min(lay.capacity - first, lay.per_item + 7)
        assert_eq(srv.read_records(S, first, n), model.records(S, range(first, first + n)), f"{name} S={S}: read_records across an item boundary")
    wants = [model.trial_streams(before[t], t, w) for t in range(trials)]
    for t in range(trials):
        assert_eq(srv.read_db_items(t, w).reshape(total, -1), wants[t], f"{name}: read_db_items of trial {t} (no bit outside the ranges changed)")
    if form == "limbs":
        srv.set_db_format(P.DB_PACKED)
        fresh = sa.PackServer(pg, out_n)
        for t in range(trials):
            fresh.load_db_items(t, wants[t], w)
        for t in range(trials):
            assert_eq(srv.read_db_items(t, 64), fresh.read_db_items(t, 64), f"{name}: trial {t} converted back == a fresh load of the updated database")
        q = fixed_query(sa, pg, out_n, [srv, fresh], 5 * s.num_per + 2 % s.num_per)
        assert_eq(srv.answer_seeded(q, want_packed=False)[0], fresh.answer_seeded(q, want_packed=False)[0], f"{name}: the raw answer to one query")
        fresh.close()
    lane.close()
    srv.close()


@pytest.mark.parametrize("kw,S", [({}, 99), ({}, 256), ({}, 3000), (dict(p_db=48), 99)], ids=["w8-S99", "w8-S256", "w8-S3000", "p48-S99"])
def test_load_records(sa, oracle, kw, S):
    """2: load_records (in two calls, the second range first) then every trial's read_db_items: the restated item stream cut at the trial's polynomial,
    padding zero; for p_db = 48 (w = 5) the same coefficients read 6 bits wide"""
    O = oracle
    out_n = 2
    po, pg = both(sa, O, 4, 2, **kw)
    lay = lay_of(po, out_n, S)
    w, cb, trials = lay.coeff_bits, load_width(po), out_n * out_n
    rng = np.random.default_rng(S)
    recs = rng.integers(0, 256, size=(lay.capacity, S), dtype=np.uint8)
    srv = sa.PackServer(pg, out_n)
    srv.gen_db(1)  # (what a partial load leaves alone would show)
    cut_at = 3 * lay.per_item
    got_lay = srv.load_records(recs[cut_at:], S, first_record=cut_at)
    srv.load_records(recs[:cut_at], S)
    assert (got_lay.per_item, got_lay.capacity, got_lay.item_bytes) == (lay.per_item, lay.capacity, lay.item_bytes)
    stream = PR.item_stream(lay, S, recs)
    assert (stream[:, lay.per_item * S:] == 0).all() and stream.shape == (64, lay.item_bytes)
    coeffs = PR.stream_coeffs(stream, w, trials)  # [item][trial][2048]
    for t in range(trials):
        want = np.stack([PR.stream_of(coeffs[i, t], cb) for i in range(len(coeffs))])
        assert_eq(srv.read_db_items(t, cb).reshape(len(coeffs), -1), want, f"trial {t}")
    assert_eq(srv.read_records(S), recs, "read_records of everything")
    srv.close()


def test_failures_leave_the_image_unchanged(sa, P, oracle):
    """3: a duplicate id, an id at the capacity, a call on a lane, an instance out of range: error returns, every trial byte-identical.  After
    fill_db_random a partial-polynomial update and a read fail naming the record, the trial and the coefficient, and the answer to a fixed query is
    bit-identical before and after."""
    O = oracle
    out_n, S = 2, 256
    po, pg = both(sa, O, 4, 2)
    s = O.pack_shape_of(po, out_n)
    lay = lay_of(po, out_n, S)
    srv = sa.PackServer(pg, out_n)
    srv.gen_db(9)
    lane = srv.create_lane()
    before = [srv.read_db_items(t, 64).copy() for t in range(s.trials)]
    two = np.full((2, S), 0x5A, dtype=np.uint8)
    L = sa.lib()
    import ctypes as C

    ids = (C.c_uint64 * 2)(5, 5)
    assert L.spiral_gpu_pack_server_update_records(srv.h, two.ctypes.data_as(C.c_void_p), S, 0, ids, 2) != 0 and b"given twice" in L.spiral_gpu_last_error()
    with pytest.raises(sa.SpiralGpuError, match="outside the database"):
        srv.update_records(two, S, [3, lay.capacity])
    with pytest.raises(sa.SpiralGpuError, match="outside the database"):
        srv.read_records_at(S, [lay.capacity])
    with pytest.raises(sa.SpiralGpuError, match="outside the database"):
        srv.read_records(S, lay.capacity - 1, 2)
    with pytest.raises(sa.SpiralGpuError, match="lane"):
        lane.update_records(two, S, [3, 4])
    with pytest.raises(sa.SpiralGpuError, match="lane"):
        lane.load_records(np.zeros((lay.per_item, S), dtype=np.uint8), S)
    with pytest.raises(sa.SpiralGpuError, match="instance 1"):
        srv.update_records(two, S, [3, 4], instance=1)
    with pytest.raises(sa.SpiralGpuError, match="instance 1"):
        srv.read_records_at(S, [3], instance=1)
    with pytest.raises(sa.SpiralGpuError, match="multiple"):
        srv.load_records(np.zeros((3, S), dtype=np.uint8), S)
    for t in range(s.trials):
        assert_eq(srv.read_db_items(t, 64), before[t], f"trial {t} after the refused calls")
    # an image that holds no record data
    srv.fill_db_random(77)
    q = fixed_query(sa, pg, out_n, [srv], 6)
    ans = srv.answer_seeded(q, want_packed=False)[0].copy()
    rid = 6 * lay.per_item + 9  # bytes [2304, 2560) of item 6: inside trial 1's polynomial, which has to be read
    with pytest.raises(sa.SpiralGpuError, match=rf"record {rid} \(trial 1, coefficient \d+"):
        srv.update_records(two[:1], S, [rid])
    with pytest.raises(sa.SpiralGpuError, match=rf"record {rid} \(trial 1, coefficient \d+"):
        srv.read_records_at(S, [rid])
    assert_eq(srv.answer_seeded(q, want_packed=False)[0], ans, "the answer to a fixed query after the failed update and read")
    # a whole-polynomial update reads nothing and goes through: 8 records of 256 bytes are trial 2 of item 6
    whole = np.arange(8 * S, dtype=np.uint32).astype(np.uint8).reshape(8, S)
    wid = [6 * lay.per_item + 16 + k for k in range(8)]
    srv.update_records(whole, S, wid)
    assert_eq(srv.read_records_at(S, wid), whole, "records that cover a polynomial whole, on an image that holds no record data elsewhere")
    lane.close()
    srv.close()


def test_failing_read_names_the_lowest_position(sa, oracle):
    """3: of two failing records the one at the lower position in the call is named"""
    O = oracle
    out_n, S = 2, 256
    po, pg = both(sa, O, 4, 2)
    lay = lay_of(po, out_n, S)
    srv = sa.PackServer(pg, out_n)
    srv.fill_db_random(5)
    a, b = 9 * lay.per_item + 20, 2 * lay.per_item + 3
    with pytest.raises(sa.SpiralGpuError, match=rf"record {a} \(trial 2,"):
        srv.read_records_at(S, [a, b])
    with pytest.raises(sa.SpiralGpuError, match=rf"record {b} \(trial 0,"):
        srv.read_records_at(S, [b, a])
    srv.close()


def test_trial_shards_fill_one_buffer(sa, oracle):
    """4: servers for trials [0, 2) and [2, 4) of out_n = 2: each reads the bytes that lie in its trials and leaves the rest, so two calls fill one
    buffer; a record that straddles trials 1 and 2 is updated by one call on each"""
    O = oracle
    out_n, S = 2, 3000
    po, pg = both(sa, O, 4, 2)
    s = O.pack_shape_of(po, out_n)
    total = s.dim0 * s.num_per
    lay = lay_of(po, out_n, S)
    shards = [sa.PackServer(pg, out_n, trial0=0, trial1=2), sa.PackServer(pg, out_n, trial0=2, trial1=4)]
    for sh in shards:
        sh.gen_db(33)
    model = oracle_model(O, po, out_n, 33)
    before = [shards[t // 2].read_db_items(t, 8).reshape(total, -1) for t in range(4)]
    # record 1 of an item is bytes [3000, 6000): trials 1 and 2; record 0 lies in trials 0 and 1 (shard 0 alone)
    ids = [7 * lay.per_item + 1, 7 * lay.per_item, 30 * lay.per_item + 1, lay.capacity - 1]
    assert list(PR.trials_of(lay, 3000, 3000)) == [1, 2]
    rng = np.random.default_rng(4)
    recs = rng.integers(0, 256, size=(len(ids), S), dtype=np.uint8)
    for sh in shards:
        sh.update_records(recs, S, ids)
    model.update(S, ids, recs)
    for t in range(4):
        assert_eq(shards[t // 2].read_db_items(t, 8).reshape(total, -1), model.trial_streams(before[t], t, 8), f"trial {t}")
    probe = ids + [ids[0] + 1, 0, ids[0]]
    want = model.records(S, probe)
    out = np.full((len(probe), S), 0xEE, dtype=np.uint8)
    shards[0].read_records_at(S, probe, out=out)
    half = want.copy()
    for k, r in enumerate(probe):  # what shard 0 leaves alone: the bytes in trials 2 and 3
        _, off, nb, _ = PR.place(lay, S, r)
        cut = min(max(4096 - off, 0), nb)
        half[k, cut:] = 0xEE
    assert_eq(out, half, "shard 0 writes the bytes of trials 0 and 1 only")
    lane = shards[1].create_shard_lane()
    lane.read_records_at(S, probe, out=out)
    assert_eq(out, want, "the second shard (through a shard lane) fills in the rest")
    out = np.full((lay.per_item + 3, S), 0xEE, dtype=np.uint8)
    first = 7 * lay.per_item - 2
    for sh in shards:
        sh.read_records(S, first, len(out), out=out)
    assert_eq(out, model.records(S, range(first, first + len(out))), "read_records through both shards")
    with pytest.raises(sa.SpiralGpuError, match="lane"):
        lane.update_records(recs[:1], S, ids[:1])
    lane.close()
    for sh in shards:
        sh.close()


def test_records_of_several_instances(sa, oracle):
    """5: S = 20000 at out_n = 2, w = 8: three instance servers, each holding its chunk at byte 0 of item r; update and read through each"""
    O = oracle
    out_n, S = 2, 20000
    po, pg = both(sa, O, 4, 2)
    s = O.pack_shape_of(po, out_n)
    total = s.dim0 * s.num_per
    lay = lay_of(po, out_n, S)
    assert (lay.instances, lay.per_item, lay.capacity) == (3, 1, total)
    servers, models, before = [], [], []
    for f in range(3):
        sv = sa.PackServer(pg, out_n)
        sv.gen_db(50 + f)
        servers.append(sv)
        models.append(oracle_model(O, po, out_n, 50 + f))
        before.append([sv.read_db_items(t, 8).reshape(total, -1) for t in range(4)])
    ids = [total - 1, 0, 17]
    rng = np.random.default_rng(11)
    recs = rng.integers(0, 256, size=(len(ids), S), dtype=np.uint8)
    for f, sv in enumerate(servers):
        sv.update_records(recs, S, ids, instance=f)
        models[f].update(S, ids, recs, instance=f)
    probe = [17, 3, total - 1, 17]
    out = np.full((len(probe), S), 0xEE, dtype=np.uint8)
    want = np.full((len(probe), S), 0xEE, dtype=np.uint8)
    for f, sv in enumerate(servers):
        sv.read_records_at(S, probe, out=out, instance=f)
        first, nb = f * lay.item_bytes, min(S - f * lay.item_bytes, lay.item_bytes)
        want[:, first:first + nb] = models[f].records(S, probe, instance=f)[:, first:first + nb]
        assert_eq(out, want, f"after instance {f}: its chunk filled in, the later chunks untouched")
    assert_eq(out[0], recs[2], "an updated record through its three instances")
    assert_eq(out[2], recs[0], "another")
    for f, sv in enumerate(servers):
        for t in range(4):
            assert_eq(sv.read_db_items(t, 8).reshape(total, -1), models[f].trial_streams(before[f][t], t, 8), f"instance {f}, trial {t}")
    with pytest.raises(sa.SpiralGpuError, match="instance 3"):
        servers[0].read_records_at(S, probe, instance=3)
    for sv in servers:
        sv.close()


E2E = [("422", (4, 2, 2), 0, 1), ("733-pairs", (7, 3, 3), 1, 2)]


@pytest.mark.parametrize("name,geom,pairs,batch", E2E, ids=[c[0] for c in E2E])
def test_end_to_end(sa, P, oracle, opts, name, geom, pairs, batch):
    """6: Client(out_n).record_queries -> answer (or answer_batch) -> decode_records, in RAW and in WIRE form: the record's bytes before and after
    update_records, and word for word decode followed by packing at w bits and cutting"""
    O = oracle
    opts(pack_pair_blocks=pairs)
    nu1, nu2, out_n = geom
    po, pg = both(sa, O, nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    srv = sa.PackServer(pg, out_n)
    srv.gen_db(61)
    lanes = [srv] + [srv.create_lane() for _ in range(batch - 1)]
    cl = sa.Client(pg, bytes([7] * 32), out_n=out_n)
    for sv in lanes:
        sv.set_pub_params_seeded(cl.pub_params("seeded"))
    model = oracle_model(O, po, out_n, 61)
    rng = np.random.default_rng(2)
    for S in (256, 3000):
        lay = lay_of(po, out_n, S)
        item = 9 * s.num_per + 3
        rids = [item * lay.per_item + 1, (item + 1) * lay.per_item + lay.per_item - 1][:batch]
        for rnd in range(2):
            qs = cl.record_queries(rids, S, "seeded")
            if batch == 1:
                resp = srv.answer_seeded(qs[0], want_packed=False)[0][None]
                wire = srv.read_response_wire()[None]
            else:
                out, _ = P.answer_batch_seeded(lanes, list(qs))
                resp = np.stack([out[b][0] for b in range(batch)])
                wire = np.stack([sv.read_response_wire() for sv in lanes])
            want = model.records(S, rids)
            got = cl.decode_records(resp, rids, S, "raw")
            assert_eq(got, want, f"{name} S={S} round {rnd}: decode_records, RAW")
            assert_eq(cl.decode_records(wire, rids, S, "wire"), want, f"{name} S={S} round {rnd}: decode_records, WIRE")
            dec = cl.decode(resp).reshape(batch, s.trials, N)  # decode, then packing at w bits and cutting
            for b, r in enumerate(rids):
                _, off, nb, _ = PR.place(lay, S, r)
                assert_eq(got[b], PR.cut(dec[b], lay.coeff_bits, off, nb), f"{name} S={S}: record {r} == decode + pack + cut")
            if rnd == 0:
                recs = rng.integers(0, 256, size=(len(rids), S), dtype=np.uint8)
                srv.update_records(recs, S, rids)
                model.update(S, rids, recs)
    cl.close()
    for sv in lanes[1:] + [srv]:
        sv.close()


DRAW_GEOMS = [(4, 2, 2, {}, 0), (7, 3, 3, {}, 1)]


@pytest.mark.parametrize("seed", range(3))
def test_random_draws_equal_a_fresh_load(sa, P, oracle, opts, seed):
    """7: random ids and sizes over two geometries (the second in the pair form) are updated and compared with a fresh load of the model"""
    O = oracle
    rng = np.random.default_rng(500 + seed)
    nu1, nu2, out_n, kw, pairs = DRAW_GEOMS[seed % len(DRAW_GEOMS)]
    opts(pack_pair_blocks=pairs)
    po, pg = both(sa, O, nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    total, trials = s.dim0 * s.num_per, s.trials
    srv = sa.PackServer(pg, out_n)
    srv.gen_db(70 + seed)
    if pairs:
        srv.set_db_format(P.DB_LIMBS)
    model = oracle_model(O, po, out_n, 70 + seed)
    before = [srv.read_db_items(t, 8).reshape(total, -1) for t in range(trials)]
    for _ in range(3):
        S = int(rng.choice([1, 7, 99, 256, 777, 2048, 3000, 5000]))
        lay = lay_of(po, out_n, S)
        ids = rng.choice(lay.capacity, size=int(rng.integers(1, 24)), replace=False).tolist()
        recs = rng.integers(0, 256, size=(len(ids), S), dtype=np.uint8)
        srv.update_records(recs, S, ids)
        model.update(S, ids, recs)
        probe = ids + rng.integers(0, lay.capacity, size=5).tolist()
        assert_eq(srv.read_records_at(S, probe), model.records(S, probe), f"seed {seed}, S={S}: read_records_at")
    if pairs:
        srv.set_db_format(P.DB_PACKED)
    fresh = sa.PackServer(pg, out_n)
    for t in range(trials):
        fresh.load_db_items(t, model.trial_streams(before[t], t, 8), 8)
        assert_eq(srv.read_db_items(t, 64), fresh.read_db_items(t, 64), f"seed {seed}: trial {t} == a fresh load of the model")
    fresh.close()
    srv.close()
