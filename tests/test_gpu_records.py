"""The record store on the device (include/spiral_gpu.h "Records": load_records, update_records, read_records, read_records_at).  Expected images come
from the oracle's db_item / encode_item, expected bytes from the numpy restatement of the layout and of the bit-level splice
(tests/records_restated.py); nothing expected comes from the code under test."""
import ctypes as C
import hashlib

import numpy as np
import pytest

import records_restated as R

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
def SV(sa):
    from spiral_amd import server

    return server


def assert_eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp) if got.shape == exp.shape else []
        raise AssertionError(f"{what}: shapes {got.shape} / {exp.shape}, {len(bad)} of {got.size} differ, first at {bad[:5].tolist() if len(bad) else '-'}")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def word(enc):
    """an oracle encoding's two residue limbs -> device words (p-residue | b-residue << 32)"""
    return enc[..., 0, :] | (enc[..., 1, :] << np.uint64(32))


def both(sa, O, nu1, nu2, **kw):
    return O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)


def lay_of(po, S):
    return R.layout(int(po.p_db), int(po.nu1), int(po.nu2), S)


def load_width(po):
    """the coefficient width at which read_db_items / load_db_items see every value below p_db: w, or w + 1 for a p_db that is no power of two"""
    w = int(po.p_db).bit_length() - 1
    return w if (1 << w) == int(po.p_db) else w + 1


class Model:
    """the plaintexts a record database should hold: item -> [2][2][2048] coefficients, from `base` until an update replaces them"""

    def __init__(self, po, base):
        self.po, self.w, self.base, self.items = po, int(po.p_db).bit_length() - 1, base, {}

    def get(self, item):
        return self.items[item] if item in self.items else self.base(item)

    def update(self, S, ids, recs, instance=0):
        lay = lay_of(self.po, S)
        for r, rec in zip(ids, np.asarray(recs).reshape(len(ids), S)):
            item, off, nb, first = R.place(lay, S, int(r), instance)
            self.items[item] = R.splice(self.get(item), self.w, off, rec[first:first + nb])

    def records(self, S, ids, instance=0):
        """[n][S]: the bytes instance `instance` holds of each record; the other bytes 0xEE (what the tests prefill their buffers with)"""
        lay = lay_of(self.po, S)
        out = np.full((len(ids), S), 0xEE, dtype=np.uint8)
        for k, r in enumerate(ids):
            item, off, nb, first = R.place(lay, S, int(r), instance)
            out[k, first:first + nb] = R.cut(self.get(item), self.w, off, nb)
        return out

    def stream(self, item, bits):
        return R.stream_of(self.get(item), bits)


def image_of(O, po, db, model):
    """the oracle database in read_db_slots' layout [z][ii][c][j][m] with the model's replaced items encoded by the oracle"""
    s = O.shape_of(po)
    want = db.reshape(N, s.num_per, 2, s.dim0, 2).copy()
    for i, pt in model.items.items():
        want[:, i % s.num_per, :, i // s.num_per, :] = word(O.encode_item(po, pt)).transpose(2, 1, 0)  # [m][c][z] -> [z][c][m]
    return want


def crafted_ids(lay, S, s):
    """the first and the last record; every record that touches polynomial 1 of item a (the polynomial is covered whole, its neighbours in part); one
    record of item a + 1 whose neighbours stay; and, where the first dimension has partner rows j / j ^ 32, a record in each item of a pair of one column
    and in a lone member of another pair"""
    pi, np_ = lay.per_item, s.num_per
    rec = lambda item, k: item * pi + k % pi
    a = 5 * np_ + 16 % np_
    pb = 256 * lay.coeff_bits
    ids = {0, lay.capacity - 1, rec(a + 1, 3)}
    ids |= {rec(a, k) for k in range(pi) if k * S < 2 * pb and (k + 1) * S > pb}
    if s.dim0 >= 64:
        ids |= {rec(10 * np_ + 3, 7), rec(42 * np_ + 3, 30), rec(33 * np_ + 40 % np_, 1)}
    ids = sorted(ids)
    ids.reverse()  # (the call's order is not the image's)
    return ids


CASES = [  # name, (nu1, nu2, parameters), form, option sweep_narrow, record sizes
    ("66-packed", (6, 6, dict(t_gsw=8)), "packed", 0, (256, 3000)),
    ("66-limbs", (6, 6, dict(t_gsw=8)), "limbs", 0, (256, 3000)),
    ("66-w5-limbs", (6, 6, dict(t_gsw=8, p_db=32)), "limbs", 0, (99,)),
    ("64-narrow-limbs", (6, 4, dict(t_gsw=8)), "limbs", 1, (256, 3000)),
    ("43-narrow-packed", (4, 3, dict(t_gsw=8)), "packed", 0, (256, 3000, 1)),
    ("32-plain", (3, 2, dict(t_gsw=4)), "packed", 0, (3000, 99)),
    ("32-plain-w5", (3, 2, dict(t_gsw=4, p_db=32)), "packed", 0, (99,)),
]


@pytest.mark.parametrize("name,geom,form,narrow,sizes", CASES, ids=[c[0] for c in CASES])
def test_update_and_read_in_every_form(sa, SV, oracle, opts, name, geom, form, narrow, sizes):
    """2 / 3: crafted id sets of each record size into the image in the form it is in.  read_db_slots over every slot equals the oracle's encoding of the
    spliced plaintexts; read_db_items shows no bit changed outside the ranges; the form is unchanged; limb planes converted back are a fresh load.
    read_records / read_records_at return the restated ranges, on the owner and on a lane."""
    O = oracle
    opts(sweep_narrow=narrow)
    nu1, nu2, kw = geom
    po, pg = both(sa, O, nu1, nu2, **kw)
    s = O.shape_of(po)
    total, w = s.dim0 * s.num_per, int(po.p_db).bit_length() - 1
    db = O.gen_db(po, 21)  # every coefficient is below p_db = 2^w: a record database
    srv = sa.Server(pg)
    srv.gen_db(21)
    fmt = SV.DB_PACKED if form == "packed" else SV.DB_LIMBS
    if form == "limbs":
        assert sa.has_limb_form(pg)
        srv.set_db_format(SV.DB_LIMBS)
    lane = sa.Server(pg, share_db_of=srv)
    model = Model(po, lambda i: O.db_item(po, 21, i))
    before = srv.read_db_items(w).reshape(total, -1)
    rng = np.random.default_rng(7)
    for S in sizes:
        lay = lay_of(po, S)
        ids = crafted_ids(lay, S, s)
        recs = rng.integers(0, 256, size=(len(ids), S), dtype=np.uint8)
        srv.update_records(recs, S, ids)
        model.update(S, ids, recs)
        assert srv.db_format() == fmt, "the image keeps its form"
        # 3: the updated records, their neighbours, duplicates; a range across an item boundary; a lane
        probe = ids + [min(i + 1, lay.capacity - 1) for i in ids[:6]] + [max(i - 1, 0) for i in ids[:6]] + ids[:2]
        assert_eq(srv.read_records_at(S, probe), model.records(S, probe), f"{name} S={S}: read_records_at")
        assert_eq(lane.read_records_at(S, probe[::-1]), model.records(S, probe[::-1]), f"{name} S={S}: read_records_at on a lane")
        first = max(0, min(lay.capacity - 1, 6 * lay.per_item - 3))
        n = min(lay.capacity - first, lay.per_item + 7)
        assert_eq(srv.read_records(S, first, n), model.records(S, range(first, first + n)), f"{name} S={S}: read_records")
        first = 5 * s.num_per * lay.per_item  # whole items (a layout without padding: the range export)
        assert_eq(lane.read_records(S, first, 2 * lay.per_item), model.records(S, range(first, first + 2 * lay.per_item)), f"{name} S={S}: read_records of whole items")
    assert_eq(srv.read_db_slots(0, N), image_of(O, po, db, model), f"{name}: read_db_slots")
    want = before.copy()
    for i in model.items:
        want[i] = model.stream(i, w)
    assert_eq(srv.read_db_items(w).reshape(total, -1), want, f"{name}: read_db_items (no bit outside the ranges changed)")
    if form == "limbs":
        srv.set_db_format(SV.DB_PACKED)
        fresh = sa.Server(pg)
        fresh.load_db_items(want, w)
        assert_eq(srv.read_db_slots(0, N), fresh.read_db_slots(0, N), f"{name}: converted back == a fresh load of the updated database")
        fresh.close()
    lane.close()
    srv.close()


@pytest.mark.parametrize("geom,S", [((4, 3, dict(t_gsw=8)), 99), ((4, 3, dict(t_gsw=8)), 256), ((4, 3, dict(t_gsw=8)), 3000), ((4, 3, dict(t_gsw=8, p_db=32)), 99),
                                    ((3, 2, dict(t_gsw=4, p_db=48)), 99)], ids=["w8-S99", "w8-S256", "w8-S3000", "w5-S99", "p48-S99"])
def test_load_records(sa, oracle, geom, S):
    """1: load_records (in two calls, the second range first) then read_db_items: the restated item stream, padding zero -- byte-identical to the
    records where there is no padding; for p_db = 48 (w = 5) the same coefficients read 6 bits wide"""
    O = oracle
    nu1, nu2, kw = geom
    po, pg = both(sa, O, nu1, nu2, **kw)
    lay = lay_of(po, S)
    w, cb = lay.coeff_bits, load_width(po)
    rng = np.random.default_rng(S)
    recs = rng.integers(0, 256, size=(lay.capacity, S), dtype=np.uint8)
    srv = sa.Server(pg)
    srv.gen_db(1)  # (what a partial load leaves alone would show)
    cut_at = 3 * lay.per_item
    got_lay = srv.load_records(recs[cut_at:], S, first_record=cut_at)
    srv.load_records(recs[:cut_at], S)
    assert (got_lay.per_item, got_lay.capacity) == (lay.per_item, lay.capacity)
    want = R.item_stream(lay, S, recs)
    if lay.per_item * S == lay.item_bytes:
        assert_eq(want.reshape(-1), recs.reshape(-1), "no padding: the records are the stream")
    if cb != w:
        want = R.stream_of(R.stream_coeffs(want, w), cb)
    assert_eq(srv.read_db_items(cb).reshape(-1), want.reshape(-1), f"S={S}: read_db_items after load_records")
    assert_eq(srv.read_records(S), recs, f"S={S}: read_records of everything")
    with pytest.raises(sa.SpiralGpuError, match="multiple"):
        srv.load_records(recs[1:1 + lay.per_item], S, first_record=1)
    srv.close()


def test_not_a_power_of_two(sa, oracle):
    """2 / 4 for p_db = 48 (w = 5): update_records on a loaded record database equals the oracle's encoding; a coefficient >= 2^w that a call would have to
    read fails it, named, with the image untouched, while calls that do not read it work"""
    O = oracle
    po, pg = both(sa, O, 3, 2, t_gsw=4, p_db=48)
    s = O.shape_of(po)
    S, total = 99, s.dim0 * s.num_per
    lay = lay_of(po, S)
    rng = np.random.default_rng(48)
    recs = rng.integers(0, 256, size=(lay.capacity, S), dtype=np.uint8)
    srv = sa.Server(pg)
    srv.load_records(recs, S)
    coeffs = R.stream_coeffs(R.item_stream(lay, S, recs), 5)
    model = Model(po, lambda i: coeffs[i])
    ids = crafted_ids(lay, S, s)
    new = rng.integers(0, 256, size=(len(ids), S), dtype=np.uint8)
    srv.update_records(new, S, ids)
    model.update(S, ids, new)
    zero = np.zeros(total * 4 * N, dtype=np.uint64)
    full = Model(po, None)
    full.items = {i: model.get(i) for i in range(total)}
    assert_eq(srv.read_db_slots(0, N), image_of(O, po, zero, full), "p_db = 48: read_db_slots")
    assert_eq(srv.read_records(S), np.stack([model.records(S, [r])[0] for r in range(lay.capacity)]), "p_db = 48: read_records")
    # coefficient 158 of item 0 holds bits 790 .. 794 of the stream: the end of record 0 (bits 0 .. 791) and the start of record 1
    bad = model.get(0).copy()
    bad.reshape(-1)[158] = 40
    srv.load_db_items(R.stream_of(bad, 6), 6, first_item=0, n_items=1)
    before = digest(srv.read_db_slots(0, N))
    with pytest.raises(sa.SpiralGpuError, match=r"record 1 \(polynomial 0, coefficient 158"):
        srv.read_records_at(S, [2, 1])
    with pytest.raises(sa.SpiralGpuError, match=r"record 0 \(polynomial 0, coefficient 158"):
        srv.update_records(new[:2], S, [4, 0])
    assert digest(srv.read_db_slots(0, N)) == before, "the failed update changed nothing"
    assert_eq(srv.read_records_at(S, [2, 3]), model.records(S, [2, 3]), "records that do not touch the coefficient")
    srv.close()


def test_failures_leave_the_image_unchanged(sa, SV, oracle):
    """4: a duplicate id, an id at the capacity, a call on a lane, and an image from fill_db_random (the message names the record and the coefficient):
    each raises and the image hashes the same as before"""
    O = oracle
    po, pg = both(sa, O, 6, 6, t_gsw=8)
    S = 256
    lay = lay_of(po, S)
    srv = sa.Server(pg)
    srv.gen_db(21)
    srv.set_db_format(SV.DB_LIMBS)
    lane = sa.Server(pg, share_db_of=srv)
    before = digest(srv.read_db_slots(0, N))
    recs = np.arange(3 * S, dtype=np.uint32).astype(np.uint8)
    L = sa.lib()
    with pytest.raises(ValueError, match="duplicate"):
        srv.update_records(recs, S, [3, 700, 3])
    ids = np.array([3, 700, 3], dtype=np.uint64)
    assert L.spiral_gpu_server_update_records(srv.h, recs.ctypes.data_as(C.c_void_p), S, 0, ids.ctypes.data_as(C.POINTER(C.c_uint64)), 3) != 0
    assert b"twice" in L.spiral_gpu_last_error()  # the library's own check
    with pytest.raises(sa.SpiralGpuError, match="outside"):
        srv.update_records(recs, S, [3, 700, lay.capacity])
    with pytest.raises(sa.SpiralGpuError, match="outside"):
        srv.read_records_at(S, [3, lay.capacity])
    with pytest.raises(sa.SpiralGpuError, match="outside"):
        srv.read_records(S, lay.capacity - 1, 2)
    with pytest.raises(sa.SpiralGpuError, match="owner"):
        lane.update_records(recs, S, [3, 700, 5])
    with pytest.raises(sa.SpiralGpuError, match="instance 1"):
        srv.update_records(recs, S, [3, 700, 5], instance=1)
    assert digest(srv.read_db_slots(0, N)) == before, "the image is byte-identical after every failed update"
    assert srv.db_format() == SV.DB_LIMBS
    srv.fill_db_random(5)
    fmt = srv.db_format()
    before = digest(srv.read_db_slots(0, N))
    with pytest.raises(sa.SpiralGpuError, match=r"no record data at record 9000 \(polynomial 1, coefficient \d+"):
        srv.update_records(recs, S, [9000, 700, 5000])  # every one fails; position 0 is record 9000: item 281, bytes 2048 .. 2303 (polynomial 1)
    with pytest.raises(sa.SpiralGpuError, match=r"no record data at record 700 \(polynomial 3, coefficient \d+"):
        lane.read_records_at(S, [700, 3])  # record 700: item 21, bytes 7168 .. 7423 (polynomial 3)
    assert digest(srv.read_db_slots(0, N)) == before and srv.db_format() == fmt, "a random image is byte-identical after the failed calls"
    lane.close()
    srv.close()


def test_graph_replays_read_the_new_record(sa, SV, oracle):
    """5: a captured one-query graph replays after update_records and returns the new record; nothing is captured again"""
    O = oracle
    po, pg = both(sa, O, 6, 6, t_gsw=8)
    S, r = 256, 700
    lay = lay_of(po, S)
    item, off, nb, _ = R.place(lay, S, r)
    cl = O.Client(po, seed=9)
    srv = sa.Server(pg)
    srv.gen_db(21)
    srv.set_pub_params(*cl.pub_params())
    srv.use_graphs(True)
    srv.set_query(cl.query(item))
    srv.run_query()
    srv.run_query()
    srv.sync()
    assert_eq(R.cut(cl.decode(srv.read(SV.BUF_RESPONSE)), 8, off, nb), R.cut(O.db_item(po, 21, item), 8, off, nb), "the record before the update")
    caps = sa.get_option("graph_captures")
    new = np.random.default_rng(3).integers(0, 256, size=S, dtype=np.uint8)
    srv.update_records(new, S, [r])
    srv.run_query()
    srv.sync()
    assert sa.get_option("graph_captures") == caps, "update_records forced a capture"
    assert_eq(R.cut(cl.decode(srv.read(SV.BUF_RESPONSE)), 8, off, nb), new, "the replayed graph returns the new record")
    srv.close()


def test_several_instances(sa, oracle):
    """6: S = 2.5 item_bytes at a small geometry: three servers take instance 0, 1, 2 of one buffer, on load and on read; then a partial last chunk is
    updated and the padding behind it stays"""
    O = oracle
    po, pg = both(sa, O, 4, 3, t_gsw=8)
    S = 20480
    lay = lay_of(po, S)
    assert (lay.instances, lay.per_item, lay.capacity) == (3, 1, 128)
    rng = np.random.default_rng(6)
    recs = rng.integers(0, 256, size=(lay.capacity, S), dtype=np.uint8)
    srvs = [sa.Server(pg) for _ in range(3)]
    for f, srv in enumerate(srvs):
        srv.load_records(recs, S, instance=f)
        stream = R.item_stream(lay, S, recs, f)
        assert_eq(srv.read_db_items(8).reshape(lay.capacity, -1), stream, f"instance {f}: the items after load_records")
    out = np.full((lay.capacity, S), 0xEE, dtype=np.uint8)
    for f, srv in enumerate(srvs):
        srv.read_records(S, out=out, instance=f)
    assert_eq(out, recs, "three instances fill one buffer")
    ids = [127, 0, 64]
    new = rng.integers(0, 256, size=(3, S), dtype=np.uint8)
    for f, srv in enumerate(srvs):
        srv.gen_db(40 + f)  # nonzero behind the last chunk: an update must not touch it
        model = Model(po, lambda i, f=f: O.db_item(po, 40 + f, i))
        srv.update_records(new, S, ids, instance=f)
        model.update(S, ids, new, f)
        for i in ids + [1, 126]:
            assert_eq(srv.read_db_items_at(8, [i]), model.stream(i, 8), f"instance {f}: item {i} after update_records")
    out = np.full((3, S), 0xEE, dtype=np.uint8)
    for f, srv in enumerate(srvs):
        srv.read_records_at(S, ids, out=out, instance=f)
    assert_eq(out, new, "the updated records, read back through the three instances")
    with pytest.raises(sa.SpiralGpuError, match="instance 3"):
        srvs[0].read_records_at(S, ids, instance=3)
    for srv in srvs:
        srv.close()


def test_shards_fill_one_buffer(sa, SV, oracle):
    """3: a j-shard pair (one in limb planes, one packed) and a column-shard pair: every shard is given every id, updates the records it holds and fills in
    its own records of a shared buffer"""
    O = oracle
    S = 256
    for tag, geom, make in [("j-shards", (7, 6), lambda pg: [sa.Server(pg, j_begin=0, j_end=64), sa.Server(pg, j_begin=64, j_end=128)]),
                            ("column shards", (5, 5), lambda pg: [sa.Server(pg, col_rank=g, col_ranks=2) for g in range(2)])]:
        po, pg = both(sa, O, *geom, t_gsw=8)
        s = O.shape_of(po)
        lay = lay_of(po, S)
        shards = make(pg)
        for srv in shards:
            srv.gen_db(5)
        if tag == "j-shards":
            shards[0].set_db_format(SV.DB_LIMBS)
        model = Model(po, lambda i: O.db_item(po, 5, i))
        pi, np_ = lay.per_item, s.num_per
        items = [0, 1, s.dim0 * np_ - 1, s.dim0 * np_ - 2, (s.dim0 // 2) * np_ + 1, (s.dim0 // 2 - 1) * np_ + 2, 20 * np_ + 9, (20 ^ (s.dim0 // 2)) * np_ + 9]
        ids = [i * pi + (3 * k) % pi for k, i in enumerate(items)] + [items[0] * pi + 4]
        rng = np.random.default_rng(11)
        recs = rng.integers(0, 256, size=(len(ids), S), dtype=np.uint8)
        for srv in shards:
            srv.update_records(recs, S, ids)
        model.update(S, ids, recs)
        probe = ids + [i + 1 for i in ids[:4]]
        out = np.full((len(probe), S), 0xEE, dtype=np.uint8)
        for srv in shards:
            srv.read_records_at(S, probe, out=out)
        assert_eq(out, model.records(S, probe), f"{tag}: read_records_at into one buffer")
        one = np.full((len(probe), S), 0xEE, dtype=np.uint8)
        shards[0].read_records_at(S, probe, out=one)
        assert (one == 0xEE).all(axis=1).any() and not (one == 0xEE).all(), f"{tag}: a shard leaves the records it does not hold alone"
        first, n = (s.dim0 // 2) * np_ * pi - 40, 80  # across the j-shards' boundary
        out = np.full((n, S), 0xEE, dtype=np.uint8)
        for srv in shards:
            srv.read_records(S, first, n, out=out)
        assert_eq(out, model.records(S, range(first, first + n)), f"{tag}: read_records into one buffer")
        whole = np.zeros(s.dim0 * np_ * lay.item_bytes, dtype=np.uint8)
        for srv in shards:
            srv.read_db_items(8, out=whole)
        whole = whole.reshape(-1, lay.item_bytes)
        for i in set(items):
            assert_eq(whole[i], model.stream(i, 8), f"{tag}: item {i}")
        for srv in shards:
            srv.close()


GEOMS = [(6, 6, dict(t_gsw=8)), (7, 6, dict(t_gsw=8)), (4, 3, dict(t_gsw=8, p_db=32)), (3, 2, dict(t_gsw=4)), (6, 6, dict(t_gsw=8, p_db=32))]


@pytest.mark.parametrize("seed", range(5))
def test_random_draws_equal_a_fresh_load(sa, SV, oracle, seed):
    """8: a seeded draw of geometry, form, record size, id set and sharding: read_db_items of the updated image is the restated item stream of the
    updated records, and read_records_at returns them"""
    O = oracle
    rng = np.random.default_rng(2000 + seed)
    nu1, nu2, kw = GEOMS[seed % len(GEOMS)]
    po, pg = both(sa, O, nu1, nu2, **kw)
    s = O.shape_of(po)
    w = int(po.p_db).bit_length() - 1
    S = int(rng.choice([1 + int(rng.integers(0, 40)), 99, 256, 1000 + int(rng.integers(0, 3000)), 1024 * w]))
    lay = lay_of(po, S)
    n_shards = int(rng.integers(1, 3)) if s.dim0 >= 128 else 1
    span = s.dim0 // n_shards
    limbs_ok = s.num_per >= 64 and 64 <= span <= 2048
    form = SV.DB_LIMBS if limbs_ok and rng.integers(2) else SV.DB_PACKED
    recs = rng.integers(0, 256, size=(lay.capacity, S), dtype=np.uint8)
    n = int(rng.integers(1, min(lay.capacity, 300)))
    ids = rng.choice(lay.capacity, size=n, replace=False)
    if limbs_ok:  # make sure some partner pairs are both present
        extra = [((i // lay.per_item) ^ (32 * s.num_per)) * lay.per_item + i % lay.per_item for i in ids[: n // 3]]
        ids = np.unique(np.concatenate([ids, extra]))
        rng.shuffle(ids)
    ids = [int(i) for i in ids]
    new = rng.integers(0, 256, size=(len(ids), S), dtype=np.uint8)
    after = recs.copy()
    after[ids] = new
    want = R.item_stream(lay, S, after)  # the restated stream of the updated records, padding zero
    for k in range(n_shards):
        j0, j1 = k * span, (k + 1) * span
        srv = sa.Server(pg, j_begin=j0, j_end=j1) if n_shards > 1 else sa.Server(pg)
        srv.load_records(recs, S)
        if form == SV.DB_LIMBS:
            srv.set_db_format(form)
        srv.update_records(new, S, ids)
        assert srv.db_format() == form
        got = np.full(want.size, 0xEE, dtype=np.uint8)
        srv.read_db_items(w, out=got)
        lo, hi = j0 * s.num_per, j1 * s.num_per  # the items of this shard's rows; the others are left alone
        assert_eq(got.reshape(want.shape)[lo:hi], want[lo:hi], f"draw {seed}: ({nu1}, {nu2}) S={S}, shard {k}/{n_shards}, form {form}: read_db_items")
        assert (got.reshape(want.shape)[:lo] == 0xEE).all() and (got.reshape(want.shape)[hi:] == 0xEE).all()
        held = [i for i in ids if j0 <= i // lay.per_item // s.num_per < j1]
        assert_eq(srv.read_records_at(S, held), after[held], f"draw {seed}: read_records_at")
        srv.close()


E2E = (4, 3, dict(t_gsw=4))  # tests/test_gpu_client.py BASE: its end-to-end checks decode reliably here


@pytest.mark.parametrize("S,form", [(256, "raw"), (256, "wire"), (99, "raw"), (20480, "raw"), (20480, "wire")])
def test_end_to_end(sa, oracle, S, form):
    """7: record_queries, the server (answer_instances over the layout's instance servers), decode_records: the loaded bytes; after update_records the
    new bytes.  And on uniformly random responses decode_records equals decode followed by the restated packing and cut."""
    O = oracle
    nu1, nu2, kw = E2E
    po, pg = both(sa, O, nu1, nu2, **kw)
    lay = lay_of(po, S)
    rng = np.random.default_rng(S)
    recs = rng.integers(0, 256, size=(lay.capacity, S), dtype=np.uint8)
    cl = sa.Client(pg, bytes(range(50, 82)))
    srvs = [sa.Server(pg) for _ in range(lay.instances)]
    for f, srv in enumerate(srvs):
        srv.load_records(recs, S, instance=f)
    srvs[0].set_pub_params(*cl.pub_params())
    ids = [5, lay.capacity - 1, 5, 3 * lay.per_item + lay.per_item // 2]

    def packed(resp):  # [n][instances][3][2][N] switched responses in the form under test
        return resp if form == "raw" else np.concatenate([O.response_to_wire(po, r) for r in resp.reshape(-1, 3, 2, N)])

    def fetch():
        qs = cl.record_queries(ids, S, "ntt")
        return np.stack([srvs[0].answer_instances(srvs, q)[0] for q in qs])

    assert_eq(cl.decode_records(packed(fetch()), ids, S, form), recs[ids], f"S={S} {form}: the loaded records")
    new = rng.integers(0, 256, size=(2, S), dtype=np.uint8)
    for f, srv in enumerate(srvs):
        srv.update_records(new, S, [ids[1], ids[0]], instance=f)
    recs[[ids[1], ids[0]]] = new
    assert_eq(cl.decode_records(packed(fetch()), ids, S, form), recs[ids], f"S={S} {form}: the records after update_records")
    # uniformly random responses: row 0 below q', the other rows below 4 p_db
    n = len(ids) * lay.instances
    rand = np.concatenate([rng.integers(0, int(cl.shape.qprime), size=(n, 1, 2, N), dtype=np.uint64),
                           rng.integers(0, 4 * int(po.p_db), size=(n, 2, 2, N), dtype=np.uint64)], axis=1)
    plain = cl.decode(rand).reshape(len(ids), lay.instances, 2, 2, N)
    want = np.zeros((len(ids), S), dtype=np.uint8)
    for k, r in enumerate(ids):
        for f in range(lay.instances):
            _, off, nb, first = R.place(lay, S, r, f)
            want[k, first:first + nb] = R.cut(plain[k, f], lay.coeff_bits, off, nb)
    assert_eq(cl.decode_records(packed(rand.reshape(len(ids), lay.instances, 3, 2, N)), ids, S, form), want, f"S={S} {form}: random responses")
    with pytest.raises(sa.SpiralGpuError, match="outside the database"):
        cl.decode_records(packed(rand.reshape(len(ids), lay.instances, 3, 2, N)), ids[:-1] + [lay.capacity], S, form)
    with pytest.raises(ValueError, match="responses"):
        cl.decode_records(packed(rand.reshape(len(ids), lay.instances, 3, 2, N)), ids[:-1], S, form)
    assert cl.decode_records(np.zeros(0, dtype=np.uint64 if form == "raw" else np.uint8), [], S, form).shape == (0, S), "no records: an empty array"
    cl.close()
    for srv in srvs:
        srv.close()


def test_one_record_named_many_times(sa, oracle):
    """3: read_records_at takes ids that are not distinct: one record named 70 000 times (more segments of one polynomial than 16 bits count) beside
    others, every copy complete"""
    O = oracle
    po, pg = both(sa, O, 4, 3, t_gsw=8)
    S = 256
    srv = sa.Server(pg)
    srv.gen_db(21)
    model = Model(po, lambda i: O.db_item(po, 21, i))
    ids = np.full(70_003, 1234, dtype=np.uint64)
    ids[[0, 35_000, 70_002]] = [7, 1235, 4095]
    got = srv.read_records_at(S, ids)
    want = model.records(S, [1234, 7, 1235, 4095])
    exp = np.broadcast_to(want[0], got.shape).copy()
    exp[[0, 35_000, 70_002]] = want[1:]
    assert_eq(got, exp, "70 000 copies of one record")
    srv.close()


def test_several_staging_passes(sa, oracle, opts):
    """1 / 3 / 4 with option db_stage_bytes small: load_records repacks a few items at a time, read_records and read_records_at stage a few records per
    pass (a lane and a shard pair too), and a coefficient that is no record data in a LATER pass fails the call and names the record"""
    O = oracle
    po, pg = both(sa, O, 3, 2, t_gsw=4, p_db=48)
    S = 99
    lay = lay_of(po, S)
    rng = np.random.default_rng(77)
    recs = rng.integers(0, 256, size=(lay.capacity, S), dtype=np.uint8)
    opts(db_stage_bytes=3 * 6144 + 100)  # three items of 6-bit coefficients per load pass
    srv = sa.Server(pg)
    srv.load_records(recs, S)
    assert_eq(srv.read_db_items(6).reshape(-1), R.stream_of(R.stream_coeffs(R.item_stream(lay, S, recs), 5), 6), "load_records in passes of three items")
    opts(db_stage_bytes=5 * S)  # five records per read pass
    assert_eq(srv.read_records(S), recs, "read_records in passes of five records")
    ids = rng.integers(0, lay.capacity, size=203)
    lane = sa.Server(pg, share_db_of=srv)
    assert_eq(lane.read_records_at(S, ids), recs[ids], "read_records_at in passes of five records, on a lane")
    shards = [sa.Server(pg, j_begin=0, j_end=4), sa.Server(pg, j_begin=4, j_end=8)]
    out = np.full((len(ids), S), 0xEE, dtype=np.uint8)
    for sh in shards:
        sh.load_records(recs, S)
        sh.read_records_at(S, ids, out=out)
    assert_eq(out, recs[ids], "a shard pair, each pass holding the records the shard has")
    # coefficient 158 of item 9 (the end of its record 0, the start of its record 1) made 40 >= 2^5: records 9 * 51 and 9 * 51 + 1 cannot be read
    coeffs = R.stream_coeffs(R.item_stream(lay, S, recs), 5)
    bad = coeffs[9].copy()
    bad.reshape(-1)[158] = 40
    srv.load_db_items(R.stream_of(bad, 6), 6, first_item=9, n_items=1)
    r = 9 * lay.per_item
    clean = [int(i) for i in ids if i not in (r, r + 1)]
    late = clean[:23] + [r + 1, r] + clean[23:40]  # positions 23 and 24: the fifth pass
    with pytest.raises(sa.SpiralGpuError, match=rf"record {r + 1} \(polynomial 0, coefficient 158"):
        srv.read_records_at(S, late)
    with pytest.raises(sa.SpiralGpuError, match=rf"record {r} \(polynomial 0, coefficient 158"):
        srv.read_records(S, r - 12, 30)
    assert_eq(srv.read_records_at(S, clean), recs[clean], "the records that do not touch the coefficient")
    for x in shards + [lane, srv]:
        x.close()
