"""Keyed records on the device (include/spiral_gpu.h "Keyed records": kv_load, kv_put, kv_delete, kv_get, Client.kv_queries, Client.kv_decode).
Expected tables, streams, values and `found` come from the restatement (tests/kv_restated.py) and from calls the oracle already checks
(read_db_items, read_db_slots against O.encode_item, decode); nothing expected comes from the code under test.  tests/test_kv_cpu.py shows that
the restated placement places every key of every key set used here."""
import hashlib
from itertools import islice

import numpy as np
import pytest

import kv_restated as K
import records_restated as R

pytestmark = pytest.mark.gpu
N = 2048
TK = K.TABLE_KEY
FP_KEY = (0x0123456789ABCDEF, 0x0FEDCBA987654321)


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


def lay_of(po, V):
    return K.layout(int(po.p_db), int(po.nu1), int(po.nu2), V)


def check_slots(O, po, srv, stream, items, what):
    """read_db_slots of the whole image against the oracle's encoding of the restated stream, at the items given"""
    s = O.shape_of(po)
    w = int(po.p_db).bit_length() - 1
    got = srv.read_db_slots(0, N).reshape(N, s.num_per, 2, s.dim0, 2)
    for i in items:
        want = word(O.encode_item(po, R.stream_coeffs(stream[i], w)[0])).transpose(2, 1, 0)  # [m][c][z] -> [z][c][m]
        assert_eq(got[:, i % s.num_per, :, i // s.num_per, :], want, f"{what}: read_db_slots, item {i}")


def fresh_keys(lay, first, count=120_000):
    """keys never loaded, as (list, tags, b1, b2)"""
    keys = K.key_set(count, first)
    tag, b1, b2 = K.kv_hash_many(lay.buckets, TK, K.key_array(keys))
    return keys, tag, b1, b2


def crafted_put(lay, model, n_loaded, s, rng):
    """(keys, values) of one put: new keys; existing keys with new values; several new keys that the rule sends into one bucket; and, where the first
    dimension has partner rows j / j ^ 32, keys whose two buckets are such a pair of one column"""
    V = lay.value_bytes
    keys, tag, b1, b2 = fresh_keys(lay, n_loaded + 1000)
    # new keys that the rule sends into one bucket, the emptiest: tried one after the other on a copy of the tags
    target, tags, new = int((model.tags != 0).sum(axis=1).argmin()), model.tags.copy(), []
    for i in np.flatnonzero((b1 == target) | (b2 == target))[:60]:
        trial = tags.copy()
        if [b for _, b, _ in model._walk([keys[i]], trial, skip_full=True)] == [target] and len(new) < min(3, lay.slots):
            tags, new = trial, new + [keys[i]]
    new += list(keys[:5])
    if s.dim0 >= 64:
        pair = np.flatnonzero((b1 ^ b2) == np.uint64(32 * s.num_per))[:3]
        assert len(pair), "the search found keys on partner rows"
        new += [keys[i] for i in pair]
    new = list(dict.fromkeys(new))
    existing = K.key_set(3, 5) + K.key_set(2, n_loaded - 2)
    call = new[:3] + existing[:2] + new[3:] + existing[2:]  # (the call's order is not the image's)
    call = model.fits(call)  # (a table of two slots per bucket may have no room for some of them)
    return call, rng.integers(0, 256, size=(len(call), V), dtype=np.uint8)


CASES = [  # name, (nu1, nu2, parameters), form, option sweep_narrow, value sizes
    ("66-packed", (6, 6, dict(t_gsw=8)), "packed", 0, (248, 3000)),
    ("66-limbs", (6, 6, dict(t_gsw=8)), "limbs", 0, (248, 3000)),
    ("66-w5-limbs", (6, 6, dict(t_gsw=8, p_db=32)), "limbs", 0, (99,)),
    ("64-narrow-limbs", (6, 4, dict(t_gsw=8)), "limbs", 1, (248,)),
    ("43-packed", (4, 3, dict(t_gsw=8)), "packed", 0, (248,)),
    ("32-plain", (3, 2, dict(t_gsw=4)), "packed", 0, (248, 3000)),
    ("32-plain-w5", (3, 2, dict(t_gsw=4, p_db=32)), "packed", 0, (99,)),
]


@pytest.mark.parametrize("name,geom,form,narrow,sizes", CASES, ids=[c[0] for c in CASES])
def test_load_put_delete_get_in_every_form(sa, SV, oracle, opts, name, geom, form, narrow, sizes):
    """kv_load of load_size keys: read_db_items is the restated stream bit for bit and read_db_slots the oracle's encoding of it (every item of an image
    of up to 1024 items, every eighth of a larger one).  Then, in the form under test, a crafted kv_put: the image is the restated one, no bit outside
    the touched tags and values changed, the form stays, limb planes converted back are a fresh load.  kv_delete, then kv_get of present, deleted and
    never-present keys on the owner and on a lane, into buffers prefilled with 0xEE."""
    O = oracle
    opts(sweep_narrow=narrow)
    nu1, nu2, kw = geom
    po, pg = both(sa, O, nu1, nu2, **kw)
    s = O.shape_of(po)
    w = int(po.p_db).bit_length() - 1
    fmt = SV.DB_PACKED if form == "packed" else SV.DB_LIMBS
    for V in sizes:
        what = f"{name} V={V}"
        lay = lay_of(po, V)
        rng = np.random.default_rng(V + nu1)
        n = K.load_size(lay)
        assert (n, lay.buckets, lay.slots) in K.KEY_SETS, "the CPU suite shows that this key set places"
        keys, vals = K.key_set(n), rng.integers(0, 256, size=(n, V), dtype=np.uint8)
        model = K.Table(lay, TK)
        model.load(K.key_array(keys), vals)
        srv = sa.Server(pg)
        srv.gen_db(3)  # (a fresh table overwrites every item)
        srv.kv_load(TK, keys, vals)
        assert_eq(srv.read_db_items(w).reshape(lay.buckets, -1), model.stream(), f"{what}: read_db_items after kv_load")
        check_slots(O, po, srv, model.stream(), range(0, lay.buckets, 1 if lay.buckets <= 1024 else 8), f"{what}: kv_load")
        if form == "limbs":
            assert sa.has_limb_form(pg)
            srv.set_db_format(SV.DB_LIMBS)
        lane = sa.Server(pg, share_db_of=srv)
        # put
        call, new_vals = crafted_put(lay, model, n, s, rng)
        before = model.stream().copy()
        is_new = [model.find(k)[0] == 0 for k in call]
        where = model.put(call, new_vals)
        new_buckets = [b for (b, _), fresh in zip(where, is_new) if fresh]
        assert sum(is_new) >= 5 and len(is_new) - sum(is_new) == 5 and len(set(new_buckets)) < len(new_buckets), "new and existing keys; several new ones into one bucket"
        srv.kv_put(TK, call, new_vals)
        assert srv.db_format() == fmt, "the image keeps its form"
        got = srv.read_db_items(w).reshape(lay.buckets, -1)
        assert_eq(got, model.stream(), f"{what}: read_db_items after kv_put")
        touched = np.zeros(got.shape, dtype=bool)
        for b, sl in where:
            touched[b, 8 * sl:8 * sl + 8] = True
            touched[b, 8 * lay.slots + sl * V:8 * lay.slots + (sl + 1) * V] = True
        assert not (got != before)[~touched].any(), f"{what}: a bit outside the touched tags and values changed"
        check_slots(O, po, srv, model.stream(), sorted({b for b, _ in where}), f"{what}: kv_put")
        # delete: loaded keys, keys of the put, keys that were never there (and one of them twice over two calls)
        gone = K.key_set(4, 10) + call[:4] + K.key_set(3, n + 500_000)
        want_n = model.delete(gone)
        assert want_n == 8
        assert srv.kv_delete(TK, gone, V) == want_n and srv.kv_delete(TK, gone[:2], V) == 0
        assert_eq(srv.read_db_items(w).reshape(lay.buckets, -1), model.stream(), f"{what}: read_db_items after kv_delete")
        assert srv.db_format() == fmt
        # get
        in2 = list(islice((k for k in keys[14:] if model.find(k)[0] == 2), 2))  # (loaded keys that sit in their second candidate)
        probe = K.key_set(6, 8) + call + in2 + K.key_set(4, n + 500_000 - 1) + K.key_set(2, n - 2) + K.key_set(2, 8)
        want_v, want_f = model.get(probe, fill=0xEE)
        assert {0, 1, 2} <= set(want_f.tolist()), "present in candidate 1, in candidate 2, and absent"
        for who, sv in (("owner", srv), ("lane", lane)):
            out = np.full((len(probe), V), 0xEE, dtype=np.uint8)
            got_v, got_f = sv.kv_get(TK, probe, V, out=out)
            assert_eq(got_f, want_f, f"{what}: kv_get found, {who}")
            assert_eq(got_v, want_v, f"{what}: kv_get values, {who}")
        if form == "limbs":
            srv.set_db_format(SV.DB_PACKED)
            fresh = sa.Server(pg)
            fresh.load_db_items(model.stream(), w)
            assert_eq(srv.read_db_slots(0, N), fresh.read_db_slots(0, N), f"{what}: converted back == a fresh load of the restated stream")
            fresh.close()
        lane.close()
        srv.close()


def test_failure_is_atomic(sa, SV, oracle):
    """a put that cannot place a key names it and leaves the image byte-identical; two equal tags are refused by position; a probe of a random image
    names the bucket; a lane, a j-shard and a column shard refuse a put by name"""
    O = oracle
    po, pg = both(sa, O, 3, 2, t_gsw=4)
    V = 3000
    lay = lay_of(po, V)
    assert lay.slots == 2
    srv = sa.Server(pg)
    srv.kv_load(TK, [], np.zeros((0, V), dtype=np.uint8))
    assert not srv.read_db_items(8).any(), "an empty table is an image of zero plaintexts"
    keys, tag, b1, b2 = fresh_keys(lay, 0, 20_000)
    same = np.flatnonzero((b1 == b1[0]) & (b2 == b2[0]))[:5]  # five keys with one pair of buckets of two slots each
    assert len(same) == 5
    pair = (b1[0], b2[0])
    other = [keys[i] for i in np.flatnonzero(~np.isin(b1, pair) & ~np.isin(b2, pair))[:3]]  # three keys that touch neither bucket of the pair
    call = [other[0], keys[same[0]], keys[same[1]], keys[same[2]], other[1], keys[same[3]], keys[same[4]], other[2]]
    vals = np.random.default_rng(1).integers(0, 256, size=(len(call), V), dtype=np.uint8)
    model = K.Table(lay, TK)
    srv.kv_put(TK, call[:2], vals[:2])
    model.put(call[:2], vals[:2])
    with pytest.raises(K.Full) as e:
        model.put(call[2:], vals[2:])  # five keys for the four slots of one pair of buckets: the restated rule refuses the last of them
    assert call[2:][e.value.position] == keys[same[4]]
    before = digest(srv.read_db_slots(0, N))
    with pytest.raises(sa.SpiralGpuError, match=rf"key {e.value.position} cannot be placed: its buckets {int(b1[0])} and {int(b2[0])} are both full"):
        srv.kv_put(TK, call[2:], vals[2:])  # (positions count within the call)
    with pytest.raises(sa.SpiralGpuError, match=r"keys 1 and 3 have equal tags"):
        srv.kv_put(TK, [call[0], call[4], call[7], call[4]], vals[:4])
    lane = sa.Server(pg, share_db_of=srv)
    with pytest.raises(sa.SpiralGpuError, match="owner"):
        lane.kv_put(TK, call[:1], vals[:1])
    with pytest.raises(sa.SpiralGpuError, match="owner"):
        lane.kv_delete(TK, call[:1], V)
    assert digest(srv.read_db_slots(0, N)) == before, "the image is byte-identical after every failed call"
    assert_eq(srv.read_db_items(8).reshape(lay.buckets, -1), model.stream(), "the table before the failed calls")
    srv.fill_db_random(5)
    before = digest(srv.read_db_slots(0, N))
    probe = other
    first = min(b for k in probe for b in model.hash(k)[1:])
    for call_ in (lambda: srv.kv_get(TK, probe, V), lambda: lane.kv_get(TK, probe, V), lambda: srv.kv_put(TK, probe, vals[:3]), lambda: srv.kv_delete(TK, probe, V)):
        with pytest.raises(sa.SpiralGpuError, match=rf"no keyed table at bucket {first} \(polynomial 0, coefficient \d+"):
            call_()
    assert digest(srv.read_db_slots(0, N)) == before, "a random image is byte-identical after the failed calls"
    lane.close()
    srv.close()
    for tag_, geom, make in [("j-shard", (7, 6), lambda p: sa.Server(p, j_begin=0, j_end=64)), ("column shard", (5, 5), lambda p: sa.Server(p, col_rank=0, col_ranks=2))]:
        _, p2 = both(sa, O, *geom, t_gsw=8)
        shard = make(p2)
        shard.gen_db(1)
        for call_ in (lambda: shard.kv_put(TK, probe, np.zeros((3, 248), dtype=np.uint8)), lambda: shard.kv_get(TK, probe, 248),
                      lambda: shard.kv_load(TK, probe, np.zeros((3, 248), dtype=np.uint8))):
            with pytest.raises(sa.SpiralGpuError, match=tag_):
                call_()
        shard.close()


@pytest.mark.parametrize("form", ["packed", "limbs"])
def test_tracked_fingerprints_follow_put_and_delete(sa, SV, oracle, form):
    """after fingerprint_track, a kv_put and a kv_delete keep fingerprint_tracked() equal to fingerprint_host of the restated stream"""
    O = oracle
    po, pg = both(sa, O, 6, 6, t_gsw=8)
    s = O.shape_of(po)
    V = 248
    lay = lay_of(po, V)
    rng = np.random.default_rng(17)
    n = K.load_size(lay)
    keys, vals = K.key_set(n), rng.integers(0, 256, size=(n, V), dtype=np.uint8)
    model = K.Table(lay, TK)
    model.load(K.key_array(keys), vals)
    srv = sa.Server(pg)
    srv.kv_load(TK, keys, vals)
    if form == "limbs":
        srv.set_db_format(SV.DB_LIMBS)
    srv.fingerprint_track(FP_KEY)
    host = lambda: sa.fingerprint_host(FP_KEY, int(po.p_db), model.stream().reshape(-1), 8)
    assert srv.fingerprint_tracked()[0] == host()
    call, new_vals = crafted_put(lay, model, n, s, rng)
    model.put(call, new_vals)
    srv.kv_put(TK, call, new_vals)
    F, n_upd = srv.fingerprint_tracked()
    assert F == host() and n_upd > 0, "kv_put keeps the tracked fingerprint current"
    gone = call[:3] + K.key_set(3, 100)
    assert srv.kv_delete(TK, gone, V) == model.delete(gone) == 6
    assert srv.fingerprint_tracked()[0] == host(), "kv_delete keeps the tracked fingerprint current"
    assert srv.fingerprint_scrub()[0] == 0, "the table of polynomial sums is the image's"
    srv.close()


E2E = [("32-V248", (3, 2, dict(t_gsw=4)), "packed", 248), ("32-V3000", (3, 2, dict(t_gsw=4)), "packed", 3000), ("32-w5-V99", (3, 2, dict(t_gsw=4, p_db=32)), "packed", 99),
       ("66-limbs-V248", (6, 6, dict(t_gsw=8)), "limbs", 248)]


@pytest.mark.parametrize("name,geom,form,V", E2E, ids=[c[0] for c in E2E])
def test_end_to_end(sa, SV, oracle, name, geom, form, V):
    """a Client's kv_queries for keys present in candidate 1, present in candidate 2 and absent; the server answers them, per query and once as the lanes
    of a run_query_batch; kv_decode on RAW and on WIRE responses gives the restatement's values and found, and bit for bit what decode of the same
    responses followed by the restated header scan and value cut gives.  V = 3000: the two slots' values straddle polynomials 0-1 and 1-2.  Then a tag
    planted in BOTH buckets of a key: candidate 1 wins, on the server and on the client."""
    O = oracle
    nu1, nu2, kw = geom
    po, pg = both(sa, O, nu1, nu2, **kw)
    w = int(po.p_db).bit_length() - 1
    lay = lay_of(po, V)
    rng = np.random.default_rng(V)
    n = K.load_size(lay)
    keys, vals = K.key_set(n), rng.integers(0, 256, size=(n, V), dtype=np.uint8)
    model = K.Table(lay, TK)
    model.load(K.key_array(keys), vals)
    srv = sa.Server(pg)
    srv.kv_load(TK, keys, vals)
    if form == "limbs":
        srv.set_db_format(SV.DB_LIMBS)
    cl = sa.Client(pg, bytes(range(50, 82)))
    srv.set_pub_params(*cl.pub_params())
    in1 = [k for k in keys[:400] if model.find(k)[0] == 1][:2]
    in2 = list(islice((k for k in keys if model.find(k)[0] == 2), 2))
    ask = [in2[0], in1[0], K.key_set(1, n + 7)[0], in1[1], in2[1], K.key_set(1, n + 8)[0]]
    want_v, want_f = model.get(ask)
    assert want_f.tolist() == [2, 1, 0, 1, 2, 0]
    tags = [model.hash(k)[0] for k in ask]

    def check(resp, what):
        """resp [2 n][3][2][N] switched responses: kv_decode in both forms against the model and against decode + the restated scan"""
        plain = cl.decode(resp)
        scan = [K.find_in(lay, plain[2 * k], plain[2 * k + 1], tags[k]) for k in range(len(resp) // 2)]
        for f, buf in (("raw", resp), ("wire", np.concatenate([O.response_to_wire(po, r) for r in resp]))):
            got_v, got_f = cl.kv_decode(TK, ask[:len(scan)], buf, V, f)
            assert_eq(got_f, [c for _, c in scan], f"{name} {what} {f}: found against decode + scan")
            assert_eq(got_v, np.stack([v for v, _ in scan]), f"{name} {what} {f}: values against decode + scan")
            assert_eq(got_f, want_f[:len(scan)], f"{name} {what} {f}: found")
            assert_eq(got_v, want_v[:len(scan)], f"{name} {what} {f}: values")

    qs = cl.kv_queries(TK, ask, "ntt")
    assert len(qs) == 2 * len(ask), "both candidates are always asked for"
    check(np.stack([srv.answer(q)[1] for q in qs]), "answer")
    # the first four keys' eight queries as the lanes of one batch, the same public parameters on every lane
    lanes = [srv] + [sa.Server(pg, share_db_of=srv) for _ in range(7)]
    pp = cl.pub_params("seeded")
    for ln in lanes:
        ln.set_pub_params_seeded(pp)
    sa.set_query_batch(lanes, list(cl.kv_queries(TK, ask[:4], "seeded")), form="seeded")
    sa.run_query_batch(lanes)
    wires = sa.read_response_wire_batch(lanes)
    got_v, got_f = cl.kv_decode(TK, ask[:4], wires, V, "wire")
    assert_eq(got_f, want_f[:4], f"{name} batch: found")
    assert_eq(got_v, want_v[:4], f"{name} batch: values")
    check(np.stack([O.response_from_wire(po, x) for x in wires]), "batch")
    for ln in lanes[1:]:
        ln.close()
    # one tag in both buckets (what two keys with equal tags would leave): candidate 1 wins
    twin = next(k for k in K.key_set(200, n + 9) if all((model.tags[b] == 0).any() for b in model.hash(k)[1:]))  # absent, with room in both buckets
    tag, b1, b2 = model.hash(twin)
    stream = model.stream()
    s1, s2 = int(np.flatnonzero(model.tags[b1] == 0)[-1]), int(np.flatnonzero(model.tags[b2] == 0)[0])
    x1, x2 = rng.integers(0, 256, size=(2, V), dtype=np.uint8)
    for b, sl, x in ((b1, s1, x1), (b2, s2, x2)):
        stream[b, 8 * sl:8 * sl + 8] = np.frombuffer(int(tag).to_bytes(8, "little"), dtype=np.uint8)
        stream[b, 8 * lay.slots + sl * V:8 * lay.slots + (sl + 1) * V] = x
    srv.load_db_items(stream, w)
    got_v, got_f = srv.kv_get(TK, [twin], V)
    assert got_f.tolist() == [1] and (got_v[0] == x1).all(), "kv_get: candidate 1 wins"
    resp = np.stack([srv.answer(q)[1] for q in cl.kv_queries(TK, [twin], "ntt")])
    got_v, got_f = cl.kv_decode(TK, [twin], resp, V, "raw")
    assert got_f.tolist() == [1] and (got_v[0] == x1).all(), "kv_decode: candidate 1 wins"
    cl.close()
    srv.close()
