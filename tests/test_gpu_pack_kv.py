"""Keyed records on SpiralPack servers and table occupancy on the device (include/spiral_gpu.h "Keyed records", SpiralPack: PackServer.kv_load,
kv_put, kv_delete, kv_get; Client(out_n).kv_queries / kv_decode; Server.kv_stats and PackServer.kv_stats).  Expected tables, streams, values, `found`
and histograms come from the restatement (tests/kv_restated.py, tests/pack_kv_restated.py) and from calls the oracle already checks (read_db_items,
decode); nothing expected comes from the code under test.  tests/test_pack_kv_cpu.py shows that the restated placement places every key of every key
set used here."""
import ctypes as C
import hashlib
import sys
from itertools import islice

import numpy as np
import pytest

import kv_restated as K
import pack_kv_restated as PK

pytestmark = pytest.mark.gpu
N = 2048
TK = PK.TABLE_KEY
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
def P(sa):
    return sys.modules["spiral_amd.pack"]


@pytest.fixture(scope="module")
def SV(sa):
    from spiral_amd import server

    return server


def assert_eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp) if got.shape == exp.shape else []
        raise AssertionError(f"{what}: shapes {got.shape} / {exp.shape}, {len(bad)} of {got.size} differ, first at {bad[:5].tolist() if len(bad) else '-'}")


def digest(arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def both(sa, O, nu1, nu2, **kw):
    return O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)


def lay_of(po, out_n, V):
    return PK.layout(int(po.p_db), int(po.nu1), int(po.nu2), out_n, V)


def loaded_model(lay, seed):
    """(keys, values, model) of a table loaded by the load rule, and the generator that drew the values"""
    rng = np.random.default_rng(seed)
    n = PK.load_size(lay)
    assert (n, lay.buckets, lay.slots) in PK.PACK_KEY_SETS + K.KEY_SETS, "the CPU suite shows that this key set places"
    keys, vals = K.key_set(n), rng.integers(0, 256, size=(n, lay.value_bytes), dtype=np.uint8)
    model = K.Table(lay, TK)
    model.load(K.key_array(keys), vals)
    return keys, vals, model, rng


def image_stream(srv, lay, trials, bits=None):
    """every trial's read_db_items side by side: [buckets][item_bytes] at the layout's width, the table's stream as the image holds it"""
    return np.concatenate([srv.read_db_items(t, bits or lay.coeff_bits).reshape(lay.buckets, -1) for t in range(trials)], axis=1)


def check_trials(srv, lay, out_n, stream, what):
    want = PK.trial_streams(stream, lay, out_n)
    for t in range(out_n * out_n):
        assert_eq(srv.read_db_items(t, lay.coeff_bits).reshape(lay.buckets, -1), want[t], f"{what}: read_db_items of trial {t}")


def fresh_keys(lay, first, count=120_000):
    """keys never loaded, as (list, tags, b1, b2)"""
    keys = K.key_set(count, first)
    tag, b1, b2 = K.kv_hash_many(lay.buckets, TK, K.key_array(keys))
    return keys, tag, b1, b2


def crafted_put(lay, model, n_loaded, num_per, dim0, rng):
    """(keys, values) of one put: new keys; existing keys with new values; several new keys that the rule sends into one bucket; and, where the first
    dimension has partner rows j / j + 64, keys whose two buckets are such a pair of one column"""
    V = lay.value_bytes
    keys, tag, b1, b2 = fresh_keys(lay, n_loaded + 1000)
    target, tags, new = int((model.tags != 0).sum(axis=1).argmin()), model.tags.copy(), []
    for i in np.flatnonzero((b1 == target) | (b2 == target))[:60]:
        trial = tags.copy()
        if [b for _, b, _ in model._walk([keys[i]], trial, skip_full=True)] == [target] and len(new) < min(3, lay.slots):
            tags, new = trial, new + [keys[i]]
    new += list(keys[:5])
    if dim0 >= 128:
        pair = np.flatnonzero((b1 ^ b2) == np.uint64(64 * num_per))[:3]
        assert len(pair), "the search found keys on partner rows"
        new += [keys[i] for i in pair]
    new = list(dict.fromkeys(new))
    existing = K.key_set(3, 5) + K.key_set(2, n_loaded - 2)
    call = new[:3] + existing[:2] + new[3:] + existing[2:]  # (the call's order is not the image's)
    call = model.fits(call)  # (a table of few slots per bucket may have no room for some of them)
    return call, rng.integers(0, 256, size=(len(call), V), dtype=np.uint8)


def plan_calls(lay, num_per, dim0, seed):
    """the model's side of one case, no device involved: the loaded table, the crafted put, the delete and the get, with what each should leave"""
    keys, vals, model, rng = loaded_model(lay, seed)
    n, V = len(keys), lay.value_bytes
    plan = dict(keys=keys, vals=vals, model=model, loaded=model.stream().copy())
    call, new_vals = crafted_put(lay, model, n, num_per, dim0, rng)
    is_new = [model.find(k)[0] == 0 for k in call]
    where = model.put(call, new_vals)
    new_buckets = [b for (b, _), fresh in zip(where, is_new) if fresh]
    assert sum(is_new) >= 5 and len(is_new) - sum(is_new) == 5 and len(set(new_buckets)) < len(new_buckets), "new and existing keys; several new ones into one bucket"
    touched = np.zeros(plan["loaded"].shape, dtype=bool)
    for b, sl in where:
        touched[b, 8 * sl:8 * sl + 8] = True
        touched[b, 8 * lay.slots + sl * V:8 * lay.slots + (sl + 1) * V] = True
    plan.update(call=call, new_vals=new_vals, touched=touched, after_put=model.stream().copy(), tags_after_put=model.tags.copy())
    gone = K.key_set(4, 10) + call[:4] + K.key_set(3, n + 500_000)
    assert model.delete(gone) == 8
    plan.update(gone=gone, after_delete=model.stream().copy())
    in2 = list(islice((k for k in keys[14:] if model.find(k)[0] == 2), 2))  # (loaded keys that sit in their second candidate)
    probe = K.key_set(6, 8) + call + in2 + K.key_set(4, n + 500_000 - 1) + K.key_set(2, n - 2) + K.key_set(2, 8)
    want_v, want_f = model.get(probe, fill=0xEE)
    assert {0, 1, 2} <= set(want_f.tolist()), "present in candidate 1, in candidate 2, and absent"
    plan.update(probe=probe, want_v=want_v, want_f=want_f)
    return plan


CASES = [  # name, (nu1, nu2, out_n, parameters), form, option pack_pair_blocks, value sizes
    ("422-packed", (4, 2, 2, {}), "packed", 0, (248, 3000)),
    ("742-limbs", (7, 4, 2, {}), "limbs", 0, (248,)),
    ("733-packed", (7, 3, 3, {}), "packed", 0, (3000,)),
    ("733-pairs", (7, 3, 3, {}), "limbs", 1, (248, 5000)),
    ("422-w5", (4, 2, 2, dict(p_db=32)), "packed", 0, (99,)),
]


@pytest.mark.parametrize("name,geom,form,pairs,sizes", CASES, ids=[c[0] for c in CASES])
def test_load_put_delete_get_in_every_form(sa, P, oracle, opts, name, geom, form, pairs, sizes):
    """kv_load: every trial's read_db_items is the restated stream.  Then, in the form under test, a crafted kv_put: every trial equals the model, no
    bit outside the touched tags and values changed, the form stays.  kv_delete, then kv_get of keys present in candidate 1, in candidate 2, deleted
    and never present, on the owner and on a lane, into buffers prefilled with 0xEE.  Limb planes converted back are a fresh load of the model.  At
    V = 5000 a bucket has 3 slots whose values span polynomials 0-2, 2-4 and 4-7."""
    O = oracle
    opts(pack_pair_blocks=pairs)
    nu1, nu2, out_n, kw = geom
    po, pg = both(sa, O, nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    trials = s.trials
    fmt = P.DB_PACKED if form == "packed" else P.DB_LIMBS
    for V in sizes:
        what = f"{name} V={V}"
        lay = lay_of(po, out_n, V)
        w = lay.coeff_bits
        pl = plan_calls(lay, s.num_per, s.dim0, V + nu1)
        srv = sa.PackServer(pg, out_n)
        srv.gen_db(3)  # (a fresh table overwrites every item of every trial)
        srv.kv_load(TK, pl["keys"], pl["vals"])
        check_trials(srv, lay, out_n, pl["loaded"], f"{what}: kv_load")
        if form == "limbs":
            assert P.has_limb_form(pg, out_n)
            srv.set_db_format(P.DB_LIMBS)
        lane = srv.create_lane()
        srv.kv_put(TK, pl["call"], pl["new_vals"])
        assert srv.db_format() == fmt, "the image keeps its form"
        got = image_stream(srv, lay, trials)
        assert_eq(got, pl["after_put"], f"{what}: every trial after kv_put")
        assert not (got != pl["loaded"])[~pl["touched"]].any(), f"{what}: a bit outside the touched tags and values changed"
        assert srv.kv_delete(TK, pl["gone"], V) == 8 and srv.kv_delete(TK, pl["gone"][:2], V) == 0
        check_trials(srv, lay, out_n, pl["after_delete"], f"{what}: kv_delete")
        assert srv.db_format() == fmt
        for who, sv in (("owner", srv), ("lane", lane)):
            out = np.full((len(pl["probe"]), V), 0xEE, dtype=np.uint8)
            got_v, got_f = sv.kv_get(TK, pl["probe"], V, out=out)
            assert_eq(got_f, pl["want_f"], f"{what}: kv_get found, {who}")
            assert_eq(got_v, pl["want_v"], f"{what}: kv_get values, {who}")
        if form == "limbs":
            srv.set_db_format(P.DB_PACKED)
            fresh = sa.PackServer(pg, out_n)
            for t, st in enumerate(PK.trial_streams(pl["after_delete"], lay, out_n)):
                fresh.load_db_items(t, st, w)
            for t in range(trials):
                assert_eq(srv.read_db_items(t, 64), fresh.read_db_items(t, 64), f"{what}: trial {t} converted back == a fresh load of the restated stream")
            fresh.close()
        lane.close()
        srv.close()


def test_failure_is_atomic(sa, P, oracle):
    """a put that cannot place a key names it and leaves every trial byte-identical; two equal tags are refused by position; after fill_db_random
    every keyed call and kv_stats name the bucket; a lane refuses put and delete; a trial-sharded server and a shard lane refuse every keyed call by
    name"""
    O = oracle
    out_n, V = 2, 3000
    po, pg = both(sa, O, 4, 2)
    s = O.pack_shape_of(po, out_n)
    lay = lay_of(po, out_n, V)
    assert lay.slots == 2
    srv = sa.PackServer(pg, out_n)
    srv.kv_load(TK, [], np.zeros((0, V), dtype=np.uint8))
    assert not image_stream(srv, lay, s.trials).any(), "an empty table is an image of zero plaintexts"
    keys, tag, b1, b2 = fresh_keys(lay, 0, 60_000)
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
    images = lambda: digest(srv.read_db_items(t, 64) for t in range(s.trials))
    before = images()
    with pytest.raises(sa.SpiralGpuError, match=rf"key {e.value.position} cannot be placed: its buckets {int(b1[0])} and {int(b2[0])} are both full \(2 slots each\); nothing was written"):
        srv.kv_put(TK, call[2:], vals[2:])  # (positions count within the call; the base server's message)
    with pytest.raises(sa.SpiralGpuError, match=r"keys 1 and 3 have equal tags"):
        srv.kv_put(TK, [call[0], call[4], call[7], call[4]], vals[:4])
    lane = srv.create_lane()
    with pytest.raises(sa.SpiralGpuError, match="owner"):
        lane.kv_put(TK, call[:1], vals[:1])
    with pytest.raises(sa.SpiralGpuError, match="owner"):
        lane.kv_delete(TK, call[:1], V)
    with pytest.raises(sa.SpiralGpuError, match="owner"):
        lane.kv_load(TK, call[:1], vals[:1])
    assert images() == before, "every trial is byte-identical after every failed call"
    assert_eq(image_stream(srv, lay, s.trials), model.stream(), "the table before the failed calls")
    srv.fill_db_random(5)  # (no plaintexts: read_db_items has nothing to return, so the image is compared through the answer to one fixed query)
    cl = sa.Client(pg, bytes([41] * 32), out_n=out_n)
    srv.set_pub_params_seeded(cl.pub_params("seeded"))
    q = cl.query(6, "seeded")
    cl.close()
    images = lambda: digest([srv.answer_seeded(q, want_packed=False)[0]])
    before = images()
    probe = other
    first = min(b for k in probe for b in model.hash(k)[1:])
    for call_ in (lambda: srv.kv_get(TK, probe, V), lambda: lane.kv_get(TK, probe, V), lambda: srv.kv_put(TK, probe, vals[:3]), lambda: srv.kv_delete(TK, probe, V)):
        with pytest.raises(sa.SpiralGpuError, match=rf"no keyed table at bucket {first} \(polynomial 0, coefficient \d+"):
            call_()
    for who, first_bucket in ((srv, 0), (lane, 5)):
        with pytest.raises(sa.SpiralGpuError, match=rf"kv_stats: the image holds no keyed table at bucket {first_bucket} \(polynomial 0, coefficient \d+"):
            who.kv_stats(V, first_bucket)
    assert images() == before, "a random image is byte-identical after the failed calls"
    lane.close()
    srv.close()
    shard = sa.PackServer(pg, out_n, trial0=0, trial1=2)
    shard.gen_db(1)
    shard_lane = shard.create_shard_lane()
    zeros = np.zeros((3, 248), dtype=np.uint8)
    # the shard itself: every keyed call names the trial shard; its lane: the reads name the trial shard, the writes the lane (refused first, as on any lane)
    for call_ in (lambda: shard.kv_put(TK, probe, zeros), lambda: shard.kv_get(TK, probe, 248), lambda: shard.kv_load(TK, probe, zeros), lambda: shard.kv_delete(TK, probe, 248),
                  lambda: shard.kv_stats(248), lambda: shard_lane.kv_get(TK, probe, 248), lambda: shard_lane.kv_stats(248)):
        with pytest.raises(sa.SpiralGpuError, match=r"this server is a trial shard \(trials \[0, 2\) of 4\)"):
            call_()
    for call_ in (lambda: shard_lane.kv_put(TK, probe, zeros), lambda: shard_lane.kv_load(TK, probe, zeros), lambda: shard_lane.kv_delete(TK, probe, 248)):
        with pytest.raises(sa.SpiralGpuError, match="this server is a lane"):
            call_()
    shard_lane.close()
    shard.close()


@pytest.mark.parametrize("form", ["packed", "limbs"])
def test_tracked_fingerprints_follow_put_and_delete(sa, P, oracle, form):
    """after fingerprint_track, a kv_put and a kv_delete keep fingerprint_tracked() equal to fingerprint_host of the restated stream, and
    fingerprint_scrub finds nothing"""
    O = oracle
    out_n, V = 2, 248
    po, pg = both(sa, O, 7, 4)
    s = O.pack_shape_of(po, out_n)
    lay = lay_of(po, out_n, V)
    keys, vals, model, rng = loaded_model(lay, 17)
    srv = sa.PackServer(pg, out_n)
    srv.kv_load(TK, keys, vals)
    if form == "limbs":
        srv.set_db_format(P.DB_LIMBS)
    srv.fingerprint_track(FP_KEY)
    host = lambda: sa.fingerprint_host(FP_KEY, int(po.p_db), model.stream().reshape(-1), 8, polys_per_item=s.trials)
    assert srv.fingerprint_tracked()[0] == host()
    call, new_vals = crafted_put(lay, model, len(keys), s.num_per, s.dim0, rng)
    model.put(call, new_vals)
    srv.kv_put(TK, call, new_vals)
    F, n_upd = srv.fingerprint_tracked()
    assert F == host() and n_upd > 0, "kv_put keeps the tracked fingerprint current"
    gone = call[:3] + K.key_set(3, 100)
    assert srv.kv_delete(TK, gone, V) == model.delete(gone) == 6
    assert srv.fingerprint_tracked()[0] == host(), "kv_delete keeps the tracked fingerprint current"
    assert srv.fingerprint_scrub()[0] == 0, "the table of polynomial sums is the image's"
    srv.close()


E2E = [("422-V248", (4, 2, 2), 0, 248), ("422-V3000", (4, 2, 2), 0, 3000), ("733-pairs-V5000", (7, 3, 3), 1, 5000)]


def pick_asked(keys, model, n):
    """six keys: present in candidate 2, in candidate 1, absent, ..."""
    in1 = [k for k in keys[:400] if model.find(k)[0] == 1][:2]
    in2 = list(islice((k for k in keys if model.find(k)[0] == 2), 2))
    ask = [in2[0], in1[0], K.key_set(1, n + 7)[0], in1[1], in2[1], K.key_set(1, n + 8)[0]]
    want_v, want_f = model.get(ask)
    assert want_f.tolist() == [2, 1, 0, 1, 2, 0]
    return ask, want_v, want_f


@pytest.mark.parametrize("name,geom,pairs,V", E2E, ids=[c[0] for c in E2E])
def test_end_to_end(sa, P, oracle, opts, name, geom, pairs, V):
    """a Client(out_n)'s kv_queries for keys present in candidate 1, present in candidate 2 and absent; the server answers them one by one, and once as
    an answer_batch; kv_decode on RAW and on WIRE responses gives the restatement's values and found, and bit for bit what decode of the same
    responses followed by the restated header scan and value cut gives.  Then a tag planted in BOTH buckets of a key: candidate 1 wins, on the server
    and on the client."""
    O = oracle
    opts(pack_pair_blocks=pairs)
    nu1, nu2, out_n = geom
    po, pg = both(sa, O, nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    lay = lay_of(po, out_n, V)
    w = lay.coeff_bits
    keys, vals, model, rng = loaded_model(lay, V)
    n = len(keys)
    srv = sa.PackServer(pg, out_n)
    srv.kv_load(TK, keys, vals)
    if pairs:
        srv.set_db_format(P.DB_LIMBS)
    cl = sa.Client(pg, bytes(range(50, 82)), out_n=out_n)
    pp = cl.pub_params("seeded")
    srv.set_pub_params_seeded(pp)
    ask, want_v, want_f = pick_asked(keys, model, n)
    tags = [model.hash(k)[0] for k in ask]

    def check(resp, wire, what):
        """resp [2 m][out_n + 1][out_n][N] switched responses and their wire forms: kv_decode in both forms against the model and against decode + scan"""
        plain = cl.decode(resp)
        scan = [PK.find_in(lay, plain[2 * k], plain[2 * k + 1], tags[k]) for k in range(len(resp) // 2)]
        for f, buf in (("raw", resp), ("wire", wire)):
            got_v, got_f = cl.kv_decode(TK, ask[:len(scan)], buf, V, f)
            assert_eq(got_f, [c for _, c in scan], f"{name} {what} {f}: found against decode + scan")
            assert_eq(got_v, np.stack([v for v, _ in scan]), f"{name} {what} {f}: values against decode + scan")
            assert_eq(got_f, want_f[:len(scan)], f"{name} {what} {f}: found")
            assert_eq(got_v, want_v[:len(scan)], f"{name} {what} {f}: values")

    qs = cl.kv_queries(TK, ask, "seeded")
    assert len(qs) == 2 * len(ask), "both candidates are always asked for"
    resp, wire = [], []
    for q in qs:
        resp.append(srv.answer_seeded(q, want_packed=False)[0].copy())
        wire.append(srv.read_response_wire().copy())
    check(np.stack(resp), np.concatenate(wire), "answer")
    # the first four keys' eight queries as one answer_batch, the same public parameters on every lane
    lanes = [srv] + [srv.create_lane() for _ in range(7)]
    for ln in lanes[1:]:
        ln.set_pub_params_seeded(pp)
    out, _ = P.answer_batch_seeded(lanes, list(cl.kv_queries(TK, ask[:4], "seeded")))
    check(np.stack([out[b][0] for b in range(8)]), np.concatenate([ln.read_response_wire() for ln in lanes]), "batch")
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
    for t, st in enumerate(PK.trial_streams(stream, lay, out_n)):
        srv.load_db_items(t, st, w)
    got_v, got_f = srv.kv_get(TK, [twin], V)
    assert got_f.tolist() == [1] and (got_v[0] == x1).all(), "kv_get: candidate 1 wins"
    resp = np.stack([srv.answer_seeded(q, want_packed=False)[0].copy() for q in cl.kv_queries(TK, [twin], "seeded")])
    got_v, got_f = cl.kv_decode(TK, [twin], resp, V, "raw")
    assert got_f.tolist() == [1] and (got_v[0] == x1).all(), "kv_decode: candidate 1 wins"
    cl.close()
    srv.close()


STATS = [  # name, kind, (nu1, nu2, out_n), form, option pack_pair_blocks, value sizes
    ("base-32", "base", (3, 2, 0), "packed", 0, (3000, 248)),
    ("base-66-limbs", "base", (6, 6, 0), "limbs", 0, (248,)),
    ("pack-422", "pack", (4, 2, 2), "packed", 0, (3000, 248)),
    ("pack-733-pairs", "pack", (7, 3, 3), "limbs", 1, (5000,)),
]


def check_stats(got, tags, first, n, what):
    buckets, used, full, max_used, hist = PK.stats_of(tags, first, n)
    assert (got.buckets, got.used, got.full_buckets, got.max_used, got.slots) == (buckets, used, full, max_used, tags.shape[1]), what
    assert list(got.hist) == hist, f"{what}: histogram"
    assert sum(got.hist) == buckets and not any(got.hist[tags.shape[1] + 1:]), f"{what}: entries above `slots` are 0"
    assert got.load() == (used / (buckets * tags.shape[1]) if buckets else 0.0)


@pytest.mark.parametrize("name,kind,geom,form,pairs,sizes", STATS, ids=[c[0] for c in STATS])
def test_kv_stats(sa, P, SV, oracle, opts, name, kind, geom, form, pairs, sizes):
    """after load, after put and after delete the histogram, used, full_buckets and max_used equal the model's counts; the 2-slot tables have full
    buckets; a sub-range, a range of one bucket and n_buckets = 0 are correct; a range past nb is refused; a lane gets the same answer"""
    O = oracle
    opts(pack_pair_blocks=pairs)
    nu1, nu2, out_n = geom
    kw = dict(t_gsw=4) if (nu1, nu2) == (3, 2) else dict(t_gsw=8) if kind == "base" else {}
    po, pg = both(sa, O, nu1, nu2, **kw)
    for V in sizes:
        what = f"{name} V={V}"
        if kind == "base":
            lay = K.layout(int(po.p_db), nu1, nu2, V)
            s = O.shape_of(po)
            srv = sa.Server(pg)
        else:
            lay = lay_of(po, out_n, V)
            s = O.pack_shape_of(po, out_n)
            srv = sa.PackServer(pg, out_n)
        keys, vals, model, rng = loaded_model(lay, V + 1) if kind == "pack" else base_model(lay, V + 1)
        nb = lay.buckets
        srv.kv_load(TK, keys, vals)
        if form == "limbs":
            srv.set_db_format((SV if kind == "base" else P).DB_LIMBS)
        lane = sa.Server(pg, share_db_of=srv) if kind == "base" else srv.create_lane()
        check_stats(srv.kv_stats(V), model.tags, 0, nb, f"{what}: after kv_load")
        if lay.slots == 2:
            assert srv.kv_stats(V).full_buckets > 0, "a 2-slot table at this load has full buckets"
        call, new_vals = crafted_put(lay, model, len(keys), s.num_per, s.dim0, rng)
        model.put(call, new_vals)
        srv.kv_put(TK, call, new_vals)
        check_stats(srv.kv_stats(V), model.tags, 0, nb, f"{what}: after kv_put")
        gone = call[:3] + K.key_set(3, 3)
        assert srv.kv_delete(TK, gone, V) == model.delete(gone) == 6
        for who, sv in (("owner", srv), ("lane", lane)):
            check_stats(sv.kv_stats(V), model.tags, 0, nb, f"{what}: after kv_delete, {who}")
            check_stats(sv.kv_stats(V, 3, nb // 2 + 1), model.tags, 3, nb // 2 + 1, f"{what}: a sub-range, {who}")
            check_stats(sv.kv_stats(V, nb - 5), model.tags, nb - 5, 5, f"{what}: to the table's end, {who}")
            busiest = int((model.tags != 0).sum(axis=1).argmax())
            check_stats(sv.kv_stats(V, busiest, 1), model.tags, busiest, 1, f"{what}: one bucket, {who}")
            check_stats(sv.kv_stats(V, nb, 0), model.tags, nb, 0, f"{what}: n_buckets = 0, {who}")
            for first, cnt in ((nb, 1), (0, nb + 1), (nb + 1, 0), (1, nb)):
                with pytest.raises(sa.SpiralGpuError, match="outside the table"):
                    sv.kv_stats(V, first, cnt)
        lane.close()
        srv.close()


def hip_runtime():
    """the HIP runtime this process already has loaded (torch's, which the library shares)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def test_kv_stats_refusals(sa, oracle):
    """kv_stats is refused by name on a base j-shard and a column shard, and inside a stream capture on both kinds of server; a refused call writes
    nothing"""
    O = oracle
    for tag_, geom, make in [("j-shard", (7, 6), lambda p: sa.Server(p, j_begin=0, j_end=64)), ("column shard", (5, 5), lambda p: sa.Server(p, col_rank=0, col_ranks=2))]:
        _, p2 = both(sa, O, *geom, t_gsw=8)
        shard = make(p2)
        shard.gen_db(1)
        with pytest.raises(sa.SpiralGpuError, match=f"kv_stats: this server is a {tag_}"):
            shard.kv_stats(248)
        shard.close()
    from spiral_amd import _lib

    L, hip = sa.lib(), hip_runtime()
    _, pb = both(sa, O, 3, 2, t_gsw=4)
    _, pp = both(sa, O, 4, 2)
    for srv, fn in ((sa.Server(pb), L.spiral_gpu_server_kv_stats), (sa.PackServer(pp, 2), L.spiral_gpu_pack_server_kv_stats)):
        srv.kv_load(TK, K.key_set(8), np.zeros((8, 248), dtype=np.uint8))
        assert srv.kv_stats(248).used == 8
        st, out = C.c_void_p(), _lib.KvStatsStruct()
        out.buckets = 77
        assert hip.hipStreamCreate(C.byref(st)) == 0
        srv.set_stream(st.value)
        assert hip.hipStreamBeginCapture(st, 2) == 0  # (hipStreamCaptureModeRelaxed)
        try:
            assert fn(srv.h, 248, 0, 4, C.byref(out)) != 0 and b"kv_stats cannot be called while the server's stream is being captured" in L.spiral_gpu_last_error()
        finally:
            g = C.c_void_p()
            assert hip.hipStreamEndCapture(st, C.byref(g)) == 0
            if g.value:
                hip.hipGraphDestroy(g)
        srv.set_stream(0)
        hip.hipStreamDestroy(st)
        assert out.buckets == 77, "a refused call wrote nothing"
        assert srv.kv_stats(248).used == 8, "and the server still answers"
        srv.close()


def base_model(lay, seed):
    """loaded_model under the base tests' load rule (tests/kv_restated.py load_size)"""
    rng = np.random.default_rng(seed)
    n = K.load_size(lay)
    assert (n, lay.buckets, lay.slots) in K.KEY_SETS, "tests/test_kv_cpu.py shows that this key set places"
    keys, vals = K.key_set(n), rng.integers(0, 256, size=(n, lay.value_bytes), dtype=np.uint8)
    model = K.Table(lay, TK)
    model.load(K.key_array(keys), vals)
    return keys, vals, model, rng
