"""Tracked fingerprints on the device (include/spiral_gpu.h "Fingerprints", Tracked): a resident table of polynomial sums and the combined value F that
update_db_items and update_records keep current, read in O(1), scrubbed against the image, exported and adopted.

After its updates every test requires all four (Tracker.check):
  - fingerprint_tracked()[0] equals fingerprint_items(key) of the same server,
  - both equal the host value from the restated plaintexts (tests/fingerprint_track_restated.py on a numpy model the test updates alongside),
  - fingerprint_tracked_polys() equals the restated g word for word,
  - fingerprint_scrub() returns (0, None).
The starting plaintexts are the ORACLE's (test_gpu_fingerprint.py's base_ref / pack_ref, shared with that module).  Exact integers throughout."""
import ctypes as C
import hashlib
import sys

import numpy as np
import pytest

import fingerprint_restated as FR
import fingerprint_track_restated as FTR
import pack_records_restated as PR
import records_restated as R
from test_gpu_fingerprint import KEY, KEY_TOP, base_ref, crafted_items, hip_runtime, pack_ref

pytestmark = pytest.mark.gpu
N = 2048
P = FR.P


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


@pytest.fixture(scope="module")
def PK(sa):
    from spiral_amd import pack as _  # noqa: F401  (spiral_amd.pack is also the name of a function: take the module itself)

    return sys.modules["spiral_amd.pack"]


_G = {}


class Tracker:
    """the plaintexts a tracked database should hold, [item][polynomial][2048], and their restated polynomial sums, kept alongside the server's updates"""

    def __init__(self, key, pts, tag):
        self.key = key
        self.pts = np.array(pts, dtype=np.uint64).reshape(len(pts), -1, N)
        k = (key, tag)
        if k not in _G:  # g of a whole database: computed once per (key, source), never written
            _G[k] = FTR.poly_sums(key, self.pts)
            _G[k].setflags(write=False)
        self.g = _G[k].copy()
        self.n_updates = 0

    def set_items(self, ids, new, q0=0):
        """items ids[k] <- new[k], polynomials q0 .. of each"""
        new = np.asarray(new, dtype=np.uint64).reshape(len(ids), -1, N)
        nq = new.shape[1]
        self.pts[ids, q0:q0 + nq] = new
        self.g[ids, q0:q0 + nq] = FTR.poly_sums(self.key, new)
        self.n_updates += len(ids) * nq

    def set_records(self, lay, S, ids, recs, instance=0, pack=False):
        """records ids[k] <- recs[k] spliced into the items' streams; returns the set of (item, polynomial) a record touches"""
        pb = 256 * lay.coeff_bits
        touched = set()
        for r, rec in zip(ids, np.asarray(recs).reshape(len(ids), S)):
            item, off, nb, first = (PR if pack else R).place(lay, S, int(r), instance)
            if pack:
                self.pts[item] = PR.splice(self.pts[item], lay.coeff_bits, off, rec[first:first + nb])
            else:
                self.pts[item] = R.splice(self.pts[item].reshape(2, 2, N), lay.coeff_bits, off, rec[first:first + nb]).reshape(4, N)
            touched |= {(item, q) for q in range(off // pb, -(-(off + nb) // pb))}
        for item in {i for i, _ in touched}:
            self.g[item] = FTR.poly_sums(self.key, self.pts[item])
        self.n_updates += len(touched)
        return touched

    def expected(self, mine=None, q0=0, q1=None):
        """the table a server should hold: rows of items it does not hold zero, the polynomials [q0, q1) it holds"""
        g = self.g[:, q0:q1]
        return g if mine is None else np.where(mine[:, None], g, 0).astype(np.uint64)

    def check(self, srv, what, mine=None, q0=0, q1=None, n_updates=None):
        g = self.expected(mine, q0, q1)
        F, n = srv.fingerprint_tracked()
        want = FTR.combined(self.key, g, q0)
        print(f"{what}: tracked F = {F}, restated F = {want}, n_updates = {n}")
        assert F == srv.fingerprint_items(self.key), f"{what}: tracked F against fingerprint_items of the same server"
        assert F == want, f"{what}: tracked F against the restated plaintexts"
        got = srv.fingerprint_tracked_polys()
        bad = np.argwhere(got != g)
        assert got.shape == g.shape and bad.size == 0, f"{what}: {len(bad)} table words differ from the restated g, first at (item, polynomial) {bad[:1].tolist()}"
        assert srv.fingerprint_scrub() == (0, None), f"{what}: scrub"
        if n_updates is not None:
            assert n == n_updates, f"{what}: n_updates"
        return F


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def spread_ids(s, n, seed):
    """n distinct items: the first, the last (the last band), both partners j and j ^ 32 of a column where the first dimension has them, and random ones"""
    total, np_ = s.dim0 * s.num_per, s.num_per
    ids = [0, total - 1, (3 % s.dim0) * np_ + 5 % np_]
    if s.dim0 >= 64:
        ids.append((3 ^ 32) * np_ + 5 % np_)
    rng = np.random.default_rng(seed)
    for i in rng.permutation(total):
        if len(ids) >= n:
            break
        if int(i) not in ids:
            ids.append(int(i))
    rng.shuffle(ids)  # (the call's order is not the image's)
    return [int(i) for i in ids]


# ---- 1. base, every form -----------------------------------------------------------------------------------------------------------------
BASE_CASES = [  # name, nu1, nu2, parameters, form, option sweep_narrow
    ("66-packed", 6, 6, dict(t_gsw=8), "packed", 0),
    ("66-limbs", 6, 6, dict(t_gsw=8), "limbs", 0),
    ("64-narrow", 6, 4, dict(t_gsw=8), "limbs", 1),
    ("43-tile", 4, 3, dict(t_gsw=8), "packed", 0),
    ("22-plain", 2, 2, dict(t_gsw=4), "packed", 0),
    ("43-p15", 4, 3, dict(t_gsw=8, p_db=1 << 15), "packed", 0),
]


def base_seed(nu1, nu2, kw):
    return 33 if "p_db" in kw else 21 if (nu1, nu2) == (6, 6) else 17


@pytest.mark.parametrize("name,nu1,nu2,kw,form,narrow", BASE_CASES, ids=[c[0] for c in BASE_CASES])
def test_base_every_form(sa, SV, oracle, opts, name, nu1, nu2, kw, form, narrow):
    """track, then update_db_items of one item (stream width log2 p_db), of a scattered list (an odd width above it), of the crafted items (40 bits), and of
    an item to its present content (64 bits): F unchanged by the last, n_updates 4 per item"""
    O = oracle
    opts(sweep_narrow=narrow)
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.shape_of(po)
    total, p_db = s.dim0 * s.num_per, int(po.p_db)
    seed = base_seed(nu1, nu2, kw)
    pts, _ = base_ref(sa, O, po, seed)
    srv = sa.Server(pg)
    srv.gen_db(seed)
    if form == "limbs":
        srv.set_db_format(SV.DB_LIMBS)
    fmt = srv.db_format()
    held = pts
    for key in ((KEY, KEY_TOP) if name == "43-tile" else (KEY,)):  # (the largest weight r = P - 2 once, on what the first key's updates left)
        t = Tracker(key, held, ("base", nu1, nu2, p_db, seed) if held is pts else ("after the first key", name))
        srv.fingerprint_track(key)
        t.check(srv, f"{name}: after track", n_updates=0)
        w0 = p_db.bit_length() - 1
        rng = np.random.default_rng(5)
        one = [total // 2 + 1]
        new = rng.integers(0, p_db, size=(1, 4 * N), dtype=np.uint64)
        srv.update_db_items(O.pack_items(new, w0), w0, one)
        t.set_items(one, new)
        t.check(srv, f"{name}: one item at {w0} bits", n_updates=4)
        ids = spread_ids(s, 7, 11)
        new = rng.integers(0, p_db, size=(len(ids), 4 * N), dtype=np.uint64)
        odd = 9 if w0 == 8 else 17
        assert odd > w0
        srv.update_db_items(O.pack_items(new, odd), odd, ids)
        t.set_items(ids, new)
        t.check(srv, f"{name}: a scattered list at an odd width", n_updates=4 * (1 + len(ids)))
        new = crafted_items(p_db)
        ids = spread_ids(s, len(new), 13)
        srv.update_db_items(O.pack_items(new, 40), 40, ids)
        t.set_items(ids, new)
        F = t.check(srv, f"{name}: the crafted items at 40 bits")
        n = t.n_updates
        same = [ids[0]] + [i for i in one if i != ids[0]]
        srv.update_db_items(O.pack_items(t.pts[same], 64), 64, same)
        assert t.check(srv, f"{name}: items updated to their present content at 64 bits", n_updates=n + 4 * len(same)) == F
        assert srv.db_format() == fmt
        held = t.pts
    srv.close()


# ---- 2. records --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["packed", "limbs"])
@pytest.mark.parametrize("S", [256, 100, 8191])
def test_records(sa, SV, oracle, form, S):
    """(6, 6): one record; the records that cover polynomial 1 of an item whole (the `full` path, nothing read) and its neighbours in part; two records in one
    polynomial; a record that leaves the other polynomials of its item untouched -- their table words are bit-identical and not counted.  S = 100 puts
    record ends inside a coefficient and records across polynomials; S = 8191 leaves padding"""
    O = oracle
    po, pg = O.make_params(6, 6, t_gsw=8), sa.make_params(6, 6, t_gsw=8)
    s = O.shape_of(po)
    np_ = s.num_per
    pts, _ = base_ref(sa, O, po, 21)
    lay = R.layout(int(po.p_db), 6, 6, S)
    pi, pb = lay.per_item, 256 * lay.coeff_bits
    rec = lambda item, k: item * pi + k % pi
    srv = sa.Server(pg)
    srv.gen_db(21)
    if form == "limbs":
        srv.set_db_format(SV.DB_LIMBS)
    t = Tracker(KEY, pts, ("base", 6, 6, 256, 21))
    srv.fingerprint_track(KEY)
    rng = np.random.default_rng(S)
    a = 5 * np_ + 16
    calls = [("one record", [rec(2 * np_ + 3, 1)]),
             ("a polynomial covered whole", sorted({rec(a, k) for k in range(pi) if k * S < 2 * pb and (k + 1) * S > pb}, reverse=True))]
    if pi >= 6:
        calls.append(("two records in one polynomial", [rec(40 * np_ + 7, 5), rec(40 * np_ + 7, 0)]))
    calls.append(("records of several items", [rec(63 * np_ + 63, pi - 1), 0, rec(a + 1, 3), rec(35 * np_ + 9, 2), rec(3 * np_ + 9, 2)]))
    for what, ids in calls:
        recs = rng.integers(0, 256, size=(len(ids), S), dtype=np.uint8)
        before = srv.fingerprint_tracked_polys()
        srv.update_records(recs, S, ids)
        touched = t.set_records(lay, S, ids, recs)
        t.check(srv, f"S = {S} {form}: {what}", n_updates=t.n_updates)
        after = srv.fingerprint_tracked_polys()
        keep = np.ones(after.shape, dtype=bool)
        keep[[i for i, _ in touched], [q for _, q in touched]] = False
        assert (after[keep] == before[keep]).all(), f"S = {S} {form}: {what}: a table word of an untouched polynomial changed"
        if S != 8191:
            assert any((i, q) not in touched for i, _ in touched for q in range(4)), "the call leaves polynomials of a touched item untouched"
    srv.close()


def test_records_second_instance(sa, oracle):
    """instance 1 of a 2-instance layout at (4, 3): the chunk behind the first item_bytes of each record, with padding behind it"""
    O = oracle
    po, pg = O.make_params(4, 3, t_gsw=8), sa.make_params(4, 3, t_gsw=8)
    S = 12000
    lay = R.layout(int(po.p_db), 4, 3, S)
    assert (lay.instances, lay.per_item) == (2, 1)
    pts, _ = base_ref(sa, O, po, 17)
    srv = sa.Server(pg)
    srv.gen_db(17)
    t = Tracker(KEY, pts, ("base", 4, 3, 256, 17))
    srv.fingerprint_track(KEY)
    ids = [127, 0, 64]
    recs = np.random.default_rng(2).integers(0, 256, size=(3, S), dtype=np.uint8)
    srv.update_records(recs, S, ids, instance=1)
    touched = t.set_records(lay, S, ids, recs, instance=1)
    assert len(touched) == 6, "12000 - 8192 bytes: polynomials 0 and 1 of each item"
    t.check(srv, "instance 1 of 2", n_updates=6)
    srv.close()


# ---- 3. SpiralPack -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu1,nu2,out_n,forms,option", [
    (7, 5, 1, ("packed", "limbs"), None),
    (7, 3, 3, ("limbs",), "pack_pair_blocks"),
    (6, 2, 2, ("packed",), None),
])
def test_pack(sa, PK, oracle_mt, opts, nu1, nu2, out_n, forms, option):
    """update_db_items on two different trials (the one trial twice at out_n = 1) and update_records with records that straddle trial images, in each form"""
    O = oracle_mt
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    total, trials = s.dim0 * s.num_per, s.trials
    pts, _ = pack_ref(sa, O, po, out_n, 41)
    srv = sa.PackServer(pg, out_n)
    srv.gen_db(41)
    if option:
        opts(**{option: 1})
    t = Tracker(KEY, pts, ("pack", nu1, nu2, out_n, 41))
    S = 100
    lay = PR.layout(int(po.p_db), nu1, nu2, out_n, S)
    rng = np.random.default_rng(out_n)
    for form in forms:
        if form == "limbs":
            srv.set_db_format(PK.DB_LIMBS)
        srv.fingerprint_track(KEY)
        n0 = t.n_updates
        what = f"({nu1}, {nu2}, {out_n}) {form}"
        t.check(srv, f"{what}: after track", n_updates=0)
        for k, trial in enumerate((0, trials - 1)):
            ids = [total - 1, 3, (70 % s.dim0) * s.num_per + 1, 9 * s.num_per + 2][:3 + k]
            assert len(set(ids)) == len(ids)
            new = rng.integers(0, 256, size=(len(ids), N), dtype=np.uint64)
            srv.update_db_items(trial, O.pack_items(new, 9 + 31 * k), 9 + 31 * k, ids)  # 9 and 40 bits
            t.set_items(ids, new, q0=trial)
            t.check(srv, f"{what}: update_db_items of trial {trial}", n_updates=t.n_updates - n0)
        pi = lay.per_item
        ids = [lay.capacity - 1, 5 * pi + 20 % pi, 5 * pi + 21 % pi, 0, (total // 2) * pi + (pi // 2)]  # 2048-byte polynomials, 100-byte records: 20 straddles
        ids = sorted(set(ids), reverse=True)
        recs = rng.integers(0, 256, size=(len(ids), S), dtype=np.uint8)
        srv.update_records(recs, S, ids)
        touched = t.set_records(lay, S, ids, recs, pack=True)
        if trials > 1:
            assert any(len(PR.trials_of(lay, *PR.place(lay, S, r)[1:3])) == 2 for r in ids), "a record of the list straddles two trial images"
            assert len({q for _, q in touched}) >= 4
        t.check(srv, f"{what}: update_records", n_updates=t.n_updates - n0)
    srv.close()


# ---- 4. conversion keeps the state -------------------------------------------------------------------------------------------------------
def test_conversion_keeps_the_state(sa, SV, oracle):
    O = oracle
    po, pg = O.make_params(6, 6, t_gsw=8), sa.make_params(6, 6, t_gsw=8)
    s = O.shape_of(po)
    pts, _ = base_ref(sa, O, po, 21)
    srv = sa.Server(pg)
    srv.gen_db(21)
    t = Tracker(KEY, pts, ("base", 6, 6, 256, 21))
    srv.fingerprint_track(KEY)
    rng = np.random.default_rng(4)
    steps = [("packed", None), ("limb planes", SV.DB_LIMBS), ("packed again", SV.DB_PACKED)]
    for k, (what, fmt) in enumerate(steps):
        if fmt is not None:
            srv.set_db_format(fmt)
            t.check(srv, f"converted to {what}", n_updates=t.n_updates)
        ids = spread_ids(s, 5, 20 + k)
        new = rng.integers(0, 256, size=(len(ids), 4 * N), dtype=np.uint64)
        srv.update_db_items(O.pack_items(new, 8), 8, ids)
        t.set_items(ids, new)
        t.check(srv, f"updated in {what}", n_updates=t.n_updates)
    srv.close()


# ---- 5. shards ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["j", "column"])
def test_base_shards(sa, SV, oracle, opts, kind):
    """j-shard halves of (6, 6) / column shards G = 2 of (6, 4): each shard tracks its local items with database indices in the powers of s; every shard is
    given the same update lists; the partial F's add to the unsharded tracked value and the shards' tables add to the unsharded table"""
    O = oracle
    nu1, nu2 = (6, 6) if kind == "j" else (6, 4)
    opts(sweep_narrow=1)
    po, pg = O.make_params(nu1, nu2, t_gsw=8), sa.make_params(nu1, nu2, t_gsw=8)
    s = O.shape_of(po)
    total, np_ = s.dim0 * s.num_per, s.num_per
    seed = base_seed(nu1, nu2, {})
    pts, _ = base_ref(sa, O, po, seed)
    item = np.arange(total)
    if kind == "j":
        shards = [sa.Server(pg, j_begin=0, j_end=32), sa.Server(pg, j_begin=32, j_end=64)]
        mine = [item // np_ < 32, item // np_ >= 32]
    else:
        shards = [sa.Server(pg, col_rank=g, col_ranks=2) for g in range(2)]
        mine = [item % 2 == 0, item % 2 == 1]
    whole = sa.Server(pg)
    t = Tracker(KEY, pts, ("base", nu1, nu2, 256, seed))
    for sv in shards + [whole]:
        sv.gen_db(seed)
        sv.fingerprint_track(KEY)
    rng = np.random.default_rng(8)
    ids = spread_ids(s, 9, 31)
    new = rng.integers(0, 256, size=(len(ids), 4 * N), dtype=np.uint64)
    S = 100
    lay = R.layout(256, nu1, nu2, S)
    rids = sorted({0, lay.capacity - 1, 5 * lay.per_item + 20, (total // 2 + 1) * lay.per_item + 3, (total // 2) * lay.per_item + 40})
    recs = rng.integers(0, 256, size=(len(rids), S), dtype=np.uint8)
    for sv in shards + [whole]:
        sv.update_db_items(O.pack_items(new, 8), 8, ids)
        sv.update_records(recs, S, rids)
    t.set_items(ids, new)
    t.set_records(lay, S, rids, recs)
    F = t.check(whole, f"{kind}-shards: the unsharded server", n_updates=t.n_updates)
    parts = [t.check(sv, f"{kind}-shard {k}", mine=mine[k]) for k, sv in enumerate(shards)]
    assert sa.fingerprint_add(*parts) == F, "the partial F's add to the unsharded tracked value"
    assert sum(sv.fingerprint_tracked()[1] for sv in shards) == t.n_updates, "each replaced word is counted by the shard that holds it"
    table = np.zeros((total, 4), dtype=np.uint64)
    for sv in shards:
        table += sv.fingerprint_tracked_polys()  # (a word is nonzero in one shard's output only: no carry, no reduction)
    assert (table == whole.fingerprint_tracked_polys()).all(), "the shards' tables reassemble the unsharded table"
    first, n = total // 2 - 5, 11  # a range across the j boundary, odd ends for the columns
    assert (sum(sv.fingerprint_tracked_polys(first, n) for sv in shards) == t.g[first:first + n]).all()
    assert all(sv.fingerprint_scrub(first, n) == (0, None) for sv in shards)
    for sv in shards + [whole]:
        sv.close()


def test_trial_shards(sa, PK, oracle_mt):
    """trial shards 2 + 7 of (6, 2, out_n 3): each tracks the polynomials of its trial range, weights from r^(2048 t0) on"""
    O = oracle_mt
    po, pg = O.make_params(6, 2), sa.make_params(6, 2)
    s = O.pack_shape_of(po, 3)
    total = s.dim0 * s.num_per
    pts, _ = pack_ref(sa, O, po, 3, 41)
    ranges = [(0, 2), (2, 9)]
    shards = [sa.PackServer(pg, 3, trial0=a, trial1=b) for a, b in ranges]
    whole = sa.PackServer(pg, 3)
    t = Tracker(KEY, pts, ("pack", 6, 2, 3, 41))
    for sv in shards + [whole]:
        sv.gen_db(41)
        sv.fingerprint_track(KEY)
    rng = np.random.default_rng(9)
    S = 100
    lay = PR.layout(256, 6, 2, 3, S)
    rids = sorted({0, lay.capacity - 1, 5 * lay.per_item + 20, 5 * lay.per_item + 40, 9 * lay.per_item + 61})  # 20 and 40 straddle trials; 40 crosses 1 | 2
    recs = rng.integers(0, 256, size=(len(rids), S), dtype=np.uint8)
    for trial in (1, 2, 8):
        ids = [total - 1, 3 + trial, 77]
        new = rng.integers(0, 256, size=(len(ids), N), dtype=np.uint64)
        for sv, (a, b) in zip(shards + [whole], ranges + [(0, 9)]):
            if a <= trial < b:
                sv.update_db_items(trial, O.pack_items(new, 8), 8, ids)
        t.set_items(ids, new, q0=trial)
    for sv in shards + [whole]:
        sv.update_records(recs, S, rids)
    t.set_records(lay, S, rids, recs, pack=True)
    F = t.check(whole, "trial shards: the unsharded server", n_updates=t.n_updates)
    parts = [t.check(sv, f"trials [{a}, {b})", q0=a, q1=b) for sv, (a, b) in zip(shards, ranges)]
    assert sa.fingerprint_add(*parts) == F
    assert sum(sv.fingerprint_tracked()[1] for sv in shards) == t.n_updates
    assert (np.hstack([sv.fingerprint_tracked_polys() for sv in shards]) == whole.fingerprint_tracked_polys()).all()
    for sv in shards + [whole]:
        sv.close()


# ---- 6. scrub finds what differs ---------------------------------------------------------------------------------------------------------
def test_scrub_finds_altered_words(sa, SV, oracle):
    O = oracle
    po, pg = O.make_params(6, 6, t_gsw=8), sa.make_params(6, 6, t_gsw=8)
    s = O.shape_of(po)
    total, np_ = s.dim0 * s.num_per, s.num_per
    pts, _ = base_ref(sa, O, po, 21)
    srv = sa.Server(pg)
    srv.gen_db(21)
    t = Tracker(KEY, pts, ("base", 6, 6, 256, 21))
    srv.fingerprint_track(KEY)
    table = srv.fingerprint_tracked_polys()
    assert (table == t.g).all()
    altered = table.copy()
    mid = 20 * np_ + 33  # the middle of a band
    for i, q in ((0, 0), (mid, 2), (total - 1, 3)):  # the first word, one inside, the last word: different polynomials
        altered[i, q] = (int(altered[i, q]) + 1) % P
    srv.fingerprint_track(KEY, altered)
    F, n = srv.fingerprint_tracked()
    assert F == FTR.combined(KEY, altered) and n == 0 and (srv.fingerprint_tracked_polys() == altered).all(), "an adopted table is taken as given"
    assert F != srv.fingerprint_items(KEY)
    assert srv.fingerprint_scrub() == (3, (0, 0))
    assert srv.fingerprint_scrub(1, mid - 1) == (0, None) and srv.fingerprint_scrub(mid + 1, total - mid - 2) == (0, None), "ranges that exclude them"
    assert srv.fingerprint_scrub(1, total - 1) == (2, (mid, 2))
    assert srv.fingerprint_scrub(total - 7, 7) == (1, (total - 1, 3)), "a range that holds only the last"
    assert srv.fingerprint_scrub(mid, 0) == (0, None)
    lane = sa.Server(pg, share_db_of=srv)
    assert lane.fingerprint_scrub() == (3, (0, 0)) and lane.fingerprint_tracked() == (F, 0), "a lane reads the owner's state"
    lane.close()
    # an update heals the words it replaces
    srv.update_db_items(O.pack_items(pts[[0]], 8), 8, [0])
    assert srv.fingerprint_scrub() == (2, (mid, 2))
    srv.close()


def test_adopt_across_servers(sa, SV, oracle, opts):
    """server B holds another database that agrees with A's in 5 items; B adopts A's table: its scrub reports exactly the polynomials whose restated g
    differ, the same in 16-item passes"""
    O = oracle
    po, pg = O.make_params(6, 4, t_gsw=8), sa.make_params(6, 4, t_gsw=8)
    s = O.shape_of(po)
    total = s.dim0 * s.num_per
    pts_a, _ = base_ref(sa, O, po, 17)
    pts_b, _ = base_ref(sa, O, po, 18)
    A, B = sa.Server(pg), sa.Server(pg)
    A.gen_db(17)
    B.gen_db(18)
    ids = [total - 1, 5, 300, 301, 64]
    B.update_db_items(O.pack_items(pts_a[ids], 8), 8, ids)
    ta, tb = Tracker(KEY, pts_a, ("base", 6, 4, 256, 17)), Tracker(KEY, pts_b, ("base", 6, 4, 256, 18))
    tb.set_items(ids, pts_a[ids])
    A.fingerprint_track(KEY)
    table = A.fingerprint_tracked_polys()
    assert (table == ta.g).all()
    B.fingerprint_track(KEY, table)
    differ = np.argwhere(ta.g != tb.g)
    assert len(differ) >= 4 * (total - len(ids)) - 8 and not any(int(i) in ids for i, _ in differ), "the restatement: all but the 5 items differ"
    want = (len(differ), (int(differ[0][0]), int(differ[0][1])))
    print("adopted table against another image:", want)
    assert B.fingerprint_scrub() == want
    opts(db_stage_bytes=8 * (4 + 1) * 16)
    assert B.fingerprint_scrub() == want, "in passes of 16 items"
    first = 290
    sub = np.argwhere(ta.g[first:first + 40] != tb.g[first:first + 40])
    assert B.fingerprint_scrub(first, 40) == (len(sub), (first + int(sub[0][0]), int(sub[0][1]))), "a range, in passes"
    opts(db_stage_bytes=64 << 20)
    assert B.fingerprint_tracked()[0] == A.fingerprint_tracked()[0] == FTR.combined(KEY, ta.g)
    with pytest.raises(sa.SpiralGpuError, match="not below"):
        B.fingerprint_track(KEY, np.where(np.arange(table.size).reshape(table.shape) == 7, P, table).astype(np.uint64))
    with pytest.raises(ValueError, match="poly_sums"):
        B.fingerprint_track(KEY, table[:-1])
    A.close()
    B.close()


# ---- 7. a failing update leaves image, table, F and n_updates as they were -----------------------------------------------------------------
def state_of(srv):
    return digest(srv.read_db_slots(0, N)), digest(srv.fingerprint_tracked_polys()), srv.fingerprint_tracked()


def test_failing_updates_change_nothing(sa, SV, oracle):
    O = oracle
    po, pg = O.make_params(6, 6, t_gsw=8), sa.make_params(6, 6, t_gsw=8)
    s = O.shape_of(po)
    total = s.dim0 * s.num_per
    pts, _ = base_ref(sa, O, po, 21)
    L = sa.lib()
    srv = sa.Server(pg)
    srv.gen_db(21)
    srv.set_db_format(SV.DB_LIMBS)
    t = Tracker(KEY, pts, ("base", 6, 6, 256, 21))
    srv.fingerprint_track(KEY)
    srv.update_db_items(O.pack_items(pts[[9]] ^ 1, 8), 8, [9])
    t.set_items([9], pts[[9]] ^ 1)
    before = state_of(srv)
    assert before[2][1] == 4
    new = np.zeros((3, 4 * N), dtype=np.uint64)
    buf, U64P = new.ctypes.data_as(C.c_void_p), C.POINTER(C.c_uint64)
    for ids, text in (([3, 700, 3], b"twice"), ([3, 700, total], b"outside")):
        a = np.array(ids, dtype=np.uint64)
        assert L.spiral_gpu_server_update_db_items(srv.h, buf, 64, a.ctypes.data_as(U64P), 3) != 0 and text in L.spiral_gpu_last_error()
        assert state_of(srv) == before, f"after a refused update ({text})"
    new[2, 4 * N - 1] = 256  # a coefficient >= p_db at width 64
    a = np.array([3, 700, 5], dtype=np.uint64)
    assert L.spiral_gpu_server_update_db_items(srv.h, buf, 64, a.ctypes.data_as(U64P), 3) != 0 and b"not below p_db" in L.spiral_gpu_last_error()
    assert state_of(srv) == before, "after a coefficient >= p_db"
    t.check(srv, "after the refused updates", n_updates=4)
    srv.close()


def test_failing_record_update_changes_nothing(sa, oracle):
    """the device-detected failure: (4, 3) with p_db = 3 * 2^13, w = 14 -- the oracle's items hold coefficients of 2^14 and more, which are no record data.
    A record that covers part of a polynomial makes the kernel read it, flag it, and everything behind it is skipped"""
    O = oracle
    kw = dict(t_gsw=8, p_db=3 << 13)
    po, pg = O.make_params(4, 3, **kw), sa.make_params(4, 3, **kw)
    pts, _ = base_ref(sa, O, po, 33)
    assert int(pts.max()) >= 1 << 14
    srv = sa.Server(pg)
    srv.gen_db(33)
    t = Tracker(KEY, pts, ("base", 4, 3, 3 << 13, 33))
    srv.fingerprint_track(KEY)
    before = state_of(srv)
    S = 100
    recs = np.random.default_rng(1).integers(0, 256, size=(2, S), dtype=np.uint8)
    with pytest.raises(sa.SpiralGpuError, match="no record data"):
        srv.update_records(recs, S, [40, 3])
    assert state_of(srv) == before
    t.check(srv, "after the failed record update", n_updates=0)
    srv.close()


# ---- 8. lifecycle ------------------------------------------------------------------------------------------------------------------------
def test_lifecycle(sa, SV, oracle):
    O = oracle
    po, pg = O.make_params(6, 6, t_gsw=8), sa.make_params(6, 6, t_gsw=8)
    s = O.shape_of(po)
    total = s.dim0 * s.num_per
    pts, _ = base_ref(sa, O, po, 21)
    L = sa.lib()
    srv = sa.Server(pg)
    with pytest.raises(sa.SpiralGpuError, match="no database loaded"):
        srv.fingerprint_track(KEY)
    with pytest.raises(sa.SpiralGpuError, match="not tracked"):
        srv.fingerprint_tracked()
    srv.gen_db(21)
    with pytest.raises(sa.SpiralGpuError, match="not tracked"):
        srv.fingerprint_scrub()
    with pytest.raises(sa.SpiralGpuError, match="not tracked"):
        srv.fingerprint_tracked_polys()
    t = Tracker(KEY, pts, ("base", 6, 6, 256, 21))
    # every loader ends tracking
    for what, load in (("gen_db", lambda: srv.gen_db(21)), ("load_db_items", lambda: srv.load_db_items(O.pack_items(pts[64:72], 8), 8, 64, 8)),
                       ("fill_db_random", lambda: srv.fill_db_random(3))):
        srv.fingerprint_track(KEY)
        assert srv.fingerprint_tracked() == (FTR.combined(KEY, t.g), 0)
        load()
        with pytest.raises(sa.SpiralGpuError, match="not tracked"):
            srv.fingerprint_tracked()
    with pytest.raises(sa.SpiralGpuError, match=r"plaintext at item 0 \(polynomial 0, coefficient 0 "):
        srv.fingerprint_track(KEY)  # (the image of fill_db_random)
    with pytest.raises(sa.SpiralGpuError, match="not tracked"):
        srv.fingerprint_tracked()
    srv.gen_db(21)
    # a graph captured before track replays after tracked updates, and nothing is captured again
    cl = O.Client(po, seed=9)
    srv.set_pub_params(*cl.pub_params())
    srv.use_graphs(True)
    idx = 700
    srv.set_query(cl.query(idx))
    srv.run_query()
    srv.run_query()
    srv.sync()
    caps = sa.get_option("graph_captures")
    srv.fingerprint_track(KEY_TOP)
    srv.fingerprint_track(KEY)  # tracking again replaces the state
    assert srv.fingerprint_tracked_key() == KEY
    new = np.random.default_rng(3).integers(0, 256, size=(1, 4 * N), dtype=np.uint64)
    srv.update_db_items(O.pack_items(new, 8), 8, [idx])
    t.set_items([idx], new)
    srv.run_query()
    srv.sync()
    assert sa.get_option("graph_captures") == caps, "a tracked update forced a capture"
    assert (cl.decode(srv.read(SV.BUF_RESPONSE)).reshape(-1) == new.reshape(-1)).all(), "the replayed graph returns the new item"
    F = t.check(srv, "after the replay", n_updates=4)
    # lanes and share_db servers read, and may not track
    lane, other = sa.Server(pg, share_db_of=srv), sa.Server(pg)
    other.share_db(srv)
    for rd in (lane, other):
        assert rd.fingerprint_tracked() == (F, 4) and rd.fingerprint_scrub(5, 9) == (0, None)
        assert (rd.fingerprint_tracked_polys(idx, 1) == t.g[idx]).all()
        with pytest.raises(sa.SpiralGpuError, match="through the owner"):
            rd.fingerprint_track(KEY)
        with pytest.raises(sa.SpiralGpuError, match="through the owner"):
            rd.fingerprint_untrack()
    lane.close()
    other.close()
    assert srv.fingerprint_tracked() == (F, 4)
    # inside a capture
    hip = hip_runtime()
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    srv.set_stream(st.value)
    assert hip.hipStreamBeginCapture(st, 2) == 0  # (hipStreamCaptureModeRelaxed)
    try:
        key = (C.c_uint64 * 2)(*KEY_TOP)
        n_bad = C.c_uint64(0)
        assert L.spiral_gpu_server_fingerprint_track(srv.h, key, None) != 0 and b"captured" in L.spiral_gpu_last_error()
        assert L.spiral_gpu_server_fingerprint_scrub(srv.h, 0, 4, C.byref(n_bad), None, None) != 0 and b"captured" in L.spiral_gpu_last_error()
    finally:
        g = C.c_void_p()
        assert hip.hipStreamEndCapture(st, C.byref(g)) == 0
        if g.value:
            hip.hipGraphDestroy(g)
    srv.set_stream(0)
    hip.hipStreamDestroy(st)
    assert srv.fingerprint_tracked() == (F, 4) and srv.fingerprint_tracked_key() == KEY, "a refused track leaves the state"
    with pytest.raises(sa.SpiralGpuError, match="outside"):
        srv.fingerprint_scrub(total - 1, 2)
    with pytest.raises(sa.SpiralGpuError, match="outside"):
        srv.fingerprint_tracked_polys(total, 1)
    srv.fingerprint_untrack()
    with pytest.raises(sa.SpiralGpuError, match="not tracked"):
        srv.fingerprint_tracked()
    srv.fingerprint_untrack()  # (nothing to free: no error)
    srv.close()


def test_pack_lifecycle(sa, PK, oracle_mt):
    O = oracle_mt
    po, pg = O.make_params(6, 2), sa.make_params(6, 2)
    pts, _ = pack_ref(sa, O, po, 2, 41)
    srv = sa.PackServer(pg, 2)
    srv.fill_db_random(3)
    with pytest.raises(sa.SpiralGpuError, match=r"plaintext at item 0 \(polynomial 0, "):
        srv.fingerprint_track(KEY)
    with pytest.raises(sa.SpiralGpuError, match="not tracked"):
        srv.fingerprint_tracked()
    srv.gen_db(41)
    t = Tracker(KEY, pts, ("pack", 6, 2, 2, 41))
    srv.fingerprint_track(KEY)
    lane = srv.create_lane()
    F = t.check(lane, "a lane of a pack server")
    with pytest.raises(sa.SpiralGpuError, match="through the owner"):
        lane.fingerprint_track(KEY)
    lane.close()
    srv.load_db_items(1, O.pack_items(pts[:4, 1], 8), 8, 0, 4)
    with pytest.raises(sa.SpiralGpuError, match="not tracked"):
        srv.fingerprint_tracked()
    srv.fingerprint_track(KEY)
    assert srv.fingerprint_tracked() == (F, 0)
    srv.close()
