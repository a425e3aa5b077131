"""Content fingerprints computed on the device from the image in whichever form it is in (include/spiral_gpu.h "Fingerprints":
spiral_gpu_server_fingerprint_items / _at and the SpiralPack pair).  Every expected value is spiral_amd.fingerprint_host -- itself checked against the
definition in Python integers by tests/test_fingerprint_cpu.py -- of the ORACLE's plaintexts (db_item, pack_db_item), the route
tests/test_gpu_db_export.py takes: the comparison is with the oracle, not with the image under test."""
import ctypes as C
import sys

import numpy as np
import pytest

import fingerprint_restated as FR

pytestmark = pytest.mark.gpu
N = 2048
P = FR.P
KEY = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F)
KEY_TOP = (P - 4, 0x1234567)  # r = P - 2, the largest weight


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


_REF = {}


def base_ref(sa, O, po, seed, key=KEY):
    """(plaintexts [item][4 * 2048] of the oracle database, their item fingerprints under `key`): computed once per geometry, seed and key, never written"""
    k = ("base", po.nu1, po.nu2, po.p_db, seed, key)
    if k not in _REF:
        s = O.shape_of(po)
        total = s.dim0 * s.num_per
        pk = k[:-1]
        if pk not in _REF:
            pts = np.empty((total, 4 * N), dtype=np.uint64)
            for i in range(total):
                pts[i] = O.db_item(po, seed, i).reshape(-1)
            pts.setflags(write=False)
            _REF[pk] = pts
        f = sa.fingerprint_host(key, po.p_db, _REF[pk], 64, per_item=True)[1]
        f.setflags(write=False)
        _REF[k] = (_REF[pk], f)
    return _REF[k]


def pack_ref(sa, O, po, out_n, seed, key=KEY):
    """(plaintexts [item][trial][2048] of the oracle's SpiralPack database -- the record layout's order -- and their item fingerprints)"""
    k = ("pack", po.nu1, po.nu2, out_n, seed, key)
    if k not in _REF:
        s = O.pack_shape_of(po, out_n)
        total = s.dim0 * s.num_per
        pts = np.empty((total, s.trials, N), dtype=np.uint64)
        for i in range(total):
            pts[i] = O.pack_db_item(po, out_n, seed, i).reshape(s.trials, N)
        pts.setflags(write=False)
        f = sa.fingerprint_host(key, po.p_db, pts, 64, polys_per_item=s.trials, per_item=True)[1]
        f.setflags(write=False)
        _REF[k] = (pts, f)
    return _REF[k]


def check_calls(srv, key, f, total, np_, what):
    """the whole database, a range that starts and ends inside a band, and an unsorted id list with a duplicate: per item and combined.  f: the expected item
    fingerprints of every database item (a shard's partial values)"""
    F, got = srv.fingerprint_items(key, per_item=True)
    assert got.dtype == np.uint64 and got.shape == (total,)
    bad = np.flatnonzero(got != f)
    assert bad.size == 0, f"{what}: {bad.size} of {total} item fingerprints differ, first at item {bad[0]}: {got[bad[0]]} for {f[bad[0]]}"
    assert F == FR.combine(key, f, range(total)), f"{what}: combined, whole database"
    assert srv.fingerprint_items(key) == F, f"{what}: combined alone"
    first = np_ + 1 if total > np_ + 3 else 1
    n = max(1, min(2 * np_ + 5, total - first - 2))
    Fr, got = srv.fingerprint_items(key, first, n, per_item=True)
    assert (got == f[first:first + n]).all() and Fr == FR.combine(key, f[first:first + n], range(first, first + n)), f"{what}: items [{first}, +{n})"
    ask = [total - 1, 0, total // 2, first + 1, 1, total // 2, 0]
    Fa, got = srv.fingerprint_items_at(key, ask)
    assert (got == f[ask]).all() and Fa == FR.combine(key, f[ask], ask), f"{what}: by id {ask}"
    return F


# ---- 1. base geometries, every form each has ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu1,nu2,kw,limbs", [
    (6, 6, dict(t_gsw=8), True),   # packed and the wide limb planes
    (6, 3, dict(t_gsw=8), True),   # the 1-wave narrow form
    (6, 4, dict(t_gsw=8), True),   # 2 waves
    (6, 5, dict(t_gsw=8), True),   # 4 waves
    (4, 3, dict(t_gsw=8), False),  # a packed tile
    (3, 2, dict(t_gsw=4), False),
    (2, 2, dict(t_gsw=4), False),  # the plain layout
    (4, 3, dict(t_gsw=8, p_db=1 << 15), False),  # the centred lift's upper half in use
])
def test_base_every_form(sa, SV, oracle, opts, nu1, nu2, kw, limbs):
    O = oracle
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.shape_of(po)
    total = s.dim0 * s.num_per
    seed = 33 if "p_db" in kw else 21 if (nu1, nu2) == (6, 6) else 17
    pts, f = base_ref(sa, O, po, seed)
    srv = sa.Server(pg)
    srv.gen_db(seed)
    F = check_calls(srv, KEY, f, total, s.num_per, f"({nu1}, {nu2}) packed")
    assert srv.db_format() == SV.DB_PACKED
    if limbs:
        opts(sweep_narrow=1)
        srv.set_db_format(SV.DB_LIMBS)
        assert check_calls(srv, KEY, f, total, s.num_per, f"({nu1}, {nu2}) limb planes") == F
        assert srv.db_format() == SV.DB_LIMBS
    assert sa.get_option("db_fingerprint_ns") > 0
    srv.close()


# ---- 2. SpiralPack, every form -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu1,nu2,out_n,forms,option", [
    (7, 7, 1, ("packed", "limbs"), None),
    (7, 5, 1, ("packed", "limbs"), None),
    (7, 3, 1, ("packed", "limbs"), "pack_pair_blocks"),
    (7, 3, 3, ("limbs",), "pack_pair_blocks"),
    (6, 2, 2, ("packed",), None),
    (3, 2, 1, ("packed",), None),
])
def test_pack_every_form(sa, PK, oracle_mt, opts, nu1, nu2, out_n, forms, option):
    """the geometry list of test_gpu_db_export.py's test_pack_every_form; the owner and a lane call in turn"""
    O = oracle_mt
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    total = s.dim0 * s.num_per
    pts, f = pack_ref(sa, O, po, out_n, 41)
    owner = sa.PackServer(pg, out_n)
    owner.gen_db(41)
    lane = owner.create_lane()
    if option:
        opts(**{option: 1})
    for k, form in enumerate(forms):
        if form == "limbs":
            owner.set_db_format(PK.DB_LIMBS)
        fmt = owner.db_format()
        assert fmt == (PK.DB_LIMBS if form == "limbs" else PK.DB_PACKED)
        check_calls(lane if k == 0 else owner, KEY, f, total, s.num_per, f"({nu1}, {nu2}, {out_n}) {form}")
        assert lane.fingerprint_items(KEY, 3, 2) == owner.fingerprint_items(KEY, 3, 2)
        assert owner.db_format() == fmt
    lane.close()
    owner.close()


def test_pack_trial_shards(sa, PK, oracle_mt):
    """9 trials split 2 + 7: each rank sums the polynomials of its trials, the partials add to the whole values"""
    O = oracle_mt
    po, pg = O.make_params(6, 2), sa.make_params(6, 2)
    s = O.pack_shape_of(po, 3)
    total = s.dim0 * s.num_per
    pts, f = pack_ref(sa, O, po, 3, 41)
    ask = [total - 1, 4, 4, 0]
    got_f, got_F, got_at = np.zeros(total, dtype=np.uint64), 0, [0] * len(ask)
    for t0, t1 in ((0, 2), (2, 9)):
        part = sa.PackServer(pg, 3, trial0=t0, trial1=t1)
        part.gen_db(41)
        exp = sa.fingerprint_host(KEY, po.p_db, np.ascontiguousarray(pts[:, t0:t1]), 64, s.trials, t0, t1 - t0, per_item=True)[1]
        F, fp = poisoned(sa, part, KEY, 0, total)
        assert (fp == exp).all() and F == FR.combine(KEY, exp, range(total)), f"trials [{t0}, {t1}): its partial sums"
        got_F = sa.fingerprint_add(got_F, F)
        got_f = np.array([sa.fingerprint_add(int(a), int(b)) for a, b in zip(got_f, fp)], dtype=np.uint64)
        fa = poisoned(sa, part, KEY, ids=ask)[1]
        got_at = [sa.fingerprint_add(a, int(b)) for a, b in zip(got_at, fa)]
        part.close()
    assert (got_f == f).all() and got_F == FR.combine(KEY, f, range(total)) and got_at == [int(v) for v in f[ask]]


# ---- 3. crafted content and linearity under update ---------------------------------------------------------------------------------------
def crafted_items(p_db):
    """[all p_db - 1, a single nonzero coefficient at each corner (x4), half - 1 and half alternating, all half, all half - 1]"""
    half = p_db >> 1
    items = np.zeros((8, 4, N), dtype=np.uint64)
    items[0] = p_db - 1
    items[1, 0, 0] = 1
    items[2, 0, N - 1] = p_db - 1
    items[3, 3, 0] = half
    items[4, 3, N - 1] = 1
    items[5, :, 0::2] = half - 1
    items[5, :, 1::2] = half
    items[6] = half
    items[7] = half - 1
    return items.reshape(8, 4 * N)


@pytest.mark.parametrize("nu1,nu2,limbs", [(6, 6, False), (6, 6, True), (6, 4, True), (4, 3, False)])
def test_crafted_items_and_linearity(sa, SV, oracle, opts, nu1, nu2, limbs):
    """crafted items scattered into the image in its current form: their fingerprints at r = P - 2 and at a random key, and
    new F = old F + sum of (f_new - f_old) s^(i + 1), the deltas from fingerprint_host"""
    O = oracle
    kw = dict(t_gsw=8)
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.shape_of(po)
    total, np_ = s.dim0 * s.num_per, s.num_per
    seed = 21 if (nu1, nu2) == (6, 6) else 17
    srv = sa.Server(pg)
    srv.gen_db(seed)
    if limbs:
        opts(sweep_narrow=1)
        srv.set_db_format(SV.DB_LIMBS)
    new = crafted_items(po.p_db)
    ids = [0, total - 1, 5 * np_ + 3, 6 * np_ - 1, (s.dim0 // 2) * np_, 9 * np_ + 1, np_, total // 2 + 5][:len(new)]
    assert len(set(ids)) == len(ids)
    for key in (KEY_TOP, KEY):
        pts, f_old = base_ref(sa, O, po, seed, key)
        old_F = srv.fingerprint_items(key)
        assert old_F == FR.combine(key, f_old, range(total))
        f_new = sa.fingerprint_host(key, po.p_db, new, 64, per_item=True)[1]
        assert int(f_new[1]) == FR.bases(key)[0], "a single 1 at coefficient 0 of polynomial 0: f = r"
        assert int(f_new[4]) == pow(FR.bases(key)[0], 4 * N, P), "a single 1 at the last coefficient: f = r^8192"
        srv.update_db_items(O.pack_items(new.astype(np.uint32), 8), 8, ids)
        Fa, got = srv.fingerprint_items_at(key, ids)
        assert [int(v) for v in got] == [int(v) for v in f_new], f"crafted items, key {key}"
        _, sb = FR.bases(key)
        delta = sum((int(a) - int(b)) * pow(sb, i + 1, P) for a, b, i in zip(f_new, f_old[ids], ids))
        assert srv.fingerprint_items(key) == (old_F + delta) % P, "linearity under update"
        srv.update_db_items(O.pack_items(pts[ids].astype(np.uint32), 8), 8, ids)  # back to the oracle's items
        assert srv.fingerprint_items(key) == old_F
    srv.close()


# ---- 4. form independence, several passes, the existing calls ----------------------------------------------------------------------------
def test_form_independence_passes_and_export(sa, SV, oracle, opts):
    """the same values before and after set_db_format, in both directions; with db_stage_bytes forcing several passes; read_db_items of the image is
    byte-identical before and after the fingerprint calls"""
    O = oracle
    po, pg = O.make_params(6, 6, t_gsw=8), sa.make_params(6, 6, t_gsw=8)
    s = O.shape_of(po)
    total = s.dim0 * s.num_per
    pts, f = base_ref(sa, O, po, 21)
    srv = sa.Server(pg)
    srv.gen_db(21)
    before = srv.read_db_items(8)
    one = srv.fingerprint_items(KEY, per_item=True)
    assert (one[1] == f).all()
    srv.set_db_format(SV.DB_LIMBS)
    two = srv.fingerprint_items(KEY, per_item=True)
    srv.set_db_format(SV.DB_PACKED)
    three = srv.fingerprint_items(KEY, per_item=True)
    assert one[0] == two[0] == three[0] and (one[1] == two[1]).all() and (one[1] == three[1]).all()
    lane, other = sa.Server(pg, share_db_of=srv), sa.Server(pg)
    other.share_db(srv)
    for rd in (lane, other):  # a lane and a share_db server read the owner's image
        assert rd.fingerprint_items(KEY) == one[0] and (rd.fingerprint_items_at(KEY, [total - 1, 5])[1] == f[[total - 1, 5]]).all()
    lane.close()
    other.close()
    ask = list(range(total - 1, 0, -7)) + [5, 5]
    at_one = srv.fingerprint_items_at(KEY, ask)
    for stage, first, n in ((40 * 100, 0, total), (40 * 700 + 3, 131, 2000), (1, 77, 300)):  # passes of 64, 512 and 1 items
        opts(db_stage_bytes=stage)
        F, got = srv.fingerprint_items(KEY, first, n, per_item=True)
        assert (got == f[first:first + n]).all() and F == FR.combine(KEY, f[first:first + n], range(first, first + n)), f"db_stage_bytes = {stage}"
    opts(db_stage_bytes=40 * 100)
    at_many = srv.fingerprint_items_at(KEY, ask)
    assert at_many[0] == at_one[0] == FR.combine(KEY, f[ask], ask) and (at_many[1] == at_one[1]).all()
    opts(db_stage_bytes=64 << 20)
    after = srv.read_db_items(8)
    assert (before == after).all(), "read_db_items after the fingerprint calls"
    assert srv.db_format() == SV.DB_PACKED
    srv.close()


# ---- 5. shards ---------------------------------------------------------------------------------------------------------------------------
POISON = 0x5A5A5A5A5A5A5A5A


def poisoned(sa, srv, key, first=None, n=None, ids=None):
    """the C entry point with a per_item buffer that holds POISON in every word (the Python wrapper hands the library zeros, which would hide a word
    the call does not write) -> (F, per-item values); the wrapper's result must be the same"""
    L = sa.lib()
    U64P = C.POINTER(C.c_uint64)
    pre = "spiral_gpu_pack_server" if isinstance(srv, sa.PackServer) else "spiral_gpu_server"
    k = (C.c_uint64 * 2)(*key)
    comb = C.c_uint64(POISON)
    if ids is None:
        out = np.full(n, POISON, dtype=np.uint64)
        rc = getattr(L, pre + "_fingerprint_items")(srv.h, k, first, n, out.ctypes.data_as(U64P), C.byref(comb))
        want = srv.fingerprint_items(key, first, n, per_item=True)
    else:
        a = np.ascontiguousarray(ids, dtype=np.uint64)
        out = np.full(len(a), POISON, dtype=np.uint64)
        rc = getattr(L, pre + "_fingerprint_items_at")(srv.h, k, a.ctypes.data_as(U64P), len(a), out.ctypes.data_as(U64P), C.byref(comb))
        want = srv.fingerprint_items_at(key, ids)
    assert rc == 0, L.spiral_gpu_last_error()
    bad = np.flatnonzero(out != want[1])
    assert bad.size == 0 and comb.value == want[0], f"into a poisoned buffer: {bad.size} words differ from the wrapper's, first at position {bad[:1]}: {out[bad[:1]]}"
    return int(comb.value), out


def add_all(sa, parts):
    return np.array([sa.fingerprint_add(*[int(p[k]) for p in parts]) for k in range(len(parts[0]))], dtype=np.uint64)


def test_j_shards(sa, SV, oracle):
    """(7, 6) over two j-shards, one in limb planes: zeros for the items of the other shard, partials add to the unsharded values"""
    O = oracle
    po, pg = O.make_params(7, 6, t_gsw=8), sa.make_params(7, 6, t_gsw=8)
    s = O.shape_of(po)
    total, np_ = s.dim0 * s.num_per, s.num_per
    pts, f = base_ref(sa, O, po, 5)
    shards = [sa.Server(pg, j_begin=0, j_end=64), sa.Server(pg, j_begin=64, j_end=128)]
    for sv in shards:
        sv.gen_db(5)
    shards[1].set_db_format(SV.DB_LIMBS)
    half = total // 2
    first, n = 62 * np_ + 7, 4 * np_ + 9  # across the boundary
    ask = [127 * np_ + 63, 3, 64 * np_, 63 * np_ + 63, 100 * np_ + 9, 3, 20 * np_ + 9]
    whole, rng_, at = [], [], []
    for k, sv in enumerate(shards):
        mine = np.zeros(total, dtype=bool)
        mine[k * half:(k + 1) * half] = True
        exp = np.where(mine, f, 0).astype(np.uint64)
        F, got = poisoned(sa, sv, KEY, 0, total)
        assert (got == exp).all() and F == FR.combine(KEY, exp, range(total)), f"shard {k}: whole database"
        whole.append((F, got))
        Fr, got = poisoned(sa, sv, KEY, first, n)
        assert (got == exp[first:first + n]).all(), f"shard {k}: a range across the boundary"
        rng_.append((Fr, got))
        Fa, got = poisoned(sa, sv, KEY, ids=ask)
        assert (got == exp[ask]).all(), f"shard {k}: by id"
        at.append((Fa, got))
        sv.close()
    assert sa.fingerprint_add(*[w[0] for w in whole]) == FR.combine(KEY, f, range(total)) and (add_all(sa, [w[1] for w in whole]) == f).all()
    assert sa.fingerprint_add(*[w[0] for w in rng_]) == FR.combine(KEY, f[first:first + n], range(first, first + n))
    assert sa.fingerprint_add(*[w[0] for w in at]) == FR.combine(KEY, f[ask], ask) and (add_all(sa, [w[1] for w in at]) == f[ask]).all()


@pytest.mark.parametrize("G", [2, 4])
def test_column_shards(sa, SV, oracle, G):
    """(6, 6) over G column shards: rank g holds the items whose column is g mod G, and writes zeros for the others; the partials add up.  Ranges whose
    ends fall on every residue mod G, one of a single item that most ranks do not hold, several passes"""
    O = oracle
    po, pg = O.make_params(6, 6, t_gsw=8), sa.make_params(6, 6, t_gsw=8)
    s = O.shape_of(po)
    total, np_ = s.dim0 * s.num_per, s.num_per
    pts, f = base_ref(sa, O, po, 21)
    ranges = [(0, total), (np_ + 3, 2 * np_ + 5), (np_ + 2, 2 * np_ + 3), (7, 1), (total - 5, 5), (9, 0)]
    ask = [total - 1, 3, 64, 63, 10 * np_ + 9, 3, 20 * np_ + 10, 2]
    got_r, got_at = [[] for _ in ranges], []
    for g in range(G):
        sv = sa.Server(pg, col_rank=g, col_ranks=G)
        sv.gen_db(21)
        exp = np.where(np.arange(total) % G == g, f, 0).astype(np.uint64)
        for k, (first, n) in enumerate(ranges):
            if k == 1:
                sa.set_option("db_stage_bytes", 8 * (4 + G) * 16)  # passes of 16 items
            F, got = poisoned(sa, sv, KEY, first, n)  # (k = 1: several passes, the words between two passes' items included)
            sa.set_option("db_stage_bytes", 64 << 20)
            assert (got == exp[first:first + n]).all() and F == FR.combine(KEY, exp[first:first + n], range(first, first + n)), f"rank {g} of {G}: items [{first}, +{n})"
            assert sv.fingerprint_items(KEY, first, n) == F
            got_r[k].append((F, got))
        Fa, got = poisoned(sa, sv, KEY, ids=ask)
        assert (got == exp[ask]).all() and Fa == FR.combine(KEY, exp[ask], ask), f"rank {g} of {G}: by id"
        got_at.append((Fa, got))
        sv.close()
    for (first, n), parts in zip(ranges, got_r):
        assert sa.fingerprint_add(*[p[0] for p in parts]) == FR.combine(KEY, f[first:first + n], range(first, first + n))
        assert (add_all(sa, [p[1] for p in parts]) == f[first:first + n]).all()
    assert sa.fingerprint_add(*[p[0] for p in got_at]) == FR.combine(KEY, f[ask], ask) and (add_all(sa, [p[1] for p in got_at]) == f[ask]).all()


# ---- 6. failures -------------------------------------------------------------------------------------------------------------------------
def hip_runtime():
    """the HIP runtime this process already has loaded (torch's, which the library shares)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def test_failures(sa, SV, oracle):
    """what is refused before any launch leaves the outputs and db_fingerprint_ns alone; an image without plaintexts is refused with the item named, and
    is untouched: a query on it still gives the oracle's answer"""
    O = oracle
    po, pg = O.make_params(6, 6, t_gsw=8), sa.make_params(6, 6, t_gsw=8)
    s = O.shape_of(po)
    total = s.dim0 * s.num_per
    L = sa.lib()
    U64P = C.POINTER(C.c_uint64)
    key = (C.c_uint64 * 2)(*KEY)
    out, comb = np.full(4, 0x5A5A, dtype=np.uint64), C.c_uint64(0x5A5A)
    outp = out.ctypes.data_as(U64P)
    ids = np.array([3, total], dtype=np.uint64)
    idp = ids.ctypes.data_as(U64P)

    empty = sa.Server(pg)
    with pytest.raises(sa.SpiralGpuError, match="no database loaded"):
        empty.fingerprint_items(KEY)
    with pytest.raises(sa.SpiralGpuError, match="no database loaded"):
        empty.fingerprint_items_at(KEY, [0])
    empty.close()

    srv = sa.Server(pg)
    srv.gen_db(21)
    pts, f = base_ref(sa, O, po, 21)
    assert srv.fingerprint_items(KEY, 0, 8) == FR.combine(KEY, f[:8], range(8))
    ns = sa.get_option("db_fingerprint_ns")
    assert ns > 0
    assert L.spiral_gpu_server_fingerprint_items(srv.h, key, total - 1, 2, outp, C.byref(comb)) != 0 and b"outside" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_server_fingerprint_items(srv.h, key, total + 1, 0, outp, C.byref(comb)) != 0
    assert L.spiral_gpu_server_fingerprint_items_at(srv.h, key, idp, 2, outp, C.byref(comb)) != 0 and b"outside" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_server_fingerprint_items(srv.h, key, 0, 2, None, None) != 0 and b"both null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_server_fingerprint_items_at(srv.h, key, idp, 1, None, None) != 0 and b"both null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_server_fingerprint_items(srv.h, None, 0, 2, outp, C.byref(comb)) != 0
    assert L.spiral_gpu_server_fingerprint_items(None, key, 0, 2, outp, C.byref(comb)) != 0
    assert L.spiral_gpu_server_fingerprint_items_at(srv.h, key, None, 1, outp, C.byref(comb)) != 0
    with pytest.raises(sa.SpiralGpuError, match="outside"):
        srv.fingerprint_items_at(KEY, [total])
    with pytest.raises(ValueError, match="key"):
        srv.fingerprint_items((1, 2, 3))
    # inside a capture
    hip = hip_runtime()
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    srv.set_stream(st.value)
    assert hip.hipStreamBeginCapture(st, 2) == 0  # (hipStreamCaptureModeRelaxed)
    try:
        assert L.spiral_gpu_server_fingerprint_items(srv.h, key, 0, 2, outp, C.byref(comb)) != 0 and b"captured" in L.spiral_gpu_last_error()
        assert L.spiral_gpu_server_fingerprint_items_at(srv.h, key, idp, 1, outp, C.byref(comb)) != 0 and b"captured" in L.spiral_gpu_last_error()
    finally:
        g = C.c_void_p()
        assert hip.hipStreamEndCapture(st, C.byref(g)) == 0
        if g.value:
            hip.hipGraphDestroy(g)
    srv.set_stream(0)
    hip.hipStreamDestroy(st)
    assert (out == 0x5A5A).all() and comb.value == 0x5A5A, "a refused call wrote nothing"
    assert sa.get_option("db_fingerprint_ns") == ns, "a refused call launched nothing"

    # not a plaintext image
    cl = O.Client(po, seed=9)
    pp = cl.pub_params()
    q = cl.query(700)
    srv.set_pub_params(*pp)
    for fmt in (SV.DB_PACKED, SV.DB_LIMBS):
        srv.fill_db_random(7)
        if fmt == SV.DB_LIMBS:
            srv.set_db_format(SV.DB_LIMBS)
        image = srv.read_db_slots(0, N)
        with pytest.raises(sa.SpiralGpuError, match=r"plaintext at item 0 \(polynomial 0, coefficient 0 "):
            srv.fingerprint_items(KEY)
        with pytest.raises(sa.SpiralGpuError, match=rf"plaintext at item {total - 3} "):
            srv.fingerprint_items_at(KEY, [total - 3, 4])
        with pytest.raises(sa.SpiralGpuError, match=r"plaintext at item 77 "):
            srv.fingerprint_items(KEY, 77, 9, per_item=True)
        assert srv.db_format() == fmt and (srv.read_db_slots(0, N) == image).all(), "the image is untouched"
        fin, _, _ = srv.answer(q)
        assert (fin == O.answer(po, q, *pp, image.reshape(-1))).all(), "a query on the random image after the refused calls"
    srv.gen_db(21)
    assert srv.fingerprint_items(KEY) == FR.combine(KEY, f, range(total)), "after the database is loaded again"
    srv.close()


def test_pack_failures(sa, PK, oracle_mt):
    O = oracle_mt
    po, pg = O.make_params(6, 2), sa.make_params(6, 2)
    s = O.pack_shape_of(po, 2)
    total = s.dim0 * s.num_per
    srv = sa.PackServer(pg, 2)
    with pytest.raises(sa.SpiralGpuError, match="no database loaded"):
        srv.fingerprint_items(KEY)
    srv.fill_db_random(3)
    with pytest.raises(sa.SpiralGpuError, match=r"plaintext at item 0 \(polynomial 0, "):
        srv.fingerprint_items(KEY)
    with pytest.raises(sa.SpiralGpuError, match=r"plaintext at item 9 "):
        srv.fingerprint_items_at(KEY, [9, 2])
    srv.gen_db(41)
    with pytest.raises(sa.SpiralGpuError, match="outside"):
        srv.fingerprint_items(KEY, total - 1, 2)
    with pytest.raises(sa.SpiralGpuError, match="outside"):
        srv.fingerprint_items_at(KEY, [0, total])
    pts, f = pack_ref(sa, O, po, 2, 41)
    assert srv.fingerprint_items(KEY) == FR.combine(KEY, f, range(total)), "after the failures"
    srv.close()
