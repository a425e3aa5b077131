"""CPU-side checks of the listing of keyed tables (include/spiral_gpu.h "Listing"): the new symbols and the entry's size, option kv_scan_chunk, and
spiral_gpu_kv_reconcile -- host only -- against the restatement (tests/kv_scan_restated.py) on listings made from restated tables, with its refusals
by position.  Nothing expected comes from the code under test."""
import ctypes as C

import numpy as np
import pytest

import kv_restated as K
import kv_scan_restated as KS

NEW_SYMBOLS = ["spiral_gpu_server_kv_scan", "spiral_gpu_server_kv_scan_at", "spiral_gpu_pack_server_kv_scan", "spiral_gpu_pack_server_kv_scan_at",
               "spiral_gpu_kv_reconcile"]
TK = K.TABLE_KEY


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def test_new_symbols_exported_and_declared(sa):
    from spiral_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
    header = open(_lib.os.path.join(_lib.HERE, "..", "include", "spiral_gpu.h")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
    assert "typedef struct spiral_gpu_kv_entry" in header and "typedef struct spiral_gpu_kv_reconcile_counts" in header
    assert C.sizeof(_lib.KvEntry) == 16 == _lib.KV_ENTRY_DTYPE.itemsize, "sizeof(spiral_gpu_kv_entry) == 16"
    assert [(_lib.KV_ENTRY_DTYPE.fields[n][1], getattr(_lib.KvEntry, n).offset) for n in ("tag", "bucket", "slot")] == [(0, 0), (8, 8), (12, 12)]
    assert C.sizeof(_lib.KvReconcileCounts) == 40
    for name in ("KvScan", "KvReconcile", "kv_reconcile", "KvScanOverflow"):
        assert hasattr(sa, name), name
    for cls in (sa.Server, sa.PackServer):
        assert callable(cls.kv_scan) and callable(cls.kv_scan_at)


def test_option_kv_scan_chunk(sa):
    assert sa.get_option("kv_scan_chunk") == 0, "the default is automatic"
    try:
        for v in (1, 65536, 3, 0):
            sa.set_option("kv_scan_chunk", v)
            assert sa.get_option("kv_scan_chunk") == v
        sa.set_option("kv_scan_chunk", 1000)
        for bad in (65537, -1, 1 << 40):
            with pytest.raises(sa.SpiralGpuError, match="out of range"):
                sa.set_option("kv_scan_chunk", bad)
            assert sa.get_option("kv_scan_chunk") == 1000, "a refused value leaves the option unchanged"
    finally:
        sa.set_option("kv_scan_chunk", 0)


def entries_of(sa, tags, buckets, slots):
    from spiral_amd import _lib

    ent = np.empty(len(tags), dtype=_lib.KV_ENTRY_DTYPE)
    ent["tag"], ent["bucket"], ent["slot"] = tags, buckets, slots
    return ent


def c_reconcile(sa, pg, keys, ent, table_key=TK):
    """the C call on a key list and a structured entry array: (rc, where, entry_class, counts dict)"""
    from spiral_amd import _lib

    L = sa.lib()
    ka = K.key_array(keys) if keys else np.zeros((0, 12), dtype=np.uint8)
    tk = np.frombuffer(table_key, dtype=np.uint8)
    where, cls, ct = np.full(len(keys), -7, dtype=np.int64), np.full(len(ent), 0xEE, dtype=np.uint8), _lib.KvReconcileCounts()
    rc = L.spiral_gpu_kv_reconcile(C.byref(pg), tk.ctypes.data_as(C.c_void_p), ka.ctypes.data_as(C.c_void_p), ka.shape[1], len(keys), ent.ctypes.data_as(C.c_void_p),
                                   len(ent), where.ctypes.data_as(C.c_void_p), cls.ctypes.data_as(C.c_void_p), C.byref(ct))
    return rc, where, cls, {n: int(getattr(ct, n)) for n in ("held", "missing", "shadowed", "misplaced", "orphans")}


def plant(table, bucket, tag, highest=False):
    """write `tag` into a free slot of `bucket` of the model's tags: the lowest free one, or the highest"""
    free = np.flatnonzero(table.tags[bucket] == 0)
    assert len(free), "the bucket has room"
    table.tags[bucket, free[-1] if highest else free[0]] = np.uint64(tag)


GEOMS = [("32-slots", dict(t_gsw=4), 248, 32), ("47-slots", dict(t_gsw=4, p_db=32), 99, 47), ("2-slots", dict(t_gsw=4), 3000, 2)]


@pytest.mark.parametrize("name,kw,V,slots", GEOMS, ids=[g[0] for g in GEOMS])
def test_reconcile_equals_the_restatement(sa, name, kw, V, slots):
    """nb = 32.  An untouched table: all held, none missing.  Then keys deleted (missing); a key's tag planted in its b2 while b1 holds it, and in b1
    again at a higher slot (shadowed); a key's tag planted in a bucket that is neither candidate, once for a present key and once for a deleted one
    (misplaced: no lookup reaches it); a foreign tag (orphan).  where, entry_class and the counts equal the restatement element for element."""
    pg = sa.make_params(3, 2, **kw)
    lay = K.layout(int(pg.p_db), 3, 2, V)
    assert (lay.buckets, lay.slots) == (32, slots)
    n = K.load_size(lay)
    keys = K.key_set(n)
    table = K.Table(lay, TK)
    table.load(K.key_array(keys), np.zeros((n, V), dtype=np.uint8))
    nb = lay.buckets

    def both(what, want_counts=None):
        tags, buckets, slots_, _ = KS.listing(table)
        want_w, want_c, want_n = KS.reconcile(nb, TK, keys, tags, buckets, slots_)
        rc, where, cls, counts = c_reconcile(sa, pg, keys, entries_of(sa, tags, buckets, slots_))
        assert rc == 0, sa.lib().spiral_gpu_last_error()
        assert np.array_equal(where, want_w), f"{name} {what}: where"
        assert np.array_equal(cls, want_c), f"{name} {what}: entry_class"
        assert counts == want_n, f"{name} {what}: counts"
        assert counts["held"] + counts["missing"] == n and sum(counts[k] for k in ("held", "shadowed", "misplaced", "orphans")) == len(tags)
        if want_counts is not None:
            assert counts == want_counts, f"{name} {what}: the case is the one described"
        # the Python wrapper on the same listing
        r = sa.kv_reconcile(pg, TK, keys, sa.KvScan(tags, buckets, slots_, None, 0, nb, nb))
        assert np.array_equal(r.where, want_w) and np.array_equal(r.entry_class, want_c)
        assert dict(held=r.held, missing=r.missing, shadowed=r.shadowed, misplaced=r.misplaced, orphans=r.orphans) == want_n
        assert np.array_equal(r.missing_keys(), np.flatnonzero(want_w < 0)) and np.array_equal(r.orphan_entries(), np.flatnonzero(want_c == KS.ORPHAN))
        assert np.array_equal(r.misplaced_entries(), np.flatnonzero(want_c == KS.MISPLACED))
        return where, cls

    both("untouched", dict(held=n, missing=0, shadowed=0, misplaced=0, orphans=0))
    gone = keys[3:6]
    assert table.delete(gone) == 3
    where, _ = both("deleted", dict(held=n - 3, missing=3, shadowed=0, misplaced=0, orphans=0))
    assert where[3:6].tolist() == [-1, -1, -1]
    room = lambda b: (table.tags[b] == 0).any()
    # shadowed: in b2 while b1 holds it, and in b1 again above the held slot
    k_sh = next(k for k in keys[6:] if table.find(k)[0] == 1 and room(table.hash(k)[2]))
    plant(table, table.hash(k_sh)[2], table.hash(k_sh)[0])
    k_sh2 = next(k for k in keys[6:] if k != k_sh and table.find(k)[0] == 1 and np.flatnonzero(table.tags[table.hash(k)[1]] == 0).max(initial=-1) > table.find(k)[2])
    plant(table, table.hash(k_sh2)[1], table.hash(k_sh2)[0], highest=True)
    both("shadowed", dict(held=n - 3, missing=3, shadowed=2, misplaced=0, orphans=0))
    # misplaced: a present key's tag, and a deleted key's tag, each in a bucket that is neither of the key's candidates
    k_mp = next(k for k in keys[6:] if k not in (k_sh, k_sh2))
    for k in (k_mp, gone[0]):
        tag, b1, b2 = table.hash(k)
        plant(table, next(b for b in range(nb) if b not in (b1, b2) and room(b)), tag)
    where, _ = both("misplaced", dict(held=n - 3, missing=3, shadowed=2, misplaced=2, orphans=0))
    assert where[3] == -1, "no lookup reaches a misplaced entry"
    # orphan: the tag of a key that is not given
    foreign = K.kv_hash(nb, TK, b"key-99999999")[0]
    plant(table, next(b for b in range(nb) if room(b)), foreign)
    both("orphan", dict(held=n - 3, missing=3, shadowed=2, misplaced=2, orphans=1))


def test_reconcile_refusals_by_position(sa):
    pg = sa.make_params(3, 2, t_gsw=4)
    lay = K.layout(256, 3, 2, 248)
    keys = K.key_set(40)
    table = K.Table(lay, TK)
    table.load(K.key_array(keys), np.zeros((40, 248), dtype=np.uint8))
    tags, buckets, slots, _ = KS.listing(table)
    good = entries_of(sa, tags, buckets, slots)
    err = lambda: sa.lib().spiral_gpu_last_error().decode()

    def refused(ent, keys_, match):
        rc, where, cls, counts = c_reconcile(sa, pg, keys_, ent)
        assert rc != 0 and match in err(), (match, err())
        assert (where == -7).all() and (cls == 0xEE).all() and not any(counts.values()), "a refused call writes nothing"

    assert c_reconcile(sa, pg, keys, good)[0] == 0
    swapped = good.copy()
    swapped[[6, 7]] = swapped[[7, 6]]
    refused(swapped, keys, "entry 7 ")  # out of order
    twice = np.concatenate([good[:10], good[9:]])
    refused(twice, keys, "entry 10 ")  # a repeated (bucket, slot)
    zero = good.copy()
    zero["tag"][12] = 0
    refused(zero, keys, "entry 12 has tag 0")
    far = good.copy()
    far["bucket"][-1] = 32
    refused(far, keys, f"entry {len(good) - 1} names bucket 32 outside the table of 32")
    refused(good, keys[:5] + keys[2:3] + keys[5:], "keys 2 and 5 have equal tags")  # the same key given twice
    # an empty listing and an empty key set are fine
    rc, where, cls, counts = c_reconcile(sa, pg, keys, good[:0])
    assert rc == 0 and (where == -1).all() and counts == dict(held=0, missing=40, shadowed=0, misplaced=0, orphans=0)
    rc, where, cls, counts = c_reconcile(sa, pg, [], good)
    assert rc == 0 and (cls == 3).all() and counts == dict(held=0, missing=0, shadowed=0, misplaced=0, orphans=len(good))
    L = sa.lib()
    assert L.spiral_gpu_kv_reconcile(None, None, None, 0, 0, None, 0, None, None, None) != 0 and b"null" in L.spiral_gpu_last_error()


def test_python_reconcile_refuses_a_partial_listing(sa):
    pg = sa.make_params(3, 2, t_gsw=4)
    e = np.zeros(0, dtype=np.uint64)
    e32 = np.zeros(0, dtype=np.uint32)
    with pytest.raises(sa.SpiralGpuError, match=r"whole table, buckets \[0, 32\).*\[5, \+17\)"):
        sa.kv_reconcile(pg, TK, K.key_set(3), sa.KvScan(e, e32, e32, None, 5, 17, 32))
    with pytest.raises(sa.SpiralGpuError, match="whole table"):
        sa.kv_reconcile(pg, TK, K.key_set(3), sa.KvScan(e, e32, e32, None, 0, 31, 32))
    with pytest.raises(sa.SpiralGpuError, match="kv_scan_at"):
        sa.kv_reconcile(pg, TK, K.key_set(3), sa.KvScan(e, e32, e32, None, None, None, 32))
    r = sa.kv_reconcile(pg, TK, K.key_set(3), sa.KvScan(e, e32, e32, None, 0, 32, 32))
    assert r.where.tolist() == [-1, -1, -1] and r.missing == 3 and len(r.entry_class) == 0


def test_null_handles_fail_with_a_message(sa):
    L = sa.lib()
    buf = np.full(4096, 0xA5, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    n = C.c_uint64(9)
    for rc in (L.spiral_gpu_server_kv_scan(None, 248, 0, 1, p, p, 4, C.byref(n)), L.spiral_gpu_server_kv_scan_at(None, 248, p, 1, p, p, 4, C.byref(n)),
               L.spiral_gpu_pack_server_kv_scan(None, 248, 0, 1, p, p, 4, C.byref(n)), L.spiral_gpu_pack_server_kv_scan_at(None, 248, p, 1, p, p, 4, C.byref(n))):
        assert rc != 0 and b"null" in L.spiral_gpu_last_error()
    assert (buf == 0xA5).all() and n.value == 9, "nothing written"
