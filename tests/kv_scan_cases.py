"""What the GPU tests of the listing (tests/test_gpu_kv_scan.py, tests/test_gpu_pack_kv_scan.py) share: the crafted table, on the model's side only, and
the checks of one server against the restatement (tests/kv_scan_restated.py).  Expected listings come from the restated table; nothing expected comes
from the code under test."""
import ctypes as C

import numpy as np
import pytest

import kv_restated as K
import kv_scan_restated as KS

TK = K.TABLE_KEY
FP_KEY = (0x0123456789ABCDEF, 0x0FEDCBA987654321)


def assert_eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp) if got.shape == exp.shape else []
        raise AssertionError(f"{what}: shapes {got.shape} / {exp.shape}, {len(bad)} of {got.size} differ, first at {bad[:5].tolist() if len(bad) else '-'}")


def crafted_table(lay, n, seed):
    """The model's side of one case, no device involved.  kv_load of key_set(n); then one bucket is FILLED by hand with further keys that have it as a
    candidate (two-choice placement keeps a table at this load balanced: no load and no delete leaves a full bucket of 32 or more slots, so the
    bucket's item is written with load_db_items -- the entries are ones a lookup finds); then a crafted delete empties one bucket and leaves another
    with its highest used slot as its only entry.  Returns a dict: keys / vals (the kv_load), fill_bucket and its stream row, every key stored, gone,
    the model after all of it, and the three buckets -- asserted here, so the inputs are known to contain them."""
    rng = np.random.default_rng(seed)
    V, nb, slots = lay.value_bytes, lay.buckets, lay.slots
    keys, vals = K.key_set(n), rng.integers(0, 256, size=(n, V), dtype=np.uint8)
    model = K.Table(lay, TK)
    model.load(K.key_array(keys), vals)  # (raises Full where the rule does not place every key)
    used = (model.tags != 0).sum(axis=1)
    full = int(used.argmax())
    extra = K.key_set(60_000, n + 1000)
    tag, b1, b2 = K.kv_hash_many(nb, TK, K.key_array(extra))
    stored = list(keys)
    for i in np.flatnonzero((b1 == full) | (b2 == full)):
        free = np.flatnonzero(model.tags[full] == 0)
        if not len(free):
            break
        model.tags[full, free[0]] = tag[i]
        model.vals[full, free[0]] = rng.integers(0, 256, size=V, dtype=np.uint8)
        stored.append(extra[i])
    loaded = model.stream()[full].copy()
    key_of_tag = dict(zip(K.kv_hash_many(nb, TK, K.key_array(stored))[0].tolist(), stored))
    used = (model.tags != 0).sum(axis=1)
    order = [int(b) for b in np.argsort(used, kind="stable") if b != full and used[b] > 0]
    empty = order[0]  # every key of the least used bucket goes
    last = next(b for b in order[1:] if used[b] >= min(2, slots))  # every key but the one in the highest used slot goes
    top = int(np.flatnonzero(model.tags[last])[-1])
    gone = [key_of_tag[int(t)] for t in model.tags[empty][model.tags[empty] != 0]]
    gone += [key_of_tag[int(t)] for s, t in enumerate(model.tags[last]) if t != 0 and s != top]
    gone += [k for k in keys[7:12] if k not in gone and model.find(k)[1] not in (full, last)] + K.key_set(2, n + 900_000)  # some others, and two keys that were never there
    n_gone = model.delete(gone)
    assert n_gone == len(gone) - 2
    used = (model.tags != 0).sum(axis=1)
    assert used[empty] == 0, "an empty bucket"
    assert used[last] == 1 and model.tags[last, top] != 0 and (top > 0 or slots == 1), "a bucket whose only entry is its highest used slot"
    assert used[full] == slots, "a full bucket"
    gone_set = set(gone)
    kept = [k for k in stored if k not in gone_set]
    return dict(keys=keys, vals=vals, fill_bucket=full, fill_stream=loaded, stored=stored, kept=kept, gone=gone, n_gone=n_gone, model=model, empty=empty, last=last, full=full)


def scan_into(srv, V, want, values, first=None, cnt=None, ids=None, spare=3):
    """one kv_scan / kv_scan_at with max_entries = the expected count + spare into buffers prefilled with 0xEE; the rows beyond the listing must stay 0xEE"""
    from spiral_amd import _lib

    room = len(want[0]) + spare
    ent = np.frombuffer(np.full(16 * room, 0xEE, dtype=np.uint8), dtype=_lib.KV_ENTRY_DTYPE).copy()
    val = np.full((room, V), 0xEE, dtype=np.uint8) if values else None
    got = srv.kv_scan_at(V, ids, values, room, out_entries=ent, out_values=val) if ids is not None else srv.kv_scan(V, first, cnt, values, room, out_entries=ent, out_values=val)
    assert (ent[len(got):].view(np.uint8) == 0xEE).all() and (val is None or (val[len(got):] == 0xEE).all()), "nothing is written beyond the listing"
    return got


def check_scan(got, want, values, what):
    assert_eq(got.tags, want[0], f"{what}: tags")
    assert_eq(got.buckets, want[1], f"{what}: buckets")
    assert_eq(got.slots, want[2], f"{what}: slots")
    assert (got.tags.dtype, got.buckets.dtype, got.slots.dtype) == (np.uint64, np.uint32, np.uint32)
    if values:
        assert_eq(got.values, want[3], f"{what}: values")
    else:
        assert got.values is None


def at_list(plan, nb, rng):
    """a shuffled list of buckets that names one bucket twice and includes the empty, the full and the one-entry bucket, bucket 0 and the last"""
    ids = {plan["empty"], plan["full"], plan["last"], 0, nb - 1} | set(rng.choice(nb, size=min(9, nb), replace=False).tolist())
    ids = rng.permutation(sorted(ids)).tolist()
    return ids + [ids[2]]


def check_listings(sa, opts, srv, plan, V, what, chunk, seed=0):
    """tags-only and with-values listings of the whole table, of [5, 5 + 17), of [nb - 1, nb), of an empty range and of a list against the restatement:
    with the automatic pass, with option kv_scan_chunk = chunk (several passes, range ends inside a pass), and with db_stage_bytes so small that the
    value read takes several passes"""
    model = plan["model"]
    nb = model.lay.buckets
    ranges = [(0, nb), (5, 17), (nb - 1, 1), (7, 0), (nb, 0)]
    ids = at_list(plan, nb, np.random.default_rng(seed))
    assert len(set(ids)) == len(ids) - 1 and plan["empty"] in ids
    saved = sa.get_option("db_stage_bytes")
    for mode in ("auto", "chunk", "stage"):
        if mode == "chunk":
            opts(kv_scan_chunk=chunk)
            assert nb // chunk >= 4 and (nb % chunk or chunk == 1), "several passes, the last one shorter"
        for values in (False, True):
            for first, cnt in ranges:
                want = KS.listing(model, first, cnt)
                if mode == "stage":
                    opts(db_stage_bytes=V * max(2, len(want[0]) // 3))
                got = scan_into(srv, V, want, values, first, cnt)
                check_scan(got, want, values, f"{what} {mode} [{first}, +{cnt}) values={values}")
                assert (got.first_bucket, got.n_buckets, got.table_buckets) == (first, cnt, nb)
            want = KS.listing_at(model, ids)
            if mode == "stage":
                opts(db_stage_bytes=V * max(2, len(want[0]) // 3))
            got = scan_into(srv, V, want, values, ids=ids)
            check_scan(got, want, values, f"{what} {mode} kv_scan_at values={values}")
            assert (got.first_bucket, got.n_buckets, got.table_buckets) == (None, None, nb)
        if mode == "stage":
            opts(db_stage_bytes=saved)
    opts(kv_scan_chunk=0)
    # max_entries=None: a count-only call first, then exactly that many
    want = KS.listing(model)
    check_scan(srv.kv_scan(V), want, True, f"{what}: the default call")
    check_scan(srv.kv_scan_at(V, ids, values=False), KS.listing_at(model, ids), False, f"{what}: the default kv_scan_at")
    assert len(srv.kv_scan_at(V, [])) == 0


def check_counts_and_overflow(sa, srv, fn, plan, V, what):
    """count-only equals kv_stats(...).used and the model's count; max_entries = count succeeds; max_entries = count - 1 fails with the count reported
    and every byte of both buffers still 0xEE.  fn: the C call (spiral_gpu_server_kv_scan or its SpiralPack twin)"""
    from spiral_amd import _lib

    model = plan["model"]
    nb = model.lay.buckets
    L = sa.lib()
    for first, cnt in ((0, nb), (5, 17), (nb - 1, 1), (nb, 0)):
        want = KS.listing(model, first, cnt)
        n = C.c_uint64(12345)
        assert fn(srv.h, V, first, cnt, None, None, 0, C.byref(n)) == 0, L.spiral_gpu_last_error()
        assert n.value == len(want[0]) == srv.kv_stats(V, first, cnt).used, f"{what}: count-only [{first}, +{cnt})"
    want = KS.listing(model, 5, 17)
    count = len(want[0])
    assert count >= 2
    got = scan_into(srv, V, want, True, 5, 17, spare=0)  # max_entries = count
    check_scan(got, want, True, f"{what}: max_entries = count")
    ent = np.frombuffer(np.full(16 * count, 0xEE, dtype=np.uint8), dtype=_lib.KV_ENTRY_DTYPE).copy()
    val = np.full((count, V), 0xEE, dtype=np.uint8)
    with pytest.raises(sa.KvScanOverflow, match=rf"hold {count} entries, max_entries is {count - 1}") as e:
        srv.kv_scan(V, 5, 17, True, count - 1, out_entries=ent, out_values=val)
    assert e.value.count == count and e.value.max_entries == count - 1
    assert (ent.view(np.uint8) == 0xEE).all() and (val == 0xEE).all(), f"{what}: not one byte of entries or values is written on overflow"
    n = C.c_uint64(0)
    assert fn(srv.h, V, 5, 17, None, val.ctypes.data_as(C.c_void_p), count, C.byref(n)) != 0 and b"entries is NULL" in L.spiral_gpu_last_error()
    assert (val == 0xEE).all()
    with pytest.raises(sa.SpiralGpuError, match="outside the table"):
        srv.kv_scan(V, nb - 3, 4)
    with pytest.raises(sa.SpiralGpuError, match="outside the table"):
        srv.kv_scan(V, nb + 1, 0)
    with pytest.raises(sa.SpiralGpuError, match=rf"bucket {nb} at position 2 outside the table of {nb}"):
        srv.kv_scan_at(V, [0, nb - 1, nb, nb + 5])


def check_reconcile(sa, pg, srv, plan, V, what):
    """end to end: kv_reconcile of the GPU's listing against every key stored gives no missing key other than the deleted ones, and no orphan"""
    stored, gone = plan["stored"], set(plan["gone"])
    r = sa.kv_reconcile(pg, TK, stored, srv.kv_scan(V, values=False))
    assert sorted(stored[k] for k in r.missing_keys()) == sorted(k for k in stored if k in gone), f"{what}: the missing keys are the deleted ones"
    assert (r.orphans, r.shadowed, r.misplaced, r.held, r.missing) == (0, 0, 0, len(plan["kept"]), len(stored) - len(plan["kept"])), what
    if len(stored) <= 10_000:  # (the restatement hashes key by key in plain Python)
        want = KS.reconcile(plan["model"].lay.buckets, TK, stored, *KS.listing(plan["model"])[:3])
        assert_eq(r.where, want[0], f"{what}: where")
        assert_eq(r.entry_class, want[1], f"{what}: entry_class")
