"""Listing (include/spiral_gpu.h "Listing") restated in plain Python / numpy for the tests, on a kv_restated.Table.  An ENTRY is a slot whose tag is
not 0, reported as (tag, bucket, slot); a LISTING of a set of buckets is all their entries, in the order of the buckets, and within a bucket by
ascending slot; with values, row k is the value of entry k.  reconcile: where[k] is the entry a lookup of key k finds (b1 first, the lowest slot) or
-1; an entry is 0 held (some key's where), 1 shadowed (a key's tag in one of its candidate buckets, but a lookup finds another entry first), 2
misplaced (a key's tag in a bucket that is neither of its candidates), 3 orphan (the tag of no key given).  Nothing here calls the library under test."""
import numpy as np

import kv_restated as K

HELD, SHADOWED, MISPLACED, ORPHAN = 0, 1, 2, 3


def listing(table, first=0, n=None):
    """(tags, buckets, slots, values) of buckets [first, first + n): np.nonzero of the tags is bucket-major, slots ascending"""
    n = table.lay.buckets - first if n is None else n
    b, s = np.nonzero(table.tags[first:first + n])
    b = b + first
    return table.tags[b, s], b.astype(np.uint32), s.astype(np.uint32), table.vals[b, s].reshape(len(b), table.lay.value_bytes)


def listing_at(table, ids):
    """the same for a list of buckets, in the order of the list; a bucket named twice is listed twice"""
    parts = [listing(table, int(i), 1) for i in ids]
    if not parts:
        return listing(table, 0, 0)
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(4))


def reconcile(nb, table_key, keys, tags, buckets, slots):
    """(where [n_keys], entry_class [n_entries], counts dict) of a whole table's listing against `keys` (a list of bytes)"""
    entries = list(zip((int(t) for t in tags), (int(b) for b in buckets), (int(s) for s in slots)))
    by_bucket = {}
    for e, (t, b, s) in enumerate(entries):
        by_bucket.setdefault(b, []).append((s, t, e))
    hashes = [K.kv_hash(nb, table_key, bytes(k)) for k in keys]
    where = []
    for tag, b1, b2 in hashes:
        found = -1
        for b in (b1, b2):
            hit = [e for s, t, e in sorted(by_bucket.get(b, [])) if t == tag]
            if hit:
                found = hit[0]
                break
        where.append(found)
    key_of_tag = {tag: k for k, (tag, _, _) in enumerate(hashes)}
    assert len(key_of_tag) == len(hashes), "the keys' tags are distinct"
    held = set(w for w in where if w >= 0)
    cls = []
    for e, (t, b, s) in enumerate(entries):
        if t not in key_of_tag:
            cls.append(ORPHAN)
        elif e in held:
            cls.append(HELD)
        elif b in hashes[key_of_tag[t]][1:]:
            cls.append(SHADOWED)
        else:
            cls.append(MISPLACED)
    counts = dict(held=cls.count(HELD), missing=where.count(-1), shadowed=cls.count(SHADOWED), misplaced=cls.count(MISPLACED), orphans=cls.count(ORPHAN))
    return np.array(where, dtype=np.int64), np.array(cls, dtype=np.uint8), counts
