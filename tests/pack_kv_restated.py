"""Keyed records on SpiralPack servers (include/spiral_gpu.h "Keyed records", SpiralPack) restated for the tests: the layout for out_n, and the
per-trial streams of a model table.  Hash, placement and the model table are those of tests/kv_restated.py (the definition says "word for word"),
the item stream and its trial polynomials those of tests/pack_records_restated.py.  Nothing here calls the library under test."""
import numpy as np

import kv_restated as K
import pack_records_restated as PR

N = 2048
TABLE_KEY = K.TABLE_KEY
key_set, key_array = K.key_set, K.key_array

# (keys, buckets, slots) of every table the GPU tests load with key_set(n) under TABLE_KEY; tests/test_pack_kv_cpu.py shows that the restated
# placement places every key of each one and finds no equal tags.
PACK_KEY_SETS = [(1536, 64, 32), (32, 64, 2), (2256, 64, 47), (49152, 2048, 32), (1024, 2048, 2), (55296, 1024, 72), (3072, 1024, 6), (768, 1024, 3)]


def load_size(lay) -> int:
    """0.75 of the capacity; 0.5 at 6 slots (0.75 at 1024 x 6 overflows at key 4336); 0.25 at 2 and 3 slots (few slots per bucket overflow early)"""
    if lay.slots in (2, 3):
        return lay.capacity // 4
    if lay.slots == 6:
        return lay.capacity // 2
    return lay.capacity * 3 // 4


def layout(p_db: int, nu1: int, nu2: int, out_n: int, value_bytes: int):
    """the layout (a kv_restated.Layout), or the reason it is refused (a string)"""
    if not 1 <= out_n <= 16:
        return "out_n"
    w = p_db.bit_length() - 1
    item_bytes, nb = out_n * out_n * 256 * w, 1 << (nu1 + nu2)
    if value_bytes < 1:
        return "value"
    slots = item_bytes // (8 + value_bytes)
    if slots == 0:
        return "slots = 0"
    if slots > 256:
        return "slots > 256"
    if 8 * slots > 256 * w:
        return "header"
    if nb < 2:
        return "buckets"
    return K.Layout(w, slots, value_bytes, item_bytes, nb, nb * slots)


def trial_streams(stream: np.ndarray, lay, out_n: int, bits: int | None = None):
    """a table's stream [buckets][item_bytes] as what read_db_items(trial = t, bits) of each trial returns: a list of [buckets][256 bits] arrays,
    polynomial t of bucket b = item b of trial t (bits: the width read at, default w)"""
    w, trials = lay.coeff_bits, out_n * out_n
    pb = 256 * w
    if bits is None or bits == w:
        return [np.ascontiguousarray(stream[:, t * pb:(t + 1) * pb]) for t in range(trials)]
    coeffs = PR.stream_coeffs(stream, w, trials)  # [bucket][trial][2048]
    return [np.stack([PR.stream_of(coeffs[b, t], bits) for b in range(len(coeffs))]) for t in range(trials)]


def value_polys(lay, slot: int) -> range:
    """the polynomials (trials) that hold a byte of slot `slot`'s value"""
    pb = 256 * lay.coeff_bits
    v0 = 8 * lay.slots + slot * lay.value_bytes
    return range(v0 // pb, -(-(v0 + lay.value_bytes) // pb))


def scan(lay, plaintext, tag: int):
    """the header scan and value cut on one decoded SpiralPack plaintext [out_n][out_n][2048] (polynomial t at (t // out_n, t % out_n)): the value
    bytes of the lowest slot whose tag is `tag`, or None"""
    w = lay.coeff_bits
    coeffs = np.asarray(plaintext).reshape(-1, N)
    header = PR.cut(coeffs, w, 0, 8 * lay.slots).view("<u8")
    hit = np.flatnonzero(header == np.uint64(tag))
    if not len(hit):
        return None
    return PR.cut(coeffs, w, 8 * lay.slots + int(hit[0]) * lay.value_bytes, lay.value_bytes)


def find_in(lay, plain1, plain2, tag: int):
    """(value bytes or zeros, found) from the two candidates' plaintexts: candidate 1 wins"""
    for c, pt in ((1, plain1), (2, plain2)):
        v = scan(lay, pt, tag)
        if v is not None:
            return v, c
    return np.zeros(lay.value_bytes, dtype=np.uint8), 0


def stats_of(tags: np.ndarray, first: int = 0, n: int | None = None):
    """(buckets, used, full_buckets, max_used, hist[257]) of buckets [first, first + n) of a model table's tags [buckets][slots]"""
    slots = tags.shape[1]
    part = tags[first:] if n is None else tags[first:first + n]
    used = (part != 0).sum(axis=1)
    hist = np.bincount(used, minlength=257).tolist()
    return len(part), int(used.sum()), int((used == slots).sum()), int(used.max()) if len(part) else 0, hist
