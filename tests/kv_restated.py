"""Keyed records (include/spiral_gpu.h "Keyed records") restated in plain Python / numpy for the tests: SipHash-2-4, the candidate buckets, the
layout, the placement rule, and a model table that builds the item stream and cuts headers and values out of plaintexts.  Nothing here calls the
library under test."""
from dataclasses import dataclass

import numpy as np

import records_restated as R

N = 2048
M64 = (1 << 64) - 1


def _rotl(x, b):
    return ((x << b) | (x >> (64 - b))) & M64


def siphash24(k0: int, k1: int, msg: bytes) -> int:
    """SipHash-2-4, 64-bit output (the public algorithm: c = 2, d = 4)"""
    v0, v1, v2, v3 = k0 ^ 0x736F6D6570736575, k1 ^ 0x646F72616E646F6D, k0 ^ 0x6C7967656E657261, k1 ^ 0x7465646279746573

    def rounds(n, v0, v1, v2, v3):
        for _ in range(n):
            v0 = (v0 + v1) & M64
            v1 = _rotl(v1, 13) ^ v0
            v0 = _rotl(v0, 32)
            v2 = (v2 + v3) & M64
            v3 = _rotl(v3, 16) ^ v2
            v0 = (v0 + v3) & M64
            v3 = _rotl(v3, 21) ^ v0
            v2 = (v2 + v1) & M64
            v1 = _rotl(v1, 17) ^ v2
            v2 = _rotl(v2, 32)
        return v0, v1, v2, v3

    full = len(msg) // 8 * 8
    for i in range(0, full, 8):
        m = int.from_bytes(msg[i:i + 8], "little")
        v3 ^= m
        v0, v1, v2, v3 = rounds(2, v0, v1, v2, v3)
        v0 ^= m
    last = int.from_bytes(msg[full:], "little") | ((len(msg) & 0xFF) << 56)
    v3 ^= last
    v0, v1, v2, v3 = rounds(2, v0, v1, v2, v3)
    v0 ^= last
    v2 ^= 0xFF
    v0, v1, v2, v3 = rounds(4, v0, v1, v2, v3)
    return v0 ^ v1 ^ v2 ^ v3


def kv_hash(nb: int, table_key: bytes, key: bytes, sip=siphash24):
    """(tag, b1, b2): the definition's values; `sip` stands in for SipHash where a test exercises the rules around it"""
    k0, k1 = int.from_bytes(table_key[:8], "little"), int.from_bytes(table_key[8:16], "little")
    tag = sip(k0, k1, key) or 1
    u = sip(k0, k1 ^ 0xA5, key)
    b1, b2 = (u & 0xFFFFFFFF) % nb, (u >> 32) % nb
    if b2 == b1:
        b2 = b1 ^ 1
    return tag, b1, b2


def siphash24_many(k0: int, k1: int, msgs: np.ndarray) -> np.ndarray:
    """siphash24 of every row of msgs [n][len] (uint8) at once: the same steps on uint64 arrays, whose sums wrap mod 2^64"""
    msgs = np.ascontiguousarray(msgs, dtype=np.uint8)
    n, ln = msgs.shape
    u = np.uint64
    rotl = lambda x, b: (x << u(b)) | (x >> u(64 - b))
    v = [np.full(n, c, dtype=np.uint64) for c in (k0 ^ 0x736F6D6570736575, k1 ^ 0x646F72616E646F6D, k0 ^ 0x6C7967656E657261, k1 ^ 0x7465646279746573)]

    def rounds(k):
        for _ in range(k):
            v[0] = v[0] + v[1]
            v[1] = rotl(v[1], 13) ^ v[0]
            v[0] = rotl(v[0], 32)
            v[2] = v[2] + v[3]
            v[3] = rotl(v[3], 16) ^ v[2]
            v[0] = v[0] + v[3]
            v[3] = rotl(v[3], 21) ^ v[0]
            v[2] = v[2] + v[1]
            v[1] = rotl(v[1], 17) ^ v[2]
            v[2] = rotl(v[2], 32)

    padded = np.zeros((n, ln // 8 * 8 + 8), dtype=np.uint8)
    padded[:, :ln] = msgs
    padded[:, -1] = ln & 0xFF
    for m in padded.view("<u8").T:
        v[3] = v[3] ^ m
        rounds(2)
        v[0] = v[0] ^ m
    v[2] = v[2] ^ u(0xFF)
    rounds(4)
    return v[0] ^ v[1] ^ v[2] ^ v[3]


def kv_hash_many(nb: int, table_key: bytes, keys: np.ndarray):
    """kv_hash of every row of keys [n][len]: (tags, b1, b2) as uint64 arrays"""
    k0, k1 = int.from_bytes(table_key[:8], "little"), int.from_bytes(table_key[8:16], "little")
    tag = siphash24_many(k0, k1, keys)
    tag[tag == 0] = 1
    h = siphash24_many(k0, k1 ^ 0xA5, keys)
    b1, b2 = (h & np.uint64(0xFFFFFFFF)) % np.uint64(nb), (h >> np.uint64(32)) % np.uint64(nb)
    b2 = np.where(b2 == b1, b1 ^ np.uint64(1), b2)
    return tag, b1, b2


def place_fresh(nb: int, slots: int, b1, b2):
    """the placement rule for keys with distinct tags into an EMPTY table, counting only: the used slots of every bucket afterwards (slots fill from 0
    upwards, so a bucket's count is its next free slot).  Raises Full at the first key whose two buckets are full"""
    used = [0] * nb
    for k, (x, y) in enumerate(zip(b1.tolist(), b2.tolist())):
        if used[x] >= slots and used[y] >= slots:
            raise Full(k)
        used[y if used[y] < used[x] else x] += 1
    return used


def key_set(n: int, first: int = 0):
    """the tests' keys: b"key-%08d" % i"""
    return [b"key-%08d" % i for i in range(first, first + n)]


def key_array(keys) -> np.ndarray:
    return np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(len(keys), -1)


TABLE_KEY = bytes(range(16))
# (keys, buckets, slots) of every table the GPU tests load with key_set(n) under TABLE_KEY; tests/test_kv_cpu.py shows that the
# restated placement places every one of them.  Tables are loaded to 0.75 of their capacity; two slots per bucket overflow early (4096 buckets of
# two: at key 2532), so those tables take 38 keys into 32 buckets and a quarter of the capacity otherwise.
KEY_SETS = [(768, 32, 32), (921, 32, 32), (504, 32, 21), (38, 32, 2), (117_964, 4096, 32),  # (the sets the feature was specified with)
            (98_304, 4096, 32), (2048, 4096, 2), (144_384, 4096, 47), (24_576, 1024, 32), (3072, 128, 32), (1128, 32, 47)]


def load_size(lay) -> int:
    if lay.slots == 2:
        return 38 if lay.buckets == 32 else lay.capacity // 4
    return lay.capacity * 3 // 4


@dataclass(frozen=True)
class Layout:
    coeff_bits: int
    slots: int
    value_bytes: int
    item_bytes: int
    buckets: int
    capacity: int


def layout(p_db: int, nu1: int, nu2: int, value_bytes: int):
    """the layout, or the reason it is refused (a string)"""
    w = p_db.bit_length() - 1
    item_bytes, nb = 1024 * w, 1 << (nu1 + nu2)
    slots = item_bytes // (8 + value_bytes)
    if value_bytes < 1:
        return "value"
    if slots == 0:
        return "slots = 0"
    if slots > 256:
        return "slots > 256"
    if 8 * slots > 256 * w:
        return "header"
    if nb < 2:
        return "buckets"
    return Layout(w, slots, value_bytes, item_bytes, nb, nb * slots)


class Full(Exception):
    """a key whose two buckets are full: .position is its place in the call"""

    def __init__(self, position):
        super().__init__(f"key {position} cannot be placed")
        self.position = position


class Table:
    """the table a sequence of load / put / delete calls should leave: tags[bucket][slot] (0: empty) and vals[bucket][slot] = bytes"""

    def __init__(self, lay: Layout, table_key: bytes):
        self.lay, self.tk = lay, bytes(table_key)
        self.tags = np.zeros((lay.buckets, lay.slots), dtype=np.uint64)
        self.vals = np.zeros((lay.buckets, lay.slots, lay.value_bytes), dtype=np.uint8)

    def hash(self, key):
        return kv_hash(self.lay.buckets, self.tk, bytes(key))

    def find(self, key, tags=None):
        """(candidate 1 or 2, bucket, slot), or (0, None, None): b1 is looked at first, the lowest slot"""
        tags = self.tags if tags is None else tags
        tag, b1, b2 = self.hash(key)
        for c, b in ((1, b1), (2, b2)):
            hit = np.flatnonzero(tags[b] == np.uint64(tag))
            if len(hit):
                return c, b, int(hit[0])
        return 0, None, None

    def _walk(self, keys, tags, skip_full=False):
        """the placement rule over the keys in the order of the call, on `tags`: [(position, bucket, slot)] of the keys placed"""
        where = []
        for k, key in enumerate(keys):
            tag, b1, b2 = self.hash(key)
            c, b, s = self.find(key, tags)
            if not c:
                u1, u2 = int((tags[b1] != 0).sum()), int((tags[b2] != 0).sum())
                if u1 >= self.lay.slots and u2 >= self.lay.slots:
                    if skip_full:
                        continue
                    raise Full(k)
                b = b2 if u2 < u1 else b1  # fewer used slots; a tie goes to b1
                s = int(np.flatnonzero(tags[b] == 0)[0])  # the lowest free slot
            tags[b, s] = tag
            where.append((k, b, s))
        return where

    def put(self, keys, values):
        """insert or overwrite; raises Full (and changes nothing) where a key does not fit.  Returns the (bucket, slot) of every key"""
        tags = self.tags.copy()
        where = self._walk(keys, tags)
        self.tags = tags
        for k, b, s in where:
            self.vals[b, s] = np.frombuffer(bytes(values[k]), dtype=np.uint8)
        return [(b, s) for _, b, s in where]

    def fits(self, keys):
        """the keys of `keys` that a put of them, in this order, could place (the others dropped); the table is not changed"""
        return [keys[k] for k, _, _ in self._walk(keys, self.tags.copy(), skip_full=True)]

    def load(self, keys, values):
        """put() of keys with distinct tags into this EMPTY table, fast: keys [n][len] and values [n][V] as uint8 arrays, hashed at once"""
        assert not self.tags.any()
        tag, b1, b2 = kv_hash_many(self.lay.buckets, self.tk, keys)
        assert len(np.unique(tag)) == len(tag)
        used, bs, ss = [0] * self.lay.buckets, [], []
        for k, (x, y) in enumerate(zip(b1.tolist(), b2.tolist())):
            if used[x] >= self.lay.slots and used[y] >= self.lay.slots:
                raise Full(k)
            b = y if used[y] < used[x] else x
            bs.append(b)
            ss.append(used[b])
            used[b] += 1
        self.tags[bs, ss] = tag
        self.vals[bs, ss] = values
        return list(zip(bs, ss))

    def delete(self, keys):
        n = 0
        for key in keys:
            c, b, s = self.find(key)
            if c:
                self.tags[b, s] = 0
                self.vals[b, s] = 0
                n += 1
        return n

    def get(self, keys, fill=0):
        """(values [n][V] with `fill` in the rows of absent keys, found [n])"""
        out = np.full((len(keys), self.lay.value_bytes), fill, dtype=np.uint8)
        found = np.zeros(len(keys), dtype=np.uint8)
        for k, key in enumerate(keys):
            c, b, s = self.find(key)
            found[k] = c
            if c:
                out[k] = self.vals[b, s]
        return out, found

    def stream(self) -> np.ndarray:
        """[buckets][item_bytes]: tags little-endian at 8 s, values at 8 slots + s V, every other byte zero"""
        L = self.lay
        out = np.zeros((L.buckets, L.item_bytes), dtype=np.uint8)
        out[:, :8 * L.slots] = self.tags.astype("<u8").view(np.uint8).reshape(L.buckets, 8 * L.slots)
        out[:, 8 * L.slots:8 * L.slots + L.slots * L.value_bytes] = self.vals.reshape(L.buckets, -1)
        return out

    def fullest(self) -> int:
        return int((self.tags != 0).sum(axis=1).max())


def scan(lay: Layout, plaintext, tag: int):
    """the header scan and value cut on one decoded plaintext [2][2][2048]: the value bytes of the lowest slot whose tag is `tag`, or None"""
    w = lay.coeff_bits
    header = R.cut(plaintext, w, 0, 8 * lay.slots).view("<u8")
    hit = np.flatnonzero(header == np.uint64(tag))
    if not len(hit):
        return None
    return R.cut(plaintext, w, 8 * lay.slots + int(hit[0]) * lay.value_bytes, lay.value_bytes)


def find_in(lay: Layout, plain1, plain2, tag: int):
    """(value bytes or zeros, found) from the two candidates' plaintexts: candidate 1 wins"""
    for c, pt in ((1, plain1), (2, plain2)):
        v = scan(lay, pt, tag)
        if v is not None:
            return v, c
    return np.zeros(lay.value_bytes, dtype=np.uint8), 0
