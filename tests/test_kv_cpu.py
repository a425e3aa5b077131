"""CPU-side checks of keyed records (include/spiral_gpu.h "Keyed records"): SipHash-2-4 against the algorithm's published vectors, kv_hash and
kv_layout against the restatement (tests/kv_restated.py), the refusals, and the restated placement on every key set the GPU tests use -- the
condition that keeps a GPU test from passing by placing nothing."""
import ctypes as C

import numpy as np
import pytest

import kv_restated as K

NEW_SYMBOLS = ["spiral_gpu_kv_layout_of", "spiral_gpu_kv_hash", "spiral_gpu_server_kv_load", "spiral_gpu_server_kv_put", "spiral_gpu_server_kv_delete",
               "spiral_gpu_server_kv_get", "spiral_gpu_client_kv_queries", "spiral_gpu_client_kv_decode"]
TK = bytes(range(16))  # the table key 00 01 .. 0f of the published vectors
K0, K1 = int.from_bytes(TK[:8], "little"), int.from_bytes(TK[8:], "little")


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


key_set = K.key_set


def test_new_symbols_exported_and_declared(sa):
    from spiral_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name


@pytest.mark.parametrize("msg,want", [(b"", 0x726FDB47DD0E0E31), (bytes(range(15)), 0xA129CA6149BE45E5), (bytes(range(8)), 0x93F5F5799A932462)],
                         ids=["empty", "15-bytes", "8-bytes"])
def test_siphash_vectors(sa, msg, want):
    """the restatement, its vectorised form and the library (through kv_hash's tag: none of the three values is 0) give the published values"""
    assert K.siphash24(K0, K1, msg) == want
    assert int(K.siphash24_many(K0, K1, np.frombuffer(msg, dtype=np.uint8).reshape(1, -1))[0]) == want
    assert sa.kv_hash(sa.make_params(6, 6), TK, msg)[0] == want


@pytest.mark.parametrize("geom", [(6, 6), (1, 0), (8, 7), (3, 2)], ids=["nb4096", "nb2", "nb32768", "nb32"])
def test_hash_equals_the_restatement(sa, geom):
    """a few hundred keys of lengths 0 .. 40 under two table keys; with nb = 2 about half of them have b2 = b1 before the rule moves b2"""
    pg = sa.make_params(*geom)
    nb = 1 << sum(geom)
    rng = np.random.default_rng(nb)
    collided = 0
    for tk in (TK, bytes(rng.integers(0, 256, size=16, dtype=np.uint8))):
        for i in range(164):
            key = bytes(rng.integers(0, 256, size=i % 41, dtype=np.uint8))
            want = K.kv_hash(nb, tk, key)
            assert sa.kv_hash(pg, tk, key) == want, (geom, i)
            u = K.siphash24(int.from_bytes(tk[:8], "little"), int.from_bytes(tk[8:], "little") ^ 0xA5, key)
            if (u & 0xFFFFFFFF) % nb == (u >> 32) % nb:
                collided += 1
                assert want[2] == want[1] ^ 1
            assert want[1] != want[2] and want[1] < nb and want[2] < nb and want[0] != 0
    if nb == 2:
        assert collided > 50, "nb = 2 exercises b2 = b1"


def test_hash_rules_around_siphash():
    """a SipHash result of 0 becomes tag 1; b2 = b1 becomes b1 XOR 1 -- exercised through the restated function with a stand-in for SipHash"""
    assert K.kv_hash(64, TK, b"x", sip=lambda k0, k1, m: 0) == (1, 0, 1)
    assert K.kv_hash(64, TK, b"x", sip=lambda k0, k1, m: (37 << 32) | 37) == ((37 << 32) | 37, 37, 36)
    assert K.kv_hash(64, TK, b"x", sip=lambda k0, k1, m: (5 << 32) | 70) == ((5 << 32) | 70, 6, 5)
    many = K.kv_hash_many(4096, TK, np.frombuffer(b"".join(key_set(300)), dtype=np.uint8).reshape(300, 12))
    assert [tuple(int(x[i]) for x in many) for i in range(300)] == [K.kv_hash(4096, TK, k) for k in key_set(300)]


@pytest.mark.parametrize("geom,p_db,V", [((6, 6), 256, 248), ((6, 6), 256, 3000), ((6, 6), 32, 99), ((6, 4), 256, 248), ((4, 3), 256, 248), ((3, 2), 16, 248),
                                         ((3, 2), 256, 24), ((8, 7), 256, 248), ((6, 6), 256, 8184), ((3, 2), 32, 24), ((11, 9), 32768, 52)])
def test_layout_equals_the_restatement(sa, geom, p_db, V):
    want = K.layout(p_db, *geom, V)
    got = sa.kv_layout(sa.make_params(*geom, p_db=p_db), V)
    assert (got.coeff_bits, got.slots, got.value_bytes, got.item_bytes, got.buckets, got.capacity) == (want.coeff_bits, want.slots, V, want.item_bytes, want.buckets,
                                                                                                    want.capacity)
    assert got.capacity == (1 << sum(geom)) * (got.item_bytes // (8 + V))


def test_the_quoted_layouts(sa):
    assert K.layout(256, 6, 6, 248).slots == 32 and K.layout(256, 6, 6, 3000).slots == 2 and K.layout(32, 6, 6, 99).slots == 47
    assert sa.kv_layout(sa.make_params(8, 7), 248).capacity == 32 * 32768


def test_layout_refusals(sa):
    pg = sa.make_params(6, 6)
    cases = [(pg, 8185, "slots = 0"), (pg, 1 << 40, "slots = 0"), (pg, 23, "slots > 256"), (sa.make_params(6, 6, p_db=32), 20, "header"),
             (sa.make_params(0, 0), 248, "buckets")]
    match = {"slots = 0": "slots = 0", "slots > 256": "at most 256", "header": "inside polynomial 0", "buckets": "at least 2 buckets"}
    for p, V, why in cases:
        assert K.layout(int(p.p_db), int(p.nu1), int(p.nu2), V) == why
        with pytest.raises(sa.SpiralGpuError, match=match[why]):
            sa.kv_layout(p, V)
    assert K.layout(256, 6, 6, 24).slots == 256 and sa.kv_layout(pg, 24).slots == 256  # the largest header: all of polynomial 0 at 8 bits
    with pytest.raises(sa.SpiralGpuError, match="at least one byte"):
        sa.kv_layout(pg, 0)
    with pytest.raises(ValueError):
        sa.kv_layout(pg, -1)
    with pytest.raises(sa.SpiralGpuError, match="base parameter sets only"):
        sa.kv_layout(pg, 248, out_n=2)
    L = sa.lib()
    out = sa.KvLayout(7, 7, 7, 7, 7, 7)
    assert L.spiral_gpu_kv_layout_of(None, 248, C.byref(out)) != 0 and b"null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_kv_layout_of(C.byref(pg), 23, C.byref(out)) != 0
    assert (out.coeff_bits, out.slots, out.capacity) == (7, 7, 7), "a refused layout writes nothing"


def test_null_handles_fail_with_a_message(sa):
    L = sa.lib()
    buf = np.full(4096, 0xA5, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    n = C.c_uint64(9)
    for rc in (L.spiral_gpu_server_kv_load(None, p, p, 4, p, 248, 1), L.spiral_gpu_server_kv_put(None, p, p, 4, p, 248, 1),
               L.spiral_gpu_server_kv_delete(None, p, p, 4, 248, 1, C.byref(n)), L.spiral_gpu_server_kv_get(None, p, p, 4, p, 248, 1, p)):
        assert rc != 0 and b"null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_client_kv_queries(None, p, p, 4, 1, 2, p, buf.size) != 0 and b"null client session" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_client_kv_decode(None, p, p, 4, p, 1, 0, 248, p, p) != 0 and b"null client session" in L.spiral_gpu_last_error()
    assert (buf == 0xA5).all() and n.value == 9, "nothing written"


def test_wrappers_reject_bad_argument_lists(sa):
    from spiral_amd import _lib

    with pytest.raises(ValueError, match="one length"):
        _lib.kv_keys([b"ab", b"abc"])
    with pytest.raises(TypeError):
        _lib.kv_keys(np.zeros((2, 3), dtype=np.uint16))
    with pytest.raises(ValueError, match="16 bytes"):
        sa.kv_hash(sa.make_params(6, 6), b"short", b"k")
    assert _lib.kv_keys([b"ab", b"cd"]).tolist() == [[97, 98], [99, 100]] and _lib.kv_keys([]).shape == (0, 0)


@pytest.mark.parametrize("n,nb,slots", K.KEY_SETS)
def test_the_restated_placement_places_every_key(n, nb, slots):
    keys = np.frombuffer(b"".join(key_set(n)), dtype=np.uint8).reshape(n, 12)
    tag, b1, b2 = K.kv_hash_many(nb, TK, keys)
    assert len(np.unique(tag)) == n, "the tags are distinct"
    used = K.place_fresh(nb, slots, b1, b2)
    assert sum(used) == n and max(used) <= (slots - 1 if slots > 2 else slots), "every key is placed, and no bucket of more than two slots is full"
    if n <= 1000:  # the counting form is the model table's rule
        V = {32: 248, 21: 187, 2: 3000}[slots]
        lay = K.layout(256 if slots != 21 else 16, 3, 2, V)
        assert (lay.buckets, lay.slots) == (nb, slots)
        t = K.Table(lay, TK)
        where = t.put(key_set(n), [bytes(V)] * n)
        assert [int((t.tags[b] != 0).sum()) for b in range(nb)] == used and len(set(where)) == n
        fast = K.Table(lay, TK)
        assert fast.load(keys, np.zeros((n, V), dtype=np.uint8)) == where and (fast.tags == t.tags).all(), "Table.load is Table.put from empty"


def test_an_overfull_pair_of_buckets_is_refused():
    """keys chosen so that both candidates are buckets 0 and 1 (nb = 2: every key): 2 x slots fit, the next one is refused by position, and the failed
    call changes nothing"""
    lay = K.layout(256, 1, 0, 3000)
    assert (lay.buckets, lay.slots) == (2, 2)
    t = K.Table(lay, TK)
    keys = key_set(6)
    t.put(keys[:3], [bytes([k]) * 3000 for k in range(3)])
    before = t.stream().copy()
    with pytest.raises(K.Full) as e:
        t.put(keys[3:], [bytes(3000)] * 3)
    assert e.value.position == 1 and (t.stream() == before).all()
    with pytest.raises(K.Full) as e:
        K.place_fresh(2, 2, *K.kv_hash_many(2, TK, np.frombuffer(b"".join(keys), dtype=np.uint8).reshape(6, 12))[1:])
    assert e.value.position == 4
    assert t.put([keys[1]], [bytes([9]) * 3000]) and t.get([keys[1], keys[5]])[1].tolist()[1] == 0  # an existing key still overwrites in a full table
