"""CPU-side checks of keyed records on SpiralPack parameter sets and of kv_stats' entry points (include/spiral_gpu.h "Keyed records", SpiralPack):
the new symbols, pack_kv_layout_of against the restatement (tests/pack_kv_restated.py) with its refusals, pack_kv_hash against kv_hash, and the
restated placement on every key set the GPU tests load -- the condition that keeps a GPU test from passing by placing nothing."""
import ctypes as C

import numpy as np
import pytest

import kv_restated as K
import pack_kv_restated as PK

NEW_SYMBOLS = ["spiral_gpu_pack_kv_layout_of", "spiral_gpu_pack_kv_hash", "spiral_gpu_pack_server_kv_load", "spiral_gpu_pack_server_kv_put",
               "spiral_gpu_pack_server_kv_delete", "spiral_gpu_pack_server_kv_get", "spiral_gpu_server_kv_stats", "spiral_gpu_pack_server_kv_stats"]
TK = PK.TABLE_KEY


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def fields(lay):
    return lay.coeff_bits, lay.slots, lay.value_bytes, lay.item_bytes, lay.buckets, lay.capacity


def test_new_symbols_exported_and_declared(sa):
    from spiral_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
    header = open(_lib.os.path.join(_lib.HERE, "..", "include", "spiral_gpu.h")).read()
    for name in NEW_SYMBOLS:
        assert f"int {name}(" in header, name
    assert C.sizeof(_lib.KvStatsStruct) == 8 * 3 + 4 * 2 + 8 * 257


# the geometries of tests/test_gpu_pack_kv.py, the quoted layout at out_n = 4, and sizes around them
GEOMS = [((4, 2), 2, 256, 248), ((4, 2), 2, 256, 3000), ((7, 4), 2, 256, 248), ((7, 4), 2, 256, 3000), ((7, 3), 3, 256, 3000), ((7, 3), 3, 256, 248),
         ((7, 3), 3, 256, 5000), ((4, 2), 2, 32, 99), ((7, 3), 4, 256, 4088), ((7, 3), 4, 256, 32760), ((4, 2), 1, 256, 248), ((9, 6), 16, 256, 500_000)]


@pytest.mark.parametrize("geom,out_n,p_db,V", GEOMS)
def test_layout_equals_the_restatement(sa, geom, out_n, p_db, V):
    want = PK.layout(p_db, *geom, out_n, V)
    got = sa.pack_kv_layout(sa.make_params(*geom, p_db=p_db), out_n, V)
    assert fields(got) == fields(want)
    assert got.item_bytes == out_n * out_n * 256 * want.coeff_bits and got.capacity == (1 << sum(geom)) * (got.item_bytes // (8 + V))


def test_the_quoted_layouts(sa):
    a, b = PK.layout(256, 4, 2, 2, 248), PK.layout(256, 7, 3, 4, 4088)
    assert (a.slots, a.item_bytes) == (32, 8192) == (K.layout(256, 4, 2, 248).slots, K.layout(256, 4, 2, 248).item_bytes), "out_n = 2: as the base server's"
    assert (b.slots, b.item_bytes) == (8, 32768)
    assert sa.pack_kv_layout(sa.make_params(7, 3), 4, 4088).slots == 8
    lay = PK.layout(256, 7, 3, 3, 5000)
    assert lay.slots == 3 and [list(PK.value_polys(lay, s)) for s in range(3)] == [[0, 1, 2], [2, 3, 4], [4, 5, 6, 7]], "V = 5000: values span polynomials 0-2, 2-4, 4-7"


def test_layout_refusals(sa):
    pg, p32 = sa.make_params(4, 2), sa.make_params(4, 2, p_db=32)
    cases = [(pg, 2, 8185, "slots = 0"), (pg, 4, 32761, "slots = 0"), (pg, 2, 1 << 40, "slots = 0"), (pg, 2, 23, "slots > 256"), (pg, 4, 119, "slots > 256"),
             (p32, 4, 94, "header"), (p32, 2, 20, "header")]
    match = {"slots = 0": "slots = 0", "slots > 256": "at most 256", "header": "inside polynomial 0"}
    for p, out_n, V, why in cases:
        assert PK.layout(int(p.p_db), int(p.nu1), int(p.nu2), out_n, V) == why, (out_n, V)
        with pytest.raises(sa.SpiralGpuError, match=match[why]):
            sa.pack_kv_layout(p, out_n, V)
    assert PK.layout(256, 4, 2, 4, 120).slots == 256 and sa.pack_kv_layout(pg, 4, 120).slots == 256  # the largest header: all of polynomial 0 at 8 bits
    with pytest.raises(sa.SpiralGpuError, match="at least one byte"):
        sa.pack_kv_layout(pg, 2, 0)
    with pytest.raises(sa.SpiralGpuError, match="out_n out of range"):
        sa.pack_kv_layout(pg, 17, 248)
    with pytest.raises(ValueError):
        sa.pack_kv_layout(pg, -1, 248)
    with pytest.raises(sa.SpiralGpuError, match="call pack_kv_layout"):
        sa.kv_layout(pg, 248, out_n=2)  # (kv_layout stays the base layout and names the SpiralPack call)
    assert PK.layout(256, 4, 2, 17, 248) == PK.layout(256, 4, 2, 0, 248) == "out_n"
    L = sa.lib()
    out = sa.KvLayout(7, 7, 7, 7, 7, 7)
    assert L.spiral_gpu_pack_kv_layout_of(C.byref(pg), 0, 248, C.byref(out)) != 0 and b"out_n out of range" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_pack_kv_layout_of(C.byref(pg), 17, 248, C.byref(out)) != 0 and b"out_n out of range" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_pack_kv_layout_of(None, 2, 248, C.byref(out)) != 0 and b"null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_pack_kv_layout_of(C.byref(pg), 2, 23, C.byref(out)) != 0
    assert (out.coeff_bits, out.slots, out.capacity) == (7, 7, 7), "a refused layout writes nothing"
    t, b1, b2 = C.c_uint64(9), C.c_uint64(9), C.c_uint64(9)
    buf = np.zeros(16, dtype=np.uint8).ctypes.data_as(C.c_void_p)
    assert L.spiral_gpu_pack_kv_hash(C.byref(pg), 0, buf, buf, 4, C.byref(t), C.byref(b1), C.byref(b2)) != 0 and b"out_n out of range" in L.spiral_gpu_last_error()
    assert (t.value, b1.value, b2.value) == (9, 9, 9)


@pytest.mark.parametrize("geom,out_n", [((4, 2), 2), ((7, 3), 3), ((7, 4), 2), ((1, 1), 1), ((7, 3), 16)])
def test_pack_hash_equals_kv_hash(sa, geom, out_n):
    """the hash depends on nu1 + nu2 alone: pack_kv_hash is kv_hash of the same parameters and the restatement's values"""
    pg = sa.make_params(*geom)
    nb = 1 << sum(geom)
    rng = np.random.default_rng(nb + out_n)
    for tk in (TK, bytes(rng.integers(0, 256, size=16, dtype=np.uint8))):
        for i in range(82):
            key = bytes(rng.integers(0, 256, size=i % 41, dtype=np.uint8))
            got = sa.kv_hash(pg, tk, key, out_n=out_n)
            assert got == sa.kv_hash(pg, tk, key) == K.kv_hash(nb, tk, key), (geom, i)


# the parameters behind every PACK_KEY_SETS entry: (nu1, nu2), out_n, p_db, V
KEY_SET_GEOMS = [((4, 2), 2, 256, 248), ((4, 2), 2, 256, 3000), ((4, 2), 2, 32, 99), ((7, 4), 2, 256, 248), ((7, 4), 2, 256, 3000), ((7, 3), 3, 256, 248),
                 ((7, 3), 3, 256, 3000), ((7, 3), 3, 256, 5000)]


@pytest.mark.parametrize("entry,params", list(zip(PK.PACK_KEY_SETS, KEY_SET_GEOMS)), ids=[f"{n}-{nb}-{s}" for n, nb, s in PK.PACK_KEY_SETS])
def test_the_restated_placement_places_every_key(sa, entry, params):
    n, nb, slots = entry
    geom, out_n, p_db, V = params
    lay = PK.layout(p_db, *geom, out_n, V)
    assert (PK.load_size(lay), lay.buckets, lay.slots) == entry, "the load rule gives the key set"
    assert fields(sa.pack_kv_layout(sa.make_params(*geom, p_db=p_db), out_n, V)) == fields(lay)
    keys = PK.key_array(PK.key_set(n))
    tag, b1, b2 = K.kv_hash_many(nb, TK, keys)
    assert len(np.unique(tag)) == n, "the tags are distinct"
    used = K.place_fresh(nb, slots, b1, b2)
    assert sum(used) == n, "every key is placed"
    if slots <= 3:  # the model table's rule is the counting form's (small tables: the walk is slow)
        t = K.Table(lay, TK)
        where = t.put(PK.key_set(n), [bytes(V)] * n)
        assert [int((t.tags[b] != 0).sum()) for b in range(nb)] == used and len(set(where)) == n
        assert PK.stats_of(t.tags)[:2] == (nb, n)


def test_null_handles_fail_with_a_message(sa):
    L = sa.lib()
    from spiral_amd import _lib

    buf = np.full(4096, 0xA5, dtype=np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    n = C.c_uint64(9)
    st = _lib.KvStatsStruct()
    st.buckets = 77
    for rc in (L.spiral_gpu_pack_server_kv_load(None, p, p, 4, p, 248, 1), L.spiral_gpu_pack_server_kv_put(None, p, p, 4, p, 248, 1),
               L.spiral_gpu_pack_server_kv_delete(None, p, p, 4, 248, 1, C.byref(n)), L.spiral_gpu_pack_server_kv_get(None, p, p, 4, p, 248, 1, p),
               L.spiral_gpu_pack_server_kv_stats(None, 248, 0, 1, C.byref(st)), L.spiral_gpu_server_kv_stats(None, 248, 0, 1, C.byref(st))):
        assert rc != 0 and b"null" in L.spiral_gpu_last_error()
    assert (buf == 0xA5).all() and n.value == 9 and st.buckets == 77, "nothing written"
    s = sa.KvStats(4, 6, 1, 2, 2, (1, 2, 1) + (0,) * 254)
    assert s.load() == 0.75 and sa.KvStats(0, 0, 0, 0, 2, (0,) * 257).load() == 0.0
