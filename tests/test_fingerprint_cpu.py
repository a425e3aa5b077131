"""Database fingerprints on the host (include/spiral_gpu.h "Fingerprints"): the symbols, spiral_gpu_fingerprint_host against the definition restated in
Python integers (tests/fingerprint_restated.py), fingerprint_add, the refusals and the Python wrappers' argument checks.  Needs no GPU."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import fingerprint_restated as FR

P = FR.P
N = 2048
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64P = C.POINTER(C.c_uint64)

KEYS = [(0, 0), (P - 4, 12345), (P - 3, 2**64 - 1), (2**64 - 1, P - 4)]
FIRSTS = [0, 1, 2**24 - 3]
SHAPES = [(4, 0, 4), (9, 4, 1), (16, 0, 16)]  # a base item stream, one SpiralPack trial's stream (trial 4 of 9), a SpiralPack record-layout item
WIDTHS = [(w, p) for w in (1, 8, 15, 16, 63, 64) for p in (2, 256, 1 << 15) if 2**w >= p]


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    return spiral_amd


def stream(items, bits):
    """items[k][q] = 2048 coefficients -> the bit-packed item stream"""
    return np.concatenate([FR.pack_bits(poly, bits) for it in items for poly in it])


def test_symbols_and_abi(sa):
    """the six calls are exported, declared in the header and bound with prototypes; the ABI version stays 1"""
    from spiral_amd import _lib

    L = sa.lib()
    header = open(os.path.join(ROOT, "include", "spiral_gpu.h")).read()
    names = ["spiral_gpu_server_fingerprint_items", "spiral_gpu_server_fingerprint_items_at", "spiral_gpu_pack_server_fingerprint_items",
             "spiral_gpu_pack_server_fingerprint_items_at", "spiral_gpu_fingerprint_host", "spiral_gpu_fingerprint_add"]
    for name in names:
        assert name in _lib.PROTOTYPES, f"{name} is not bound"
        assert getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
        assert re.search(rf"\b{name}\(", header), f"{name} is not declared"
    assert L.spiral_gpu_abi_version() == 1 and "#define SPIRAL_GPU_ABI_VERSION 1\n" in header
    assert header.count("---- Fingerprints") == 1, "the definition is stated once"
    assert sa.FINGERPRINT_MODULUS == P
    assert sa.get_option("db_fingerprint_ns") == 0, "read-only, 0 before any call"
    with pytest.raises(Exception):
        sa.set_option("db_fingerprint_ns", 5)
    for srv in (sa.Server, sa.PackServer):
        assert callable(srv.fingerprint_items) and callable(srv.fingerprint_items_at)


def test_key_bases(sa):
    """the library's r and s at the edges of the key range: a single 1 at coefficient 0 of polynomial 0 of item 0 gives f = r and F = r s"""
    one = np.zeros((1, 4, N), dtype=np.uint64)
    one[0, 0, 0] = 1
    for key, (r, s) in (((0, 0), (2, 2)), ((P - 4, P - 4), (P - 2, P - 2)), ((P - 3, P - 3), (2, 2)), ((P - 2, 1), (3, 3)),
                        ((2**64 - 1, 2**64 - 1), (2 + (2**64 - 1) % (P - 3),) * 2)):
        assert FR.bases(key) == (r, s) and 2 <= r <= P - 2
        F, f = sa.fingerprint_host(key, 256, one, 64, per_item=True)
        assert int(f[0]) == r and F == r * s % P, f"key {key}"


@pytest.mark.parametrize("case", range(len(WIDTHS) * len(SHAPES)))
def test_host_against_restatement(sa, case):
    """two random items per (width, p_db, stream shape), under every key, the first item cycling through 0, 1 and 2^24 - 3"""
    (bits, p_db), (polys, poly0, n_polys) = WIDTHS[case // len(SHAPES)], SHAPES[case % len(SHAPES)]
    rng = np.random.default_rng(100 + case)
    items = rng.integers(0, p_db, size=(2, n_polys, N), dtype=np.uint64)
    items[0, 0, 0] = p_db - 1
    items[1, -1, -1] = p_db - 1
    raw = stream(items, bits)
    for k, key in enumerate(KEYS):
        first = FIRSTS[(case + k) % len(FIRSTS)]
        F, fs = FR.fingerprints(key, items, poly0, first)
        gotF, got = sa.fingerprint_host(key, p_db, raw, bits, polys, poly0, n_polys, first, per_item=True)
        assert [int(v) for v in got] == fs and gotF == F, f"key {key}, first item {first}"
        assert sa.fingerprint_host(key, p_db, raw, bits, polys, poly0, n_polys, first) == F, "combined alone"
        if bits == 64:
            assert sa.fingerprint_host(key, p_db, items.reshape(-1), 64, polys, poly0, n_polys, first) == F, "a uint64 array"


@pytest.mark.parametrize("polys", [4, 9])
def test_crafted_items(sa, polys):
    """all zero, all p_db - 1 (the largest sums), a single 1 at the first and at the last coefficient; at r = P - 2 and at random keys"""
    rng = np.random.default_rng(7)
    keys = [(P - 4, P - 4)] + [tuple(int(v) for v in rng.integers(0, 2**64, size=2, dtype=np.uint64)) for _ in range(2)]
    for key, p_db in itertools.product(keys, (2, 256, 1 << 15)):
        r, s = FR.bases(key)
        zero = np.zeros((1, polys, N), dtype=np.uint64)
        assert sa.fingerprint_host(key, p_db, zero, 64, polys, per_item=True)[1][0] == 0
        full = np.full((1, polys, N), p_db - 1, dtype=np.uint64)
        exp = (p_db - 1) * sum(pow(r, e, P) for e in range(1, N * polys + 1)) % P
        F, f = sa.fingerprint_host(key, p_db, full, 64, polys, first_item=5, per_item=True)
        assert int(f[0]) == exp == FR.item_fingerprint(key, full[0]) and F == exp * pow(s, 6, P) % P
        one = zero.copy()
        one[0, 0, 0] = 1
        assert int(sa.fingerprint_host(key, p_db, one, 64, polys, per_item=True)[1][0]) == r
        one = zero.copy()
        one[0, -1, -1] = 1
        assert int(sa.fingerprint_host(key, p_db, one, 64, polys, per_item=True)[1][0]) == pow(r, N * polys, P)


def test_ranges_and_slices_add(sa):
    """F of adjoining ranges adds to F of their union; the poly0 slices of an item add to the whole item's f"""
    rng = np.random.default_rng(11)
    key = (int(rng.integers(0, 2**63)), int(rng.integers(0, 2**63)))
    items = rng.integers(0, 256, size=(7, 9, N), dtype=np.uint64)
    raw = stream(items, 8)
    F, fs = sa.fingerprint_host(key, 256, raw, 8, 9, first_item=40, per_item=True)
    cut = 3 * 9 * 2048
    Fa = sa.fingerprint_host(key, 256, raw[:cut], 8, 9, first_item=40)
    Fb = sa.fingerprint_host(key, 256, raw[cut:], 8, 9, first_item=43)
    assert sa.fingerprint_add(Fa, Fb) == F == FR.combine(key, fs, range(40, 47))
    parts = []
    for q0, nq in ((0, 4), (4, 1), (5, 4)):
        sl = np.ascontiguousarray(items[:, q0:q0 + nq])
        parts.append(sa.fingerprint_host(key, 256, stream(sl, 8), 8, 9, q0, nq, 40, per_item=True))
    assert sa.fingerprint_add(*[p[0] for p in parts]) == F
    for k in range(7):
        assert sa.fingerprint_add(*[int(p[1][k]) for p in parts]) == int(fs[k])
    assert sa.fingerprint_host(key, 256, raw[:0], 8, 9, per_item=True)[0] == 0, "no items"


def test_fingerprint_add(sa):
    L = sa.lib()
    assert L.spiral_gpu_fingerprint_add(0, 0) == 0
    assert L.spiral_gpu_fingerprint_add(P - 1, 0) == P - 1
    assert L.spiral_gpu_fingerprint_add(P - 1, 1) == 0
    assert L.spiral_gpu_fingerprint_add(P - 1, P - 1) == P - 2
    for a, b in ((P, 0), (0, P), (2**64 - 1, 1)):
        assert L.spiral_gpu_fingerprint_add(a, b) == P, "refused: P is no fingerprint"
        assert b"fingerprint" in L.spiral_gpu_last_error()
    assert sa.fingerprint_add() == 0 and sa.fingerprint_add(5) == 5 and sa.fingerprint_add(P - 1, P - 1, 3) == 1
    for bad in (P, -1, 1.5, True):
        with pytest.raises(ValueError):
            sa.fingerprint_add(1, bad)


def test_refusals(sa):
    L = sa.lib()
    key = (C.c_uint64 * 2)(3, 4)
    items = np.zeros((2, 4, N), dtype=np.uint64)
    items[1, 2, 77] = 256
    out, comb = np.zeros(2, dtype=np.uint64), C.c_uint64(0)

    def raw(p_db=256, bits=64, polys=4, poly0=0, n_polys=4, per=True, com=True, k=key, buf=items):
        return L.spiral_gpu_fingerprint_host(k, p_db, buf.ctypes.data_as(C.c_void_p), bits, polys, poly0, n_polys, 10, 2, out.ctypes.data_as(U64P) if per else None,
                                             C.byref(comb) if com else None)

    assert raw() != 0
    msg = L.spiral_gpu_last_error().decode()
    assert "coefficient 77 of polynomial 2 of item 11" in msg and "p_db" in msg, msg
    with pytest.raises(sa.SpiralGpuError, match="coefficient 77 of polynomial 2 of item 1 "):
        sa.fingerprint_host((3, 4), 256, items, 64)
    items[1, 2, 77] = 255
    assert raw() == 0
    assert raw(per=False, com=False) != 0 and b"both null" in L.spiral_gpu_last_error()
    assert raw(per=False) == 0 and raw(com=False) == 0
    assert raw(poly0=1) != 0 and b"outside an item" in L.spiral_gpu_last_error()
    assert raw(polys=3) != 0 and raw(polys=0, n_polys=0) != 0 and raw(polys=257, n_polys=1) != 0
    assert raw(k=None) != 0
    assert raw(bits=7) != 0 and b"coeff_bits" in L.spiral_gpu_last_error()
    assert raw(bits=0) != 0 and raw(bits=65) != 0
    assert raw(p_db=1) != 0 and raw(p_db=P + 1) != 0


def test_python_argument_checks(sa):
    items = np.zeros((1, 4, N), dtype=np.uint64)
    for key in (5, (1,), (1, 2, 3), (-1, 0), (0, 2**64), (0.5, 1), "ab", (True, 1)):
        with pytest.raises(ValueError, match="key"):
            sa.fingerprint_host(key, 256, items, 64)
    assert sa.fingerprint_host([1, 2], 256, items, 64) == 0 and sa.fingerprint_host(np.array([1, 2], dtype=np.uint64), 256, items, 64) == 0
    with pytest.raises(ValueError, match="whole items"):
        sa.fingerprint_host((1, 2), 256, np.zeros(8191, dtype=np.uint8), 8)
    with pytest.raises(TypeError):
        sa.fingerprint_host((1, 2), 256, items, 8)
    with pytest.raises(TypeError):
        sa.fingerprint_host((1, 2), 256, items.astype(np.float64), 64)
    with pytest.raises(ValueError, match="coeff_bits"):
        sa.fingerprint_host((1, 2), 256, np.zeros(8192, dtype=np.uint8), 0)
    with pytest.raises(ValueError):
        sa.fingerprint_host((1, 2), 256, items, 64, first_item=-1)
    with pytest.raises(sa.SpiralGpuError, match="outside an item"):
        sa.fingerprint_host((1, 2), 256, items, 64, polys_per_item=4, poly0=2, n_polys=4)
    assert sa.fingerprint_host((1, 2), 256, bytes(8192), 8) == 0, "bytes are taken"
