"""Tracked fingerprints on the host (include/spiral_gpu.h "Fingerprints", Tracked): the new symbols, spiral_gpu_fingerprint_of_polys against
spiral_gpu_fingerprint_host and against the restatement (tests/fingerprint_track_restated.py), its refusals, and the device calls failing loudly where
there is no device.  Needs no GPU.  Every comparison is of exact integers."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fingerprint_restated as FR
import fingerprint_track_restated as FTR

P, N = FR.P, FR.N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64P = C.POINTER(C.c_uint64)
KEY = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F)
TRACK_CALLS = ("track", "untrack", "tracked", "tracked_polys", "scrub")


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    return spiral_amd


def test_symbols(sa):
    """the eleven calls are exported, declared in the header and bound with prototypes; the ABI version stays as it is"""
    from spiral_amd import _lib

    L = sa.lib()
    header = open(os.path.join(ROOT, "include", "spiral_gpu.h")).read()
    names = [f"{pre}_fingerprint_{c}" for pre in ("spiral_gpu_server", "spiral_gpu_pack_server") for c in TRACK_CALLS] + ["spiral_gpu_fingerprint_of_polys"]
    for name in names:
        assert name in _lib.PROTOTYPES, f"{name} is not bound"
        assert getattr(L, name).argtypes == _lib.PROTOTYPES[name][1]
        assert re.search(rf"\b{name}\(", header), f"{name} is not declared"
    assert L.spiral_gpu_abi_version() == 1
    assert header.count("/* Tracked.") == 1 and header.count("---- Fingerprints") == 1, "the definition is stated once"
    for srv in (sa.Server, sa.PackServer):
        for c in TRACK_CALLS:
            assert callable(getattr(srv, "fingerprint_" + c))
    assert callable(sa.fingerprint_of_polys)


def test_restatement_against_python_integers():
    """the numpy route of the restatement (three-limb products) against plain Python integers, at the largest weight too"""
    rng = np.random.default_rng(3)
    polys = rng.integers(0, 1 << 16, size=(3, N), dtype=np.uint64)
    polys[2] = (1 << 24) - 1
    for key in (KEY, (P - 4, 1), (0, 0)):
        assert [int(v) for v in FTR.poly_sums(key, polys)] == [FTR.poly_sum_slow(key, p) for p in polys]
    g = FTR.poly_sums(KEY, polys[:2].reshape(1, 2, N))
    assert FTR.item_values(KEY, g, 3) == [FR.item_fingerprint(KEY, polys[:2], 3)]
    F = FTR.combined(KEY, g, 3, first_item=5)
    g2 = g.copy()
    g2[0, 1] = FTR.poly_sums(KEY, polys[2])
    assert FTR.apply(KEY, F, g[0, 1], g2[0, 1], 3 + 1, 5) == FTR.combined(KEY, g2, 3, first_item=5), "the apply rule is the definition's difference"


@pytest.mark.parametrize("polys,poly0,n_polys", [(4, 0, 4), (9, 2, 1), (9, 2, 7)], ids=["base", "one-trial", "trial-range"])
def test_of_polys_against_host(sa, polys, poly0, n_polys):
    """g from fingerprint_host with polys_per_item = 1 on single polynomials; f and F from fingerprint_of_polys equal fingerprint_host of the same
    stream, for a range that does not start at item 0"""
    rng = np.random.default_rng(polys * 10 + n_polys)
    first, n = 5, 6
    for p_db, bits in ((256, 8), (1 << 15, 17)):
        x = rng.integers(0, p_db, size=(n, n_polys, N), dtype=np.uint64)
        x[0, 0] = p_db - 1
        stream = np.concatenate([FR.pack_bits(poly, bits) for it in x for poly in it])
        want_F, want_f = sa.fingerprint_host(KEY, p_db, stream, bits, polys, poly0, n_polys, first, per_item=True)
        g = np.array([[sa.fingerprint_host(KEY, p_db, FR.pack_bits(poly, bits), bits, 1, 0, 1, 0, per_item=True)[1][0] for poly in it] for it in x], dtype=np.uint64)
        assert (g == FTR.poly_sums(KEY, x)).all(), "g: the library's host function against the restatement"
        F, f = sa.fingerprint_of_polys(KEY, g, polys, poly0, n_polys, first, per_item=True)
        assert F == want_F and (f == want_f).all()
        assert sa.fingerprint_of_polys(KEY, g, polys, poly0, n_polys, first) == F == FTR.combined(KEY, g, poly0, first_item=first)
        assert [int(v) for v in f] == FTR.item_values(KEY, g, poly0)


def test_of_polys_refusals(sa):
    L = sa.lib()
    key = (C.c_uint64 * 2)(*KEY)
    g = np.zeros((2, 4), dtype=np.uint64)
    out, comb = np.full(2, 0x5A5A, dtype=np.uint64), C.c_uint64(0x5A5A)
    gp, outp = g.ctypes.data_as(U64P), out.ctypes.data_as(U64P)
    assert L.spiral_gpu_fingerprint_of_polys(key, gp, 4, 0, 4, 0, 2, outp, C.byref(comb)) == 0 and comb.value == 0 and (out == 0).all()
    comb.value = 0x5A5A
    g[1, 2] = P
    assert L.spiral_gpu_fingerprint_of_polys(key, gp, 4, 0, 4, 7, 2, outp, C.byref(comb)) != 0
    assert b"polynomial 2 of item 8" in L.spiral_gpu_last_error() and comb.value == 0x5A5A, "a word >= P is refused, and named"
    g[1, 2] = P - 1
    assert L.spiral_gpu_fingerprint_of_polys(key, gp, 4, 0, 4, 7, 2, outp, C.byref(comb)) == 0
    assert L.spiral_gpu_fingerprint_of_polys(key, gp, 4, 0, 4, 0, 2, None, None) != 0 and b"both null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_fingerprint_of_polys(key, gp, 4, 1, 4, 0, 2, outp, C.byref(comb)) != 0 and b"outside an item" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_fingerprint_of_polys(key, gp, 4, 5, 0, 0, 2, outp, C.byref(comb)) != 0
    assert L.spiral_gpu_fingerprint_of_polys(key, gp, 0, 0, 0, 0, 2, outp, C.byref(comb)) != 0
    assert L.spiral_gpu_fingerprint_of_polys(key, gp, 257, 0, 4, 0, 2, outp, C.byref(comb)) != 0
    assert L.spiral_gpu_fingerprint_of_polys(None, gp, 4, 0, 4, 0, 2, outp, C.byref(comb)) != 0
    assert L.spiral_gpu_fingerprint_of_polys(key, None, 4, 0, 4, 0, 2, outp, C.byref(comb)) != 0
    with pytest.raises(sa.SpiralGpuError, match="not below"):
        sa.fingerprint_of_polys(KEY, np.full((1, 4), P, dtype=np.uint64))
    with pytest.raises(ValueError, match="whole items"):
        sa.fingerprint_of_polys(KEY, np.zeros(7, dtype=np.uint64))
    with pytest.raises(TypeError, match="uint64"):
        sa.fingerprint_of_polys(KEY, np.zeros(8, dtype=np.int32))
    with pytest.raises(ValueError, match="key"):
        sa.fingerprint_of_polys((1, 2, 3), g)


def test_device_calls_fail_loudly(sa):
    """a null server is refused by every call, with a message; where there is no device, so is creating the server to track"""
    L = sa.lib()
    key = (C.c_uint64 * 2)(*KEY)
    w = (C.c_uint64 * 8)()
    bad = C.c_uint32(0)
    for pre in ("spiral_gpu_server", "spiral_gpu_pack_server"):
        calls = [(f"{pre}_fingerprint_track", (None, key, None)), (f"{pre}_fingerprint_untrack", (None,)), (f"{pre}_fingerprint_tracked", (None, w, w, w)),
                 (f"{pre}_fingerprint_tracked_polys", (None, 0, 1, w)), (f"{pre}_fingerprint_scrub", (None, 0, 1, w, w, C.byref(bad)))]
        for name, args in calls:
            assert getattr(L, name)(*args) != 0 and b"null server" in L.spiral_gpu_last_error(), name
    if L.spiral_gpu_device_count() == 0:
        with pytest.raises(sa.SpiralGpuError):
            sa.Server(sa.make_params(4, 3, t_gsw=8)).fingerprint_track(KEY)
        with pytest.raises(sa.SpiralGpuError):
            sa.PackServer(sa.make_params(6, 2), 2).fingerprint_track(KEY)
