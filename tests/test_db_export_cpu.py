"""CPU-side checks of the database export (include/spiral_gpu.h spiral_gpu_db_items_bytes, spiral_gpu_server_read_db_items / _at,
spiral_gpu_pack_server_read_db_items / _at): the size function against its formula, the entry points exported, declared and bound with the
documented signatures, and the wrappers' argument checks, none of which needs a device."""
import ctypes as C
import inspect
import sys

import numpy as np
import pytest

N = 2048
READ_SYMBOLS = ["spiral_gpu_server_read_db_items", "spiral_gpu_server_read_db_items_at", "spiral_gpu_pack_server_read_db_items",
                "spiral_gpu_pack_server_read_db_items_at"]


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


@pytest.fixture(scope="module")
def P(sa):
    return sys.modules["spiral_amd.pack"]


def test_symbols_exported_and_declared(sa):
    from spiral_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in READ_SYMBOLS + ["spiral_gpu_db_items_bytes"]:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
    assert sa.lib().spiral_gpu_abi_version() == 1, "additive: the ABI version is unchanged"


def test_db_items_bytes_is_the_formula(sa):
    L = sa.lib()
    p256, p32k = sa.make_params(6, 6, t_gsw=8), sa.make_params(6, 6, t_gsw=8, p_db=1 << 15)
    # the item sizes the header cites for load_db_items
    assert L.spiral_gpu_db_items_bytes(C.byref(p256), 0, 8, 1) == 8192
    assert L.spiral_gpu_db_items_bytes(C.byref(p32k), 0, 15, 1) == 15360
    for p, p_db in ((p256, 256), (p32k, 1 << 15)):
        for out_n, polys in ((0, 4), (1, 1), (3, 1)):
            for bits in range(1, 65):
                for n in (0, 1, 7, 4096, 1 << 24):
                    got = L.spiral_gpu_db_items_bytes(C.byref(p), out_n, bits, n)
                    if bits < 64 and (1 << bits) < p_db:
                        assert got == 0 and b"coeff_bits" in L.spiral_gpu_last_error(), (p_db, bits)
                    else:
                        assert got == n * polys * 2048 * bits // 8, (p_db, out_n, bits, n)
    for bits in (0, 65, 1 << 20):
        assert L.spiral_gpu_db_items_bytes(C.byref(p256), 0, bits, 3) == 0
        assert b"coeff_bits" in L.spiral_gpu_last_error() and b"1..64" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_db_items_bytes(None, 0, 8, 1) == 0 and b"null" in L.spiral_gpu_last_error()
    # the Python form
    assert sa.db_items_bytes(p256, 8, 4096) == 32 << 20
    assert sa.db_items_bytes(p256, 64, 2, out_n=2) == 2 * 2048 * 8
    assert sa.db_items_bytes(p256, 8, 0) == 0
    for bits in (0, 7, 65):
        with pytest.raises((RuntimeError, ValueError), match="coeff_bits"):
            sa.db_items_bytes(p256, bits, 1)
    with pytest.raises((RuntimeError, ValueError), match="coeff_bits"):
        sa.db_items_bytes(p32k, 14, 1)


def test_python_binding_signatures(sa, P):
    from spiral_amd import server as SV

    def names(fn):
        return [(p.name, p.default) for p in inspect.signature(fn).parameters.values()]

    E = inspect.Parameter.empty
    assert names(SV.Server.read_db_items)[:4] == [("self", E), ("coeff_bits", E), ("first_item", 0), ("n_items", None)]
    assert names(SV.Server.read_db_items_at)[:3] == [("self", E), ("coeff_bits", E), ("ids", E)]
    assert names(P.PackServer.read_db_items)[:5] == [("self", E), ("trial", E), ("coeff_bits", E), ("first_item", 0), ("n_items", None)]
    assert names(P.PackServer.read_db_items_at)[:4] == [("self", E), ("trial", E), ("coeff_bits", E), ("ids", E)]
    assert names(sa.db_items_bytes) == [("params", E), ("coeff_bits", E), ("n_items", E), ("out_n", 0)]
    for fn in (SV.Server.read_db_items, SV.Server.read_db_items_at, P.PackServer.read_db_items, P.PackServer.read_db_items_at):
        assert all(d is None for _, d in names(fn)[len(names(fn)) - 1:]), "anything beyond the documented arguments is optional"


def test_null_handles_fail_with_a_message(sa):
    L = sa.lib()
    buf = np.full(8192, 0x5A, dtype=np.uint8)
    ids = (C.c_uint64 * 1)(0)
    assert L.spiral_gpu_server_read_db_items(None, buf.ctypes.data_as(C.c_void_p), 8, 0, 1) != 0 and b"null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_server_read_db_items_at(None, buf.ctypes.data_as(C.c_void_p), 8, ids, 1) != 0 and b"null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_pack_server_read_db_items(None, 0, buf.ctypes.data_as(C.c_void_p), 8, 0, 1) != 0 and b"null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_pack_server_read_db_items_at(None, 0, buf.ctypes.data_as(C.c_void_p), 8, ids, 1) != 0 and b"null" in L.spiral_gpu_last_error()
    assert (buf == 0x5A).all()


def test_wrappers_check_their_arguments(sa, P):
    """bad widths, id lists and output buffers are refused before a server handle is used (the fakes' handles must never reach the library)"""
    from spiral_amd import server as SV
    from spiral_amd._lib import read_args, read_ids

    pg = sa.make_params(6, 6, t_gsw=8)
    s = SV.Server.__new__(SV.Server)
    s.h, s.params = C.c_void_p(0x1000), pg
    ps = P.PackServer.__new__(P.PackServer)
    ps.h, ps.params, ps.out_n = C.c_void_p(0x2000), pg, 2
    try:
        for call in (lambda **kw: s.read_db_items_at(**kw), lambda **kw: ps.read_db_items_at(0, **kw)):
            with pytest.raises(TypeError, match="integers"):
                call(coeff_bits=8, ids=[1.5])
            with pytest.raises(TypeError, match="integers"):
                call(coeff_bits=8, ids=[True])
            with pytest.raises(ValueError, match="non-negative"):
                call(coeff_bits=8, ids=[3, -1])
            with pytest.raises(ValueError, match="flat"):
                call(coeff_bits=8, ids=[[1, 2]])
            with pytest.raises((RuntimeError, ValueError), match="coeff_bits"):
                call(coeff_bits=7, ids=[1])
            with pytest.raises(ValueError, match="out must be"):
                call(coeff_bits=8, ids=[1, 2], out=np.zeros(8192, dtype=np.uint8))
        with pytest.raises((RuntimeError, ValueError), match="coeff_bits"):
            s.read_db_items(65, 0, 1)
        with pytest.raises(ValueError, match="out must be"):
            s.read_db_items(8, 0, 2, out=np.zeros(2 * 8192, dtype=np.uint16))
        with pytest.raises(ValueError, match="out must be"):
            ps.read_db_items(0, 8, 0, 2, out=np.zeros((2, 4096), dtype=np.uint8)[:, :2048])
    finally:
        s.h = ps.h = None
    assert read_ids([5, 5, 2]).tolist() == [5, 5, 2] and read_ids([]).dtype == np.uint64  # duplicates and any order are fine
    assert read_args(pg, 13, 3, 0, None).size == 3 * 4 * 2048 * 13 // 8
    own = np.zeros(2 * 2048, dtype=np.uint8)
    assert read_args(pg, 8, 2, 1, own) is own
