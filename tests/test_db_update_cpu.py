"""CPU-side checks of the in-place item update (include/spiral_gpu.h spiral_gpu_server_update_db_items, spiral_gpu_pack_server_update_db_items):
the library exports both symbols, the Python binding declares them, and the wrappers refuse bad argument lists before anything reaches the
library."""
import ctypes as C
import sys

import numpy as np
import pytest

N = 2048
NEW_SYMBOLS = ["spiral_gpu_server_update_db_items", "spiral_gpu_pack_server_update_db_items"]


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


@pytest.fixture(scope="module")
def P(sa):
    return sys.modules["spiral_amd.pack"]


@pytest.fixture
def fakes(sa, P):
    """a Server and a PackServer that never touched the library (a handle no wrapper may pass on): closed again whatever the test did"""
    from spiral_amd import server as SV

    s = SV.Server.__new__(SV.Server)
    s.h = C.c_void_p(0x1000)
    ps = P.PackServer.__new__(P.PackServer)
    ps.h, ps.out_n = C.c_void_p(0x2000), 2
    yield s, ps
    s.h = ps.h = None


def test_new_symbols_exported_and_declared(sa):
    from spiral_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
    assert sa.lib().spiral_gpu_abi_version() == 1


def test_null_server_fails_with_a_message(sa):
    L = sa.lib()
    ids = (C.c_uint64 * 1)(0)
    item = np.zeros(4 * N, dtype=np.uint8)
    assert L.spiral_gpu_server_update_db_items(None, item.ctypes.data_as(C.c_void_p), 8, ids, 1) != 0
    assert b"null" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_pack_server_update_db_items(None, 0, item.ctypes.data_as(C.c_void_p), 8, ids, 1) != 0
    assert b"null" in L.spiral_gpu_last_error()


@pytest.mark.parametrize("which", ["base", "pack"])
def test_wrappers_reject_bad_argument_lists(fakes, which):
    s, ps = fakes
    polys = 4 if which == "base" else 1
    call = s.update_db_items if which == "base" else (lambda items, bits, ids: ps.update_db_items(0, items, bits, ids))
    two = np.zeros(2 * polys * N, dtype=np.uint8)  # two plaintexts of 8-bit coefficients
    with pytest.raises(ValueError, match="bytes"):
        call(two, 8, [1])  # two items for one id
    with pytest.raises(ValueError, match="bytes"):
        call(two, 8, [1, 2, 3])
    with pytest.raises(ValueError, match="bytes"):
        call(two, 16, [1, 2])  # the same bytes read as 16-bit coefficients are one item
    with pytest.raises(ValueError, match="duplicate"):
        call(two, 8, [5, 5])
    with pytest.raises(TypeError, match="integers"):
        call(two, 8, [1.0, 2.0])
    with pytest.raises(TypeError, match="integers"):
        call(two, 8, [True, False])
    with pytest.raises(TypeError, match="integers"):
        call(two, 8, ["1", "2"])
    with pytest.raises(ValueError, match="non-negative"):
        call(two, 8, [-1, 2])
    with pytest.raises(ValueError, match="flat"):
        call(two, 8, [[1, 2]])
    with pytest.raises(TypeError, match="coeff_bits"):
        call(two, 8.0, [1, 2])


def test_update_args_accepts_a_good_list():
    from spiral_amd._lib import update_args

    items, ids = update_args(np.zeros((3, 4 * N), dtype=np.uint8), 8, np.array([7, 0, 9], dtype=np.int32), 4)
    assert ids.dtype == np.uint64 and ids.tolist() == [7, 0, 9] and items.flags["C_CONTIGUOUS"]
    items, ids = update_args(np.zeros(N, dtype=np.uint64), 64, [3], 1)
    assert ids.tolist() == [3]
    items, ids = update_args(np.zeros(0, dtype=np.uint8), 8, [], 4)
    assert ids.size == 0 and ids.dtype == np.uint64
