"""CPU-side checks of the batched SpiralPack entry points: the library exports them, the Python binding declares them, and the Python
wrappers refuse bad argument lists before anything reaches the library."""
import ctypes as C
import sys

import numpy as np
import pytest

NEW_SYMBOLS = [
    "spiral_gpu_pack_server_create_lane",
    "spiral_gpu_pack_server_answer_batch",
    "spiral_gpu_pack_server_set_db_format",
    "spiral_gpu_pack_server_db_format",
    "spiral_gpu_pack_server_db_device_bytes",
    "spiral_gpu_pack_server_time_sweep_batch",
]


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


@pytest.fixture(scope="module")
def P(sa):
    return sys.modules["spiral_amd.pack"]


@pytest.fixture
def fakes(P):
    """PackServer objects that never touched the library (a handle no wrapper may pass on): closed again whatever the test did"""
    made = []

    def make(k):
        for _ in range(k):
            s = P.PackServer.__new__(P.PackServer)
            s.h, s.out_n = C.c_void_p(0x1000 + 16 * len(made)), 2
            made.append(s)
        return made[-k:]

    yield make
    for s in made:
        s.h = None


def test_new_symbols_exported_and_declared(sa):
    from spiral_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
    assert sa.lib().spiral_gpu_pack_server_db_format(None) == -1
    assert sa.lib().spiral_gpu_pack_server_db_device_bytes(None) == 0


def test_null_arguments_fail_with_a_message(sa):
    L = sa.lib()
    out = C.c_void_p()
    assert L.spiral_gpu_pack_server_create_lane(None, C.byref(out)) != 0
    assert L.spiral_gpu_pack_server_answer_batch(None, 2, None, None, None, None) != 0
    assert b"no servers" in L.spiral_gpu_last_error()
    ms = C.c_float()
    assert L.spiral_gpu_pack_server_time_sweep_batch(None, 2, 1, C.byref(ms)) != 0
    assert L.spiral_gpu_pack_server_set_db_format(None, 1) != 0


def test_wrappers_reject_bad_argument_lists(P, fakes):
    q = np.zeros(8, dtype=np.uint64)
    with pytest.raises(ValueError, match="1 .. 8"):
        P.answer_batch([], [])
    nine = fakes(9)
    with pytest.raises(ValueError, match="1 .. 8"):
        P.answer_batch(nine, [q] * 9)
    a, b = fakes(2)
    with pytest.raises(ValueError, match="twice"):
        P.answer_batch([a, a], [q, q])
    with pytest.raises(ValueError, match="queries"):
        P.answer_batch([a, b], [q])
    with pytest.raises(TypeError):
        P.answer_batch([a, object()], [q, q])
    with pytest.raises(ValueError, match="iters"):
        P.time_sweep_batch([a, b], 0)
    with pytest.raises(ValueError, match="1 .. 8"):
        P.time_sweep_batch([], 3)
    b.h = None
    with pytest.raises(ValueError, match="closed"):
        P.answer_batch([a, b], [q, q])
