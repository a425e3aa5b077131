"""CPU-side checks of the SpiralPack item entry points (include/spiral_gpu.h, spiral_gpu_pack_server_answer_batch_instances and its _wire form):
the library exports them, the header and the Python binding declare them, the checks that need no device fail with a message, and the Python
wrappers refuse bad argument lists before anything reaches the library."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["spiral_gpu_pack_server_answer_batch_instances", "spiral_gpu_pack_server_answer_batch_instances_wire"]
N = 2048


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
    """PackServer objects that never touched the library (handles no wrapper may pass on), with a real geometry: closed again whatever the test did"""
    made = []
    params = sa.make_params(6, 2)
    shape = P.get_pack_shape(params, 2)

    def make(k):
        for _ in range(k):
            s = P.PackServer.__new__(P.PackServer)
            s.h, s.out_n, s.params, s.shape = C.c_void_p(0x1000 + 16 * len(made)), 2, params, shape
            made.append(s)
        return made[-k:]

    yield make
    for s in made:
        s.h = None


def test_symbols_exported_and_declared(sa):
    from spiral_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "spiral_gpu.h")).read()
    for name in SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
        assert f"int {name}(" in header, name
    assert sa.pack_answer_instances is not None and sa.pack_answer_batch_instances is not None


def test_item_group_option(sa):
    L = sa.lib()
    v = C.c_int64()
    assert L.spiral_gpu_get_option(b"pack_item_group", C.byref(v)) == 0 and v.value == 0
    assert L.spiral_gpu_set_option(b"pack_item_group", 3) == 0
    assert L.spiral_gpu_get_option(b"pack_item_group", C.byref(v)) == 0 and v.value == 3
    assert L.spiral_gpu_set_option(b"pack_item_group", -1) != 0
    assert L.spiral_gpu_set_option(b"pack_item_group", 0) == 0


def _call(L, servers, n, instances, n_inst, queries, resp, wire):
    rc = L.spiral_gpu_pack_server_answer_batch_instances(servers, n, instances, n_inst, queries, resp, wire, None)
    assert rc != 0
    return L.spiral_gpu_last_error().decode()


def _call_wire(L, servers, n, instances, n_inst, queries, bytes_each, resp, wire):
    rc = L.spiral_gpu_pack_server_answer_batch_instances_wire(servers, n, instances, n_inst, queries, bytes_each, resp, wire, None)
    assert rc != 0
    return L.spiral_gpu_last_error().decode()


def test_checks_without_a_device(sa):
    """every check that needs no device fails with a message in spiral_gpu_last_error, before any handle is dereferenced (the arrays hold nulls)"""
    from spiral_amd._lib import U64P

    L = sa.lib()
    hs = (C.c_void_p * 9)()
    ins = (C.c_void_p * 2)()
    qbuf = np.zeros(8, dtype=np.uint64)
    qs = (U64P * 9)(*([qbuf.ctypes.data_as(U64P)] * 9))
    out = np.zeros(8, dtype=np.uint64)
    outp = out.ctypes.data_as(U64P)
    assert "null" in _call(L, None, 1, ins, 1, qs, outp, None)
    assert "null" in _call(L, hs, 1, None, 1, qs, outp, None)
    assert "null" in _call(L, hs, 1, ins, 1, None, outp, None)
    assert "no servers" in _call(L, hs, 0, ins, 1, qs, outp, None)
    assert "at most 8 clients" in _call(L, hs, 9, ins, 1, qs, outp, None)
    assert "no instances" in _call(L, hs, 1, ins, 0, qs, outp, None)
    assert "no output" in _call(L, hs, 1, ins, 1, qs, None, None)
    assert "null server 0" in _call(L, hs, 1, ins, 1, qs, outp, None)  # a null client handle
    wq = (C.c_void_p * 9)(*([qbuf.ctypes.data] * 9))
    assert "null" in _call_wire(L, None, 1, ins, 1, wq, 64, outp, None)
    assert "null" in _call_wire(L, hs, 1, ins, 1, None, 64, outp, None)
    assert "at most 8 clients" in _call_wire(L, hs, 9, ins, 1, wq, 64, outp, None)
    assert "no instances" in _call_wire(L, hs, 1, ins, 0, wq, 64, outp, None)
    assert "no output" in _call_wire(L, hs, 1, ins, 1, wq, 64, None, None)
    assert out.sum() == 0


def test_wrappers_reject_bad_argument_lists(P, fakes):
    a, b, i0, i1 = fakes(4)
    words = a.shape.n_query_cts * 2 * 2 * N
    q = np.zeros(words, dtype=np.uint64)
    with pytest.raises(ValueError, match="1 .. 8"):
        P.answer_batch_instances([], [i0], [])
    with pytest.raises(ValueError, match="1 .. 8"):
        P.answer_batch_instances(fakes(9), [i0], [q] * 9)
    with pytest.raises(ValueError, match="twice"):
        P.answer_batch_instances([a, a], [i0], [q, q])
    with pytest.raises(ValueError, match="no instances"):
        P.answer_batch_instances([a], [], [q])
    with pytest.raises(TypeError, match="instance"):
        P.answer_batch_instances([a], [i0, "not a server"], [q])
    with pytest.raises(ValueError, match="2 queries for 1"):
        P.answer_batch_instances([a], [i0, i1], [q, q])
    with pytest.raises(ValueError, match="1 queries for 2"):
        P.answer_batch_instances([a, b], [i0, i1], [q])
    with pytest.raises(TypeError, match="uint64"):
        P.answer_batch_instances([a], [i0], [q.astype(np.int64)])
    with pytest.raises(TypeError, match="uint64"):
        P.answer_instances(a, [i0, i1], q.astype(np.uint32))
    with pytest.raises(ValueError, match="words"):
        P.answer_instances(a, [i0, i1], q[:-1])
    with pytest.raises(ValueError, match="queries for"):
        P.answer_batch_instances_wire([a, b], [i0], [np.zeros(16, dtype=np.uint8)])
    with pytest.raises(TypeError):
        P.answer_instances_wire(a, [i0], np.zeros(16, dtype=np.uint64))
    with pytest.raises(ValueError, match="bytes"):
        P.answer_instances_wire(a, [i0], np.zeros(16, dtype=np.uint8))
    closed = fakes(1)[0]
    closed.h = None
    with pytest.raises(ValueError, match="closed"):
        P.answer_instances(a, [i0, closed], q)
