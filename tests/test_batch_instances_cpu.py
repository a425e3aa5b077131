"""CPU-side checks of batched item queries (include/spiral_gpu.h spiral_gpu_server_run_query_batch_instances,
spiral_gpu_server_answer_batch_instances): the library exports both symbols, the Python wrappers exist, the argument checks that come before any
server is touched fail with a message, and ./spiral refuses bad --batch / --instances combinations before it looks for a device."""
import ctypes as C
import inspect
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")
NEW_SYMBOLS = ["spiral_gpu_server_run_query_batch_instances", "spiral_gpu_server_answer_batch_instances"]


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def test_new_symbols_exported_and_declared(sa):
    from spiral_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
    assert sa.lib().spiral_gpu_abi_version() == 1


def test_python_wrappers(sa):
    from spiral_amd import server as SV

    assert sa.run_query_batch_instances is SV.run_query_batch_instances
    assert sa.answer_batch_instances is SV.answer_batch_instances
    assert list(inspect.signature(SV.run_query_batch_instances).parameters) == ["servers", "instances", "responses_ptr", "finals_ptr", "wire_ptr", "pre"]
    assert list(inspect.signature(SV.answer_batch_instances).parameters) == ["servers", "instances", "queries", "wire"]


def fake_handles(n, base=0x1000):
    """pointers no check below may dereference: the calls must fail before touching a server"""
    return (C.c_void_p * n)(*[base + 0x100 * i for i in range(n)])


def test_argument_checks_fail_loudly(sa):
    L = sa.lib()
    out = C.c_void_p(0x5000)
    two = fake_handles(2)
    # no output
    assert L.spiral_gpu_server_run_query_batch_instances(two, 2, two, 2, 1, None, out, None) != 0
    assert b"no output" in L.spiral_gpu_last_error()
    # no servers / no instances
    assert L.spiral_gpu_server_run_query_batch_instances(None, 0, two, 2, 1, out, None, None) != 0
    assert b"no servers" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_server_run_query_batch_instances(two, 2, None, 0, 1, out, None, None) != 0
    assert b"no servers" in L.spiral_gpu_last_error()
    # more clients than lanes of one pass
    nine = fake_handles(9)
    assert L.spiral_gpu_server_run_query_batch_instances(nine, 9, two, 2, 1, out, None, out) != 0
    assert b"at most 8 clients" in L.spiral_gpu_last_error()
    # a null client
    holes = (C.c_void_p * 2)(None, None)
    assert L.spiral_gpu_server_run_query_batch_instances(holes, 2, two, 2, 1, out, None, None) != 0
    assert b"null server" in L.spiral_gpu_last_error()
    # host form: no queries, no output, too many clients
    qs = (C.POINTER(C.c_uint64) * 2)()
    assert L.spiral_gpu_server_answer_batch_instances(two, 2, two, 2, None, C.cast(out, C.POINTER(C.c_uint64)), None, None) != 0
    assert b"null queries" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_server_answer_batch_instances(two, 2, two, 2, qs, None, None, None) != 0
    assert b"no output" in L.spiral_gpu_last_error()
    assert L.spiral_gpu_server_answer_batch_instances(nine, 9, two, 2, (C.POINTER(C.c_uint64) * 9)(), None, out, None) != 0
    assert b"at most 8 clients" in L.spiral_gpu_last_error()


def test_graph_capture_counter_is_read_only(sa):
    v = C.c_int64(-1)
    assert sa.lib().spiral_gpu_get_option(b"graph_captures", C.byref(v)) == 0
    assert v.value >= 0
    assert sa.lib().spiral_gpu_set_option(b"graph_captures", 0) != 0


@pytest.mark.parametrize("flags", [
    ["--batch", "9", "--instances", "3"],
    ["--batch", "1", "--instances", "3"],
    ["--batch", "3", "--instances", "17"],
    ["--batch", "3", "--instances", "1"],
    ["--high-rate", "--batch", "2", "--instances", "2"],
])
def test_cli_rejects_bad_batch_instances_combinations(sa, flags):
    assert os.path.exists(BIN), "build() must produce spiral_amd/spiral"
    r = subprocess.run([BIN, "4", "2", "3", "a"] + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1
    assert "--batch B --instances F takes" in r.stderr, r.stderr
