"""CPU-side checks of set_query_batch / read_response_wire_batch (include/spiral_gpu.h, spiral_amd/server.py): the library exports and declares the
two symbols and the form enum, both calls fail loudly without a device, the Python wrappers refuse a wrong message count or form before they reach
the library, and ./spiral parses --query-batch before it looks for a device."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")
NEW_SYMBOLS = {"spiral_gpu_server_set_query_batch": 5, "spiral_gpu_server_read_response_wire_batch": 4}


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def test_new_symbols_exported_and_declared(sa):
    from spiral_amd import _lib, server

    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "spiral_gpu.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs and _lib.PROTOTYPES[name][0] is C.c_int, name
        assert name + "(" in header, name
    assert "enum spiral_gpu_message_form { SPIRAL_GPU_FORM_WIRE = 1, SPIRAL_GPU_FORM_SEEDED = 2 }" in header
    assert (_lib.FORM_NTT, _lib.FORM_WIRE, _lib.FORM_SEEDED) == (0, 1, 2)
    assert server.MESSAGE_FORMS == {"ntt": 0, "wire": 1, "seeded": 2}
    assert sa.set_query_batch is server.set_query_batch and sa.read_response_wire_batch is server.read_response_wire_batch
    sig = inspect.signature(sa.set_query_batch).parameters
    assert list(sig) == ["servers", "msgs", "form"] and sig["form"].default == "wire"
    assert list(inspect.signature(sa.read_response_wire_batch).parameters) == ["servers"]
    # the pass size of messages too large for the host's check: an option like the others, 1 at the least
    assert '"query_batch_chunk"' in header and sa.get_option("query_batch_chunk") == 512
    sa.set_option("query_batch_chunk", 1)
    assert sa.get_option("query_batch_chunk") == 1
    with pytest.raises(sa.SpiralGpuError, match="out of range"):
        sa.set_option("query_batch_chunk", 0)
    sa.set_option("query_batch_chunk", 512)


def test_fail_loudly_without_servers(sa):
    """no server can exist without a device: the list checks refuse a missing list, an empty one, nine entries and a null entry with a message, and
    dereference nothing"""
    L = sa.lib()
    msg = np.zeros(16, dtype=np.uint8)
    ptrs = (C.c_void_p * 9)(*[msg.ctypes.data] * 9)
    nulls = (C.c_void_p * 9)()
    out = np.zeros(16, dtype=np.uint8)
    for n, hs, err in ((1, None, "no servers"), (0, nulls, "no servers"), (9, nulls, "at most 8 clients"), (2, nulls, "null server 0")):
        assert L.spiral_gpu_server_set_query_batch(hs, n, 1, ptrs, 16) != 0
        assert "set_query_batch: " + err in L.spiral_gpu_last_error().decode()
        assert L.spiral_gpu_server_read_response_wire_batch(hs, n, out.ctypes.data_as(C.c_void_p), 16) != 0
        assert "read_response_wire_batch: " + err in L.spiral_gpu_last_error().decode()
    assert not out.any()


def test_wrappers_check_before_the_library(sa):
    class Fake:  # (never reaches the library: the wrapper's own checks come first)
        h = None

    with pytest.raises(ValueError, match="2 servers, 3 messages"):
        sa.set_query_batch([Fake(), Fake()], [b"a", b"b", b"c"])
    with pytest.raises(ValueError, match="'wire' or 'seeded'"):
        sa.set_query_batch([Fake()], [b"a"], form="packed")
    with pytest.raises(ValueError, match="'wire' or 'seeded'"):
        sa.set_query_batch([Fake()], [b"a"], form=1)
    with pytest.raises(ValueError, match="different sizes"):
        sa.set_query_batch([Fake(), Fake()], [b"ab", b"abc"])
    with pytest.raises(TypeError, match="uint8"):
        sa.set_query_batch([Fake()], [np.zeros(4, dtype=np.uint64)])
    with pytest.raises(sa.SpiralGpuError, match="null server 0"):  # (a well-formed call does reach it, and fails there by name)
        sa.set_query_batch([Fake()], [b"abcd"], form="seeded")
    with pytest.raises(sa.SpiralGpuError, match="no servers"):
        sa.read_response_wire_batch([])


def test_cli_parses_query_batch(sa):
    """--query-batch is taken by the argument parser (it announces itself, then looks for a device or runs); without a valid --batch, or with
    --instances / --high-rate, it is refused before that"""
    r = subprocess.run([BIN, "4", "3", "40", "a", "--batch", "3", "--query-batch"], capture_output=True, text=True, env=dict(os.environ, TGSW="4"), timeout=300)
    assert "Taking the batch's queries in one call and its responses in one read" in r.stdout, r.stdout + r.stderr
    assert "--query-batch takes" not in r.stderr
    assert r.returncode == 0 or "no ROCm device" in r.stderr, r.stdout[-1000:] + r.stderr
    for flags in (["--query-batch"], ["--batch", "9", "--query-batch"], ["--batch", "3", "--instances", "2", "--query-batch"],
                  ["--high-rate", "--batch", "3", "--query-batch", "--seeded"]):
        r = subprocess.run([BIN, "4", "3", "40", "a"] + flags, capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and "--query-batch takes" in r.stderr, (flags, r.stdout + r.stderr)
