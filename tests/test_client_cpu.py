"""CPU-side checks of the client session (include/spiral_gpu.h spiral_gpu_client_*): every new symbol is declared, exported and bound, the noise
table is the closed form of csrc/client_device.h, a session cannot be created without a device, and the numpy restatement the GPU tests stand on
(tests/client_restated.py) is RFC 8439's block function and decodes what it encodes."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import client_restated as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = {  # name -> number of arguments
    "spiral_gpu_client_noise_table": 1, "spiral_gpu_client_create": 6, "spiral_gpu_client_destroy": 1, "spiral_gpu_client_get_secret": 3,
    "spiral_gpu_client_set_secret": 3, "spiral_gpu_client_decode": 5, "spiral_gpu_client_get_counter": 2, "spiral_gpu_client_set_counter": 2,
    "spiral_gpu_client_pub_params": 5, "spiral_gpu_client_pub_params_msg": 4, "spiral_gpu_client_queries": 6,
}
KEY = bytes(range(32))


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def test_new_symbols_exported_and_declared(sa):
    from spiral_amd import _lib, client

    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "spiral_gpu.h")).read()
    for name, nargs in NEW_SYMBOLS.items():
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == nargs, name
        assert name + "(" in header, name
    assert "enum spiral_gpu_response_form { SPIRAL_GPU_RESPONSE_RAW = 0, SPIRAL_GPU_RESPONSE_WIRE = 1 }" in header
    assert "client_device.h" in header, "the header names the one definition of the format"
    assert (client.RESPONSE_RAW, client.RESPONSE_WIRE) == (0, 1)
    assert sa.Client is client.Client and sa.client_noise_table is client.client_noise_table
    assert "#define SPIRAL_GPU_FORM_NTT 0" in header and "A MESSAGE NUMBER MUST NEVER BE USED FOR TWO DIFFERENT QUERIES" in header
    assert callable(sa.KeyStore.put_client) and isinstance(sa.Client.counter, property)
    for f in ("secret", "set_secret", "decode", "pub_params", "queries", "query"):
        assert callable(getattr(sa.Client, f)), f
    assert sa.lib().spiral_gpu_abi_version() == 1, "additive: the ABI version is unchanged"
    # the format's tags start at 16, clear of the seeded form's
    dev = open(os.path.join(ROOT, "spiral_amd", "csrc", "client_device.h")).read()
    assert "CLIENT_SECRET = 16, CLIENT_MSG_SEED = 17, CLIENT_NOISE_KEY = 18, CLIENT_NOISE = 19" in dev
    assert (R.D_SECRET, R.D_MSG_SEED, R.D_NOISE_KEY, R.D_NOISE) == (16, 17, 18, 19)


def test_noise_table_is_the_closed_form(sa):
    """non-decreasing, and within 2^16 of numpy's double-precision C_i / C_128 * 2^64: double arithmetic gives about 2^-50 relative error, 2^14
    absolute at 2^64, and two extra bits are margin"""
    T = [int(x) for x in sa.client_noise_table()]
    assert len(T) == 128 and all(a <= b for a, b in zip(T, T[1:]))
    want = R.noise_table_closed_form()
    for i in range(128):
        assert abs(T[i] - int(want[i])) <= 2**16, (i, T[i], int(want[i]))
    # the distribution it encodes is symmetric: P(v <= -1) + P(v <= 0) = 1, so T[63] + T[64] = 2^64 up to the roundings
    assert abs(T[63] + T[64] - 2**64) <= 4
    assert T[0] == 0 and T[127] == 2**64 - 1, "the tails round to 0 and to 1"
    assert sa.lib().spiral_gpu_client_noise_table(None) != 0 and "null" in sa.lib().spiral_gpu_last_error().decode()


def test_sampler_restated():
    """v = -64 + #{ i : T[i] <= u } on a table with ties and on the ends of the draw's range"""
    T = np.array([0] * 3 + list(range(10, 10 + 124)) + [2**64 - 1], dtype=np.uint64)
    for u, want in ((0, 3), (9, 3), (10, 4), (133, 127), (2**63, 127), (2**64 - 2, 127), (2**64 - 1, 128)):
        got = int(np.searchsorted(T, np.uint64(u), side="right"))
        assert got == want == sum(int(t) <= u for t in T), u


def test_create_needs_a_device(sa):
    """without a device create fails with a message and leaves *out null; with bad arguments it fails before it looks for one"""
    L = sa.lib()
    p = sa.make_params(4, 3, t_gsw=4)
    h = C.c_void_p(12345)
    assert L.spiral_gpu_client_create(C.byref(p), 0, 0, None, 0, C.byref(h)) != 0 and h.value is None
    assert "null" in L.spiral_gpu_last_error().decode()
    h = C.c_void_p(12345)
    assert L.spiral_gpu_client_create(C.byref(sa.make_params(4, 3, t_gsw=1)), 0, 0, KEY, 0, C.byref(h)) != 0 and h.value is None
    assert L.spiral_gpu_client_create(C.byref(p), 17, 0, KEY, 0, C.byref(h)) != 0 and h.value is None
    # q' of 2^31 and more: the device decode keeps row 0 in 32-bit words
    assert L.spiral_gpu_client_create(C.byref(sa.make_params(4, 3, t_gsw=4, qprime_bits=32)), 0, 0, KEY, 0, C.byref(h)) != 0 and h.value is None
    assert "exact range" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_client_create(C.byref(p), 0, 0, KEY, 0, None) != 0
    if L.spiral_gpu_device_count() == 0:
        h = C.c_void_p(12345)
        assert L.spiral_gpu_client_create(C.byref(p), 0, 0, KEY, 0, C.byref(h)) != 0 and h.value is None
        assert L.spiral_gpu_last_error().decode()
        with pytest.raises(sa.SpiralGpuError):
            sa.Client(p, KEY)
    with pytest.raises(ValueError, match="32 bytes"):
        sa.Client(p, bytes(31))
    # a null session is refused by name, without a device
    buf = np.zeros(2048, dtype=np.uint64)
    U = C.POINTER(C.c_uint64)
    for rc in (L.spiral_gpu_client_get_secret(None, buf.ctypes.data_as(U), None), L.spiral_gpu_client_set_secret(None, buf.ctypes.data_as(U), buf.ctypes.data_as(U)),
               L.spiral_gpu_client_decode(None, buf.ctypes.data_as(C.c_void_p), 1, 0, buf.ctypes.data_as(U))):
        assert rc != 0 and "null client session" in L.spiral_gpu_last_error().decode()
    L.spiral_gpu_client_destroy(None)


def test_restatement_is_rfc8439():
    """the restatement's block function passes the known answer of tests/test_seeded_input_cpu.py (RFC 8439 section 2.3.2), for several counters at once"""
    out = R.chacha20_blocks(KEY, [0, 1, 7], bytes.fromhex("000000090000004a00000000"))
    ser = struct.pack("<16I", *[int(x) for x in out[1]])
    assert ser[:16].hex() == "10f1e7e4d13b5915500fdd1fa32071c4"
    assert ser[-4:].hex() == "a2503c4e"
    assert not (out[0] == out[1]).all() and not (out[2] == out[1]).all()
    # and it agrees with the library's host expansion of a seeded row 0 (the same block function, another reading of the words)
    import spiral_amd as sa

    got = sa.seed_expand(KEY, 2, 479, 1)[0]
    w = [int(x) for x in R.chacha20_blocks(KEY, [5 >> 1], R.nonce(2, 479))[0]]
    h = 5 & 1
    assert int(got[0, 5]) == sum(w[8 * h + i] << (32 * i) for i in range(4)) % R.P
    assert int(got[1, 5]) == sum(w[8 * h + 4 + i] << (32 * i) for i in range(4)) % R.B


def test_restated_decode_recovers_what_it_encodes(sa):
    """valid_response and decode of the restatement are inverse, and the numpy wire packer is the library's format (response_from_wire, host code)"""
    rng = np.random.default_rng(11)
    T = sa.client_noise_table()
    for kw, out_n in ((dict(t_gsw=4), 0), (dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1), 3)):
        p = sa.make_params(5, 2, **kw)
        rows = cols = out_n or 2
        qprime = sa.get_pack_shape(p, out_n).qprime if out_n else sa.get_shape(p).qprime
        _, sp = R.secret(T, KEY, rows)
        assert sp.min() >= -64 and sp.max() <= 64 and sp.std() > 1.5, "samples of width 6.4 / sqrt(2 pi)"
        resp, m = R.valid_response(rng, sp, qprime, p.p_db, cols)
        assert (R.decode(sp, resp, qprime, p.p_db) == m).all()
        wire = R.response_to_wire(resp, p.qprime_bits, 10)
        assert wire.size == sa.response_wire_bytes(p, cols)
        assert (sa.response_from_wire(p, wire, cols) == resp).all()
