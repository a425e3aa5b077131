"""CPU-side checks of the wire form of what a client sends (include/spiral_gpu.h spiral_gpu_query_wire_bytes ... spiral_gpu_server_set_query_wire):
the library exports every new symbol, the client's half (raw_to_wire / raw_from_wire, plain host code) round-trips and pins the byte order, values
above Q are refused without writing anything, the sizes equal the figures the command line's summary prints, bad arguments fail with a message,
and ./spiral refuses --wire-input with bad --batch / --instances values before it looks for a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")
N = 2048
POLY = 7 * N
NEW_SYMBOLS = [
    "spiral_gpu_query_wire_bytes", "spiral_gpu_pub_params_wire_bytes", "spiral_gpu_pack_query_wire_bytes", "spiral_gpu_pack_pub_params_wire_bytes",
    "spiral_gpu_raw_to_wire", "spiral_gpu_raw_from_wire", "spiral_gpu_server_set_query_wire", "spiral_gpu_server_set_pub_params_wire",
    "spiral_gpu_pack_server_set_pub_params_wire", "spiral_gpu_pack_server_answer_wire", "spiral_gpu_pack_server_answer_batch_wire",
]
# bench.py's configs[1] .. [3] and the SpiralPack set of bench.py --workload pack (configs[4])
CONFIGS = {
    1: dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256),
    2: dict(nu1=9, nu2=10, t_gsw=10, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=22, p_db=256),
    3: dict(nu1=11, nu2=9, t_gsw=4, t_conv=56, t_exp=2, t_exp_right=56, qprime_bits=27, p_db=32768, direct_upload=1),
}
PACK4 = (dict(nu1=10, nu2=8, t_gsw=8, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=20, p_db=256), 4)


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def test_new_symbols_exported_and_declared(sa):
    from spiral_amd import _lib

    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "spiral_gpu.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
        assert name + "(" in header, name
    assert "SPIRAL_GPU_BUF_QUERY = 7" in header
    assert sa.lib().spiral_gpu_abi_version() == 1
    import sys

    from spiral_amd import server
    from spiral_amd import pack as _  # noqa: F401  (spiral_amd.pack is also a function's name: take the module)

    pack = sys.modules["spiral_amd.pack"]

    assert server.BUF_QUERY == 7
    for f in ("set_query_wire", "set_pub_params_wire"):
        assert callable(getattr(server.Server, f))
    for f in ("set_pub_params_wire", "answer_wire"):
        assert callable(getattr(pack.PackServer, f))
    assert callable(pack.answer_batch_wire)
    for f in ("raw_to_wire", "raw_from_wire", "query_wire_bytes", "pub_params_wire_bytes", "pack_query_wire_bytes", "pack_pub_params_wire_bytes"):
        assert callable(getattr(sa, f)), f


def test_round_trip_and_edges(sa):
    rng = np.random.default_rng(7)
    raw = rng.integers(0, sa.Q + 1, size=(5, N), dtype=np.uint64)
    edges = np.array([0, sa.P - 1, sa.B - 1, sa.Q, 1, sa.P, sa.B, sa.Q - 1], dtype=np.uint64)
    raw[0, : edges.size] = edges
    raw[4, -edges.size :] = edges
    w = sa.raw_to_wire(raw)
    assert w.dtype == np.uint8 and w.size == 5 * POLY
    back = sa.raw_from_wire(w)
    assert back.shape == (5, N) and (back == raw).all()
    assert (sa.raw_from_wire(bytes(w)) == raw).all()


def test_byte_order_pinned(sa):
    raw = np.zeros(N, dtype=np.uint64)
    raw[0] = 0x0102030405060708 & ((1 << 56) - 1)  # 0x02030405060708
    raw[1] = sa.Q
    raw[N - 1] = 0xABCDEF
    w = sa.raw_to_wire(raw)
    assert list(w[:7]) == [0x08, 0x07, 0x06, 0x05, 0x04, 0x03, 0x02]
    assert list(w[7:14]) == list(int(sa.Q).to_bytes(7, "little"))
    assert list(w[-7:]) == [0xEF, 0xCD, 0xAB, 0, 0, 0, 0]
    assert not w[14:-7].any()


@pytest.mark.parametrize("bad", ["q+1", "max"])
def test_above_q_refused_untouched(sa, bad):
    raw = np.ones((2, N), dtype=np.uint64)
    raw[1, 77] = sa.Q + 1 if bad == "q+1" else (1 << 56) - 1
    out = np.full(2 * POLY, 0x5A, dtype=np.uint8)
    rc = sa.lib().spiral_gpu_raw_to_wire(raw.ctypes.data_as(C.POINTER(C.c_uint64)), 2, out.ctypes.data_as(C.c_void_p))
    assert rc != 0
    msg = sa.lib().spiral_gpu_last_error().decode()
    assert "2125" in msg and "above Q" in msg, msg  # message-wide index 2048 + 77
    assert (out == 0x5A).all(), "raw_to_wire wrote into the output before refusing"
    with pytest.raises(sa.SpiralGpuError, match="above Q"):
        sa.raw_to_wire(raw)


def test_sizes_equal_summary(sa):
    b_per_elem = N * 56 // 8  # spiral_main.cpp's print_summary
    for k, kw in CONFIGS.items():
        p = sa.make_params(**kw)
        s = sa.get_shape(p)
        qnum = (1 << kw["nu1"]) + kw["t_gsw"] * kw["nu2"] if kw.get("direct_upload") else 1
        assert sa.query_wire_bytes(p) == qnum * 2 * b_per_elem, k  # "Total online query size"
        # client.cpp gen_pub_params' offline count, with V counted (the server takes it on every geometry)
        offline = (s.n_left * 2 * kw["t_exp"] + s.n_right * 2 * kw["t_exp_right"] + 2 * 3 * 2 * kw["t_conv"]) * b_per_elem
        assert sa.pub_params_wire_bytes(p) == offline, k
    assert sa.query_wire_bytes(sa.make_params(**CONFIGS[3])) == 59_752_448
    assert sa.pub_params_wire_bytes(sa.make_params(**CONFIGS[1])) == 976 * POLY
    kw, out_n = PACK4
    p = sa.make_params(**kw)
    s = sa.get_pack_shape(p, out_n)
    assert sa.pack_query_wire_bytes(p, out_n) == 2 * POLY
    assert sa.pack_pub_params_wire_bytes(p, out_n) == (s.n_left * 2 * 16 + s.n_right * 2 * 56 + 2 * 2 * 4 + out_n * (out_n + 1) * 4) * POLY
    # SpiralStreamPack (direct upload): the query's dim0 + 2 nu2 t_GSW ciphertexts, only v_W as public parameters
    ps = sa.make_params(8, 4, t_gsw=5, t_conv=4, t_exp=2, qprime_bits=20, p_db=256, direct_upload=1)
    assert sa.pack_query_wire_bytes(ps, 2) == (256 + 2 * 4 * 5) * 2 * POLY
    assert sa.pack_pub_params_wire_bytes(ps, 2) == 2 * 3 * 4 * POLY
    # refused parameters
    assert sa.query_wire_bytes(sa.make_params(8, 7, t_gsw=1)) == 0
    assert sa.pub_params_wire_bytes(sa.make_params(8, 7, qprime_bits=3)) == 0
    assert sa.pack_query_wire_bytes(p, 0) == 0 and sa.pack_pub_params_wire_bytes(p, 17) == 0
    assert sa.lib().spiral_gpu_query_wire_bytes(None) == 0
    assert sa.lib().spiral_gpu_pack_pub_params_wire_bytes(None, 2) == 0


def test_bad_arguments(sa):
    L = sa.lib()
    raw = np.zeros(N, dtype=np.uint64)
    w = np.zeros(POLY, dtype=np.uint8)
    U = C.POINTER(C.c_uint64)
    assert L.spiral_gpu_raw_to_wire(None, 1, w.ctypes.data_as(C.c_void_p)) != 0
    assert "null" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_raw_to_wire(raw.ctypes.data_as(U), 1, None) != 0
    assert L.spiral_gpu_raw_from_wire(None, 1, raw.ctypes.data_as(U)) != 0
    assert "null" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_raw_from_wire(w.ctypes.data_as(C.c_void_p), 1, None) != 0
    for f in ("spiral_gpu_server_set_query_wire", "spiral_gpu_server_set_pub_params_wire", "spiral_gpu_pack_server_set_pub_params_wire"):
        assert getattr(L, f)(None, w.ctypes.data_as(C.c_void_p), w.size) != 0, f
        assert "null" in L.spiral_gpu_last_error().decode(), f
    assert L.spiral_gpu_pack_server_answer_wire(None, w.ctypes.data_as(C.c_void_p), w.size, None, None, None) != 0
    assert L.spiral_gpu_pack_server_answer_batch_wire(None, 1, None, w.size, None, None, None) != 0
    assert "no servers" in L.spiral_gpu_last_error().decode()
    # short or ragged buffers are refused by the wrappers before the library sees them
    with pytest.raises(ValueError, match="whole polynomials"):
        sa.raw_from_wire(np.zeros(POLY - 1, dtype=np.uint8))
    with pytest.raises(ValueError, match="whole polynomials"):
        sa.raw_to_wire(np.zeros(N + 5, dtype=np.uint64))
    with pytest.raises(TypeError):
        sa.raw_from_wire(np.zeros(POLY, dtype=np.uint16))


@pytest.mark.parametrize("flags", [
    ["--wire-input", "--batch", "1"],
    ["--wire-input", "--batch", "9"],
    ["--wire-input", "--instances", "1"],
    ["--wire-input", "--instances", "17"],
    ["--wire-input", "--high-rate", "--instances", "3"],
])
def test_cli_refuses_bad_flags(sa, flags):
    r = subprocess.run([BIN, "4", "3", "40", "a"] + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "--wire-input takes" in r.stderr, r.stderr
