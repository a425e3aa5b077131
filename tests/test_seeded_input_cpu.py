"""CPU-side checks of the seeded form of what a client sends (include/spiral_gpu.h spiral_gpu_query_seeded_bytes ... spiral_gpu_seed_expand): the
library exports and declares every new symbol, the client's row-0 expansion (plain host code) matches RFC 8439's ChaCha20 and the known answers of
the format, a pure-Python restatement of the format agrees with it, every residue is reduced, the sizes are the figures the format gives, and
./spiral refuses --seeded wherever it refuses --wire-input, before it looks for a device."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")
N = 2048
P = 268369921
B = 249561089
POLY = 7 * N
NEW_SYMBOLS = [
    "spiral_gpu_query_seeded_bytes", "spiral_gpu_pub_params_seeded_bytes", "spiral_gpu_pack_query_seeded_bytes", "spiral_gpu_pack_pub_params_seeded_bytes",
    "spiral_gpu_seed_expand", "spiral_gpu_server_set_query_seeded", "spiral_gpu_server_set_pub_params_seeded",
    "spiral_gpu_pack_server_set_pub_params_seeded", "spiral_gpu_pack_server_answer_seeded", "spiral_gpu_pack_server_answer_batch_seeded",
    "spiral_gpu_pack_server_answer_batch_instances_seeded",
]
CONFIGS = {  # bench.py's configs[1] and [3]
    1: dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256),
    3: dict(nu1=11, nu2=9, t_gsw=4, t_conv=56, t_exp=2, t_exp_right=56, qprime_bits=27, p_db=32768, direct_upload=1),
}
KEY = bytes(range(32))
KNOWN = {(1, 0, 0): (152493557, 59619473), (1, 0, 1): (109008191, 25025367), (1, 0, 2047): (202971876, 225615871),
         (2, 479, 5): (226054267, 34976987), (4, 3, 1024): (143898211, 105262535)}


# ---- the format, restated in Python -------------------------------------------------------------------------------------------------------
def _rotl(x, n):
    return ((x << n) | (x >> (32 - n))) & 0xFFFFFFFF


def _qr(s, a, b, c, d):
    s[a] = (s[a] + s[b]) & 0xFFFFFFFF; s[d] = _rotl(s[d] ^ s[a], 16)  # noqa: E702
    s[c] = (s[c] + s[d]) & 0xFFFFFFFF; s[b] = _rotl(s[b] ^ s[c], 12)  # noqa: E702
    s[a] = (s[a] + s[b]) & 0xFFFFFFFF; s[d] = _rotl(s[d] ^ s[a], 8)  # noqa: E702
    s[c] = (s[c] + s[d]) & 0xFFFFFFFF; s[b] = _rotl(s[b] ^ s[c], 7)  # noqa: E702


def chacha20_block(key, counter, nonce):
    st = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, *struct.unpack("<8I", key), counter, *struct.unpack("<3I", nonce)]
    w = list(st)
    for _ in range(10):
        _qr(w, 0, 4, 8, 12); _qr(w, 1, 5, 9, 13); _qr(w, 2, 6, 10, 14); _qr(w, 3, 7, 11, 15)  # noqa: E702
        _qr(w, 0, 5, 10, 15); _qr(w, 1, 6, 11, 12); _qr(w, 2, 7, 8, 13); _qr(w, 3, 4, 9, 14)  # noqa: E702
    return [(a + b) & 0xFFFFFFFF for a, b in zip(w, st)]


def residues(seed, d, k, z):
    w = chacha20_block(seed, z >> 1, struct.pack("<IQ", d, k))
    h = z & 1
    x = sum(w[8 * h + i] << (32 * i) for i in range(4))
    y = sum(w[8 * h + 4 + i] << (32 * i) for i in range(4))
    return x % P, y % B


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def test_new_symbols_exported_and_declared(sa):
    import sys

    from spiral_amd import _lib, server
    from spiral_amd import pack as _  # noqa: F401

    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "spiral_gpu.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), name
        assert name in _lib.PROTOTYPES, name
        assert name + "(" in header, name
    assert "MUST BE FRESH FOR EVERY QUERY" in header
    assert sa.lib().spiral_gpu_abi_version() == 1
    pack = sys.modules["spiral_amd.pack"]
    for f in ("set_query_seeded", "set_pub_params_seeded"):
        assert callable(getattr(server.Server, f))
    for f in ("set_pub_params_seeded", "answer_seeded"):
        assert callable(getattr(pack.PackServer, f))
    assert callable(pack.answer_batch_seeded) and callable(pack.answer_batch_instances_seeded)
    for f in ("seed_expand", "query_seeded_bytes", "pub_params_seeded_bytes", "pack_query_seeded_bytes", "pack_pub_params_seeded_bytes"):
        assert callable(getattr(sa, f)), f


def test_rfc8439_block():
    """the restatement's block function is RFC 8439 section 2.3.2's"""
    out = struct.pack("<16I", *chacha20_block(KEY, 1, bytes.fromhex("000000090000004a00000000")))
    assert out[:16].hex() == "10f1e7e4d13b5915500fdd1fa32071c4"
    assert out[-4:].hex() == "a2503c4e"  # (the last bytes of the RFC's serialized block)


def test_known_answers(sa):
    for (d, k, z), want in KNOWN.items():
        got = sa.seed_expand(KEY, d, k, 1)
        assert got.shape == (1, 2, N)
        assert (int(got[0, 0, z]), int(got[0, 1, z])) == want, (d, k, z)
        assert residues(KEY, d, k, z) == want, (d, k, z)
    # first_k offsets the numbering: polynomial 479 of a run that starts at 470
    assert (sa.seed_expand(KEY, 2, 470, 12)[9] == sa.seed_expand(KEY, 2, 479, 1)[0]).all()
    # the RFC's own vector through the host function: nonce 00 00 00 09 | 00 00 00 4a 00 00 00 00 is d = 0x09000000, k = 0x4a000000, and block 1
    # gives slots 2 (bytes 0..31 of the serialized block) and 3 (bytes 32..63)
    rfc = bytes.fromhex("10f1e7e4d13b5915500fdd1fa32071c4c7d1f4c733c068030422aa9ac3d46c4e"
                        "d2826446079faa0914c2d705d98b02a2b5129cd1de164eb9cbd083e8a2503c4e")
    got = sa.seed_expand(KEY, 0x09000000, 0x4A000000, 1)[0]
    for h in range(2):
        x = int.from_bytes(rfc[32 * h:32 * h + 16], "little") % P
        y = int.from_bytes(rfc[32 * h + 16:32 * h + 32], "little") % B
        assert (int(got[0, 2 + h]), int(got[1, 2 + h])) == (x, y), h


def test_python_restatement_agrees(sa):
    rng = np.random.default_rng(8439)
    for _ in range(40):
        seed = rng.integers(0, 256, size=32, dtype=np.uint8).tobytes()
        d = int(rng.integers(1, 5)) if rng.random() < 0.8 else int(rng.integers(0, 1 << 32))
        k = int(rng.integers(0, 1 << 20)) if rng.random() < 0.8 else int(rng.integers(0, 1 << 63))
        got = sa.seed_expand(seed, d, k, 1)[0]
        for z in rng.integers(0, N, size=6):
            assert (int(got[0, z]), int(got[1, z])) == residues(seed, d, k, int(z)), (d, k, int(z))


def test_residues_reduced_and_spread(sa):
    seed = bytes(range(100, 132))
    x = sa.seed_expand(seed, 2, 0, 64)
    assert (x[:, 0] < P).all() and (x[:, 1] < B).all()
    # uniform residues: the mean is near m / 2 and neither field repeats a whole polynomial
    assert abs(x[:, 0].mean() / P - 0.5) < 0.01 and abs(x[:, 1].mean() / B - 0.5) < 0.01
    assert len({x[i, 0].tobytes() for i in range(64)}) == 64
    # other seed, domain or k: other polynomials
    a = sa.seed_expand(seed, 1, 0, 1)
    assert not (a == sa.seed_expand(seed, 2, 0, 1)).all() and not (a == sa.seed_expand(seed, 1, 1, 1)).all()
    assert not (a == sa.seed_expand(bytes(32), 1, 0, 1)).all()


def test_sizes(sa):
    p1, p3 = sa.make_params(**CONFIGS[1]), sa.make_params(**CONFIGS[3])
    assert sa.query_seeded_bytes(p1) == 14_368
    assert sa.pub_params_seeded_bytes(p1) == 7_110_688
    assert sa.query_seeded_bytes(p3) == 29_876_256
    # 32 + (wire polynomials - row-0 polynomials) x 14 336
    s = sa.get_shape(p1)
    row0 = s.n_left * 8 + s.n_right * 56 + 2 * 2 * 4
    assert row0 == 480 and sa.pub_params_wire_bytes(p1) == 976 * POLY
    assert sa.pub_params_seeded_bytes(p1) == 32 + (976 - 480) * POLY
    for p in (p1, p3):
        assert sa.query_seeded_bytes(p) == 32 + sa.query_wire_bytes(p) // 2
    # SpiralPack: compressed (expansion keys, V, v_W) and streaming (v_W only)
    pk = sa.make_params(10, 8, t_gsw=8, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=20, p_db=256)
    ps = sa.get_pack_shape(pk, 4)
    assert sa.pack_query_seeded_bytes(pk, 4) == 32 + POLY
    assert sa.pack_pub_params_seeded_bytes(pk, 4) == 32 + (ps.n_left * 16 + ps.n_right * 56 + 2 * 4 + 4 * 4 * 4) * POLY
    pst = sa.make_params(8, 4, t_gsw=5, t_conv=4, t_exp=2, qprime_bits=20, p_db=256, direct_upload=1)
    assert sa.pack_query_seeded_bytes(pst, 2) == 32 + (256 + 2 * 4 * 5) * POLY
    assert sa.pack_pub_params_seeded_bytes(pst, 2) == 32 + 2 * 2 * 4 * POLY
    # refused parameters
    assert sa.query_seeded_bytes(sa.make_params(8, 7, t_gsw=1)) == 0
    assert sa.pub_params_seeded_bytes(sa.make_params(8, 7, qprime_bits=3)) == 0
    assert sa.pack_query_seeded_bytes(pk, 0) == 0 and sa.pack_pub_params_seeded_bytes(pk, 17) == 0
    assert sa.lib().spiral_gpu_query_seeded_bytes(None) == 0
    assert sa.lib().spiral_gpu_pack_pub_params_seeded_bytes(None, 2) == 0


def test_bad_arguments(sa):
    L = sa.lib()
    out = np.zeros((1, 2, N), dtype=np.uint64)
    U = C.POINTER(C.c_uint64)
    assert L.spiral_gpu_seed_expand(None, 1, 0, 1, out.ctypes.data_as(U)) != 0
    assert "null" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_seed_expand(KEY, 1, 0, 1, None) != 0
    w = np.zeros(32 + POLY, dtype=np.uint8)
    for f in ("spiral_gpu_server_set_query_seeded", "spiral_gpu_server_set_pub_params_seeded", "spiral_gpu_pack_server_set_pub_params_seeded"):
        assert getattr(L, f)(None, w.ctypes.data_as(C.c_void_p), w.size) != 0, f
        assert "null" in L.spiral_gpu_last_error().decode(), f
    assert L.spiral_gpu_pack_server_answer_seeded(None, w.ctypes.data_as(C.c_void_p), w.size, None, None, None) != 0
    assert L.spiral_gpu_pack_server_answer_batch_seeded(None, 1, None, w.size, None, None, None) != 0
    assert L.spiral_gpu_pack_server_answer_batch_instances_seeded(None, 1, None, 1, None, w.size, None, None, None) != 0
    with pytest.raises(ValueError, match="32 bytes"):
        sa.seed_expand(bytes(31), 1, 0, 1)


@pytest.mark.parametrize("flags", [
    ["--batch", "1"],
    ["--batch", "9"],
    ["--instances", "1"],
    ["--instances", "17"],
    ["--high-rate", "--instances", "3"],
])
def test_cli_refuses_bad_flags(sa, flags):
    r = subprocess.run([BIN, "4", "3", "40", "a", "--seeded"] + flags, capture_output=True, text=True, timeout=60)
    assert r.returncode == 1, r.stdout + r.stderr
    assert "--seeded takes" in r.stderr, r.stderr
