"""The client session's format (spiral_amd/csrc/client_device.h, include/spiral_gpu.h spiral_gpu_client_*) restated in numpy, independently of the
library's code: the ChaCha20 block function of RFC 8439 over arrays of blocks, the noise sampler, the secret key, the seeds and noise keys of the
session's messages, and check_final's decode in Python / int64 arithmetic.  Shared by tests/test_client_cpu.py and tests/test_gpu_client.py; the only
thing taken from the library is the threshold table (spiral_amd.client_noise_table), which the CPU test checks against its closed form."""
import struct

import numpy as np

N = 2048
P = 268369921
B = 249561089
Q = P * B
D_SECRET, D_MSG_SEED, D_NOISE_KEY, D_NOISE = 16, 17, 18, 19


def _rotl(x, n):
    return (x << np.uint32(n)) | (x >> np.uint32(32 - n))


def _qr(s, a, b, c, d):
    s[a] = s[a] + s[b]; s[d] = _rotl(s[d] ^ s[a], 16)  # noqa: E702
    s[c] = s[c] + s[d]; s[b] = _rotl(s[b] ^ s[c], 12)  # noqa: E702
    s[a] = s[a] + s[b]; s[d] = _rotl(s[d] ^ s[a], 8)  # noqa: E702
    s[c] = s[c] + s[d]; s[b] = _rotl(s[b] ^ s[c], 7)  # noqa: E702


def chacha20_blocks(key: bytes, counters, nonce: bytes) -> np.ndarray:
    """the ChaCha20 block function (RFC 8439 section 2.3) for every block counter of `counters` under one key and 12-byte nonce: uint32 [len][16]"""
    counters = np.asarray(counters, dtype=np.uint32).reshape(-1)
    const = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, *struct.unpack("<8I", key), 0, *struct.unpack("<3I", nonce)]
    st = [np.full(counters.shape, c, dtype=np.uint32) for c in const]
    st[12] = counters.copy()
    w = [x.copy() for x in st]
    with np.errstate(over="ignore"):
        for _ in range(10):
            _qr(w, 0, 4, 8, 12); _qr(w, 1, 5, 9, 13); _qr(w, 2, 6, 10, 14); _qr(w, 3, 7, 11, 15)  # noqa: E702
            _qr(w, 0, 5, 10, 15); _qr(w, 1, 6, 11, 12); _qr(w, 2, 7, 8, 13); _qr(w, 3, 4, 9, 14)  # noqa: E702
        return np.stack([a + b for a, b in zip(w, st)], axis=1)


def nonce(domain: int, i: int) -> bytes:
    return struct.pack("<IQ", domain, i)


def noise_table_closed_form() -> np.ndarray:
    """C_i / C_128 * 2^64 in double precision (about 2^-50 relative: 2^14 absolute)"""
    j = np.arange(-64, 65, dtype=np.float64)
    c = np.cumsum(np.exp(-np.pi * j * j / (6.4 * 6.4)))
    return c[:128] / c[128] * 2.0**64


def noise_poly(table, key: bytes, domain: int, i: int, nonoise: bool = False) -> np.ndarray:
    """noise polynomial i under noise key `key` and domain tag `domain`: the 2048 samples v in [-64, 64] as int64"""
    if nonoise:
        return np.zeros(N, dtype=np.int64)
    w = chacha20_blocks(key, np.arange(N // 8), nonce(domain, i)).astype(np.uint64)  # block z >> 3 holds coefficients 8 (z >> 3) ..
    u = (w[:, 0::2] | (w[:, 1::2] << np.uint64(32))).reshape(-1)  # coefficient z: words 2 (z & 7), 2 (z & 7) + 1
    return np.searchsorted(np.asarray(table, dtype=np.uint64), u, side="right").astype(np.int64) - 64  # -64 + #{ i : T[i] <= u }


def raw_of(v) -> np.ndarray:
    """samples -> raw values mod Q"""
    v = np.asarray(v, dtype=np.int64)
    return np.where(v < 0, v + Q, v).astype(np.uint64)


def centred(raw) -> np.ndarray:
    raw = np.asarray(raw, dtype=np.uint64).astype(np.int64)
    return np.where(raw >= Q // 2, raw - Q, raw)


def secret(table, K: bytes, rows: int, nonoise: bool = False):
    """(sr, Sp [rows]) as samples: noise polynomials 0 and 1.. under K itself with the secret's tag"""
    return noise_poly(table, K, D_SECRET, 0, nonoise), np.stack([noise_poly(table, K, D_SECRET, 1 + r, nonoise) for r in range(rows)])


def message_seed(K: bytes, n: int) -> bytes:
    return chacha20_blocks(K, [0], nonce(D_MSG_SEED, n))[0, :8].astype("<u4").tobytes()


def message_noise_key(K: bytes, n: int) -> bytes:
    return chacha20_blocks(K, [0], nonce(D_NOISE_KEY, n))[0, :8].astype("<u4").tobytes()


def negacyclic(s, a) -> np.ndarray:
    """s * a in Z[x] / (x^N + 1), int64 (|s| <= 64, 0 <= a < 2^31: every sum below 2^48)"""
    full = np.convolve(np.asarray(s, dtype=np.int64), np.asarray(a, dtype=np.int64))
    out = full[:N].copy()
    out[: N - 1] -= full[N:]
    return out


def decode(sp, resp, qprime: int, p_db: int) -> np.ndarray:
    """check_final's client half (src/spiral.cpp:1451-1491, src/testing.cpp:1086-1122): sp = the samples of Sp [rows][N], resp = the switched response
    [(rows + 1)][cols][N] -> the plaintexts [rows][cols][N]"""
    sp, resp = np.asarray(sp, dtype=np.int64), np.asarray(resp, dtype=np.uint64).astype(np.int64)
    rows, cols = sp.shape[0], resp.shape[1]
    q1, denom = 4 * p_db, qprime * 4
    out = np.zeros((rows, cols, N), dtype=np.uint64)
    for r in range(rows):
        for c in range(cols):
            vf = negacyclic(sp[r], resp[0, c] % qprime) % qprime  # to_ntt_qprime's product, in [0, q')
            vf = np.where(vf >= qprime // 2, vf - qprime, vf)
            vr = resp[1 + r, c]
            vr = np.where(vr >= q1 // 2, vr - q1, vr)
            x = vf * q1 + vr * qprime
            res = np.sign(x) * ((np.abs(x) + denom // 2) // denom)  # (x + sign * denom / 2) / denom, truncated
            out[r, c] = (res % p_db).astype(np.uint64)
    return out


def valid_response(rng, sp, qprime: int, p_db: int, cols: int):
    """a response that decodes: a uniform row 0, chosen plaintexts m, and rows 1.. = 4 m - round(4 p t / q') + e with t the centred product Sp_r * row 0
    and |e| <= 1 -- the rounding error stays below 1/8 + 1/4.  Returns (response, m)"""
    sp = np.asarray(sp, dtype=np.int64)
    rows = sp.shape[0]
    resp = np.zeros((rows + 1, cols, N), dtype=np.uint64)
    resp[0] = rng.integers(0, qprime, size=(cols, N), dtype=np.uint64)
    m = rng.integers(0, p_db, size=(rows, cols, N), dtype=np.int64)
    for r in range(rows):
        for c in range(cols):
            t = negacyclic(sp[r], resp[0, c].astype(np.int64)) % qprime
            t = np.where(t >= qprime // 2, t - qprime, t)
            scaled = (8 * p_db * t + qprime) // (2 * qprime)  # round(4 p t / q'), floor division of the doubled fraction
            resp[1 + r, c] = ((4 * m[r, c] - scaled + rng.integers(-1, 2, size=N)) % (4 * p_db)).astype(np.uint64)
    return resp, m.astype(np.uint64)


def response_to_wire(resp, w0: int, w1: int) -> np.ndarray:
    """the bit stream of a switched response (include/spiral_gpu.h spiral_gpu_response_wire_bytes): row 0 at w0 bits per coefficient, then the other rows
    at w1, little-endian bit order"""
    resp = np.asarray(resp, dtype=np.uint64)

    def bits(v, w):
        return ((v.reshape(-1, 1) >> np.arange(w, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).reshape(-1)

    return np.packbits(np.concatenate([bits(resp[0], w0), bits(resp[1:], w1)]), bitorder="little")
