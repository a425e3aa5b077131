"""The response noise of include/spiral_gpu.h (spiral_gpu_client_response_noise) restated in numpy and Python integers, independently of the library's
code: the error e of the switched forms and of the unswitched (FINAL) form, the six-word record, and builders of responses that carry a chosen
error.  Products are exact int64 convolutions -- per modulus q' as client_restated.negacyclic does, per 28-bit prime for the FINAL form -- and the
recombination mod Q is Python-integer CRT.  Shared by tests/test_response_noise_cpu.py, tests/test_gpu_response_noise.py and tests/test_cli_noise.py."""
import numpy as np

import client_restated as R

N, P, B, Q = R.N, R.P, R.B, R.Q
_CP = B * pow(B, -1, P)  # 1 mod P, 0 mod B
_CB = P * pow(P, -1, B)  # 0 mod P, 1 mod B


def product_mod_q(s, a) -> np.ndarray:
    """s * a in Z_Q[x] / (x^N + 1) for samples |s| <= 64 and 0 <= a < Q: one int64 convolution per prime (sums below 2048 * 64 * 2^28 < 2^46), then
    Python-integer CRT.  An object array of Python ints in [0, Q)"""
    a = np.asarray(a, dtype=np.uint64)
    xp = R.negacyclic(s, (a % np.uint64(P)).astype(np.int64)) % P
    xb = R.negacyclic(s, (a % np.uint64(B)).astype(np.int64)) % B
    return np.array([(int(x) * _CP + int(y) * _CB) % Q for x, y in zip(xp, xb)], dtype=object)


def switched_x(sp_r, row0, row, qprime: int, p_db: int) -> np.ndarray:
    """x = vf 4p + vr q' of one output polynomial, int64: decode's quantities"""
    q1 = 4 * p_db
    vf = R.negacyclic(sp_r, np.asarray(row0, dtype=np.uint64).astype(np.int64) % qprime) % qprime
    vf = np.where(vf >= qprime // 2, vf - qprime, vf)
    vr = np.asarray(row, dtype=np.uint64).astype(np.int64) % q1
    vr = np.where(vr >= q1 // 2, vr - q1, vr)
    return vf * q1 + vr * qprime


def switched_error(sp, resp, qprime: int, p_db: int, expected=None):
    """(e, plaintext), int64 and uint64 [rows][cols][N], of one switched response [(rows + 1)][cols][N]; plaintext is what decode returns"""
    sp, resp = np.asarray(sp, dtype=np.int64), np.asarray(resp, dtype=np.uint64)
    rows, cols = sp.shape[0], resp.shape[1]
    D = 4 * qprime
    span = p_db * D
    e = np.zeros((rows, cols, N), dtype=np.int64)
    pt = np.zeros((rows, cols, N), dtype=np.uint64)
    for r in range(rows):
        for c in range(cols):
            x = switched_x(sp[r], resp[0, c], resp[1 + r, c], qprime, p_db)
            res0 = np.sign(x) * ((np.abs(x) + D // 2) // D)  # round half away from zero
            pt[r, c] = (res0 % p_db).astype(np.uint64)
            if expected is None:
                e[r, c] = x - D * res0
            else:
                y = (x - D * np.asarray(expected, dtype=np.uint64)[r, c].astype(np.int64)) % span  # numpy's % of a positive modulus: in [0, span)
                e[r, c] = np.where(y >= span // 2, y - span, y)
    return e, pt


def final_error(sp, fin, p_db: int, expected=None):
    """(e, m0) of one unswitched ciphertext [(rows + 1)][cols][N] of raw values mod Q (a word is taken mod Q): e int64, m0 uint64"""
    sp, fin = np.asarray(sp, dtype=np.int64), np.asarray(fin, dtype=np.uint64) % np.uint64(Q)
    rows, cols = sp.shape[0], fin.shape[1]
    scale = Q // p_db
    e = np.zeros((rows, cols, N), dtype=np.int64)
    m0 = np.zeros((rows, cols, N), dtype=np.uint64)
    for c in range(cols):
        for r in range(rows):
            prod = product_mod_q(sp[r], fin[0, c]).astype(np.int64)
            v = (fin[1 + r, c].astype(np.int64) + prod) % Q  # everything from here on is below 2^57: int64 is exact
            m0[r, c] = ((v + scale // 2) // scale % p_db).astype(np.uint64)
            m = m0[r, c] if expected is None else np.asarray(expected, dtype=np.uint64)[r, c]
            d = (v - scale * m.astype(np.int64)) % Q
            e[r, c] = np.where(d >= Q // 2, d - Q, d)
    return e, m0


def record(e, n_wrong: int = 0) -> list:
    """the six words of one output polynomial's record, from Python-integer sums"""
    vals = [int(x) for x in np.asarray(e).reshape(-1)]
    s, sq = sum(vals) % (1 << 128), sum(x * x for x in vals)
    assert sq < 1 << 127
    return [max(abs(x) for x in vals), int(n_wrong), s & (2**64 - 1), s >> 64, sq & (2**64 - 1), sq >> 64]


def records(e, plaintext, expected=None) -> np.ndarray:
    """uint64 [rows][cols][6]: record() of every polynomial of one response; n_wrong counts plaintext != expected"""
    rows, cols = e.shape[:2]
    out = np.zeros((rows, cols, 6), dtype=np.uint64)
    for r in range(rows):
        for c in range(cols):
            wrong = 0 if expected is None else int((np.asarray(plaintext)[r, c] != np.asarray(expected, dtype=np.uint64)[r, c]).sum())
            out[r, c] = np.array(record(e[r, c], wrong), dtype=np.uint64)
    return out


def restate(form: str, sp, resp, qprime: int, p_db: int, expected=None):
    """(e, plaintext, records) of one response in `form` ("switched" or "final")"""
    e, pt = switched_error(sp, resp, qprime, p_db, expected) if form == "switched" else final_error(sp, resp, p_db, expected)
    return e, pt, records(e, pt, expected)


# ---- builders: a ciphertext or a response from a chosen (row 0, m, e) ------------------------------------------------------------------------------
def build_final(sp, row0, m, e, p_db: int) -> np.ndarray:
    """the unswitched ciphertext [(rows + 1)][cols][N] with row 0 = row0 [cols][N] whose v is scale_k m + e mod Q: rows 1.. = scale_k m + e - Sp_r * row 0"""
    sp = np.asarray(sp, dtype=np.int64)
    rows, cols = sp.shape[0], np.asarray(row0).shape[0]
    scale = Q // p_db
    fin = np.zeros((rows + 1, cols, N), dtype=np.uint64)
    fin[0] = row0
    for r in range(rows):
        for c in range(cols):
            prod = product_mod_q(sp[r], fin[0, c])
            fin[1 + r, c] = [(scale * int(m[r][c][k]) + int(e[r][c][k]) - prod[k]) % Q for k in range(N)]
    return fin


def build_switched(sp, row0, m, u, qprime: int, p_db: int):
    """(response, e): the switched response with row 0 = row0 [cols][N] (below q') and rows 1.. = 4 m - s + u mod 4p, s = round(4 p t / q') for the
    centred product t = Sp_r * row 0 mod q'.  Its x is 4 p t + q' (4 m - s + u) up to a multiple of p D, so against expected = m the error is
    e = 4 p t - q' s + q' u (returned, int64): the rounding of the product plus q' times the injected u, exact while |e| < p D / 2"""
    sp = np.asarray(sp, dtype=np.int64)
    rows, cols = sp.shape[0], np.asarray(row0).shape[0]
    resp = np.zeros((rows + 1, cols, N), dtype=np.uint64)
    resp[0] = row0
    e = np.zeros((rows, cols, N), dtype=np.int64)
    for r in range(rows):
        for c in range(cols):
            t = R.negacyclic(sp[r], resp[0, c].astype(np.int64)) % qprime
            t = np.where(t >= qprime // 2, t - qprime, t)
            s = (8 * p_db * t + qprime) // (2 * qprime)
            uu = np.asarray(u)[r, c].astype(np.int64)
            resp[1 + r, c] = ((4 * np.asarray(m)[r, c].astype(np.int64) - s + uu) % (4 * p_db)).astype(np.uint64)
            e[r, c] = 4 * p_db * t - qprime * s + qprime * uu
    return resp, e
