"""CPU-side checks of the response noise (include/spiral_gpu.h spiral_gpu_client_response_noise): the symbol is declared, exported and bound, a null
session is refused without a device, the numpy restatement the GPU tests stand on (tests/noise_restated.py) recovers errors it injected, in both
forms and at the ends of the centred range, and scheme.response_noise_model returns the denominator of p_err_log2."""
import ctypes as C
import json
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import client_restated as R  # noqa: E402
import noise_restated as NR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, Q = R.N, R.Q


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


def test_symbol_exported_declared_and_bound(sa):
    from spiral_amd import _lib, client

    name = "spiral_gpu_client_response_noise"
    raw = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "spiral_gpu.h")).read()
    assert hasattr(raw, name)
    assert name in _lib.PROTOTYPES and len(_lib.PROTOTYPES[name][1]) == 7
    assert name + "(" in header
    assert "SPIRAL_GPU_RESPONSE_FINAL = 2" in header
    assert client.RESPONSE_FINAL == 2
    assert sa.lib().spiral_gpu_abi_version() == 1, "additive: the ABI version is unchanged"
    assert callable(sa.Client.response_noise) and sa.ResponseNoise is client.ResponseNoise
    for f in ("variance", "budget_bits", "width2"):
        assert callable(getattr(sa.ResponseNoise, f)), f


def test_null_session_is_refused_without_a_device(sa):
    L = sa.lib()
    buf = np.full(8, 77, dtype=np.uint64)
    err = np.full(8, 77, dtype=np.int64)
    rc = L.spiral_gpu_client_response_noise(None, buf.ctypes.data_as(C.c_void_p), 1, 0, None, buf.ctypes.data_as(C.POINTER(C.c_uint64)),
                                            err.ctypes.data_as(C.POINTER(C.c_int64)))
    assert rc != 0 and "client_response_noise: null client session" in L.spiral_gpu_last_error().decode()
    assert (buf == 77).all() and (err == 77).all()


def test_record_words():
    """Python-integer sums, two's complement for the signed one"""
    assert NR.record([3, -5, 1]) == [5, 0, 2**64 - 1, 2**64 - 1, 35, 0]
    big = 2**57
    rec = NR.record([big] * 2048 + [-1], 7)
    assert rec[0] == big and rec[1] == 7
    assert rec[2] + (rec[3] << 64) == 2048 * big - 1 and rec[4] + (rec[5] << 64) == 2048 * big * big + 1


def test_response_noise_object_is_exact(sa):
    """sum and sumsq are exact Python ints, the variance comes from them, the budget from max_abs"""
    words = np.array([[[NR.record([-(2**57)] * 2047 + [5])]]], dtype=np.uint64)
    rn = sa.ResponseNoise(words, step=2**60)
    assert int(rn.sum[0, 0, 0]) == -(2**57) * 2047 + 5 and int(rn.sumsq[0, 0, 0]) == 2047 * 2**114 + 25
    assert int(rn.max_abs[0, 0, 0]) == 2**57 and rn.budget_bits() == 2.0
    from fractions import Fraction

    want = float(Fraction(2047 * 2**114 + 25, 2048) - Fraction(-(2**57) * 2047 + 5, 2048) ** 2)
    assert rn.variance()[0, 0, 0] == want == rn.variance(pooled=True)
    assert rn.width2() == 2 * math.pi * want / 2.0**120


GEOMS = [(2, 2, 1 << 20, 256), (3, 3, (1 << 27) - 39, 32768)]  # (rows, cols, q', p_db): a base and a SpiralPack shape, the widest published q' and p


@pytest.mark.parametrize("rows,cols,qprime,p_db", GEOMS, ids=["base", "pack3-wide"])
def test_final_restatement_recovers_an_injected_error(rows, cols, qprime, p_db):
    rng = np.random.default_rng(21 + rows)
    sp = rng.integers(-64, 65, size=(rows, N))
    row0 = rng.integers(0, Q, size=(cols, N), dtype=np.uint64)
    m = rng.integers(0, p_db, size=(rows, cols, N), dtype=np.uint64)
    m[rows - 1, cols - 1, 7] = 5  # (clear of the wrap at m = 0, where Q mod p decides the neighbour below)
    scale = Q // p_db
    e = rng.integers(-(scale // 2) + 1, scale // 2, size=(rows, cols, N))  # |e| < scale_k / 2
    e[0, 0, 0], e[0, 0, 1], e[0, 0, 2] = scale // 2 - 1, -(scale // 2) + 1, 0
    fin = NR.build_final(sp, row0, m, e, p_db)
    assert int(fin.max()) < Q
    for expected in (m, None):
        got, m0 = NR.final_error(sp, fin, p_db, expected)
        assert (got == e).all() and (m0 == m).all()
    assert (NR.records(e, m, m)[..., 1] == 0).all()
    # beyond the radius: the nearest plaintext is the neighbour, n_wrong counts it, and against the true m the error is still the injected one
    far = e.copy()
    far[0, 0, :10] = scale // 2 + 5
    far[rows - 1, cols - 1, 7] = -(scale // 2) - 9
    fin = NR.build_final(sp, row0, m, far, p_db)
    got, m0, rec = NR.restate("final", sp, fin, 0, p_db, m)
    assert (got == far).all()
    assert int(rec[0, 0, 1]) == 10 and int(rec[rows - 1, cols - 1, 1]) == 1 and int(rec[..., 1].sum()) == 11
    assert (m0[0, 0, :10] == (m[0, 0, :10] + 1) % p_db).all()
    near, _ = NR.final_error(sp, fin, p_db, None)
    assert (np.abs(near) <= scale // 2 + p_db).all() and int(near[0, 0, 0]) == far[0, 0, 0] - scale


@pytest.mark.parametrize("rows,cols,qprime,p_db", GEOMS, ids=["base", "pack3-wide"])
def test_switched_restatement_recovers_an_injected_error(rows, cols, qprime, p_db):
    rng = np.random.default_rng(31 + rows)
    sp = rng.integers(-64, 65, size=(rows, N))
    row0 = rng.integers(0, qprime, size=(cols, N), dtype=np.uint64)
    m = rng.integers(0, p_db, size=(rows, cols, N), dtype=np.uint64)
    u = rng.integers(-1, 2, size=(rows, cols, N))
    resp, e = NR.build_switched(sp, row0, m, u, qprime, p_db)
    D = 4 * qprime
    assert np.abs(e).max() < D // 2, "|u| <= 1: the error stays below 1/8 + 1/4 of a step"
    for expected in (m, None):
        got, pt = NR.switched_error(sp, resp, qprime, p_db, expected)
        assert (got == e).all() and (pt == m).all(), "e / D comes back exactly"
    assert (pt == R.decode(sp, resp, qprime, p_db)).all()
    # expected one step off moves e by exactly D
    up, _ = NR.switched_error(sp, resp, qprime, p_db, (m + 1) % p_db)
    assert (up == e - D).all()
    down, _, rec = NR.restate("switched", sp, resp, qprime, p_db, (m + p_db - 1) % p_db)
    assert (down == e + D).all() and (rec[..., 1] == N).all()
    # an injected u of 3 quarter steps decodes to the neighbour; against the true m the error is the injected one
    u3 = u.copy()
    u3[0, 0, :5] = 3
    resp3, e3 = NR.build_switched(sp, row0, m, u3, qprime, p_db)
    got, pt, rec = NR.restate("switched", sp, resp3, qprime, p_db, m)
    assert (got == e3).all() and int(rec[0, 0, 1]) == 5 and (pt[0, 0, :5] == (m[0, 0, :5] + 1) % p_db).all()


def test_switched_half_open_ends():
    """with row 0 = 0, x = vr q': a row value of 4 m + 2 p puts e at -p D / 2 exactly (the end that is reached), one less at p D / 2 - q' (the largest
    e this row 0 allows), and +p D / 2 never comes out; without expected the ties |e| = D / 2 take the sign the rounding leaves"""
    qprime, p_db = 1 << 20, 256
    D, span = 4 * qprime, 4 * qprime * p_db
    sp = np.ones((2, N), dtype=np.int64)
    rng = np.random.default_rng(4)
    m = rng.integers(0, p_db, size=(2, 2, N), dtype=np.uint64)
    resp = np.zeros((3, 2, N), dtype=np.uint64)
    resp[1:] = (4 * m + 2 * p_db) % (4 * p_db)
    e, _ = NR.switched_error(sp, resp, qprime, p_db, m)
    assert (e == -(span // 2)).all()
    resp[1:] = (4 * m + 2 * p_db - 1) % (4 * p_db)
    e, _ = NR.switched_error(sp, resp, qprime, p_db, m)
    assert (e == span // 2 - qprime).all()
    for _ in range(3):
        resp[1:] = rng.integers(0, 4 * p_db, size=(2, 2, N), dtype=np.uint64)
        resp[0] = rng.integers(0, qprime, size=(2, N), dtype=np.uint64)
        e, _ = NR.switched_error(sp, resp, qprime, p_db, m)
        assert e.min() >= -(span // 2) and e.max() < span // 2
    # ties: x = D k + D / 2 > 0 rounds up, e = -D / 2; x = -(D k + D / 2) rounds down, e = +D / 2
    resp[0] = 0
    k = np.arange(N) % (p_db // 2)
    resp[1:] = 4 * k + 2
    resp[1, 1] = 4 * p_db - (4 * k + 2)
    e, pt = NR.switched_error(sp, resp, qprime, p_db)
    assert (e[0, 0] == -(D // 2)).all() and (pt[0, 0] == k + 1).all()
    assert (e[0, 1] == D // 2).all() and (pt[0, 1] == (-(k + 1)) % p_db).all()


def test_model_figures_reproduce_p_err_log2():
    """response_noise_model's second figure is the denominator of p_err_log2: put into that formula it gives p_err_log2 (1e-9 relative: double
    arithmetic of one expression), on base and packing sets of the golden sample; its first figure is noise_variance"""
    from spiral_amd import scheme as S

    gold = json.load(open(os.path.join(ROOT, "tests", "golden", "scheme_model.json")))["noise"]
    sets = [v for v in gold if v["feasible"] and v["kind"] in ("spiral", "spiralstream")][:4] + [v for v in gold if v["feasible"] and v["kind"].endswith("-pack")][:3]
    assert sum(1 for v in sets if not v["kind"].endswith("-pack")) >= 3 and sum(1 for v in sets if v["kind"].endswith("-pack")) >= 2
    for v in sets:
        kw = {k: v[k] for k in ("p", "t_GSW", "t_conv", "t_exp", "t_exp_right", "nu_1", "nu_2")}
        n = v.get("n", 2)
        for q_prime in (v["p"] * 2 ** 20, 2 ** v["q_prime_bits"] - 5):
            s_e, w2 = S.response_noise_model(v["kind"], q_prime=q_prime, n=n, **kw)
            assert s_e == S.noise_variance(v["kind"], n=n, **kw) and abs(math.log2(s_e) - v["s_e"]) < 1e-9
            nn = n if v["kind"].endswith("-pack") else 2
            pr = float(S.real_p(v["p"]))
            thresh = 0.25 - (1.0 / 8.0) * ((4 * pr) * (float(S.REAL_Q) % pr) / float(S.REAL_Q))
            mine = (math.log(2) + (-math.pi * thresh ** 2) / w2 + math.log(nn * nn * S.POLY_LEN)) * math.log(math.e, 2)
            want = S.p_err_log2(v["p"], q_prime, s_e, nn)
            assert abs(mine - want) <= 1e-9 * abs(want), (v, q_prime, mine, want)
