"""The response noise on the device (include/spiral_gpu.h spiral_gpu_client_response_noise; kernel: csrc/client.hip).  Expected values never come from
the session: the secret is exported, and every error, plaintext and record is the numpy / Python-integer restatement of the definition
(tests/noise_restated.py) on the same bytes -- on responses built to carry a chosen error, on uniformly random words, on the extreme operands of
the exactness bounds, and on whole runs through the server against the oracle's database items.  The geometries are those of
tests/test_gpu_client.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import client_restated as R  # noqa: E402
import noise_restated as NR  # noqa: E402

pytestmark = pytest.mark.gpu
N, Q = R.N, R.Q
K1 = bytes(range(7, 39))
BASE = (4, 3, dict(t_gsw=4), 0)
BASE_DIRECT = (5, 2, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1), 0)
PACK = (6, 2, dict(), 2)
STREAM_PACK = (7, 7, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1), 2)
PACK3 = (6, 2, dict(qprime_bits=27, p_db=32768), 3)
GEOMS = [BASE, BASE_DIRECT, PACK, STREAM_PACK, PACK3]
IDS = ["base", "base-direct", "pack", "stream-pack", "pack3-wide"]
U64, I64 = C.POINTER(C.c_uint64), C.POINTER(C.c_int64)


@pytest.fixture(scope="module")
def sa():
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


def params_of(sa, geom):
    nu1, nu2, kw, out_n = geom
    p = sa.make_params(nu1, nu2, **kw)
    qprime = sa.get_pack_shape(p, out_n).qprime if out_n else sa.get_shape(p).qprime
    return p, out_n, int(qprime)


def assert_eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp) if got.shape == exp.shape else []
        raise AssertionError(f"{what}: shapes {got.shape} / {exp.shape}, {len(bad)} of {got.size} words differ, first at {bad[:5].tolist() if len(bad) else bad}")


def to_wire(p, resps):
    w1 = int(4 * p.p_db - 1).bit_length()
    return np.concatenate([R.response_to_wire(r, p.qprime_bits, w1) for r in resps])


def restated(form, sp, resps, qprime, p_db, expected):
    """(errors [n][rows][cols][N], plaintexts, records [n][rows][cols][6]) of n responses; form "final" or "switched" """
    out = [NR.restate(form, sp, r, qprime, p_db, None if expected is None else expected[b]) for b, r in enumerate(resps)]
    return tuple(np.stack([o[i] for o in out]) for i in range(3))


def check_forms(sa, c, forms, resps, expected, want, what):
    """every form of `forms` (name -> the responses in that form) gives want = (errors, plaintexts, records): with both outputs, with the records
    alone, and with the errors alone (stats = NULL, through the C call)"""
    e_want, _, rec_want = want
    n = len(resps)
    for form, data in forms.items():
        rn = c.response_noise(data, form=form, expected=expected, errors=True)
        assert rn.errors.dtype == np.int64 and rn.step == c.noise_step(form)
        assert_eq(rn.errors, e_want, f"{what}, {form}: errors")
        assert_eq(rn.stats, rec_want, f"{what}, {form}: records")
        assert_eq(c.response_noise(data, form=form, expected=expected).stats, rec_want, f"{what}, {form}: records with errors = NULL")
        buf = np.ascontiguousarray(data)
        err = np.zeros(e_want.shape, dtype=np.int64)
        exp = None if expected is None else np.ascontiguousarray(expected, dtype=np.uint64)
        rc = sa.lib().spiral_gpu_client_response_noise(c.h, buf.ctypes.data_as(C.c_void_p), n, {"raw": 0, "wire": 1, "final": 2}[form],
                                                       None if exp is None else exp.ctypes.data_as(U64), None, err.ctypes.data_as(I64))
        assert rc == 0, sa.lib().spiral_gpu_last_error().decode()
        assert_eq(err, e_want, f"{what}, {form}: errors with stats = NULL")
        # the object's exact sums are the records' words
        assert int(rn.sum[0, 0, 0]) == int(e_want[0, 0, 0].astype(object).sum()) and int(rn.sumsq[0, 0, 0]) == int((e_want[0, 0, 0].astype(object) ** 2).sum())


@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_response_noise_bit_for_bit(sa, geom):
    """n = 5 in one launch and n = 1; RAW, WIRE and FINAL; with and without expected; responses built to carry a chosen error and uniformly random
    words (which make n_wrong and the 128-bit sums work): errors and records equal the restatement"""
    p, out_n, qprime = params_of(sa, geom)
    p_db = int(p.p_db)
    rows = cols = out_n or 2
    c = sa.Client(p, K1, out_n=out_n)
    sp = R.centred(c.secret()[1])
    rng = np.random.default_rng(rows * 1000 + qprime % 997)
    m = rng.integers(0, p_db, size=(5, rows, cols, N), dtype=np.uint64)
    # switched: built responses (|u| <= 1: they decode) at 0, 2, 4, random words at 1, 3
    resps = np.zeros((5, rows + 1, cols, N), dtype=np.uint64)
    built_e = {}
    for b in (0, 2, 4):
        resps[b], built_e[b] = NR.build_switched(sp, rng.integers(0, qprime, size=(cols, N), dtype=np.uint64), m[b], rng.integers(-1, 2, size=(rows, cols, N)), qprime, p_db)
    for b in (1, 3):
        resps[b, 0] = rng.integers(0, qprime, size=(cols, N), dtype=np.uint64)
        resps[b, 1:] = rng.integers(0, 4 * p_db, size=(rows, cols, N), dtype=np.uint64)
    forms = {"raw": resps, "wire": to_wire(p, resps)}
    for expected in (m, None):
        want = restated("switched", sp, resps, qprime, p_db, expected)
        for b in (0, 2, 4):
            assert_eq(want[0][b], built_e[b], "the restatement on a response built from a chosen error")
            assert not want[2][b, ..., 1].any()
        if expected is not None:
            assert int(want[2][1, ..., 1].min()) > 0, "random words decode wrongly: n_wrong is exercised"
        check_forms(sa, c, forms, resps, expected, want, f"five switched responses, expected {'given' if expected is not None else 'NULL'}")
        one = {"raw": resps[3:4], "wire": to_wire(p, resps[3:4])}
        check_forms(sa, c, one, resps[3:4], None if expected is None else expected[3:4], tuple(w[3:4] for w in want), "one switched response")
    # FINAL: built ciphertexts with |e| < scale_k / 2 at 0, 2, 4; random words below Q at 1; random 64-bit words (taken mod Q) at 3
    scale = Q // p_db
    fins = np.zeros((5, rows + 1, cols, N), dtype=np.uint64)
    for b in (0, 2, 4):
        built_e[b] = rng.integers(-(scale // 2) + 1, scale // 2, size=(rows, cols, N))
        fins[b] = NR.build_final(sp, rng.integers(0, Q, size=(cols, N), dtype=np.uint64), m[b], built_e[b], p_db)
    fins[1] = rng.integers(0, Q, size=(rows + 1, cols, N), dtype=np.uint64)
    fins[3] = rng.integers(0, 2**64, size=(rows + 1, cols, N), dtype=np.uint64)
    for expected in (m, None):
        want = restated("final", sp, fins, qprime, p_db, expected)
        for b in (0, 2, 4):
            assert_eq(want[0][b], built_e[b], "the restatement on a ciphertext built from a chosen error")
            assert not want[2][b, ..., 1].any()
        check_forms(sa, c, {"final": fins}, fins, expected, want, f"five FINAL ciphertexts, expected {'given' if expected is not None else 'NULL'}")
        check_forms(sa, c, {"final": fins[3:4]}, fins[3:4], None if expected is None else expected[3:4], tuple(w[3:4] for w in want), "one FINAL ciphertext")
    c.close()


@pytest.mark.parametrize("geom", [BASE, PACK3], ids=["base", "pack3-wide"])
def test_response_noise_extreme_operands(sa, geom):
    """the corners of the exactness bounds: a secret of +-64 everywhere and alternating against a row 0 of q' - 1 (switched) and of Q - 1 (FINAL: both
    residues maximal) with the other rows at their maximum; an expected that puts every e at -p D / 2; ties |e| = D / 2 of both signs.  decode
    returns what the restatement of check_final returns on the same operands, and (x - e) / D mod p is decode's output"""
    p, out_n, qprime = params_of(sa, geom)
    p_db = int(p.p_db)
    rows = cols = out_n or 2
    D, span = 4 * qprime, 4 * qprime * p_db
    c = sa.Client(p, K1, out_n=out_n)
    rng = np.random.default_rng(5)
    signs = [np.full(N, 64), np.full(N, -64), np.where(np.arange(N) % 2 == 0, 64, -64)]
    sp = np.stack([signs[r % 3] for r in range(rows)])
    c.set_secret(R.raw_of(np.full(N, -64)), R.raw_of(sp))
    m = rng.integers(0, p_db, size=(4, rows, cols, N), dtype=np.uint64)
    resp = np.zeros((4, rows + 1, cols, N), dtype=np.uint64)
    resp[:2, 0] = qprime - 1
    resp[0, 1:] = rng.integers(0, 4 * p_db, size=(rows, cols, N), dtype=np.uint64)
    resp[1, 1:] = 4 * p_db - 1
    resp[1, 0, 0, ::2] = 0  # (and a row 0 that alternates between the ends of its range)
    resp[2, 1:] = (4 * m[2] + 2 * p_db) % (4 * p_db)  # row 0 = 0: x - D m = 2 p q' = p D / 2 mod p D
    k = (np.arange(N) % (p_db // 2)).astype(np.uint64)
    resp[3, 1:] = 4 * k + 2  # x = D k + D / 2
    resp[3, 1, 0] = 4 * p_db - (4 * k + 2)  # x = -(D k + D / 2)
    forms = {"raw": resp, "wire": to_wire(p, resp)}
    for expected in (m, None):
        want = restated("switched", sp, resp, qprime, p_db, expected)
        if expected is not None:
            assert (want[0][2] == -(span // 2)).all(), "every e at the closed end of the centred range"
        else:
            assert (want[0][3, 0, 0] == D // 2).all() and (want[0][3, rows - 1, cols - 1] == -(D // 2)).all(), "ties of both signs"
        check_forms(sa, c, forms, resp, expected, want, f"switched extremes, expected {'given' if expected is not None else 'NULL'}")
    # decode is unchanged on these operands, and the error without expected is consistent with it
    dec = np.stack([R.decode(sp, r, qprime, p_db) for r in resp])
    got = c.decode(resp)
    assert_eq(got, dec, "decode at the extreme operands")
    assert_eq(c.decode(forms["wire"], form="wire"), dec, "the same in WIRE form")
    e = c.response_noise(resp, errors=True).errors
    for b in range(4):
        for r in range(rows):
            for cc in range(cols):
                x = NR.switched_x(sp[r], resp[b, 0, cc], resp[b, 1 + r, cc], qprime, p_db)
                assert not ((x - e[b, r, cc]) % D).any()
                assert_eq(((x - e[b, r, cc]) // D % p_db).astype(np.uint64), got[b, r, cc], "(x - e) / D mod p against decode")
    # FINAL: row 0 at Q - 1 everywhere, the other rows at Q - 1 and random
    fin = np.full((2, rows + 1, cols, N), Q - 1, dtype=np.uint64)
    fin[1, 1:] = rng.integers(0, Q, size=(rows, cols, N), dtype=np.uint64)
    for expected in (m[:2], None):
        want = restated("final", sp, fin, qprime, p_db, expected)
        check_forms(sa, c, {"final": fin}, fin, expected, want, f"FINAL extremes, expected {'given' if expected is not None else 'NULL'}")
    c.close()


def check_end_to_end(sa, c, fins, resps, wires, items, qprime, p_db):
    """n_wrong = 0, every max_abs below half a step, and the records equal the restatement's on the same bytes, in all three forms"""
    sp = R.centred(c.secret()[1])
    for form, data, kind, raw in (("final", fins, "final", fins), ("raw", resps, "switched", resps), ("wire", wires, "switched", resps)):
        rn = c.response_noise(data, form=form, expected=items, errors=True)
        assert not rn.n_wrong.any(), f"{form}: n_wrong"
        assert int(rn.max_abs.max()) < rn.step // 2, f"{form}: max |e| = {int(rn.max_abs.max())} of a radius {rn.step // 2}"
        assert rn.budget_bits() > 0
        want = restated(kind, sp, raw, qprime, p_db, items)
        assert_eq(rn.errors, want[0], f"{form}: errors")
        assert_eq(rn.stats, want[2], f"{form}: records")
        assert_eq(want[1], items, f"{form}: the restatement's plaintext is the item")
        # the variance is at most the largest e squared, and that lies inside the radius
        assert 0 < rn.variance(pooled=True) <= float(int(rn.max_abs.max())) ** 2 * (1 + 1e-12) and rn.width2() < 2 * np.pi / 4


def test_end_to_end_base(sa, oracle):
    """one session, its keys through KeyStore.put_client + bind_keys, two queries through set_query_batch on a two-lane batch; the lanes' folded
    ciphertexts, responses and wire forms against the oracle's db_item"""
    from spiral_amd import server as SV

    nu1, nu2, kw, _ = BASE
    po, pg = oracle.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    owner = sa.Server(pg, device=0)
    owner.gen_db(1234)
    lanes = [owner, sa.Server(pg, device=0, share_db_of=owner)]
    c = sa.Client(pg, bytes([40] * 32))
    store = sa.KeyStore(pg, 2, form="compact")
    store.put_client(1, c)
    sa.bind_keys(lanes, store, [1, 1])
    idx = [37, 127]
    sa.set_query_batch(lanes, list(c.queries(idx, "seeded")), form="seeded")
    sa.run_query_batch(lanes)
    for s in lanes:
        s.sync()
    fins = np.stack([s.read(SV.BUF_FINAL) for s in lanes]).reshape(2, 3, 2, N)
    resps = np.stack([s.read(SV.BUF_RESPONSE) for s in lanes]).reshape(2, 3, 2, N)
    wires = np.ascontiguousarray(sa.read_response_wire_batch(lanes)).reshape(-1)
    items = np.stack([oracle.db_item(po, 1234, i) for i in idx]).astype(np.uint64)
    check_end_to_end(sa, c, fins, resps, wires, items, int(c.shape.qprime), int(pg.p_db))
    for x in (lanes[1], owner, c):
        x.close()
    store.close()


def test_end_to_end_pack(sa, oracle):
    """one SpiralPack answer: the packed ciphertext through ops.from_ntt is the FINAL form"""
    from spiral_amd import ops

    nu1, nu2, kw, out_n = PACK
    po, pg = oracle.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    srv = sa.PackServer(pg, out_n, device=0)
    srv.gen_db(99)
    c = sa.Client(pg, bytes([60] * 32), out_n=out_n)
    srv.set_pub_params_seeded(c.pub_params("seeded"))
    idx = 11
    resp, packed, _ = srv.answer_seeded(c.query(idx, "seeded"))
    fin = ops.from_ntt(packed)
    wire = srv.read_response_wire()
    items = np.asarray(oracle.pack_db_item(po, out_n, 99, idx), dtype=np.uint64)[None]
    check_end_to_end(sa, c, fin[None], resp[None], wire, items, int(c.shape.qprime), int(pg.p_db))
    srv.close()
    c.close()


def test_response_noise_refusals(sa):
    """every refusal leaves both output buffers untouched"""
    p, _, _ = params_of(sa, BASE)
    c = sa.Client(p, K1)
    L = sa.lib()
    resp = np.zeros((2, 3, 2, N), dtype=np.uint64)
    stats = np.full((2, 2, 2, 6), 77, dtype=np.uint64)
    err = np.full((2, 2, 2, N), 77, dtype=np.int64)
    exp = np.zeros((2, 2, 2, N), dtype=np.uint64)
    exp[1, 0, 1, 9] = p.p_db
    vp, sp_, ep, xp = resp.ctypes.data_as(C.c_void_p), stats.ctypes.data_as(U64), err.ctypes.data_as(I64), exp.ctypes.data_as(U64)
    for args, msg in (((None, vp, 1, 0, None, sp_, ep), "null client session"), ((c.h, None, 1, 0, None, sp_, ep), "null argument"),
                      ((c.h, vp, 1, 0, None, None, None), "stats and errors are both null"), ((c.h, vp, 1, 3, None, sp_, ep), "unknown response form 3"),
                      ((c.h, vp, 1, -1, None, sp_, ep), "unknown response form"), ((c.h, vp, 0, 0, None, sp_, ep), "0 responses"),
                      ((c.h, vp, 65536, 2, None, sp_, ep), "65536 responses"),
                      ((c.h, vp, 2, 0, xp, sp_, ep), f"expected value {p.p_db} of response 1, row 0, column 1, coefficient 9"),
                      ((c.h, vp, 2, 2, xp, sp_, None), "response 1, row 0, column 1, coefficient 9")):
        assert L.spiral_gpu_client_response_noise(*args) != 0
        assert msg in L.spiral_gpu_last_error().decode(), (msg, L.spiral_gpu_last_error().decode())
        assert "client_response_noise" in L.spiral_gpu_last_error().decode()
    assert (stats == 77).all() and (err == 77).all(), "a refused call writes nothing"
    # the first response alone holds no bad value: accepted
    assert L.spiral_gpu_client_response_noise(c.h, vp, 1, 0, xp, sp_, ep) == 0
    assert (stats[0] != 77).any() and (stats[1] == 77).all()
    with pytest.raises(ValueError, match="whole number of responses"):
        c.response_noise(np.zeros(5, dtype=np.uint64))
    with pytest.raises(ValueError, match="'raw', 'wire' or 'final'"):
        c.response_noise(resp, form="ntt")
    with pytest.raises(ValueError, match="expected holds"):
        c.response_noise(resp, expected=np.zeros(7, dtype=np.uint64))
    # decode still takes the two switched forms only
    out = np.zeros((1, 2, 2, N), dtype=np.uint64)
    assert L.spiral_gpu_client_decode(c.h, vp, 1, 2, out.ctypes.data_as(U64)) != 0 and "unknown response form" in L.spiral_gpu_last_error().decode()
    c.close()
