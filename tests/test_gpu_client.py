"""The client session on the device (include/spiral_gpu.h spiral_gpu_client_*; kernels: csrc/client.hip).  Expected values never come from the session
itself: the secret key is the numpy restatement of the format (tests/client_restated.py) on the library's threshold table; every decoded
plaintext is the restatement of check_final -- on responses built to decode to chosen plaintexts, on uniformly random words and on the extreme
operands of the exactness bound -- in both response forms, for one and for several responses per launch, on base and SpiralPack shapes; every
message is taken apart with the exported secret, the oracle's ring operations and the restated noise; and whole runs end at the oracle's db_item."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import client_restated as R  # noqa: E402

pytestmark = pytest.mark.gpu
N = 2048
K1 = bytes(range(7, 39))
K2 = bytes(range(100, 132))
# (nu1, nu2, parameters, out_n): the small geometries of the seeded-input tests; the decode depends on q', p_db and the response's shape alone
BASE = (4, 3, dict(t_gsw=4), 0)
BASE_DIRECT = (5, 2, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1), 0)
PACK = (6, 2, dict(), 2)
STREAM_PACK = (7, 7, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1), 2)
PACK3 = (6, 2, dict(qprime_bits=27, p_db=32768), 3)  # an odd out_n, the widest published q' and plaintext modulus
GEOMS = [BASE, BASE_DIRECT, PACK, STREAM_PACK, PACK3]
IDS = ["base", "base-direct", "pack", "stream-pack", "pack3-wide"]


@pytest.fixture(scope="module")
def sa():
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


@pytest.fixture(scope="module")
def table(sa):
    return sa.client_noise_table()


def params_of(sa, geom):
    nu1, nu2, kw, out_n = geom
    p = sa.make_params(nu1, nu2, **kw)
    qprime = sa.get_pack_shape(p, out_n).qprime if out_n else sa.get_shape(p).qprime
    return p, out_n, int(qprime)


def assert_eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[:5].tolist()}")


@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_secret_is_the_restated_format(sa, table, geom):
    """sr and the rows of Sp are noise polynomials 0, 1.. under the client seed with the secret's tag; two sessions from one seed hold one key,
    another seed gives another key, nonoise gives zeros"""
    p, out_n, _ = params_of(sa, geom)
    rows = out_n or 2
    c = sa.Client(p, K1, out_n=out_n)
    sr, sp = c.secret()
    want_sr, want_sp = R.secret(table, K1, rows)
    assert sp.shape == (rows, N)
    assert_eq(sr, R.raw_of(want_sr), "sr")
    assert_eq(sp, R.raw_of(want_sp), "Sp")
    assert np.abs(want_sp).max() <= 64 and want_sp.std() > 1.5
    twin = sa.Client(p, K1, out_n=out_n)
    assert_eq(twin.secret()[1], sp, "a second session from the same seed")
    other = sa.Client(p, K2, out_n=out_n)
    assert not (other.secret()[1] == sp).all() and not (other.secret()[0] == sr).all()
    quiet = sa.Client(p, K1, out_n=out_n, nonoise=True)
    assert not quiet.secret()[0].any() and not quiet.secret()[1].any()
    for x in (c, twin, other, quiet):
        x.close()


def test_set_secret_round_trip_and_refusals(sa, table):
    p, out_n, qprime = params_of(sa, PACK)
    c = sa.Client(p, K1, out_n=out_n)
    before = c.secret()
    rng = np.random.default_rng(3)
    sr = R.raw_of(rng.integers(-64, 65, size=N))
    sp = R.raw_of(rng.integers(-64, 65, size=(2, N)))
    sp[0, 0], sp[0, 1], sp[1, 2047] = 64, R.Q - 64, 0  # the ends of the range are taken
    c.set_secret(sr, sp)
    got = c.secret()
    assert_eq(got[0], sr, "sr after set_secret")
    assert_eq(got[1], sp, "Sp after set_secret")
    # a coefficient of 65, of -65, and one that is no residue: refused by name, the key unchanged
    for bad, where in ((65, (1, 5)), (R.Q - 65, (0, 2047)), (R.Q, (1, 0)), (2**63, (0, 9))):
        sp2 = sp.copy()
        sp2[where] = bad
        with pytest.raises(sa.SpiralGpuError, match=r"outside \[-64, 64\]"):
            c.set_secret(sr, sp2)
    sr2 = sr.copy()
    sr2[100] = 65
    with pytest.raises(sa.SpiralGpuError, match=r"coefficient 100 of sr"):
        c.set_secret(sr2, sp)
    assert_eq(c.secret()[1], sp, "Sp after refused calls")
    with pytest.raises(ValueError):
        c.set_secret(sr, sp[:1])
    L, U = sa.lib(), C.POINTER(C.c_uint64)
    assert L.spiral_gpu_client_set_secret(c.h, sr.ctypes.data_as(U), None) != 0 and "null" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_client_set_secret(None, sr.ctypes.data_as(U), sp.ctypes.data_as(U)) != 0 and "null client session" in L.spiral_gpu_last_error().decode()
    c.set_secret(*before)
    assert_eq(c.secret()[1], before[1], "the first key restored")
    c.close()


@pytest.mark.parametrize("geom", GEOMS, ids=IDS)
def test_decode_bit_for_bit(sa, table, geom):
    """n = 5 responses in one launch and n = 1, RAW and WIRE: responses built to decode to chosen plaintexts, and uniformly random words (row 0
    below q', the other rows below 4 p_db) -- each equal to the numpy restatement of check_final"""
    p, out_n, qprime = params_of(sa, geom)
    rows = cols = out_n or 2
    c = sa.Client(p, K1, out_n=out_n)
    sp = R.centred(c.secret()[1])
    assert_eq(sp, R.secret(table, K1, rows)[1], "the session's Sp")
    rng = np.random.default_rng(rows * 1000 + qprime % 997)
    valid = [R.valid_response(rng, sp, qprime, p.p_db, cols) for _ in range(3)]
    rand = []
    for _ in range(2):
        r = np.zeros((rows + 1, cols, N), dtype=np.uint64)
        r[0] = rng.integers(0, qprime, size=(cols, N), dtype=np.uint64)
        r[1:] = rng.integers(0, 4 * p.p_db, size=(rows, cols, N), dtype=np.uint64)
        rand.append(r)
    resps = np.stack([valid[0][0], rand[0], valid[1][0], rand[1], valid[2][0]])
    want = np.stack([R.decode(sp, r, qprime, p.p_db) for r in resps])
    for k, (_, m) in zip((0, 2, 4), valid):
        assert_eq(want[k], m, "the restatement on a response built from chosen plaintexts")
    got = c.decode(resps)
    assert got.shape == (5, rows, cols, N) and int(got.max()) < p.p_db
    assert_eq(got, want, "decode of five RAW responses")
    assert_eq(c.decode(resps[3]), want[3:4], "decode of one RAW response")
    w1 = int(4 * p.p_db - 1).bit_length()
    wires = [R.response_to_wire(r, p.qprime_bits, w1) for r in resps]
    assert all(w.size == sa.response_wire_bytes(p, cols) for w in wires)
    assert_eq(sa.response_from_wire(p, wires[1], cols), resps[1], "the test's wire packer against the library's host reader")
    assert_eq(c.decode(np.concatenate(wires), form="wire"), want, "decode of five WIRE responses")
    assert_eq(c.decode(wires[4].tobytes(), form="wire"), want[4:5], "decode of one WIRE response")
    c.close()


@pytest.mark.parametrize("geom", [BASE, PACK3], ids=["base", "pack3-wide"])
def test_decode_extreme_operands(sa, geom):
    """the exactness bound's corner: a secret of +-64 everywhere against a row 0 of q' - 1 everywhere, where the 64-bit sums reach 2048 * 64 * (q' - 1)"""
    p, out_n, qprime = params_of(sa, geom)
    rows = cols = out_n or 2
    c = sa.Client(p, K1, out_n=out_n)
    rng = np.random.default_rng(5)
    signs = [np.full(N, 64), np.full(N, -64), np.where(np.arange(N) % 2 == 0, 64, -64)]
    sp = np.stack([signs[r % 3] for r in range(rows)])
    c.set_secret(R.raw_of(np.full(N, -64)), R.raw_of(sp))
    resp = np.zeros((2, rows + 1, cols, N), dtype=np.uint64)
    resp[:, 0] = qprime - 1
    resp[0, 1:] = rng.integers(0, 4 * p.p_db, size=(rows, cols, N), dtype=np.uint64)
    resp[1, 1:] = 4 * p.p_db - 1
    resp[1, 0, 0, ::2] = 0  # (and a row 0 that alternates between the ends of its range)
    want = np.stack([R.decode(sp, r, qprime, p.p_db) for r in resp])
    assert_eq(c.decode(resp), want, "decode at the extreme operands")
    w1 = int(4 * p.p_db - 1).bit_length()
    wire = np.concatenate([R.response_to_wire(r, p.qprime_bits, w1) for r in resp])
    assert_eq(c.decode(wire, form="wire"), want, "the same in WIRE form")
    c.close()


def test_decode_refusals(sa):
    p, out_n, _ = params_of(sa, BASE)
    c = sa.Client(p, K1)
    L, U = sa.lib(), C.POINTER(C.c_uint64)
    resp = np.zeros((3, 2, N), dtype=np.uint64)
    out = np.full((2, 2, N), 77, dtype=np.uint64)
    vp = resp.ctypes.data_as(C.c_void_p)
    for args, msg in (((None, vp, 1, 0, out.ctypes.data_as(U)), "null client session"), ((c.h, None, 1, 0, out.ctypes.data_as(U)), "null argument"),
                      ((c.h, vp, 1, 0, None), "null argument"), ((c.h, vp, 1, 2, out.ctypes.data_as(U)), "unknown response form"),
                      ((c.h, vp, 0, 0, out.ctypes.data_as(U)), "0 responses"), ((c.h, vp, 65536, 1, out.ctypes.data_as(U)), "65536 responses")):
        assert L.spiral_gpu_client_decode(*args) != 0
        assert msg in L.spiral_gpu_last_error().decode(), msg
    assert (out == 77).all(), "a refused call writes nothing"
    with pytest.raises(ValueError, match="whole number of responses"):
        c.decode(np.zeros(5, dtype=np.uint64))
    with pytest.raises(ValueError, match="whole number of responses"):
        c.decode(np.zeros(sa.response_wire_bytes(p, 2) + 1, dtype=np.uint8), form="wire")
    with pytest.raises(ValueError, match="'raw' or 'wire'"):
        c.decode(resp, form="ntt")
    c.close()


# ---- messages: public parameters and queries ------------------------------------------------------------------------------------------------------
# The stopround = 0 branch of the query plaintext (ell * nu2 > dim0): (2, 2, t_gsw=8, p_db=16), ell * nu2 = 16 > dim0 = 4.  Not (3, 3, t_gsw=4) or
# (2, 2, t_gsw=4): get_shape takes them and their messages have the same structure, but at q' of 20 bits and p_db = 256 their answers do not always
# decode with the oracle's own Client either (6 to 389 wrong coefficients of 8192 at the first, up to 21 on two of eight client seeds at the second),
# so they cannot carry an end-to-end check.  t_gsw = 8 decoded cleanly on eight of eight seeds at p_db = 256; p_db = 16 adds a factor 16 of margin.
STOP0 = (2, 2, dict(t_gsw=8, p_db=16), 0)
MSG_GEOMS = [BASE, BASE_DIRECT, PACK, STREAM_PACK, STOP0]
MSG_IDS = ["base", "base-direct", "pack", "stream-pack", "base-stopround0"]
MOD = np.array([R.P, R.B], dtype=np.uint64).reshape(2, 1)


def bits_per(t):
    return 1 if t == 56 else 56 // t + 1


def gadget(t, j):
    sh = bits_per(t) * j
    return 0 if sh >= 64 else 1 << sh


def ntt_neg(x):
    return (MOD - x) % MOD


def ntt_sub(x, y):
    return (x + MOD - y) % MOD


def ntt_scale(x, c):
    """a constant times NTT-form polynomials"""
    return x * np.array([c % R.P, c % R.B], dtype=np.uint64).reshape(2, 1) % MOD


class Restated:
    """what a session's messages must contain, from the exported secret, the oracle's ring operations and the restated randomness"""

    def __init__(self, sa, O, table, client, K, nonoise=False):
        self.sa, self.O, self.T, self.c, self.K, self.nonoise = sa, O, table, client, K, nonoise
        self.p, self.out_n, self.s = client.params, client.out_n, client.shape
        sr, sp = client.secret()
        want_sr, want_sp = R.secret(table, K, client.rows, nonoise)
        assert_eq(sr, R.raw_of(want_sr), "sr")
        assert_eq(sp, R.raw_of(want_sp), "Sp")
        self.sr = sr
        self.s0 = O.to_ntt(sr.reshape(1, 1, N))  # [1][1][2][N]
        self.sp = O.to_ntt(sp.reshape(client.rows, 1, N))  # [rows][1][2][N]
        self.sps0 = np.stack([O.multiply(self.sp[r:r + 1], self.s0)[0] for r in range(client.rows)])
        self.s0sq = O.multiply(self.s0, self.s0)

    def tau(self, i):
        return self.O.to_ntt(self.O.automorph(self.sr.reshape(1, 1, N), (N >> i) + 1))[0, 0]

    def check_matrix(self, mat, seed, noise_key, domain, k0, noise0, S, msg, what):
        """mat [rows][cols][2][N]: row 0 is the seed's expansion; b_r - a S_r - msg_r, lifted, is exactly noise polynomial noise0 + (r - 1) cols + c.
        S: [rows - 1] NTT polynomials [1][1][2][N]; msg: [rows - 1][cols][2][N] NTT.  Returns the number of noise coefficients compared"""
        rows, cols = mat.shape[:2]
        assert_eq(mat[0], self.sa.seed_expand(seed, domain, k0, cols), f"{what}: row 0")
        a = ntt_neg(mat[0]).reshape(1, cols, 2, N)
        n = 0
        for r in range(1, rows):
            resid = ntt_sub(ntt_sub(mat[r], self.O.multiply(S[r - 1], a)[0]), msg[r - 1])
            got = self.O.from_ntt(np.ascontiguousarray(resid))
            want = np.stack([R.raw_of(R.noise_poly(self.T, noise_key, R.D_NOISE, noise0 + (r - 1) * cols + c, self.nonoise)) for c in range(cols)])
            assert_eq(got, want, f"{what}: noise of row {r}")
            n += want.size
        return n

    def check_pub_params(self, pp):
        p, s, tc, rows = self.p, self.s, self.p.t_conv, self.c.rows
        seed, nk = R.message_seed(self.K, 0), R.message_noise_key(self.K, 0)
        dom = 4 if self.out_n else 2
        k = noise = compared = 0
        zero = np.zeros((2, N), dtype=np.uint64)
        for part, (count, prow, pcol) in enumerate(self.c.parts):
            for mi in range(count):
                mat = pp[part][mi]
                if part < 2:  # W_exp: tau_i(s0) g under s0
                    S = [self.s0]
                    msg = np.stack([ntt_scale(self.tau(mi), gadget(pcol, c)) for c in range(pcol)])[None]
                elif self.out_n == 0 and part == 2:  # W: s0 2^(bits j) on row i of column i + 2 j
                    S = [self.sp[r:r + 1] for r in range(2)]
                    msg = np.stack([np.stack([ntt_scale(self.s0[0, 0], gadget(tc, c // 2)) if c % 2 == r else zero for c in range(pcol)]) for r in range(2)])
                elif self.out_n == 0:  # V: Sp [s0 gv | gv]
                    S = [self.sp[r:r + 1] for r in range(2)]
                    msg = np.stack([np.stack([ntt_scale(self.sps0[r, 0] if c < tc else self.sp[r, 0], gadget(tc, c % tc)) for c in range(pcol)]) for r in range(2)])
                elif part == 2:  # SpiralPack's V: s0^2 2^(bits j), s0 2^(bits j)
                    S = [self.s0]
                    msg = np.stack([ntt_scale(self.s0sq[0, 0] if c % 2 == 0 else self.s0[0, 0], gadget(tc, c // 2)) for c in range(pcol)])[None]
                else:  # v_W[i]: s0 g on row i
                    S = [self.sp[r:r + 1] for r in range(rows)]
                    msg = np.stack([np.stack([ntt_scale(self.s0[0, 0], gadget(tc, c)) if r == mi else zero for c in range(pcol)]) for r in range(rows)])
                compared += self.check_matrix(mat, seed, nk, dom, k, noise, S, msg, f"part {part} matrix {mi}")
                k += pcol
                noise += (prow - 1) * pcol
        return compared, noise

    def sigma(self, idx):
        """the compressed query's plaintext (src/spiral.cpp:2104-2152, src/testing.cpp:991-1006), raw"""
        s, p = self.s, self.p
        i0, rest, scale, bits = idx // s.num_per, idx % s.num_per, R.Q // p.p_db, bits_per(s.ell)
        sig = [0] * N
        if self.out_n or s.stopround != 0:
            sig[2 * i0] = scale
            for i in range(p.nu2):
                for j in range(s.ell):
                    sig[2 * (i * s.ell + j) + 1] = (1 << (bits * j)) * ((rest >> i) & 1)
            inv_first, inv_rest = pow(1 << s.g, -1, R.Q), pow(1 << (s.stopround + 1), -1, R.Q)
            sig = [x * (inv_rest if z % 2 else inv_first) % R.Q for z, x in enumerate(sig)]
        else:
            sig[i0] = scale
            for i in range(p.nu2):
                for j in range(s.ell):
                    sig[s.dim0 + i * s.ell + j] = (1 << (bits * j)) * ((rest >> i) & 1)
            inv = pow(1 << s.g, -1, R.Q)
            sig = [x * inv % R.Q for x in sig]
        return np.array(sig, dtype=np.uint64)

    def check_query(self, q, idx, number):
        """q [n_query_cts][2][1][2][N], message `number`"""
        s, p, O = self.s, self.p, self.O
        seed, nk = R.message_seed(self.K, number), R.message_noise_key(self.K, number)
        n = s.n_query_cts
        i0, rest, scale, bits = idx // s.num_per, idx % s.num_per, R.Q // p.p_db, bits_per(s.ell)
        const = lambda v: O.to_ntt(np.array([v] + [0] * (N - 1), dtype=np.uint64).reshape(1, N))[0]  # noqa: E731
        if not p.direct_upload:
            msgs = [O.to_ntt(self.sigma(idx).reshape(1, N))[0]]
        else:
            msgs = [const(scale if i == i0 else 0) for i in range(s.dim0)]
            for t in range(n - s.dim0):
                d = t // 2 if self.out_n else t
                val = (1 << (bits * (d % s.ell))) * ((rest >> (d // s.ell)) & 1)
                msgs.append(O.multiply(self.s0, const(val).reshape(1, 1, 2, N))[0, 0] if self.out_n and t % 2 == 0 else const(val))
        assert len(msgs) == n
        assert_eq(q[:, 0, 0], self.sa.seed_expand(seed, 3 if self.out_n else 1, 0, n), f"query {number}: row 0")
        a = ntt_neg(q[:, 0, 0]).reshape(1, n, 2, N)
        resid = ntt_sub(ntt_sub(q[:, 1, 0], O.multiply(self.s0, a)[0]), np.stack(msgs))
        want = np.stack([R.raw_of(R.noise_poly(self.T, nk, R.D_NOISE, i, self.nonoise)) for i in range(n)])
        assert_eq(O.from_ntt(np.ascontiguousarray(resid)), want, f"query {number}: noise")
        return seed


def session(sa, geom, K=K1, **kw):
    nu1, nu2, pkw, out_n = geom
    return sa.Client(sa.make_params(nu1, nu2, **pkw), K, out_n=out_n, **kw)


@pytest.mark.parametrize("geom", MSG_GEOMS, ids=MSG_IDS)
def test_messages_structure_bit_for_bit(sa, oracle, table, geom):
    """pub_params and three consecutive queries: every row 0 is the expansion of the restated message seed, and for every column and secret row
    b - a S - message is exactly the restated noise polynomial: no coefficient is skipped.  This pins sigma, the gadget constants and the column order"""
    c = session(sa, geom)
    rs = Restated(sa, oracle, table, c, K1)
    compared, n_noise = rs.check_pub_params(c.pub_params())
    sent = sum(n * (r - 1) * cc for n, r, cc in c.parts)
    assert n_noise == sent and compared == sent * N and sent > 0
    assert c.counter == 1, "the public parameters are message 0 and move no counter"
    idx = [c.n_items - 1, 0, (5 * c.shape.num_per + 3) % c.n_items]
    qs = c.queries(idx, "ntt")
    assert c.counter == 4
    seeds = [rs.check_query(qs[b], idx[b], 1 + b) for b in range(3)]
    assert len(set(seeds)) == 3 and R.message_seed(K1, 0) not in seeds, "consecutive messages have different seeds"
    c.close()


def test_nonoise_messages(sa, oracle, table):
    """nonoise: every restated noise term is 0, the secret included -- the same structure check with zeros"""
    c = session(sa, BASE, nonoise=True)
    rs = Restated(sa, oracle, table, c, K1, nonoise=True)
    rs.check_pub_params(c.pub_params())
    rs.check_query(c.query(9, "ntt"), 9, 1)
    c.close()


def rescaled(O, fin, qprime, p_db):
    out = np.zeros_like(fin)
    flat, o = fin.reshape(3, -1), out.reshape(3, -1)
    for r in range(3):
        o[r] = [O.rescale(int(x), R.Q, qprime if r == 0 else 4 * p_db) for x in flat[r]]
    return out


@pytest.mark.parametrize("geom,nonoise", [(BASE, False), (BASE_DIRECT, False), (STOP0, False), (PACK, False), (STREAM_PACK, False), (BASE, True)],
                         ids=MSG_IDS[:2] + ["base-stopround0", "pack", "stream-pack", "base-nonoise"])
def test_end_to_end_through_the_oracle(sa, oracle, geom, nonoise):
    """the session's NTT-form keys and query, the oracle's answer on the CPU against its generated database, the session's decode: the database item"""
    O = oracle
    nu1, nu2, kw, out_n = geom
    po = O.make_params(nu1, nu2, **kw)
    c = session(sa, geom, K2, nonoise=nonoise)
    pp = c.pub_params()
    idx = (3 * c.shape.num_per + 5) % c.n_items
    q = c.query(idx, "ntt")
    if out_n:
        resp, _ = O.pack_answer(po, out_n, q, *pp, O.pack_gen_db(po, out_n, 77))
        want = O.pack_db_item(po, out_n, 77, idx)
    else:
        resp = rescaled(O, O.answer(po, q, *pp, O.gen_db(po, 77)), int(c.shape.qprime), po.p_db)
        want = O.db_item(po, 77, idx)
    assert_eq(c.decode(resp)[0], want, "the decoded item")
    c.close()


def test_forms_leave_one_server_state(sa, oracle):
    """the NTT, wire and seeded forms of the public parameters and of one query (the same message number, through the counter) leave a server with
    identical buffers and identical answers on a generated database; the item decodes"""
    from spiral_amd import server as SV

    for geom in (BASE, BASE_DIRECT):
        c = session(sa, geom)
        idx, states = 21 % c.n_items, []
        for form in ("ntt", "wire", "seeded"):
            srv = sa.Server(c.params, device=0)
            srv.gen_db(31)
            c.counter = 6
            pp, q = c.pub_params(form), c.query(idx, form)
            assert c.counter == 7
            if form == "ntt":
                srv.set_pub_params(*pp)
                srv.set_query(q)
            else:
                getattr(srv, "set_pub_params_" + form)(pp)
                getattr(srv, "set_query_" + form)(q)
            srv.run_query()
            srv.sync()
            states.append({b: srv.read(b) for b in (SV.BUF_QUERY, SV.BUF_EXPANDED, SV.BUF_GSW, SV.BUF_FINAL, SV.BUF_RESPONSE)})
            srv.close()
        for form, st in zip(("wire", "seeded"), states[1:]):
            for b, words in st.items():
                assert_eq(words, states[0][b], f"buffer {b} after the {form} form")
        po = oracle.make_params(geom[0], geom[1], **geom[2])
        assert_eq(c.decode(states[0][SV.BUF_RESPONSE])[0], oracle.db_item(po, 31, idx), "the decoded item")
        c.close()


def test_determinism_freshness_and_refusals(sa):
    """two sessions from one seed emit identical messages; consecutive queries differ; set_counter reproduces a query; a refused call (a wrong
    bytes_each, an index out of range, set_counter(0), a null session) leaves the counter and the output alone"""
    c, twin = session(sa, BASE), session(sa, BASE)
    assert (c.pub_params("seeded") == twin.pub_params("seeded")).all() and (c.pub_params("seeded") == c.pub_params("seeded")).all()
    a, b = c.queries([3, 3], "seeded"), twin.queries([3, 3], "seeded")
    assert (a == b).all() and not (a[0] == a[1]).all() and not (a[0, :32] == a[1, :32]).all()
    assert c.counter == 3
    c.counter = 2
    assert (c.query(3, "seeded") == a[1]).all(), "set_counter reproduces message 2"
    assert c.counter == 3
    other = session(sa, BASE, K2)
    assert not (other.query(3, "seeded")[:32] == a[0, :32]).all()
    L, U = sa.lib(), C.POINTER(C.c_uint64)
    each = sa.query_seeded_bytes(c.params)
    out = np.full(each + 8, 0x5A, dtype=np.uint8)
    ids = np.array([3], dtype=np.uint64)
    vp = out.ctypes.data_as(C.c_void_p)
    for args, msg in (((c.h, ids.ctypes.data_as(U), 1, 2, vp, each + 1), "bytes_each"), ((c.h, ids.ctypes.data_as(U), 1, 1, vp, each), "bytes_each"),
                      ((c.h, np.array([c.n_items], dtype=np.uint64).ctypes.data_as(U), 1, 2, vp, each), "outside the database"),
                      ((c.h, ids.ctypes.data_as(U), 1, 3, vp, each), "unknown form"), ((c.h, ids.ctypes.data_as(U), 0, 2, vp, each), "0 queries"),
                      ((None, ids.ctypes.data_as(U), 1, 2, vp, each), "null client session"), ((c.h, None, 1, 2, vp, each), "null argument")):
        assert L.spiral_gpu_client_queries(*args) != 0
        assert msg in L.spiral_gpu_last_error().decode(), msg
    assert (out == 0x5A).all() and c.counter == 3, "a refused call writes nothing and the counter does not move"
    with pytest.raises(sa.SpiralGpuError, match="message 0 is the public parameters"):
        c.counter = 0
    assert c.counter == 3
    n = C.c_uint64()
    assert L.spiral_gpu_client_set_counter(None, 5) != 0 and "null client session" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_client_get_counter(None, C.byref(n)) != 0 and "null client session" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_client_pub_params(None, None, None, None, None) != 0 and "null client session" in L.spiral_gpu_last_error().decode()
    small = np.zeros(64, dtype=np.uint8)
    assert L.spiral_gpu_client_pub_params_msg(c.h, 2, small.ctypes.data_as(C.c_void_p), small.size) != 0 and "capacity" in L.spiral_gpu_last_error().decode()
    assert L.spiral_gpu_client_pub_params_msg(c.h, 0, small.ctypes.data_as(C.c_void_p), small.size) != 0
    assert not small.any()
    for x in (c, twin, other):
        x.close()


def test_end_to_end_through_the_server(sa, oracle):
    """three lanes, three sessions: keys through KeyStore.put_client + bind_keys, queries through set_query_batch(form="seeded"), run_query_batch,
    read_response_wire_batch and ONE decode(form="wire") per session of its lane's response; every lane's item is the database's"""
    nu1, nu2, kw, _ = BASE
    po, pg = oracle.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    owner = sa.Server(pg, device=0)
    owner.gen_db(1234)
    lanes = [owner] + [sa.Server(pg, device=0, share_db_of=owner) for _ in range(2)]
    clients = [sa.Client(pg, bytes([40 + i] * 32)) for i in range(3)]
    store = sa.KeyStore(pg, 4, form="compact")
    slots = [2, 0, 3]
    for cl, slot in zip(clients, slots):
        store.put_client(slot, cl)
    sa.bind_keys(lanes, store, slots)
    idx = [37, 5, 127]
    sa.set_query_batch(lanes, [cl.query(i, "seeded") for cl, i in zip(clients, idx)], form="seeded")
    sa.run_query_batch(lanes)
    wires = sa.read_response_wire_batch(lanes)
    for b, cl in enumerate(clients):
        assert_eq(cl.decode(wires[b], form="wire")[0], oracle.db_item(po, 1234, idx[b]), f"lane {b}")
    # one session decoding a batch of its own responses in one launch: lane 0's client asks all three lanes
    store.put_client(1, clients[0])
    sa.bind_keys(lanes, store, [2, 1, 1])
    sa.set_query_batch(lanes, list(clients[0].queries(idx, "seeded")), form="seeded")
    sa.run_query_batch(lanes)
    got = clients[0].decode(sa.read_response_wire_batch(lanes), form="wire")
    for b in range(3):
        assert_eq(got[b], oracle.db_item(po, 1234, idx[b]), f"item {b} of one decode of three")
    for x in lanes[1:] + [owner] + clients:
        x.close()
    store.close()


def test_pack_batch_end_to_end(sa, oracle):
    """a SpiralPack batch through answer_batch_seeded: two sessions, two lanes, each lane's response decodes to its item"""
    P = sys.modules["spiral_amd.pack"]
    nu1, nu2, kw, out_n = PACK
    po, pg = oracle.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    owner = sa.PackServer(pg, out_n, device=0)
    owner.gen_db(99)
    lanes = [owner, owner.create_lane()]
    clients = [sa.Client(pg, bytes([60 + i] * 32), out_n=out_n) for i in range(2)]
    for srv, cl in zip(lanes, clients):
        srv.set_pub_params_seeded(cl.pub_params("seeded"))
    idx = [11, clients[0].n_items - 2]
    results, _ = P.answer_batch_seeded(lanes, [cl.query(i, "seeded") for cl, i in zip(clients, idx)])
    for b, cl in enumerate(clients):
        assert_eq(cl.decode(results[b][0])[0], oracle.pack_db_item(po, out_n, 99, idx[b]), f"lane {b}")
    for x in [lanes[1], owner] + clients:
        x.close()
