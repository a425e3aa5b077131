"""Every narrow instantiation of the matrix-core sweep (csrc/sweep_mfma.hip) on operands of the test's choosing: the base W = 4, 2, 1 forms (option
"sweep_narrow", through multiplyQueriesByDatabase) and the three ROWS = 2 forms of SpiralPack -- wide, NARROW and, with option "pack_pair_blocks",
PAIR -- through fastMultiplyQueriesByDatabaseDim1, which also checks guard words behind the last trial's accumulators.  Operands are uniform
residues with the limb decomposition's edge values sprinkled over 3 % of them (tests/limb_edges.py), or constant fields at the limb edges and at the
pairs that drive the recombined sum furthest from zero.  Every comparison is bit-exact: whole outputs against the oracle, 64 sampled outputs per case
against the product in Python integers, constant fields against their closed form.  Every case reads the counter "mfma_sweeps": +1 where the
matrix-core form is taken, +0 in the fallbacks.

Instantiations reached (NT = column tiles: base (12 n + 15) / 16, pack (8 n + 15) / 16 for n queries):
  base   W = 4, 2, 1 (nu2 = 5, 4, 3) x NT = 1 .. 6 (n = 1, 2, 3 | 4, 5, 6, 7 | 8)          18
  pack   PAIR, NARROW, wide x NT = 1 .. 4 (n = 1 | 2, 3 | 4, 5 | 6, 7 | 8)                  12
Full K (4096 terms per sum, the most the kernels admit) runs once per family on constant fields: the only large cases."""
import functools
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limb_edges as L  # noqa: E402

pytestmark = pytest.mark.gpu
N = L.N
SAMPLES = 64


@pytest.fixture(scope="module")
def sa():
    # torch first: it ships its own HIP runtime and the two must not be initialised in the opposite order
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


def assert_eq(got, exp, what):
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[:5].tolist()}: got {got[tuple(bad[0])]}, exp {exp[tuple(bad[0])]}")


class counted:
    """the matrix-core sweep launches made inside the block"""

    def __init__(self, sa, rise, what):
        self.sa, self.rise, self.what = sa, rise, what

    def __enter__(self):
        self.before = self.sa.get_option("mfma_sweeps")

    def __exit__(self, exc_type, exc, tb):
        if exc_type is None:
            rose = self.sa.get_option("mfma_sweeps") - self.before
            assert rose == self.rise, f"{self.what}: mfma_sweeps rose by {rose}, expected {self.rise}"


# ---- operands ---------------------------------------------------------------------------------------------------------------------------------
def words(rng, count):
    """`count` words p | b << 32 of uniform residues with the edge values sprinkled over them"""
    both = np.stack([rng.integers(0, m, size=count, dtype=np.uint64) for m in L.MODS])
    L.sprinkle(rng, both[:, None, :], 0)
    return both[0] | (both[1] << np.uint64(32))


def frozen(a):
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=1)  # (the cases of a geometry follow one another)
def base_world(nu1, nu2):
    """a database, eight queries in reorientCiphertexts' layout (row 3 of 4 is padding) and the oracle outputs computed so far"""
    rng = np.random.default_rng(3000 + 16 * nu1 + nu2)
    dim0, num_per = 1 << nu1, 1 << nu2
    db = frozen(words(rng, dim0 * num_per * 4 * N))
    res = []
    for _ in range(8):
        re = np.zeros((N, dim0, 2, 4), dtype=np.uint64)
        re[..., :3] = words(rng, N * dim0 * 2 * 3).reshape(N, dim0, 2, 3)
        res.append(frozen(re))
    return db, res, {}


@functools.lru_cache(maxsize=1)
def pack_world(dim0, num_per, trials):
    """`trials` images in convertDb's layout, eight queries in reorientCiphertextsDim1's, and the oracle outputs computed so far"""
    rng = np.random.default_rng(5000 + 64 * num_per + trials + dim0)
    dbs = [frozen(words(rng, N * num_per * dim0)) for _ in range(trials)]
    res = [frozen(words(rng, N * dim0 * 2).reshape(N, dim0, 2)) for _ in range(8)]
    return dbs, res, {}


def check_samples(got, pick, seed, sprinkled=True):
    """SAMPLES output words against the product in Python integers; pick(index of got) -> (database, query, position as limb_edges.operands takes it)"""
    rng = np.random.default_rng(seed)
    with_edges = 0
    for ix in L.sample_positions(rng, got.shape, SAMPLES):
        db, q, pos = pick(ix)
        d, v = L.operands(db, q, pos)
        with_edges += bool(L.is_edge(d, pos[-2]).any() or L.is_edge(v, pos[-2]).any())
        assert int(got[ix]) == L.exact(db, q, [pos])[0], f"output {ix} differs from the exact product"
    if sprinkled:
        assert with_edges >= SAMPLES // 2, "the sampled outputs' operands hold no sprinkled edges"


# ---- constant fields ---------------------------------------------------------------------------------------------------------------------------
LIMB_MINUS, LIMB_PLUS = (15 << 24) - L.BIAS, (14 << 24) - L.BIAS + 0xFFFFFF  # three limb bytes of -128 under top 15 / of +127 under top 14
VALUES = {"max": (L.P - 1, L.B - 1), "limb-": (LIMB_MINUS,) * 2, "limb+": (LIMB_PLUS,) * 2, "wrap": (L.WRAP, L.B - 1), "zero": (0, 0)}
# (query, database) fields: the five of test_matrix_core_sweep_extremes, then both primes' pairs that maximise / minimise the recombined sum
FIELDS = [("max", "max"), ("limb-", "limb-"), ("limb-", "limb+"), ("wrap", "max"), ("zero", "max"), ("form", "max"), ("form", "min")]
extremes = functools.lru_cache(maxsize=None)(L.extreme_pairs)


def field(vq, vd):
    """((query residue mod p, mod b), (database residue mod p, mod b))"""
    if vq == "form":
        (dp, qp), (db_, qb) = (extremes(m)[0 if vd == "max" else 1][0] for m in L.MODS)
    else:
        (qp, qb), (dp, db_) = VALUES[vq], VALUES[vd]
    assert max(qp, dp) < L.P and max(qb, db_) < L.B
    return (qp, qb), (dp, db_)


def base_field(sa, dim0, num_per, n, vq, vd):
    (qp, qb), (dp, db_) = field(vq, vd)
    re = np.zeros((N, dim0, 2, 4), dtype=np.uint64)
    re[..., :3] = qp | (qb << 32)
    db = np.full(dim0 * num_per * 4 * N, dp | (db_ << 32), dtype=np.uint64)
    with counted(sa, 1, f"base field ({vq}, {vd})"):
        got = sa.multiplyQueriesByDatabase([re] * n, db, dim0, num_per)
    assert got.shape == (n, num_per, 3, 2, 2, N)
    assert (got[..., 0, :] == (2 * dim0 * qp * dp) % L.P).all() and (got[..., 1, :] == (2 * dim0 * qb * db_) % L.B).all(), f"2 dim0 vq vd mod m, ({vq}, {vd})"


def pack_field(sa, dim0, num_per, trials, n, vq, vd):
    (qp, qb), (dp, db_) = field(vq, vd)
    re = np.full((N, dim0, 2), qp | (qb << 32), dtype=np.uint64)
    db = np.full(N * num_per * dim0, dp | (db_ << 32), dtype=np.uint64)
    with counted(sa, 1, f"pack field ({vq}, {vd})"):
        got = sa.fastMultiplyQueriesByDatabaseDim1([db] * trials, [re] * n, dim0, num_per)
    assert got.shape == (n, trials, num_per, 2, 2, N)
    assert (got[..., 0, :] == (dim0 * qp * dp) % L.P).all() and (got[..., 1, :] == (dim0 * qb * db_) % L.B).all(), f"dim0 vq vd mod m, ({vq}, {vd})"


# ---- the base W forms ---------------------------------------------------------------------------------------------------------------------------
# nu1 = 6: one piece of 128 terms per prime, every (NT, W); nu1 = 7: two pieces (the prime boundary inside an item, the run-ahead across items)
BASE = [(6, nu2, n) for nu2 in (3, 4, 5) for n in range(1, 9)] + [(7, nu2, n) for nu2 in (3, 4, 5) for n in (3, 8)]


@pytest.mark.parametrize("nu1,nu2,n", BASE)
def test_base_w_forms_on_sprinkled_operands(sa, oracle, opts, nu1, nu2, n):
    O = oracle
    opts(sweep_narrow=1)
    dim0, num_per = 1 << nu1, 1 << nu2
    db, res, want = base_world(nu1, nu2)
    with counted(sa, 1, f"W = {num_per // 8}, {n} queries"):
        got = sa.multiplyQueriesByDatabase(res[:n], db, dim0, num_per)
    for b in range(n):
        if b not in want:
            want[b] = O.multiply_query_by_database(res[b], db, dim0, num_per)
        assert_eq(got[b], want[b], f"({nu1}, {nu2}): query {b} of {n} against the oracle")
    check_samples(got, lambda ix: (db, res[ix[0]], ix[1:]), 100 * nu1 + 10 * nu2 + n)


@pytest.mark.parametrize("vq,vd", FIELDS)
@pytest.mark.parametrize("nu2", [3, 4, 5])
def test_base_w_forms_on_constant_fields(sa, opts, nu2, vq, vd):
    opts(sweep_narrow=1)
    base_field(sa, 128, 1 << nu2, 3, vq, vd)


# ---- the ROWS = 2 forms --------------------------------------------------------------------------------------------------------------------------
# (dim0, num_per, trials, n)
PAIR = [(128, 8, 3, n) for n in range(1, 9)] + [(128, 8, 1, 2), (128, 8, 17, 5), (256, 8, 3, 4)]  # odd trials and six surplus waves; a single, half-empty
#                                                                                                 pair-block; two groups, both ragged ends
NARROW = [(128, 16, 9, 3), (128, 16, 9, 8), (128, 32, 3, 1), (128, 32, 3, 6), (128, 64, 3, 2), (128, 64, 3, 4), (128, 64, 3, 7), (256, 16, 3, 5)]  # (16, 9): a ragged second group
WIDE = [(128, 128, 2, 1), (128, 128, 2, 3), (128, 128, 2, 5), (128, 128, 2, 8), (128, 256, 1, 4), (256, 128, 1, 2)]  # (256, 1): two column groups per trial


def run_pack(sa, O, dim0, num_per, trials, n, rise):
    dbs, res, want = pack_world(dim0, num_per, trials)
    with counted(sa, rise, f"dim0 = {dim0}, {num_per} per slot, {trials} trials, {n} queries"):
        got = sa.fastMultiplyQueriesByDatabaseDim1(dbs, res[:n], dim0, num_per)
    assert got.shape == (n, trials, num_per, 2, 2, N)
    for b in range(n):
        for t in range(trials):
            if (b, t) not in want:
                want[b, t] = O.sweep_dim1(dbs[t], res[b], dim0, num_per)
            assert_eq(got[b, t], want[b, t], f"query {b} of {n}, trial {t} of {trials} against the oracle")
    check_samples(got, lambda ix: (dbs[ix[1]], res[ix[0]], ix[2:]), 1000 * num_per + 10 * trials + n)


@pytest.mark.parametrize("dim0,num_per,trials,n", PAIR)
def test_pack_pair_form_on_sprinkled_operands(sa, oracle, opts, dim0, num_per, trials, n):
    opts(pack_pair_blocks=1)
    run_pack(sa, oracle, dim0, num_per, trials, n, 1)


@pytest.mark.parametrize("dim0,num_per,trials,n", NARROW)
def test_pack_narrow_form_on_sprinkled_operands(sa, oracle, dim0, num_per, trials, n):
    run_pack(sa, oracle, dim0, num_per, trials, n, 1)


@pytest.mark.parametrize("dim0,num_per,trials,n", WIDE)
def test_pack_wide_form_on_sprinkled_operands(sa, oracle, dim0, num_per, trials, n):
    run_pack(sa, oracle, dim0, num_per, trials, n, 1)


@pytest.mark.parametrize("vq,vd", FIELDS)
@pytest.mark.parametrize("num_per,trials", [(8, 3), (16, 3), (128, 1)], ids=["pair", "narrow", "wide"])
def test_pack_forms_on_constant_fields(sa, opts, num_per, trials, vq, vd):
    opts(pack_pair_blocks=1)
    pack_field(sa, 128, num_per, trials, 3, vq, vd)


@pytest.mark.parametrize("dim0,num_per,trials,pair_blocks", [(128, 4, 2, 1), (128, 8, 3, 0), (64, 16, 2, 1)], ids=["4-per-slot", "pair-option-off", "dim0-64"])
def test_pack_fallbacks_sweep_on_the_vector_alu(sa, oracle, opts, dim0, num_per, trials, pair_blocks):
    """geometries without a limb-plane form: one vector-ALU sweep per query, the same results, no matrix-core launch"""
    opts(pack_pair_blocks=pair_blocks)
    run_pack(sa, oracle, dim0, num_per, trials, 2, 0)


# ---- full K ------------------------------------------------------------------------------------------------------------------------------------
FULL_K = [("limb-", "limb-"), ("form", "max")]  # all limb bytes -128 in both operands; each prime's maximising pair


def timed(request, what, call):
    t0 = time.perf_counter()
    call()
    line = f"full K, {what}: {time.perf_counter() - t0:.2f} s"
    print(line)
    request.config._spiral_evidence.append(line)


@pytest.mark.parametrize("vq,vd", FULL_K)
def test_base_w1_at_full_k(sa, opts, request, vq, vd):
    """nu1 = 11, nu2 = 3: K = 4096 terms per sum, W = 1, 1 GiB of database words"""
    opts(sweep_narrow=1)
    timed(request, f"base W = 1 ({vq}, {vd})", lambda: base_field(sa, 2048, 8, 2, vq, vd))


@pytest.mark.parametrize("vq,vd", FULL_K)
@pytest.mark.parametrize("num_per", [8, 16], ids=["pair", "narrow"])
def test_pack_forms_at_full_k(sa, opts, request, num_per, vq, vd):
    """dim0 = 4096, one trial: PAIR (512 MiB of database words) and NARROW (1 GiB)"""
    opts(pack_pair_blocks=1)
    timed(request, f"pack {num_per} per slot ({vq}, {vd})", lambda: pack_field(sa, 4096, num_per, 1, 2, vq, vd))
