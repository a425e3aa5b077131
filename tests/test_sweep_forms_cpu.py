"""CPU-side checks of what tests/test_gpu_sweep_forms.py stands on: the limb model of tests/limb_edges.py (the decomposition the header of
csrc/sweep_mfma.hip states) is exact and stays inside the bounds the kernel's comments claim at K = 4096 terms; the sprinkled edge set finds
defects of the decomposition; and the stage call spiral_gpu_fast_multiply_queries_by_database_dim1 with the counter "mfma_sweeps" is declared,
exported, documented and checks its arguments before it touches a device."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import limb_edges as L  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sa():
    import spiral_amd

    spiral_amd.build()
    return spiral_amd


# ---- the decomposition ------------------------------------------------------------------------------------------------------------------
def check_decomposition(values, m):
    a = np.asarray(values, dtype=np.int64)
    s, t = L.TRUE.db_limbs(a, m), L.TRUE.query_limbs(a, m)
    assert ((s[..., :3] >= -128) & (s[..., :3] <= 127)).all() and ((s[..., 3] >= 0) & (s[..., 3] <= 15)).all(), "database limbs: three signed bytes, a 4-bit top"
    assert ((t[..., :3] >= -128) & (t[..., :3] <= 127)).all() and ((t[..., 3] >= 0) & (t[..., 3] <= 16)).all(), "query limbs: three signed bytes, top 0 .. 16"
    stored = L.recompose(s)
    assert (stored == np.where(a >= L.WRAP, a - m, a)).all(), "database limbs recompose to a'' = a or a - m"
    assert ((stored >= -L.BIAS) & (stored < L.WRAP)).all() and ((stored - a) % m == 0).all()
    assert (L.recompose(t) == a).all(), "query limbs recompose to v"


@pytest.mark.parametrize("prime", [0, 1])
def test_decomposition_is_exact_on_edges_and_uniform_residues(prime):
    m = L.MODS[prime]
    edges = [v for v in L.EDGES[prime] if v < m]
    assert {0, 1, m - 1} <= set(edges) and (prime == 1 or {L.WRAP - 1, L.WRAP, L.WRAP + 1} <= set(edges))
    check_decomposition(edges, m)
    check_decomposition(np.random.default_rng(40 + prime).integers(0, m, size=100_000), m)
    for a in edges:  # the per-term form is the product, mod m
        for v in edges:
            form = L.term_form(L.TRUE.db_limbs(np.array(a), m), L.TRUE.query_limbs(np.array(v), m), m)
            assert (form - a * v) % m == 0, (a, v)


# ---- the bounds behind combine_limbs and mod_est -------------------------------------------------------------------------------------------
# the search made when the tests were asked for: a check of extreme_pairs, not its source
FOUND = {L.P: ((260013951, 260013951), (260013696, 260013952)), L.B: ((243236735, 243236735), (8355712, 243236480))}


@pytest.mark.parametrize("m", L.MODS)
def test_extreme_pairs_and_the_bounds_at_full_k(m):
    """K = 4096 terms of the operand pair that maximises (minimises) the per-term form: every int32 limb sum within K 2^14, |sum| < m 2^30 (so the
    biased sum is positive) and sum + m 2^30 < 2^59 (mod_est's domain).  The same from the box bound, which holds for ANY residues."""
    (hi, hi_form), (lo, lo_form) = L.extreme_pairs(m)
    assert (hi, lo) == FOUND[m]
    assert lo_form < 0 < hi_form and max(hi_form, -lo_form) <= L.box_bound(m)
    K = L.K_MAX
    for (a, v), form in ((hi, hi_form), (lo, lo_form)):
        assert a < m and v < m
        c, total = L.TRUE.sums(np.full(K, a), np.full(K, v), m)
        assert total == K * form
        assert max(abs(x) for row in c for x in row) <= K << 14, "an int32 limb sum beyond K 2^14"
        assert abs(total) < m << 30 and 0 <= total + (m << 30) < 1 << 59
        assert (total + (m << 30)) % m == (K * a * v) % m
    worst = K * L.box_bound(m)  # 2^51.3 (p), 2^53.2 (b)
    assert worst < 1 << 54 and worst < m << 30 and worst + (m << 30) < 1 << 59
    # the figures the search gave: K terms of the extremes reach about 2^51.2 (p) and 2^53.1 (b)
    assert abs(np.log2(K * hi_form) - {L.P: 51.2, L.B: 53.1}[m]) < 0.05


def mod_est(x, m):
    """mod_est of sweep_mfma.hip on a 64-bit x: quotient estimated in double, remainder fixed up in 32 bits"""
    hi, lo = x >> 32, x & 0xFFFFFFFF
    xd = float(hi) * 4294967296.0 + float(lo)
    q = int(xd * (1.0 / float(m))) & 0xFFFFFFFF
    r = (lo - q * m) & 0xFFFFFFFF
    if r >> 31:
        r = (r + m) & 0xFFFFFFFF
    return r - m if r >= m else r


@pytest.mark.parametrize("m", L.MODS)
def test_mod_est_is_exact_below_2_59(m):
    rng = np.random.default_rng(m % 1000)
    xs = [int(x) for x in rng.integers(0, 1 << 59, size=100_000, dtype=np.uint64)]
    for k in (1, 2, (1 << 30) - 1, 1 << 30, (1 << 30) + 1, ((1 << 59) - 1) // m):  # either side of multiples of m, up to the domain's end
        xs += [k * m - 1, k * m, k * m + 1]
    xs += [0, 1, m - 1, (1 << 59) - 1]
    (hi, hi_form), (lo, lo_form) = L.extreme_pairs(m)
    xs += [L.K_MAX * hi_form + (m << 30), L.K_MAX * lo_form + (m << 30), L.K_MAX * L.box_bound(m) + (m << 30), (m << 30) - L.K_MAX * L.box_bound(m)]
    for x in xs:
        if 0 <= x < 1 << 59:
            assert mod_est(x, m) == x % m, x


# ---- the edge set earns its place -------------------------------------------------------------------------------------------------------------
OUTPUTS, TERMS = 24, 128  # 3072 terms per prime and data set: 24 outputs of one 128-term piece


def operand_sets(kind, prime):
    m = L.MODS[prime]
    rng = np.random.default_rng(500 + prime)
    both = [np.stack([rng.integers(0, mm, size=OUTPUTS * TERMS, dtype=np.uint64) for mm in L.MODS]) for _ in range(2)]
    if kind == "sprinkled":
        for x in both:
            L.sprinkle(rng, x[:, None, :], 0)
    a, v = (x[prime].reshape(OUTPUTS, TERMS) for x in both)
    return m, a, v


def triggers(model, a, v, m):
    """operand values whose limbs the model reads differently from the true decomposition"""
    return int((model.db_limbs(a, m) != L.TRUE.db_limbs(a, m)).any(axis=-1).sum() + (model.query_limbs(v, m) != L.TRUE.query_limbs(v, m)).any(axis=-1).sum())


@pytest.mark.parametrize("kind", ["uniform", "sprinkled"])
@pytest.mark.parametrize("prime", [0, 1])
def test_the_model_agrees_with_the_exact_product(kind, prime):
    m, a, v = operand_sets(kind, prime)
    for k in range(OUTPUTS):
        assert L.TRUE.dot(a[k], v[k], m) == sum(int(x) * int(y) for x, y in zip(a[k], v[k])) % m


@pytest.mark.parametrize("defect", list(L.DEFECTS))
def test_defective_models_are_caught_by_the_sprinkled_data(defect):
    """Three defective readings of the decomposition, each held against the exact product on uniform and on sprinkled operands of the same size
    (prime p: prime b has no wrap point and no top limb 16).  Every one of them differs on the sprinkled data.  On any data a defect shows on an
    output exactly when one of that output's operands is a value the defect misreads, and those values, from the model alone, are:
      no wrap at 2^28 - 0x808080     the wrap point itself (one residue of p): uniform data of this size never holds it -- only the edge set finds it
      query top limb cut to 4 bits   every query residue of p from the wrap point up, 3.1 % of them: found on uniform data too
      byte -128 read as +128         every residue with a zero byte in its biased word, 3 in 256: found on uniform data too
    so the last two are within reach of whole-answer tests on uniform operands; the expectation that all three agree on uniform data holds for
    the first alone, and the test states which it is for each."""
    model = L.DEFECTS[defect]
    seen = {}
    for kind in ("uniform", "sprinkled"):
        m, a, v = operand_sets(kind, 0)
        wrong = 0
        for k in range(OUTPUTS):
            differs = model.dot(a[k], v[k], m) != sum(int(x) * int(y) for x, y in zip(a[k], v[k])) % m
            assert differs == (triggers(model, a[k], v[k], m) > 0), f"{defect}, {kind} output {k}"
            wrong += differs
        seen[kind] = wrong
    assert seen["sprinkled"] > 0, f"the sprinkled data does not find: {defect}"
    uniform_rate = {"no wrap at 2^28 - 0x808080": 0.0, "query top limb cut to 4 bits": (L.P - L.WRAP) / L.P, "byte -128 read as +128": 2 * 3 / 256}[defect]
    if uniform_rate == 0.0:
        assert seen["uniform"] == 0, "found by uniform data: not a defect that needs the edge set"
    else:  # a uniform output of 128 terms holds none of the misread values with probability (1 - rate)^128 < 5 %
        assert seen["uniform"] >= OUTPUTS // 2


def test_prime_b_has_no_wrap_and_no_top_limb_16():
    """why the defects above are held against prime p: no residue of b reaches the wrap point, as a database value or as a query value"""
    assert L.B <= L.WRAP < L.P
    m, a, v = operand_sets("sprinkled", 1)
    for name in ("no wrap at 2^28 - 0x808080", "query top limb cut to 4 bits"):
        assert triggers(L.DEFECTS[name], a, v, m) == 0
    assert triggers(L.DEFECTS["byte -128 read as +128"], a, v, m) > 0


def test_exact_reads_the_reference_layouts():
    """exact() against a direct evaluation on tiny arrays in both layouts (dim0 = 4; only slots 0 and N - 1 filled)"""
    rng = np.random.default_rng(9)
    dim0, num_per = 4, 2
    word = lambda shape: rng.integers(0, L.P, size=shape, dtype=np.uint64) | (rng.integers(0, L.B, size=shape, dtype=np.uint64) << np.uint64(32))
    re = np.zeros((L.N, dim0, 2, 4), dtype=np.uint64)
    db = np.zeros((L.N, num_per, 2, dim0, 2), dtype=np.uint64)
    for z in (0, L.N - 1):
        re[z, :, :, :3], db[z] = word((dim0, 2, 3)), word((num_per, 2, dim0, 2))
    pos = [(1, 2, 1, 1, L.N - 1), (0, 0, 0, 0, 0)]
    want = [sum((int(re[z, j, mm, r]) >> 32 * n & 0xFFFFFFFF) * (int(db[z, i, c, j, mm]) >> 32 * n & 0xFFFFFFFF) for j in range(dim0) for mm in range(2)) % L.MODS[n]
            for i, r, c, n, z in pos]
    assert L.exact(db.reshape(-1), re, pos) == want
    re1 = np.zeros((L.N, dim0, 2), dtype=np.uint64)
    db1 = np.zeros((L.N, num_per, dim0), dtype=np.uint64)
    for z in (0, L.N - 1):
        re1[z], db1[z] = word((dim0, 2)), word((num_per, dim0))
    pos1 = [(1, 1, 1, L.N - 1), (0, 0, 0, 0)]
    want1 = [sum((int(re1[z, j, r]) >> 32 * n & 0xFFFFFFFF) * (int(db1[z, i, j]) >> 32 * n & 0xFFFFFFFF) for j in range(dim0)) % L.MODS[n] for i, r, n, z in pos1]
    assert L.exact(db1.reshape(-1), re1, pos1) == want1


# ---- the stage call and the counter ---------------------------------------------------------------------------------------------------------
NAME = "spiral_gpu_fast_multiply_queries_by_database_dim1"


def test_the_stage_call_is_declared_exported_and_documented(sa):
    from spiral_amd import _lib

    assert NAME in _lib.PROTOTYPES and hasattr(sa.lib(), NAME)
    assert callable(sa.fastMultiplyQueriesByDatabaseDim1) and sys.modules["spiral_amd.pack"].fastMultiplyQueriesByDatabaseDim1 is sa.fastMultiplyQueriesByDatabaseDim1
    header = open(os.path.join(ROOT, "include", "spiral_gpu.h")).read()
    readme = open(os.path.join(ROOT, "README.md")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for text in (header, readme, integration):
        assert NAME in text and "mfma_sweeps" in text


@pytest.mark.parametrize("n,trials,dim0,num_per,message", [(0, 1, 128, 8, "queries per pass"), (9, 1, 128, 8, "queries per pass"), (1, 0, 128, 8, "trials"),
                                                          (1, 1, 0, 8, "first dimension"), (1, 1, 127, 8, "first dimension"), (1, 1, 128, 0, "ciphertexts per slot")])
def test_bad_arguments_fail_before_any_device_call(sa, n, trials, dim0, num_per, message):
    """-1 and a message naming the argument; the buffers are never read (they are eight words long), and no device is needed to get there"""
    buf = np.zeros(8, dtype=np.uint64)
    p = buf.ctypes.data_as(C.POINTER(C.c_uint64))
    assert getattr(sa.lib(), NAME)(p, p, p, n, trials, dim0, num_per) == -1
    assert message in sa.lib().spiral_gpu_last_error().decode()
    assert not buf.any()


def test_null_buffers_fail(sa):
    buf = np.zeros(8, dtype=np.uint64)
    p, null = buf.ctypes.data_as(C.POINTER(C.c_uint64)), C.POINTER(C.c_uint64)()
    for args in ((null, p, p), (p, null, p), (p, p, null)):
        assert getattr(sa.lib(), NAME)(*args, 1, 1, 128, 8) == -1
        assert "null argument" in sa.lib().spiral_gpu_last_error().decode()


def test_the_python_call_raises_on_bad_arguments(sa):
    re = np.zeros((L.N, 2, 2), dtype=np.uint64)
    db = np.zeros((L.N, 1, 2), dtype=np.uint64)
    with pytest.raises(sa.SpiralGpuError, match="queries per pass"):
        sa.fastMultiplyQueriesByDatabaseDim1([db], [], 2, 1)
    with pytest.raises(sa.SpiralGpuError, match="queries per pass"):
        sa.fastMultiplyQueriesByDatabaseDim1([db], [re] * 9, 2, 1)
    with pytest.raises(sa.SpiralGpuError, match="trials"):
        sa.fastMultiplyQueriesByDatabaseDim1([], [re], 2, 1)


def test_mfma_sweeps_reads_zero_in_a_fresh_process(sa):
    code = "import spiral_amd as sa; print('count', sa.get_option('mfma_sweeps'))"
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.split() == ["count", "0"], r.stdout


def test_mfma_sweeps_is_read_only(sa):
    count = sa.get_option("mfma_sweeps")
    for v in (0, 1):
        with pytest.raises(sa.SpiralGpuError, match="mfma_sweeps"):
            sa.set_option("mfma_sweeps", v)
    assert sa.get_option("mfma_sweeps") == count
