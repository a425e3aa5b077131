"""Crafted inputs for the fold's balanced gadget digits (split_and_crt, src/spiral.cpp:270-330), shared by tests/test_digit_edges_cpu.py and
tests/test_gpu_digit_edges.py.  Pure Python / numpy: importable without a GPU and without the oracle.

balanced_digits() is the reference's carry walk written out in Python integers.  It shares no code with oracle/spiral_oracle.c or with the
kernels (csrc/digits_device.h), so a misreading of the walk that the C restatement and the kernels had in common would show against it.
crafted_pair() places the values on which a carry compare, a shift wrap or a bias constant can go wrong, and coverage_gaps() states as
conditions -- evaluated from the walk alone, before any output is looked at -- that the set really contains them."""
import functools

import numpy as np

N = 2048
Q = 268369921 * 249561089  # < 2^56
ELLS = tuple(range(2, 29))  # every gadget dimension the server accepts
# the forms the pair-form loaders take (csrc/digits_device.h sdigit_diff8); every other dimension folds through the two-product form
TIER_SFAST = (4, 6, 8, 10, 12, 15, 16, 19, 20)
TIER_SDIG32 = (3, 5, 7, 9, 11, 13, 21, 22)
TIER_GENERIC = (2,)
PAIR_ELLS = tuple(sorted(TIER_SFAST + TIER_SDIG32 + TIER_GENERIC))
N_VALUES = 6 * N  # the coefficients of one ciphertext: H and L of one fold round at num_per = 2


def bits_per(ell):
    """get_bits_per (include/util.h:34-38) for logQ = 56"""
    return 1 if ell == 56 else 56 // ell + 1


def chain_start(k, ell):
    return 0 if k < ell // 2 else ell // 2


def may_borrow(k, ell):
    """the first chain's last digit never borrows, every other digit may"""
    half = ell // 2
    return k + 1 < half if k < half else True


def free_digits(ell):
    """the digit positions a value below Q can set freely: wholly below bit 56 and not the digit that holds the value's top bits"""
    return range(55 // bits_per(ell))


def walk(v, ell):
    """[(plain digit, carry in, balanced digit)] for k = 0 .. ell - 1: two chains, 0 .. ell/2 - 1 and ell/2 .. ell - 1; a piece (digit + carry)
    above B/2 borrows B from the next digit of its chain, except at the first chain's last digit; digits at bit 64 and beyond are 0"""
    bits = bits_per(ell)
    base = 1 << bits
    half = ell // 2
    out, carry = [], 0
    for k in range(ell):
        if k == half:
            carry = 0
        sh = k * bits
        dig = 0 if sh >= 64 else (v >> sh) & (base - 1)
        piece = dig + carry
        if piece > base // 2 and may_borrow(k, ell):
            out.append((dig, carry, piece - base))
            carry = 1
        else:
            out.append((dig, carry, piece))
            carry = 0
    return out


def balanced_digits(v, ell):
    """the signed digits of v: sum(d_k B^k) over a chain recomposes the chain's bits"""
    return [d for _, _, d in walk(int(v), ell)]


class Table:
    """the walk of many values: dig, cin, d as [n][ell] int64 arrays"""

    def __init__(self, values, ell):
        w = np.array([walk(int(v), ell) for v in np.asarray(values).reshape(-1)], dtype=np.int64).reshape(-1, ell, 3)
        self.ell, self.dig, self.cin, self.d = ell, w[:, :, 0], w[:, :, 1], w[:, :, 2]


def digits_mod_q(table, shape):
    """balanced digits as raw polynomials in split_and_crt's row order: values [num][3][2][N] -> [num][3 ell][2][N], row = r + 3 k, a
    negative digit d written as Q + d"""
    num, ell = shape[0], table.ell
    d = np.where(table.d < 0, table.d + Q, table.d).astype(np.uint64).reshape(num, 3, 2, N, ell)
    return np.ascontiguousarray(d.transpose(0, 4, 1, 2, 3)).reshape(num, 3 * ell, 2, N)


# ---- the generator -------------------------------------------------------------------------------------------------------------
def alphabet(ell):
    b = 1 << bits_per(ell)
    return [0, 1, b // 2 - 1, b // 2, b // 2 + 1, b - 1]


def crafted_values(ell, n=N_VALUES, seed=0):
    """n values in [0, Q), deterministic in (ell, n, seed): the constants 0, 1, Q/2, Q - 1; for every free digit k past its chain's first, a
    carry source (B/2 or B/2 + 1) at the chain's first digit, a run of B/2 or of B - 1 up to k, and every letter of the alphabet at k; whole
    chains of B/2 and of B - 1; an eighth uniform; the rest composed digit by digit from the alphabet {0, 1, B/2 - 1, B/2, B/2 + 1, B - 1}.
    The top digit is drawn below Q's own, so every composition stays below Q."""
    rng = np.random.default_rng(1000 * seed + ell)
    bits = bits_per(ell)
    b = 1 << bits
    al = alphabet(ell)
    free = list(free_digits(ell))
    ktop = len(free)
    top_max = Q >> (ktop * bits)

    def compose(fixed):
        v = int(rng.integers(0, top_max)) << (ktop * bits)
        for k in free:
            v |= (fixed[k] if k in fixed else al[int(rng.integers(0, 6))]) << (k * bits)
        return v

    vals = [0, 1, Q // 2, Q - 1]
    for k in free:
        s = chain_start(k, ell)
        if k == s:
            continue
        for head in (b // 2, b // 2 + 1):
            for run in (b // 2, b - 1):
                for letter in al:
                    vals.append(compose({s: head, k: letter, **{i: run for i in range(s + 1, k)}}))
    for s in {chain_start(k, ell) for k in free}:
        chain = [k for k in free if chain_start(k, ell) == s]
        for run in (b // 2, b - 1):
            vals.append(compose({k: run for k in chain}))
            vals.append(compose({k: run for k in free}))
    assert len(vals) <= n // 4, "the structured part must leave most of the set to the composed values"
    vals += [int(x) for x in rng.integers(0, Q, size=n // 8)]
    rest = n - len(vals)
    idx = rng.integers(0, 6, size=(rest, ktop))
    comp = rng.integers(0, top_max, size=rest).astype(np.uint64) << np.uint64(ktop * bits)
    lut = np.array(al, dtype=np.uint64)
    for k in free:
        comp |= lut[idx[:, k]] << np.uint64(k * bits)
    out = np.concatenate([np.array(vals, dtype=np.uint64), comp])
    assert out.shape == (n,) and int(out.max()) < Q
    return out[rng.permutation(n)]


class Pair:
    """one fold round's inputs at num_per = 2: raw[0] = L, raw[1] = H ([3][2][N] each), L a shuffle of the H values"""

    def __init__(self, ell, seed=0):
        self.ell = ell
        h = crafted_values(ell, seed=seed)
        l = h[np.random.default_rng(77000 + 1000 * seed + ell).permutation(h.size)]
        self.raw = np.ascontiguousarray(np.stack([l, h]).reshape(2, 3, 2, N))
        self.table = Table(self.raw, ell)  # rows [0, 6 N): L, rows [6 N, 12 N): H
        self.gaps = coverage_gaps(ell, self.table, N_VALUES)


@functools.lru_cache(maxsize=None)
def crafted_pair(ell, seed=0):
    return Pair(ell, seed)


# ---- the coverage conditions -----------------------------------------------------------------------------------------------------
def coverage_gaps(ell, table, n_low):
    """the conditions the crafted set must meet, from the walk alone; returns what is missing (empty: all hold).  Rows [0, n_low) of the
    table are the L values, the rest the H values paired with them in order."""
    bits = bits_per(ell)
    b = 1 << bits
    dig, cin, d = table.dig[n_low:], table.cin[n_low:], table.d[n_low:]
    diff = d - table.d[:n_low]
    gaps = []

    def need(cond, what, k):
        if not bool(np.any(cond)):
            gaps.append(f"ell={ell} k={k}: no {what}")

    for k in free_digits(ell):
        s = chain_start(k, ell)
        j = k - s
        need((dig[:, k] == b // 2) & (cin[:, k] == 0), "piece B/2 without a carry in", k)
        if j >= 1:
            need((dig[:, k] == b // 2 - 1) & (cin[:, k] == 1), "piece brought to B/2 by a carry", k)
            need((dig[:, k] == b // 2) & (cin[:, k] == 1), "digit B/2 with a carry in", k)
            need((dig[:, k] == b - 1) & (cin[:, k] == 1), "digit B - 1 with a carry in (piece == B)", k)
            # the carry threshold of the chain prefix met exactly: every lower digit of the chain B/2, no carry arrives
            need(np.all(dig[:, s:k] == b // 2, axis=1) & (cin[:, k] == 0), "chain prefix of B/2 digits alone (no carry)", k)
        if j >= 2:
            need((dig[:, s] == b // 2 + 1) & np.all(dig[:, s + 1:k] == b // 2, axis=1) & (cin[:, k] == 1), "carry through a run of B/2 spanning the chain prefix", k)
        if may_borrow(k, ell):
            lo, hi = -(b - 1), b - 1
        elif j >= 1:  # the first chain's last digit keeps its piece, B included
            lo, hi = -b, b
        else:  # ... and without a carry in (ell = 2, 3) it is the plain digit
            lo, hi = -(b - 1), b - 1
        if int(diff[:, k].max()) != hi or int(diff[:, k].min()) != lo:
            gaps.append(f"ell={ell} k={k}: digit differences span [{int(diff[:, k].min())}, {int(diff[:, k].max())}], not [{lo}, {hi}]")
    return gaps


def extra_values(ell, seed=0):
    """a third ciphertext for the split_and_crt stage op: uniform values, and Q itself, which the raw contract allows (the walk is on the
    value as given)"""
    rng = np.random.default_rng(5000 + 1000 * seed + ell)
    x = rng.integers(0, Q, size=(3, 2, N), dtype=np.uint64)
    x[0, 0, :3] = Q
    x[1, 1, 1000] = Q
    x[2, 1, N - 1] = Q
    return x


# ---- keys and expected values (through the oracle module the caller hands in) --------------------------------------------------------
_KEYS = {}


def fold_keys(O, ell, nu1=2, nu2=1):
    """a client's public parameters and a query at t_gsw = ell, and the GSW matrices the oracle's expansion and conversion make of them"""
    if (ell, nu1, nu2) not in _KEYS:
        po = O.make_params(nu1, nu2, t_gsw=ell)
        cl = O.Client(po, seed=100 + ell)
        pp = cl.pub_params()
        q = cl.query(3)
        _, gsw = O.stage_convert(po, O.stage_expand(po, q, pp[0], pp[1]), pp[2], pp[3])
        _KEYS[ell, nu1, nu2] = dict(po=po, pp=pp, q=q, gsw=gsw, want=O.stage_fold(po, crafted_pair(ell).raw, gsw) if (nu1, nu2) == (2, 1) else None)
    return _KEYS[ell, nu1, nu2]
