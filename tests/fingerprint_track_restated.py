"""The tracked fingerprint (include/spiral_gpu.h "Fingerprints", Tracked) restated for the tests: no library code.

With P = 2^61 - 1 and r, s from the key as tests/fingerprint_restated.py states them:
    g(i, q) = sum over c of x[q][c] * r^(c + 1) mod P          -- the polynomial sum, one table word
    f(i)    = sum over q of g(i, q) * r^(2048 q) mod P
    F       = sum over database indices i of f(i) * s^(i + 1) mod P
    apply:    replacing g_old by g_new at (i, q) moves F by (g_new - g_old) * r^(2048 q) * s^(i + 1) mod P.

g over a whole database is the one place numpy does the arithmetic, exactly: a weight below 2^61 is split into three limbs below 2^21, a coefficient is
below 2^24 (asserted), so a product is below 2^45 and a sum of 2048 of them below 2^56: no uint64 wraps, and the limbs are recombined in Python integers."""
import numpy as np

import fingerprint_restated as FR

P, N = FR.P, FR.N
_LIMB = 21


def _weight_limbs(key):
    r, _ = FR.bases(key)
    w, cur = [], r
    for _ in range(N):
        w.append(cur)
        cur = cur * r % P
    return np.array([[(v >> (_LIMB * k)) & ((1 << _LIMB) - 1) for k in range(3)] for v in w], dtype=np.uint64)  # [c][limb]


def poly_sums(key, polys):
    """g of every polynomial of `polys` (any shape [..., 2048], coefficients below 2^24) -> a uint64 array of shape [...]"""
    x = np.ascontiguousarray(polys, dtype=np.uint64)
    assert x.shape[-1] == N and (x.size == 0 or int(x.max()) < 1 << 24)
    limbs = x.reshape(-1, N) @ _weight_limbs(key)  # [polynomial][limb], each below 2^56
    g = [(int(a) + (int(b) << _LIMB) + (int(c) << (2 * _LIMB))) % P for a, b, c in limbs]
    return np.array(g, dtype=np.uint64).reshape(x.shape[:-1])


def poly_sum_slow(key, poly):
    """g of one polynomial in Python integers alone (what poly_sums is checked against)"""
    r, _ = FR.bases(key)
    return sum(int(x) * pow(r, c + 1, P) for c, x in enumerate(poly)) % P


def item_values(key, g, poly0=0):
    """[f per item] of g[item][q], the polynomials poly0 + q"""
    r, _ = FR.bases(key)
    return [sum(int(v) * pow(r, N * (poly0 + q), P) for q, v in enumerate(row)) % P for row in g]


def combined(key, g, poly0=0, ids=None, first_item=0):
    """F of g[k][q], row k being database item ids[k] (default first_item + k)"""
    _, s = FR.bases(key)
    f = item_values(key, g, poly0)
    ids = range(first_item, first_item + len(f)) if ids is None else ids
    return sum(v * pow(s, int(i) + 1, P) for v, i in zip(f, ids)) % P


def apply(key, F, g_old, g_new, q, i):
    """F after the table word of polynomial q of database item i goes from g_old to g_new"""
    r, s = FR.bases(key)
    return (F + (int(g_new) - int(g_old)) * pow(r, N * q, P) * pow(s, i + 1, P)) % P
