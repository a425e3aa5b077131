"""The database fingerprint (include/spiral_gpu.h "Fingerprints") restated in Python integers, for the tests: no library code, only pow(r, e, P).

P = 2^61 - 1; key -> r = 2 + key[0] mod (P - 3), s = 2 + key[1] mod (P - 3);
f(item) = sum over q, c of x[q][c] * r^(2048 q + c + 1) mod P;  F = sum over items i of f(item i) * s^(i + 1) mod P, i the database index."""
import numpy as np

P = 2**61 - 1
N = 2048


def bases(key):
    return 2 + key[0] % (P - 3), 2 + key[1] % (P - 3)


def item_fingerprint(key, polys, poly0=0):
    """f over the polynomials polys[k] (each 2048 coefficients), which are the polynomials poly0 + k of their item"""
    r, _ = bases(key)
    f = 0
    for k, poly in enumerate(polys):
        assert len(poly) == N
        e = N * (poly0 + k) + 1
        w = pow(r, e, P)
        for x in poly:
            x = int(x)
            if x:
                f += x * w
            w = w * r % P
    return f % P


def fingerprints(key, items, poly0=0, first_item=0):
    """(F, [f per item]) of items[k] = the polynomials poly0 .. of database item first_item + k"""
    _, s = bases(key)
    fs = [item_fingerprint(key, it, poly0) for it in items]
    F = sum(f * pow(s, first_item + k + 1, P) for k, f in enumerate(fs)) % P
    return F, fs


def combine(key, fs, ids):
    """F of item fingerprints fs[k] of the database items ids[k], summed over the list as given"""
    _, s = bases(key)
    return sum(int(f) * pow(s, int(i) + 1, P) for f, i in zip(fs, ids)) % P


def pack_bits(values, bits):
    """the little-endian bit string of `bits`-wide values (a whole number of bytes), as the item stream of load_db_items lays a polynomial out"""
    acc = 0
    for k, v in enumerate(values):
        v = int(v)
        assert 0 <= v < 2**bits
        acc |= v << (k * bits)
    n = len(values) * bits
    assert n % 8 == 0
    return np.frombuffer(acc.to_bytes(n // 8, "little"), dtype=np.uint8)
