"""The crafted carry-chain inputs of tests/digit_edges.py without a GPU: the set meets its coverage conditions for every gadget dimension, the
oracle's split_and_crt is the Python walk on it, and the fold result the GPU tests expect is the reference's formula evaluated from that walk."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digit_edges as D  # noqa: E402


def test_walk_on_worked_values():
    """ell = 4: 15-bit digits, chains (0, 1) and (2, 3); digit 1 never borrows"""
    b = 1 << 15
    assert D.bits_per(4) == 15 and D.bits_per(2) == 29 and D.bits_per(28) == 3
    assert D.balanced_digits(0, 4) == [0, 0, 0, 0]
    assert D.balanced_digits(b // 2, 4) == [b // 2, 0, 0, 0]                          # B/2 stays
    assert D.balanced_digits(b // 2 + 1, 4) == [-(b // 2 - 1), 1, 0, 0]                # B/2 + 1 borrows
    assert D.balanced_digits((b // 2 + 1) | ((b - 1) << 15), 4) == [-(b // 2 - 1), b, 0, 0]  # the chain's last digit keeps piece == B
    v = ((b // 2 + 1) << 30) | ((b // 2) << 45)                                       # second chain: a carry onto B/2 borrows again
    assert D.balanced_digits(v, 4) == [0, 0, -(b // 2 - 1), -(b // 2 - 1)]
    v = ((b // 2) << 30) | ((b // 2) << 45)                                           # ... and B/2 alone does not
    assert D.balanced_digits(v, 4) == [0, 0, b // 2, b // 2]
    # ell = 28: 3-bit digits, digits 22 .. 27 start at bit 66 and beyond
    assert D.balanced_digits(D.Q - 1, 28)[22:] == [0] * 6
    for ell in D.ELLS:  # each chain's digits recompose the chain's bits wherever nothing is cut off at bit 64
        bits, half = D.bits_per(ell), ell // 2
        for v in (1, D.Q // 2, D.Q - 1, D.Q):
            d = D.balanced_digits(v, ell)
            if (ell - 1) * bits < 64:
                assert sum(x << (k * bits) for k, x in enumerate(d)) == v, (ell, v)
            assert sum(x << (k * bits) for k, x in enumerate(d[:half])) == v & ((1 << (half * bits)) - 1), (ell, v)


def test_tiers_partition_the_pair_form_dimensions():
    """fold_pair_exact (csrc/kernels.h): the digits recompose the value and the last offset is below bit 64"""
    exact = [ell for ell in D.ELLS if ell * D.bits_per(ell) >= 57 and (ell - 1) * D.bits_per(ell) < 64]
    assert list(D.PAIR_ELLS) == exact == [2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 19, 20, 21, 22]
    assert len(set(D.PAIR_ELLS)) == len(D.TIER_SFAST) + len(D.TIER_SDIG32) + len(D.TIER_GENERIC)


@pytest.mark.parametrize("ell", D.ELLS)
def test_crafted_set_meets_its_coverage(ell):
    p = D.crafted_pair(ell)
    assert p.raw.shape == (2, 3, 2, D.N) and int(p.raw.max()) < D.Q
    assert not p.gaps, "\n".join(p.gaps)


def test_coverage_check_notices_a_thinner_set():
    """uniform values alone miss the rare carry conditions (8-bit digits here): the check is not vacuous"""
    rng = np.random.default_rng(1)
    t = D.Table(rng.integers(0, D.Q, size=2 * 4096, dtype=np.uint64), 8)
    gaps = D.coverage_gaps(8, t, 4096)
    assert any("carry through a run" in g for g in gaps) and any("digit differences" in g for g in gaps)


@pytest.mark.parametrize("ell", D.ELLS)
def test_oracle_split_and_crt_is_the_python_walk(oracle, ell):
    """orc_split_and_crt == to_ntt of balanced_digits on the crafted set and on the value Q itself"""
    O = oracle
    p = D.crafted_pair(ell)
    assert not p.gaps, "\n".join(p.gaps)
    extra = D.extra_values(ell)
    raw = np.concatenate([p.raw, extra[None]])
    exp = np.concatenate([D.digits_mod_q(p.table, p.raw.shape), D.digits_mod_q(D.Table(extra, ell), (1,))])
    got = O.from_ntt(O.split_and_crt(raw, ell))  # back to digits mod Q: a mismatch names its coefficient
    if not np.array_equal(got, exp):
        i, row, c, z = (int(x) for x in np.argwhere(got != exp)[0])
        raise AssertionError(f"ell={ell} k={row // 3} v={int(raw[i, row % 3, c, z])}: oracle digit {int(got[i, row, c, z])}, walk {int(exp[i, row, c, z])}")
    assert np.array_equal(O.split_and_crt(raw, ell), O.to_ntt(exp))


@pytest.mark.parametrize("ell", [8, 5, 2])  # one dimension per pair-form tier
def test_fold_expectation_is_the_reference_formula(oracle, ell):
    """at nu2 = 1 the fold is Q_neg G^-1(L) + Q G^-1(H) with Q_neg = G2 - Q (src/spiral.cpp:1349-1410, :2361-2379): evaluated from the Python
    digits with the oracle's ring operations only, it is what stage_fold gives -- the value the GPU tests compare with does not rest on the
    C walk"""
    O = oracle
    k = D.fold_keys(O, ell)
    p = D.crafted_pair(ell)
    dg = O.to_ntt(D.digits_mod_q(p.table, p.raw.shape))  # [2][3 ell][2] NTT: G^-1(L), G^-1(H)
    gsw = k["gsw"][0]
    g2 = O.build_gadget(3, 3 * ell)
    q_neg = O.to_ntt((g2.astype(object) - O.from_ntt(gsw).astype(object)) % D.Q)
    want = O.from_ntt(O.add(O.multiply(q_neg, dg[0]), O.multiply(gsw, dg[1])))
    assert np.array_equal(want, O.stage_fold(k["po"], p.raw, k["gsw"]))



def test_write_acc_rejects_null_arguments():
    import spiral_amd as sa

    assert sa.lib().spiral_gpu_server_write_acc(None, None) != 0
    assert b"null" in sa.lib().spiral_gpu_last_error()
