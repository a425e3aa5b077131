"""The fold's balanced-digit loaders (csrc/digits_device.h through csrc/ntt.hip) on crafted carry-chain inputs: tests/digit_edges.py places a
digit equal to B/2 with and without a carry in, carries through runs of B/2 and of B - 1, piece == B and the extreme digit differences at
every free digit of every gadget dimension, and spiral_gpu_server_write_acc puts those ciphertexts where the first fold round reads them.
Every comparison is bit-exact.  Geometry: nu1 = 2, nu2 = 1 (num_per = 2, one fold round) unless stated.

Which loader a route reaches ("The balanced-digit loaders"):
  split_and_crt stage op, write_raw + fold(), fold_chain = 0      LD_SDIGIT (sdigit_of)
  write_acc + lift() + fold(), run_post(), pair-form dimensions   LD_SDIFF (sfast / sdig32 / generic by dimension), fwd2 = 0 / 1: either kernel
  write_acc + run_post(), fold_pair = 0                           fold_chain_kernel (sdigit_of on the lift held in LDS)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import digit_edges as D  # noqa: E402

pytestmark = pytest.mark.gpu


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


def canon(O, a):
    a = a.copy()
    a[..., 0, :] %= O.P
    a[..., 1, :] %= O.B
    return a


def crafted(ell):
    """the crafted pair of a dimension, its coverage asserted before any GPU output is looked at"""
    p = D.crafted_pair(ell)
    assert not p.gaps, "\n".join(p.gaps)
    return p


def keyed_server(sa, k):
    """a server holding the fold keys of D.fold_keys (its own expansion and conversion of the same query); created after the test's opts()"""
    srv = sa.Server(sa.make_params(k["po"].nu1, k["po"].nu2, t_gsw=k["po"].t_gsw))
    srv.set_pub_params(*k["pp"])
    srv.set_query(k["q"])
    srv.expand()
    srv.convert()
    return srv


# ---- a. the stage op: LD_SDIGIT, every dimension ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_gsw", D.ELLS)
def test_split_and_crt_is_the_python_walk(sa, oracle, t_gsw):
    O = oracle
    p = crafted(t_gsw)
    extra = D.extra_values(t_gsw)  # uniform values and Q itself
    raw = np.concatenate([p.raw, extra[None]])
    digits = np.concatenate([D.digits_mod_q(p.table, p.raw.shape), D.digits_mod_q(D.Table(extra, t_gsw), (1,))])
    got = canon(O, sa.split_and_crt(raw, t_gsw))
    exp = O.to_ntt(digits)
    if not np.array_equal(got, exp):  # back to digits mod Q, so that the failure names the coefficient
        back = O.from_ntt(got)
        i, row, c, z = (int(x) for x in np.argwhere(back != digits)[0])
        raise AssertionError(f"split_and_crt ell={t_gsw} k={row // 3} v={int(raw[i, row % 3, c, z])}: digit {int(back[i, row, c, z])} (mod Q), the walk gives "
                             f"{int(digits[i, row, c, z])}; {int((got != exp).sum())} transformed words differ")


# ---- b. the pair form from the accumulators: LD_SDIFF in both digit kernels --------------------------------------------------------------
@pytest.mark.parametrize("fwd2", [0, 1])
@pytest.mark.parametrize("ell", D.PAIR_ELLS)
def test_pair_form_from_the_accumulators(sa, oracle, opts, ell, fwd2):
    """fwd2 = 0: ntt_forward_kernel (with its one-word loads where a chain lies in one word); fwd2 = 1: ntt_forward2_kernel, two digits per
    workgroup, an odd dimension's last job carrying one"""
    O = oracle
    from spiral_amd import server as SV

    p = crafted(ell)
    k = D.fold_keys(O, ell)
    opts(fwd2=fwd2)
    srv = keyed_server(sa, k)
    acc = O.to_ntt(p.raw)
    srv.write_acc(acc)
    assert_eq(srv.read(SV.BUF_ACC), acc, f"ell={ell}: accumulators as written")
    srv.lift()
    assert_eq(srv.read(SV.BUF_RAW), p.raw, f"ell={ell}: lift of the written accumulators")
    srv.fold()  # the stage API after lift(): LD_SDIFF on the lifted ciphertexts, the accumulators as the addend
    assert_eq(srv.read(SV.BUF_FINAL), k["want"], f"ell={ell} fwd2={fwd2}: lift() + fold()")
    srv.use_graphs(True)
    for rep in range(2):  # captured, then replayed
        srv.write_acc(acc)
        srv.run_post()  # the lift chained into round 0
        srv.sync()
        assert_eq(srv.read(SV.BUF_FINAL), k["want"], f"ell={ell} fwd2={fwd2}: run_post() with graphs, pass {rep}")
    srv.close()


# ---- c. the two-product forms, every dimension ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ell", D.ELLS)
def test_two_product_fold_from_written_raw(sa, oracle, ell):
    """write_raw + fold(): LD_SDIGIT"""
    O = oracle
    from spiral_amd import server as SV

    p = crafted(ell)
    k = D.fold_keys(O, ell)
    srv = keyed_server(sa, k)
    srv.write_raw(p.raw)
    srv.fold()
    assert_eq(srv.read(SV.BUF_FINAL), k["want"], f"ell={ell}: write_raw() + fold()")
    srv.close()


@pytest.mark.parametrize("ell,env", [(ell, dict(fold_pair=0)) for ell in D.ELLS]
                         + [(ell, dict(fold_pair=0, fold_blocks=fb)) for ell in (2, 9, 23) for fb in (0, 1000000)]  # every digit in one block; one block per digit
                         + [(ell, dict(fold_chain=0)) for ell in D.ELLS])
def test_two_product_fold_from_the_accumulators(sa, oracle, opts, ell, env):
    """fold_pair = 0: fold_chain_kernel, the lift held in LDS; fold_chain = 0: a lift launch, then LD_SDIGIT"""
    O = oracle
    from spiral_amd import server as SV

    p = crafted(ell)
    k = D.fold_keys(O, ell)
    opts(**env)
    srv = keyed_server(sa, k)
    srv.write_acc(O.to_ntt(p.raw))
    srv.run_post()
    srv.sync()
    assert_eq(srv.read(SV.BUF_FINAL), k["want"], f"ell={ell} {env}: run_post()")
    srv.close()


# ---- e. the dimensions no other test runs: one whole query each ---------------------------------------------------------------------------------
@pytest.mark.parametrize("t_gsw", [13, 15, 16, 18, 19, 20, 21, 22, 23, 28])
def test_whole_query_at_unvisited_dimensions(sa, oracle, t_gsw):
    """(nu1, nu2) = (3, 2): the second round chains from a product; from t_gsw = 23 on digit offsets pass bit 64"""
    O = oracle
    from spiral_amd import server as SV

    po, pg = O.make_params(3, 2, t_gsw=t_gsw), sa.make_params(3, 2, t_gsw=t_gsw)
    cl = O.Client(po, seed=200 + t_gsw)
    pp = cl.pub_params()
    db = O.gen_db(po, 31)
    srv = sa.Server(pg)
    srv.gen_db(31)
    srv.set_pub_params(*pp)
    q = cl.query(21)
    fin, _, _ = srv.answer(q)
    assert_eq(fin, O.answer(po, q, *pp, db), f"t_gsw={t_gsw}: answer()")
    q = cl.query(10)
    srv.use_graphs(True)
    srv.set_query(q)
    srv.run_query()
    srv.sync()
    assert_eq(srv.read(SV.BUF_FINAL), O.answer(po, q, *pp, db), f"t_gsw={t_gsw}: run_query() with graphs")
    srv.close()
