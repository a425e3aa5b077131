"""Batched SpiralPack answers (include/spiral_gpu.h, spiral_gpu_pack_server_answer_batch): n <= 8 clients' queries, one per server -- an owner
and its lanes -- with ONE first-dimension pass over the trial images (the matrix-core sweep of csrc/sweep_mfma.hip where the geometry is covered,
one vector-ALU sweep per lane elsewhere).  Every lane's response, packed ciphertext and accumulators must equal the oracle's and its own single
answer's, whatever form the image is in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2048
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sa():
    # torch first: it ships its own HIP runtime and the two must not be initialised in the opposite order
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0
    return spiral_amd


@pytest.fixture(scope="module")
def P(sa):
    from spiral_amd import pack as _  # noqa: F401  (spiral_amd.pack is also the name of a function: take the module itself)
    import sys

    return sys.modules["spiral_amd.pack"]


def assert_eq(got, exp, what):
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[:5].tolist()}")


def lanes_of(sa, O, po, pg, out_n, n, db_seed, client_seed=100):
    """an owner with the device-generated database and n - 1 lanes, each lane with its own client's public parameters (a client draws new
    ones on every pub_params() call: the lanes' own are kept in clients[b].pp)"""
    owner = sa.PackServer(pg, out_n)
    owner.gen_db(db_seed)
    servers = [owner] + [owner.create_lane() for _ in range(n - 1)]
    clients = []
    for b, srv in enumerate(servers):
        cl = O.PackClient(po, out_n, seed=client_seed + 17 * b)
        cl.pp = cl.pub_params()
        srv.set_pub_params(*cl.pp)
        clients.append(cl)
    return servers, clients


def indices(s, n, salt=0):
    total = s.dim0 * s.num_per
    return [(salt + 1 + 7919 * b) % total if b else total - 1 for b in range(n)]


COVERED = [
    (7, 7, 1, {}),                                                        # num_per = 128, dim0 = 128: the smallest covered shape
    (7, 8, 1, dict(t_gsw=4)),                                             # num_per = 256: two column groups per trial
    (7, 7, 2, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1)),   # direct upload, four trials
]
UNCOVERED = [
    (6, 2, 2, {}),                                                        # 4 output columns
    (6, 7, 1, {}),                                                        # 128 columns, but a 64-term first dimension (half a piece)
    (3, 2, 12, dict(t_gsw=3, t_conv=56, t_exp=56, qprime_bits=31, p_db=524288, direct_upload=1)),  # n = 12, t_conv = 56
]


@pytest.mark.parametrize("nu1,nu2,out_n,kw,n,covered", [g + (n, True) for g, n in zip(COVERED, (8, 3, 2))] + [g + (n, False) for g, n in zip(UNCOVERED, (3, 2, 2))])
def test_batch_matches_oracle(sa, P, oracle_mt, nu1, nu2, out_n, kw, n, covered):
    O = oracle_mt
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    db = O.pack_gen_db(po, out_n, 41)
    servers, clients = lanes_of(sa, O, po, pg, out_n, n, 41)
    idx = indices(s, n)
    qs = [cl.query(i) for cl, i in zip(clients, idx)]
    out, us = P.answer_batch(servers, qs, want_packed=True)
    assert us["n"] == n and us["total_us"] > 0
    for b in range(n):
        wl, wr, v, vw = clients[b].pp
        exp_resp, exp_packed = O.pack_answer(po, out_n, qs[b], wl, wr, v, vw, db)
        assert_eq(out[b][1], exp_packed, f"lane {b}: packed ciphertext")
        assert_eq(out[b][0], exp_resp, f"lane {b}: response")
        assert_eq(clients[b].decode(out[b][0]), O.pack_db_item(po, out_n, 41, idx[b]), f"lane {b}: decoded items")
    assert servers[0].db_format() == (P.DB_LIMBS if covered else P.DB_PACKED)
    for srv in servers:
        srv.close()


def _singles(srv, q, trials):
    resp, packed, _ = srv.answer(q)
    return resp, packed, srv.read_response_wire(), [srv.read_acc(t) for t in range(trials)]


def test_batch_equals_singles(sa, P, oracle):
    """singles on the packed image first, then the batch (which converts the image): responses, wire forms, packed ciphertexts and the
    accumulators of every trial of every lane bit for bit; afterwards single answers on the limb-plane image still match"""
    O = oracle
    nu1, nu2, out_n, kw, n = 7, 8, 2, dict(t_gsw=4), 4
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    servers, clients = lanes_of(sa, O, po, pg, out_n, n, 5)
    qs = [cl.query(i) for cl, i in zip(clients, indices(s, n, 3))]
    bytes0 = servers[0].db_device_bytes()
    assert servers[0].db_format() == P.DB_PACKED
    single = [_singles(srv, q, s.trials) for srv, q in zip(servers, qs)]
    assert servers[1].db_format() == P.DB_PACKED  # a single answer never converts
    out, _ = P.answer_batch(servers, qs, want_packed=True)
    assert servers[0].db_format() == P.DB_LIMBS and servers[n - 1].db_format() == P.DB_LIMBS
    assert servers[0].db_device_bytes() == bytes0 == servers[1].db_device_bytes()  # converted in place: no second image
    for b, srv in enumerate(servers):
        resp, packed, wire, accs = single[b]
        assert_eq(out[b][0], resp, f"lane {b}: response")
        assert_eq(out[b][1], packed, f"lane {b}: packed ciphertext")
        assert_eq(srv.read_response_wire(), wire, f"lane {b}: wire form")
        for t in range(s.trials):
            assert_eq(srv.read_acc(t), accs[t], f"lane {b}, trial {t}: accumulators")
    # one query alone on the limb-plane image: the one-query instance of the matrix-core sweep
    for b in (0, n - 1):
        again = _singles(servers[b], qs[b], s.trials)
        assert_eq(again[0], single[b][0], f"lane {b}: single answer on the limb-plane image")
        assert_eq(again[1], single[b][1], f"lane {b}: packed ciphertext on the limb-plane image")
        for t in range(s.trials):
            assert_eq(again[3][t], single[b][3][t], f"lane {b}, trial {t}: accumulators on the limb-plane image")
    ms = P.time_sweep_batch(servers, 3)
    assert ms > 0
    for srv in servers:
        srv.close()


def test_image_forms_and_reloads(sa, P, oracle):
    O = oracle
    nu1, nu2, out_n, kw, n = 7, 7, 2, {}, 3
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    servers, clients = lanes_of(sa, O, po, pg, out_n, n, 21)
    owner = servers[0]
    qs = [cl.query(i) for cl, i in zip(clients, indices(s, n, 11))]
    bytes0 = owner.db_device_bytes()
    ref = owner.answer(qs[0])[0]
    owner.set_db_format(P.DB_LIMBS)
    assert owner.db_format() == P.DB_LIMBS and owner.db_device_bytes() == bytes0
    assert_eq(owner.answer(qs[0])[0], ref, "single answer on the limb-plane image")
    owner.set_db_format(P.DB_PACKED)
    assert owner.db_format() == P.DB_PACKED and owner.db_device_bytes() == bytes0
    assert_eq(owner.answer(qs[0])[0], ref, "single answer after packed -> limbs -> packed")
    with pytest.raises(sa.SpiralGpuError):
        servers[1].set_db_format(P.DB_LIMBS)  # a lane converts nothing
    with pytest.raises(sa.SpiralGpuError):
        servers[1].gen_db(3)  # loads through a lane fail
    # a batch converts; a reload with another seed then gives the oracle's answers for the new database, as a batch and alone
    P.answer_batch(servers, qs)
    assert owner.db_format() == P.DB_LIMBS
    owner.gen_db(77)
    db77 = O.pack_gen_db(po, out_n, 77)
    out, _ = P.answer_batch(servers, qs)
    for b in range(n):
        assert_eq(out[b][0], O.pack_answer(po, out_n, qs[b], *clients[b].pp, db77)[0], f"lane {b} after gen_db(77)")
    # one trial uploaded over the limb-plane image (the image goes back to packed form first, the other trials keep their words)
    db77[1] = O.pack_gen_db(po, out_n, 78)[1]
    owner.load_db(1, db77[1])
    assert owner.db_format() == P.DB_PACKED
    out, _ = P.answer_batch(servers, qs)
    for b in range(n):
        assert_eq(out[b][0], O.pack_answer(po, out_n, qs[b], *clients[b].pp, db77)[0], f"lane {b} after load_db of trial 1")
    # fill_db_random over a limb-plane image: a correct packed image again (the batch and the single answer agree)
    owner.fill_db_random(9)
    assert owner.db_format() == P.DB_PACKED
    alone = servers[2].answer(qs[2], want_packed=False)[0]
    out, _ = P.answer_batch(servers, qs)
    assert_eq(out[2][0], alone, "random database: batch vs single")
    owner.close()  # the lanes keep the image alive
    out, _ = P.answer_batch(servers[1:], qs[1:])
    assert_eq(out[1][0], alone, "lane after its owner was destroyed")
    for srv in servers[1:]:
        srv.close()
    # no limb-plane form on an uncovered geometry
    small = sa.PackServer(sa.make_params(6, 2), 2)
    small.gen_db(1)
    with pytest.raises(sa.SpiralGpuError, match="limb-plane"):
        small.set_db_format(P.DB_LIMBS)
    assert small.db_format() == P.DB_PACKED
    small.close()


def test_batch_validation(sa, P, oracle):
    O = oracle
    nu1, nu2, out_n = 6, 2, 2
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    servers, clients = lanes_of(sa, O, po, pg, out_n, 3, 2)
    qs = [cl.query(i) for cl, i in zip(clients, indices(s, 3))]
    out, _ = P.answer_batch(servers, qs, want_packed=True)
    before = [(srv.read_response_wire(), srv.read_acc(0)) for srv in servers]
    L = sa.lib()
    hs = (C.c_void_p * 9)(*([servers[0].h] * 9))

    def c_batch(n):
        rc = L.spiral_gpu_pack_server_answer_batch(hs, n, None, None, None, None)
        assert rc != 0
        return L.spiral_gpu_last_error().decode()

    assert "no servers" in c_batch(0)
    assert "at most 8 clients" in c_batch(9)
    with pytest.raises(ValueError):
        P.answer_batch([], [])
    with pytest.raises(ValueError):
        P.answer_batch([servers[0]] + [servers[1]] * 8, qs * 3)
    with pytest.raises(ValueError):
        P.answer_batch([servers[0], servers[0]], qs[:2])
    other, other_cl = lanes_of(sa, O, po, pg, out_n, 2, 2, client_seed=7)
    with pytest.raises(sa.SpiralGpuError, match="database image"):
        P.answer_batch([servers[0], other[1]], qs[:2])  # a lane of another owner
    mism = sa.PackServer(sa.make_params(nu1, nu2, t_gsw=4), out_n)
    mism.gen_db(2)
    mism.set_pub_params(*O.PackClient(O.make_params(nu1, nu2, t_gsw=4), out_n, seed=3).pub_params())
    with pytest.raises(sa.SpiralGpuError):
        P.answer_batch([servers[0], mism], qs[:2])  # other parameters (and another image)
    bare = servers[0].create_lane()
    with pytest.raises(sa.SpiralGpuError, match="public parameters"):
        P.answer_batch([servers[0], bare], qs[:2])
    sharded = sa.PackServer(pg, out_n, trial0=0, trial1=2)
    sharded.gen_db(2)
    with pytest.raises(sa.SpiralGpuError, match="trial-sharded"):
        sharded.create_lane()
    sharded.set_pub_params(*clients[0].pp)
    with pytest.raises(sa.SpiralGpuError, match="trial-sharded"):
        P.answer_batch([sharded], qs[:1])
    fresh = servers[0].create_lane()
    fresh.set_pub_params(*clients[1].pp)
    with pytest.raises(sa.SpiralGpuError, match="converted query"):
        P.time_sweep_batch([servers[0], fresh])
    for b, srv in enumerate(servers):
        assert_eq(srv.read_response_wire(), before[b][0], f"lane {b}: response after the refused calls")
        assert_eq(srv.read_acc(0), before[b][1], f"lane {b}: accumulators after the refused calls")
    for srv in servers + other + [mism, bare, fresh, sharded]:
        srv.close()


def _random_batch_sets(count, seed):
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        covered = len(out) % 2 == 0
        nu1, nu2, out_n = (7, 7, 1) if covered else (int(rng.integers(2, 7)), int(rng.integers(1, 6)), int(rng.choice([1, 2, 3, 4, 5])))
        kw = dict(t_gsw=int(rng.integers(2, 9)), t_conv=int(rng.choice([2, 3, 4, 8, 16, 56])), t_exp=int(rng.choice([2, 4, 8, 16, 56])),
                  qprime_bits=int(rng.integers(14, 37)), p_db=int(rng.choice([2, 256, 4096, 65536])), direct_upload=int(rng.integers(0, 2)))
        if out_n * out_n * (1 << (nu1 + nu2)) > 16384:
            continue
        if not kw["direct_upload"] and kw["t_gsw"] * nu2 > (1 << nu1):
            continue
        out.append((nu1, nu2, out_n, kw, int(rng.integers(2, 9))))
    return out


@pytest.mark.parametrize("nu1,nu2,out_n,kw,n", _random_batch_sets(4, 11), ids=[f"set{i}" for i in range(4)])
def test_random_batch_sets(sa, P, oracle, nu1, nu2, out_n, kw, n):
    O = oracle
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    db = O.pack_gen_db(po, out_n, 3)
    servers, clients = lanes_of(sa, O, po, pg, out_n, n, 3, client_seed=nu1 + 10 * nu2)
    idx = indices(s, n, 5)
    qs = [cl.query(i) for cl, i in zip(clients, idx)]
    out, _ = P.answer_batch(servers, qs, want_packed=True)
    for b in range(n):
        exp_resp, exp_packed = O.pack_answer(po, out_n, qs[b], *clients[b].pp, db)
        assert_eq(out[b][1], exp_packed, f"lane {b}: packed ciphertext, params {nu1},{nu2},{out_n},{kw}")
        assert_eq(out[b][0], exp_resp, f"lane {b}: response")
    for srv in servers:
        srv.close()


@pytest.mark.slow
def test_config5_batch_of_four_equals_singles(sa, P, oracle_mt, request):
    """configs[4] (SpiralPack nu1=10, nu2=8, n=4, 16 trial images of 3.75 GiB): four lanes answered alone on the packed image, then as one
    batch (which converts the image in place): every lane's response and trial 5's accumulators bit for bit, and each lane's decoded item"""
    M = oracle_mt
    kw = dict(t_gsw=8, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=20, p_db=256)
    po, pg = M.make_params(10, 8, **kw), sa.make_params(10, 8, **kw)
    out_n, n, seed = 4, 4, 2024
    s = M.pack_shape_of(po, out_n)
    servers, clients = lanes_of(sa, M, po, pg, out_n, n, seed, client_seed=12)
    idx = indices(s, n, 123456)
    qs = [cl.query(i) for cl, i in zip(clients, idx)]
    single = []
    for srv, q in zip(servers, qs):
        resp, _, _ = srv.answer(q, want_packed=False)
        single.append((resp, srv.read_acc(5)))
    out, us = P.answer_batch(servers, qs)
    assert servers[0].db_format() == P.DB_LIMBS
    for b in range(n):
        assert_eq(out[b][0], single[b][0], f"config 5, lane {b}: batch response vs its single answer")
        assert_eq(servers[b].read_acc(5), single[b][1], f"config 5, lane {b}: trial 5 accumulators")
        assert_eq(clients[b].decode(out[b][0]), M.pack_db_item(po, out_n, seed, idx[b]), f"config 5, lane {b}: decoded item")
    getattr(request.config, "_spiral_evidence", []).append(
        f"config 5 batch of {n}: every lane bit-exact with its single answer; shared sweep {us['first_dim_us']:.0f} us, batch {us['total_us']:.0f} us")
    for srv in servers:
        srv.close()


@pytest.mark.parametrize("args,env", [
    (["7", "7", "300", "a", "--high-rate", "--batch", "3", "--seed", "4"], {"OUTN": "1"}),  # covered: the shared matrix-core pass
    (["6", "7", "77", "a", "--high-rate", "--batch", "3", "--seed", "5"], {"OUTN": "2"}),  # uncovered: one sweep per lane
])
def test_cli_high_rate_batch(sa, args, env):
    e = dict(os.environ)
    e.update(env)
    r = subprocess.run([os.path.join(ROOT, "spiral_amd", "spiral")] + args, capture_output=True, text=True, env=e, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Is correct? : 1" in r.stdout
    assert "Batch of 3 queries, Is correct?: 1 1 1" in r.stdout, r.stdout[-2000:]
