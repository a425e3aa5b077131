"""The SpiralPack batch's shared matrix-core pass at 8 ciphertexts per slot (csrc/sweep_mfma.hip, the PAIR form of sweep_mfma_kernel<NT, 2>: the 16
rows of a wave's operand are the 8 columns of two adjacent trials), taken only under option "pack_pair_blocks" = 1.  Every comparison is bit for bit:
against the lanes' own single answers on the PACKED image (the vector-ALU sweep) and against the CPU oracle (pack_answer, pack_db_item)."""
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2048


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

    return sys.modules["spiral_amd.pack"]


def assert_eq(got, exp, what):
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[:5].tolist()}")


def lanes_of(sa, O, po, pg, out_n, n, db_seed, client_seed=100, clients=None):
    """an owner with the device-generated database and n - 1 lanes, each with its own client's public parameters (kept in clients[b].pp)"""
    owner = sa.PackServer(pg, out_n)
    owner.gen_db(db_seed)
    servers = [owner] + [owner.create_lane() for _ in range(n - 1)]
    if clients is None:
        clients = []
        for b in range(n):
            cl = O.PackClient(po, out_n, seed=client_seed + 17 * b)
            cl.pp = cl.pub_params()
            clients.append(cl)
    for srv, cl in zip(servers, clients):
        srv.set_pub_params(*cl.pp)
    return servers, clients


def indices(s, n, salt=0):
    total = s.dim0 * s.num_per
    return [(salt + 1 + 7919 * b) % total if b else total - 1 for b in range(n)]


def single_state(srv, q, trials):
    resp, packed, _ = srv.answer(q)
    return resp, packed, srv.read_response_wire(), [srv.read_acc(t) for t in range(trials)]


def batch_states(P, servers, qs, trials):
    out, us = P.answer_batch(servers, qs, want_packed=True)
    assert us["n"] == len(servers) and us["total_us"] > 0
    return [(out[b][0], out[b][1], srv.read_response_wire(), [srv.read_acc(t) for t in range(trials)]) for b, srv in enumerate(servers)]


def assert_state_eq(got, exp, what):
    assert_eq(got[0], exp[0], f"{what}: response")
    assert_eq(got[1], exp[1], f"{what}: packed ciphertext")
    assert_eq(got[2], exp[2], f"{what}: wire form")
    assert len(got[3]) == len(exp[3])
    for t, (a, b) in enumerate(zip(got[3], exp[3])):
        assert_eq(a, b, f"{what}: accumulators of trial {t}")


def close_all(*groups):
    for g in groups:
        for srv in g:
            srv.close()


DIRECT = dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1)
PAIRS = [
    # nu1, nu2, out_n, params, clients     trials -> pair-blocks
    (7, 3, 1, {}, 2),       # 1 -> 1: the upper half of the only pair-block is surplus, 7 surplus waves, one piece per prime
    (8, 3, 2, {}, 8),       # 4 -> 2: first dimension 256 (sums carried across two pieces per prime), NT = 4 full
    (7, 3, 3, {}, 3),       # 9 -> 5: the last pair-block half empty; NT = 2 with a partly filled tile
    (7, 3, 5, {}, 2),       # 25 -> 13: one full group of 8 pair-blocks, then a ragged group whose last block is half empty
    (7, 3, 2, DIRECT, 2),   # records taken from an uploaded query
]


@pytest.mark.parametrize("nu1,nu2,out_n,kw,n", PAIRS, ids=[f"{g[0]}-{g[1]}-{g[2]}{'-direct' if g[3].get('direct_upload') else ''}" for g in PAIRS])
def test_pair_batch_equals_singles_and_oracle(sa, P, oracle_mt, opts, nu1, nu2, out_n, kw, n):
    O = oracle_mt
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    assert s.num_per == 8 and s.dim0 == 1 << nu1 and s.trials == out_n * out_n
    db = O.pack_gen_db(po, out_n, 41)
    servers, clients = lanes_of(sa, O, po, pg, out_n, n, 41)
    idx = indices(s, n)
    qs = [cl.query(i) for cl, i in zip(clients, idx)]
    bytes0 = servers[0].db_device_bytes()
    singles = [single_state(srv, q, s.trials) for srv, q in zip(servers, qs)]
    assert servers[0].db_format() == P.DB_PACKED
    opts(pack_pair_blocks=1)
    assert P.has_limb_form(pg, out_n)
    got = batch_states(P, servers, qs, s.trials)
    assert servers[0].db_format() == P.DB_LIMBS and servers[n - 1].db_format() == P.DB_LIMBS
    assert servers[0].db_device_bytes() == bytes0  # converted in place: no second image
    for b in range(n):
        assert_state_eq(got[b], singles[b], f"lane {b}: the shared pass vs its own answer on the packed image")
        exp_resp, exp_packed = O.pack_answer(po, out_n, qs[b], *clients[b].pp, db)
        assert_eq(got[b][1], exp_packed, f"lane {b}: packed ciphertext vs the oracle")
        assert_eq(got[b][0], exp_resp, f"lane {b}: response vs the oracle")
        assert_eq(clients[b].decode(got[b][0]), O.pack_db_item(po, out_n, 41, idx[b]), f"lane {b}: decoded items")
    close_all(servers)


def test_pair_single_answers_and_round_trip(sa, P, oracle, opts):
    """single answers on the converted image (the one-query pair form, NT = 1) equal the packed image's, accumulators of all 9 trials included; back to
    PACKED -- through both conversion kernels -- they are there again"""
    O = oracle
    nu1, nu2, out_n = 7, 3, 3
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    servers, clients = lanes_of(sa, O, po, pg, out_n, 2, 5)
    owner = servers[0]
    qs = [cl.query(i) for cl, i in zip(clients, indices(s, 2, 3))]
    bytes0 = owner.db_device_bytes()
    singles = [single_state(srv, q, s.trials) for srv, q in zip(servers, qs)]
    opts(pack_pair_blocks=1)
    owner.set_db_format(P.DB_LIMBS)
    assert owner.db_format() == P.DB_LIMBS and owner.db_device_bytes() == bytes0
    for b in range(2):
        assert_state_eq(single_state(servers[b], qs[b], s.trials), singles[b], f"lane {b}: single answer on the limb-plane image")
    owner.set_db_format(P.DB_PACKED)
    assert owner.db_format() == P.DB_PACKED and owner.db_device_bytes() == bytes0
    for b in range(2):
        assert_state_eq(single_state(servers[b], qs[b], s.trials), singles[b], f"lane {b}: single answer after packed -> limbs -> packed")
    close_all(servers)


def test_pair_option_semantics(sa, P, oracle, opts):
    """option 0: today's behaviour (the batch leaves the image PACKED, LIMBS is refused).  Option 1: convert; option back to 0: the converted image is
    still swept by batches, bit-identically, and converts back"""
    O = oracle
    nu1, nu2, out_n = 7, 3, 2
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    servers, clients = lanes_of(sa, O, po, pg, out_n, 2, 9)
    owner = servers[0]
    qs = [cl.query(i) for cl, i in zip(clients, indices(s, 2, 5))]
    opts(pack_pair_blocks=0)
    assert not P.has_limb_form(pg, out_n)
    packed = batch_states(P, servers, qs, s.trials)
    assert owner.db_format() == P.DB_PACKED
    with pytest.raises(sa.SpiralGpuError, match="limb-plane"):
        owner.set_db_format(P.DB_LIMBS)
    assert owner.db_format() == P.DB_PACKED
    sa.set_option("pack_pair_blocks", 1)
    owner.set_db_format(P.DB_LIMBS)
    sa.set_option("pack_pair_blocks", 0)
    assert owner.db_format() == P.DB_LIMBS and not P.has_limb_form(pg, out_n)
    limbs = batch_states(P, servers, qs, s.trials)
    assert owner.db_format() == P.DB_LIMBS
    for b in range(2):
        assert_state_eq(limbs[b], packed[b], f"lane {b}: batch on the limb-plane image with the option back at 0")
    owner.set_db_format(P.DB_PACKED)  # never stranded
    assert owner.db_format() == P.DB_PACKED
    again = batch_states(P, servers, qs, s.trials)
    assert owner.db_format() == P.DB_PACKED
    for b in range(2):
        assert_state_eq(again[b], packed[b], f"lane {b}: batch after converting back")
    close_all(servers)


def test_pair_update_in_limb_form(sa, P, oracle, opts):
    """update_db_items on a limb-plane image of 8 columns, in trial 0 and trial 8 (the lone trial of the last pair-block): a partner pair (j, j ^ 64) of
    one column, a lone low partner, a lone high partner, the first and the last item and one more column.  Batch answers then equal those of a fresh
    server that got the same items through load_db_items; a refused update (an id outside the database) changes nothing"""
    O = oracle
    nu1, nu2, out_n = 7, 3, 3
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    np_, total = s.num_per, s.dim0 * s.num_per
    assert s.trials == 9 and np_ == 8
    opts(pack_pair_blocks=1)
    servers, clients = lanes_of(sa, O, po, pg, out_n, 3, 41)
    owner = servers[0]
    owner.set_db_format(P.DB_LIMBS)
    ids = sorted({5 * np_ + 3, (5 ^ 64) * np_ + 3, 33 * np_ + 7, 70 * np_ + 1, 0, total - 1, 9 * np_ + 5})
    new = {}
    for trial, seed in ((0, 61), (8, 62)):
        pts = np.stack([O.pack_db_item(po, out_n, seed, i).reshape(s.trials, N)[trial] for i in ids])
        owner.update_db_items(trial, O.pack_items(pts, 8), 8, ids)
        new[trial] = pts
    assert owner.db_format() == P.DB_LIMBS
    fresh, _ = lanes_of(sa, O, po, pg, out_n, 3, 41, clients=clients)
    for trial, pts in new.items():
        for k, i in enumerate(ids):
            fresh[0].load_db_items(trial, O.pack_items(pts[k:k + 1], 8), 8, first_item=i, n_items=1)
    idx = [5 * np_ + 3, (5 ^ 64) * np_ + 3, 70 * np_ + 1]
    qs = [cl.query(i) for cl, i in zip(clients, idx)]
    got = batch_states(P, servers, qs, s.trials)
    want = batch_states(P, fresh, qs, s.trials)
    assert owner.db_format() == P.DB_LIMBS
    for b in range(3):
        assert_state_eq(got[b], want[b], f"lane {b}: the updated limb-plane image vs a fresh server with the same items")
        dec = clients[b].decode(got[b][0]).reshape(s.trials, N)
        k = ids.index(idx[b])
        assert_eq(dec[0], new[0][k], f"lane {b}: the updated item of trial 0 decodes")
        assert_eq(dec[8], new[8][k], f"lane {b}: the updated item of trial 8 decodes")
        assert_eq(dec[4], O.pack_db_item(po, out_n, 41, idx[b]).reshape(s.trials, N)[4], f"lane {b}: trial 4 kept its item")
    # the unchanged partners of the lone items kept their values (their nibbles share a byte with the updated ones)
    q2 = [clients[0].query((33 ^ 64) * np_ + 7), clients[1].query((70 ^ 64) * np_ + 1), clients[2].query(6 * np_ + 3)]
    got2, want2 = batch_states(P, servers, q2, s.trials), batch_states(P, fresh, q2, s.trials)
    for b in range(3):
        assert_state_eq(got2[b], want2[b], f"lane {b}: an untouched partner")
    with pytest.raises(sa.SpiralGpuError):
        owner.update_db_items(0, O.pack_items(new[8][:2], 8), 8, [3, total])
    after = batch_states(P, servers, qs, s.trials)
    for b in range(3):
        assert_state_eq(after[b], got[b], f"lane {b}: after a refused update")
    close_all(servers, fresh)


def test_pair_sharded_trials(sa, P, oracle, opts):
    """a server for trials [0, 5) of 9 (3 pair-blocks, the last half empty): fold_trials on its packed and on its limb-plane image leave the same
    accumulators and folded ciphertexts"""
    import torch

    O = oracle
    nu1, nu2, out_n = 7, 3, 3
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    cl = O.PackClient(po, out_n, seed=31)
    sh = sa.PackServer(pg, out_n, trial0=0, trial1=5)
    sh.gen_db(17)
    sh.set_pub_params(*cl.pub_params())
    q = cl.query(777 % (s.dim0 * s.num_per))
    opts(pack_pair_blocks=1)
    folded = torch.zeros(2, 5 * 2 * N, dtype=torch.int64, device="cuda")
    got = []
    for step in range(2):
        if step:
            sh.set_db_format(P.DB_LIMBS)
        assert sh.db_format() == (P.DB_LIMBS if step else P.DB_PACKED)
        sh.fold_trials(q, folded[step].data_ptr())
        torch.cuda.synchronize()
        got.append([sh.read_acc(t) for t in range(5)])
    for t in range(5):
        assert_eq(got[1][t], got[0][t], f"trial {t}: the shard's limb-plane image vs its packed image")
    assert torch.equal(folded[0], folded[1]) and int(folded[0].ne(0).sum()) > 0, "folded ciphertexts of the two forms"
    sh.close()


def test_pair_items(sa, P, oracle, opts):
    """answer_batch_instances, 2 clients x 2 instances: slot [q, k] is client q's own answer against instance k taken on the packed images, and both
    instances end in limb planes"""
    O = oracle
    nu1, nu2, out_n, B, F = 7, 3, 2, 2, 2
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    seeds = [300, 311]
    instances = []
    for k in range(F):
        inst = sa.PackServer(pg, out_n)
        inst.gen_db(seeds[k])
        instances.append(inst)
    owner = instances[0]
    servers = [owner, owner.create_lane()]
    clients, queries, idx = [], [], indices(s, B, 9)
    for q, srv in enumerate(servers):
        cl = O.PackClient(po, out_n, seed=50 + 13 * q)
        srv.set_pub_params(*cl.pub_params())
        clients.append(cl)
        queries.append(cl.query(idx[q]))
    ones = [P.answer_instances(servers[q], instances, queries[q], wire=True) for q in range(B)]
    assert [i.db_format() for i in instances] == [P.DB_PACKED] * F
    opts(pack_pair_blocks=1)
    resp, wire = P.answer_batch_instances(servers, instances, queries, wire=True)
    assert [i.db_format() for i in instances] == [P.DB_LIMBS] * F
    for q in range(B):
        assert_eq(resp[q], ones[q][0], f"client {q}: batch vs its own item call on the packed images")
        assert_eq(wire[q], ones[q][1], f"client {q}: wire forms")
        for k in range(F):
            assert_eq(clients[q].decode(resp[q, k]), O.pack_db_item(po, out_n, seeds[k], idx[q]), f"client {q}, instance {k}: decoded")
    close_all(servers[1:], instances)


def test_pair_lane_form(sa, P, oracle, opts):
    """the lane form (pack_batch_lanes = 2) on top of the pair form, 3 clients on 9 trials: bit-identical to the per-lane form, counted once"""
    O = oracle
    nu1, nu2, out_n, n = 7, 3, 3, 3
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    servers, clients = lanes_of(sa, O, po, pg, out_n, n, 23)
    qs = [cl.query(i) for cl, i in zip(clients, indices(s, n, 2))]
    opts(pack_pair_blocks=1, pack_batch_lanes=0)
    counted = sa.get_option("pack_lane_batches")
    per_lane = batch_states(P, servers, qs, s.trials)
    assert servers[0].db_format() == P.DB_LIMBS and sa.get_option("pack_lane_batches") == counted
    sa.set_option("pack_batch_lanes", 2)
    lane_form = batch_states(P, servers, qs, s.trials)
    assert sa.get_option("pack_lane_batches") == counted + 1
    for b in range(n):
        assert_state_eq(lane_form[b], per_lane[b], f"lane {b}: lane form vs per-lane form")
    close_all(servers)


def test_pair_time_sweep_batch(sa, P, oracle, opts):
    O = oracle
    nu1, nu2, out_n = 7, 3, 2
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    servers, clients = lanes_of(sa, O, po, pg, out_n, 2, 3)
    for srv, cl, i in zip(servers, clients, indices(s, 2)):
        srv.answer(cl.query(i))
    opts(pack_pair_blocks=1)
    assert P.time_sweep_batch(servers, 2) > 0
    assert servers[0].db_format() == P.DB_LIMBS
    close_all(servers)
