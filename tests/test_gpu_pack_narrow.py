"""The SpiralPack batch's shared matrix-core pass on NARROW trial geometries (csrc/sweep_mfma.hip, the NARROW form of sweep_mfma_kernel<NT, 2>):
16, 32 or 64 ciphertexts per slot, where the eight waves of a workgroup take 16-column blocks of different trials.  Every comparison is bit for bit
against the CPU oracle (pack_answer, pack_db_item) on the client's own keys, and against the vector-ALU sweep of the packed image."""
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


def lanes_of(sa, O, po, pg, out_n, n, db_seed, client_seed=100):
    """an owner with the device-generated database and n - 1 lanes, each with its own client's public parameters (kept in clients[b].pp)"""
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


def word(enc):
    """an oracle encoding's two residue limbs -> device words (p-residue | b-residue << 32)"""
    return enc[..., 0, :] | (enc[..., 1, :] << np.uint64(32))


def pack_word(O, po, pt):
    """a 1 x 1 plaintext's database words (the centred lift and transform are the base item's: the oracle's base encoder on a 2 x 2 item)"""
    return word(O.encode_item(po, np.stack([pt] * 4).reshape(2, 2, N)))[0, 0]


def put_item(want_db, s, trial, i, w):
    want_db[trial].reshape(N, s.num_per, s.dim0)[:, i % s.num_per, i // s.num_per] = w


DIRECT = dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1)
NARROW = [
    # nu1, nu2, out_n, params, clients                   num_per x trials, blocks of 16 columns
    (7, 4, 2, {}, 8),                                  # 16 x 4, 4: a half-empty single group
    (7, 4, 3, {}, 3),                                  # 16 x 9, 9: one full group and a ragged one
    (7, 5, 2, dict(t_gsw=4), 4),                       # 32 x 4, 8: two blocks per trial, packed tiles of 2 slots
    (7, 6, 1, {}, 2),                                  # 64 x 1, 4: four blocks of one trial, packed tiles of 1 slot
    (8, 4, 2, {}, 5),                                  # 16 x 4, first dimension 256: two pieces per prime
    (7, 4, 2, DIRECT, 2),                              # direct upload
]


@pytest.mark.parametrize("nu1,nu2,out_n,kw,n", NARROW, ids=[f"{g[0]}-{g[1]}-{g[2]}{'-direct' if g[3].get('direct_upload') else ''}" for g in NARROW])
def test_narrow_batch_matches_oracle(sa, P, oracle_mt, nu1, nu2, out_n, kw, n):
    O = oracle_mt
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    assert s.num_per < 128 and P.has_limb_form(pg, out_n)
    db = O.pack_gen_db(po, out_n, 41)
    servers, clients = lanes_of(sa, O, po, pg, out_n, n, 41)
    idx = indices(s, n)
    qs = [cl.query(i) for cl, i in zip(clients, idx)]
    out, us = P.answer_batch(servers, qs, want_packed=True)
    assert us["n"] == n and us["total_us"] > 0
    for b in range(n):
        exp_resp, exp_packed = O.pack_answer(po, out_n, qs[b], *clients[b].pp, db)
        assert_eq(out[b][1], exp_packed, f"lane {b}: packed ciphertext")
        assert_eq(out[b][0], exp_resp, f"lane {b}: response")
        assert_eq(clients[b].decode(out[b][0]), O.pack_db_item(po, out_n, 41, idx[b]), f"lane {b}: decoded items")
    assert servers[0].db_format() == P.DB_LIMBS
    for srv in servers:
        srv.close()


def _singles(srv, q, trials):
    resp, packed, _ = srv.answer(q)
    return resp, packed, srv.read_response_wire(), [srv.read_acc(t) for t in range(trials)]


def test_narrow_batch_equals_singles(sa, P, oracle):
    """singles on the packed image, then the batch (which converts in place), then singles on the limb-plane image (the one-query narrow form):
    responses, wire forms, packed ciphertexts and the accumulators of all 9 trials of every lane agree bit for bit"""
    O = oracle
    nu1, nu2, out_n, n = 7, 4, 3, 4
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    assert s.trials == 9 and s.num_per == 16
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
    for b in range(n):
        again = _singles(servers[b], qs[b], s.trials)
        assert_eq(again[0], single[b][0], f"lane {b}: single answer on the limb-plane image")
        assert_eq(again[1], single[b][1], f"lane {b}: packed ciphertext on the limb-plane image")
        assert_eq(again[2], single[b][2], f"lane {b}: wire form on the limb-plane image")
        for t in range(s.trials):
            assert_eq(again[3][t], single[b][3][t], f"lane {b}, trial {t}: accumulators on the limb-plane image")
    assert P.time_sweep_batch(servers, 2) > 0
    for srv in servers:
        srv.close()


@pytest.mark.parametrize("nu1,nu2,out_n,kw", [(7, 4, 2, {}), (7, 5, 2, dict(t_gsw=4)), (7, 6, 1, {})], ids=["7-4-2", "7-5-2", "7-6-1"])
def test_narrow_image_round_trip(sa, P, oracle_mt, nu1, nu2, out_n, kw):
    """packed -> limbs -> packed: one client's answer (response, packed ciphertext, every trial's accumulators) is the oracle's in all three states;
    a partial load_db_items on the limb-plane image leaves a correct packed image"""
    O = oracle_mt
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    total = s.dim0 * s.num_per
    db = O.pack_gen_db(po, out_n, 21)
    servers, clients = lanes_of(sa, O, po, pg, out_n, 2, 21)
    owner, lane = servers
    q = clients[0].query(indices(s, 2, 11)[1])
    exp_resp, exp_packed = O.pack_answer(po, out_n, q, *clients[0].pp, db)
    bytes0 = owner.db_device_bytes()
    states = []
    for step, fmt in enumerate((None, P.DB_LIMBS, P.DB_PACKED)):
        if fmt is not None:
            owner.set_db_format(fmt)
            if fmt == P.DB_LIMBS:
                with pytest.raises(sa.SpiralGpuError, match="lane"):
                    lane.set_db_format(P.DB_PACKED)
        assert owner.db_format() == (P.DB_LIMBS if step == 1 else P.DB_PACKED) and owner.db_device_bytes() == bytes0
        resp, packed, _ = owner.answer(q)
        states.append((resp, packed, [owner.read_acc(t) for t in range(s.trials)]))
    for step, (resp, packed, accs) in enumerate(states):
        assert_eq(resp, exp_resp, f"state {step}: response vs the oracle")
        assert_eq(packed, exp_packed, f"state {step}: packed ciphertext vs the oracle")
        for t in range(s.trials):
            assert_eq(accs[t], states[0][2][t], f"state {step}, trial {t}: accumulators")
    # a run of items of one trial reloaded over the limb-plane image: the image goes back to the packed form, the other words keep their values
    owner.set_db_format(P.DB_LIMBS)
    trial = s.trials - 1
    first, count = 3 * s.num_per + 5, 40
    pts = [O.pack_db_item(po, out_n, 78, i).reshape(s.trials, N)[trial] for i in range(first, first + count)]
    owner.load_db_items(trial, O.pack_items(np.stack(pts), 8), 8, first_item=first, n_items=count)
    assert owner.db_format() == P.DB_PACKED and owner.db_device_bytes() == bytes0
    for i, pt in zip(range(first, first + count), pts):
        put_item(db, s, trial, i, pack_word(O, po, pt))
    q2 = clients[0].query(first + 1)
    got = owner.answer(q2)
    want = O.pack_answer(po, out_n, q2, *clients[0].pp, db)
    assert_eq(got[0], want[0], "after load_db_items on the limb-plane image: response")
    assert_eq(got[1], want[1], "after load_db_items on the limb-plane image: packed ciphertext")
    assert_eq(clients[0].decode(got[0]).reshape(s.trials, N)[trial], pts[1], "the reloaded item decodes")
    assert total > first + count
    for srv in servers:
        srv.close()


def test_narrow_update_in_limb_form(sa, P, oracle_mt):
    """update_db_items on a limb-plane image of 16 columns: a partner pair (j, j ^ 64 of one column), a lone partner, the first and the last item,
    in the first and the last trial; a batch and a single answer then return the oracle's answer for the updated database"""
    O = oracle_mt
    nu1, nu2, out_n = 7, 4, 2
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    np_, total = s.num_per, s.dim0 * s.num_per
    db = O.pack_gen_db(po, out_n, 41)
    servers, clients = lanes_of(sa, O, po, pg, out_n, 3, 41)
    owner = servers[0]
    owner.set_db_format(P.DB_LIMBS)
    ids = sorted({0, total - 1, 5 * np_ + 3, (5 ^ 64) * np_ + 3, 70 * np_ + 9, 33 * np_ + 15})
    for trial, seed in ((0, 61), (s.trials - 1, 62)):
        pts = [O.pack_db_item(po, out_n, seed, i).reshape(s.trials, N)[trial] for i in ids]
        owner.update_db_items(trial, O.pack_items(np.stack(pts), 8), 8, ids)
        for i, pt in zip(ids, pts):
            put_item(db, s, trial, i, pack_word(O, po, pt))
    assert owner.db_format() == P.DB_LIMBS
    idx = [5 * np_ + 3, (5 ^ 64) * np_ + 3, 70 * np_ + 9]
    qs = [cl.query(i) for cl, i in zip(clients, idx)]
    out, _ = P.answer_batch(servers, qs, want_packed=True)
    for b in range(3):
        exp_resp, exp_packed = O.pack_answer(po, out_n, qs[b], *clients[b].pp, db)
        assert_eq(out[b][1], exp_packed, f"lane {b}: packed ciphertext after the update")
        assert_eq(out[b][0], exp_resp, f"lane {b}: response after the update")
    dec = clients[0].decode(out[0][0]).reshape(s.trials, N)
    assert_eq(dec[s.trials - 1], O.pack_db_item(po, out_n, 62, idx[0]).reshape(s.trials, N)[s.trials - 1], "the updated item of the last trial decodes")
    q = clients[1].query(6 * np_ + 9)  # the unchanged partner of the lone item
    resp, packed, _ = servers[1].answer(q)
    want = O.pack_answer(po, out_n, q, *clients[1].pp, db)
    assert_eq(resp, want[0], "single answer after the update: response")
    assert_eq(packed, want[1], "single answer after the update: packed ciphertext")
    assert_eq(clients[1].decode(resp), O.pack_db_item(po, out_n, 41, 6 * np_ + 9), "the lone item's partner kept its value")
    assert owner.db_format() == P.DB_LIMBS
    for srv in servers:
        srv.close()


def test_narrow_items(sa, P, oracle, request):
    """answer_batch_instances, 3 clients x 3 instances, one instance in limb planes and two packed going in: slot [q, k] is client q's own item call,
    every instance ends in limb planes, and the group size does not show"""
    O = oracle
    nu1, nu2, out_n, B, F = 7, 4, 2, 3, 3
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    L = sa.lib()
    request.addfinalizer(lambda: L.spiral_gpu_set_option(b"pack_item_group", 0))
    seeds = [300 + 11 * k for k in range(F)]
    outs = {}
    for g in (1, 0):
        instances = []
        for k in range(F):
            inst = sa.PackServer(pg, out_n)
            inst.gen_db(seeds[k])
            instances.append(inst)
        owner = instances[0]
        servers = [owner] + [owner.create_lane() for _ in range(B - 1)]
        clients, queries, idx = [], [], indices(s, B, 9)
        for q, srv in enumerate(servers):
            cl = O.PackClient(po, out_n, seed=50 + 13 * q)
            cl.pp = cl.pub_params()
            srv.set_pub_params(*cl.pp)
            clients.append(cl)
            queries.append(cl.query(idx[q]))
        instances[1].set_db_format(P.DB_LIMBS)
        assert [i.db_format() for i in instances] == [P.DB_PACKED, P.DB_LIMBS, P.DB_PACKED]
        assert L.spiral_gpu_set_option(b"pack_item_group", g) == 0
        resp, wire = P.answer_batch_instances(servers, instances, queries, wire=True)
        assert resp.shape[:2] == (B, F) and wire.shape[:2] == (B, F)
        assert [i.db_format() for i in instances] == [P.DB_LIMBS] * F
        for q in range(B):
            one, w1 = P.answer_instances(servers[q], instances, queries[q], wire=True)
            assert_eq(resp[q], one, f"group {g}, client {q}: batch vs its own item call")
            assert_eq(wire[q], w1, f"group {g}, client {q}: wire forms")
            for k in range(F):
                assert_eq(clients[q].decode(resp[q, k]), O.pack_db_item(po, out_n, seeds[k], idx[q]), f"group {g}, client {q}, instance {k}: decoded")
        outs[g] = (resp, wire)
        for srv in servers[1:] + instances:
            srv.close()
    assert_eq(outs[0][0], outs[1][0], "pack_item_group 0 vs 1: responses")
    assert_eq(outs[0][1], outs[1][1], "pack_item_group 0 vs 1: wire forms")


def test_narrow_sharded_trials(sa, P, oracle):
    """a server for trials [4, 9) of 9 (5 blocks: one ragged group whose first trial is not trial 0): fold_trials on its packed image and on its
    limb-plane image leave the same accumulators, the unsharded server's for those trials"""
    import torch

    O = oracle
    nu1, nu2, out_n = 7, 4, 3
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    cl = O.PackClient(po, out_n, seed=31)
    pp = cl.pub_params()
    full = sa.PackServer(pg, out_n)
    full.gen_db(17)
    full.set_pub_params(*pp)
    q = cl.query(1234 % (s.dim0 * s.num_per))
    full.answer(q)
    want = {t: full.read_acc(t) for t in range(4, 9)}
    sh = sa.PackServer(pg, out_n, trial0=4, trial1=9)
    sh.gen_db(17)
    sh.set_pub_params(*pp)
    folded = torch.zeros(2, 5 * 2 * N, dtype=torch.int64, device="cuda")
    got = []
    for step in range(2):
        if step:
            sh.set_db_format(P.DB_LIMBS)
        assert sh.db_format() == (P.DB_LIMBS if step else P.DB_PACKED)
        sh.fold_trials(q, folded[step].data_ptr())
        torch.cuda.synchronize()
        got.append({t: sh.read_acc(t) for t in range(4, 9)})
    for t in range(4, 9):
        assert_eq(got[0][t], want[t], f"trial {t}: the shard's packed image vs the unsharded server")
        assert_eq(got[1][t], got[0][t], f"trial {t}: the shard's limb-plane image vs its packed image")
    assert torch.equal(folded[0], folded[1]) and int(folded[0].ne(0).sum()) > 0, "folded ciphertexts of the two forms"
    with pytest.raises(sa.SpiralGpuError, match="trial-sharded"):
        sh.create_lane()
    sh.close()
    full.close()


@pytest.mark.parametrize("nu1,nu2,out_n", [(7, 3, 2), (6, 4, 2)], ids=["7-3-2", "6-4-2"])
def test_uncovered_stays_uncovered(sa, P, oracle_mt, nu1, nu2, out_n):
    """8 ciphertexts per slot, or a 64-term first dimension: no limb-plane form, the batch sweeps once per lane on the packed image"""
    O = oracle_mt
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    assert not P.has_limb_form(pg, out_n)
    db = O.pack_gen_db(po, out_n, 41)
    servers, clients = lanes_of(sa, O, po, pg, out_n, 2, 41)
    idx = indices(s, 2)
    qs = [cl.query(i) for cl, i in zip(clients, idx)]
    out, _ = P.answer_batch(servers, qs, want_packed=True)
    for b in range(2):
        exp_resp, exp_packed = O.pack_answer(po, out_n, qs[b], *clients[b].pp, db)
        assert_eq(out[b][1], exp_packed, f"lane {b}: packed ciphertext")
        assert_eq(out[b][0], exp_resp, f"lane {b}: response")
        assert_eq(clients[b].decode(out[b][0]), O.pack_db_item(po, out_n, 41, idx[b]), f"lane {b}: decoded items")
    assert servers[0].db_format() == P.DB_PACKED
    with pytest.raises(sa.SpiralGpuError, match="limb-plane"):
        servers[0].set_db_format(P.DB_LIMBS)
    assert servers[0].db_format() == P.DB_PACKED
    for srv in servers:
        srv.close()
