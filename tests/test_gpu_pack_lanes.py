"""The lane form of SpiralPack batch calls (include/spiral_gpu.h, option "pack_batch_lanes"): from that many clients on, answer_batch runs as ONE
launch sequence whose every launch carries all clients in gridDim.z -- one expansion and conversion, the shared first-dimension pass, one folding,
one packing and switch -- instead of one client after another around the shared pass.  Both forms must leave every lane's response, packed
ciphertext, wire form and accumulators of every trial exactly as its own answer does; the counter "pack_lane_batches" shows which form ran."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2048

# (nu1, nu2, out_n, params)
G_SMALL = (7, 7, 1, {})                                                       # the smallest covered geometry, with expansion
G_WIDE = (7, 8, 1, dict(t_gsw=4))                                             # num_per = 256: fold round 0 has 128 pairs (pack_fold_mac_kernel<4>), later rounds <1>
G_DIRECT = (7, 7, 2, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1))  # direct upload: pack_gsw_from_upload, qs1 from the query, four trials, out_n = 2
G_UNCOVERED = (6, 2, 2, {})                                                   # one sweep1_kernel per lane between the lane-aware pieces, two narrow fold rounds
G_N12 = (3, 2, 12, dict(t_gsw=3, t_conv=56, t_exp=56, qprime_bits=31, p_db=524288, direct_upload=1))  # pack_mac reduces before 256 terms; 144 trials


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


class Setup:
    def __init__(self, sa, O, geom, n, db_seed=41, salt=0):
        nu1, nu2, self.out_n, kw = geom
        self.O, self.n, self.db_seed = O, n, db_seed
        self.po, self.pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
        self.s = O.pack_shape_of(self.po, self.out_n)
        self.servers, self.clients = lanes_of(sa, O, self.po, self.pg, self.out_n, n, db_seed)
        self.idx = indices(self.s, n, salt)
        self.qs = [cl.query(i) for cl, i in zip(self.clients, self.idx)]

    def close(self):
        for srv in self.servers:
            srv.close()


def state_of(srv, out, trials):
    """everything a batch leaves for one lane: (response, packed ciphertext, wire form, accumulators of every trial)"""
    return out[0], out[1], srv.read_response_wire(), [srv.read_acc(t) for t in range(trials)]


def assert_state_eq(got, exp, what):
    for k, name in enumerate(("response", "packed ciphertext", "wire form")):
        assert_eq(got[k], exp[k], f"{what}: {name}")
    assert len(got[3]) == len(exp[3])
    for t, (a, e) in enumerate(zip(got[3], exp[3])):
        assert_eq(a, e, f"{what}: accumulators of trial {t}")


def single_of(srv, q, trials):
    resp, packed, _ = srv.answer(q)
    return state_of(srv, (resp, packed), trials)


def batch_with(sa, P, lanes_value, servers, qs, trials, expect_counted):
    """one answer_batch under pack_batch_lanes = lanes_value (restored afterwards): every lane's state and the stage times; the counter must move by
    expect_counted"""
    before = sa.get_option("pack_batch_lanes")
    try:
        sa.set_option("pack_batch_lanes", lanes_value)
        counted = sa.get_option("pack_lane_batches")
        out, us = P.answer_batch(servers, qs, want_packed=True)
        assert sa.get_option("pack_lane_batches") - counted == expect_counted, f"pack_batch_lanes = {lanes_value}, {len(servers)} clients"
    finally:
        sa.set_option("pack_batch_lanes", before)
    return [state_of(srv, o, trials) for srv, o in zip(servers, out)], us


def both_forms(sa, P, st, lanes_value=2):
    """the batch per lane (pack_batch_lanes = 0), then in lane form, on the same servers: equal bit for bit; returns the lane form's states"""
    per_lane, _ = batch_with(sa, P, 0, st.servers, st.qs, st.s.trials, 0)
    lane_form, _ = batch_with(sa, P, lanes_value, st.servers, st.qs, st.s.trials, 1)
    for b in range(st.n):
        assert_state_eq(lane_form[b], per_lane[b], f"lane {b}, lane form vs per-lane form")
    return lane_form


def assert_oracle(st, states):
    O, db = st.O, st.O.pack_gen_db(st.po, st.out_n, st.db_seed)
    for b in range(st.n):
        exp_resp, exp_packed = O.pack_answer(st.po, st.out_n, st.qs[b], *st.clients[b].pp, db)
        assert_eq(states[b][1], exp_packed, f"lane {b}: packed ciphertext vs the oracle")
        assert_eq(states[b][0], exp_resp, f"lane {b}: response vs the oracle")
        assert_eq(st.clients[b].decode(states[b][0]), O.pack_db_item(st.po, st.out_n, st.db_seed, st.idx[b]), f"lane {b}: decoded items")


@pytest.mark.parametrize("geom,n,with_oracle", [(G_SMALL, 8, True), (G_WIDE, 3, True), (G_DIRECT, 2, False), (G_UNCOVERED, 3, False), (G_N12, 2, True)],
                         ids=["small-B8", "wide-B3", "direct-B2", "uncovered-B3", "n12-B2"])
def test_lane_form_equals_per_lane_form(sa, P, oracle_mt, geom, n, with_oracle):
    st = Setup(sa, oracle_mt, geom, n)
    try:
        states = both_forms(sa, P, st)
        if with_oracle:
            assert_oracle(st, states)
    finally:
        st.close()


def test_any_server_first(sa, P, oracle):
    """[lane 2, owner, lane 1]: negative and mixed arena offsets and a lane as servers[0]; then the same queries owner first: each client's words
    are the same in both orders"""
    st = Setup(sa, oracle, G_SMALL, 3, salt=9)
    try:
        order = [2, 0, 1]
        mixed = Setup.__new__(Setup)
        mixed.__dict__.update(st.__dict__)
        mixed.servers, mixed.qs = [st.servers[i] for i in order], [st.qs[i] for i in order]
        got = both_forms(sa, P, mixed)
        owner_first, _ = batch_with(sa, P, 2, st.servers, st.qs, st.s.trials, 1)
        for pos, i in enumerate(order):
            assert_state_eq(got[pos], owner_first[i], f"client {i}: [lane 2, owner, lane 1] vs owner first")
    finally:
        st.close()


@pytest.mark.parametrize("fold_pair", [0, 1])
@pytest.mark.parametrize("fwd2", [0, 1])
def test_fold_forms_under_lanes(sa, P, oracle, fold_pair, fwd2):
    """the two-product fold (fold_chain with pack = 1) and the two-digit transform kernel with lanes"""
    before = {k: sa.get_option(k) for k in ("fold_pair", "fwd2")}
    st = None
    try:
        sa.set_option("fold_pair", fold_pair)
        sa.set_option("fwd2", fwd2)
        st = Setup(sa, oracle, G_WIDE, 2, salt=4)
        both_forms(sa, P, st)
    finally:
        for k, v in before.items():
            sa.set_option(k, v)
        if st:
            st.close()


@pytest.mark.parametrize("lanes_value", [3, 0, 1])
def test_threshold(sa, P, oracle, lanes_value):
    """a batch of two under pack_batch_lanes = 3 and = 0 runs per lane (the counter stays); under = 1 it runs in lane form, and a batch of ONE client
    is a single answer (the counter stays)"""
    st = Setup(sa, oracle, G_SMALL, 2, salt=2)
    try:
        singles = [single_of(srv, q, st.s.trials) for srv, q in zip(st.servers, st.qs)]
        got, _ = batch_with(sa, P, lanes_value, st.servers, st.qs, st.s.trials, 1 if lanes_value == 1 else 0)
        for b in range(2):
            assert_state_eq(got[b], singles[b], f"pack_batch_lanes = {lanes_value}, lane {b}: batch of two vs its single answer")
        one, _ = batch_with(sa, P, lanes_value, st.servers[1:], st.qs[1:], st.s.trials, 0)
        assert_state_eq(one[0], singles[1], f"pack_batch_lanes = {lanes_value}: a batch of one vs the single answer")
    finally:
        st.close()


def test_servers_stay_usable_alone(sa, P, oracle):
    """a lane-form batch, a single answer on lane 2 with a new query, a second batch: every result equals its single answer's (flags, events and
    stage times of each server are its own again)"""
    st = Setup(sa, oracle, G_SMALL, 4, salt=6)
    try:
        trials = st.s.trials
        singles = [single_of(srv, q, trials) for srv, q in zip(st.servers, st.qs)]
        q2 = st.clients[2].query((st.idx[2] + 12345) % (st.s.dim0 * st.s.num_per))
        single2 = single_of(st.servers[2], q2, trials)
        first, _ = batch_with(sa, P, 2, st.servers, st.qs, trials, 1)
        for b in range(4):
            assert_state_eq(first[b], singles[b], f"first batch, lane {b} vs its single answer")
        alone = single_of(st.servers[2], q2, trials)
        assert_state_eq(alone, single2, "lane 2 alone after a lane-form batch")
        us = st.servers[2].stage_us()
        assert us["total_us"] > 0 and all(v >= 0 for v in us.values())
        qs = st.qs[:2] + [q2] + st.qs[3:]
        second, _ = batch_with(sa, P, 2, st.servers, qs, trials, 1)
        for b in range(4):
            assert_state_eq(second[b], single2 if b == 2 else singles[b], f"second batch, lane {b} vs its single answer")
        assert st.servers[0].stage_us()["total_us"] > 0  # (servers[0]'s events are those of the batch)
    finally:
        st.close()


def test_stage_times_of_a_lane_form_batch(sa, P, oracle):
    st = Setup(sa, oracle, G_SMALL, 4, salt=1)
    try:
        _, us = batch_with(sa, P, 2, st.servers, st.qs, st.s.trials, 1)
        assert us["n"] == 4 and us["total_us"] > 0
        assert all(v >= 0 for v in us.values()), us
        assert us["first_dim_us"] == us["sweep_kernels_us"]  # (include/spiral_gpu.h: [2] = [5] the shared sweep)
        # the stages were timed on servers[0]'s events alone: its stage_us describes the batch, another lane's says so instead of old times
        assert st.servers[0].stage_us()["total_us"] == us["total_us"]
        with pytest.raises(sa.SpiralGpuError, match="servers\\[0\\]"):
            st.servers[1].stage_us()
        st.servers[1].answer(st.qs[1])
        assert st.servers[1].stage_us()["total_us"] > 0  # (its own events again)
    finally:
        st.close()


@pytest.mark.parametrize("group", [0, 1])
def test_items_convert_in_lane_form(sa, P, oracle, group):
    """answer_batch_instances, B = 3 clients, F = 2 instances: the clients' expansion and conversion as one lane-aware sequence (the counter moves by
    one per call); results equal the per-lane form's, and slot [q, k] equals client q's single answer on instance k"""
    O = oracle
    nu1, nu2, out_n, kw = G_SMALL
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    B, F = 3, 2
    instances, probes, servers = [], [], []
    before = {k: sa.get_option(k) for k in ("pack_item_group", "pack_batch_lanes")}
    try:
        for k in range(F):
            inst = sa.PackServer(pg, out_n)
            inst.gen_db(300 + 11 * k)
            instances.append(inst)
            probes.append(inst.create_lane())
        servers = [instances[0]] + [instances[0].create_lane() for _ in range(B - 1)]
        clients, qs = [], []
        for q, srv in enumerate(servers):
            cl = O.PackClient(po, out_n, seed=50 + 13 * q)
            cl.pp = cl.pub_params()
            srv.set_pub_params(*cl.pp)
            clients.append(cl)
            qs.append(cl.query(indices(s, B, 8)[q]))
        single = {}
        for q in range(B):
            for k in range(F):
                probes[k].set_pub_params(*clients[q].pp)
                single[q, k] = (probes[k].answer(qs[q])[0], probes[k].read_response_wire())
        sa.set_option("pack_item_group", group)
        outs = {}
        for lanes_value in (0, 2):
            sa.set_option("pack_batch_lanes", lanes_value)
            counted = sa.get_option("pack_lane_batches")
            outs[lanes_value] = P.answer_batch_instances(servers, instances, qs, wire=True)
            assert sa.get_option("pack_lane_batches") - counted == (1 if lanes_value else 0)
        assert_eq(outs[2][0], outs[0][0], "responses: lane form vs per-lane form")
        assert_eq(outs[2][1], outs[0][1], "wire forms: lane form vs per-lane form")
        for q in range(B):
            for k in range(F):
                assert_eq(outs[2][0][q, k], single[q, k][0], f"slot [{q}, {k}]: response vs client {q}'s single answer on instance {k}")
                assert_eq(outs[2][1][q, k], single[q, k][1], f"slot [{q}, {k}]: wire form vs the single answer's")
    finally:
        for k, v in before.items():
            sa.set_option(k, v)
        for srv in servers[1:] + probes + instances:
            srv.close()


@pytest.mark.parametrize("geom", [G_SMALL, G_UNCOVERED], ids=["small", "uncovered"])
def test_mixed_streams(sa, P, oracle_mt, geom):
    """three clients, the owner and lane 1 on one caller-made stream and lane 2 on its own: the join and release of every multi-lane call skip the
    lanes that share servers[0]'s stream and order the other.  The batch per lane and in lane form, an item call on one instance and a lane-form
    batch behind one bind_keys of all three lanes leave every lane's response, packed ciphertext, wire form and accumulators as its own single
    answer does; at the covered geometry the responses are the oracle's too"""
    import torch

    st = Setup(sa, oracle_mt, geom, 3, salt=5)
    stream = torch.cuda.Stream()  # (outlives the servers: set_stream does not give a server's own stream back)
    store = None
    before = sa.get_option("pack_batch_lanes")
    try:
        for srv in st.servers[:2]:
            srv.set_stream(stream.cuda_stream)
        trials = st.s.trials
        singles = [single_of(srv, q, trials) for srv, q in zip(st.servers, st.qs)]
        states = both_forms(sa, P, st)
        for b in range(3):
            assert_state_eq(states[b], singles[b], f"lane {b}: batch vs its single answer")
        if geom is G_SMALL:
            assert_oracle(st, states)
        sa.set_option("pack_batch_lanes", 2)
        counted = sa.get_option("pack_lane_batches")
        resp, wire = P.answer_batch_instances(st.servers, st.servers[:1], st.qs, wire=True)
        assert sa.get_option("pack_lane_batches") - counted == 1
        for b in range(3):
            assert_eq(resp[b, 0], singles[b][0], f"item call, client {b}: response vs its single answer")
            assert_eq(wire[b, 0], singles[b][2], f"item call, client {b}: wire form vs its single answer's")
        # lane b now serves client (b + 1) % 3: one bind of all three lanes, then a lane-form batch of those clients' queries
        store = sa.KeyStore(st.pg, 3, out_n=st.out_n, form="full")
        for c, cl in enumerate(st.clients):
            store.put(c, *cl.pp)
        slots = [1, 2, 0]
        P.bind_keys(st.servers, store, slots)
        bound = Setup.__new__(Setup)
        bound.__dict__.update(st.__dict__)
        bound.clients, bound.idx, bound.qs = ([x[c] for c in slots] for x in (st.clients, st.idx, st.qs))
        got, _ = batch_with(sa, P, 2, bound.servers, bound.qs, trials, 1)
        for b in range(3):
            assert_state_eq(got[b], single_of(bound.servers[b], bound.qs[b], trials), f"behind bind_keys, lane {b}: batch vs its single answer")
        if geom is G_SMALL:
            assert_oracle(bound, got)
    finally:
        sa.set_option("pack_batch_lanes", before)
        if store:
            store.close()
        st.close()
