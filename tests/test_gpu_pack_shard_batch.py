"""SpiralPack batches on trial-sharded servers (include/spiral_gpu.h create_shard_lane, fold_trials_batch, pack_gathered_batch): the ranks are emulated on
one device, one owner per trial range plus its shard lanes.  Every rank's block [lane][k] is written into one torch buffer at
spiral_amd.dist.pack_batch_position -- the buffer an all-gather would fill -- whose padding and tail guard are pre-filled with a sentinel and must stay
untouched.  Every lane's block must equal its own fold_trials', the root's responses its own pack_gathered's and the oracle's."""
import ctypes as C
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2048
CT = 2 * N
SENT = -0x5A5A5A5A5A5A5A5B  # 0xA5A5A5A5A5A5A5A5: above Q = 2^56, no ciphertext word


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


@pytest.fixture(scope="module")
def D(sa):
    from spiral_amd import dist

    return dist


def assert_eq(got, exp, what):
    got, exp = np.asarray(got), np.asarray(exp)
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp) if got.shape == exp.shape else []
        raise AssertionError(f"{what}: shapes {got.shape} / {exp.shape}, {len(bad)} of {got.size} words differ, first at {bad[:5].tolist() if len(bad) else []}")


def sentinel_buffer(cts):
    import torch

    return torch.full((cts * CT,), SENT, dtype=torch.int64, device="cuda")


class Ranks:
    """the emulated ranks: per trial range an owner with the device-generated database and B - 1 shard lanes, lane b with client b's keys"""

    def __init__(self, sa, D, O, po, pg, out_n, cuts, B, db_seed=41, client_seed=100, extra_lanes=0):
        self.sa, self.D, self.O, self.po, self.pg, self.out_n, self.cuts, self.B = sa, D, O, po, pg, out_n, list(cuts), B
        self.s = O.pack_shape_of(po, out_n)
        assert self.cuts[-1] == self.s.trials
        self.clients = []
        for b in range(B):
            cl = O.PackClient(po, out_n, seed=client_seed + 17 * b)
            cl.pp = cl.pub_params()
            self.clients.append(cl)
        self.ranks = []
        for a, e in zip(self.cuts[:-1], self.cuts[1:]):
            own = sa.PackServer(pg, out_n, 0, a, e)
            own.gen_db(db_seed)
            srv = [own] + [own.create_shard_lane() for _ in range(B - 1 + extra_lanes)]
            for sv, cl in zip(srv, self.clients):
                sv.set_pub_params(*cl.pp)
            self.ranks.append(srv)
        self.block = D.pack_batch_block_cts(B, self.cuts)
        self.n_ranks = len(self.cuts) - 1

    def length(self, r):
        return self.cuts[r + 1] - self.cuts[r]

    def buffer(self):
        return sentinel_buffer(self.n_ranks * self.block + 1)  # (one ciphertext of tail guard)

    def fold(self, P, qs, buf, form="ntt", lists=None):
        import torch

        for r, srv in enumerate(lists or [srv[:self.B] for srv in self.ranks]):
            P.fold_trials_batch(srv, qs, buf.data_ptr() + r * self.block * CT * 8, form=form)
        torch.cuda.synchronize()

    def blocks(self, buf):
        """{(rank, lane): [len_r, CT] words} read at pack_batch_position; everything else of the buffer must still be the sentinel"""
        host = buf.cpu().numpy().reshape(-1, CT)
        seen = np.zeros(host.shape[0], dtype=bool)
        out = {}
        for r in range(self.n_ranks):
            for b in range(self.B):
                at = [self.D.pack_batch_position(r, b, k, self.B, self.cuts, self.block) for k in range(self.length(r))]
                seen[at] = True
                out[r, b] = host[at].view(np.uint64)
        assert (host[~seen] == SENT).all(), "padding or the tail guard of the gathered buffer was written"
        assert (~seen).sum() == self.n_ranks * self.block + 1 - self.B * self.s.trials
        return out

    def close(self):
        for srv in self.ranks:
            for sv in reversed(srv):
                sv.close()


def fold_alone(sv, q, nt):
    """one server's own fold_trials: ([nt, CT] folded words, the accumulators of its trials); the word behind its output stays untouched"""
    import torch

    t = sentinel_buffer(nt + 1)
    sv.fold_trials(q, t.data_ptr())
    torch.cuda.synchronize()
    host = t.cpu().numpy().reshape(-1, CT)
    assert (host[nt] == SENT).all()
    return host[:nt].view(np.uint64).copy(), [sv.read_acc(tr) for tr in range(sv.trial0, sv.trial1)]


def pack_alone(sv, folded_by_rank):
    """one server's own pack_gathered on its trial-ordered ciphertexts: (response, packed ciphertext, wire form)"""
    import torch

    g = torch.from_numpy(np.concatenate(folded_by_rank).view(np.int64)).cuda()
    resp, packed = sv.pack_gathered(g.data_ptr(), want_packed=True)
    return resp, packed, sv.read_response_wire()


def check_against_singles(rk, blocks, single, tag):
    for r in range(rk.n_ranks):
        for b in range(rk.B):
            assert_eq(blocks[r, b], single[r, b][0], f"{tag}: rank {r}, lane {b}: block vs the lane's own fold_trials")
            for k, acc in enumerate(single[r, b][1]):
                assert_eq(rk.ranks[r][b].read_acc(rk.cuts[r] + k), acc, f"{tag}: rank {r}, lane {b}: accumulators of trial {rk.cuts[r] + k}")


def test_packed_image_unequal_ranges(sa, P, D, oracle, opts):
    """(4, 2, 2), cuts (0, 1, 3, 4), three clients with their own keys, the vector-ALU sweeps: per lane and in lane form, bit for bit the same"""
    O = oracle
    nu1, nu2, out_n, kw, B, cuts = 4, 2, 2, dict(t_gsw=4), 3, (0, 1, 3, 4)
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    rk = Ranks(sa, D, O, po, pg, out_n, cuts, B)
    s = rk.s
    total = s.dim0 * s.num_per
    idx = [total - 1, 5, 22]
    qs = [cl.query(i) for cl, i in zip(rk.clients, idx)]
    db = O.pack_gen_db(po, out_n, 41)
    single = {(r, b): fold_alone(rk.ranks[r][b], qs[b], rk.length(r)) for r in range(rk.n_ranks) for b in range(B)}
    results = {}
    for lanes_opt in (0, 2):
        opts(pack_batch_lanes=lanes_opt)
        c0 = sa.get_option("pack_lane_batches")
        buf = rk.buffer()
        rk.fold(P, qs, buf)
        moved = sa.get_option("pack_lane_batches") - c0
        assert moved == (rk.n_ranks if lanes_opt else 0), f"pack_batch_lanes = {lanes_opt}: pack_lane_batches moved by {moved}"
        blocks = rk.blocks(buf)
        check_against_singles(rk, blocks, single, f"pack_batch_lanes = {lanes_opt}")
        assert rk.ranks[0][0].db_format() == P.DB_PACKED
        root = rk.ranks[0][:B]
        out, wires = P.pack_gathered_batch(root, buf.data_ptr(), cuts, rk.block, want_packed=True, wire=True)
        for b in range(B):
            exp_resp, exp_packed = O.pack_answer(po, out_n, qs[b], *rk.clients[b].pp, db)
            assert_eq(out[b][1], exp_packed, f"lane {b}: packed ciphertext vs the oracle")
            assert_eq(out[b][0], exp_resp, f"lane {b}: response vs the oracle")
            assert_eq(rk.clients[b].decode(out[b][0]), O.pack_db_item(po, out_n, 41, idx[b]), f"lane {b}: decoded items")
            assert_eq(wires[b], root[b].read_response_wire(), f"lane {b}: wire form vs read_response_wire")
        assert (buf.cpu().numpy().reshape(-1, CT)[-1] == SENT).all()
        results[lanes_opt] = (blocks, out, wires)
    for key in results[0][0]:
        assert_eq(results[2][0][key], results[0][0][key], f"block {key}: lane form vs per-lane form")
    for b in range(B):
        assert_eq(results[2][1][b][0], results[0][1][b][0], f"lane {b}: response, lane form vs per-lane form")
        assert_eq(results[2][2][b], results[0][2][b], f"lane {b}: wire form, lane form vs per-lane form")
    rk.close()


LIMB_CASES = [
    (7, 4, 3, (0, 4, 9), 2, {}),                          # 16 ciphertexts per slot: the narrow form; a ragged group, a first trial that is not 0
    (7, 4, 3, (0, 4, 9), 8, {}),
    (7, 3, 3, (0, 5, 9), 2, dict(pack_pair_blocks=1)),    # 8 per slot: the pair form; a half-empty pair block
]


@pytest.mark.parametrize("nu1,nu2,out_n,cuts,B,options", LIMB_CASES, ids=["narrow-B2", "narrow-B8", "pair-B2"])
def test_limb_planes(sa, P, D, oracle, opts, nu1, nu2, out_n, cuts, B, options):
    """the first batch converts each shard's images in place, every fold_trials_batch is ONE matrix-core pass, and the blocks equal the single
    flows' on the packed images of a second, unconverted set of shards"""
    O = oracle
    opts(**options)
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    assert P.has_limb_form(pg, out_n)
    rk = Ranks(sa, D, O, po, pg, out_n, cuts, B)
    total = rk.s.dim0 * rk.s.num_per
    qs = [cl.query((1 + 7919 * b) % total if b else total - 1) for b, cl in enumerate(rk.clients)]
    refs = []
    for a, e in zip(cuts[:-1], cuts[1:]):
        ref = sa.PackServer(pg, out_n, 0, a, e)
        ref.gen_db(41)
        refs.append(ref)
    single = {}
    for b, cl in enumerate(rk.clients):
        for r, ref in enumerate(refs):
            ref.set_pub_params(*cl.pp)
            single[r, b] = fold_alone(ref, qs[b], rk.length(r))
    buf = rk.buffer()
    import torch

    for r, srv in enumerate(rk.ranks):
        assert srv[0].db_format() == P.DB_PACKED
        m0 = sa.get_option("mfma_sweeps")
        P.fold_trials_batch(srv, qs, buf.data_ptr() + r * rk.block * CT * 8)
        torch.cuda.synchronize()
        assert sa.get_option("mfma_sweeps") == m0 + 1, f"rank {r}: one matrix-core pass per fold_trials_batch"
        assert srv[0].db_format() == P.DB_LIMBS and srv[-1].db_format() == P.DB_LIMBS
        assert refs[r].db_format() == P.DB_PACKED
    check_against_singles(rk, rk.blocks(buf), single, "first batch")
    m0 = sa.get_option("mfma_sweeps")
    buf2 = rk.buffer()
    rk.fold(P, qs, buf2)  # on the converted images
    assert sa.get_option("mfma_sweeps") == m0 + rk.n_ranks
    assert_eq(buf2.cpu().numpy(), buf.cpu().numpy(), "second batch, on the converted images")
    root = rk.ranks[0]
    out, wires = P.pack_gathered_batch(root, buf.data_ptr(), cuts, rk.block, want_packed=True, wire=True)
    for b, cl in enumerate(rk.clients):
        refs[0].set_pub_params(*cl.pp)
        resp, packed, wire = pack_alone(refs[0], [single[r, b][0] for r in range(rk.n_ranks)])
        assert_eq(out[b][0], resp, f"lane {b}: response vs its own pack_gathered")
        assert_eq(out[b][1], packed, f"lane {b}: packed ciphertext vs its own pack_gathered")
        assert_eq(wires[b], wire, f"lane {b}: wire form vs its own pack_gathered's")
        assert_eq(root[b].read_response_wire(), wire, f"lane {b}: read_response_wire")
    for ref in refs:
        ref.close()
    rk.close()


# ---- the message forms of a query (tests/test_gpu_seeded_input.py's client half) ----
def wire_of(sa, O, *mats):
    raws = [O.from_ntt(np.ascontiguousarray(m).reshape(-1, 2, N)).reshape(-1, N) for m in mats if np.asarray(m).size >= 2 * N]
    return sa.raw_to_wire(np.concatenate(raws))


def seeded_query(sa, O, seed, q, domain=3):
    """the seeded message of a query and the query with row 0 of every ciphertext replaced by the seed's expansion (what the server ends up holding)"""
    a = np.array(q, dtype=np.uint64, copy=True)
    v = a.reshape(-1, 2, 1, 2, N)
    nm = v.shape[0]
    v[:, 0] = sa.seed_expand(seed, domain, 0, nm).reshape(nm, 1, 2, N)
    raw = O.from_ntt(np.ascontiguousarray(v[:, 1:].reshape(-1, 2, N))).reshape(-1, N)
    return np.concatenate([np.frombuffer(seed, dtype=np.uint8), sa.raw_to_wire(raw)]), a


def test_direct_upload_query_forms(sa, P, D, oracle):
    """direct upload, t_conv = 56: the wire and the seeded form of the queries leave the NTT form's words, and the root's responses are the oracle's"""
    O = oracle
    nu1, nu2, out_n, B, cuts = 3, 3, 3, 2, (0, 5, 9)
    kw = dict(t_gsw=3, t_conv=56, t_exp=56, qprime_bits=27, p_db=4096, direct_upload=1)
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    rk = Ranks(sa, D, O, po, pg, out_n, cuts, B)
    total = rk.s.dim0 * rk.s.num_per
    idx = [total - 1, 3]
    rng = np.random.default_rng(77)
    msgs, qs = zip(*[seeded_query(sa, O, rng.integers(0, 256, size=32, dtype=np.uint8).tobytes(), cl.query(i)) for cl, i in zip(rk.clients, idx)])
    assert msgs[0].size == sa.pack_query_seeded_bytes(pg, out_n)
    wires_in = [wire_of(sa, O, q) for q in qs]
    single = {(r, b): fold_alone(rk.ranks[r][b], qs[b], rk.length(r)) for r in range(rk.n_ranks) for b in range(B)}
    bufs = {}
    for form, queries in (("ntt", list(qs)), ("wire", wires_in), ("seeded", list(msgs))):
        bufs[form] = rk.buffer()
        rk.fold(P, queries, bufs[form], form=form)
        check_against_singles(rk, rk.blocks(bufs[form]), single, f"{form} form")
    db = O.pack_gen_db(po, out_n, 41)
    out = P.pack_gathered_batch(rk.ranks[1][:B], bufs["seeded"].data_ptr(), cuts, rk.block, want_packed=True)  # (the root need not hold trial 0)
    for b in range(B):
        exp_resp, exp_packed = O.pack_answer(po, out_n, qs[b], *rk.clients[b].pp, db)
        assert_eq(out[b][1], exp_packed, f"lane {b}: packed ciphertext vs the oracle")
        assert_eq(out[b][0], exp_resp, f"lane {b}: response vs the oracle")
    rk.close()


def test_one_rank_equals_answer_batch(sa, P, D, oracle):
    """n_ranks = 1: a server that holds every trial and its shard lanes (ordinary lanes then): fold_trials_batch + pack_gathered_batch leave
    answer_batch's words for the same clients and queries"""
    O = oracle
    nu1, nu2, out_n, kw, B = 4, 2, 2, dict(t_gsw=4), 3
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    rk = Ranks(sa, D, O, po, pg, out_n, (0, 4), B)
    servers = rk.ranks[0]
    qs = [cl.query(i) for cl, i in zip(rk.clients, (7, 0, 33))]
    want, _ = P.answer_batch(servers, qs, want_packed=True)  # (shard lanes of a full owner are usable where create_lane's are)
    want_wire = [sv.read_response_wire() for sv in servers]
    want_acc = [[sv.read_acc(t) for t in range(4)] for sv in servers]
    P.answer_batch(servers, [cl.query(1) for cl in rk.clients])  # other results in between
    buf = rk.buffer()
    rk.fold(P, qs, buf)
    rk.blocks(buf)
    out, wires = P.pack_gathered_batch(servers, buf.data_ptr(), (0, 4), rk.block, want_packed=True, wire=True)
    for b in range(B):
        assert_eq(out[b][0], want[b][0], f"lane {b}: response vs answer_batch's")
        assert_eq(out[b][1], want[b][1], f"lane {b}: packed ciphertext vs answer_batch's")
        assert_eq(wires[b], want_wire[b], f"lane {b}: wire form vs answer_batch's")
        for t in range(4):
            assert_eq(servers[b].read_acc(t), want_acc[b][t], f"lane {b}: accumulators of trial {t}")
    one = P.pack_gathered_batch(servers[1:2], buf.data_ptr() + rk.block // B * CT * 8, (0, 4), 4)  # n = 1: lane 1's [k] as a block of its own
    assert_eq(one[0][0], want[1][0], "n = 1: lane 1's response")
    rk.close()


def test_bind_keys_on_shard_lanes(sa, P, D, oracle):
    """bind_keys on an owner and its shard lanes, then a batch == the batch after set_pub_params of the same clients"""
    O = oracle
    nu1, nu2, out_n, kw, B, cuts = 4, 2, 2, dict(t_gsw=4), 2, (0, 2, 4)
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    rk = Ranks(sa, D, O, po, pg, out_n, cuts, B)
    qs = [cl.query(i) for cl, i in zip(rk.clients, (9, 60))]
    buf = rk.buffer()
    rk.fold(P, qs, buf)
    want_blocks = rk.blocks(buf)
    want = P.pack_gathered_batch(rk.ranks[0], buf.data_ptr(), cuts, rk.block)
    store = sa.KeyStore(pg, B, out_n=out_n, form="full")
    for c, cl in enumerate(rk.clients):
        store.put(c, *cl.pp)
    for srv in rk.ranks:  # lane b now serves client 1 - b, on every rank
        P.bind_keys(srv, store, [1, 0])
    buf2 = rk.buffer()
    rk.fold(P, qs[::-1], buf2)
    got_blocks = rk.blocks(buf2)
    got = P.pack_gathered_batch(rk.ranks[0], buf2.data_ptr(), cuts, rk.block)
    for r in range(rk.n_ranks):
        for b in range(B):
            assert_eq(got_blocks[r, b], want_blocks[r, 1 - b], f"rank {r}, lane {b} behind bind_keys: client {1 - b}'s block")
    for b in range(B):
        assert_eq(got[b][0], want[1 - b][0], f"lane {b} behind bind_keys: client {1 - b}'s response")
    store.close()
    rk.close()


def test_update_enqueued_before_a_batch_is_seen(sa, P, D, oracle):
    """an update_db_items enqueued on the owner's stream right before fold_trials_batch is seen by every lane, with the owner listed last and with
    the owner not listed at all: the blocks equal the single flows' on a shard updated and synchronised beforehand, and the item decodes"""
    import torch

    O = oracle
    nu1, nu2, out_n, kw, B, cuts = 4, 2, 2, dict(t_gsw=4), 2, (0, 2, 4)
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    rk = Ranks(sa, D, O, po, pg, out_n, cuts, B, extra_lanes=1)
    s = rk.s
    for srv in rk.ranks:
        srv[2].set_pub_params(*rk.clients[0].pp)  # the extra lane serves client 0 too
    item = 37
    pts = O.pack_db_item(po, out_n, 99, item).reshape(s.trials, N)  # another database's item: one plaintext per trial
    qs = [cl.query(item) for cl in rk.clients]
    refs = []
    for r, (a, e) in enumerate(zip(cuts[:-1], cuts[1:])):
        ref = sa.PackServer(pg, out_n, 0, a, e)
        ref.gen_db(41)
        for t in range(a, e):
            ref.update_db_items(t, O.pack_items(pts[t:t + 1], 8), 8, [item])
        refs.append(ref)
    torch.cuda.synchronize()
    single = {}
    for b, cl in enumerate(rk.clients):
        for r, ref in enumerate(refs):
            ref.set_pub_params(*cl.pp)
            single[r, b] = fold_alone(ref, qs[b], rk.length(r))
    lists = [[rk.ranks[0][1], rk.ranks[0][0]], [rk.ranks[1][2], rk.ranks[1][1]]]  # rank 0: the owner last; rank 1: lanes only (client 0 on the extra lane)
    buf = rk.buffer()
    for r, (a, e) in enumerate(zip(cuts[:-1], cuts[1:])):
        for t in range(a, e):
            rk.ranks[r][0].update_db_items(t, O.pack_items(pts[t:t + 1], 8), 8, [item])
        order = [1, 0] if r == 0 else [0, 1]  # the client of each listed server
        P.fold_trials_batch(lists[r], [qs[c] for c in order], buf.data_ptr() + r * rk.block * CT * 8)
    torch.cuda.synchronize()
    blocks = rk.blocks(buf)
    for b in range(B):
        assert_eq(blocks[0, b], single[0, 1 - b][0], f"rank 0, lane {b} (client {1 - b}): block after the update")
        assert_eq(blocks[1, b], single[1, b][0], f"rank 1, lane {b}: block after the update")
    # the same clients in one order on both ranks for the pack: client 1 is lane 0 on rank 0 only, so fold rank 1 again in that order
    P.fold_trials_batch(lists[1][::-1], [qs[1], qs[0]], buf.data_ptr() + rk.block * CT * 8)
    torch.cuda.synchronize()
    out = P.pack_gathered_batch(lists[0], buf.data_ptr(), cuts, rk.block)
    for b, c in enumerate((1, 0)):
        assert_eq(rk.clients[c].decode(out[b][0]).reshape(s.trials, N), pts, f"lane {b} (client {c}): the updated item decodes")
    for ref in refs:
        ref.close()
    rk.close()


def test_refusals_leave_every_lane_as_it_was(sa, P, D, oracle):
    O = oracle
    nu1, nu2, out_n, kw, B, cuts = 4, 2, 2, dict(t_gsw=4), 2, (0, 2, 4)
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    rk = Ranks(sa, D, O, po, pg, out_n, cuts, B, extra_lanes=1)  # (the extra lane of each rank has no public parameters)
    qs = [cl.query(i) for cl, i in zip(rk.clients, (9, 60))]
    buf = rk.buffer()
    rk.fold(P, qs, buf)
    P.pack_gathered_batch(rk.ranks[0][:B], buf.data_ptr(), cuts, rk.block)
    lanes = rk.ranks[0][:B]
    before = [(sv.read_response_wire(), sv.read_acc(0), sv.read_acc(1)) for sv in lanes]
    L = sa.lib()
    err = lambda: L.spiral_gpu_last_error().decode()
    scratch = sentinel_buffer(rk.block + 1)
    out_host = np.zeros((B, out_n + 1, out_n, N), dtype=np.uint64)
    from spiral_amd._lib import U64P

    def handles(servers):
        return (C.c_void_p * max(len(servers), 1))(*[sv.h for sv in servers])

    def c_fold(servers, queries, form=0, bytes_each=0, n=None):
        ptrs = (C.c_void_p * max(len(queries), 1))(*[q.ctypes.data if q is not None else None for q in queries])
        rc = L.spiral_gpu_pack_server_fold_trials_batch(handles(servers), len(servers) if n is None else n, form, ptrs, bytes_each, C.c_void_p(scratch.data_ptr()))
        assert rc != 0
        return err()

    def c_pack(servers, cuts_=cuts, block=rk.block, outputs=True, n=None):
        resp = (U64P * B)(*[out_host[b].ctypes.data_as(U64P) for b in range(B)]) if outputs else None
        rc = L.spiral_gpu_pack_server_pack_gathered_batch(handles(servers), len(servers) if n is None else n, C.c_void_p(buf.data_ptr()),
                                                          (C.c_uint32 * len(cuts_))(*cuts_), len(cuts_) - 1, block, resp, None, None)
        assert rc != 0
        return err()

    other = Ranks(sa, D, O, po, pg, out_n, cuts, B, db_seed=42)
    bare = rk.ranks[0][2]
    assert "no servers" in c_fold(lanes, qs, n=0) and "no servers" in c_pack(lanes, n=0)
    nine = [lanes[0]] * 9
    assert "at most 8 clients" in c_fold(nine, qs * 5, n=9) and "at most 8 clients" in c_pack(nine, n=9)
    assert "listed twice" in c_fold([lanes[0], lanes[0]], qs) and "listed twice" in c_pack([lanes[0], lanes[0]])
    assert "database image" in c_fold([lanes[0], other.ranks[0][1]], qs) and "database image" in c_pack([lanes[0], other.ranks[0][1]])
    assert "other parameters" in c_fold([lanes[0], rk.ranks[1][1]], qs)  # a lane of the other trial range
    assert "public parameters" in c_fold([lanes[0], bare], qs) and "public parameters" in c_pack([lanes[0], bare])
    assert "query 1 is null" in c_fold(lanes, [qs[0], None])
    wq = [wire_of(sa, O, q) for q in qs]
    assert "bytes per query" in c_fold(lanes, wq, form=1, bytes_each=wq[0].size - 7)
    bad = wq[1].copy()
    bad[7 * 5:7 * 6] = 0xFF
    assert "query 1: coefficient 5 " in c_fold(lanes, [wq[0], bad], form=1, bytes_each=wq[0].size)
    assert "unknown query form" in c_fold(lanes, qs, form=7)
    assert "from 0 to" in c_pack(lanes, cuts_=(1, 2, 4)) and "from 0 to" in c_pack(lanes, cuts_=(0, 2, 3))
    assert "strictly increasing" in c_pack(lanes, cuts_=(0, 2, 2, 4)) and "strictly increasing" in c_pack(lanes, cuts_=(0, 3, 2, 4))
    assert "need at least" in c_pack(lanes, block=rk.block - 1)
    assert "no output" in c_pack(lanes, outputs=False)
    with pytest.raises(ValueError):
        P.fold_trials_batch(lanes, qs[:1], scratch.data_ptr())
    with pytest.raises(ValueError):
        P.fold_trials_batch(lanes, qs, scratch.data_ptr(), form="raw")
    # what the other calls refuse of a trial shard stays refused
    with pytest.raises(sa.SpiralGpuError, match="trial-sharded"):
        rk.ranks[0][0].create_lane()
    with pytest.raises(sa.SpiralGpuError, match="trial-sharded"):
        P.answer_batch(lanes, qs)
    with pytest.raises(sa.SpiralGpuError, match="trial-sharded"):
        P.answer_batch(lanes[1:], qs[1:])
    with pytest.raises(sa.SpiralGpuError, match="trial-sharded"):
        P.time_sweep_batch(lanes)
    with pytest.raises(sa.SpiralGpuError, match="lane"):
        lanes[1].gen_db(3)
    with pytest.raises(sa.SpiralGpuError, match="lane"):
        lanes[1].set_db_format(P.DB_PACKED)
    with pytest.raises(sa.SpiralGpuError, match="owner"):
        bare.create_shard_lane()  # a lane owns no image
    with pytest.raises(sa.SpiralGpuError, match="trial"):
        lanes[1].read_acc(2)
    assert_eq(lanes[1].read_db_items(1, 8, 3, 2), lanes[0].read_db_items(1, 8, 3, 2), "read_db_items through a shard lane")
    import torch

    torch.cuda.synchronize()
    assert (scratch.cpu().numpy() == SENT).all() and not out_host.any(), "a refused call wrote to its output"
    for b, sv in enumerate(lanes):
        assert_eq(sv.read_response_wire(), before[b][0], f"lane {b}: response after the refused calls")
        assert_eq(sv.read_acc(0), before[b][1], f"lane {b}: accumulators of trial 0 after the refused calls")
        assert_eq(sv.read_acc(1), before[b][2], f"lane {b}: accumulators of trial 1 after the refused calls")
    # the image outlives its owner while a shard lane holds it
    own, lane = rk.ranks[1][0], rk.ranks[1][1]
    want = fold_alone(lane, qs[1], 2)[0]
    own.close()
    assert_eq(fold_alone(lane, qs[1], 2)[0], want, "a shard lane after its owner was destroyed")
    rk.ranks[1] = rk.ranks[1][1:]
    other.close()
    rk.close()
