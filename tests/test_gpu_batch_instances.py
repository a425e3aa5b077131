"""Batched item queries (include/spiral_gpu.h spiral_gpu_server_run_query_batch_instances / answer_batch_instances): B clients -- an owner and its
lanes, each with its own keys and query -- against the same n database instances, one sweep per instance for all of them.  Expected values: each
client's own run_query_instances (answer_instances) alone, bit for bit, and the oracle's client decoding every plaintext of every item."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2048
WORDS = 6 * N

COVERED = (6, 6, dict(t_gsw=8))  # the matrix-core sweep covers it (sweep_mfma_ok)
COVERED_DIRECT = (6, 6, dict(t_gsw=4, t_conv=56, t_exp=2, t_exp_right=56, qprime_bits=27, p_db=32768, direct_upload=1))  # configs[3]'s form, small
FALLBACK = (4, 3, dict(t_gsw=4))  # no limb-plane form: per-query vector-ALU sweeps


@pytest.fixture(scope="module")
def sa():
    # torch first: it ships its own HIP runtime and the two must not be initialised in the opposite order
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


@pytest.fixture(scope="module")
def SV(sa):
    from spiral_amd import server

    return server


def assert_eq(got, exp, what):
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[:5].tolist()}")


def captures(sa):
    v = C.c_int64()
    assert sa.lib().spiral_gpu_get_option(b"graph_captures", C.byref(v)) == 0
    return v.value


class Setup:
    """n_inst instances (seeded db_seed + k) and n_clients client servers: an owner -- instance 0, or a server whose own database is none of the
    instances -- and its lanes, each with its own client's keys and a query for its own index"""

    def __init__(self, sa, O, nu1, nu2, kw, n_clients, n_inst, db_seed, owner_is_instance=True, stream_mode="own"):
        self.sa, self.O = sa, O
        self.po, self.pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
        self.db_seed = db_seed
        self.inst = []
        for k in range(n_inst):
            sv = sa.Server(self.pg)
            sv.gen_db(db_seed + k)
            self.inst.append(sv)
        if owner_is_instance:
            owner = self.inst[0]
        else:  # (create_lane needs an owner with a database: one the item batch never sweeps)
            owner = sa.Server(self.pg)
            owner.gen_db(db_seed + 100)
        self.own_owner = not owner_is_instance
        self.servers = [owner] + [sa.Server(self.pg, share_db_of=owner) for _ in range(n_clients - 1)]
        st = sa.lib().spiral_gpu_server_get_stream(owner.h)
        for b, sv in enumerate(self.servers[1:], 1):
            if stream_mode == "one" or (stream_mode == "two" and b % 2 == 0):
                sv.set_stream(st)
        total = 1 << (nu1 + nu2)
        self.clients = [O.Client(self.po, seed=300 + 17 * b + nu1) for b in range(n_clients)]
        self.pps = [c.pub_params() for c in self.clients]
        self.idx = [(7 + 977 * b) % total for b in range(n_clients)]
        self.queries = [c.query(i) for c, i in zip(self.clients, self.idx)]
        for sv, pp in zip(self.servers, self.pps):
            sv.set_pub_params(*pp)
        self.wb = sa.lib().spiral_gpu_response_wire_bytes(C.byref(self.pg), 2)

    def singles(self, n_inst):
        """each client's own run_query_instances on instances[:n_inst] (host form): (responses [B][n][3][2][N], folded ciphertexts likewise)"""
        out = [sv.answer_instances(self.inst[:n_inst], q) for sv, q in zip(self.servers, self.queries)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def batch(self, B, n, graphs=False, pre=True, wire=True, finals=True, repeat=1):
        """run_query_batch_instances for clients[:B] on instances[:n] into device buffers: (responses, finals or None, wire or None) on the host"""
        import torch

        S = self.servers[:B]
        S[0].use_graphs(graphs)
        resp = torch.zeros(B * n * WORDS, dtype=torch.int64, device="cuda")
        fin = torch.zeros(B * n * WORDS, dtype=torch.int64, device="cuda") if finals else None
        wir = torch.zeros(B * n * self.wb, dtype=torch.uint8, device="cuda") if wire else None
        for _ in range(repeat):
            for sv, q in zip(S, self.queries):
                sv.set_query(q)
                if not pre:
                    sv.run_pre()
            self.sa.run_query_batch_instances(S, self.inst[:n], resp.data_ptr(), fin.data_ptr() if finals else 0, wir.data_ptr() if wire else 0, pre=pre)
        for sv in S:
            sv.sync()
        torch.cuda.synchronize()
        host = lambda t: t.cpu().numpy().view(np.uint64).reshape(B, n, 3, 2, N)
        return host(resp), (host(fin) if finals else None), (wir.cpu().numpy().reshape(B, n, self.wb) if wire else None)

    def check_decode(self, resp, B, n, what, seeds=None):
        for b in range(B):
            for k in range(n):
                want = self.O.db_item(self.po, (seeds or {}).get(k, self.db_seed + k), self.idx[b])
                assert_eq(self.clients[b].decode(resp[b, k]), want, f"{what}: client {b}, plaintext {k} of item {self.idx[b]}")

    def close(self):
        for sv in self.servers[1:]:
            sv.close()
        if self.own_owner:
            self.servers[0].close()
        for sv in self.inst:
            sv.close()


@pytest.mark.parametrize("geom,owner_is_instance,stream_mode", [
    (COVERED, True, "own"),          # query compression, covered geometry; every client on its own stream
    (COVERED_DIRECT, False, "one"),  # direct upload (SpiralStream), covered; the owner's own image is not an instance; every client on the owner's stream
    (FALLBACK, True, "two"),         # a geometry without limb planes; clients on two streams
], ids=["covered", "covered-direct", "fallback"])
def test_bit_exact_per_client(sa, SV, oracle, geom, owner_is_instance, stream_mode):
    """B in {1, 2, 3, 8} x n in {1, 3, 7}, graphs on and off, pre = 1 and 0: every (client, instance) response and folded ciphertext equals the
    client's own run_query_instances, and every plaintext decodes.  The singles run on the packed images; the batches (B >= 2 on a covered geometry)
    convert them to limb planes on first use."""
    nu1, nu2, kw = geom
    T = Setup(sa, oracle, nu1, nu2, kw, 8, 7, 500, owner_is_instance, stream_mode)
    want_r, want_f = T.singles(7)
    covered = geom is not FALLBACK
    i = 0
    for B in (1, 2, 3, 8):
        for n in (1, 3, 7):
            graphs, pre = i % 2 == 1, i % 3 != 2
            r, f, _ = T.batch(B, n, graphs=graphs, pre=pre, wire=False, repeat=2 if graphs else 1)
            what = f"B={B} n={n} graphs={graphs} pre={pre}"
            assert_eq(r, want_r[:B, :n], f"{what}: responses")
            assert_eq(f, want_f[:B, :n], f"{what}: folded ciphertexts")
            i += 1
        if B >= 2:
            assert all(sv.db_format() == (SV.DB_LIMBS if covered else SV.DB_PACKED) for sv in T.inst), "instance image forms after a batch"
    T.check_decode(want_r, 8, 7, "singles")
    T.close()


def test_wire_form_and_one_client(sa, SV, oracle):
    """wire slot (q, k) == read_response_wire of client q answered alone on instance k, and round-trips through spiral_gpu_response_from_wire to the
    response; only wire (no responses buffer) gives the same bytes; n_clients = 1 equals run_query_instances, through the host form too"""
    import torch

    from spiral_amd import ops

    nu1, nu2, kw = COVERED
    T = Setup(sa, oracle, nu1, nu2, kw, 3, 3, 610)
    want = np.zeros((3, 3, T.wb), dtype=np.uint8)
    for b, (sv, q) in enumerate(zip(T.servers, T.queries)):
        for k in range(3):
            sv.answer_instances([T.inst[k]], q)
            want[b, k] = sv.read_response_wire()
    r, f, w = T.batch(3, 3, graphs=True, repeat=2)
    assert_eq(w, want, "wire slots")
    for b in range(3):
        for k in range(3):
            assert_eq(ops.response_from_wire(T.pg, w[b, k]), r[b, k], f"client {b} instance {k}: wire round trip")
    # wire alone: the switch goes to each lane's own response buffer first
    wir = torch.zeros(9 * T.wb, dtype=torch.uint8, device="cuda")
    for sv, q in zip(T.servers, T.queries):
        sv.set_query(q)
    sa.run_query_batch_instances(T.servers, T.inst, wire_ptr=wir.data_ptr())
    torch.cuda.synchronize()
    T.servers[0].sync()
    assert_eq(wir.cpu().numpy().reshape(3, 3, T.wb), want, "wire slots without a responses buffer")
    # host form, both outputs
    hr, us = sa.answer_batch_instances(T.servers, T.inst, T.queries)
    hw, _ = sa.answer_batch_instances(T.servers, T.inst, T.queries, wire=True)
    assert_eq(hr, r, "host form: responses")
    assert_eq(hw, want, "host form: wire")
    assert us > 0
    # one client: run_query_instances' results, in both forms
    r1, f1, w1 = T.batch(1, 3, graphs=False)
    want_r, want_f = T.singles(3)
    assert_eq(r1[0], want_r[0], "one client: responses")
    assert_eq(f1[0], want_f[0], "one client: folded ciphertexts")
    assert_eq(w1[0], want[0], "one client: wire")
    T.check_decode(r, 3, 3, "batch")
    T.close()


def test_image_forms(sa, SV, oracle):
    """instances in packed form, in limb-plane form, and a mixed set: one client (no conversion) and three (the packed ones converted on first
    use); afterwards single run_query_instances and run_query on the converted images still match the oracle"""
    O = oracle
    nu1, nu2, kw = COVERED
    T = Setup(sa, O, nu1, nu2, kw, 3, 3, 720)
    want_r, want_f = T.singles(3)
    T.inst[1].set_db_format(SV.DB_LIMBS)  # mixed: packed, limbs, packed
    r, f, _ = T.batch(1, 3)
    assert [sv.db_format() for sv in T.inst] == [SV.DB_PACKED, SV.DB_LIMBS, SV.DB_PACKED], "one client converts nothing"
    assert_eq(r[0], want_r[0], "mixed forms, one client")
    r, f, _ = T.batch(3, 3, graphs=True)
    assert all(sv.db_format() == SV.DB_LIMBS for sv in T.inst)
    assert_eq(r, want_r, "mixed forms, three clients")
    assert_eq(f, want_f, "mixed forms, three clients: folded ciphertexts")
    r, f, _ = T.batch(2, 3, graphs=True)  # all limb planes
    assert_eq(r, want_r[:2], "limb planes, two clients")
    # single paths on the converted images
    again_r, again_f = T.singles(3)
    assert_eq(again_r, want_r, "run_query_instances after the batch")
    lone = T.servers[1]
    fin, resp, _ = lone.answer(T.queries[1])  # run_query on the owner's (instance 0's) converted image
    assert_eq(fin, O.answer(T.po, T.queries[1], *T.pps[1], O.gen_db(T.po, 720)), "run_query on a converted image vs the oracle")
    T.check_decode(r, 2, 3, "limb planes")
    T.close()


def test_update_between_replays(sa, SV, oracle):
    """update_db_items on one instance between two replays of the same captured item batch: no re-capture (the process's capture count is unchanged),
    and the second batch reads the new items"""
    O = oracle
    nu1, nu2, kw = COVERED
    T = Setup(sa, O, nu1, nu2, kw, 3, 3, 830)
    r1, _, _ = T.batch(3, 3, graphs=True)  # converts the images to limb planes
    T.check_decode(r1, 3, 3, "before the update")
    import torch

    # one capture, then replays with the same buffers around an update of instance 1 (every client's index gets new items)
    resp = torch.zeros(9 * WORDS, dtype=torch.int64, device="cuda")
    S = T.servers
    S[0].use_graphs(True)

    def run():
        for sv, q in zip(S, T.queries):
            sv.set_query(q)
        sa.run_query_batch_instances(S, T.inst, resp.data_ptr())
        for sv in S:
            sv.sync()
        torch.cuda.synchronize()
        return resp.cpu().numpy().view(np.uint64).reshape(3, 3, 3, 2, N)

    run()
    c0 = captures(sa)
    ids = sorted(set(T.idx))
    pts = [O.db_item(T.po, 9999, i) for i in ids]
    T.inst[1].update_db_items(O.pack_items(np.stack(pts), 8), 8, ids)
    r2 = run()
    assert captures(sa) == c0, "update_db_items forced a re-capture"
    new = dict(zip(ids, pts))
    for b in range(3):
        assert_eq(T.clients[b].decode(r2[b, 1]), new[T.idx[b]], f"client {b}: the updated item on instance 1")
        assert_eq(T.clients[b].decode(r2[b, 0]), O.db_item(T.po, 830, T.idx[b]), f"client {b}: instance 0 unchanged")
    want_r, _ = T.singles(3)
    assert_eq(r2, want_r, "after the update: each client's own run_query_instances")
    # other output buffers are baked into another capture: exactly one, with the same answers
    resp2 = torch.zeros_like(resp)
    for sv, q in zip(S, T.queries):
        sv.set_query(q)
    c1 = captures(sa)
    sa.run_query_batch_instances(S, T.inst, resp2.data_ptr())
    for sv in S:
        sv.sync()
    assert captures(sa) == c1 + 1, "new output buffers: one capture"
    assert torch.equal(resp2, resp), "new output buffers: the same answers"
    T.close()


def test_atomic_failures(sa, SV, oracle):
    """each bad argument fails before anything is launched: pre-filled output buffers stay byte-identical"""
    import torch

    nu1, nu2, kw = FALLBACK
    T = Setup(sa, oracle, nu1, nu2, kw, 8, 2, 940)
    extra = sa.Server(T.pg, share_db_of=T.servers[0])  # a ninth client
    extra.set_pub_params(*T.pps[0])
    extra.set_query(T.queries[0])
    nodb = sa.Server(T.pg)
    other = sa.Server(sa.make_params(nu1, nu2 + 1, **kw))
    other.gen_db(1)
    fresh = sa.Server(T.pg, share_db_of=T.servers[0])  # its query is set but not converted
    fresh.set_pub_params(*T.pps[1])
    fresh.set_query(T.queries[1])
    for sv, q in zip(T.servers, T.queries):
        sv.set_query(q)
    fill = lambda n: torch.full((n,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    resp, fin, wir = fill(9 * 2 * WORDS), fill(9 * 2 * WORDS), fill(9 * 2 * T.wb)
    snap = [t.clone() for t in (resp, fin, wir)]
    S = T.servers
    cases = [
        ("listed twice", lambda: sa.run_query_batch_instances([S[0], S[1], S[1]], T.inst, resp.data_ptr(), fin.data_ptr(), wir.data_ptr())),
        ("at most 8", lambda: sa.run_query_batch_instances(S + [extra], T.inst, resp.data_ptr(), fin.data_ptr(), wir.data_ptr())),
        ("no database", lambda: sa.run_query_batch_instances(S[:2], [T.inst[0], nodb], resp.data_ptr(), fin.data_ptr(), wir.data_ptr())),
        ("differs", lambda: sa.run_query_batch_instances(S[:2], [T.inst[0], other], resp.data_ptr(), fin.data_ptr(), wir.data_ptr())),
        ("not converted", lambda: sa.run_query_batch_instances([S[0], fresh], T.inst, resp.data_ptr(), fin.data_ptr(), wir.data_ptr(), pre=False)),
        ("no output", lambda: sa.run_query_batch_instances(S[:2], T.inst, 0, fin.data_ptr(), 0)),
    ]
    for S_ in S[:1]:
        S_.run_pre()  # client 0 converted: only `fresh` is not
    for msg, call in cases:
        with pytest.raises(RuntimeError, match=msg):
            call()
        torch.cuda.synchronize()
        for t, s in zip((resp, fin, wir), snap):
            assert torch.equal(t, s), f"{msg}: an output buffer was written"
    for sv in (extra, fresh, nodb, other):
        sv.close()
    T.close()


def _random_sets(count, seed):
    """seeded small parameter sets (both query forms, several gadget dimensions and moduli) with a client count and an instance count"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < count:
        nu1, nu2 = int(rng.integers(2, 7)), int(rng.integers(1, 5))
        kw = dict(t_gsw=int(rng.integers(3, 9)), t_conv=int(rng.choice([2, 4, 8])), t_exp=int(rng.choice([2, 4, 8, 16])), qprime_bits=int(rng.integers(18, 30)),
                  p_db=int(rng.choice([4, 256, 4096])), direct_upload=int(rng.integers(0, 2)))
        if not kw["direct_upload"] and (1 << nu1) + kw["t_gsw"] * nu2 > 2048:
            continue
        out.append((nu1, nu2, kw, int(rng.integers(2, 5)), int(rng.integers(2, 4))))
    return out


@pytest.mark.parametrize("nu1,nu2,kw,B,n", _random_sets(4, 4242), ids=[f"set{i}" for i in range(4)])
def test_random_parameter_sets(sa, SV, oracle, nu1, nu2, kw, B, n):
    """seeded random draws through the new call: every slot's folded ciphertext == the oracle's answer for that client and instance, the response ==
    the oracle's switch of it, and both == the client's own run_query_instances"""
    O = oracle
    T = Setup(sa, O, nu1, nu2, kw, B, n, 1050)
    want_r, want_f = T.singles(n)
    r, f, _ = T.batch(B, n, graphs=True, repeat=2)
    assert_eq(r, want_r, f"{nu1},{nu2},{kw}: responses vs singles")
    assert_eq(f, want_f, f"{nu1},{nu2},{kw}: folded ciphertexts vs singles")
    for k in range(n):
        db = O.gen_db(T.po, 1050 + k)
        for b in range(B):
            want = O.answer(T.po, T.queries[b], *T.pps[b], db)
            assert_eq(f[b, k], want, f"{nu1},{nu2},{kw}: client {b} instance {k} vs the oracle")
            assert_eq(r[b, k], O.stage_rescale(T.po, want), f"{nu1},{nu2},{kw}: client {b} instance {k} response vs the oracle")
    T.close()


@pytest.mark.slow
def test_configs3_batch_of_four_items_at_full_size(sa, oracle_mt, request):
    """configs[3] at its real geometry (nu1 = 11, nu2 = 9, 56 GiB per image): four clients x three instances in one item batch.  Every response is
    bit-for-bit the client's own run_query_instances on the same images, equals the oracle's switch of its folded ciphertext, and every plaintext of
    every item decodes through the oracle's client."""
    M = oracle_mt
    kw = dict(t_gsw=4, t_conv=56, t_exp=2, t_exp_right=56, qprime_bits=27, p_db=32768, direct_upload=1)
    T = Setup(sa, M, 11, 9, kw, 4, 3, 4100, stream_mode="one")
    r, f, w = T.batch(4, 3, graphs=True, repeat=2)
    want_r, want_f = T.singles(3)
    assert_eq(r, want_r, "configs[3]: responses vs each client's run_query_instances")
    assert_eq(f, want_f, "configs[3]: folded ciphertexts vs each client's run_query_instances")
    for b in range(4):
        for k in range(3):
            assert_eq(r[b, k], M.stage_rescale(T.po, f[b, k]), f"configs[3]: client {b} instance {k}: the oracle's switch")
    T.check_decode(r, 4, 3, "configs[3]")
    us = sa.answer_batch_instances(T.servers, T.inst, T.queries)[1]
    lines = getattr(request.config, "_spiral_evidence", None)
    if lines is not None:
        lines.append(f"configs[3] item batch, 4 clients x 3 instances of {T.inst[0].db_device_bytes() / 2**30:.0f} GiB: bit-exact vs singles, every plaintext "
                     f"decoded; {us / 1e3:.1f} ms on the device (host form)")
    T.close()
