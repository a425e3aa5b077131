"""Queries and public parameters in their wire form (include/spiral_gpu.h spiral_gpu_server_set_query_wire, ..._set_pub_params_wire, the SpiralPack
answer_wire / answer_batch_wire): decoded and transformed on the device (ntt.hip LD_WIRE) into the buffers the NTT-form entry points fill.  Expected
values: the same server state and the same answers, bit for bit, as set_query / set_pub_params on the NTT form of the same ciphertexts, and the
oracle's to_ntt of the raw query."""
import ctypes as C
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2048
POLY = 7 * N

COMPRESSED = (4, 3, dict(t_gsw=4))
DIRECT = (5, 2, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1))
COVERED = (6, 6, dict(t_gsw=8))  # the matrix-core batch sweep covers it
COVERED_DIRECT = (6, 6, dict(t_gsw=4, t_conv=56, t_exp=2, t_exp_right=56, qprime_bits=27, p_db=32768, direct_upload=1))  # configs[3]'s form


@pytest.fixture(scope="module")
def sa():
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


@pytest.fixture(scope="module")
def SV(sa):
    from spiral_amd import server

    return server


@pytest.fixture(scope="module")
def P(sa):
    from spiral_amd import pack as _  # noqa: F401

    return sys.modules["spiral_amd.pack"]


def assert_eq(got, exp, what):
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[:5].tolist()}")


def captures(sa):
    v = C.c_int64()
    assert sa.lib().spiral_gpu_get_option(b"graph_captures", C.byref(v)) == 0
    return v.value


def wire_of(O, *mats):
    """the client's half: NTT-form matrices ([..][2][N] words; the oracle pads an absent one to one word) -> raw -> one wire message"""
    raws = [O.from_ntt(np.ascontiguousarray(m).reshape(-1, 2, N)).reshape(-1, N) for m in mats if np.asarray(m).size >= 2 * N]
    import spiral_amd

    return spiral_amd.raw_to_wire(np.concatenate(raws) if raws else np.zeros((0, N), dtype=np.uint64))


def make(sa, O, geom, seed=5, db_seed=77):
    nu1, nu2, kw = geom
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    cl = O.Client(po, seed=seed)
    return po, pg, cl


@pytest.mark.parametrize("geom", [COMPRESSED, DIRECT, COVERED_DIRECT], ids=["compressed", "direct", "covered-direct"])
def test_resident_query_equal(sa, SV, oracle, geom):
    """read(BUF_QUERY) after set_query_wire(raw_to_wire(from_ntt(q))) == after set_query(q) == the oracle's to_ntt of the raw query; a crafted
    query holding 0, p - 1, b - 1 and Q decodes to the oracle's transform too"""
    O = oracle
    po, pg, cl = make(sa, O, geom)
    s = O.shape_of(po)
    q = cl.query(3)
    raw = O.from_ntt(q.reshape(-1, 2, N)).reshape(-1, N)
    srv = sa.Server(pg)
    srv.set_query(q)
    a = srv.read(SV.BUF_QUERY)
    assert_eq(a.reshape(-1), q.reshape(-1), "set_query's resident query vs the client's")
    srv.set_query_wire(sa.raw_to_wire(raw))
    b = srv.read(SV.BUF_QUERY)
    assert_eq(b, a, "set_query_wire vs set_query")
    assert_eq(b.reshape(-1), O.to_ntt(raw).reshape(-1), "set_query_wire vs oracle to_ntt")
    assert b.shape == (s.n_query_cts, 2, 2, N)
    rng = np.random.default_rng(11)
    crafted = rng.integers(0, sa.Q + 1, size=raw.shape, dtype=np.uint64)
    edges = np.array([0, sa.P - 1, sa.B - 1, sa.Q], dtype=np.uint64)
    crafted[0, :4] = edges
    crafted[-1, -4:] = edges
    crafted[0, 100:2048:4] = sa.Q
    srv.set_query_wire(sa.raw_to_wire(crafted))
    assert_eq(srv.read(SV.BUF_QUERY).reshape(-1), O.to_ntt(crafted).reshape(-1), "crafted query with edge values vs oracle to_ntt")
    srv.close()


@pytest.mark.parametrize("geom", [COMPRESSED, DIRECT], ids=["compressed", "direct"])
def test_run_query_bit_identical(sa, SV, oracle, geom):
    """run_query's final ciphertext, response and response wire agree between the two ingest paths, graphs on and off, and with the public parameters
    through set_pub_params_wire too; the answer decodes to the item"""
    O = oracle
    po, pg, cl = make(sa, O, geom)
    wl, wr, w, v = cl.pub_params()
    idx = 5
    q = cl.query(idx)
    out = {}
    for graphs in (False, True):
        for path in ("ntt", "wire"):
            srv = sa.Server(pg)
            srv.gen_db(77)
            srv.use_graphs(graphs)
            if path == "ntt":
                srv.set_pub_params(wl, wr, w, v)
            else:
                srv.set_pub_params_wire(wire_of(O, wl, wr, w, v))
            for _ in range(2 if graphs else 1):
                if path == "ntt":
                    srv.set_query(q)
                else:
                    srv.set_query_wire(wire_of(O, q))
                srv.run_query()
                srv.sync()
            out[graphs, path] = (srv.read(SV.BUF_FINAL), srv.read(SV.BUF_RESPONSE), srv.read_response_wire())
            srv.close()
        for i, what in enumerate(("final ciphertext", "response", "response wire")):
            assert_eq(out[graphs, "wire"][i], out[graphs, "ntt"][i], f"graphs={graphs}: {what}")
    assert_eq(out[True, "wire"][1], out[False, "ntt"][1], "graphs on vs off")
    assert_eq(cl.decode(out[True, "wire"][1]), O.db_item(po, 77, idx), "decoded item")


def lanes(sa, O, pg, po, n, db_seed, seed0=300):
    owner = sa.Server(pg)
    owner.gen_db(db_seed)
    servers = [owner] + [sa.Server(pg, share_db_of=owner) for _ in range(n - 1)]
    clients = [O.Client(po, seed=seed0 + 17 * b) for b in range(n)]
    pps = [c.pub_params() for c in clients]
    for sv, pp in zip(servers, pps):
        sv.set_pub_params(*pp)
    return servers, clients, pps


@pytest.mark.parametrize("geom", [COVERED, COVERED_DIRECT], ids=["covered", "covered-direct"])
def test_batches_bit_identical(sa, SV, oracle, geom):
    """run_query_batch (B = 1, 3, 8), run_query_instances and run_query_batch_instances on wire-ingested queries (every lane set through
    set_query_wire) give the responses of the NTT-form queries, bit for bit"""
    import torch

    O = oracle
    nu1, nu2, kw = geom
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    servers, clients, _ = lanes(sa, O, pg, po, 8, 500)
    total = 1 << (nu1 + nu2)
    idx = [(7 + 977 * b) % total for b in range(8)]
    qs = [c.query(i) for c, i in zip(clients, idx)]
    qw = [wire_of(O, q) for q in qs]
    servers[0].use_graphs(True)
    for B in (1, 3, 8):
        res = {}
        for path in ("ntt", "wire"):
            for _ in range(2):  # capture + replay
                for b in range(B):
                    servers[b].set_query(qs[b]) if path == "ntt" else servers[b].set_query_wire(qw[b])
                sa.run_query_batch(servers[:B])
            for sv in servers[:B]:
                sv.sync()
            res[path] = [sv.read(SV.BUF_RESPONSE) for sv in servers[:B]]
        for b in range(B):
            assert_eq(res["wire"][b], res["ntt"][b], f"run_query_batch B={B}: lane {b}")
            assert_eq(clients[b].decode(res["wire"][b]), O.db_item(po, 500, idx[b]), f"B={B} lane {b}: decoded")
    servers[0].use_graphs(False)
    inst = [servers[0]]
    for k in range(1, 3):
        sv = sa.Server(pg)
        sv.gen_db(500 + k)
        inst.append(sv)
    words = 6 * N
    # run_query_instances: one client, three instances
    want = servers[1].answer_instances(inst, qs[1])[0]
    d = torch.zeros(3 * words, dtype=torch.int64, device="cuda")
    servers[1].set_query_wire(qw[1])
    servers[1].run_query_instances(inst, d.data_ptr())
    servers[1].sync()
    torch.cuda.synchronize()
    assert_eq(d.cpu().numpy().view(np.uint64).reshape(want.shape), want, "run_query_instances")
    # run_query_batch_instances: four clients, three instances
    want_b, _ = sa.answer_batch_instances(servers[:4], inst, qs[:4])
    d = torch.zeros(4 * 3 * words, dtype=torch.int64, device="cuda")
    for b in range(4):
        servers[b].set_query_wire(qw[b])
    sa.run_query_batch_instances(servers[:4], inst, d.data_ptr())
    for sv in servers[:4]:
        sv.sync()
    torch.cuda.synchronize()
    assert_eq(d.cpu().numpy().view(np.uint64).reshape(want_b.shape), want_b, "run_query_batch_instances")
    for sv in inst[1:] + servers[1:]:
        sv.close()
    servers[0].close()


def test_query_across_staging_chunks(sa, SV, oracle):
    """a direct-upload query of more polynomials than one staging chunk (4096): the configs[3] query geometry (nu1 = 11: 4168 polynomials) with a
    small second dimension; read back and answered like the NTT form"""
    O = oracle
    po, pg, cl = make(sa, O, (11, 2, dict(t_gsw=4, t_conv=56, t_exp=2, t_exp_right=56, qprime_bits=27, p_db=32768, direct_upload=1)))
    s = O.shape_of(po)
    assert s.n_query_cts * 2 > 4096
    q = cl.query(4321)
    srv = sa.Server(pg)
    srv.gen_db(9)
    srv.set_pub_params(*cl.pub_params())
    srv.set_query(q)
    srv.run_query()
    srv.sync()
    want_q, want_r = srv.read(SV.BUF_QUERY), srv.read(SV.BUF_RESPONSE)
    srv.set_query_wire(wire_of(O, q))
    assert_eq(srv.read(SV.BUF_QUERY), want_q, "resident query")
    srv.run_query()
    srv.sync()
    assert_eq(srv.read(SV.BUF_RESPONSE), want_r, "response")
    assert_eq(cl.decode(want_r), O.db_item(po, 9, 4321), "decoded")
    srv.close()


def test_failures(sa, SV, oracle):
    """a coefficient above Q and a wrong byte count fail, naming the index; afterwards run_query fails with the existing message; the next valid
    query is served, and a captured graph replays it without a re-capture.  Bad public parameters leave none set; NTT-form ones with a null
    buffer leave the previous ones."""
    O = oracle
    po, pg, cl = make(sa, O, COMPRESSED)
    wl, wr, w, v = cl.pub_params()
    srv = sa.Server(pg)
    srv.gen_db(77)
    srv.set_pub_params(wl, wr, w, v)
    srv.use_graphs(True)
    q = cl.query(6)
    good = wire_of(O, q)
    for _ in range(2):
        srv.set_query_wire(good)
        srv.run_query()
    srv.sync()
    want = srv.read(SV.BUF_RESPONSE)
    # NTT-form public parameters with a null buffer after two valid ones: refused before anything is written, the previous keys still answer
    U64P = C.POINTER(C.c_uint64)
    wl2, wr2 = O.Client(po, seed=6).pub_params()[:2]
    assert not (wl2 == wl).all()
    assert sa.lib().spiral_gpu_server_set_pub_params(srv.h, wl2.ctypes.data_as(U64P), wr2.ctypes.data_as(U64P), None, v.ctypes.data_as(U64P)) != 0
    assert "null" in sa.lib().spiral_gpu_last_error().decode()
    srv.run_query()
    srv.sync()
    assert_eq(srv.read(SV.BUF_RESPONSE), want, "after NTT-form public parameters with a null buffer")
    n0 = captures(sa)
    # the out-of-range value written into the bytes directly (raw_to_wire refuses it)
    wbad = good.copy()
    off = (2048 + 1234) * 7
    wbad[off:off + 7] = np.frombuffer(int(sa.Q + 1).to_bytes(7, "little"), dtype=np.uint8)
    with pytest.raises(sa.SpiralGpuError, match=r"coefficient 3282 \(polynomial 1, index 1234\) is above Q"):
        srv.set_query_wire(wbad)
    with pytest.raises(sa.SpiralGpuError, match="query and public parameters must be set first"):
        srv.run_query()
    srv.set_query_wire(good)
    srv.run_query()
    srv.sync()
    assert_eq(srv.read(SV.BUF_RESPONSE), want, "after a refused query")
    with pytest.raises(sa.SpiralGpuError, match=r"\d+ bytes, the wire form of 2 polynomials takes 28672"):
        srv.set_query_wire(good[:-7])
    with pytest.raises(sa.SpiralGpuError, match="query and public parameters must be set first"):
        srv.run_query()
    srv.set_query_wire(good)
    srv.run_query()
    srv.sync()
    assert_eq(srv.read(SV.BUF_RESPONSE), want, "after a short buffer")
    assert captures(sa) == n0, "a wire-ingested query forced a re-capture"
    # the largest 56-bit value, and bad public parameters
    wbad[off:off + 7] = 0xFF
    with pytest.raises(sa.SpiralGpuError, match="coefficient 3282"):
        srv.set_query_wire(wbad)
    pw = wire_of(O, wl, wr, w, v)
    pbad = pw.copy()
    pbad[-7:] = 0xFF
    npp = pw.size // POLY
    with pytest.raises(sa.SpiralGpuError, match=f"coefficient {npp * N - 1} "):
        srv.set_pub_params_wire(pbad)
    srv.set_query_wire(good)
    with pytest.raises(sa.SpiralGpuError, match="query and public parameters must be set first"):
        srv.run_query()
    srv.set_pub_params_wire(pw)
    srv.run_query()
    srv.sync()
    assert_eq(srv.read(SV.BUF_RESPONSE), want, "after bad public parameters")
    srv.use_graphs(False)
    srv.close()
    # a query of more than four polynomials: the device's flag names the coefficient (the two-polynomial one above was checked on the host)
    po, pg, cl = make(sa, O, DIRECT)
    srv = sa.Server(pg)
    srv.set_query(cl.query(2))
    qd = wire_of(O, cl.query(2))
    assert qd.size // POLY > 4
    k = 50 * N + 2047
    qd[7 * k:7 * k + 7] = np.frombuffer(int(sa.Q + 1).to_bytes(7, "little"), dtype=np.uint8)
    with pytest.raises(sa.SpiralGpuError, match=rf"coefficient {k} \(polynomial 50, index 2047\) is above Q"):
        srv.set_query_wire(qd)
    with pytest.raises(sa.SpiralGpuError, match="query and public parameters must be set first"):
        srv.run_query()
    srv.close()


PACK_GEOMS = [
    (6, 2, 2, {}),                                                        # SpiralPack, compressed
    (7, 7, 2, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1)),   # SpiralStreamPack, batch sweep covered
]


@pytest.mark.parametrize("nu1,nu2,out_n,kw", PACK_GEOMS, ids=["pack", "streampack"])
def test_pack_bit_identical(sa, P, oracle, nu1, nu2, out_n, kw):
    """answer_wire and answer_batch_wire (B = 1, 4) == answer / answer_batch, with set_pub_params_wire on the lanes; a bad query in a batch
    leaves every lane's previous results intact, and NTT-form public parameters with a null buffer the previous keys"""
    O = oracle
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    owner = sa.PackServer(pg, out_n)
    owner.gen_db(41)
    servers = [owner] + [owner.create_lane() for _ in range(3)]
    clients = [O.PackClient(po, out_n, seed=100 + 17 * b) for b in range(4)]
    pps = [c.pub_params() for c in clients]
    total = s.dim0 * s.num_per
    idx = [(1 + 7919 * b) % total for b in range(4)]
    qs = [c.query(i) for c, i in zip(clients, idx)]
    qw = [wire_of(O, q) for q in qs]
    for sv, pp in zip(servers, pps):
        sv.set_pub_params(*pp)
    r0, k0, _ = owner.answer(qs[0])
    # NTT-form public parameters with a null v_W after valid new keys: refused before anything is written, the previous keys still answer
    U64P = C.POINTER(C.c_uint64)
    ptr = [np.ascontiguousarray(m).ctypes.data_as(U64P) for m in pps[1][:3]]
    assert sa.lib().spiral_gpu_pack_server_set_pub_params(owner.h, ptr[0], ptr[1], ptr[2], None) != 0
    assert "null" in sa.lib().spiral_gpu_last_error().decode()
    r0b, k0b, _ = owner.answer(qs[0])
    assert_eq(r0b, r0, "answer after NTT-form public parameters with a null buffer: response")
    assert_eq(k0b, k0, "answer after NTT-form public parameters with a null buffer: packed ciphertext")
    want1, _ = P.answer_batch(servers[:1], qs[:1], want_packed=True)
    want4, _ = P.answer_batch(servers, qs, want_packed=True)
    for sv, pp in zip(servers, pps):  # (direct upload: v_W alone -- the oracle's client draws expansion keys it does not send)
        sv.set_pub_params_wire(wire_of(O, *(pp[3:] if kw.get("direct_upload") else pp)))
    r, k, us = owner.answer_wire(qw[0])
    assert_eq(r, r0, "answer_wire: response")
    assert_eq(k, k0, "answer_wire: packed ciphertext")
    assert us["total_us"] > 0
    got1, _ = P.answer_batch_wire(servers[:1], qw[:1], want_packed=True)
    got4, _ = P.answer_batch_wire(servers, qw, want_packed=True)
    for b in range(4):
        assert_eq(got4[b][0], want4[b][0], f"answer_batch_wire B=4 lane {b}: response")
        assert_eq(got4[b][1], want4[b][1], f"answer_batch_wire B=4 lane {b}: packed")
        assert_eq(clients[b].decode(got4[b][0]), O.pack_db_item(po, out_n, 41, idx[b]), f"lane {b}: decoded")
    assert_eq(got1[0][0], want1[0][0], "answer_batch_wire B=1")
    # a bad query (last lane) and a wrong size: refused, every lane's previous results intact
    before = [sv.read_response_wire() for sv in servers]
    acc = [sv.read_acc(0) for sv in servers]
    bad = qw[3].copy()
    bad[7 * 5:7 * 6] = 0xFF
    with pytest.raises(sa.SpiralGpuError, match=r"query 3: coefficient 5 "):
        P.answer_batch_wire(servers, qw[:3] + [bad])
    with pytest.raises(sa.SpiralGpuError, match="bytes per query"):
        P.answer_batch_wire(servers, [w[:-14] for w in qw])
    for b, sv in enumerate(servers):
        assert_eq(sv.read_response_wire(), before[b], f"lane {b}: response after a refused batch")
        assert_eq(sv.read_acc(0), acc[b], f"lane {b}: accumulators after a refused batch")
    got4b, _ = P.answer_batch_wire(servers, qw)
    for b in range(4):
        assert_eq(got4b[b][0], want4[b][0], f"after a refused batch: lane {b}")
    for sv in servers[1:]:
        sv.close()
    owner.close()


def test_seeded_random_sets(sa, SV, oracle):
    """seeded random parameter sets: set_pub_params_wire + set_query_wire answer like the oracle"""
    O = oracle
    rng = np.random.default_rng(2026)
    for _ in range(3):
        nu1, nu2 = int(rng.integers(2, 6)), int(rng.integers(1, 4))
        direct = int(rng.integers(0, 2))
        kw = dict(t_gsw=int(rng.integers(3, 9)), t_exp=int(rng.integers(2, 9)), qprime_bits=int(rng.choice([19, 20, 22])), direct_upload=direct)
        po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
        try:
            cl = O.Client(po, seed=int(rng.integers(1, 1 << 30)))
        except ValueError:
            continue
        pp = cl.pub_params()
        idx = int(rng.integers(0, 1 << (nu1 + nu2)))
        q = cl.query(idx)
        db_seed = int(rng.integers(1, 1000))
        srv = sa.Server(pg)
        srv.gen_db(db_seed)
        srv.set_pub_params_wire(wire_of(O, *pp))
        srv.set_query_wire(wire_of(O, q))
        srv.run_query()
        srv.sync()
        fin = O.answer(po, q, *pp, O.gen_db(po, db_seed))
        assert_eq(srv.read(SV.BUF_FINAL), fin, f"nu1={nu1} nu2={nu2} {kw}: final ciphertext")
        assert_eq(srv.read(SV.BUF_RESPONSE), O.stage_rescale(po, fin), f"nu1={nu1} nu2={nu2} {kw}: response")
        assert_eq(cl.decode(srv.read(SV.BUF_RESPONSE)), O.db_item(po, db_seed, idx), f"nu1={nu1} nu2={nu2} {kw}: decoded")
        srv.close()
