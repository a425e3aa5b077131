"""Queries and public parameters in their seeded form (include/spiral_gpu.h spiral_gpu_server_set_query_seeded, ..._set_pub_params_seeded and the
SpiralPack _seeded calls): row 0 of every matrix generated on the device from the message's seed (seed.hip), the other rows decoded as the wire form.
Expected values: row 0 equals the host expansion (spiral_gpu_seed_expand) and the server state and answers equal, bit for bit, those of the NTT-form
(resp. wire-form) entry points on the same matrices with row 0 replaced by that expansion -- and the oracle's answer on them.  ./spiral --seeded
runs valid encryptions end to end, so its decoded items check the client's half too."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2048
POLY = 7 * N
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "spiral_amd", "spiral")

COMPRESSED = (4, 3, dict(t_gsw=4))
DIRECT = (5, 2, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1))
COVERED = (6, 6, dict(t_gsw=8))
COVERED_DIRECT = (6, 6, dict(t_gsw=4, t_conv=56, t_exp=2, t_exp_right=56, qprime_bits=27, p_db=32768, direct_upload=1))
# a direct query whose seeded form sends more polynomials than one staging chunk (4096): 2^12 + 2 * 4 = 4104 ciphertexts, one polynomial each
CHUNKED = (12, 2, dict(t_gsw=4, t_conv=56, t_exp=2, t_exp_right=56, qprime_bits=27, p_db=32768, direct_upload=1))
STAGING_CHUNK = 4096


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


def new_seed(rng):
    return rng.integers(0, 256, size=32, dtype=np.uint8).tobytes()


def seeded(sa, O, seed, domain, mats):
    """the client's half: mats = (NTT-form array, rows, cols) in message order (an absent matrix: fewer than 2N words).  Returns the seeded
    message and the arrays with row 0 of every matrix replaced by the seed's expansion (what the server must end up holding)"""
    k, sent, out = 0, [], []
    for m, r, c in mats:
        a = np.array(m, dtype=np.uint64, copy=True)
        out.append(a)
        if a.size < 2 * N:
            continue
        v = a.reshape(-1, r, c, 2, N)
        nm = v.shape[0]
        v[:, 0] = sa.seed_expand(seed, domain, k, nm * c).reshape(nm, c, 2, N)
        k += nm * c
        sent.append(v[:, 1:].reshape(-1, 2, N))
    raw = O.from_ntt(np.ascontiguousarray(np.concatenate(sent))).reshape(-1, N)
    return np.concatenate([np.frombuffer(seed, dtype=np.uint8), sa.raw_to_wire(raw)]), out


def wire_of(sa, O, *mats):
    raws = [O.from_ntt(np.ascontiguousarray(m).reshape(-1, 2, N)).reshape(-1, N) for m in mats if np.asarray(m).size >= 2 * N]
    return sa.raw_to_wire(np.concatenate(raws))


def seeded_query(sa, O, seed, q, domain=1):
    msg, (q2,) = seeded(sa, O, seed, domain, [(q, 2, 1)])
    return msg, q2


def seeded_pp(sa, O, seed, pg, pp):
    msg, out = seeded(sa, O, seed, 2, [(pp[0], 2, pg.t_exp), (pp[1], 2, pg.t_exp_right), (pp[2], 3, 2 * pg.t_conv), (pp[3], 3, 2 * pg.t_conv)])
    return msg, tuple(out)


def make(sa, O, geom, seed=5):
    nu1, nu2, kw = geom
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    return po, pg, O.Client(po, seed=seed)


@pytest.mark.parametrize("geom", [COMPRESSED, DIRECT, CHUNKED], ids=["compressed", "direct", "direct-chunked"])
def test_device_row0_equals_host(sa, SV, oracle, geom):
    """read(BUF_QUERY) after set_query_seeded: row 0 of every ciphertext is seed_expand's, row 1 the oracle's transform of the decoded wire"""
    O = oracle
    po, pg, cl = make(sa, O, geom)
    s = O.shape_of(po)
    rng = np.random.default_rng(31)
    seed = new_seed(rng)
    msg, _ = seeded_query(sa, O, seed, cl.query(3))
    assert msg.size == sa.query_seeded_bytes(pg) == 32 + s.n_query_cts * POLY
    srv = sa.Server(pg)
    srv.set_query_seeded(msg)
    got = srv.read(SV.BUF_QUERY)
    assert got.shape == (s.n_query_cts, 2, 2, N)
    assert_eq(got[:, 0], sa.seed_expand(seed, 1, 0, s.n_query_cts), "row 0 vs the host expansion")
    rows1 = sa.raw_from_wire(msg[32:])
    assert_eq(got[:, 1].reshape(-1), O.to_ntt(rows1).reshape(-1), "row 1 vs the oracle's transform of the wire")
    if geom is CHUNKED:  # the ciphertexts on both sides of the chunk boundary, spelled out
        assert s.n_query_cts > STAGING_CHUNK
        tail = slice(STAGING_CHUNK - 2, s.n_query_cts)
        assert_eq(got[tail, 0], sa.seed_expand(seed, 1, STAGING_CHUNK - 2, s.n_query_cts - STAGING_CHUNK + 2), "row 0 across the chunk boundary")
        assert_eq(got[tail, 1].reshape(-1), O.to_ntt(rows1[tail]).reshape(-1), "row 1 across the chunk boundary")
    srv.close()


def test_query_across_staging_chunks(sa, SV, oracle):
    """the chunked geometry answered: a seeded query of more than one staging chunk gives the NTT path's resident query and response on the same
    ciphertexts with row 0 replaced"""
    O = oracle
    po, pg, cl = make(sa, O, CHUNKED)
    s = O.shape_of(po)
    assert s.n_query_cts > STAGING_CHUNK
    rng = np.random.default_rng(4104)
    qmsg, q2 = seeded_query(sa, O, new_seed(rng), cl.query(4321))
    pp = cl.pub_params()
    srv = sa.Server(pg)
    srv.gen_db(9)
    srv.set_pub_params(*pp)
    srv.set_query(q2)
    srv.run_query()
    srv.sync()
    want_q, want_r = srv.read(SV.BUF_QUERY), srv.read(SV.BUF_RESPONSE)
    srv.set_query_seeded(qmsg)
    assert_eq(srv.read(SV.BUF_QUERY), want_q, "resident query")
    srv.run_query()
    srv.sync()
    assert_eq(srv.read(SV.BUF_RESPONSE), want_r, "response")
    srv.close()


def run_once(sa, SV, srv):
    srv.run_query()
    srv.sync()
    return srv.read(SV.BUF_FINAL), srv.read(SV.BUF_RESPONSE), srv.read_response_wire()


@pytest.mark.parametrize("geom", [COMPRESSED, DIRECT, COVERED], ids=["compressed", "direct", "covered"])
def test_run_query_bit_identical(sa, SV, oracle, geom):
    """set_pub_params + set_query on the NTT form with row 0 replaced == set_pub_params_seeded + set_query_seeded: final ciphertext, response and
    wire response; both equal the oracle on those inputs.  A graph captured after one seeded query replays a second one without a re-capture"""
    O = oracle
    po, pg, cl = make(sa, O, geom)
    rng = np.random.default_rng(77)
    pp = cl.pub_params()
    pmsg, pp2 = seeded_pp(sa, O, new_seed(rng), pg, pp)
    assert pmsg.size == sa.pub_params_seeded_bytes(pg)
    qmsg, q2 = seeded_query(sa, O, new_seed(rng), cl.query(5))
    db_seed = 77
    ref = sa.Server(pg)
    ref.gen_db(db_seed)
    ref.set_pub_params(*pp2)
    ref.set_query(q2)
    want = run_once(sa, SV, ref)
    fin = O.answer(po, q2, *pp2, O.gen_db(po, db_seed))
    assert_eq(want[0], fin, "NTT path vs oracle: final ciphertext")
    assert_eq(want[1], O.stage_rescale(po, fin), "NTT path vs oracle: response")
    srv = sa.Server(pg)
    srv.gen_db(db_seed)
    srv.set_pub_params_seeded(pmsg)
    srv.set_query_seeded(qmsg)
    got = run_once(sa, SV, srv)
    for i, what in enumerate(("final ciphertext", "response", "response wire")):
        assert_eq(got[i], want[i], f"seeded vs NTT path: {what}")
    # graph replay: capture after one seeded query, replay a second
    qmsg_b, q2_b = seeded_query(sa, O, new_seed(rng), cl.query(9))
    ref.set_query(q2_b)
    want_b = run_once(sa, SV, ref)
    srv.use_graphs(True)
    srv.set_query_seeded(qmsg)
    srv.run_query()
    srv.sync()
    n0 = captures(sa)
    srv.set_query_seeded(qmsg_b)
    got_b = run_once(sa, SV, srv)
    assert captures(sa) == n0, "a seeded query forced a re-capture"
    for i, what in enumerate(("final ciphertext", "response", "response wire")):
        assert_eq(got_b[i], want_b[i], f"graph replay of a second seeded query: {what}")
    srv.use_graphs(False)
    srv.close()
    ref.close()


@pytest.mark.parametrize("geom", [COVERED, COVERED_DIRECT], ids=["covered", "covered-direct"])
def test_batches_bit_identical(sa, SV, oracle, geom):
    """run_query_batch with lanes (B = 3, 8) and run_query_batch_instances on seeded public parameters and queries == the NTT form with row 0
    replaced"""
    import torch

    O = oracle
    nu1, nu2, kw = geom
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    rng = np.random.default_rng(5150)
    owner = sa.Server(pg)
    owner.gen_db(500)
    servers = [owner] + [sa.Server(pg, share_db_of=owner) for _ in range(7)]
    clients = [O.Client(po, seed=300 + 17 * b) for b in range(8)]
    total = 1 << (nu1 + nu2)
    idx = [(7 + 977 * b) % total for b in range(8)]
    pps, qs, pms, qms = [], [], [], []
    for c, i in zip(clients, idx):
        pm, pp2 = seeded_pp(sa, O, new_seed(rng), pg, c.pub_params())
        qm, q2 = seeded_query(sa, O, new_seed(rng), c.query(i))
        pms.append(pm), pps.append(pp2), qms.append(qm), qs.append(q2)
    owner.use_graphs(True)
    for B in (3, 8):
        res = {}
        for path in ("ntt", "seeded"):
            for b in range(B):
                servers[b].set_pub_params(*pps[b]) if path == "ntt" else servers[b].set_pub_params_seeded(pms[b])
            for _ in range(2):  # capture + replay
                for b in range(B):
                    servers[b].set_query(qs[b]) if path == "ntt" else servers[b].set_query_seeded(qms[b])
                sa.run_query_batch(servers[:B])
            for sv in servers[:B]:
                sv.sync()
            res[path] = [sv.read(SV.BUF_RESPONSE) for sv in servers[:B]]
        for b in range(B):
            assert_eq(res["seeded"][b], res["ntt"][b], f"run_query_batch B={B}: lane {b}")
    owner.use_graphs(False)
    inst = [owner]
    for k in range(1, 3):
        sv = sa.Server(pg)
        sv.gen_db(500 + k)
        inst.append(sv)
    for b in range(4):
        servers[b].set_pub_params(*pps[b])
    want_b, _ = sa.answer_batch_instances(servers[:4], inst, qs[:4])
    for b in range(4):
        servers[b].set_pub_params_seeded(pms[b])
        servers[b].set_query_seeded(qms[b])
    d = torch.zeros(4 * 3 * 6 * N, dtype=torch.int64, device="cuda")
    sa.run_query_batch_instances(servers[:4], inst, d.data_ptr())
    for sv in servers[:4]:
        sv.sync()
    torch.cuda.synchronize()
    assert_eq(d.cpu().numpy().view(np.uint64).reshape(want_b.shape), want_b, "run_query_batch_instances")
    for sv in inst[1:] + servers[1:]:
        sv.close()
    owner.close()


def hip_runtime():
    """the HIP runtime this process already has loaded (torch's, which the library shares)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def test_failures(sa, SV, oracle):
    """a wrong size, a coefficient above Q (named by its index after the seed), a call under stream capture and a null message fail and leave no
    query (resp. no public parameters); the next valid message is served"""
    O = oracle
    po, pg, cl = make(sa, O, DIRECT)
    rng = np.random.default_rng(404)
    pmsg, _ = seeded_pp(sa, O, new_seed(rng), pg, cl.pub_params())
    qmsg, _ = seeded_query(sa, O, new_seed(rng), cl.query(2))
    srv = sa.Server(pg)
    srv.gen_db(77)
    srv.set_pub_params_seeded(pmsg)
    srv.set_query_seeded(qmsg)
    want = run_once(sa, SV, srv)[1]
    not_set = "query and public parameters must be set first"
    ncts = O.shape_of(po).n_query_cts
    with pytest.raises(sa.SpiralGpuError, match=rf"{qmsg.size - 7} bytes, the seeded form of {2 * ncts} polynomials \({ncts} of them row 0\) takes {qmsg.size}"):
        srv.set_query_seeded(qmsg[:-7])
    with pytest.raises(sa.SpiralGpuError, match=not_set):
        srv.run_query()
    srv.set_query_seeded(qmsg)
    assert_eq(run_once(sa, SV, srv)[1], want, "after a short message")
    assert ncts > 40  # (more than four polynomials sent: the device's error word names the coefficient)
    k = 40 * N + 2047
    bad = qmsg.copy()
    bad[32 + 7 * k:32 + 7 * k + 7] = np.frombuffer(int(sa.Q + 1).to_bytes(7, "little"), dtype=np.uint8)
    with pytest.raises(sa.SpiralGpuError, match=rf"coefficient {k} \(polynomial 40, index 2047\) is above Q"):
        srv.set_query_seeded(bad)
    with pytest.raises(sa.SpiralGpuError, match=not_set):
        srv.run_query()
    assert sa.lib().spiral_gpu_server_set_query_seeded(srv.h, None, qmsg.size) != 0
    assert "null" in sa.lib().spiral_gpu_last_error().decode()
    with pytest.raises(sa.SpiralGpuError, match=not_set):
        srv.run_query()
    with pytest.raises(sa.SpiralGpuError, match="shorter than the 32-byte seed"):
        srv.set_query_seeded(qmsg[:31])
    pbad = pmsg.copy()
    pbad[-7:] = 0xFF
    npp = (pmsg.size - 32) // POLY
    srv.set_query_seeded(qmsg)
    with pytest.raises(sa.SpiralGpuError, match=f"coefficient {npp * N - 1} "):
        srv.set_pub_params_seeded(pbad)
    with pytest.raises(sa.SpiralGpuError, match=not_set):
        srv.run_query()
    srv.set_pub_params_seeded(pmsg)
    assert_eq(run_once(sa, SV, srv)[1], want, "after bad public parameters")
    # under stream capture: refused before anything is enqueued, and no query is left
    hip = hip_runtime()
    st = C.c_void_p()
    assert hip.hipStreamCreate(C.byref(st)) == 0
    srv.set_stream(st.value)
    assert hip.hipStreamBeginCapture(st, 2) == 0  # (hipStreamCaptureModeRelaxed)
    try:
        with pytest.raises(sa.SpiralGpuError, match="capturing"):
            srv.set_query_seeded(qmsg)
        with pytest.raises(sa.SpiralGpuError, match="capturing"):
            srv.set_pub_params_seeded(pmsg)
    finally:
        g = C.c_void_p()
        assert hip.hipStreamEndCapture(st, C.byref(g)) == 0
        if g.value:
            hip.hipGraphDestroy(g)
    with pytest.raises(sa.SpiralGpuError, match=not_set):
        srv.run_query()
    srv.set_pub_params_seeded(pmsg)
    srv.set_query_seeded(qmsg)
    assert_eq(run_once(sa, SV, srv)[1], want, "after a refused call under capture")
    srv.close()
    hip.hipStreamDestroy(st)


PACK_GEOMS = [
    (6, 2, 2, {}),                                                        # SpiralPack, compressed
    (7, 7, 2, dict(t_gsw=5, t_exp=2, qprime_bits=19, direct_upload=1)),   # SpiralStreamPack, batch sweep covered
]


@pytest.mark.parametrize("nu1,nu2,out_n,kw", PACK_GEOMS, ids=["pack", "streampack"])
def test_pack_bit_identical(sa, P, oracle, nu1, nu2, out_n, kw):
    """set_pub_params_seeded, answer_seeded, answer_batch_seeded (B = 1, 4) and answer_batch_instances_seeded == their _wire forms on the same
    matrices with row 0 replaced; a bad query in a batch is refused"""
    O = oracle
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    direct = bool(kw.get("direct_upload"))
    rng = np.random.default_rng(606)
    owner = sa.PackServer(pg, out_n)
    owner.gen_db(41)
    servers = [owner] + [owner.create_lane() for _ in range(3)]
    clients = [O.PackClient(po, out_n, seed=100 + 17 * b) for b in range(4)]
    total = s.dim0 * s.num_per
    idx = [(1 + 7919 * b) % total for b in range(4)]
    pms, pws, qms, qws = [], [], [], []
    for c, i in zip(clients, idx):
        wl, wr, v, vw = c.pub_params()
        if direct:  # (v_W alone: the oracle's client draws expansion keys it does not send)
            wl = wr = v = np.zeros(1, dtype=np.uint64)
        pm, (wl2, wr2, v2, vw2) = seeded(sa, O, new_seed(rng), 4, [(wl, 2, pg.t_exp), (wr, 2, pg.t_exp_right), (v, 2, 2 * pg.t_conv),
                                                                   (vw, out_n + 1, pg.t_conv)])
        assert pm.size == sa.pack_pub_params_seeded_bytes(pg, out_n)
        pms.append(pm), pws.append(wire_of(sa, O, wl2, wr2, v2, vw2))
        qm, q2 = seeded_query(sa, O, new_seed(rng), c.query(i), domain=3)
        assert qm.size == sa.pack_query_seeded_bytes(pg, out_n)
        qms.append(qm), qws.append(wire_of(sa, O, q2))
    for sv, pw in zip(servers, pws):
        sv.set_pub_params_wire(pw)
    r0, k0, _ = owner.answer_wire(qws[0])
    want1, _ = P.answer_batch_wire(servers[:1], qws[:1], want_packed=True)
    want4, _ = P.answer_batch_wire(servers, qws, want_packed=True)
    inst = [owner]
    for k in range(1, 3):
        sv = sa.PackServer(pg, out_n)
        sv.gen_db(41 + k)
        inst.append(sv)
    want_i = P.answer_batch_instances_wire(servers[:2], inst, qws[:2])
    for sv, pm in zip(servers, pms):
        sv.set_pub_params_seeded(pm)
    r, k, us = owner.answer_seeded(qms[0])
    assert_eq(r, r0, "answer_seeded: response")
    assert_eq(k, k0, "answer_seeded: packed ciphertext")
    got1, _ = P.answer_batch_seeded(servers[:1], qms[:1], want_packed=True)
    assert_eq(got1[0][0], want1[0][0], "answer_batch_seeded B=1")
    got4, _ = P.answer_batch_seeded(servers, qms, want_packed=True)
    for b in range(4):
        assert_eq(got4[b][0], want4[b][0], f"answer_batch_seeded B=4 lane {b}: response")
        assert_eq(got4[b][1], want4[b][1], f"answer_batch_seeded B=4 lane {b}: packed")
    got_i = P.answer_batch_instances_seeded(servers[:2], inst, qms[:2])
    assert_eq(got_i, want_i, "answer_batch_instances_seeded")
    bad = qms[3].copy()
    bad[32 + 7 * 5:32 + 7 * 6] = 0xFF
    with pytest.raises(sa.SpiralGpuError, match=r"query 3: coefficient 5 "):
        P.answer_batch_seeded(servers, qms[:3] + [bad])
    with pytest.raises(sa.SpiralGpuError, match="bytes per query, the seeded form"):
        P.answer_batch_seeded(servers, [w[:-14] for w in qms])
    for sv in inst[1:] + servers[1:]:
        sv.close()
    owner.close()


def test_seeded_random_sets(sa, SV, oracle):
    """seeded random parameter sets: set_pub_params_seeded + set_query_seeded answer like the oracle on the row-0-replaced inputs"""
    O = oracle
    rng = np.random.default_rng(4242)
    done = 0
    for _ in range(4):
        nu1, nu2 = int(rng.integers(2, 6)), int(rng.integers(1, 4))
        direct = int(rng.integers(0, 2))
        kw = dict(t_gsw=int(rng.integers(3, 9)), t_exp=int(rng.integers(2, 9)), qprime_bits=int(rng.choice([19, 20, 22])), direct_upload=direct)
        po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
        try:
            cl = O.Client(po, seed=int(rng.integers(1, 1 << 30)))
        except ValueError:
            continue
        pmsg, pp2 = seeded_pp(sa, O, new_seed(rng), pg, cl.pub_params())
        qmsg, q2 = seeded_query(sa, O, new_seed(rng), cl.query(int(rng.integers(0, 1 << (nu1 + nu2)))))
        db_seed = int(rng.integers(1, 1000))
        srv = sa.Server(pg)
        srv.gen_db(db_seed)
        srv.set_pub_params_seeded(pmsg)
        srv.set_query_seeded(qmsg)
        srv.run_query()
        srv.sync()
        fin = O.answer(po, q2, *pp2, O.gen_db(po, db_seed))
        assert_eq(srv.read(SV.BUF_FINAL), fin, f"nu1={nu1} nu2={nu2} {kw}: final ciphertext")
        assert_eq(srv.read(SV.BUF_RESPONSE), O.stage_rescale(po, fin), f"nu1={nu1} nu2={nu2} {kw}: response")
        srv.close()
        done += 1
    assert done >= 2


def summary(out, name):
    m = re.search(name + r" \(b\): (\d+)", out)
    return int(m.group(1)) if m else None


@pytest.mark.parametrize("args", [
    ["8", "7", "1234", "a", "--seed", "41"],
    ["4", "3", "40", "a", "--seed", "42", "--batch", "4"],
    ["4", "3", "40", "a", "--seed", "43", "--batch", "3", "--instances", "3"],
    ["5", "2", "7", "a", "--direct-upload", "--seed", "44", "--batch", "3", "--instances", "3"],
    ["6", "2", "9", "a", "--high-rate", "--seed", "45"],
    ["6", "2", "9", "a", "--high-rate", "--seed", "46", "--batch", "3"],
], ids=["configs1", "batch", "batch-instances", "direct-batch-instances", "high-rate", "high-rate-batch"])
def test_cli_seeded(sa, args):
    """./spiral ... --seeded: valid encryptions with row 0 from the seeds, every plaintext decodes; the seeded sizes are printed on lines of their
    own and equal the size functions'; the reference's summary lines keep their figures"""
    e = dict(os.environ)
    if "--direct-upload" in args:
        e.update({"TEXP": "2", "TGSW": "5", "QPBITS": "19"})
    r = subprocess.run([BIN] + args + ["--seeded"], capture_output=True, text=True, env=e, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = r.stdout
    assert re.search(r"Is correct\s?\?\s?: 1\n", out), out
    for m in re.finditer(r"Is correct\?:((?: [01])+)", out):
        assert set(m.group(1).split()) == {"1"}, out
    pp, q = summary(out, "Seeded public parameters upload"), summary(out, "Seeded query upload")
    assert pp and q, out
    assert "Wire input, uploaded" not in out
    if args[:2] == ["8", "7"]:
        assert (q, pp) == (14_368, 7_110_688)
        assert summary(out, "Total online query size") == 28_672
    if "--high-rate" not in args:
        assert q == 32 + summary(out, "Total online query size") // 2
