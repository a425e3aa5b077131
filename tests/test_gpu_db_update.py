"""In-place item updates (include/spiral_gpu.h spiral_gpu_server_update_db_items, spiral_gpu_pack_server_update_db_items): a scattered set of
items replaced in the image's CURRENT form -- packed or limb planes -- without converting it, without dropping captured graphs, ordered on the
holder's stream, and atomic on failure.  Expected images and answers come from the oracle's own helpers."""
import ctypes as C
import hashlib
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N = 2048
P_MOD, B_MOD = 268369921, 249561089


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


@pytest.fixture(scope="module")
def P(sa):
    return sys.modules["spiral_amd.pack"]


def assert_eq(got, exp, what):
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[:5].tolist()}")


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def word(enc):
    """an oracle encoding's two residue limbs -> device words (p-residue | b-residue << 32)"""
    return enc[..., 0, :] | (enc[..., 1, :] << np.uint64(32))


def updated_db5(O, po, db, ids, pts):
    """the oracle database in read_db_slots' layout [z][ii][c][j][m] with item ids[k] replaced by plaintext pts[k]"""
    s = O.shape_of(po)
    want = db.reshape(N, s.num_per, 2, s.dim0, 2).copy()
    for i, pt in zip(ids, pts):
        want[:, i % s.num_per, :, i // s.num_per, :] = word(O.encode_item(po, pt)).transpose(2, 1, 0)  # [m][c][z] -> [z][c][m]
    return want


def updated_db(O, po, db, ids, pts):
    s = O.shape_of(po)
    return updated_db5(O, po, db, ids, pts).reshape(db.shape) if len(ids) else db


def scattered_ids(s):
    """item 0, the last item, items of one 16-column block (ic = 2 ii + c: ii 16 .. 23), partner pairs j / j ^ 32 of one column, and a lone
    member of a pair (its partner keeps the old top-limb nibble)"""
    np_, last = s.num_per, s.dim0 * s.num_per - 1
    ids = [0, last] + [5 * np_ + ii for ii in range(16, 24)] + [10 * np_ + 3, (10 ^ 32) * np_ + 3, 33 * np_ + 40, (33 ^ 32) * np_ + 40, 7 * np_ + 3]
    assert len(set(ids)) == len(ids)
    return ids


def new_items(O, po, ids, seed):
    return [O.db_item(po, seed, i) for i in ids]


def hip_runtime():
    """the HIP runtime this process already has loaded (torch's, which the library shares)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            hip = C.CDLL(line.split()[-1])
            hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            return hip
    raise RuntimeError("no HIP runtime loaded")


# ---- base server -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def base66(sa, oracle):
    O = oracle
    kw = dict(t_gsw=8)
    po, pg = O.make_params(6, 6, **kw), sa.make_params(6, 6, **kw)
    return O, po, pg, O.shape_of(po), O.gen_db(po, 21)


@pytest.mark.parametrize("form", ["packed", "limbs"])
def test_update_in_place_keeps_the_form(sa, SV, base66, form):
    """1 / 2: a scattered id set into the packed image and into the limb planes: read_db_slots over every slot is the oracle database with those
    items replaced, read_db_item of updated and neighbouring items is right, the form is unchanged; the limb planes converted back give the bytes of
    a fresh load of the updated database (no top-limb nibble torn)"""
    O, po, pg, s, db = base66
    srv = sa.Server(pg)
    srv.gen_db(21)
    fmt = SV.DB_PACKED if form == "packed" else SV.DB_LIMBS
    if form == "limbs":
        srv.set_db_format(SV.DB_LIMBS)
    bytes0 = srv.db_device_bytes()
    ids = scattered_ids(s)
    pts = new_items(O, po, ids, 99)
    srv.update_db_items(O.pack_items(np.stack(pts), 8), 8, ids)
    assert srv.db_format() == fmt, "the image keeps its form"
    assert srv.db_device_bytes() == bytes0
    want = updated_db5(O, po, db, ids, pts)
    assert_eq(srv.read_db_slots(0, N), want, f"{form}: read_db_slots")
    for i in ids[:4] + [ids[2] + 1, 10 * s.num_per + 4, 1]:
        pt = pts[ids.index(i)] if i in ids else O.db_item(po, 21, i)
        assert_eq(srv.read_db_item(i), O.encode_item(po, pt), f"{form}: read_db_item({i})")
    if form == "limbs":
        srv.set_db_format(SV.DB_PACKED)
        fresh = sa.Server(pg)
        total = s.dim0 * s.num_per
        all_pts = [pts[ids.index(i)] if i in ids else O.db_item(po, 21, i) for i in range(total)]
        fresh.load_db_items(O.pack_items(np.stack(all_pts), 8), 8)
        assert_eq(srv.read_db_slots(0, N), fresh.read_db_slots(0, N), "converted back == a fresh load of the updated database")
        fresh.close()
    srv.close()


def test_serving_across_an_update(sa, SV, base66):
    """3: an owner and three lanes, graphs on, limb planes.  batch, update on the owner's stream, batch -- no host synchronisation in between: the
    first batch saw the old database (its accumulators, copied on the owner's stream before the update, equal a warm-up batch's), the second the
    new one (oracle), the image was not converted, a query for an updated index decodes to the new plaintext, and a single run_query matches."""
    import torch

    O, po, pg, s, db = base66
    cl = O.Client(po, seed=9)
    pp = cl.pub_params()
    owner = sa.Server(pg)
    owner.gen_db(21)
    owner.set_db_format(SV.DB_LIMBS)
    servers = [owner] + [sa.Server(pg, share_db_of=owner) for _ in range(3)]
    ids = scattered_ids(s)
    idx = [ids[1], ids[3], 77, ids[-1]]  # updated, updated, untouched, the lone pair member
    qs = [cl.query(i) for i in idx]
    for sv, q in zip(servers, qs):
        sv.set_pub_params(*pp)
        sv.use_graphs(True)
        sv.set_query(q)
    hip = hip_runtime()
    stream = sa.lib().spiral_gpu_server_get_stream(owner.h)
    accs = [sv.acc() for sv in servers]
    warm = [torch.empty(nbytes // 8, dtype=torch.int64, device="cuda") for _, nbytes in accs]
    snaps = [torch.empty(nbytes // 8, dtype=torch.int64, device="cuda") for _, nbytes in accs]
    torch.cuda.synchronize()

    def snapshot(into):  # the lanes' accumulators, copied on the owner's stream (the batch's): ordered after what was enqueued there before
        for t, (ptr, nbytes) in zip(into, accs):
            assert hip.hipMemcpyAsync(t.data_ptr(), ptr, nbytes, 3, stream) == 0

    sa.run_query_batch(servers)  # warm-up: captures the batch graph on the limb planes
    snapshot(warm)
    for sv in servers:
        sv.sync()
    for sv, q, i in zip(servers, qs, idx):
        assert_eq(sv.read(SV.BUF_FINAL), O.answer(po, q, *pp, db), f"warm-up batch, item {i}")

    pts = new_items(O, po, ids, 99)
    items = O.pack_items(np.stack(pts), 8)
    sa.run_query_batch(servers)  # batch 1 (graph replay)
    snapshot(snaps)
    owner.update_db_items(items, 8, ids)
    sa.run_query_batch(servers)  # batch 2 (the same graph, replayed)
    for sv in servers:
        sv.sync()
    for b in range(len(servers)):
        assert_eq(snaps[b].cpu().numpy(), warm[b].cpu().numpy(), f"batch 1, lane {b}: the old database")
    assert owner.db_format() == SV.DB_LIMBS, "the update did not convert the image"
    new_db = updated_db(O, po, db, ids, pts)
    for b, (sv, q) in enumerate(zip(servers, qs)):
        assert_eq(sv.read(SV.BUF_FINAL), O.answer(po, q, *pp, new_db), f"batch 2, lane {b}: the new database")
    assert_eq(cl.decode(owner.read(SV.BUF_RESPONSE)), pts[1], "an updated index decodes to its new plaintext")
    owner.set_query(qs[1])
    owner.run_query()
    owner.sync()
    assert_eq(owner.read(SV.BUF_FINAL), O.answer(po, qs[1], *pp, new_db), "single run_query after the update")
    for sv in servers[1:] + [owner]:
        sv.close()


def test_sharded_and_second_image(sa, SV, oracle, opts):
    """4: a first dimension sharded over two servers (one in limb planes, one packed): ids outside a shard's j-range are skipped, each shard's image is
    the oracle's slice, and the shards' first-dimension accumulators sum to the unsharded server's.  Option one_image = 0: the packed image AND the
    valid second limb image are updated (a batch afterwards reads the limb image and matches the oracle)"""
    O = oracle
    kw = dict(t_gsw=8)
    po, pg = O.make_params(7, 6, **kw), sa.make_params(7, 6, **kw)
    s = O.shape_of(po)
    db = O.gen_db(po, 5)
    cl = O.Client(po, seed=4)
    pp = cl.pub_params()
    np_ = s.num_per
    ids = [0, 63 * np_ + 1, 64 * np_, 127 * np_ + np_ - 1, (64 + 40) * np_ + 9, (64 + 8) * np_ + 9, 20 * np_ + 9, (20 ^ 32) * np_ + 9]
    pts = new_items(O, po, ids, 7)
    items = O.pack_items(np.stack(pts), 8)
    want = updated_db5(O, po, db, ids, pts)
    full = sa.Server(pg)
    shards = [sa.Server(pg, j_begin=0, j_end=64), sa.Server(pg, j_begin=64, j_end=128)]
    for sv in [full] + shards:
        sv.gen_db(5)
        sv.set_pub_params(*pp)
    shards[0].set_db_format(SV.DB_LIMBS)
    for sv in [full] + shards:
        sv.update_db_items(items, 8, ids)
    assert shards[0].db_format() == SV.DB_LIMBS and shards[1].db_format() == SV.DB_PACKED
    for k, sv in enumerate(shards):
        assert_eq(sv.read_db_slots(0, 64), want[:64, :, :, 64 * k:64 * (k + 1), :], f"shard {k}: image")
        assert_eq(sv.read_db_slots(N - 8, 8), want[N - 8:, :, :, 64 * k:64 * (k + 1), :], f"shard {k}: image, last slots")
    q = cl.query(ids[4])
    accs = []
    for sv in [full] + shards:
        sv.set_query(q)
        sv.run_pre()
        sv.first_dim()
        sv.sync()
        accs.append(sv.read(SV.BUF_ACC).astype(np.uint64))
    a0, a1 = accs[1], accs[2]  # [ii][r][c][limb][z]: limb 0 mod p, limb 1 mod b
    summed = np.stack([(a0[..., 0, :] + a1[..., 0, :]) % np.uint64(P_MOD), (a0[..., 1, :] + a1[..., 1, :]) % np.uint64(B_MOD)], axis=-2)
    assert_eq(summed, accs[0], "the shards' accumulators sum to the unsharded server's")
    for sv in [full] + shards:
        sv.close()

    # option one_image = 0: a second limb image beside the packed one, built by a batch, updated with it
    opts(one_image=0)
    po, pg = O.make_params(6, 6, **kw), sa.make_params(6, 6, **kw)
    s = O.shape_of(po)
    db = O.gen_db(po, 21)
    owner = sa.Server(pg)
    owner.gen_db(21)
    lane = sa.Server(pg, share_db_of=owner)
    servers = [owner, lane]
    cl2 = O.Client(po, seed=11)
    pp2 = cl2.pub_params()
    ids = scattered_ids(s)
    qs = [cl2.query(ids[0]), cl2.query(ids[2])]
    for sv, q in zip(servers, qs):
        sv.set_pub_params(*pp2)
        sv.set_query(q)
    sa.run_query_batch(servers)
    owner.sync()
    bytes2 = owner.db_device_bytes()
    assert owner.db_format() == SV.DB_PACKED and bytes2 == 2 * N * s.dim0 * s.num_per * 4 * 7, "a second (limb-plane) image exists"
    pts = new_items(O, po, ids, 98)
    owner.update_db_items(O.pack_items(np.stack(pts), 8), 8, ids)
    assert owner.db_device_bytes() == bytes2, "the second image is kept"
    new_db = updated_db(O, po, db, ids, pts)
    assert_eq(owner.read_db_slots(0, 16), updated_db5(O, po, db, ids, pts)[:16], "packed image")
    sa.run_query_batch(servers)  # reads the limb image
    for b, (sv, q) in enumerate(zip(servers, qs)):
        sv.sync()
        assert_eq(sv.read(SV.BUF_FINAL), O.answer(po, q, *pp2, new_db), f"one_image = 0, lane {b}: the limb image was updated")
    lane.close()
    owner.close()


def test_small_geometry_packed_only(sa, SV, oracle):
    """4: geometries outside matrix-core coverage, packed form only: the 7-byte layout of a narrow shape and the plain layout (dim0 < 8)"""
    O = oracle
    for nu1, nu2, kw in [(4, 3, dict(t_gsw=8)), (2, 2, dict(t_gsw=4))]:
        po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
        s = O.shape_of(po)
        total = s.dim0 * s.num_per
        db = O.gen_db(po, 3)
        srv = sa.Server(pg)
        srv.gen_db(3)
        ids = sorted({0, total - 1, total // 2, 1})
        pts = new_items(O, po, ids, 4)
        srv.update_db_items(O.pack_items(np.stack(pts), 64), 64, ids)  # raw u64 words
        assert srv.db_format() == SV.DB_PACKED
        assert_eq(srv.read_db_slots(0, N), updated_db5(O, po, db, ids, pts), f"({nu1}, {nu2}): image")
        cl = O.Client(po, seed=2, nonoise=True)  # (the noisy client misdecodes a few coefficients at the 2^2 x 2^2 toy shape whatever the image)
        pp = cl.pub_params()
        srv.set_pub_params(*pp)
        q = cl.query(ids[-1])
        fin, resp, _ = srv.answer(q)
        assert_eq(fin, O.answer(po, q, *pp, updated_db(O, po, db, ids, pts)), f"({nu1}, {nu2}): answer")
        assert_eq(cl.decode(resp), pts[-1], f"({nu1}, {nu2}): decoded")
        srv.close()


def test_failures_leave_the_image_unchanged(sa, SV, base66):
    """5: a coefficient >= p_db in the last item, duplicate ids, an id >= the item count, a call through a lane: each raises, the image hashes the same
    as before, and a following query is still right"""
    O, po, pg, s, db = base66
    total = s.dim0 * s.num_per
    srv = sa.Server(pg)
    srv.gen_db(21)
    srv.set_db_format(SV.DB_LIMBS)
    lane = sa.Server(pg, share_db_of=srv)
    before = digest(srv.read_db_slots(0, N))
    ids = [3, 700, total - 2]
    pts = np.stack(new_items(O, po, ids, 50))
    bad = pts.copy()
    bad[-1, 1, 1, N - 1] = po.p_db  # the very last coefficient of the last item
    L = sa.lib()

    def raw_call(srv_, items, bits, id_list):
        a = np.ascontiguousarray(id_list, dtype=np.uint64)
        return L.spiral_gpu_server_update_db_items(srv_.h, items.ctypes.data_as(C.c_void_p), bits, a.ctypes.data_as(C.POINTER(C.c_uint64)), len(a))

    with pytest.raises(RuntimeError, match="p_db"):
        srv.update_db_items(O.pack_items(bad, 64), 64, ids)
    with pytest.raises(ValueError, match="duplicate"):
        srv.update_db_items(O.pack_items(pts, 8), 8, [3, 700, 3])
    assert raw_call(srv, O.pack_items(pts, 8), 8, [3, 700, 3]) != 0 and b"twice" in L.spiral_gpu_last_error()  # the library's own check
    with pytest.raises(RuntimeError, match="outside"):
        srv.update_db_items(O.pack_items(pts, 8), 8, [3, 700, total])
    with pytest.raises(RuntimeError, match="owner"):
        lane.update_db_items(O.pack_items(pts, 8), 8, ids)
    assert digest(srv.read_db_slots(0, N)) == before, "the image is byte-identical after every failed update"
    assert srv.db_format() == SV.DB_LIMBS
    cl = O.Client(po, seed=9)
    pp = cl.pub_params()
    srv.set_pub_params(*pp)
    q = cl.query(700)
    fin, resp, _ = srv.answer(q)
    assert_eq(fin, O.answer(po, q, *pp, db), "a query after the failed updates")
    lane.close()
    srv.close()


# ---- SpiralPack ------------------------------------------------------------------------------------------------------------------
def pack_word(O, po, pt):
    """a SpiralPack 1 x 1 plaintext's device words (the centred lift and transform are the base item's; the oracle's base encoder on a 2 x 2 item)"""
    return word(O.encode_item(po, np.stack([pt] * 4).reshape(2, 2, N)))[0, 0]


@pytest.mark.parametrize("nu1,nu2,out_n,kw,covered", [
    (7, 7, 1, {}, True),        # sweep1_mfma_ok: the batch converts to limb planes (terms j, partner j ^ 64)
    (6, 2, 2, {}, False),       # 4 output columns: packed only
])
def test_pack_update_both_forms(sa, P, oracle_mt, nu1, nu2, out_n, kw, covered):
    """6: a trial updated in place in both forms: every lane of answer_batch matches its own oracle answer on the updated trials; a trial outside
    a trial-sharded server's range is refused"""
    O = oracle_mt
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.pack_shape_of(po, out_n)
    total = s.dim0 * s.num_per
    db = O.pack_gen_db(po, out_n, 41)
    owner = sa.PackServer(pg, out_n)
    owner.gen_db(41)
    servers = [owner, owner.create_lane(), owner.create_lane()]
    clients = []
    for b, sv in enumerate(servers):
        cl = O.PackClient(po, out_n, seed=100 + 17 * b)
        cl.pp = cl.pub_params()
        sv.set_pub_params(*cl.pp)
        clients.append(cl)
    ids_all = [0, total - 1, 5 * s.num_per + 3, min(total - 1, (5 ^ 64) * s.num_per + 3) if s.dim0 > 64 else 6 * s.num_per + 3, 2 * s.num_per + 9 % s.num_per]
    ids_all = sorted(set(ids_all))
    rounds = [("packed", ids_all[:3], 61), ("after a batch", ids_all[2:], 62)]
    want_db = db.copy()
    for rnd, (tag, ids, seed) in enumerate(rounds):
        trial = rnd % s.trials
        pts = [O.pack_db_item(po, out_n, seed, i).reshape(s.trials, N)[trial] for i in ids]
        owner.update_db_items(trial, O.pack_items(np.stack(pts), 8), 8, ids)
        for i, pt in zip(ids, pts):
            w = pack_word(O, po, pt)
            want_db[trial].reshape(N, s.num_per, s.dim0)[:, i % s.num_per, i // s.num_per] = w
        idx = [ids[0], ids[-1], 17 % total]
        qs = [cl.query(i) for cl, i in zip(clients, idx)]
        out, _ = P.answer_batch(servers, qs, want_packed=True)
        assert owner.db_format() == (P.DB_LIMBS if covered else P.DB_PACKED)
        for b in range(len(servers)):
            wl, wr, v, vw = clients[b].pp
            exp_resp, exp_packed = O.pack_answer(po, out_n, qs[b], wl, wr, v, vw, want_db)
            assert_eq(out[b][0], exp_resp, f"{tag}: lane {b}, response")
        dec = clients[0].decode(out[0][0]).reshape(s.trials, N)
        assert_eq(dec[trial], pts[0], f"{tag}: the updated item decodes")
    with pytest.raises(RuntimeError, match="trial"):
        owner.update_db_items(s.trials, O.pack_items(np.stack(pts[:1]), 8), 8, ids[:1])
    with pytest.raises(RuntimeError, match="owner"):
        servers[1].update_db_items(0, O.pack_items(np.stack(pts[:1]), 8), 8, ids[:1])
    for sv in servers[1:] + [owner]:
        sv.close()
    if s.trials > 1:
        half = sa.PackServer(pg, out_n, trial0=0, trial1=1)
        half.gen_db(41)
        with pytest.raises(RuntimeError, match="trial"):
            half.update_db_items(1, O.pack_items(np.stack(pts[:1]), 8), 8, ids[:1])
        half.close()


# ---- seeded random draws ---------------------------------------------------------------------------------------------------------
GEOMS = [(6, 6, dict(t_gsw=8)), (7, 6, dict(t_gsw=8)), (4, 3, dict(t_gsw=8)), (3, 2, dict(t_gsw=4))]


@pytest.mark.parametrize("seed", range(6))
def test_random_draws_equal_a_fresh_load(sa, SV, oracle, seed):
    """7: a seeded draw of geometry, form, id set, coefficient width and sharding: the updated image reads back as a fresh load of the updated database"""
    O = oracle
    rng = np.random.default_rng(1000 + seed)
    nu1, nu2, kw = GEOMS[seed % len(GEOMS)]
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    s = O.shape_of(po)
    total = s.dim0 * s.num_per
    n_shards = int(rng.integers(1, 3)) if s.dim0 >= 128 else 1
    span = s.dim0 // n_shards
    limbs_ok = s.num_per >= 64 and 64 <= span <= 2048
    form = SV.DB_LIMBS if limbs_ok and rng.integers(2) else SV.DB_PACKED
    n = int(rng.integers(1, min(total, 200)))
    ids = rng.choice(total, size=n, replace=False)
    if limbs_ok:  # make sure some partner pairs are both present
        extra = [(i ^ (32 * s.num_per)) for i in ids[: n // 3]]
        ids = np.unique(np.concatenate([ids, extra]))
        rng.shuffle(ids)
    ids = [int(i) for i in ids]
    bits = int(rng.choice([8, 64]))
    pts = new_items(O, po, ids, 500 + seed)
    items = O.pack_items(np.stack(pts), bits)
    gen_seed = 30 + seed
    for k in range(n_shards):
        j0, j1 = k * span, (k + 1) * span
        srv = sa.Server(pg, j_begin=j0, j_end=j1) if n_shards > 1 else sa.Server(pg)
        srv.gen_db(gen_seed)
        if form == SV.DB_LIMBS:
            srv.set_db_format(form)
        srv.update_db_items(items, bits, ids)
        assert srv.db_format() == form
        fresh = sa.Server(pg, j_begin=j0, j_end=j1) if n_shards > 1 else sa.Server(pg)
        fresh.gen_db(gen_seed)
        for i, pt in zip(ids, pts):
            fresh.load_db_items(O.pack_items(pt, 8), 8, first_item=i, n_items=1)
        z0 = int(rng.integers(0, N - 64))
        for z, nz in ((0, 16), (z0, 64), (N - 16, 16)):
            assert_eq(srv.read_db_slots(z, nz), fresh.read_db_slots(z, nz), f"draw {seed}: ({nu1}, {nu2}), shard {k}/{n_shards}, form {form}, slots {z}+{nz}")
        fresh.close()
        srv.close()
