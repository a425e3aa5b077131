"""Database items read back as plaintexts (include/spiral_gpu.h spiral_gpu_server_read_db_items / _at, spiral_gpu_pack_server_read_db_items / _at): the
bit-packed item stream that load_db_items / update_db_items take, gathered from the image in whichever form it is in -- packed, plain, limb planes
(wide, narrow, and SpiralPack's pair form) -- without converting it.  Every expected byte comes from the oracle's generators (db_item, pack_db_item)
and its packer (pack_items)."""
import ctypes as C
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

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


@pytest.fixture(scope="module")
def SV(sa):
    from spiral_amd import server

    return server


@pytest.fixture(scope="module")
def P(sa):
    from spiral_amd import pack as _  # noqa: F401  (spiral_amd.pack is also the name of a function: take the module itself)

    return sys.modules["spiral_amd.pack"]


def assert_bytes(got, exp, what, item_bytes=None):
    assert got.dtype == np.uint8 and got.shape == exp.shape, f"{what}: {got.dtype} {got.shape} for {exp.shape}"
    if not (got == exp).all():
        bad = np.flatnonzero(got != exp)
        where = f", first in item {bad[0] // item_bytes} of the call" if item_bytes else ""
        raise AssertionError(f"{what}: {len(bad)} of {got.size} bytes differ, first at byte {bad[0]}{where}")


def assert_eq(got, exp, what):
    if not (got.shape == exp.shape and (got == exp).all()):
        bad = np.argwhere(got != exp)
        raise AssertionError(f"{what}: {len(bad)} of {got.size} words differ, first at {bad[:5].tolist()}")


_PLAIN = {}


def plain_db(O, po, seed):
    """every plaintext of the oracle database, [item][4 * 2048] (computed once per geometry and seed, never written)"""
    s = O.shape_of(po)
    key = (po.nu1, po.nu2, po.p_db, seed)
    if key not in _PLAIN:
        total = s.dim0 * s.num_per
        pts = np.empty((total, 4 * N), dtype=np.uint32)
        for i in range(total):
            pts[i] = O.db_item(po, seed, i).reshape(-1)
        pts.setflags(write=False)
        _PLAIN[key] = pts
    return _PLAIN[key]


def packed(O, pts, bits):
    """the oracle packer's bytes of the plaintexts pts[k] (a few hundred items at a time: the packer works on u64)"""
    if len(pts) == 0:
        return np.zeros(0, dtype=np.uint8)
    return np.concatenate([O.pack_items(pts[k:k + 256], bits) for k in range(0, len(pts), 256)])


def base_params(sa, O, nu1, nu2, **kw):
    po, pg = O.make_params(nu1, nu2, **kw), sa.make_params(nu1, nu2, **kw)
    return po, pg, O.shape_of(po)


def scattered_ids(s):
    """(tests/test_gpu_db_update.py's set) item 0, the last item, items of one 16-column block (ic = 2 ii + c: ii 16 .. 23), partner pairs j / j ^ 32 of
    one column, and a lone member of a pair"""
    np_, last = s.num_per, s.dim0 * s.num_per - 1
    ids = [0, last] + [5 * np_ + ii for ii in range(16, 24)] + [10 * np_ + 3, (10 ^ 32) * np_ + 3, 33 * np_ + 40, (33 ^ 32) * np_ + 40, 7 * np_ + 3]
    assert len(set(ids)) == len(ids)
    return ids


KW66 = dict(t_gsw=8)


# ---- 1. the whole database, both forms ---------------------------------------------------------------------------------------------
def test_whole_database_both_forms(sa, SV, oracle, opts):
    """a full 8-bit export in three staging passes equals the packer's bytes of all 4096 oracle items, from the packed image and again from the limb planes;
    form, device bytes and the capture count are unchanged, and a graph captured before the export replays after it"""
    O = oracle
    po, pg, s = base_params(sa, O, 6, 6, **KW66)
    total = s.dim0 * s.num_per
    want = packed(O, plain_db(O, po, 21), 8)
    item_bytes = sa.db_items_bytes(pg, 8, 1)
    assert item_bytes == 8192 and want.size == total * item_bytes
    opts(db_stage_bytes=12 << 20)  # 1536 items per pass: 3 passes
    srv = sa.Server(pg)
    srv.gen_db(21)
    cl = O.Client(po, seed=9)
    pp = cl.pub_params()
    srv.set_pub_params(*pp)
    srv.use_graphs(True)
    q = cl.query(700)
    exp_fin = O.answer(po, q, *pp, O.gen_db(po, 21))
    for fmt, tag in ((SV.DB_PACKED, "packed"), (SV.DB_LIMBS, "limb planes")):
        if fmt == SV.DB_LIMBS:
            srv.set_db_format(SV.DB_LIMBS)
        srv.set_query(q)
        srv.run_query()  # captures the query's graph on this form
        srv.sync()
        assert_eq(srv.read(SV.BUF_FINAL), exp_fin, f"{tag}: the query before the export")
        bytes0, caps = srv.db_device_bytes(), sa.get_option("graph_captures")
        got = srv.read_db_items(8)
        assert_bytes(got, want, f"{tag}: full export", item_bytes)
        assert srv.db_format() == fmt and srv.db_device_bytes() == bytes0, f"{tag}: the image keeps its form and its size"
        srv.set_query(cl.query(701))
        srv.run_query()
        srv.set_query(q)
        srv.run_query()  # the captured graph, replayed
        srv.sync()
        assert sa.get_option("graph_captures") == caps, f"{tag}: the export forced a capture"
        assert_eq(srv.read(SV.BUF_FINAL), exp_fin, f"{tag}: the captured graph replays after the export")
    srv.close()


# ---- 2. widths and sub-ranges -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["packed", "limbs"])
def test_widths_and_subranges(sa, SV, oracle, form):
    """coeff_bits 8, 9, 13 and 64 at p_db = 256: sub-ranges that start and end inside a j row, the first items, the last items"""
    O = oracle
    po, pg, s = base_params(sa, O, 6, 6, **KW66)
    total, np_ = s.dim0 * s.num_per, s.num_per
    pts = plain_db(O, po, 21)
    srv = sa.Server(pg)
    srv.gen_db(21)
    if form == "limbs":
        srv.set_db_format(SV.DB_LIMBS)
    for bits in (8, 9, 13, 64):
        assert sa.db_items_bytes(pg, bits, 1) == 1024 * bits
        for first, n in ((np_ + 3, 2 * np_ + 5), (0, 3), (total - 2, 2), (9 * np_ - 1, 1)):
            got = srv.read_db_items(bits, first, n)
            assert_bytes(got, packed(O, pts[first:first + n], bits), f"{form}, {bits} bits, items [{first}, +{n})", 1024 * bits)
    assert srv.read_db_items(8, 5, 0).size == 0
    srv.close()


def test_widths_at_p_db_2_15(sa, SV, oracle):
    """p_db = 2^15 (values up to 15 bits, the centred lift's upper half in use): widths 15, 16 and 64, the whole database and a sub-range"""
    O = oracle
    po, pg, s = base_params(sa, O, 4, 3, t_gsw=8, p_db=1 << 15)
    total, np_ = s.dim0 * s.num_per, s.num_per
    pts = plain_db(O, po, 33)
    assert pts.max() >= 1 << 14, "the upper half of the plaintext range is exercised"
    srv = sa.Server(pg)
    srv.gen_db(33)
    assert sa.db_items_bytes(pg, 15, 1) == 15360
    for bits in (15, 16, 64):
        assert_bytes(srv.read_db_items(bits), packed(O, pts, bits), f"{bits} bits, whole database", 1024 * bits)
        first, n = np_ + 3, 2 * np_ + 5
        assert_bytes(srv.read_db_items(bits, first, n), packed(O, pts[first:first + n], bits), f"{bits} bits, items [{first}, +{n})", 1024 * bits)
    with pytest.raises(RuntimeError, match="coeff_bits"):
        srv.read_db_items(14)
    srv.close()


# ---- 3. after updates, by id ------------------------------------------------------------------------------------------------------
def test_after_updates_by_id(sa, SV, oracle):
    """limb planes, a scattered update: read_db_items_at of the updated ids and untouched neighbours (duplicates, any order) gives the new and the old
    plaintexts; the full export is the packer's bytes of the updated database"""
    O = oracle
    po, pg, s = base_params(sa, O, 6, 6, **KW66)
    total = s.dim0 * s.num_per
    now = plain_db(O, po, 21).copy()
    srv = sa.Server(pg)
    srv.gen_db(21)
    srv.set_db_format(SV.DB_LIMBS)
    ids = scattered_ids(s)
    new = np.stack([O.db_item(po, 99, i) for i in ids])
    srv.update_db_items(O.pack_items(new, 8), 8, ids)
    now[ids] = new.reshape(len(ids), -1)
    ask = ids + [1, ids[2] + 1, 10 * s.num_per + 4, (33 ^ 32) * s.num_per + 41, total - 2]
    ask = ask[::-1] + [ids[3], 1, ids[3]]  # unsorted, with duplicates
    got = srv.read_db_items_at(8, ask)
    assert_bytes(got, packed(O, now[ask], 8), "read_db_items_at after the update", 8192)
    assert_bytes(srv.read_db_items_at(13, ask[:7]), packed(O, now[ask[:7]], 13), "read_db_items_at, 13 bits", 1024 * 13)
    assert srv.read_db_items_at(8, []).size == 0
    assert_bytes(srv.read_db_items(8), packed(O, now, 8), "full export of the updated database", 8192)
    assert srv.db_format() == SV.DB_LIMBS
    srv.close()


# ---- 4. narrow, packed-only and plain layouts -------------------------------------------------------------------------------------
@pytest.mark.parametrize("nu1,nu2,kw,limbs", [
    (6, 3, dict(t_gsw=8), True),   # the 1-wave narrow form (16 columns)
    (6, 4, dict(t_gsw=8), True),   # 2 waves
    (6, 5, dict(t_gsw=8), True),   # 4 waves
    (4, 3, dict(t_gsw=8), False),  # packed, a tile of 16 columns x 4 slots
    (3, 2, dict(t_gsw=4), False),  # packed, first dimension 8: one group of rows
    (2, 2, dict(t_gsw=4), False),  # the plain layout (first dimension 4)
])
def test_narrow_and_small_geometries(sa, SV, oracle, opts, nu1, nu2, kw, limbs):
    O = oracle
    po, pg, s = base_params(sa, O, nu1, nu2, **kw)
    pts = plain_db(O, po, 17)
    want = packed(O, pts, 8)
    srv = sa.Server(pg)
    srv.gen_db(17)
    assert_bytes(srv.read_db_items(8), want, f"({nu1}, {nu2}) packed: full export", 8192)
    if limbs:
        opts(sweep_narrow=1)
        srv.set_db_format(SV.DB_LIMBS)
        assert_bytes(srv.read_db_items(8), want, f"({nu1}, {nu2}) limb planes: full export", 8192)
        assert srv.db_format() == SV.DB_LIMBS
    total = s.dim0 * s.num_per
    ask = [total - 1, 0, total // 2, 1, 0]
    assert_bytes(srv.read_db_items_at(64, ask), packed(O, pts[ask], 64), f"({nu1}, {nu2}): by id, raw words", 65536)
    srv.close()


# ---- 5. shards ------------------------------------------------------------------------------------------------------------------------
def test_shards_fill_one_buffer(sa, SV, oracle):
    """a first dimension of 128 over two servers (one in limb planes): each writes its own items and leaves the other half of the buffer alone, in the range
    form and in the _at form"""
    O = oracle
    po, pg, s = base_params(sa, O, 7, 6, **KW66)
    total, np_ = s.dim0 * s.num_per, s.num_per
    pts = plain_db(O, po, 5)
    want = packed(O, pts, 8)
    shards = [sa.Server(pg, j_begin=0, j_end=64), sa.Server(pg, j_begin=64, j_end=128)]
    for sv in shards:
        sv.gen_db(5)
    shards[1].set_db_format(SV.DB_LIMBS)
    half = want.size // 2
    buf = np.full(want.size, 0xA5, dtype=np.uint8)
    shards[0].read_db_items(8, out=buf)
    assert_bytes(buf[:half], want[:half], "shard 0: its own items", 8192)
    assert (buf[half:] == 0xA5).all(), "shard 0 left the other shard's bytes alone"
    shards[1].read_db_items(8, out=buf)
    assert_bytes(buf, want, "both shards: the whole database", 8192)
    # a range across the shard boundary that starts and ends inside a j row
    first, n = 62 * np_ + 7, 4 * np_ + 9
    buf = np.full(n * 8192, 0xA5, dtype=np.uint8)
    shards[1].read_db_items(8, first, n, out=buf)
    cut = (64 * np_ - first) * 8192
    assert (buf[:cut] == 0xA5).all(), "shard 1 left shard 0's items of the range alone"
    shards[0].read_db_items(8, first, n, out=buf)
    assert_bytes(buf, want[first * 8192:(first + n) * 8192], "a range across the boundary", 8192)
    # by id, from both halves
    ask = [127 * np_ + 63, 3, 64 * np_, 63 * np_ + 63, 100 * np_ + 9, 3, 20 * np_ + 9]
    mine = [i // np_ < 64 for i in ask]
    buf = np.full(len(ask) * 8192, 0xA5, dtype=np.uint8)
    shards[0].read_db_items_at(8, ask, out=buf)
    exp = packed(O, pts[ask], 8).reshape(len(ask), 8192)
    for k, m in enumerate(mine):
        got = buf.reshape(len(ask), 8192)[k]
        assert (got == exp[k]).all() if m else (got == 0xA5).all(), f"shard 0, id {ask[k]}: {'read' if m else 'skipped'}"
    shards[1].read_db_items_at(8, ask, out=buf)
    assert_bytes(buf, exp.reshape(-1), "both shards, by id", 8192)
    for sv in shards:
        sv.close()


# ---- 6. SpiralPack, every form ----------------------------------------------------------------------------------------------------
_PACK_PLAIN = {}


def pack_plain_db(O, po, out_n, seed):
    """[trial][item][2048] plaintext coefficients of the oracle's SpiralPack database"""
    s = O.pack_shape_of(po, out_n)
    key = (po.nu1, po.nu2, out_n, seed)
    if key not in _PACK_PLAIN:
        total = s.dim0 * s.num_per
        pts = np.empty((s.trials, total, N), dtype=np.uint32)
        for i in range(total):
            pts[:, i] = O.pack_db_item(po, out_n, seed, i).reshape(s.trials, N)
        pts.setflags(write=False)
        _PACK_PLAIN[key] = pts
    return _PACK_PLAIN[key]


@pytest.mark.parametrize("nu1,nu2,out_n,forms,option", [
    (7, 7, 1, ("packed", "limbs"), None),              # limb planes, wide
    (7, 5, 1, ("packed", "limbs"), None),              # limb planes, narrow (32 columns)
    (7, 3, 1, ("packed", "limbs"), "pack_pair_blocks"),  # limb planes, the 8-column pair form (512-byte planes)
    (7, 3, 3, ("limbs",), "pack_pair_blocks"),         # 9 trials in pair-blocks, the last one half empty
    (6, 2, 2, ("packed",), None),                      # 4 columns, 4 trials: packed only
    (3, 2, 1, ("packed",), None),                      # the plain layout (first dimension 8)
])
def test_pack_every_form(sa, P, oracle_mt, opts, nu1, nu2, out_n, forms, option):
    """every trial in full, and an _at read across j and j ^ 64 (the limb planes' nibble partners), in every form the geometry has"""
    O = oracle_mt
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    total, np_ = s.dim0 * s.num_per, s.num_per
    pts = pack_plain_db(O, po, out_n, 41)
    owner = sa.PackServer(pg, out_n)
    owner.gen_db(41)
    lane = owner.create_lane()
    assert sa.db_items_bytes(pg, 8, 1, out_n=out_n) == 2048
    if option:
        opts(**{option: 1})
    jx = 64 if s.dim0 > 64 else 1
    ask = [5 * np_ + 3 % np_, (5 ^ jx) * np_ + 3 % np_, total - 1, 0, 5 * np_ + 3 % np_, (s.dim0 - 1) * np_, np_ - 1]
    for form in forms:
        if form == "limbs":
            owner.set_db_format(P.DB_LIMBS)
        fmt = owner.db_format()
        assert fmt == (P.DB_LIMBS if form == "limbs" else P.DB_PACKED)
        for t in range(s.trials):
            assert_bytes(owner.read_db_items(t, 8), packed(O, pts[t], 8), f"{form}: trial {t} in full", 2048)
            reader = lane if t & 1 else owner
            assert_bytes(reader.read_db_items_at(t, 8, ask), packed(O, pts[t][ask], 8), f"{form}: trial {t} by id", 2048)
        first, n = np_ + 3, min(total - np_ - 3, 2 * np_ + 5)
        assert_bytes(lane.read_db_items(s.trials - 1, 11, first, n), packed(O, pts[-1][first:first + n], 11), f"{form}: a sub-range at 11 bits, through a lane", 256 * 11)
        assert owner.db_format() == fmt
    with pytest.raises(RuntimeError, match="trial"):
        owner.read_db_items(s.trials, 8)
    lane.close()
    owner.close()
    if s.trials > 1:
        half = sa.PackServer(pg, out_n, trial0=1, trial1=2)
        half.gen_db(41)
        assert_bytes(half.read_db_items(1, 8), packed(O, pts[1], 8), "a trial-sharded server: its own trial", 2048)
        with pytest.raises(RuntimeError, match="trial"):
            half.read_db_items(0, 8)
        with pytest.raises(RuntimeError, match="trial"):
            half.read_db_items_at(2, 8, [0])
        half.close()


# ---- 7. round trip the other way --------------------------------------------------------------------------------------------------
def test_round_trip_base(sa, SV, oracle):
    """a second server that loads the export holds the same image, word for word"""
    O = oracle
    po, pg, s = base_params(sa, O, 6, 6, **KW66)
    a, b = sa.Server(pg), sa.Server(pg)
    a.gen_db(21)
    ids = scattered_ids(s)
    a.update_db_items(O.pack_items(np.stack([O.db_item(po, 98, i) for i in ids]), 8), 8, ids)
    a.set_db_format(SV.DB_LIMBS)
    b.load_db_items(a.read_db_items(8), 8)
    assert_eq(b.read_db_slots(0, N), a.read_db_slots(0, N), "the reloaded export")
    a.close()
    b.close()


def test_round_trip_pack(sa, P, oracle_mt):
    """SpiralPack: a second server loads each trial's export; both servers' lanes give the same answer_batch responses"""
    O = oracle_mt
    nu1, nu2, out_n = 6, 2, 2
    po, pg = O.make_params(nu1, nu2), sa.make_params(nu1, nu2)
    s = O.pack_shape_of(po, out_n)
    a, b = sa.PackServer(pg, out_n), sa.PackServer(pg, out_n)
    a.gen_db(41)
    for t in range(s.trials):
        b.load_db_items(t, a.read_db_items(t, 8), 8)
    outs = []
    for owner in (a, b):
        servers = [owner, owner.create_lane()]
        qs = []
        for k, sv in enumerate(servers):
            cl = O.PackClient(po, out_n, seed=100 + 17 * k)
            sv.set_pub_params(*cl.pub_params())
            qs.append(cl.query((37 + 101 * k) % (s.dim0 * s.num_per)))
        out, _ = P.answer_batch(servers, qs, want_packed=True)
        outs.append(out)
        servers[1].close()
    for k in range(2):
        assert_eq(outs[1][k][0], outs[0][k][0], f"lane {k}: response on the reloaded export")
        assert_eq(outs[1][k][1], outs[0][k][1], f"lane {k}: packed ciphertext on the reloaded export")
    a.close()
    b.close()


# ---- 8. failures ------------------------------------------------------------------------------------------------------------------
def test_failures(sa, SV, oracle):
    """what is refused, and that nothing is harmed by it: the output buffer of a call refused before its launch is untouched, the image and the
    server still answer a query with the oracle's answer"""
    O = oracle
    po, pg, s = base_params(sa, O, 6, 6, **KW66)
    total = s.dim0 * s.num_per
    L = sa.lib()
    pts = plain_db(O, po, 21)
    cl = O.Client(po, seed=9)
    pp = cl.pub_params()
    q = cl.query(700)

    def answers(srv, db, what):
        srv.set_pub_params(*pp)
        fin, _, _ = srv.answer(q)
        assert_eq(fin, O.answer(po, q, *pp, db), what)

    def raw_range(srv, buf, bits, first, n):
        return L.spiral_gpu_server_read_db_items(srv.h, buf.ctypes.data_as(C.c_void_p), bits, first, n)

    def raw_at(srv, buf, bits, ids):
        a = np.ascontiguousarray(ids, dtype=np.uint64)
        return L.spiral_gpu_server_read_db_items_at(srv.h, buf.ctypes.data_as(C.c_void_p), bits, a.ctypes.data_as(C.POINTER(C.c_uint64)), len(a))

    empty = sa.Server(pg)
    with pytest.raises(RuntimeError, match="no database loaded"):
        empty.read_db_items(8, 0, 1)
    with pytest.raises(RuntimeError, match="no database loaded"):
        empty.read_db_items_at(8, [0])

    srv = sa.Server(pg)
    srv.gen_db(21)
    db = O.gen_db(po, 21)
    sentinel = np.full(2 * 8192, 0x5A, dtype=np.uint8)
    for bits in (7, 0, 65):  # refused before any launch: the message names coeff_bits, the buffer is untouched
        assert raw_range(srv, sentinel, bits, 0, 2) != 0 and b"coeff_bits" in L.spiral_gpu_last_error(), f"coeff_bits = {bits}, range form"
        assert raw_at(srv, sentinel, bits, [0, 1]) != 0 and b"coeff_bits" in L.spiral_gpu_last_error(), f"coeff_bits = {bits}, _at form"
        with pytest.raises((RuntimeError, ValueError), match="coeff_bits"):
            srv.read_db_items(bits, 0, 2)
    assert raw_range(srv, sentinel, 8, total - 1, 2) != 0 and b"outside" in L.spiral_gpu_last_error(), "a range past the end"
    assert raw_range(srv, sentinel, 8, total + 1, 0) != 0, "a range that starts past the end"
    assert raw_at(srv, sentinel, 8, [3, total]) != 0 and b"outside" in L.spiral_gpu_last_error(), "an id >= the item count"
    assert L.spiral_gpu_server_read_db_items(srv.h, None, 8, 0, 1) != 0 and L.spiral_gpu_server_read_db_items(None, sentinel.ctypes.data_as(C.c_void_p), 8, 0, 1) != 0
    assert L.spiral_gpu_server_read_db_items_at(srv.h, sentinel.ctypes.data_as(C.c_void_p), 8, None, 1) != 0
    assert (sentinel == 0x5A).all(), "a refused call wrote nothing"
    with pytest.raises(RuntimeError, match="outside"):
        srv.read_db_items(8, total - 1, 2)
    with pytest.raises(RuntimeError, match="outside"):
        srv.read_db_items_at(8, [total])
    answers(srv, db, "a query after the refused calls")

    # a lane and a share_db server read the owner's image
    lane = sa.Server(pg, share_db_of=srv)
    other = sa.Server(pg)
    other.share_db(srv)
    for rd, tag in ((lane, "lane"), (other, "share_db server")):
        assert_bytes(rd.read_db_items(8, 130, 70), packed(O, pts[130:200], 8), f"{tag}: a range", 8192)
        assert_bytes(rd.read_db_items_at(8, [total - 1, 5]), packed(O, pts[[total - 1, 5]], 8), f"{tag}: by id", 8192)
    lane.close()
    other.close()

    # not a plaintext image
    for fmt in (SV.DB_PACKED, SV.DB_LIMBS):
        srv.fill_db_random(7)
        if fmt == SV.DB_LIMBS:
            srv.set_db_format(SV.DB_LIMBS)
        with pytest.raises(RuntimeError, match=r"plaintext at item 0 .*coefficient 0 "):
            srv.read_db_items(8)
        with pytest.raises(RuntimeError, match=rf"plaintext at item {total - 3} "):
            srv.read_db_items_at(8, [total - 3, 4])
        with pytest.raises(RuntimeError, match=r"plaintext at item 77 "):
            srv.read_db_items(64, 77, 9)
        assert srv.db_format() == fmt
        answers(srv, srv.read_db_slots(0, N).reshape(-1), "a query on the random image after the failed exports")
    srv.gen_db(21)
    assert_bytes(srv.read_db_items(8, 0, 64), packed(O, pts[:64], 8), "an export after the database is loaded again", 8192)
    answers(srv, db, "a query after everything")
    srv.close()
    empty.close()


def test_pack_failures(sa, P, oracle_mt):
    O = oracle_mt
    po, pg = O.make_params(6, 2), sa.make_params(6, 2)
    s = O.pack_shape_of(po, 2)
    total = s.dim0 * s.num_per
    srv = sa.PackServer(pg, 2)
    with pytest.raises(RuntimeError, match="no database loaded"):
        srv.read_db_items(0, 8)
    srv.fill_db_random(3)
    with pytest.raises(RuntimeError, match=r"plaintext at item 0 "):
        srv.read_db_items(1, 8)
    with pytest.raises(RuntimeError, match=r"plaintext at item 9 "):
        srv.read_db_items_at(1, 8, [9, 2])
    srv.gen_db(41)
    with pytest.raises((RuntimeError, ValueError), match="coeff_bits"):
        srv.read_db_items(0, 7)
    with pytest.raises(RuntimeError, match="outside"):
        srv.read_db_items(0, 8, total - 1, 2)
    with pytest.raises(RuntimeError, match="outside"):
        srv.read_db_items_at(0, 8, [0, total])
    pts = pack_plain_db(O, po, 2, 41)
    assert_bytes(srv.read_db_items(3, 8), packed(O, pts[3], 8), "an export after the failures", 2048)
    srv.close()


# ---- 9. seeded draws --------------------------------------------------------------------------------------------------------------
GEOMS = [(6, 6, dict(t_gsw=8)), (7, 6, dict(t_gsw=8)), (4, 3, dict(t_gsw=8)), (3, 2, dict(t_gsw=4))]


@pytest.mark.parametrize("seed", range(6))
def test_seeded_draws(sa, SV, oracle, opts, seed):
    """a seeded draw of geometry, form, sharding, range or id list, width and staging size: the export equals the packer's bytes"""
    O = oracle
    rng = np.random.default_rng(2000 + seed)
    nu1, nu2, kw = GEOMS[seed % len(GEOMS)]
    po, pg, s = base_params(sa, O, nu1, nu2, **kw)
    total, np_ = s.dim0 * s.num_per, s.num_per
    pts = plain_db(O, po, 5 if (nu1, nu2) == (7, 6) else 21 if (nu1, nu2) == (6, 6) else 17)
    gen_seed = 5 if (nu1, nu2) == (7, 6) else 21 if (nu1, nu2) == (6, 6) else 17
    n_shards = int(rng.integers(1, 3)) if s.dim0 >= 128 else 1
    span = s.dim0 // n_shards
    limbs_ok = s.num_per >= 64 and 64 <= span <= 2048
    bits = int(rng.choice([8, 11, 64]))
    item_bytes = 1024 * bits
    by_id = bool(rng.integers(2))
    if by_id:
        ask = [int(i) for i in rng.integers(0, total, size=int(rng.integers(1, 300)))]
        exp = packed(O, pts[ask], bits)
    else:
        first = int(rng.integers(0, total))
        n = int(rng.integers(1, min(total - first, 600) + 1))
        exp = packed(O, pts[first:first + n], bits)
    opts(db_stage_bytes=int(rng.choice([1, 5 * item_bytes, 100 * item_bytes + 7, 64 << 20])))
    buf = np.full(exp.size, 0xA5, dtype=np.uint8)
    forms = []
    for k in range(n_shards):
        srv = sa.Server(pg, j_begin=k * span, j_end=(k + 1) * span) if n_shards > 1 else sa.Server(pg)
        srv.gen_db(gen_seed)
        form = SV.DB_LIMBS if limbs_ok and rng.integers(2) else SV.DB_PACKED
        forms.append(form)
        if form == SV.DB_LIMBS:
            srv.set_db_format(form)
        if by_id:
            srv.read_db_items_at(bits, ask, out=buf)
        else:
            srv.read_db_items(bits, first, n, out=buf)
        assert srv.db_format() == form
        srv.close()
    what = f"draw {seed}: ({nu1}, {nu2}), {n_shards} shard(s) in forms {forms}, {bits} bits, " + (f"{len(ask)} ids" if by_id else f"items [{first}, +{n})")
    assert_bytes(buf, exp, what, item_bytes)
