"""The listing of keyed tables on the device, base servers (include/spiral_gpu.h "Listing": Server.kv_scan, kv_scan_at, kv_reconcile).  Expected
listings come from the restated table (tests/kv_restated.py, tests/kv_scan_restated.py); the table each case lists is crafted on the model's side
(tests/kv_scan_cases.py: an empty bucket, a bucket whose only entry is its highest used slot, a full bucket) and asserted there.  Nothing expected
comes from the code under test."""
import ctypes as C

import numpy as np
import pytest

import kv_restated as K
import kv_scan_cases as KC
import kv_scan_restated as KS

pytestmark = pytest.mark.gpu
TK = K.TABLE_KEY


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


def load_size(lay):
    """kv_restated.load_size; one slot per bucket overflows early (two choices, one place each), so a quarter of the capacity there, as for two slots"""
    return lay.capacity // 4 if lay.slots == 1 else K.load_size(lay)


CASES = [  # name, (nu1, nu2, parameters), form, option sweep_narrow, value size, kv_scan_chunk of the several-pass runs
    ("32-V248", (3, 2, dict(t_gsw=4)), "packed", 0, 248, 3),  # 32 slots
    ("32-V3000", (3, 2, dict(t_gsw=4)), "packed", 0, 3000, 3),  # 2 slots
    ("32-V8184", (3, 2, dict(t_gsw=4)), "packed", 0, 8184, 3),  # 1 slot
    ("32-V24", (3, 2, dict(t_gsw=4)), "packed", 0, 24, 3),  # 256 slots: all four waves list, and the header fills polynomial 0 exactly
    ("32-w5-V99", (3, 2, dict(t_gsw=4, p_db=32)), "packed", 0, 99, 3),  # w = 5, 47 slots: tags straddle coefficients
    ("66-limbs-V248", (6, 6, dict(t_gsw=8)), "limbs", 0, 248, 1000),
    ("64-narrow-limbs-V248", (6, 4, dict(t_gsw=8)), "limbs", 1, 248, 250),
]


@pytest.mark.parametrize("name,geom,form,narrow,V,chunk", CASES, ids=[c[0] for c in CASES])
def test_listing_in_every_form(sa, SV, opts, name, geom, form, narrow, V, chunk):
    """kv_load, the hand-filled bucket, the crafted kv_delete; then every listing of tests/kv_scan_cases.py check_listings in the form under test,
    count-only against kv_stats, max_entries = count and count - 1, the refusals of a bad range, a bad id and a missing entries buffer; the same
    listing from a lane, in the other form and back; a tracked fingerprint that a scan leaves alone; a kv_put after a scan and the re-scan that
    shows it; kv_reconcile of the GPU's listing."""
    opts(sweep_narrow=narrow)
    nu1, nu2, kw = geom
    pg = sa.make_params(nu1, nu2, **kw)
    lay = K.layout(int(pg.p_db), nu1, nu2, V)
    w, nb = lay.coeff_bits, lay.buckets
    assert lay.slots == {248: 32, 3000: 2, 8184: 1, 24: 256, 99: 47}[V]
    plan = KC.crafted_table(lay, load_size(lay), V + nu1)
    model = plan["model"]
    srv = sa.Server(pg)
    srv.gen_db(3)  # (a fresh table overwrites every item)
    srv.kv_load(TK, plan["keys"], plan["vals"])
    srv.load_db_items(plan["fill_stream"], w, first_item=plan["fill_bucket"], n_items=1)
    if form == "limbs":
        assert sa.has_limb_form(pg)
        srv.set_db_format(SV.DB_LIMBS)
    fmt = srv.db_format()
    assert srv.kv_delete(TK, plan["gone"], V) == plan["n_gone"]
    assert srv.db_format() == fmt
    KC.assert_eq(srv.read_db_items(w).reshape(nb, -1), model.stream(), f"{name}: the image is the crafted table")
    lane = sa.Server(pg, share_db_of=srv)
    KC.check_listings(sa, opts, srv, plan, V, name, chunk)
    assert srv.db_format() == fmt, "a scan converts nothing"
    KC.check_counts_and_overflow(sa, srv, sa.lib().spiral_gpu_server_kv_scan, plan, V, name)
    whole = KS.listing(model)
    for values in (False, True):
        KC.check_scan(lane.kv_scan(V, values=values), whole, values, f"{name}: from a lane")
    KC.check_scan(lane.kv_scan_at(V, [plan["full"], plan["empty"], plan["last"], plan["full"]]), KS.listing_at(model, [plan["full"], plan["empty"], plan["last"], plan["full"]]), True,
                  f"{name}: kv_scan_at from a lane")
    if sa.has_limb_form(pg):
        other = SV.DB_PACKED if fmt == SV.DB_LIMBS else SV.DB_LIMBS
        srv.set_db_format(other)
        KC.check_scan(srv.kv_scan(V), whole, True, f"{name}: in the other form")
        srv.set_db_format(fmt)
        KC.check_scan(srv.kv_scan(V), whole, True, f"{name}: back in the form under test")
    # a tracked fingerprint is untouched by a scan
    srv.fingerprint_track(KC.FP_KEY)
    before = srv.fingerprint_tracked()
    assert before[0] == sa.fingerprint_host(KC.FP_KEY, int(pg.p_db), model.stream().reshape(-1), w)
    srv.kv_scan(V)
    lane.kv_scan_at(V, [0, nb - 1])
    assert srv.fingerprint_tracked() == before, "a scan leaves the tracked fingerprint and its update count alone"
    # a put after a scan (the probe reuses the scan's workspace), and the re-scan that shows it
    new = model.fits(K.key_set(6, load_size(lay) + 700_000))
    assert new, "the table has room for a new key"
    new_vals = np.random.default_rng(5).integers(0, 256, size=(len(new), V), dtype=np.uint8)
    model.put(new, new_vals)
    srv.kv_put(TK, new, new_vals)
    KC.check_scan(srv.kv_scan(V), KS.listing(model), True, f"{name}: after a kv_put")
    got_v, got_f = lane.kv_get(TK, new, V)
    assert (got_f != 0).all() and (got_v == new_vals).all()
    plan["stored"], plan["kept"] = plan["stored"] + new, plan["kept"] + new
    KC.check_reconcile(sa, pg, srv, plan, V, name)
    lane.close()
    srv.close()


def hip_runtime():
    """the HIP runtime this process already has loaded (torch's, which the library shares)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def test_refused_inside_a_capture(sa):
    """kv_scan and kv_scan_at are refused while the server's stream is being captured, on both kinds of server; a refused call writes nothing and
    the server still lists afterwards"""
    L, hip = sa.lib(), hip_runtime()
    ids = np.arange(4, dtype=np.uint64)
    for srv, scan, scan_at in ((sa.Server(sa.make_params(3, 2, t_gsw=4)), L.spiral_gpu_server_kv_scan, L.spiral_gpu_server_kv_scan_at),
                               (sa.PackServer(sa.make_params(4, 2), 2), L.spiral_gpu_pack_server_kv_scan, L.spiral_gpu_pack_server_kv_scan_at)):
        srv.kv_load(TK, K.key_set(8), np.zeros((8, 248), dtype=np.uint8))
        assert len(srv.kv_scan(248)) == 8
        st, n = C.c_void_p(), C.c_uint64(77)
        buf = np.full(16 * 8 + 8 * 248, 0xEE, dtype=np.uint8)
        ent, val = buf[:128].ctypes.data_as(C.c_void_p), buf[128:].ctypes.data_as(C.c_void_p)
        assert hip.hipStreamCreate(C.byref(st)) == 0
        srv.set_stream(st.value)
        assert hip.hipStreamBeginCapture(st, 2) == 0  # (hipStreamCaptureModeRelaxed)
        try:
            assert scan(srv.h, 248, 0, 4, ent, val, 8, C.byref(n)) != 0 and b"kv_scan cannot be called while the server's stream is being captured" in L.spiral_gpu_last_error()
            assert scan_at(srv.h, 248, ids.ctypes.data_as(C.c_void_p), 4, ent, val, 8, C.byref(n)) != 0
            assert b"kv_scan_at cannot be called while the server's stream is being captured" in L.spiral_gpu_last_error()
        finally:
            g = C.c_void_p()
            assert hip.hipStreamEndCapture(st, C.byref(g)) == 0
            if g.value:
                hip.hipGraphDestroy(g)
        srv.set_stream(0)
        hip.hipStreamDestroy(st)
        assert n.value == 77 and (buf == 0xEE).all(), "a refused call wrote nothing"
        assert len(srv.kv_scan(248)) == 8, "and the server still lists"
        srv.close()


def test_refusals(sa):
    """a j-shard and a column shard refuse by name; an image after fill_db_random fails the call naming the lowest bucket (kv_scan_at: the lowest
    position) and a coefficient, from the owner and from a lane, and nothing is written"""
    for tag_, geom, make in [("j-shard", (7, 6), lambda p: sa.Server(p, j_begin=0, j_end=64)), ("column shard", (5, 5), lambda p: sa.Server(p, col_rank=0, col_ranks=2))]:
        p2 = sa.make_params(*geom, t_gsw=8)
        shard = make(p2)
        shard.gen_db(1)
        with pytest.raises(sa.SpiralGpuError, match=f"kv_scan: this server is a {tag_}"):
            shard.kv_scan(248)
        with pytest.raises(sa.SpiralGpuError, match=f"kv_scan_at: this server is a {tag_}"):
            shard.kv_scan_at(248, [1, 2])
        shard.close()
    pg = sa.make_params(3, 2, t_gsw=4)
    V = 248
    srv = sa.Server(pg)
    with pytest.raises(sa.SpiralGpuError, match="no database loaded"):
        srv.kv_scan(V)
    srv.fill_db_random(5)
    lane = sa.Server(pg, share_db_of=srv)
    from spiral_amd import _lib

    for who, first in ((srv, 0), (lane, 5)):
        ent = np.frombuffer(np.full(16 * 64, 0xEE, dtype=np.uint8), dtype=_lib.KV_ENTRY_DTYPE).copy()
        val = np.full((64, V), 0xEE, dtype=np.uint8)
        with pytest.raises(sa.SpiralGpuError, match=rf"kv_scan: the image holds no keyed table at bucket {first} \(polynomial 0, coefficient \d+"):
            who.kv_scan(V, first, None, True, 64, out_entries=ent, out_values=val)
        with pytest.raises(sa.SpiralGpuError, match=rf"kv_scan: the image holds no keyed table at bucket {first} \(polynomial 0, coefficient \d+"):
            who.kv_scan(V, first)  # (the count-only call fails the same way)
        with pytest.raises(sa.SpiralGpuError, match=rf"kv_scan_at: the image holds no keyed table at position 0 of the list, bucket 9 \(polynomial 0, coefficient \d+"):
            who.kv_scan_at(V, [9, 3, 9, first], True, 64, out_entries=ent, out_values=val)
        assert (ent.view(np.uint8) == 0xEE).all() and (val == 0xEE).all(), "a failed call writes nothing"
    lane.close()
    srv.close()
