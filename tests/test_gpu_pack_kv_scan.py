"""The listing of keyed tables on the device, SpiralPack servers (include/spiral_gpu.h "Listing": PackServer.kv_scan, kv_scan_at, kv_reconcile): the
headers come from trial image 0, the entries' values span the trial images.  Expected listings come from the restated table (tests/kv_restated.py,
tests/pack_kv_restated.py, tests/kv_scan_restated.py); the table each case lists is crafted on the model's side (tests/kv_scan_cases.py) and asserted
there.  Nothing expected comes from the code under test."""
import sys

import numpy as np
import pytest

import kv_restated as K
import kv_scan_cases as KC
import kv_scan_restated as KS
import pack_kv_restated as PK

pytestmark = pytest.mark.gpu
TK = PK.TABLE_KEY


@pytest.fixture(scope="module")
def sa():
    # torch first: it ships its own HIP runtime and the two must not be initialised in the opposite order
    import torch

    torch.cuda.is_available()
    import spiral_amd

    assert spiral_amd.lib().spiral_gpu_device_count() > 0, "GPU tests need a device"
    return spiral_amd


@pytest.fixture(scope="module")
def P(sa):
    return sys.modules["spiral_amd.pack"]


CASES = [  # name, (nu1, nu2, out_n, parameters), form, option pack_pair_blocks, value size, kv_scan_chunk of the several-pass runs
    ("422-packed-V248", (4, 2, 2, {}), "packed", 0, 248, 3),
    ("422-packed-V3000", (4, 2, 2, {}), "packed", 0, 3000, 3),  # 2 slots, values across polynomials 0-1 and 1-2
    ("742-limbs-V248", (7, 4, 2, {}), "limbs", 0, 248, 500),
    ("733-w5-packed-V99", (7, 3, 3, dict(p_db=32)), "packed", 0, 99, 250),  # w = 5, 107 slots: tags straddle coefficients, values straddle trials
    ("733-w5-pairs-V5000", (7, 3, 3, dict(p_db=32)), "limbs", 1, 5000, 250),  # the pair form; 2 slots whose values span 4 and 5 trial images
]


@pytest.mark.parametrize("name,geom,form,pairs,V,chunk", CASES, ids=[c[0] for c in CASES])
def test_listing_in_every_form(sa, P, opts, name, geom, form, pairs, V, chunk):
    """the base test's checks on a SpiralPack server: kv_load, the hand-filled bucket (one item of every trial), the crafted kv_delete; every listing
    of check_listings, with kv_scan_chunk forcing several passes; counts, overflow and refusals; a lane, the other form and back, a tracked
    fingerprint, a kv_put and its re-scan, kv_reconcile.  Values span several trial images."""
    opts(pack_pair_blocks=pairs)
    nu1, nu2, out_n, kw = geom
    pg = sa.make_params(nu1, nu2, **kw)
    lay = PK.layout(int(pg.p_db), nu1, nu2, out_n, V)
    w, nb, trials = lay.coeff_bits, lay.buckets, out_n * out_n
    plan = KC.crafted_table(lay, PK.load_size(lay), V + nu1)
    model = plan["model"]
    whole = KS.listing(model)
    spans = [PK.value_polys(lay, int(s)) for s in np.unique(whole[2])]
    assert max(len(r) for r in spans) > 1 and any(r[0] > 0 for r in spans), "values span several trial images, and lie beyond trial 0"
    srv = sa.PackServer(pg, out_n)
    srv.gen_db(3)  # (a fresh table overwrites every item of every trial)
    srv.kv_load(TK, plan["keys"], plan["vals"])
    for t, st in enumerate(PK.trial_streams(plan["fill_stream"][None, :], lay, out_n)):
        srv.load_db_items(t, st, w, first_item=plan["fill_bucket"], n_items=1)
    if form == "limbs":
        assert P.has_limb_form(pg, out_n)
        srv.set_db_format(P.DB_LIMBS)
    fmt = srv.db_format()
    assert srv.kv_delete(TK, plan["gone"], V) == plan["n_gone"]
    assert srv.db_format() == fmt
    image = np.concatenate([srv.read_db_items(t, w).reshape(nb, -1) for t in range(trials)], axis=1)
    KC.assert_eq(image, model.stream(), f"{name}: the trial images are the crafted table")
    lane = srv.create_lane()
    KC.check_listings(sa, opts, srv, plan, V, name, chunk)
    assert srv.db_format() == fmt, "a scan converts nothing"
    KC.check_counts_and_overflow(sa, srv, sa.lib().spiral_gpu_pack_server_kv_scan, plan, V, name)
    for values in (False, True):
        KC.check_scan(lane.kv_scan(V, values=values), whole, values, f"{name}: from a lane")
    ids = [plan["full"], plan["empty"], plan["last"], plan["full"]]
    KC.check_scan(lane.kv_scan_at(V, ids), KS.listing_at(model, ids), True, f"{name}: kv_scan_at from a lane")
    if P.has_limb_form(pg, out_n):
        other = P.DB_PACKED if fmt == P.DB_LIMBS else P.DB_LIMBS
        srv.set_db_format(other)
        KC.check_scan(srv.kv_scan(V), whole, True, f"{name}: in the other form")
        srv.set_db_format(fmt)
        KC.check_scan(srv.kv_scan(V), whole, True, f"{name}: back in the form under test")
    # a tracked fingerprint is untouched by a scan
    srv.fingerprint_track(KC.FP_KEY)
    before = srv.fingerprint_tracked()
    assert before[0] == sa.fingerprint_host(KC.FP_KEY, int(pg.p_db), model.stream().reshape(-1), w, polys_per_item=trials)
    srv.kv_scan(V)
    lane.kv_scan_at(V, [0, nb - 1])
    assert srv.fingerprint_tracked() == before, "a scan leaves the tracked fingerprint and its update count alone"
    # a put after a scan (the probe reuses the scan's workspace), and the re-scan that shows it
    new = model.fits(K.key_set(6, PK.load_size(lay) + 700_000))
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


def test_refusals(sa, P):
    """a trial-sharded server and its shard lane refuse by name; an image after fill_db_random fails the call naming the lowest bucket (kv_scan_at: the
    lowest position) and a coefficient, from the owner and from a lane, and nothing is written"""
    from spiral_amd import _lib

    out_n, V = 2, 248
    pg = sa.make_params(4, 2)
    shard = sa.PackServer(pg, out_n, trial0=0, trial1=2)
    shard.gen_db(1)
    shard_lane = shard.create_shard_lane()
    for call_ in (lambda: shard.kv_scan(V), lambda: shard.kv_scan_at(V, [1]), lambda: shard_lane.kv_scan(V), lambda: shard_lane.kv_scan_at(V, [1])):
        with pytest.raises(sa.SpiralGpuError, match=r"kv_scan(_at)?: this server is a trial shard \(trials \[0, 2\) of 4\)"):
            call_()
    shard_lane.close()
    shard.close()
    srv = sa.PackServer(pg, out_n)
    srv.fill_db_random(5)
    lane = srv.create_lane()
    for who, first in ((srv, 0), (lane, 5)):
        ent = np.frombuffer(np.full(16 * 64, 0xEE, dtype=np.uint8), dtype=_lib.KV_ENTRY_DTYPE).copy()
        val = np.full((64, V), 0xEE, dtype=np.uint8)
        with pytest.raises(sa.SpiralGpuError, match=rf"kv_scan: the image holds no keyed table at bucket {first} \(polynomial 0, coefficient \d+"):
            who.kv_scan(V, first, None, True, 64, out_entries=ent, out_values=val)
        with pytest.raises(sa.SpiralGpuError, match=rf"kv_scan_at: the image holds no keyed table at position 0 of the list, bucket 9 \(polynomial 0, coefficient \d+"):
            who.kv_scan_at(V, [9, 3, 9, first], True, 64, out_entries=ent, out_values=val)
        assert (ent.view(np.uint8) == 0xEE).all() and (val == 0xEE).all(), "a failed call writes nothing"
    lane.close()
    srv.close()
