"""Batched SpiralPack answers at configs[4] (SpiralPack 2^18 x 30 KB: nu1=10, nu2=8, out_n=4, 16 trial images, ~60 GB on the device, generated
there) or, --geom pack14, at the parameter selector's spiral-pack pick (2^14 x 1 MB: nu1=10, nu2=4, out_n=12, 144 trial images of 16 ciphertexts per
slot, 33.8 GB: the narrow form of the shared pass): for B = 1, 2, 4, 8 lanes of one owner, the time per answer_batch call, queries/s, and the batched
first-dimension sweep alone (time_sweep_batch: ms, algorithmic GB/s, fraction of the 8 TB/s HBM peak) -- beside the single-query answer on the packed
image (the path bench.py --workload pack times) and on the limb-plane image.  Per row the median and the min-to-max spread of the repetitions' device
times, and the one-time in-place conversion of the image.  Every row also carries the batch's stage times (median and spread per stage) and the form it
took: option pack_batch_lanes as the library had it (--lanes sets it; null for a build that has no such option) and whether the batch ran as one
lane-aware launch sequence (the counter pack_lane_batches moved), and which form of the sweep ran (sweep_form: pair / narrow / wide on the limb-plane
image, per-lane on the packed one) with the shared pass as a multiple of the same leg's one-query sweep1_kernel pass.  --geom stream12 is the selector's
spiralstream-pack pick (nu1=9, nu2=3, out_n=10: 100 trial images of 8 ciphertexts per slot), where the shared pass is the pair form and needs option
pack_pair_blocks: --pair-blocks 0|1 sets it, and a list (--pair-blocks 0,1,0,1) runs that many legs in ONE process on the same servers, the image
back in the packed form between them.

    python tools/pack_batch.py [--geom config5|pack14|stream12] [--reps 5] [--sizes 1,2,4,8] [--lanes N] [--pair-blocks 0|1|0,1,0,1] [--out profiles/pack_batch.json]

Prints one JSON line (and writes it to --out); with several legs the line is {"legs": [one such object per leg]}.  Synthetic keys and queries (uniform residues, as bench.py): timing only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBPS = 8000.0
# name: (nu1, nu2, out_n, params, what it is)
GEOMS = {
    "config5": (10, 8, 4, dict(t_gsw=8, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=20, p_db=256),
                "configs[4]: SpiralPack nu1=10, nu2=8, out_n=4, 16 trial images generated on the device"),
    "pack14": (10, 4, 12, dict(t_gsw=16, t_conv=4, t_exp=56, t_exp_right=56, qprime_bits=23, p_db=1024),
               "scheme --select 14,1000000 --variant spiral-pack (first pick): nu1=10, nu2=4, out_n=12, 144 trial images of 16 ciphertexts per slot"),
    "stream12": (9, 3, 10, dict(t_gsw=3, t_conv=56, t_exp=56, t_exp_right=56, qprime_bits=32, p_db=1 << 20, direct_upload=1),
                 "scheme --select 12,4000000 --variant spiralstream-pack (first pick): nu1=9, nu2=3, out_n=10, 100 trial images of 8 ciphertexts per slot"),
}


def synth(rng, sa, shape):
    return np.stack([rng.integers(0, m, size=shape + (sa.N,), dtype=np.uint64) for m in (sa.P, sa.B)], axis=-2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geom", choices=sorted(GEOMS), default="config5")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,2,4,8")
    ap.add_argument("--lanes", type=int, default=None, help="option pack_batch_lanes (default: the library's)")
    ap.add_argument("--pair-blocks", default=None, help="option pack_pair_blocks: 0 or 1, or a list of them = legs in one process (default: the library's)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    legs = [None] if args.pair_blocks is None else [int(x) for x in args.pair_blocks.split(",")]
    if any(x not in (None, 0, 1) for x in legs):
        ap.error("--pair-blocks takes 0 or 1, or a comma-separated list of them")
    import torch

    torch.cuda.is_available()
    import spiral_amd as sa

    P = sys.modules["spiral_amd.pack"]

    def option(name):  # None: a build without the option (SPIRAL_LIB = an earlier build)
        try:
            return sa.get_option(name)
        except sa.SpiralGpuError:
            return None

    if args.lanes is not None:
        sa.set_option("pack_batch_lanes", args.lanes)
    sizes = [int(x) for x in args.sizes.split(",")]
    nu1, nu2, out_n, kw, what = GEOMS[args.geom]
    pg = sa.make_params(nu1, nu2, **kw)
    shp = sa.get_pack_shape(pg, out_n)
    owner = sa.PackServer(pg, out_n)
    owner.gen_db(2024)
    servers = [owner] + [owner.create_lane() for _ in range(max(sizes) - 1)]
    rng = np.random.default_rng(1)
    qs = []
    for srv in servers:
        srv.set_pub_params(synth(rng, sa, (max(shp.n_left, 1), 2, pg.t_exp)), synth(rng, sa, (max(shp.n_right, 1), 2, pg.t_exp_right)), synth(rng, sa, (2, 2 * pg.t_conv)),
                           synth(rng, sa, (out_n, out_n + 1, pg.t_conv)))
        qs.append(synth(rng, sa, (shp.n_query_cts, 2)))
    sweep_bytes = shp.trials * owner.sweep_bytes()  # algorithmic bytes of one pass over every trial image

    def run_leg(pair):
        if pair is not None:
            sa.set_option("pack_pair_blocks", pair)
        if owner.db_format() != P.DB_PACKED:
            owner.set_db_format(P.DB_PACKED)  # every leg starts from the packed image (going back never asks the option)
        # the single-query path on the packed image first (what bench.py --workload pack measures)
        owner.answer(qs[0], want_packed=False)
        st = []
        t0 = time.perf_counter()
        for _ in range(args.reps):
            st.append(owner.answer(qs[0], want_packed=False)[2])
        single_ms = (time.perf_counter() - t0) * 1e3 / args.reps
        single_sweep_ms = float(np.mean([u["sweep_kernels_us"] for u in st])) / 1e3
        assert owner.db_format() == P.DB_PACKED
        sweep_form = lambda: "per-lane" if owner.db_format() == P.DB_PACKED else "pair" if shp.num_per == 8 else "narrow" if shp.num_per < 128 else "wide"
        med = lambda v: float(np.median(v))
        spread = lambda v: [round(float(min(v)), 1), round(float(max(v)), 1)]
        rows, convert_ms = [], None
        for b in sizes:
            lanes, q = servers[:b], qs[:b]
            if b >= 2 and owner.db_format() == P.DB_PACKED and P.has_limb_form(pg, out_n):
                t0 = time.perf_counter()
                owner.set_db_format(P.DB_LIMBS)  # what the first batch of two or more would do by itself: the one-time in-place conversion, timed alone
                convert_ms = (time.perf_counter() - t0) * 1e3
            P.answer_batch(lanes, q)  # warm-up
            stages = []
            counted = option("pack_lane_batches")
            t0 = time.perf_counter()
            for _ in range(args.reps):
                stages.append(P.answer_batch(lanes, q)[1])
            ms = (time.perf_counter() - t0) * 1e3 / args.reps
            lane_form = counted is not None and option("pack_lane_batches") - counted == args.reps
            form = "limbs" if owner.db_format() == P.DB_LIMBS else "packed"  # (the form the timed batches ran on)
            if owner.db_format() == P.DB_PACKED and P.has_limb_form(pg, out_n):  # (time_sweep_batch converts a covered image, whatever the lane count)
                t0 = time.perf_counter()
                owner.set_db_format(P.DB_LIMBS)
                convert_ms = (time.perf_counter() - t0) * 1e3
            sws = [P.time_sweep_batch(lanes, 3) for _ in range(args.reps)]
            swept = sweep_form()  # (the form time_sweep_batch ran)
            sw = med(sws)
            gbs = sweep_bytes / (sw * 1e-3) / 1e9
            dev = [s["total_us"] for s in stages]
            rows.append({"B": b, "ms_per_batch": round(ms, 3), "queries_per_s": round(b / (ms * 1e-3), 1), "device_us_median": round(med(dev), 1), "device_us_spread": spread(dev),
                         "device_queries_per_s": round(b / (med(dev) * 1e-6), 1), "sweep_ms": round(sw, 3), "sweep_ms_spread": [round(min(sws), 3), round(max(sws), 3)],
                         "sweep_algorithmic_GBps": round(gbs, 1),
                         "sweep_frac_of_peak": round(gbs / HBM_PEAK_GBPS, 4), "image_form": form, "sweep_image_form": "limbs" if owner.db_format() == P.DB_LIMBS else "packed",
                         "stages_us": {k: round(float(np.mean([s[k] for s in stages])), 1) for k in stages[0]},
                         "stages_us_median": {k: round(med([s[k] for s in stages]), 1) for k in stages[0]},
                         "stages_us_spread": {k: spread([s[k] for s in stages]) for k in stages[0]},
                         "sweep_form": swept, "sweep_x_one_query_pass": round(sw / single_sweep_ms, 3),
                         "pack_batch_lanes": option("pack_batch_lanes"), "lane_form": lane_form, "pack_pair_blocks": option("pack_pair_blocks")})
        # and the single answer again, now on the limb-plane image (the one-query instance of the batched kernel)
        t0 = time.perf_counter()
        st2 = [owner.answer(qs[0], want_packed=False)[2] for _ in range(args.reps)]
        single_limbs_ms = (time.perf_counter() - t0) * 1e3 / args.reps
        dev1, dev2 = [u["total_us"] for u in st], [u["total_us"] for u in st2]
        out = {"tool": "pack_batch", "config": what, "reps": args.reps, "library": os.environ.get("SPIRAL_LIB", "product"), "pack_batch_lanes": option("pack_batch_lanes"),
               "pack_pair_blocks": option("pack_pair_blocks"), "has_limb_form": P.has_limb_form(pg, out_n),
               "sweep_algorithmic_bytes": int(sweep_bytes), "device_db_bytes": owner.db_device_bytes(), "in_place_conversion_ms": convert_ms and round(convert_ms, 1),
               "single_packed_device_us": {"median": round(med(dev1), 1), "spread": spread(dev1), "sweep_us_spread": spread([u["sweep_kernels_us"] for u in st])},
               "single_limbs_device_us": {"median": round(med(dev2), 1), "spread": spread(dev2), "sweep_us_spread": spread([u["sweep_kernels_us"] for u in st2]),
                                          "image_form": "limbs" if owner.db_format() == P.DB_LIMBS else "packed"},
               "single_packed": {"ms_per_query": round(single_ms, 3), "queries_per_s": round(1e3 / single_ms, 1), "sweep_ms": round(single_sweep_ms, 3),
                                 "sweep_frac_of_peak": round(sweep_bytes / (single_sweep_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)},
               "single_limbs": {"ms_per_query": round(single_limbs_ms, 3), "sweep_ms": round(float(np.mean([u["sweep_kernels_us"] for u in st2])) / 1e3, 3)},
               "batches": rows}
        return out

    results = [run_leg(x) for x in legs]
    out = results[0] if len(results) == 1 else {"tool": "pack_batch", "config": what, "legs": results}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for srv in servers:
        srv.close()


if __name__ == "__main__":
    main()
