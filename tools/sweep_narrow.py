"""The narrow base forms of the batch's shared pass (option sweep_narrow; csrc/sweep_mfma.hip, workgroups of 4, 2, 1 waves per slot) against the per-lane
vector-ALU sweeps they replace, at the three published base parameter sets whose batches do not reach the matrix cores today: 14,100000:spiral and
14,100000:spiralstream (nu 9/5: 32 ciphertexts per slot) and movie:spiralstream (nu 11/3: 8 per slot, direct upload).  fill_db_random databases,
synthetic keys and queries (uniform residues, as bench.py): timing only -- tests/test_gpu_sweep_narrow.py is the proof that the answers are the same.

Per set, legs with the option at 0 and at 1 ALTERNATE in one process on the same servers (default 0,1,0,1), the image back in the PACKED form between
legs.  Per leg and B = 1, 2, 4, 8 lanes, over --reps repetitions (median, min - max):
    ms per batch (run_query_batch, replayed as one hipGraph, between two device events on the lanes' stream) and queries/s from its median,
    the sweep of the batch alone (time_sweep_batch: the shared pass on a LIMBS image, the B per-lane passes on a PACKED one),
    that sweep as a multiple of the same leg's one-query sweep (time_sweep on the image form the leg's batches run on),
and per leg the one-query sweep on the PACKED image and, with the option on, the one-time in-place conversion (wall time of set_db_format).
An option-1 leg converts the image before its first size, so B = 1 is the one-query instance of the matrix-core kernel on the LIMBS image.
The summary compares the option-1 legs with the option-0 legs of the same run, per B: `faster` / `slower` only when the ranges do not overlap.

    python tools/sweep_narrow.py [--sets "14,100000:spiral;movie:spiralstream"] [--legs 0,1,0,1] [--reps 7] [--sizes 1,2,4,8] [--out profiles/sweep_narrow.json]"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# spiral_amd/scheme.py PUBLISHED, as make_params takes them
SETS = {
    "14,100000:spiral": dict(nu1=9, nu2=5, t_gsw=9, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=21, p_db=512),
    "14,100000:spiralstream": dict(nu1=9, nu2=5, t_gsw=4, t_conv=16, t_exp=2, t_exp_right=56, qprime_bits=26, p_db=16384, direct_upload=1),
    "movie:spiralstream": dict(nu1=11, nu2=3, t_gsw=4, t_conv=56, t_exp=2, t_exp_right=56, qprime_bits=27, p_db=32768, direct_upload=1),
}


def stat(v, nd=4):
    return {"median": round(statistics.median(v), nd), "min": round(min(v), nd), "max": round(max(v), nd)}


def verdict(new, old):
    """`new` against `old` (lists of times): faster / slower only when the two ranges do not overlap"""
    if max(new) < min(old):
        return "faster"
    if min(new) > max(old):
        return "slower"
    return "within the spreads"


def run_set(sa, torch, name, kw, legs, sizes, reps):
    SV = sa.server
    pg = sa.make_params(**kw)
    shp = sa.get_shape(pg)
    owner = sa.Server(pg)
    owner.fill_db_random(3)
    lanes = [owner] + [sa.Server(pg, share_db_of=owner) for _ in range(max(sizes) - 1)]
    stream = torch.cuda.Stream()
    rng = np.random.default_rng(1)
    synth = lambda shape: np.stack([rng.integers(0, m, size=shape + (sa.N,), dtype=np.uint64) for m in (sa.P, sa.B)], axis=-2)
    for ln in lanes:
        ln.set_stream(stream.cuda_stream)
        ln.set_pub_params(synth((max(shp.n_left, 1), 2, pg.t_exp)), synth((max(shp.n_right, 1), 2, pg.t_exp_right)), synth((3, 2 * pg.t_conv)), synth((3, 2 * pg.t_conv)))
        ln.set_query(synth((shp.n_query_cts, 2)))
        ln.use_graphs(True)
    sync = lambda: (owner.sync(), torch.cuda.synchronize())

    def batch_ms(b):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        sa.run_query_batch(lanes[:b])
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1)

    out_legs = []
    for opt in legs:
        sa.set_option("sweep_narrow", opt)
        sync()
        if owner.db_format() != SV.DB_PACKED:
            owner.set_db_format(SV.DB_PACKED)  # every leg starts from the packed image (going back never asks the option)
        owner.time_sweep(3)
        one_packed = [owner.time_sweep(5) for _ in range(reps)]
        convert_ms = None
        if opt and sa.has_limb_form(pg):
            sync()
            t0 = time.perf_counter()
            owner.set_db_format(SV.DB_LIMBS)  # what the first batch of two or more would do by itself, timed alone
            convert_ms = (time.perf_counter() - t0) * 1e3
        form = "limbs" if owner.db_format() == SV.DB_LIMBS else "packed"
        owner.time_sweep(3)
        one_leg = [owner.time_sweep(5) for _ in range(reps)]  # the one-query sweep on the form this leg's batches run on
        rows = []
        for b in sizes:
            for _ in range(2):  # warm-up: the capture, first launches
                batch_ms(b)
            ms = [batch_ms(b) for _ in range(reps)]
            sa.time_sweep_batch(lanes[:b], 3)
            sw = [sa.time_sweep_batch(lanes[:b], 5) for _ in range(reps)]
            assert owner.db_format() == (SV.DB_LIMBS if form == "limbs" else SV.DB_PACKED), "the image changed form inside a leg"
            rows.append({"B": b, "ms_per_batch": stat(ms), "queries_per_s": round(b / (statistics.median(ms) * 1e-3), 1), "sweep_ms": stat(sw),
                         "sweep_x_one_query_sweep": round(statistics.median(sw) / statistics.median(one_leg), 3), "_ms": ms, "_sw": sw})
        out_legs.append({"sweep_narrow": opt, "image_form": form, "one_query_sweep_packed_ms": stat(one_packed), "one_query_sweep_this_form_ms": stat(one_leg),
                         "in_place_conversion_wall_ms": convert_ms and round(convert_ms, 1), "batches": rows, "_one_packed": one_packed})
    db_bytes = int(owner.db_device_bytes())
    for ln in lanes[::-1]:
        ln.close()

    # option 1 against option 0 of this run, the legs of each pooled
    summary = []
    off, on = [l for l in out_legs if l["sweep_narrow"] == 0], [l for l in out_legs if l["sweep_narrow"] == 1]
    if off and on:
        pool = lambda ls, b, key: [x for l in ls for r in l["batches"] if r["B"] == b for x in r[key]]
        one = [x for l in off for x in l["_one_packed"]]
        for b in sizes:
            sw1, sw0, ms1, ms0 = pool(on, b, "_sw"), pool(off, b, "_sw"), pool(on, b, "_ms"), pool(off, b, "_ms")
            summary.append({"B": b, "shared_pass_ms": stat(sw1), "per_lane_sweeps_ms": stat(sw0), "B_one_query_sweeps_ms": stat([b * x for x in one]),
                            "shared_pass_vs_per_lane_sweeps": verdict(sw1, sw0), "shared_pass_vs_B_one_query_sweeps": verdict(sw1, [b * x for x in one]),
                            "shared_pass_speedup_median": round(statistics.median(sw0) / statistics.median(sw1), 3),
                            "batch_ms_on": stat(ms1), "batch_ms_off": stat(ms0), "batch_vs_off": verdict(ms1, ms0),
                            "batch_speedup_median": round(statistics.median(ms0) / statistics.median(ms1), 3)})
    for l in out_legs:
        l.pop("_one_packed")
        for r in l["batches"]:
            r.pop("_ms"), r.pop("_sw")
    return {"set": name, "nu1": kw["nu1"], "nu2": kw["nu2"], "ciphertexts_per_slot": 1 << kw["nu2"], "direct_upload": kw.get("direct_upload", 0),
            "device_db_bytes": db_bytes, "legs": out_legs, "option_1_vs_option_0": summary}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sets", default=";".join(SETS), help="parameter sets, separated by ';'")
    ap.add_argument("--legs", default="0,1,0,1", help="values of option sweep_narrow, one leg each, in order")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="1,2,4,8")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    names = [n for n in a.sets.split(";") if n in SETS]
    legs, sizes = [int(x) for x in a.legs.split(",")], [int(x) for x in a.sizes.split(",")]
    if not names or any(x not in (0, 1) for x in legs) or a.reps < 5 or not all(1 <= b <= 8 for b in sizes):
        ap.error("--sets names known sets, --legs takes 0s and 1s, --reps at least 5, --sizes 1 .. 8")
    import torch

    torch.cuda.is_available()
    import spiral_amd as sa

    assert sa.lib().spiral_gpu_device_count() > 0, "this tool times the GPU; there is nothing to time without one"
    res = {"tool": "sweep_narrow", "device": torch.cuda.get_device_name(0), "reps": a.reps, "legs": legs, "sizes": sizes, "sets": []}
    for name in names:
        res["sets"].append(run_set(sa, torch, name, SETS[name], legs, sizes, a.reps))
        print(json.dumps(res["sets"][-1]), flush=True)
        if a.out:  # (after every set: a run that is cut short keeps what it measured)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
    sa.set_option("sweep_narrow", 0)


if __name__ == "__main__":
    main()
