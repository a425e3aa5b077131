"""Batched SpiralPack answers at configs[4] (SpiralPack 2^18 x 30 KB: nu1=10, nu2=8, out_n=4, 16 trial images, ~60 GB on the device, generated
there): for B = 1, 2, 4, 8 lanes of one owner, the time per answer_batch call, queries/s, and the batched first-dimension sweep alone (ms, algorithmic
GB/s, fraction of the 8 TB/s HBM peak) -- beside the single-query answer on the packed image (the path bench.py --workload pack times).

    python tools/pack_batch.py [--reps 5] [--sizes 1,2,4,8] [--out profiles/pack_batch.json]

Prints one JSON line (and writes it to --out).  Synthetic keys and queries (uniform residues, as bench.py): timing only."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBPS = 8000.0


def synth(rng, sa, shape):
    return np.stack([rng.integers(0, m, size=shape + (sa.N,), dtype=np.uint64) for m in (sa.P, sa.B)], axis=-2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,2,4,8")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    torch.cuda.is_available()
    import spiral_amd as sa

    P = sys.modules["spiral_amd.pack"]
    sizes = [int(x) for x in args.sizes.split(",")]
    out_n = 4
    pg = sa.make_params(10, 8, t_gsw=8, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=20, p_db=256)
    shp = sa.get_pack_shape(pg, out_n)
    owner = sa.PackServer(pg, out_n)
    owner.gen_db(2024)
    servers = [owner] + [owner.create_lane() for _ in range(max(sizes) - 1)]
    rng = np.random.default_rng(1)
    qs = []
    for srv in servers:
        srv.set_pub_params(synth(rng, sa, (shp.n_left, 2, pg.t_exp)), synth(rng, sa, (shp.n_right, 2, pg.t_exp_right)), synth(rng, sa, (2, 2 * pg.t_conv)),
                           synth(rng, sa, (out_n, out_n + 1, pg.t_conv)))
        qs.append(synth(rng, sa, (shp.n_query_cts, 2)))
    sweep_bytes = shp.trials * owner.sweep_bytes()  # algorithmic bytes of one pass over every trial image

    # the single-query path on the packed image first (what bench.py --workload pack measures)
    owner.answer(qs[0], want_packed=False)
    st = []
    t0 = time.perf_counter()
    for _ in range(args.reps):
        st.append(owner.answer(qs[0], want_packed=False)[2])
    single_ms = (time.perf_counter() - t0) * 1e3 / args.reps
    single_sweep_ms = float(np.mean([u["sweep_kernels_us"] for u in st])) / 1e3
    assert owner.db_format() == P.DB_PACKED
    rows = []
    for b in sizes:
        lanes, q = servers[:b], qs[:b]
        P.answer_batch(lanes, q)  # warm-up (the first batch of two or more converts the image in place)
        stages = []
        t0 = time.perf_counter()
        for _ in range(args.reps):
            stages.append(P.answer_batch(lanes, q)[1])
        ms = (time.perf_counter() - t0) * 1e3 / args.reps
        sw = P.time_sweep_batch(lanes, args.reps)
        gbs = sweep_bytes / (sw * 1e-3) / 1e9
        rows.append({"B": b, "ms_per_batch": round(ms, 3), "queries_per_s": round(b / (ms * 1e-3), 1), "sweep_ms": round(sw, 3), "sweep_algorithmic_GBps": round(gbs, 1),
                     "sweep_frac_of_peak": round(gbs / HBM_PEAK_GBPS, 4), "image_form": "limbs" if owner.db_format() == P.DB_LIMBS else "packed",
                     "stages_us": {k: round(float(np.mean([s[k] for s in stages])), 1) for k in stages[0]}})
    # and the single answer again, now on the limb-plane image (the one-query instance of the batched kernel)
    t0 = time.perf_counter()
    st2 = [owner.answer(qs[0], want_packed=False)[2] for _ in range(args.reps)]
    single_limbs_ms = (time.perf_counter() - t0) * 1e3 / args.reps
    out = {"tool": "pack_batch", "config": "configs[4]: SpiralPack nu1=10, nu2=8, out_n=4, 16 trial images generated on the device", "reps": args.reps,
           "sweep_algorithmic_bytes": int(sweep_bytes),
           "single_packed": {"ms_per_query": round(single_ms, 3), "queries_per_s": round(1e3 / single_ms, 1), "sweep_ms": round(single_sweep_ms, 3),
                             "sweep_frac_of_peak": round(sweep_bytes / (single_sweep_ms * 1e-3) / 1e9 / HBM_PEAK_GBPS, 4)},
           "single_limbs": {"ms_per_query": round(single_limbs_ms, 3), "sweep_ms": round(float(np.mean([u["sweep_kernels_us"] for u in st2])) / 1e3, 3)},
           "batches": rows}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for srv in servers:
        srv.close()


if __name__ == "__main__":
    main()
