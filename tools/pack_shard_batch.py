"""SpiralPack batches on a trial-sharded server: ONE rank's share on one GPU.  A server for trial1 - trial0 = out_n^2 / G of the trial images of
configs[4] (SpiralPack nu1=10, nu2=8, out_n=4: 16 images of 3.75 GiB, so 8 for G = 2 and 4 for G = 4) or, --geom pack14, of the parameter selector's
spiral-pack pick (nu1=10, nu2=4, out_n=12: 144 images of 16 ciphertexts per slot), with its shard lanes.  For B = 1, 2, 4, 8 clients and option
pack_batch_lanes = 0 and 2 it times

  fold:  one fold_trials_batch of B clients         against  B fold_trials in sequence, one per lane
  pack:  one pack_gathered_batch of B clients       against  B pack_gathered in sequence (the root's half; the gathered buffer holds this rank's
                                                             block G times over: valid words, timing only)

The two legs of a pair alternate in one process, --reps repetitions each (default 7), timed with device events on the servers' stream; per leg the
median and the min-to-max spread.  The image is converted to its limb-plane form first where the geometry has one (what the first batch of two would
do), so both legs sweep the same image.  The collective is not run: one GPU has no xGMI peer.

    python tools/pack_shard_batch.py [--geom config5|pack14] [--ranks 2,4] [--sizes 1,2,4,8] [--lanes 0,2] [--reps 7] [--out profiles/pack_shard_batch.json]

Prints one JSON line (and writes it to --out).  Synthetic keys and queries (uniform residues, as bench.py): timing only."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
GEOMS = {
    "config5": (10, 8, 4, dict(t_gsw=8, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=20, p_db=256),
                "configs[4]: SpiralPack nu1=10, nu2=8, out_n=4, 16 trial images generated on the device"),
    "pack14": (10, 4, 12, dict(t_gsw=16, t_conv=4, t_exp=56, t_exp_right=56, qprime_bits=23, p_db=1024),
               "scheme --select 14,1000000 --variant spiral-pack (first pick): nu1=10, nu2=4, out_n=12, 144 trial images of 16 ciphertexts per slot"),
}
CT = 2 * 2048


def synth(rng, sa, shape):
    return np.stack([rng.integers(0, m, size=shape + (sa.N,), dtype=np.uint64) for m in (sa.P, sa.B)], axis=-2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--geom", choices=sorted(GEOMS), default="config5")
    ap.add_argument("--ranks", default="2,4", help="G: the server holds out_n^2 / G trial images")
    ap.add_argument("--sizes", default="1,2,4,8")
    ap.add_argument("--lanes", default="0,2", help="values of option pack_batch_lanes")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    torch.cuda.is_available()
    import spiral_amd as sa
    from spiral_amd import dist as D

    P = sys.modules["spiral_amd.pack"]
    sizes = [int(x) for x in args.sizes.split(",")]
    nu1, nu2, out_n, kw, what = GEOMS[args.geom]
    pg = sa.make_params(nu1, nu2, **kw)
    shp = sa.get_pack_shape(pg, out_n)
    stream = torch.cuda.Stream()
    med = lambda v: round(float(np.median(v)), 1)
    spread = lambda v: [round(float(min(v)), 1), round(float(max(v)), 1)]

    def timed(fn):
        """device microseconds of fn() between two events on the servers' stream"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3

    shares = []
    for G in [int(x) for x in args.ranks.split(",")]:
        cuts = D.pack_trial_cuts(G, shp.trials)
        nt = cuts[1] - cuts[0]
        owner = sa.PackServer(pg, out_n, 0, cuts[0], cuts[1])
        owner.gen_db(2024)
        servers = [owner] + [owner.create_shard_lane() for _ in range(max(sizes) - 1)]
        rng = np.random.default_rng(1)
        qs = []
        for srv in servers:
            srv.set_stream(stream.cuda_stream)
            srv.set_pub_params(synth(rng, sa, (max(shp.n_left, 1), 2, pg.t_exp)), synth(rng, sa, (max(shp.n_right, 1), 2, pg.t_exp_right)),
                               synth(rng, sa, (2, 2 * pg.t_conv)), synth(rng, sa, (out_n, out_n + 1, pg.t_conv)))
            qs.append(synth(rng, sa, (shp.n_query_cts, 2)))
        if P.has_limb_form(pg, out_n):
            owner.set_db_format(P.DB_LIMBS)
        rows = []
        with torch.cuda.stream(stream):
            for B in sizes:
                lanes, q = servers[:B], qs[:B]
                block = D.pack_batch_block_cts(B, cuts)
                mine = torch.zeros(block * CT, dtype=torch.int64, device="cuda")
                alone = [torch.zeros(nt * CT, dtype=torch.int64, device="cuda") for _ in range(B)]
                ordered = [torch.zeros(shp.trials * CT, dtype=torch.int64, device="cuda") for _ in range(B)]
                for lanes_opt in [int(x) for x in args.lanes.split(",")]:
                    sa.set_option("pack_batch_lanes", lanes_opt)
                    counted = sa.get_option("pack_lane_batches")
                    fold_batch = lambda: P.fold_trials_batch(lanes, q, mine.data_ptr())
                    fold_singles = lambda: [sv.fold_trials(x, t.data_ptr()) for sv, x, t in zip(lanes, q, alone)]
                    fold_batch(), fold_singles()  # warm-up
                    torch.cuda.synchronize()
                    t_fold = {"batch": [], "singles": []}
                    for _ in range(args.reps):
                        t_fold["batch"].append(timed(fold_batch))
                        t_fold["singles"].append(timed(fold_singles))
                    lane_form = sa.get_option("pack_lane_batches") - counted == args.reps + 1
                    # the root's half: this rank's block G times over, and each lane's own trial-ordered ciphertexts
                    gathered = mine.repeat(G)
                    for b in range(B):
                        ordered[b].copy_(alone[b].repeat(G)[:shp.trials * CT])
                    torch.cuda.synchronize()
                    pack_batch = lambda: P.pack_gathered_batch(lanes, gathered.data_ptr(), cuts, block)
                    pack_singles = lambda: [sv.pack_gathered(t.data_ptr()) for sv, t in zip(lanes, ordered)]
                    pack_batch(), pack_singles()
                    t_pack = {"batch": [], "singles": []}
                    for _ in range(args.reps):
                        t_pack["batch"].append(timed(pack_batch))
                        t_pack["singles"].append(timed(pack_singles))
                    row = {"B": B, "pack_batch_lanes": lanes_opt, "lane_form": bool(lane_form)}
                    for name, t in (("fold", t_fold), ("pack", t_pack)):
                        row[name] = {k: {"median_us": med(v), "spread_us": spread(v)} for k, v in t.items()}
                        row[name]["batch_over_singles"] = round(float(np.median(t["batch"]) / np.median(t["singles"])), 3)
                    rows.append(row)
        shares.append({"G": G, "trials_local": nt, "image_form": "limbs" if owner.db_format() == P.DB_LIMBS else "packed",
                       "device_db_bytes": owner.db_device_bytes(), "all_gather_payload_bytes": {str(B): B * shp.trials * CT * 8 for B in sizes}, "rows": rows})
        for srv in reversed(servers):
            srv.close()
        torch.cuda.empty_cache()
    out = {"tool": "pack_shard_batch", "config": what, "reps": args.reps, "timing": "device events on the servers' stream; the pack legs include their downloads",
           "collective": "not run (one GPU)", "shares": shares}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
