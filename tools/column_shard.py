"""One rank's share of a batch step on a G-way sharded database, the two shardings side by side on one GPU with no collectives:
tools/column_shard.py [--out FILE] [--configs config2,config3] [--G 2,4,8] [--B 1,2,4,8] [--reps R].  Each point alternates, in one process,
  - the j-shard step on shard 0 of G: run_pre_sweep_batch + fold_local_batch (replicated expansion) -- the baseline, the code as it was;
  - the column step on column shard 0 of G: run_column_batch.
Both replay hipGraphs; device events on the servers' stream; medians of R >= 7 alternated repetitions after warm-up, with min and max.  The sweep
launch alone (time_sweep_batch: events around the launch) is recorded for both.  Where a column shard has fewer than 64 columns the point is run
with option sweep_narrow 0 and 1, labelled.  The collectives are NOT run and NOT timed -- one GPU has no xGMI peer --: the bytes each flow would put
on the wire come from the shapes (spiral_amd/dist.py batch_collective_bytes, column_batch_collective_bytes).  Neither step includes fold_root_batch,
which is the same call on the same data in both flows.  Writes profiles/column_shard.json by default."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import spiral_amd as sa
from spiral_amd import dist as sdist

CONFIGS = {  # bench.py's configs[1] and configs[2] parameter sets (tools/shard_batch.py's)
    "config2": dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256),
    "config3": dict(nu1=9, nu2=10, t_gsw=10, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=22, p_db=256),
}
LABEL = {"config2": "configs[1]: 2^20 x 256B (nu1=8, nu2=7)", "config3": "configs[2]: 2^24 x 256B (nu1=9, nu2=10)"}


def ev_time(fn, stream):
    """device us of one call of fn (events on the servers' stream around it)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3


def stats(xs):
    return {"median": float(np.median(xs)), "min": float(min(xs)), "max": float(max(xs)), "samples": [float(x) for x in xs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "column_shard.json"))
    ap.add_argument("--configs", default="config2,config3")
    ap.add_argument("--G", default="2,4,8")
    ap.add_argument("--B", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=7, help="alternations of j-shard step / column step per point (at least 7)")
    a = ap.parse_args()
    if a.reps < 7:
        ap.error("--reps: at least 7 alternated repetitions per point")
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    rng = np.random.default_rng(1)
    narrow0 = sa.get_option("sweep_narrow")
    points = []
    for cname in a.configs.split(","):
        pg = sa.make_params(**CONFIGS[cname])
        shp = sa.get_shape(pg)
        mk = lambda shape: np.stack([rng.integers(0, m, size=shape + (sa.N,), dtype=np.uint64) for m in (sa.P, sa.B)], axis=-2)
        pp = (mk((shp.n_left, 2, pg.t_exp)), mk((shp.n_right, 2, pg.t_exp_right)), mk((3, 2 * pg.t_conv)), mk((3, 2 * pg.t_conv)))
        q = mk((1, 2))
        for G in [int(x) for x in a.G.split(",")]:
            Bs = [int(x) for x in a.B.split(",")]
            L = shp.num_per // G
            for narrow in ((0, 1) if L < 64 else (narrow0,)):
                sa.set_option("sweep_narrow", narrow)  # (read where an image takes the limb-plane form: the first batch of two or more)

                def lanes_of(own):
                    own.fill_db_random(3)
                    srvs = [own] + [sa.Server(pg, 0, share_db_of=own) for _ in range(max(Bs) - 1)]
                    for s in srvs:
                        s.set_stream(stream.cuda_stream)
                        s.set_pub_params(*pp)
                        s.set_query(q)
                    own.use_graphs(True)
                    return srvs

                jl = lanes_of(sa.Server(pg, 0, 0, shp.dim0 // G))
                for s in jl:
                    s.set_fold_ranks(G)
                cl = lanes_of(sa.Server(pg, 0, col_rank=0, col_ranks=G))
                for B in Bs:
                    with torch.cuda.stream(stream):
                        jb = sdist.batch_buffers(jl[:B], G, G, False, dev)
                        cb = sdist.column_batch_buffers(cl[:B], G, dev)

                        def j_step():
                            sa.run_pre_sweep_batch(jl[:B], jb["acc"].data_ptr())
                            sa.fold_local_batch(jl[:B], jb["chunk"].data_ptr(), jb["cts"].data_ptr())

                        def c_step():
                            sa.run_column_batch(cl[:B], cb["cts"].data_ptr())

                        for _ in range(2):  # captures, conversions and first launches
                            j_step()
                            c_step()
                        torch.cuda.synchronize()
                        tj, tc = [], []
                        for _ in range(a.reps):  # alternating, same process
                            tj.append(ev_time(j_step, stream))
                            tc.append(ev_time(c_step, stream))
                        sj = [sa.time_sweep_batch(jl[:B], 3) * 1e3 for _ in range(a.reps)]
                        sc = [sa.time_sweep_batch(cl[:B], 3) * 1e3 for _ in range(a.reps)]
                    J, Cc = stats(tj), stats(tc)
                    pt = {"config": cname, "label": LABEL[cname], "G": G, "B": B, "sweep_narrow": narrow, "num_per": shp.num_per, "dim0": shp.dim0,
                          "j_shard": {"dim0": shp.dim0 // G, "columns": shp.num_per, "image_form": "limbs" if jl[0].db_format() else "packed",
                                      "step_us": J, "sweep_us": stats(sj), "collective_bytes": sdist.batch_collective_bytes(shp, B, G)},
                          "column_shard": {"dim0": shp.dim0, "columns": L, "image_form": "limbs" if cl[0].db_format() else "packed",
                                           "step_us": Cc, "sweep_us": stats(sc), "collective_bytes": sdist.column_batch_collective_bytes(shp, B, G)},
                          "column_over_j": Cc["median"] / J["median"], "column_slower": Cc["median"] > J["median"]}
                    points.append(pt)
                    print(json.dumps({"config": cname, "G": G, "B": B, "sweep_narrow": narrow, "j_us": round(J["median"], 1), "col_us": round(Cc["median"], 1),
                                      "ratio": round(pt["column_over_j"], 3), "j_sweep_us": round(pt["j_shard"]["sweep_us"]["median"], 1),
                                      "col_sweep_us": round(pt["column_shard"]["sweep_us"]["median"], 1)}), flush=True)
                    del jb, cb
                for s in list(reversed(jl)) + list(reversed(cl)):
                    s.close()
                torch.cuda.empty_cache()
    sa.set_option("sweep_narrow", narrow0)
    out = {"what": "one rank's share of a batch step on a G-way sharded database, on ONE MI355X: the j-shard step (run_pre_sweep_batch + fold_local_batch, "
                   "replicated expansion) against the column step (run_column_batch), alternated in one process, hipGraphs on, device events",
           "note": "No collective was run or timed: one GPU has no xGMI peer. collective_bytes (from the shapes) is what each flow would put on the wire per "
                   "batch; the j-shard step's reduce-scatter is not in its time. column_slower marks the points where the column step took longer.",
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "points": points}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
