"""What ONE rank of a G-GPU answer to a batch of B clients computes, timed on one GPU with no collectives: tools/shard_batch.py [--out FILE]
[--configs config2,config3] [--G 1,2,4,8] [--B 1,2,4,8] [--reps R].  Each point is this rank's owner on j-shard 0 of G and its B - 1 lanes:
run_pre_sweep_batch (or, with a sharded expansion, run_expand_pack_batch + run_unpack_convert_sweep_batch), fold_local_batch, fold_root_batch --
and, alternating with it in the same process, B single-query flows of the same rank (run_pre_sweep or run_expand_pack + run_unpack_convert_sweep,
fold_local, fold_root).  All calls replay hipGraphs.  The collectives are NOT run and NOT timed: their bytes per batch are computed from the
shapes (spiral_amd/dist.py batch_collective_bytes).  Writes profiles/shard_batch.json by default."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import spiral_amd as sa
from spiral_amd import dist as sdist

CONFIGS = {  # bench.py's configs[1] and configs[2] parameter sets
    "config2": dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256),
    "config3": dict(nu1=9, nu2=10, t_gsw=10, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=22, p_db=256),
}
LABEL = {"config2": "configs[1]: 2^20 x 256B (nu1=8, nu2=7)", "config3": "configs[2]: 2^24 x 256B (nu1=9, nu2=10)"}


def ev_time(fn, stream, reps):
    """device us per call of fn (events on the servers' stream around reps calls)"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(reps):
        fn()
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "shard_batch.json"))
    ap.add_argument("--configs", default="config2,config3")
    ap.add_argument("--G", default="1,2,4,8")
    ap.add_argument("--B", default="1,2,4,8")
    ap.add_argument("--reps", type=int, default=5, help="alternations of batch / singles per point")
    ap.add_argument("--expansion", default="replicated,sharded")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    rng = np.random.default_rng(1)
    points = []
    for cname in a.configs.split(","):
        pg = sa.make_params(**CONFIGS[cname])
        shp = sa.get_shape(pg)
        mk = lambda shape: np.stack([rng.integers(0, m, size=shape + (sa.N,), dtype=np.uint64) for m in (sa.P, sa.B)], axis=-2)
        pp = (mk((shp.n_left, 2, pg.t_exp)), mk((shp.n_right, 2, pg.t_exp_right)), mk((3, 2 * pg.t_conv)), mk((3, 2 * pg.t_conv)))
        q = mk((1, 2))
        for G in [int(x) for x in a.G.split(",")]:
            Bs = [int(x) for x in a.B.split(",")]
            own = sa.Server(pg, 0, 0, shp.dim0 // G)
            own.fill_db_random(3)
            srvs = [own] + [sa.Server(pg, 0, share_db_of=own) for _ in range(max(Bs) - 1)]
            for s in srvs:
                s.set_stream(stream.cuda_stream)
                s.set_pub_params(*pp)
                s.set_query(q)
                s.set_fold_ranks(G)
            own.use_graphs(True)
            # the single-query flow's buffers (fold_local reads a chunk, fold_root the gathered cts)
            chunk1 = torch.zeros(shp.num_per * 6 * sa.N // G, dtype=torch.int64, device=dev)
            ct1 = torch.zeros(6 * sa.N, dtype=torch.int64, device=dev)
            gath1 = torch.zeros(G * 6 * sa.N, dtype=torch.int64, device=dev)
            acc1 = torch.zeros(shp.num_per * 6 * sa.N, dtype=torch.int64, device=dev)
            own.set_acc(acc1.data_ptr())
            for mode in a.expansion.split(","):
                sharded = mode == "sharded"
                if sharded and G == 1:
                    continue  # (one rank expands everything)
                for s in srvs:
                    s.set_expand_shard(0, G if sharded else 1)
                for B in Bs:
                    lanes = srvs[:B]
                    with torch.cuda.stream(stream):
                        bufs = sdist.batch_buffers(lanes, G, G, sharded, dev)
                        if G == 1:
                            bufs["chunk"], bufs["gathered_cts"] = bufs["acc"], bufs["cts"]
                        bits1 = torch.zeros(own.gsw_bits_words(), dtype=torch.int64, device=dev) if sharded else None
                        gbits1 = torch.zeros(G * own.gsw_bits_words(), dtype=torch.int64, device=dev) if sharded else None
                        steps_b = {}
                        if sharded:
                            steps_b["expand_pack_batch"] = lambda: sa.run_expand_pack_batch(lanes, bufs["bits"].data_ptr())
                            steps_b["unpack_convert_sweep_batch"] = lambda: sa.run_unpack_convert_sweep_batch(lanes, bufs["gathered_bits"].data_ptr(), bufs["acc"].data_ptr())
                        else:
                            steps_b["pre_sweep_batch"] = lambda: sa.run_pre_sweep_batch(lanes, bufs["acc"].data_ptr())
                        steps_b["fold_local_batch"] = lambda: sa.fold_local_batch(lanes, bufs["chunk"].data_ptr(), bufs["cts"].data_ptr())
                        steps_b["fold_root_batch"] = lambda: sa.fold_root_batch(lanes, bufs["gathered_cts"].data_ptr(), bufs["responses"].data_ptr())
                        steps_1 = {}
                        if sharded:
                            steps_1["expand_pack"] = lambda: own.run_expand_pack(bits1.data_ptr())
                            steps_1["unpack_convert_sweep"] = lambda: own.run_unpack_convert_sweep(gbits1.data_ptr())
                        else:
                            steps_1["pre_sweep"] = own.run_pre_sweep
                        steps_1["fold_local"] = lambda: own.fold_local(chunk1.data_ptr(), ct1.data_ptr())
                        steps_1["fold_root"] = lambda: own.fold_root(gath1.data_ptr())
                        batch = lambda: [f() for f in steps_b.values()]
                        singles = lambda: [f() for _ in range(B) for f in steps_1.values()]
                        batch()
                        singles()  # captures and first launches
                        torch.cuda.synchronize()
                        tb, ts = [], []
                        for _ in range(a.reps):  # alternating, same process
                            tb.append(ev_time(batch, stream, 1))
                            ts.append(ev_time(singles, stream, 1))
                        per_step = {k: ev_time(f, stream, 3) for k, f in steps_b.items()}
                        per_step_1 = {k: ev_time(f, stream, 3) for k, f in steps_1.items()}
                    bt, st = float(np.median(tb)), float(np.median(ts))
                    pt = {"config": cname, "label": LABEL[cname], "G": G, "B": B, "expansion": mode, "shard_dim0": shp.dim0 // G, "num_per": shp.num_per,
                          "batch_step_us": bt, "singles_step_us": st, "batch_over_singles": bt / st,
                          "batch_us_samples": tb, "singles_us_samples": ts,
                          "per_step_batch_us": per_step, "per_step_single_us": per_step_1,
                          "queries_per_s_per_rank_excluding_collectives": {"batch": B / bt * 1e6, "singles": B / st * 1e6},
                          "collective_bytes_per_batch": sdist.batch_collective_bytes(shp, B, G, own.gsw_bits_words() if sharded else 0)}
                    points.append(pt)
                    print(json.dumps({k: pt[k] for k in ("config", "G", "B", "expansion", "batch_step_us", "singles_step_us", "batch_over_singles")}), flush=True)
                    del bufs
            for s in reversed(srvs):
                s.close()
            torch.cuda.empty_cache()
    out = {"what": "one rank's share of a batch step of a j-sharded answer, on ONE MI355X: every library step, NO collective (neither run nor timed)",
           "note": "No multi-GPU time was measured. The collectives' cost at these sizes (collective_bytes_per_batch, computed from the shapes) is the open "
                   "number this path rests on: queries_per_s_per_rank_excluding_collectives is an upper bound of a deployment's rate, not a prediction.",
           "device": torch.cuda.get_device_name(0), "reps": a.reps, "points": points}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(f"wrote {a.out}")


if __name__ == "__main__":
    main()
