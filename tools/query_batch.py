"""Fresh clients AND fresh queries on every lane of every batch, all responses read: what the per-client steps around a batch cost, and what taking
the queries in one call (spiral_gpu_server_set_query_batch) and the responses in one read (spiral_gpu_server_read_response_wire_batch) saves.  One
process, one build, the configs[1] geometry with B = 8 lanes, keys bound from a FULL key store of 64 clients:

    (a) fixed             keys and queries fixed: run_query_batch + one batched read -- the reference point of this run
    (b) per lane          the parent's path: bind_keys + eight set_query_seeded + run_query_batch + eight read_response_wire
    (c) batch, seeded     bind_keys + set_query_batch(seeded) + run_query_batch + read_response_wire_batch
    (d) batch, wire       (c) with the wire form
    (e) the ingest launch alone (copy + kernel) by device events, for 1 lane and for 8, both forms

queries/s = 8 / wall time of one step, steps back to back (every step ends in its read, which synchronises); the cases alternate within a run;
median of --runs runs with min - max.  Keys and queries are random words below Q (timing does not depend on them); the batch replays as one hipGraph.
The yardstick is (b), measured in the same run.

    python tools/query_batch.py --out profiles/query_batch.json"""
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

CONFIG1 = dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256)  # bench.py WORKLOADS configs[1]
N = 2048
B, POPULATION = 8, 64


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--steps", type=int, default=40, help="batches per run")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    torch.cuda.is_available()
    import spiral_amd as sa

    pg = sa.make_params(**CONFIG1)
    s = sa.get_shape(pg)
    rng = np.random.default_rng(1)
    owner = sa.Server(pg)
    owner.fill_db_random(3)
    lanes = [owner] + [sa.Server(pg, share_db_of=owner) for _ in range(B - 1)]
    stream = torch.cuda.Stream()
    for ln in lanes:
        ln.set_stream(stream.cuda_stream)
        ln.use_graphs(True)
    wire_of = lambda polys: sa.raw_to_wire(rng.integers(0, sa.Q, size=(polys, N), dtype=np.uint64))
    seed = lambda: rng.integers(0, 256, size=32, dtype=np.uint8)
    sent = (sa.pub_params_seeded_bytes(pg) - 32) // (7 * N)
    store = sa.KeyStore(pg, POPULATION, form="full")
    for c in range(POPULATION):
        store.put_seeded(c, np.concatenate([seed(), wire_of(sent)]))
    # two fresh queries per client, in both forms
    q_wire = [wire_of(2 * s.n_query_cts) for _ in range(2 * POPULATION)]
    q_seeded = [np.concatenate([seed(), wire_of(s.n_query_cts)]) for _ in range(2 * POPULATION)]
    assert q_wire[0].size == sa.query_wire_bytes(pg) and q_seeded[0].size == sa.query_seeded_bytes(pg)
    sync = lambda: (owner.sync(), torch.cuda.synchronize())
    slots_of = lambda step: [(step * B + b) % POPULATION for b in range(B)]  # fresh clients on all eight lanes, every batch
    msgs_of = lambda pool, step: [pool[(step * B + b) % len(pool)] for b in range(B)]
    sa.bind_keys(lanes, store, slots_of(0))
    sa.set_query_batch(lanes, msgs_of(q_seeded, 0), form="seeded")

    def fixed(step):
        sa.run_query_batch(lanes)
        sa.read_response_wire_batch(lanes)

    def per_lane(step):
        sa.bind_keys(lanes, store, slots_of(step))
        for ln, m in zip(lanes, msgs_of(q_seeded, step)):
            ln.set_query_seeded(m)
        sa.run_query_batch(lanes)
        for ln in lanes:
            ln.read_response_wire()

    def batch(form, pool):
        def step_(step):
            sa.bind_keys(lanes, store, slots_of(step))
            sa.set_query_batch(lanes, msgs_of(pool, step), form=form)
            sa.run_query_batch(lanes)
            sa.read_response_wire_batch(lanes)

        return step_

    cases = {"a_fixed": fixed, "b_per_lane_seeded": per_lane, "c_batch_seeded": batch("seeded", q_seeded), "d_batch_wire": batch("wire", q_wire)}
    qps = {k: [] for k in cases}
    for k, step_ in cases.items():  # warm-up: graph capture, staging buffers, first launches
        for step in range(3):
            step_(step)
    sync()
    for run in range(a.runs):  # the cases alternate, so that drift of the box lands on all of them
        for k, step_ in cases.items():
            sync()
            t0 = time.perf_counter()
            for step in range(a.steps):
                step_(run * a.steps + step + 1)
            sync()
            qps[k].append(B * a.steps / (time.perf_counter() - t0))

    # the ingest alone (one copy + one launch), by device events on the lanes' stream
    def ingest_us(form, pool, n, reps=20):
        ts = []
        for r in range(reps + 2):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            sa.set_query_batch(lanes[:n], msgs_of(pool, r)[:n], form=form)
            e1.record(stream)
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) * 1e3)
        return spread(ts[2:])

    # ... and the host's side of the two ways in: wall time of the calls alone, the stream idle
    def host_us(fn, reps=20):
        ts = []
        for r in range(reps + 2):
            sync()
            t0 = time.perf_counter()
            fn(r)
            ts.append((time.perf_counter() - t0) * 1e6)
        return spread(ts[2:])

    def eight_setters(r):
        for ln, m in zip(lanes, msgs_of(q_seeded, r)):
            ln.set_query_seeded(m)

    res = {
        "device": torch.cuda.get_device_name(0), "geometry": "configs[1]", "B": B, "population": POPULATION, "runs": a.runs, "steps_per_run": a.steps,
        "queries_per_s": {k: spread(v) for k, v in qps.items()},
        "ingest_launch_us": {f"{form}_n{n}": ingest_us(form, pool, n) for form, pool in (("seeded", q_seeded), ("wire", q_wire)) for n in (1, 8)},
        "host_call_us": {"eight_set_query_seeded": host_us(eight_setters),
                         "set_query_batch_seeded": host_us(lambda r: sa.set_query_batch(lanes, msgs_of(q_seeded, r), form="seeded")),
                         "eight_read_response_wire": host_us(lambda r: [ln.read_response_wire() for ln in lanes]),
                         "read_response_wire_batch": host_us(lambda r: sa.read_response_wire_batch(lanes))},
        "query_bytes": {"seeded": int(q_seeded[0].size), "wire": int(q_wire[0].size)},
    }
    q = res["queries_per_s"]
    res["relative_to_per_lane"] = {k: q[k]["median"] / q["b_per_lane_seeded"]["median"] for k in q}
    slim = lambda d: {k: {kk: vv for kk, vv in v.items() if kk != "runs"} for k, v in d.items()}
    print(json.dumps({k: v for k, v in res.items() if k not in ("queries_per_s", "ingest_launch_us", "host_call_us")} |
                     {"queries_per_s": slim(q), "ingest_launch_us": slim(res["ingest_launch_us"]), "host_call_us": slim(res["host_call_us"])}))
    store.close()
    for ln in lanes[::-1]:
        ln.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
