"""Query and public-parameter ingest in the seeded form against the wire and NTT forms (include/spiral_gpu.h spiral_gpu_server_set_query_seeded):
wall time of set_query / set_query_wire / set_query_seeded on the same-sized messages at configs[1] and configs[3], of the three set_pub_params forms
at configs[1], and a configs[3] item batch of B = 8 clients including their eight query uploads, all three ways.  Each triple is alternated in one
process, `--reps` repetitions; medians.

    python tools/seeded_input.py --out profiles/seeded_input.json
    rocprofv3 --kernel-trace --stats -d DIR -o seeded -- python tools/seeded_input.py --kernels   # row-0 generator launches, for the kernel trace

The item batch keeps `--instances` configs[3] images resident (56 GiB each) and scales to 7 instances as tools/wire_input.py does."""
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

CONFIGS = {  # bench.py WORKLOADS
    "configs[1]": dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256),
    "configs[3]": dict(nu1=11, nu2=9, t_gsw=4, t_conv=56, t_exp=2, t_exp_right=56, qprime_bits=27, p_db=32768, direct_upload=1),
}
N = 2048
FORMS = ("ntt", "wire", "seeded")


def client_forms(sa, rng, npolys, seeded_bytes):
    """a random message in its three forms: the NTT form, the wire form, and a seeded form of seeded_bytes (a seed, then random raw rows 1..)"""
    raw = rng.integers(0, sa.Q, size=(npolys, N), dtype=np.uint64)
    sent = (seeded_bytes - 32) // (7 * N)
    seeded = np.concatenate([rng.integers(0, 256, size=32, dtype=np.uint8), sa.raw_to_wire(raw[:sent])])
    assert seeded.size == seeded_bytes
    return sa.to_ntt(raw), sa.raw_to_wire(raw), seeded


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def alternate(fns, reps, sync):
    ts = {k: [] for k in fns}
    for f in fns.values():  # warm-up (staging buffers, first launches)
        f()
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(timed(f, sync))
    out = {f"{k}_ms": v for k, v in ts.items()}
    out.update({f"{k}_median_ms": statistics.median(v) for k, v in ts.items()})
    out["seeded_over_wire"] = out["seeded_median_ms"] / out["wire_median_ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--instances", type=int, default=2, help="resident configs[3] images for the item batch (>= 2)")
    ap.add_argument("--kernels", action="store_true", help="only seeded configs[3] queries (for a kernel trace of the row-0 generator)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    torch.cuda.is_available()
    import spiral_amd as sa

    rng = np.random.default_rng(1)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    if a.kernels:
        pg = sa.make_params(**CONFIGS["configs[3]"])
        s = sa.get_shape(pg)
        srv = sa.Server(pg)
        _, _, m = client_forms(sa, rng, s.n_query_cts * 2, sa.query_seeded_bytes(pg))
        for _ in range(10):
            srv.set_query_seeded(m)
        srv.sync()
        print(json.dumps({"row0_polys_per_call": s.n_query_cts, "calls": 10}))
        srv.close()
        return
    for name in ("configs[1]", "configs[3]"):
        pg = sa.make_params(**CONFIGS[name])
        s = sa.get_shape(pg)
        srv = sa.Server(pg)
        q, w, m = client_forms(sa, rng, s.n_query_cts * 2, sa.query_seeded_bytes(pg))
        r = alternate({"ntt": lambda: srv.set_query(q), "wire": lambda: srv.set_query_wire(w), "seeded": lambda: srv.set_query_seeded(m)}, a.reps, srv.sync)
        r.update(polys=s.n_query_cts * 2, ntt_bytes=int(q.nbytes), wire_bytes=int(w.size), seeded_bytes=int(m.size))
        res[f"set_query {name}"] = r
        if name == "configs[1]":
            n_pp = sa.pub_params_wire_bytes(pg) // (7 * N)
            nl, nr = s.n_left * 2 * pg.t_exp, s.n_right * 2 * pg.t_exp_right
            ntt, wpp, mpp = client_forms(sa, rng, n_pp, sa.pub_params_seeded_bytes(pg))
            parts = [np.ascontiguousarray(x) for x in np.split(ntt, [nl, nl + nr, nl + nr + 6 * pg.t_conv])]
            r = alternate({"ntt": lambda: srv.set_pub_params(*parts), "wire": lambda: srv.set_pub_params_wire(wpp),
                           "seeded": lambda: srv.set_pub_params_seeded(mpp)}, a.reps, srv.sync)
            r.update(polys=n_pp, ntt_bytes=int(ntt.nbytes), wire_bytes=int(wpp.size), seeded_bytes=int(mpp.size))
            res[f"set_pub_params {name}"] = r
        srv.close()
        print(json.dumps({k: {kk: vv for kk, vv in v.items() if not kk.endswith("_ms")} for k, v in res.items() if k.endswith(name)}), flush=True)
    # configs[3] item batch, B = 8, eight query uploads included
    pg = sa.make_params(**CONFIGS["configs[3]"])
    s = sa.get_shape(pg)
    B, n_res = 8, max(2, a.instances)
    inst = []
    for k in range(n_res):
        sv = sa.Server(pg)
        sv.fill_db_random(100 + k)
        inst.append(sv)
    servers = [inst[0]] + [sa.Server(pg, share_db_of=inst[0]) for _ in range(B - 1)]
    st = sa.lib().spiral_gpu_server_get_stream(inst[0].h)
    for sv in servers[1:]:
        sv.set_stream(st)
    _, _, mpp = client_forms(sa, rng, sa.pub_params_wire_bytes(pg) // (7 * N), sa.pub_params_seeded_bytes(pg))
    forms = [client_forms(sa, rng, s.n_query_cts * 2, sa.query_seeded_bytes(pg)) for _ in range(B)]
    for sv in servers:
        sv.set_pub_params_seeded(mpp)
    d = torch.zeros(B * n_res * 6 * N, dtype=torch.int64, device="cuda")
    sync = lambda: (servers[0].sync(), torch.cuda.synchronize())
    setters = {"ntt": lambda sv, f: sv.set_query(f[0]), "wire": lambda sv, f: sv.set_query_wire(f[1]), "seeded": lambda sv, f: sv.set_query_seeded(f[2])}
    out = {}
    for n in (1, n_res):
        def path(form, n=n):
            def run():
                for sv, f in zip(servers, forms):
                    setters[form](sv, f)
                sa.run_query_batch_instances(servers, inst[:n], d.data_ptr())
            return run

        out[n] = alternate({form: path(form) for form in FORMS}, a.reps, sync)
    item = {}
    for form in FORMS:
        t1, tn = out[1][f"{form}_median_ms"], out[n_res][f"{form}_median_ms"]
        per_inst = (tn - t1) / (n_res - 1)
        t7 = t1 + 6 * per_inst
        item[form] = {"ms_1_instance": t1, f"ms_{n_res}_instances": tn, "ms_per_instance": per_inst, "ms_7_instances_scaled": t7, "items_per_s": B / t7 * 1e3}
    item["raw"] = {str(k): v for k, v in out.items()}
    res["item batch configs[3] B=8 (query uploads included)"] = item
    print(json.dumps({f: item[f] for f in FORMS}), flush=True)
    for sv in servers[1:]:
        sv.close()
    for sv in inst:
        sv.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
