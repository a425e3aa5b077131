"""Query and public-parameter ingest in the wire form against the NTT form (include/spiral_gpu.h spiral_gpu_server_set_query_wire): wall time of
set_query vs set_query_wire on the same queries at configs[1] and configs[3], of set_pub_params vs set_pub_params_wire at configs[1], and a
configs[3] item batch of B = 8 clients including their eight query uploads, both ways.  Each pair is alternated, `--reps` repetitions; medians.

    python tools/wire_input.py --out profiles/wire_input.json
    rocprofv3 --kernel-trace --stats -d DIR -o wire -- python tools/wire_input.py --kernels   # decode launches alone, for the kernel trace

The item batch keeps `--instances` configs[3] images resident (56 GiB each) and scales to 7 instances as tools/batch_instances.py does: the time of
n instances minus that of one is n - 1 times the per-instance cost."""
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


def rand_raw(rng, npolys, Q):
    return rng.integers(0, Q, size=(npolys, N), dtype=np.uint64)


def client_forms(sa, rng, npolys):
    """a random raw message in both of its forms: the NTT form (what set_query takes) and the wire form"""
    raw = rand_raw(rng, npolys, sa.Q)
    return sa.to_ntt(raw), sa.raw_to_wire(raw)


def timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def alternate(a, b, reps, sync):
    ta, tb = [], []
    a(), b()  # warm-up (staging buffers, first launches)
    for _ in range(reps):
        ta.append(timed(a, sync))
        tb.append(timed(b, sync))
    return {"ntt_ms": ta, "wire_ms": tb, "ntt_median_ms": statistics.median(ta), "wire_median_ms": statistics.median(tb),
            "speedup": statistics.median(ta) / statistics.median(tb)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--instances", type=int, default=2, help="resident configs[3] images for the item batch (>= 2)")
    ap.add_argument("--kernels", action="store_true", help="only the decode launches and the existing forward transform (for a kernel trace)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    torch.cuda.is_available()
    import spiral_amd as sa

    rng = np.random.default_rng(1)
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    if a.kernels:
        pg = sa.make_params(**CONFIGS["configs[3]"])
        srv = sa.Server(pg)
        s = sa.get_shape(pg)
        _, w = client_forms(sa, rng, s.n_query_cts * 2)
        for _ in range(5):
            srv.set_query_wire(w)
        fwd, inv = sa.time_ntt(4168, 5)
        print(json.dumps({"polys_per_decode": s.n_query_cts * 2, "to_ntt_ms_4168": fwd}))
        srv.close()
        return
    for name in ("configs[1]", "configs[3]"):
        pg = sa.make_params(**CONFIGS[name])
        s = sa.get_shape(pg)
        srv = sa.Server(pg)
        q, w = client_forms(sa, rng, s.n_query_cts * 2)
        r = alternate(lambda: srv.set_query(q), lambda: srv.set_query_wire(w), a.reps, srv.sync)
        r.update(polys=s.n_query_cts * 2, ntt_bytes=int(q.nbytes), wire_bytes=int(w.size))
        res[f"set_query {name}"] = r
        if name == "configs[1]":
            n_pp = sa.pub_params_wire_bytes(pg) // (7 * N)
            nl, nr = s.n_left * 2 * pg.t_exp, s.n_right * 2 * pg.t_exp_right
            ntt, wpp = client_forms(sa, rng, n_pp)
            parts = np.split(ntt, [nl, nl + nr, nl + nr + 6 * pg.t_conv])
            r = alternate(lambda: srv.set_pub_params(*[np.ascontiguousarray(x) for x in parts]), lambda: srv.set_pub_params_wire(wpp), a.reps, srv.sync)
            r.update(polys=n_pp, ntt_bytes=int(ntt.nbytes), wire_bytes=int(wpp.size))
            res[f"set_pub_params {name}"] = r
        srv.close()
        print(json.dumps({k: v for k, v in res.items() if k.endswith(name)}), flush=True)
    # configs[3] item batch, B = 8, eight query uploads included
    import torch

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
    npp = sa.pub_params_wire_bytes(pg) // (7 * N)
    _, wpp = client_forms(sa, rng, npp)
    forms = [client_forms(sa, rng, s.n_query_cts * 2) for _ in range(B)]
    for sv in servers:
        sv.set_pub_params_wire(wpp)
    words = 6 * N
    d = torch.zeros(B * n_res * words, dtype=torch.int64, device="cuda")
    sync = lambda: (servers[0].sync(), torch.cuda.synchronize())
    out = {}
    for n in (1, n_res):
        def ntt_path():
            for sv, (q, _) in zip(servers, forms):
                sv.set_query(q)
            sa.run_query_batch_instances(servers, inst[:n], d.data_ptr())

        def wire_path():
            for sv, (_, w) in zip(servers, forms):
                sv.set_query_wire(w)
            sa.run_query_batch_instances(servers, inst[:n], d.data_ptr())

        out[n] = alternate(ntt_path, wire_path, a.reps, sync)
    item = {}
    for path in ("ntt", "wire"):
        t1, tn = out[1][f"{path}_median_ms"], out[n_res][f"{path}_median_ms"]
        per_inst = (tn - t1) / (n_res - 1)
        t7 = t1 + 6 * per_inst
        item[path] = {"ms_1_instance": t1, f"ms_{n_res}_instances": tn, "ms_per_instance": per_inst, "ms_7_instances_scaled": t7, "items_per_s": B / t7 * 1e3}
    item["raw"] = {str(k): v for k, v in out.items()}
    res["item batch configs[3] B=8 (query uploads included)"] = item
    print(json.dumps(item["ntt"]), json.dumps(item["wire"]), flush=True)
    for sv in servers[1:]:
        sv.close()
    for sv in inst:
        sv.close()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
