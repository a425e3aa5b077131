"""What a client session costs (include/spiral_gpu.h spiral_gpu_client_*), at the configs[1] geometry (base Spiral) and at the configs[4] SpiralPack
geometry, in one process on one build:

    public parameters per client          pub_params("seeded"), one call
    queries/s at 1, 8 and 64 per call     queries(idx, "seeded")
    decode per response at 1 and 8        decode(responses, "wire"), the responses of a server run on the session's own queries

Every call returns synchronised, so a call's wall time is what a caller waits; each figure is the median of --runs calls with min - max, after one
untimed call.  Every decoded response is compared with the database's item.  The host client's figures -- the `Key generation`, `Query generation`
and `Decoding` lines of ./spiral's summary -- are read from --host-runs runs of the command line, alternated with runs of --device-client, on the
same machine; they are what the ratios in the output are taken against.

    python tools/client.py --out profiles/client.json"""
from __future__ import annotations

import argparse
import json
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
BIN = os.path.join(ROOT, "spiral_amd", "spiral")

CONFIG1 = dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256)  # bench.py WORKLOADS configs[1]
PACK4 = dict(nu1=10, nu2=8, t_gsw=8, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=20, p_db=256)  # configs[4], out_n = 4
CLI = {"configs1": (["8", "7", "1234", "a"], {}), "configs4_pack": (["10", "8", "1234", "a", "--high-rate"], {"TEXP": "16", "OUTN": "4"})}
LINES = {"key_generation_us": "Key generation", "query_generation_us": "Query generation", "decoding_us": "Decoding"}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "runs": v}


def timed(fn, runs):
    fn()
    out = []
    for _ in range(runs):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e6)
    return out


def cli_lines(args, env, extra):
    r = subprocess.run([BIN] + args + ["--seed", "5"] + extra, capture_output=True, text=True, env=dict(os.environ, **env), timeout=900)
    assert r.returncode == 0 and re.search(r"Is correct\s?\?\s?: 1\n", r.stdout), r.stdout[-1500:] + r.stderr[-1500:]
    return {k: float(re.search(name + r" \(CPU·us\): (\d+)", r.stdout).group(1)) for k, name in LINES.items()}


def session_figures(sa, pg, out_n, runs):
    import torch

    cl = sa.Client(pg, bytes(range(32)), out_n=out_n)
    n_items = cl.n_items
    res = {"pub_params_us": spread(timed(lambda: cl.pub_params("seeded"), runs))}
    for n in (1, 8, 64):
        us = timed(lambda: cl.queries(np.arange(n) * 97 % n_items, "seeded"), runs)
        res[f"queries_per_call_{n}"] = {"call_us": spread(us), "queries_per_s": spread([n / u * 1e6 for u in us])}
    # responses to decode: the session's own queries answered by a server
    idx = [(1234 + 7919 * b) % n_items for b in range(8)]
    if out_n:
        srv = sa.PackServer(pg, out_n)
        srv.gen_db(1234)
        srv.set_pub_params_seeded(cl.pub_params("seeded"))
        wires = []
        for i in idx:
            srv.answer_seeded(cl.query(i, "seeded"))
            wires.append(srv.read_response_wire())
        wires = np.stack(wires)
    else:
        owner = sa.Server(pg)
        owner.gen_db(1234)
        lanes = [owner] + [sa.Server(pg, share_db_of=owner) for _ in range(7)]
        msg = cl.pub_params("seeded")
        for ln in lanes:
            ln.set_pub_params_seeded(msg)
        sa.set_query_batch(lanes, list(cl.queries(idx, "seeded")), form="seeded")
        sa.run_query_batch(lanes)
        wires = sa.read_response_wire_batch(lanes)
    torch.cuda.synchronize()
    got = cl.decode(wires, form="wire")
    res["decoded_items_checked"] = check_items(sa, pg, out_n, got, idx)
    for n in (1, 8):
        us = timed(lambda: cl.decode(wires[:n], form="wire"), runs)
        res[f"decode_per_call_{n}"] = {"call_us": spread(us), "per_response_us": spread([u / n for u in us])}
    res["eight_queries_call_us"] = res["queries_per_call_8"]["call_us"]["median"]
    res["eight_decodes_call_us"] = res["decode_per_call_8"]["call_us"]["median"]
    res["decoding_eight_costs_less_than_their_queries"] = res["eight_decodes_call_us"] < res["eight_queries_call_us"]
    return res


def check_items(sa, pg, out_n, got, idx):
    """every decoded plaintext against the seeded database's item (the generator of gen_db, restated: splitmix64 of seed ^ position)"""
    def splitmix(x):
        x = (x + np.uint64(0x9E3779B97F4A7C15))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))

    seed, n_ok = np.uint64(1234), 0
    total = np.uint64((1 << pg.nu1) * (1 << pg.nu2))
    with np.errstate(over="ignore"):
        for b, item in enumerate(idx):
            if out_n:
                t = np.arange(out_n * out_n, dtype=np.uint64).reshape(-1, 1)
                pos = (t * total + np.uint64(item)) * np.uint64(2048) + np.arange(2048, dtype=np.uint64)
            else:
                pos = np.uint64(item) * np.uint64(4 * 2048) + np.arange(4 * 2048, dtype=np.uint64)
            want = splitmix(seed ^ pos) % np.uint64(pg.p_db)
            assert (got[b].reshape(-1) == want.reshape(-1)).all(), f"response {b} does not decode to item {item}"
            n_ok += 1
    return n_ok


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=3, help="runs of ./spiral per client kind and geometry (the host client takes seconds each)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    torch.cuda.is_available()
    import spiral_amd as sa
    from spiral_amd import pack as _  # noqa: F401

    out = {"what": "client session vs the command line's host client; wall time of synchronous calls, us; medians with min - max",
           "device": torch.cuda.get_device_name(0), "runs": a.runs, "host_runs": a.host_runs}
    for name, (pg, out_n) in {"configs1": (sa.make_params(**CONFIG1), 0), "configs4_pack": (sa.make_params(**PACK4), 4)}.items():
        fig = {"session": session_figures(sa, pg, out_n, a.runs)}
        host, dev = [], []
        args, env = CLI[name]
        for _ in range(a.host_runs):  # alternated
            host.append(cli_lines(args, env, []))
            dev.append(cli_lines(args, env, ["--device-client"]))
        fig["cli_host_client"] = {k: spread([h[k] for h in host]) for k in LINES}
        fig["cli_device_client"] = {k: spread([d[k] for d in dev]) for k in LINES}
        fig["host_over_device"] = {k: fig["cli_host_client"][k]["median"] / max(fig["cli_device_client"][k]["median"], 1.0) for k in LINES}
        out[name] = fig
        print(name, json.dumps({k: v for k, v in fig.items() if k != "session"}, indent=1), flush=True)
        print(name, "session", json.dumps({k: (v["call_us"]["median"] if isinstance(v, dict) and "call_us" in v else v.get("median") if isinstance(v, dict) else v)
                                             for k, v in fig["session"].items()}), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
