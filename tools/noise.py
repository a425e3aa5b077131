"""The noise this implementation leaves in a response, measured on the device (include/spiral_gpu.h spiral_gpu_client_response_noise), beside the
noise model the parameter selector rests on (spiral_amd/scheme.py), and what the measurement costs.

Per parameter set -- configs[1], the configs[4] SpiralPack geometry and the published sets whose one database instance fits --max-db-gib -- with
gen_db, over --queries queries of distinct items from each of --seeds client seeds:

    the measured width2() of the unswitched (FINAL) and of the switched response against the true item
    the model's two figures for the same set (scheme.response_noise_model) and the ratio measured / model
    the smallest budget_bits() seen and the total n_wrong

The ratio is recorded, not judged: the model is a heuristic bound.  Units: the FINAL form's width2() is in steps of scale_k = Q // p, the model's
s_e in units of Q, so s_e (p / Q)^2 is the model in the same steps; the switched width2() is in steps of D = 4 q', one plaintext step (x / D is
the plaintext), the unit of the model's second figure.

Timing (configs[1] and configs[4]): medians of --runs alternated repetitions with min - max, wall time of the synchronous calls in one process --
response_noise in its RAW and FINAL forms against decode on the same 1, 8 and 64 responses; and, with --parent-lib PATH (a build of the parent
commit's library), decode of this build against decode of that build on the same responses, alternated.

    python tools/noise.py --out profiles/noise.json [--parent-lib /path/to/parent/libspiral_gpu.so]"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Q = 268369921 * 249561089
N = 2048
EXTRA = {  # beside scheme.PUBLISHED: bench.py WORKLOADS configs[1] and configs[4]
    "configs1": ("spiral", dict(nu_1=8, nu_2=7, p=256, q_prime_bits=20, t_GSW=8, t_conv=4, t_exp=8, t_exp_right=56)),
    "configs4_pack": ("spiral-pack", dict(n=4, nu_1=10, nu_2=8, p=256, q_prime_bits=20, t_GSW=8, t_conv=4, t_exp=16, t_exp_right=56)),
}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def db_items(prm, out_n, idx):
    """the seeded database's items (the generator of gen_db, restated: splitmix64 of seed ^ position): [len(idx)][rows][cols][2048]"""
    def splitmix(x):
        x = (x + np.uint64(0x9E3779B97F4A7C15))
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))

    total = np.uint64(1 << (prm.nu1 + prm.nu2))
    rows = out_n or 2
    out = []
    with np.errstate(over="ignore"):
        for item in idx:
            if out_n:
                t = np.arange(out_n * out_n, dtype=np.uint64).reshape(-1, 1)
                pos = (t * total + np.uint64(item)) * np.uint64(N) + np.arange(N, dtype=np.uint64)
            else:
                pos = np.uint64(item) * np.uint64(4 * N) + np.arange(4 * N, dtype=np.uint64)
            out.append((splitmix(np.uint64(1234) ^ pos) % np.uint64(prm.p_db)).reshape(rows, rows, N))
    return np.stack(out)


def answers(sa, prm, out_n, seeds, queries):
    """per client seed: (session, FINAL ciphertexts, wire responses, item indices) of `queries` queries of distinct items against gen_db(1234)"""
    from spiral_amd import ops
    from spiral_amd import server as SV

    srv = sa.PackServer(prm, out_n) if out_n else sa.Server(prm)
    srv.gen_db(1234)
    out = []
    for k, seed in enumerate(seeds):
        cl = sa.Client(prm, seed, out_n=out_n)
        idx = [(1234 + 7919 * (k * queries + b)) % cl.n_items for b in range(queries)]
        assert len(set(idx)) == len(idx) or cl.n_items < len(seeds) * queries
        srv.set_pub_params_seeded(cl.pub_params("seeded"))
        fins, wires = [], []
        for i in idx:
            if out_n:
                _, packed, _ = srv.answer_seeded(cl.query(i, "seeded"))
                fins.append(ops.from_ntt(packed))
            else:
                srv.set_query_seeded(cl.query(i, "seeded"))
                srv.run_query()
                srv.sync()
                fins.append(srv.read(SV.BUF_FINAL).reshape(3, 2, N))
            wires.append(np.ascontiguousarray(srv.read_response_wire()).reshape(-1))
        out.append((cl, np.stack(fins), np.stack(wires), idx))
    srv.close()
    return out


def measure(sa, S, name, kind, prm_d, seeds, queries):
    out_n = prm_d.get("n", 0) if kind.endswith("-pack") else 0
    p = S.real_p(prm_d["p"])
    prm = sa.make_params(prm_d["nu_1"], prm_d["nu_2"], t_gsw=prm_d["t_GSW"], t_conv=prm_d["t_conv"], t_exp=prm_d["t_exp"], t_exp_right=prm_d["t_exp_right"],
                         qprime_bits=prm_d["q_prime_bits"], p_db=p, direct_upload=prm_d.get("direct", 0))
    runs = answers(sa, prm, out_n, seeds, queries)
    qprime = int(runs[0][0].shape.qprime)
    sums = {"final": [0, 0, 0], "wire": [0, 0, 0]}  # sum, sum of squares, count
    budget = {"final": math.inf, "wire": math.inf}
    wrong = {"final": 0, "wire": 0}
    for cl, fins, wires, idx in runs:
        items = db_items(prm, out_n, idx)
        for form, data in (("final", fins), ("wire", wires)):
            rn = cl.response_noise(data, form=form, expected=items)
            sums[form][0] += int(rn.sum.sum())
            sums[form][1] += int(rn.sumsq.sum())
            sums[form][2] += rn.count * rn.sum.size
            budget[form] = min(budget[form], rn.budget_bits())
            wrong[form] += int(rn.n_wrong.sum())
    from fractions import Fraction

    var = {f: float(Fraction(s[1], s[2]) - Fraction(s[0], s[2]) ** 2) for f, s in sums.items()}
    step = {"final": Q // p, "wire": 4 * qprime}
    width2 = {f: 2 * math.pi * var[f] / float(step[f]) ** 2 for f in var}
    kw = {k: prm_d[k] for k in ("p", "t_GSW", "t_conv", "t_exp", "t_exp_right", "nu_1", "nu_2")}
    s_e, w2 = S.response_noise_model(kind, q_prime=qprime, n=prm_d.get("n", 2), **kw)
    model_final = s_e * (float(p) / float(S.REAL_Q)) ** 2  # the model's unswitched width^2 in steps of scale_k
    res = {"kind": kind, "params": prm_d, "out_n": out_n, "q_prime": qprime, "clients": len(seeds), "queries": len(seeds) * queries,
           "coefficients": sums["final"][2],
           "final": {"width2_steps": width2["final"], "variance_log2": math.log2(var["final"]) if var["final"] else None, "model_s_e_log2": math.log2(s_e),
                     "model_width2_steps": model_final, "measured_over_model": width2["final"] / model_final,
                     "min_budget_bits": budget["final"], "radius_bits": math.log2(step["final"] / 2), "n_wrong": wrong["final"]},
           # rows 1.. of a switched response are rounded to multiples of a quarter step (modulus 4 p): a uniform error of variance 1 / 192 of a step^2,
           # width^2 = 2 pi / 192, which the model does not carry as variance (it takes it off the threshold: 1/4 in place of 1/2)
           "switched": {"width2_steps": width2["wire"], "model_width2_steps": w2, "measured_over_model": width2["wire"] / w2,
                        "width2_steps_less_row_rounding": width2["wire"] - 2 * math.pi / 192, "less_row_rounding_over_model": (width2["wire"] - 2 * math.pi / 192) / w2, "min_budget_bits": budget["wire"], "radius_bits": math.log2(step["wire"] / 2),
                        "n_wrong": wrong["wire"]}}
    print(name, json.dumps({k: res[k] for k in ("final", "switched")}), flush=True)
    return res, prm, out_n, runs


def timed_alternated(fns, runs):
    """{name: [us]}: every function once untimed, then `runs` rounds in which each is timed once, in order"""
    for fn in fns.values():
        fn()
    out = {k: [] for k in fns}
    for _ in range(runs):
        for k, fn in fns.items():
            t0 = time.perf_counter()
            fn()
            out[k].append((time.perf_counter() - t0) * 1e6)
    return out


class ParentDecode:
    """decode through another build of the library (the parent commit's): a session from the same seed holds the same key"""

    def __init__(self, path, prm, out_n, seed):
        from spiral_amd._lib import Params

        L = C.CDLL(path)
        L.spiral_gpu_client_create.argtypes = [C.POINTER(Params), C.c_uint32, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_void_p)]
        L.spiral_gpu_client_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(C.c_uint64)]
        L.spiral_gpu_client_destroy.argtypes = [C.c_void_p]
        L.spiral_gpu_client_destroy.restype = None
        L.spiral_gpu_last_error.restype = C.c_char_p
        self.L, self.h, self.rows = L, C.c_void_p(), out_n or 2
        assert L.spiral_gpu_client_create(C.byref(prm), out_n, 0, seed, 0, C.byref(self.h)) == 0, L.spiral_gpu_last_error()

    def decode(self, wires):
        out = np.zeros((len(wires), self.rows, self.rows, N), dtype=np.uint64)
        assert self.L.spiral_gpu_client_decode(self.h, wires.ctypes.data_as(C.c_void_p), len(wires), 1, out.ctypes.data_as(C.POINTER(C.c_uint64))) == 0
        return out

    def close(self):
        self.L.spiral_gpu_client_destroy(self.h)


def timing(sa, prm, out_n, run, seed, reps, parent_lib):
    cl, fins, wires, _ = run
    res = {}
    for n in (1, 8, 64):
        w = np.ascontiguousarray(np.tile(wires, (n // len(wires) + 1, 1))[:n])
        f = np.ascontiguousarray(np.tile(fins, (n // len(fins) + 1, 1, 1, 1))[:n])
        raw = np.stack([sa.response_from_wire(cl.params, x, cl.cols) for x in w])
        us = timed_alternated({"decode_wire": lambda: cl.decode(w, form="wire"), "noise_wire": lambda: cl.response_noise(w, form="wire"),
                               "decode_raw": lambda: cl.decode(raw), "noise_raw": lambda: cl.response_noise(raw), "noise_final": lambda: cl.response_noise(f, form="final")}, reps)
        res[f"responses_{n}"] = {k: spread(v) for k, v in us.items()}
        res[f"responses_{n}"]["noise_over_decode"] = {k: statistics.median(us["noise_" + k]) / statistics.median(us["decode_" + k]) for k in ("wire", "raw")}
        res[f"responses_{n}"]["noise_final_over_decode_raw"] = statistics.median(us["noise_final"]) / statistics.median(us["decode_raw"])
    if parent_lib:
        par = ParentDecode(parent_lib, prm, out_n, seed)
        for n in (1, 8, 64):
            w = np.ascontiguousarray(np.tile(wires, (n // len(wires) + 1, 1))[:n])
            assert (par.decode(w) == cl.decode(w, form="wire")).all(), "decode of this build differs from the parent build's"
            us = timed_alternated({"this": lambda: cl.decode(w, form="wire"), "parent": lambda: par.decode(w)}, reps)
            t, q = spread(us["this"]), spread(us["parent"])
            res[f"decode_vs_parent_{n}"] = {"this": t, "parent": q, "parent_spread": q["max"] - q["min"],
                                           "slower_by_more_than_parent_spread": t["median"] - q["median"] > q["max"] - q["min"]}
        par.close()
    else:
        res["decode_vs_parent"] = "not taken: no --parent-lib"
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=12, help="queries per client seed")
    ap.add_argument("--seeds", type=int, default=2)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--max-db-gib", type=float, default=80.0, help="published sets whose one database instance is larger are left out and named")
    ap.add_argument("--only", default="", help="comma-separated set names")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    import torch

    torch.cuda.is_available()
    import spiral_amd as sa
    from spiral_amd import pack as _  # noqa: F401
    from spiral_amd import scheme as S

    sets = dict(EXTRA)
    for work, variants in S.PUBLISHED.items():
        for kind, prm_d in variants.items():
            sets[f"{work}:{kind}"] = (kind, prm_d)
    seeds = [bytes([17 + 40 * k] * 32) for k in range(a.seeds)]
    out = {"what": "response noise measured on the device against the true item, beside scheme.response_noise_model; ratios recorded, not judged",
           "device": torch.cuda.get_device_name(0), "queries_per_seed": a.queries, "seeds": a.seeds, "timing_runs": a.runs, "sets": {}, "left_out": {}, "timing_us": {}}
    for name, (kind, prm_d) in sets.items():
        if a.only and name not in a.only.split(","):
            out["left_out"][name] = "not selected by --only in this run"
            continue
        n = prm_d.get("n", 2)
        gib = (n * n if kind.endswith("-pack") else 4) * (1 << (prm_d["nu_1"] + prm_d["nu_2"])) * N * 8 / 2**30
        if gib > a.max_db_gib:
            out["left_out"][name] = f"one database instance takes {gib:.0f} GiB on the device, above --max-db-gib {a.max_db_gib:g}"
            continue
        try:
            res, prm, out_n, runs = measure(sa, S, name, kind, prm_d, seeds, a.queries)
        except (sa.SpiralGpuError, KeyError) as e:
            out["left_out"][name] = f"refused: {e}"
            continue
        out["sets"][name] = res
        if name in EXTRA:
            out["timing_us"][name] = timing(sa, prm, out_n, runs[0], seeds[0], a.runs, a.parent_lib)
            print(name, "timing", json.dumps(out["timing_us"][name]), flush=True)
        for r in runs:
            r[0].close()
        if a.out:
            with open(a.out, "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
