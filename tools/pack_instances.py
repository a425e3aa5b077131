"""SpiralPack items of several database instances (spiral_gpu_pack_server_answer_batch_instances) at the parameter selector's picks: per geometry one
B = 1 item call against F separate answer calls on the same handles with the same query and against the selector's predicted_total_us; items/s at
B = 2, 4, 8 (with the repetitions' spread) and the shared first-dimension pass alone; groups of one (option pack_item_group = 1) against automatic grouping.  Every shape is warmed up first, the compared forms alternate within
the process, device-event times (the call's total_us, each answer's total_us).  Synthetic keys, queries and databases (uniform residues): timing only.

    python tools/pack_instances.py [--reps 5] [--geoms pack14,stream12,config5] [--out profiles/pack_instances.json]
    python tools/pack_instances.py --trace answer|item      (one small answer, or one small B = 1 item of F = 3: what a kernel trace counts)

Prints one JSON line (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# name: (nu1, nu2, out_n, params, F, the selector's predicted_total_us and its expansion + conversion stage, what it is)
GEOMS = {
    "pack14": (10, 4, 12, dict(t_gsw=16, t_conv=4, t_exp=56, t_exp_right=56, qprime_bits=23, p_db=1024), 3, 20125.7, 1316.4 + 32.1,
               "scheme --select 14,1000000 --variant spiral-pack --one-gpu (first pick, 101 GB)"),
    "stream12": (9, 3, 10, dict(t_gsw=3, t_conv=56, t_exp=56, t_exp_right=56, qprime_bits=32, p_db=1 << 20, direct_upload=1), 8, 11986.9, 10.9,
                 "scheme --select 12,4000000 --variant spiralstream-pack --one-gpu (first pick, 47 GB)"),
    "config5": (10, 8, 4, dict(t_gsw=8, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=20, p_db=256), 3, None, None,
                "BASELINE.json configs[4]'s geometry (bench.py --workload pack), three instances (~180 GB)"),
    "small": (6, 2, 2, {}, 3, None, None, "a small geometry (the kernel trace)"),
}


def synth(rng, sa, shape):
    return np.stack([rng.integers(0, m, size=shape + (sa.N,), dtype=np.uint64) for m in (sa.P, sa.B)], axis=-2)


def setup(sa, name, n_clients, seed=1):
    nu1, nu2, out_n, kw, F = GEOMS[name][:5]
    pg = sa.make_params(nu1, nu2, **kw)
    shp = sa.get_pack_shape(pg, out_n)
    instances = []
    for k in range(F):
        srv = sa.PackServer(pg, out_n)
        srv.fill_db_random(1000 + k)
        instances.append(srv)
    servers = [instances[0]] + [instances[0].create_lane() for _ in range(n_clients - 1)]
    rng = np.random.default_rng(seed)
    pps, qs = [], []
    for srv in servers:
        pp = (synth(rng, sa, (max(shp.n_left, 1), 2, pg.t_exp)), synth(rng, sa, (max(shp.n_right, 1), 2, pg.t_exp_right)), synth(rng, sa, (2, 2 * pg.t_conv)),
              synth(rng, sa, (out_n, out_n + 1, pg.t_conv)))
        srv.set_pub_params(*pp)
        pps.append(pp)
        qs.append(synth(rng, sa, (shp.n_query_cts, 2)))
    for inst in instances[1:]:  # the instances answer client 0 alone too (the F separate calls)
        inst.set_pub_params(*pps[0])
    return pg, shp, instances, servers, qs


def set_group(sa, g):
    assert sa.lib().spiral_gpu_set_option(b"pack_item_group", g) == 0


def measure(sa, P, name, reps):
    nu1, nu2, out_n, kw, F, predicted, exp_conv_pred, what = GEOMS[name]
    bmax = 8
    t_setup = time.perf_counter()
    pg, shp, instances, servers, qs = setup(sa, name, bmax)
    r = dict(geometry=dict(nu1=nu1, nu2=nu2, out_n=out_n, F=F, **kw), what=what, predicted_total_us=predicted,
             device_db_bytes=sum(i.db_device_bytes() for i in instances), setup_s=round(time.perf_counter() - t_setup, 1))

    def item(B):
        st = {}
        P.answer_batch_instances(servers[:B], instances, qs[:B], stats=st)
        return st["total_us"]

    def singles():
        us = [inst.answer(qs[0], want_packed=False)[2] for inst in instances]
        return sum(u["total_us"] for u in us), us[0]["expansion_us"] + us[0]["conversion_us"]

    # B = 1 on the images as loaded (packed): item vs F answers, groups of one vs automatic, alternating
    item(1), singles()
    set_group(sa, 1), item(1), set_group(sa, 0)
    rows = []
    for _ in range(reps):
        a = item(1)
        s, ec = singles()
        set_group(sa, 1)
        g1 = item(1)
        set_group(sa, 0)
        rows.append((a, s, ec, g1))
    a, s, ec, g1 = (float(np.median([x[i] for x in rows])) for i in range(4))
    r["b1"] = dict(item_us=a, singles_sum_us=s, expansion_conversion_us=ec, bound_us=s - (F - 1) * ec, item_le_bound=a <= s - (F - 1) * ec,
                   item_vs_predicted=(a / predicted if predicted else None), group1_us=g1, auto_no_slower=a <= g1 * 1.02,
                   spread_item_us=[min(x[0] for x in rows), max(x[0] for x in rows)], spread_singles_us=[min(x[1] for x in rows), max(x[1] for x in rows)])
    # batches (a covered geometry converts the instance images to limb planes on the first): items/s, automatic groups vs groups of one
    for B in (2, 4, 8):
        item(B)
    set_group(sa, 1), item(8), set_group(sa, 0)
    per = {B: [] for B in (1, 2, 4, 8)}
    g8 = []
    for _ in range(reps):
        for B in (1, 2, 4, 8):
            per[B].append(item(B))
        set_group(sa, 1)
        g8.append(item(8))
        set_group(sa, 0)
    r["batches"] = {str(B): dict(call_us=float(np.median(v)), items_per_s=B / float(np.median(v)) * 1e6, spread_call_us=[min(v), max(v)]) for B, v in per.items()}
    # the shared first-dimension pass alone over instance 0's images (time_sweep_batch; the matrix-core pass where the geometry has limb planes)
    r["shared_pass_ms"] = {str(B): float(np.median([P.time_sweep_batch(servers[:B], 3) for _ in range(reps)])) for B in (1, 2, 4, 8)}
    r["batches"]["8_group1_call_us"] = float(np.median(g8))
    r["b8_vs_8x_b1"] = r["batches"]["8"]["items_per_s"] / (8 * r["batches"]["1"]["items_per_s"])
    r["image_form_after"] = [i.db_format() for i in instances]
    for srv in servers[1:] + instances:
        srv.close()
    return r


def trace(sa, P, which):
    pg, shp, instances, servers, qs = setup(sa, "small", 1)
    if which == "answer":
        instances[0].answer(qs[0], want_packed=False)
    else:
        P.answer_instances(servers[0], instances, qs[0])
    for srv in instances:
        srv.close()
    print(json.dumps(dict(trace=which, F=len(instances))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--geoms", default="pack14,stream12,config5")
    ap.add_argument("--trace", choices=["answer", "item"], default=None)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    torch.cuda.is_available()
    import spiral_amd as sa

    P = sys.modules["spiral_amd.pack"]
    if args.trace:
        return trace(sa, P, args.trace)
    out = dict(tool="tools/pack_instances.py", reps=args.reps, results={})
    for name in args.geoms.split(","):
        try:
            out["results"][name] = measure(sa, P, name, args.reps)
        except Exception as e:  # (an instance set that does not fit is recorded, not fatal)
            out["results"][name] = dict(error=f"{type(e).__name__}: {e}")
            import gc

            gc.collect()
        print(json.dumps({name: out["results"][name]}), flush=True)
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
