"""What the SpiralPack record calls cost against the routes that existed before them (include/spiral_gpu.h "Records", SpiralPack), 256-byte records at
configs[4] (nu1 = 10, nu2 = 8, out_n = 4: 16 trial images, 32 KiB items) unless --nu / --outn say otherwise:

  1. update_records of one record and of 4096 scattered records, against one read_db_items_at per touched trial + a splice on the host + one
     update_db_items per touched trial;
  2. read_records_at of the same sets, against one read_db_items_at per touched trial + a cut on the host;
  3. decode_records of 1 and 8 responses, against decode + a cut on the host.

Wall time of each route to completion, the two routes of a pair alternated in one process; medians of --reps repetitions with min and max.  For the
update device events are taken too: `update_device` is the time between two events on the server's stream around update_records, beside the same
around the per-trial update_db_items calls of the old route (their bytes already read and spliced: the device part of the old route's last step
alone).  A figure slower than its reference point shows as a ratio above 1.

--parent=ROOT: also times pack_server_update_db_items, pack_server_read_db_items_at and decode from this tree's build and from the build of the
parent commit checked out (and built) at ROOT: fresh child processes, `--existing=ROOT` and `--existing=<this tree>` in turn, --reps of each; "same"
means this tree's median over its children lies inside the spread (min .. max) of the parent's children.
--parent-only: that comparison alone.
usage: tools/pack_records.py [--nu=10,8] [--outn=4] [--reps=7] [--parent=ROOT [--parent-only]] [--out=FILE]     (prints one JSON document)"""
import json
import os
import sys
import time

opts = dict((a[2:].split("=", 1) + [""])[:2] for a in sys.argv[1:] if a.startswith("--"))
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, opts.get("existing") or HERE)  # (--existing=ROOT: that tree's package and build)
import numpy as np
import torch  # (before the library initialises the device)

import spiral_amd as sa

NU1, NU2 = (int(x) for x in opts.get("nu", "10,8").split(","))
OUT_N = int(opts.get("outn", 4))
PARAMS = dict(t_gsw=8, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=20, p_db=256)  # bench.py --workload pack (configs[4])
reps = int(opts.get("reps", 7))
S, W, POLY = 256, 8, 2048  # record bytes, bits per coefficient, bytes per polynomial at 8 bits


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def alternated(routes):
    """routes: name -> callable; each run once as a warm-up, then `reps` rounds in turn"""
    for fn in routes.values():
        fn()
    ms = {k: [] for k in routes}
    for _ in range(reps):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            ms[k].append((time.perf_counter() - t0) * 1e3)
    out = {k: stats(v) for k, v in ms.items()}
    names = list(routes)
    out["ratio_new_over_reference"] = out[names[0]]["median_ms"] / out[names[1]]["median_ms"]
    return out


def server_rows():
    pg = sa.make_params(NU1, NU2, **PARAMS)
    lay = sa.record_layout(pg, S, OUT_N)
    rng = np.random.default_rng(4)
    srv = sa.PackServer(pg, OUT_N)
    srv.gen_db(3)  # (coefficients below 256: a record database)
    st = torch.cuda.Stream()
    srv.set_stream(st.cuda_stream)

    def device_ms(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        e0.record(st)
        fn()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1)

    rows = []
    for n in (1, 4096):
        ids = rng.choice(lay.capacity, size=n, replace=False).astype(np.uint64)
        recs = rng.integers(0, 256, size=(n, S), dtype=np.uint8)
        item, off = ids // lay.per_item, (ids % lay.per_item) * S  # a 256-byte record lies inside one polynomial: trial off // 2048
        trial = (off // POLY).astype(np.int64)
        groups = []  # per touched trial: its items, and where each record of the call lies in them
        for t in np.unique(trial):
            sel = np.nonzero(trial == t)[0]
            items, at = np.unique(item[sel], return_inverse=True)
            cols = (off[sel] % POLY).astype(np.int64)[:, None] + np.arange(S, dtype=np.int64)[None, :]
            groups.append((int(t), sel, items, at, cols))

        def new_update():
            srv.update_records(recs, S, ids)
            st.synchronize()

        def old_update():
            for t, sel, items, at, cols in groups:
                buf = srv.read_db_items_at(t, W, items).reshape(len(items), POLY)
                buf[at[:, None], cols] = recs[sel]
                srv.update_db_items(t, buf, W, items)
            st.synchronize()

        out = np.zeros((n, S), dtype=np.uint8)

        def old_read():
            for t, sel, items, at, cols in groups:
                buf = srv.read_db_items_at(t, W, items).reshape(len(items), POLY)
                out[sel] = buf[at[:, None], cols]

        row = dict(nu1=NU1, nu2=NU2, out_n=OUT_N, n_records=n, touched_trials=len(groups), touched_polynomials=int(sum(len(g[2]) for g in groups)))
        row["update"] = alternated({"update_records": new_update, "per-trial read_db_items_at+splice+update_db_items": old_update})
        spliced = []
        for t, sel, items, at, cols in groups:
            buf = srv.read_db_items_at(t, W, items).reshape(len(items), POLY)
            buf[at[:, None], cols] = recs[sel]
            spliced.append(buf)

        def old_scatter():
            for (t, sel, items, at, cols), buf in zip(groups, spliced):
                srv.update_db_items(t, buf, W, items)

        dev = {"update_records": [], "per-trial update_db_items": []}
        for rep in range(reps + 1):  # (the first round is the warm-up)
            for k, fn in (("update_records", lambda: srv.update_records(recs, S, ids)), ("per-trial update_db_items", old_scatter)):
                ms = device_ms(fn)
                if rep:
                    dev[k].append(ms)
        row["update_device"] = {k: stats(v) for k, v in dev.items()}
        got = np.zeros((n, S), dtype=np.uint8)
        row["read"] = alternated({"read_records_at": lambda: srv.read_records_at(S, ids, out=got), "per-trial read_db_items_at+cut": old_read})
        assert (got == recs).all() and (out == recs).all()
        rows.append(row)
        print(json.dumps(row), flush=True)
    srv.close()
    return rows


def decode_rows():
    pg = sa.make_params(NU1, NU2, **PARAMS)
    lay = sa.record_layout(pg, S, OUT_N)
    rng = np.random.default_rng(9)
    cl = sa.Client(pg, bytes(range(32)), out_n=OUT_N)
    rows = []
    for n in (1, 8):
        resp = np.concatenate([rng.integers(0, int(cl.shape.qprime), size=(n, 1, OUT_N, sa.N), dtype=np.uint64),
                               rng.integers(0, 4 * int(pg.p_db), size=(n, OUT_N, OUT_N, sa.N), dtype=np.uint64)], axis=1)
        ids = rng.choice(lay.capacity, size=n, replace=False)
        off = (ids % lay.per_item) * S

        def old_decode():
            pt = cl.decode(resp).reshape(n, -1).astype(np.uint8)  # (8-bit coefficients: the item's stream is its coefficients as bytes)
            return np.stack([pt[k, off[k]:off[k] + S] for k in range(n)])

        row = dict(nu1=NU1, nu2=NU2, out_n=OUT_N, n_responses=n)
        row["decode"] = alternated({"decode_records": lambda: cl.decode_records(resp, ids, S), "decode+cut": old_decode})
        assert (cl.decode_records(resp, ids, S) == old_decode()).all()
        rows.append(row)
        print(json.dumps(row), flush=True)
    cl.close()
    return rows


def existing_calls():
    """the calls that existed before the pack record store: median wall ms of five runs each after a warm-up"""
    pg = sa.make_params(NU1, NU2, **PARAMS)
    s = sa.get_pack_shape(pg, OUT_N)
    rng = np.random.default_rng(5)
    srv = sa.PackServer(pg, OUT_N)
    srv.gen_db(3)
    cl = sa.Client(pg, bytes(range(32)), out_n=OUT_N)
    ids = np.sort(rng.choice(s.dim0 * s.num_per, size=4096, replace=False)).astype(np.uint64)
    items = rng.integers(0, 256, size=(4096, POLY), dtype=np.uint8)
    resp = np.concatenate([rng.integers(0, int(cl.shape.qprime), size=(8, 1, OUT_N, sa.N), dtype=np.uint64),
                           rng.integers(0, 4 * int(pg.p_db), size=(8, OUT_N, OUT_N, sa.N), dtype=np.uint64)], axis=1)
    whole = np.zeros(4096 * POLY, dtype=np.uint8)
    st = torch.cuda.Stream()
    srv.set_stream(st.cuda_stream)

    def update(n):
        srv.update_db_items(1, items[:n], W, ids[:n])
        st.synchronize()

    calls = {"pack_update_db_items_1": lambda: update(1), "pack_update_db_items_4096": lambda: update(4096),
             "pack_read_db_items_at_1": lambda: srv.read_db_items_at(1, W, ids[:1], out=whole[:POLY]),
             "pack_read_db_items_at_4096": lambda: srv.read_db_items_at(1, W, ids, out=whole),
             "decode_1": lambda: cl.decode(resp[:1]), "decode_8": lambda: cl.decode(resp)}
    out = {}
    for name, fn in calls.items():
        fn()
        ms = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        out[name] = float(np.median(ms))
    cl.close()
    srv.close()
    return out


def against_parent(parent_root):
    """children of the two trees in turn, each a fresh process"""
    import subprocess

    runs = {"parent": [], "tree": []}
    env = {k: v for k, v in os.environ.items() if k != "SPIRAL_LIB"}
    for rep in range(reps):
        for name, root in (("parent", parent_root), ("tree", HERE))[:: 1 if rep % 2 == 0 else -1]:  # (which goes first alternates too)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing=" + os.path.abspath(root), f"--nu={NU1},{NU2}", f"--outn={OUT_N}"],
                               capture_output=True, text=True, env=env, timeout=600)
            if r.returncode != 0:
                raise RuntimeError(f"the {name} child failed: {r.stderr[-2000:]}")
            runs[name].append(json.loads(r.stdout.strip().splitlines()[-1]))
    rows = []
    for call in runs["tree"][0]:
        par, tree = [x[call] for x in runs["parent"]], [x[call] for x in runs["tree"]]
        row = dict(call=call, parent=stats(par), tree=stats(tree))
        row["tree_median_inside_parent_spread"] = bool(min(par) <= float(np.median(tree)) <= max(par))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


if __name__ == "__main__":
    assert sa.lib().spiral_gpu_device_count() > 0, "needs a GPU"
    if "existing" in opts:
        print(json.dumps(existing_calls()))
        sys.exit(0)
    res = dict(tool="tools/pack_records.py", reps=reps, record_bytes=S, nu1=NU1, nu2=NU2, out_n=OUT_N, device=torch.cuda.get_device_name(0),
               rows=[] if "parent-only" in opts else server_rows() + decode_rows())
    if opts.get("parent"):
        res["existing_calls_against_the_parent_build"] = dict(reps=reps, order="which build's child goes first alternates from repetition to repetition",
                                                              rows=against_parent(opts["parent"]))
    text = json.dumps(res, indent=1)
    print(text)
    if "out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
        with open(opts["out"], "w") as f:
            f.write(text + "\n")
