"""What the record calls cost against the routes that existed before them (include/spiral_gpu.h "Records"), 256-byte records at configs[1] (and the
update also at configs[2]):

  1. update_records of one record and of 4096 scattered records, against read_db_items_at of the containing items + a splice on the host +
     update_db_items of those items;
  2. read_records_at of the same sets, against read_db_items_at of the containing items;
  3. decode_records of 1, 8 and 64 responses, against decode.

Wall time of each route to completion (the call or calls, then a synchronisation of the server's stream where a call is asynchronous), the two routes
of a pair alternated in one process; medians of --reps repetitions with min and max.  For the asynchronous calls device events are taken too, as
tools/db_update.py takes them: `update_device` is the time between two events on the server's stream around update_records, beside the same around
update_db_items of the containing items (their bytes already read and spliced: the device part of the old route's last step alone).  The reference point of every figure is the existing call in the
same process; a figure slower than its reference point shows as a ratio above 1.

--parent=ROOT: also records that update_db_items, read_db_items_at and decode time the same from this tree's build as from the build of the parent
commit checked out (and built) at ROOT: fresh child processes, `--existing=ROOT` and `--existing=<this tree>` in turn, --reps of each; every child
imports the package of its own tree (SPIRAL_LIB unset), times each call five times after a warm-up and reports the median; "same" means this tree's
median over its children lies inside the spread (min .. max) of the parent's children.
(Not one process through SPIRAL_LIB: the package refuses a library that lacks a declared entry point, and the parent's build has none of the record
calls; each tree's children therefore load their own package and library, and the children of the two trees take turns.)
--parent-only: that comparison alone.
usage: tools/records.py [--configs=1,2] [--reps=7] [--parent=ROOT [--parent-only]] [--out=FILE]          (prints one JSON document; --out also writes it)"""
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
from spiral_amd import server as SV

CONFIGS = {  # bench.py WORKLOADS configs[1] / configs[2]
    1: dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256),
    2: dict(nu1=9, nu2=10, t_gsw=10, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=22, p_db=256),
}
which = [int(c) for c in opts.get("configs", "1,2").split(",")]
reps = int(opts.get("reps", 7))
S = 256


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


def params_of(cfg):
    kw = dict(CONFIGS[cfg])
    return sa.make_params(kw.pop("nu1"), kw.pop("nu2"), **kw)


def server_rows(cfg):
    pg = params_of(cfg)
    lay = sa.record_layout(pg, S)
    rng = np.random.default_rng(cfg)
    srv = sa.Server(pg)
    srv.gen_db(3)  # (coefficients below 256: a record database)
    st = torch.cuda.Stream()
    srv.set_stream(st.cuda_stream)

    def device_ms(fn):
        """device ms between two events on the server's stream around fn"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        e0.record(st)
        fn()
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1)

    rows = []
    for form, fmt in (("packed", SV.DB_PACKED), ("limbs", SV.DB_LIMBS)):
        srv.set_db_format(fmt)
        for n in (1, 4096):
            ids = rng.choice(lay.capacity, size=n, replace=False).astype(np.uint64)
            recs = rng.integers(0, 256, size=(n, S), dtype=np.uint8)
            items, at = np.unique(ids // lay.per_item, return_inverse=True)
            cols = ((ids % lay.per_item) * S).astype(np.int64)[:, None] + np.arange(S, dtype=np.int64)[None, :]

            def new_update():
                srv.update_records(recs, S, ids)
                srv.sync()

            def old_update():
                buf = srv.read_db_items_at(8, items).reshape(len(items), lay.item_bytes)
                buf[at[:, None], cols] = recs
                srv.update_db_items(buf, 8, items)
                srv.sync()

            row = dict(config=cfg, form=form, n_records=n, n_items=int(len(items)))
            row["update"] = alternated({"update_records": new_update, "read_db_items_at+splice+update_db_items": old_update})
            spliced = srv.read_db_items_at(8, items).reshape(len(items), lay.item_bytes)
            spliced[at[:, None], cols] = recs
            dev = {"update_records": [], "update_db_items": []}
            for rep in range(reps + 1):  # (the first round is the warm-up)
                for k, fn in (("update_records", lambda: srv.update_records(recs, S, ids)), ("update_db_items", lambda: srv.update_db_items(spliced, 8, items))):
                    ms = device_ms(fn)
                    if rep:
                        dev[k].append(ms)
            row["update_device"] = {k: stats(v) for k, v in dev.items()}
            assert srv.db_format() == fmt
            if cfg == 1:
                out = np.zeros((n, S), dtype=np.uint8)
                whole = np.zeros(len(items) * lay.item_bytes, dtype=np.uint8)
                row["read"] = alternated({"read_records_at": lambda: srv.read_records_at(S, ids, out=out),
                                          "read_db_items_at": lambda: srv.read_db_items_at(8, items, out=whole)})
                assert (out == recs).all()
            rows.append(row)
            print(json.dumps(row), flush=True)
    srv.close()
    return rows


def decode_rows():
    pg = params_of(1)
    lay = sa.record_layout(pg, S)
    rng = np.random.default_rng(9)
    cl = sa.Client(pg, bytes(range(32)))
    rows = []
    for n in (1, 8, 64):
        resp = np.concatenate([rng.integers(0, int(cl.shape.qprime), size=(n, 1, 2, sa.N), dtype=np.uint64),
                               rng.integers(0, 4 * int(pg.p_db), size=(n, 2, 2, sa.N), dtype=np.uint64)], axis=1)
        ids = rng.choice(lay.capacity, size=n, replace=False)
        row = dict(config=1, n_responses=n)
        row["decode"] = alternated({"decode_records": lambda: cl.decode_records(resp, ids, S), "decode": lambda: cl.decode(resp)})
        rows.append(row)
        print(json.dumps(row), flush=True)
    cl.close()
    return rows


def existing_calls():
    """the calls that existed before the record store, at configs[1]: median wall ms of five runs each after a warm-up"""
    pg = params_of(1)
    s = sa.get_shape(pg)
    rng = np.random.default_rng(5)
    srv = sa.Server(pg)
    srv.gen_db(3)
    cl = sa.Client(pg, bytes(range(32)))
    ids = np.sort(rng.choice(s.dim0 * s.num_per, size=4096, replace=False)).astype(np.uint64)
    items = rng.integers(0, 256, size=(4096, 8192), dtype=np.uint8)
    resp = np.concatenate([rng.integers(0, int(cl.shape.qprime), size=(64, 1, 2, sa.N), dtype=np.uint64),
                           rng.integers(0, 4 * int(pg.p_db), size=(64, 2, 2, sa.N), dtype=np.uint64)], axis=1)
    whole = np.zeros(4096 * 8192, dtype=np.uint8)

    def update(n):
        srv.update_db_items(items[:n], 8, ids[:n])
        srv.sync()

    calls = {"update_db_items_1": lambda: update(1), "update_db_items_4096": lambda: update(4096),
             "read_db_items_at_1": lambda: srv.read_db_items_at(8, ids[:1], out=whole[:8192]), "read_db_items_at_4096": lambda: srv.read_db_items_at(8, ids, out=whole),
             "decode_1": lambda: cl.decode(resp[:1]), "decode_64": lambda: cl.decode(resp)}
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
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing=" + os.path.abspath(root)], capture_output=True, text=True, env=env, timeout=300)
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
    res = dict(tool="tools/records.py", reps=reps, record_bytes=S, device=torch.cuda.get_device_name(0), library=os.environ.get("SPIRAL_LIB", "this tree's"),
               rows=[] if "parent-only" in opts else [r for c in which for r in server_rows(c)] + decode_rows())
    if opts.get("parent"):
        res["existing_calls_against_the_parent_build"] = dict(reps=reps, order="which build's child goes first alternates from repetition to repetition",
                                                              rows=against_parent(opts["parent"]))
    text = json.dumps(res, indent=1)
    print(text)
    if "out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
        with open(opts["out"], "w") as f:
            f.write(text + "\n")
