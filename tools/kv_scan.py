"""What listing a keyed table costs (include/spiral_gpu.h "Listing") against its floor and against the route that existed before it, on the tables of
tools/kv.py and tools/pack_kv.py: a base server at configs[1] with 248-byte values (32 slots, 786 432 keys) and a SpiralPack server at configs[4]
(out_n = 4) with 4088-byte values (8 slots, 1 048 576 keys), packed and limb planes.

  kv_scan count-only, kv_scan tags-only and kv_scan with values, against
  kv_stats of the same range -- the same gather with nothing listed: the floor -- and
  the old route: read_db_items of the range, the header scan and the compaction in numpy (SpiralPack: trial 0 for the tags, every trial for the values).

Tags and counts are measured on the whole table.  With values, the base table is listed whole; the SpiralPack table over --pack-value-buckets buckets
(default an eighth of it: the old route holds the range's image of every trial on the host).  Wall time of each route to completion, all routes of a
row alternated in one process; medians of --reps repetitions with min and max.  A figure slower than its reference shows as a ratio above 1.

--parent=ROOT: also records that kv_put, kv_get (1 and 4096 keys) and kv_stats (one bucket, the whole table) on the base table time the same from this
tree's build as from the build of the parent commit checked out (and built) at ROOT: fresh child processes of each tree taking turns.
usage: tools/kv_scan.py [--reps=7] [--only=base|pack] [--parent=ROOT [--parent-only]] [--out=FILE]      (prints one JSON document; --out also writes it)"""
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

P = sys.modules["spiral_amd.pack"]
CONFIG1 = dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256)  # bench.py WORKLOADS configs[1]
PACK = dict(t_gsw=8, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=20, p_db=256)  # bench.py --workload pack (configs[4])
NU1, NU2, OUT_N = 10, 8, 4
reps = int(opts.get("reps", 7))
TK = bytes(range(16))
POLY = 2048  # bytes per polynomial at 8 bits per coefficient


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def alternated(routes):
    """routes: name -> callable; each run once as a warm-up, then `reps` rounds in turn"""
    ms = {k: [] for k in routes}
    for rep in range(reps + 1):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                ms[k].append((time.perf_counter() - t0) * 1e3)
    return {k: stats(v) for k, v in ms.items()}


def key_array(first, n):
    return np.frombuffer(b"".join(b"key-%08d" % i for i in range(first, first + n)), dtype=np.uint8).reshape(n, 12).copy()


def values_of(first, n, width):
    """counter-based values: row i is a function of first + i alone (a whole table's values without a generator's state)"""
    out = np.empty((n, width), dtype=np.uint8)
    c = (np.arange(width, dtype=np.uint32) * np.uint32(2246822519))[None, :]
    for r0 in range(0, n, 1 << 15):  # (in blocks: the 32-bit intermediates of a whole table would not fit)
        i = np.arange(first + r0, first + min(r0 + (1 << 15), n), dtype=np.uint64).astype(np.uint32)[:, None]
        out[r0:r0 + len(i)] = ((i * np.uint32(2654435761) + c) >> np.uint32(24)).astype(np.uint8)
    return out


def old_route(read_trial, trials, lay, V, first, n, values):
    """read_db_items of the range, then the definition on the host: the header scan, np.nonzero's bucket-major compaction, the value cut"""
    n_polys = trials if values else 1
    img = np.empty((n, n_polys * POLY), dtype=np.uint8)
    for t in range(n_polys):
        img[:, t * POLY:(t + 1) * POLY] = read_trial(t, first, n).reshape(n, POLY)
    heads = img[:, :8 * lay.slots].view("<u8")
    b, s = np.nonzero(heads)
    tags = heads[b, s]
    vals = img[:, 8 * lay.slots:8 * lay.slots + lay.slots * V].reshape(n, lay.slots, V)[b, s] if values else None
    return tags, (b + first).astype(np.uint32), s.astype(np.uint32), vals


def scan_rows(kind, srv, read_trial, trials, lay, V, forms, value_buckets):
    nb = int(lay.buckets)
    rows = []
    for form, fmt in forms:
        srv.set_db_format(fmt)
        got = {}
        whole = dict(kv_stats=lambda: got.__setitem__("stats", srv.kv_stats(V)),
                     kv_scan_count_only=lambda: got.__setitem__("count", count_only(srv, V, nb)),
                     kv_scan_tags=lambda: got.__setitem__("tags", srv.kv_scan(V, values=False, max_entries=got["count"])),
                     old_tags=lambda: got.__setitem__("old_tags", old_route(read_trial, trials, lay, V, 0, nb, False)))
        row = dict(server=kind, form=form, buckets=nb, slots=int(lay.slots), value_bytes=V, whole_table=alternated(whole))
        new, old = got["tags"], got["old_tags"]
        assert got["count"] == got["stats"].used == len(new) == len(old[0]), "the routes count the same entries"
        assert (new.tags == old[0]).all() and (new.buckets == old[1]).all() and (new.slots == old[2]).all(), "the routes list the same entries"
        row["entries"] = int(got["count"])
        vb = nb if value_buckets is None else value_buckets
        n_val = count_only(srv, V, vb)
        valued = dict(kv_stats=lambda: srv.kv_stats(V, 0, vb),
                      kv_scan_values=lambda: got.__setitem__("vals", srv.kv_scan(V, 0, vb, values=True, max_entries=n_val)),
                      old_values=lambda: got.__setitem__("old_vals", old_route(read_trial, trials, lay, V, 0, vb, True)))
        row["with_values"] = dict(buckets=vb, entries=int(n_val), value_megabytes=n_val * V / 1e6, **alternated(valued))
        assert (got["vals"].tags == got["old_vals"][0]).all() and (got["vals"].values == got["old_vals"][3]).all(), "the routes return the same values"
        w, wv = row["whole_table"], row["with_values"]
        row["ratios"] = {"count_only / kv_stats": w["kv_scan_count_only"]["median_ms"] / w["kv_stats"]["median_ms"],
                         "tags / kv_stats": w["kv_scan_tags"]["median_ms"] / w["kv_stats"]["median_ms"],
                         "tags / old route": w["kv_scan_tags"]["median_ms"] / w["old_tags"]["median_ms"],
                         "values / kv_stats": wv["kv_scan_values"]["median_ms"] / wv["kv_stats"]["median_ms"],
                         "values / old route": wv["kv_scan_values"]["median_ms"] / wv["old_values"]["median_ms"]}
        assert srv.db_format() == fmt
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def count_only(srv, V, n_buckets):
    """the C call's count-only form (max_entries = 0, no buffers)"""
    import ctypes as C

    n = C.c_uint64()
    fn = sa.lib().spiral_gpu_pack_server_kv_scan if isinstance(srv, sa.PackServer) else sa.lib().spiral_gpu_server_kv_scan
    if fn(srv.h, V, 0, n_buckets, None, None, 0, C.byref(n)) != 0:
        raise RuntimeError(sa.lib().spiral_gpu_last_error().decode())
    return n.value


def base_table():
    kw = dict(CONFIG1)
    pb = sa.make_params(kw.pop("nu1"), kw.pop("nu2"), **kw)
    lb = sa.kv_layout(pb, 248)
    n_loaded = int(lb.capacity) * 3 // 4
    base = sa.Server(pb)
    base.kv_load(TK, key_array(0, n_loaded), values_of(0, n_loaded, 248))
    return pb, lb, n_loaded, base


def new_rows():
    rows, tables = [], {}
    if opts.get("only") in (None, "base"):
        pb, lb, n_loaded, base = base_table()
        tables["base configs[1]"] = dict(slots=int(lb.slots), buckets=int(lb.buckets), keys_loaded=n_loaded)
        # (a base item is 4 polynomials in one image: read_db_items returns them together, so the old route reads whole items for the tags too)
        rows += scan_rows("base configs[1]", base, BaseReader(base), 4, lb, 248, [("packed", SV.DB_PACKED), ("limbs", SV.DB_LIMBS)], None)
        base.close()
    if opts.get("only") in (None, "pack"):
        pg = sa.make_params(NU1, NU2, **PACK)
        lay = sa.pack_kv_layout(pg, OUT_N, 4088)
        n_loaded = int(lay.capacity) // 2
        srv = sa.PackServer(pg, OUT_N)
        srv.kv_load(TK, key_array(0, n_loaded), values_of(0, n_loaded, 4088))
        tables["pack configs[4]"] = dict(slots=int(lay.slots), buckets=int(lay.buckets), keys_loaded=n_loaded, out_n=OUT_N)
        forms = [("packed", P.DB_PACKED)] + ([("limbs", P.DB_LIMBS)] if P.has_limb_form(pg, OUT_N) else [])
        vb = int(opts.get("pack-value-buckets", int(lay.buckets) // 8))
        rows += scan_rows("pack configs[4]", srv, lambda t, first, n: srv.read_db_items(t, 8, first, n), OUT_N * OUT_N, lay, 4088, forms, vb)
        srv.close()
    return tables, rows


class BaseReader:
    """the base server's old route reads whole items (4 polynomials, one image): one read_db_items serves every `trial` of a call"""

    def __init__(self, srv):
        self.srv, self.buf = srv, None

    def __call__(self, t, first, n):
        if t == 0:
            self.buf = self.srv.read_db_items(8, first, n).reshape(n, 4 * POLY)
        return self.buf[:, t * POLY:(t + 1) * POLY]


def existing_calls():
    """calls that existed before the listing, on the base table at configs[1]: median wall ms of five runs each after a warm-up"""
    pb, lb, n_loaded, base = base_table()
    have, new, vals = key_array(5000, 4096), key_array(n_loaded + 10_000, 4096), values_of(1, 4096, 248)
    out = np.zeros((4096, 248), dtype=np.uint8)

    def put(n):
        base.kv_put(TK, new[:n], vals[:n])  # (the first run inserts, the timed ones overwrite: the same probe and the same write)
        base.sync()

    calls = {"kv_put_1": lambda: put(1), "kv_put_4096": lambda: put(4096), "kv_get_1": lambda: base.kv_get(TK, have[:1], 248, out=out[:1]),
             "kv_get_4096": lambda: base.kv_get(TK, have, 248, out=out), "kv_stats_1_bucket": lambda: base.kv_stats(248, 77, 1),
             "kv_stats_4096_buckets": lambda: base.kv_stats(248, 77, 4096), "kv_stats_whole_table": lambda: base.kv_stats(248)}
    res = {}
    for name, fn in calls.items():
        fn()
        ms = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        res[name] = float(np.median(ms))
    base.close()
    return res


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
            print(f"repetition {rep}: the {name} build's child is done", file=sys.stderr, flush=True)
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
    tables, rows = (None, []) if "parent-only" in opts else new_rows()
    res = dict(tool="tools/kv_scan.py", reps=reps, tables=tables, device=torch.cuda.get_device_name(0), rows=rows)
    if opts.get("parent"):
        res["existing_calls_against_the_parent_build"] = dict(reps=reps, order="which build's child goes first alternates from repetition to repetition",
                                                              rows=against_parent(opts["parent"]))
    text = json.dumps(res, indent=1)
    print(text)
    if "out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
        with open(opts["out"], "w") as f:
            f.write(text + "\n")
