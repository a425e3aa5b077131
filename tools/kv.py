"""What the keyed-record calls cost against the routes that existed before them (include/spiral_gpu.h "Keyed records"), at configs[1] with 248-byte
values (32 slots per 8 KiB bucket), a table loaded to three quarters, in both image forms:

  1. kv_put of 1 and of 4096 new keys, against read_db_items_at of both candidate items of every key + the header scan, the placement rule and the
     splice on the host + update_db_items of the touched items;
  2. kv_get of 1 and of 4096 present keys, against read_db_items_at of both candidate items + the scan and the cut on the host;
  3. kv_decode of 1, 8 and 64 lookups (real responses of the server; every key present), against decode of the 2 n responses + the scan on the host.

Wall time of each route to completion, the two routes of a pair alternated in one process; medians of --reps repetitions with min and max.  The old
routes are given their hashes (tag, b1, b2 computed before the clock starts) and do their host work in numpy, with a Python loop only where the
placement rule is sequential; the new calls hash inside the call.  Between two timed puts the keys are deleted again (not timed), so every put places
new keys.  A figure slower than its reference point shows as a ratio above 1.

--parent=ROOT: also records that update_records, read_records_at and decode time the same from this tree's build as from the build of the parent
commit checked out (and built) at ROOT: fresh child processes of each tree taking turns, as tools/records.py does it.
usage: tools/kv.py [--reps=7] [--parent=ROOT [--parent-only]] [--out=FILE]          (prints one JSON document; --out also writes it)"""
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

CONFIG1 = dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256)  # bench.py WORKLOADS configs[1]
reps = int(opts.get("reps", 7))
V = 248
TK = bytes(range(16))


def stats(ms):
    return dict(median_ms=float(np.median(ms)), min_ms=float(min(ms)), max_ms=float(max(ms)))


def alternated(routes, between=None):
    """routes: name -> callable; each run once as a warm-up, then `reps` rounds in turn; between(): untimed, after every run"""
    ms = {k: [] for k in routes}
    for rep in range(reps + 1):
        for k, fn in routes.items():
            t0 = time.perf_counter()
            fn()
            if rep:
                ms[k].append((time.perf_counter() - t0) * 1e3)
            if between:
                between()
    out = {k: stats(v) for k, v in ms.items()}
    names = list(routes)
    out["ratio_new_over_reference"] = out[names[0]]["median_ms"] / out[names[1]]["median_ms"]
    return out


def params():
    kw = dict(CONFIG1)
    return sa.make_params(kw.pop("nu1"), kw.pop("nu2"), **kw)


def key_array(first, n):
    return np.frombuffer(b"".join(b"key-%08d" % i for i in range(first, first + n)), dtype=np.uint8).reshape(n, 12).copy()


def hashes(pg, keys):
    h = np.array([sa.kv_hash(pg, TK, bytes(k)) for k in keys], dtype=np.uint64)
    return h[:, 0], h[:, 1], h[:, 2]


class OldRoute:
    """put and get of keys through the item calls: both candidate items of every key to the host, the definition's scan, placement and splice there"""

    def __init__(self, srv, lay, tag, b1, b2):
        self.srv, self.lay, self.tag = srv, lay, tag
        self.items, at = np.unique(np.concatenate([b1, b2]), return_inverse=True)
        self.i1, self.i2 = at[:len(b1)], at[len(b1):]
        self.buf = np.zeros(len(self.items) * lay.item_bytes, dtype=np.uint8)

    def read(self):
        L = self.lay
        buf = self.srv.read_db_items_at(8, self.items, out=self.buf).reshape(len(self.items), L.item_bytes)
        heads = buf[:, :8 * L.slots].view("<u8")
        hit1, hit2 = heads[self.i1] == self.tag[:, None], heads[self.i2] == self.tag[:, None]
        return buf, heads, hit1, hit2

    def get(self, out):
        L = self.lay
        buf, _, hit1, hit2 = self.read()
        in1, in2 = hit1.any(axis=1), hit2.any(axis=1)
        item = np.where(in1, self.i1, self.i2)
        slot = np.where(in1, hit1.argmax(axis=1), hit2.argmax(axis=1))
        cols = (8 * L.slots + slot * V)[:, None] + np.arange(V)[None, :]
        found = in1 | in2
        out[found] = buf[item[:, None], cols][found]
        return np.where(in1, 1, np.where(in2, 2, 0)).astype(np.uint8)

    def put(self, values):
        L = self.lay
        buf, heads, hit1, hit2 = self.read()
        in1, in2 = hit1.any(axis=1), hit2.any(axis=1)
        item = np.where(in1, self.i1, self.i2)
        slot = np.where(in1, hit1.argmax(axis=1), hit2.argmax(axis=1))
        occ = (heads != 0).astype(np.uint64)
        masks = [int(x) for x in (occ << np.arange(L.slots, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)]  # one occupancy bitmap per item
        full = (1 << L.slots) - 1
        for k in np.flatnonzero(~(in1 | in2)).tolist():  # the placement rule, in the order of the call
            a, b = int(self.i1[k]), int(self.i2[k])
            ua, ub = bin(masks[a]).count("1"), bin(masks[b]).count("1")
            if ua >= L.slots and ub >= L.slots:
                raise RuntimeError(f"key {k} cannot be placed")
            i = b if ub < ua else a
            free = ~masks[i] & full
            s = (free & -free).bit_length() - 1
            masks[i] |= 1 << s
            item[k], slot[k] = i, s
        heads[item, slot] = self.tag
        buf[item[:, None], (8 * L.slots + slot * V)[:, None] + np.arange(V)[None, :]] = values
        self.srv.update_db_items(buf, 8, self.items)
        self.srv.sync()


def server_rows(pg, srv, lay, n_loaded):
    rng = np.random.default_rng(1)
    rows = []
    for form, fmt in (("packed", SV.DB_PACKED), ("limbs", SV.DB_LIMBS)):
        srv.set_db_format(fmt)
        for n in (1, 4096):
            new = key_array(n_loaded + 10_000, n)
            vals = rng.integers(0, 256, size=(n, V), dtype=np.uint8)
            old = OldRoute(srv, lay, *hashes(pg, new))

            def new_put():
                srv.kv_put(TK, new, vals)
                srv.sync()

            row = dict(form=form, n_keys=n, n_candidate_items=int(len(old.items)))
            row["put"] = alternated({"kv_put": new_put, "read_db_items_at+scan+place+splice+update_db_items": lambda: old.put(vals)},
                                    between=lambda: srv.kv_delete(TK, new, V))
            have = key_array(5000, n)
            oldg = OldRoute(srv, lay, *hashes(pg, have))
            out_new, out_old = np.zeros((n, V), dtype=np.uint8), np.zeros((n, V), dtype=np.uint8)
            found = {}

            def new_get():
                found["new"] = srv.kv_get(TK, have, V, out=out_new)[1]

            def old_get():
                found["old"] = oldg.get(out_old)

            row["get"] = alternated({"kv_get": new_get, "read_db_items_at+scan+cut": old_get})
            assert (found["new"] == found["old"]).all() and found["new"].all() and (out_new == out_old).all(), "the two routes return the same values"
            assert srv.db_format() == fmt
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def decode_rows(pg, srv, lay):
    cl = sa.Client(pg, bytes(range(32)))
    srv.set_pub_params(*cl.pub_params())
    rows = []
    keys = key_array(7000, 64)
    tag, _, _ = hashes(pg, keys)
    resp = np.stack([srv.answer(q)[1] for q in cl.kv_queries(TK, keys, "ntt")])  # [128][3][2][N]
    for n in (1, 8, 64):
        got = {}

        def new_decode():
            got["new"] = cl.kv_decode(TK, keys[:n], resp[:2 * n], V)

        def old_decode():
            plain = cl.decode(resp[:2 * n]).reshape(2 * n, -1).astype(np.uint8)  # (p_db = 256: a coefficient is a byte of the stream)
            heads = plain[:, :8 * lay.slots].view("<u8").reshape(n, 2, lay.slots)
            hit = heads == tag[:n, None, None]
            cand = np.where(hit[:, 0].any(axis=1), 0, 1)
            slot = hit[np.arange(n), cand].argmax(axis=1)
            found = hit.any(axis=(1, 2))
            vals = plain.reshape(n, 2, -1)[np.arange(n)[:, None], cand[:, None], (8 * lay.slots + slot * V)[:, None] + np.arange(V)[None, :]]
            got["old"] = (np.where(found[:, None], vals, 0).astype(np.uint8), np.where(found, cand + 1, 0).astype(np.uint8))

        row = dict(n_lookups=n, n_responses=2 * n)
        row["decode"] = alternated({"kv_decode": new_decode, "decode+scan+cut": old_decode})
        assert (got["new"][1] == got["old"][1]).all() and got["new"][1].all() and (got["new"][0] == got["old"][0]).all(), "the two routes return the same values"
        rows.append(row)
        print(json.dumps(row), flush=True)
    cl.close()
    return rows


def existing_calls():
    """the calls that existed before keyed records, at configs[1]: median wall ms of five runs each after a warm-up"""
    pg = params()
    rng = np.random.default_rng(5)
    lay = sa.record_layout(pg, 256)
    srv = sa.Server(pg)
    srv.gen_db(3)
    cl = sa.Client(pg, bytes(range(32)))
    ids = rng.choice(lay.capacity, size=4096, replace=False).astype(np.uint64)
    recs = rng.integers(0, 256, size=(4096, 256), dtype=np.uint8)
    resp = np.concatenate([rng.integers(0, int(cl.shape.qprime), size=(64, 1, 2, sa.N), dtype=np.uint64),
                           rng.integers(0, 4 * int(pg.p_db), size=(64, 2, 2, sa.N), dtype=np.uint64)], axis=1)
    out = np.zeros((4096, 256), dtype=np.uint8)

    def update(n):
        srv.update_records(recs[:n], 256, ids[:n])
        srv.sync()

    calls = {"update_records_1": lambda: update(1), "update_records_4096": lambda: update(4096),
             "read_records_at_1": lambda: srv.read_records_at(256, ids[:1], out=out[:1]), "read_records_at_4096": lambda: srv.read_records_at(256, ids, out=out),
             "decode_1": lambda: cl.decode(resp[:1]), "decode_64": lambda: cl.decode(resp)}
    res = {}
    for name, fn in calls.items():
        fn()
        ms = []
        for _ in range(5):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        res[name] = float(np.median(ms))
    cl.close()
    srv.close()
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
    rows = []
    for call in runs["tree"][0]:
        par, tree = [x[call] for x in runs["parent"]], [x[call] for x in runs["tree"]]
        row = dict(call=call, parent=stats(par), tree=stats(tree))
        row["tree_median_inside_parent_spread"] = bool(min(par) <= float(np.median(tree)) <= max(par))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def new_rows():
    pg = params()
    lay = sa.kv_layout(pg, V)
    n_loaded = int(lay.capacity) * 3 // 4
    rng = np.random.default_rng(0)
    srv = sa.Server(pg)
    t0 = time.perf_counter()
    srv.kv_load(TK, key_array(0, n_loaded), rng.integers(0, 256, size=(n_loaded, V), dtype=np.uint8))
    load_ms = (time.perf_counter() - t0) * 1e3
    rows = server_rows(pg, srv, lay, n_loaded) + decode_rows(pg, srv, lay)
    srv.close()
    return dict(slots=int(lay.slots), buckets=int(lay.buckets), keys_loaded=n_loaded, kv_load_ms=load_ms), rows


if __name__ == "__main__":
    assert sa.lib().spiral_gpu_device_count() > 0, "needs a GPU"
    if "existing" in opts:
        print(json.dumps(existing_calls()))
        sys.exit(0)
    table, rows = (None, []) if "parent-only" in opts else new_rows()
    res = dict(tool="tools/kv.py", reps=reps, value_bytes=V, config=CONFIG1, table=table, device=torch.cuda.get_device_name(0), rows=rows)
    if opts.get("parent"):
        res["existing_calls_against_the_parent_build"] = dict(reps=reps, order="which build's child goes first alternates from repetition to repetition",
                                                              rows=against_parent(opts["parent"]))
    text = json.dumps(res, indent=1)
    print(text)
    if "out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
        with open(opts["out"], "w") as f:
            f.write(text + "\n")
