"""What keyed records on a SpiralPack server and kv_stats cost against the routes that existed before them (include/spiral_gpu.h "Keyed records",
SpiralPack), at configs[4] (nu1 = 10, nu2 = 8, out_n = 4: 16 trial images, 32 KiB buckets) with 4088-byte values (8 slots per bucket), the table
loaded to --load of its capacity (default 0.5: at 0.75 kv_load refuses this key set -- key 1 479 680 of 1 572 864 finds both its buckets full, a load of
0.706 --, which is why the run is not at the 0.75 of the base server's tool), in both image forms:

  1. kv_put of 1 and of 4096 new keys, against: read_db_items_at of trial 0 of both candidate items of every key + header scan and placement rule on
     the host, then per touched trial read_db_items_at + splice + update_db_items;
  2. kv_get of 1 and of 4096 present keys, against: read_db_items_at of trial 0 of both candidate items + scan, then per touched trial
     read_db_items_at + cut;
  3. kv_decode of 1, 8 and 64 lookups (real responses of the server; every key present), against decode of the 2 n responses + scan and cut on the host;
  4. kv_stats of the whole table, on a base server at configs[1] (V = 248) and on the SpiralPack server, against kv_get of absent keys whose candidate
     buckets number about as many (the probe alone: nothing is found, nothing read) and against fingerprint_items of the same image (the same gather and
     transform, over every polynomial instead of one).

Wall time of each route to completion, the routes of a pair alternated in one process; medians of --reps repetitions with min and max.  The old
routes are given their hashes (computed before the clock starts); the new calls hash inside the call.  Between two timed puts the keys are deleted
again (not timed).  A figure slower than its reference point shows as a ratio above 1.

--parent=ROOT: also records that kv_put / kv_get / kv_decode on a base server (configs[1]) and update_records / read_records_at on a SpiralPack server
(--nu / --outn) time the same from this tree's build as from the build of the parent commit checked out (and built) at ROOT: fresh child processes of
each tree taking turns.
usage: tools/pack_kv.py [--reps=7] [--load=0.5] [--nu=10,8] [--outn=4] [--value-bytes=4088] [--parent=ROOT [--parent-only]] [--out=FILE]   (prints one JSON document)"""
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
NU1, NU2 = (int(x) for x in opts.get("nu", "10,8").split(","))
OUT_N = int(opts.get("outn", 4))
PACK = dict(t_gsw=8, t_conv=4, t_exp=16, t_exp_right=56, qprime_bits=20, p_db=256)  # bench.py --workload pack (configs[4])
CONFIG1 = dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256)  # bench.py WORKLOADS configs[1]
reps = int(opts.get("reps", 7))
V = int(opts.get("value-bytes", 4088))
LOAD = float(opts.get("load", 0.5))
TK = bytes(range(16))
POLY = 2048  # bytes per polynomial at 8 bits per coefficient


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
    out["ratio_new_over_reference"] = {n: out[names[0]]["median_ms"] / out[n]["median_ms"] for n in names[1:]}
    return out


def key_array(first, n):
    return np.frombuffer(b"".join(b"key-%08d" % i for i in range(first, first + n)), dtype=np.uint8).reshape(n, 12).copy()


def hashes(pg, keys, out_n):
    h = np.array([sa.kv_hash(pg, TK, bytes(k), out_n=out_n) for k in keys], dtype=np.uint64)
    return h[:, 0], h[:, 1], h[:, 2]


def values_of(first, n, width):
    """counter-based values: row i is a function of first + i alone (a whole table's values without a generator's state)"""
    out = np.empty((n, width), dtype=np.uint8)
    c = (np.arange(width, dtype=np.uint32) * np.uint32(2246822519))[None, :]
    for r0 in range(0, n, 1 << 15):  # (in blocks: the 32-bit intermediates of a whole table would not fit)
        i = np.arange(first + r0, first + min(r0 + (1 << 15), n), dtype=np.uint64).astype(np.uint32)[:, None]
        out[r0:r0 + len(i)] = ((i * np.uint32(2654435761) + c) >> np.uint32(24)).astype(np.uint8)
    return out


def spans(rows, a, b, at):
    """index arrays for copying byte ranges [a[k], b[k]) of row rows[k] of a polynomial buffer to / from bytes [at[k], ...) of value k: (row, column,
    value row, value column), one entry per byte"""
    n = (b - a).astype(np.int64)
    start = np.cumsum(n) - n
    step = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(start, n)
    return np.repeat(rows, n), np.repeat(a, n) + step, np.repeat(np.arange(len(n)), n), np.repeat(at, n) + step


class OldRoute:
    """put and get of keys through the per-trial item calls: trial 0 of both candidate items of every key to the host, the definition's scan and
    placement there, then the trials the values lie in, one read (and one update) per touched trial"""

    def __init__(self, srv, sync, lay, tag, b1, b2):
        self.srv, self.sync, self.lay, self.tag = srv, sync, lay, tag
        self.items, at = np.unique(np.concatenate([b1, b2]), return_inverse=True)
        self.i1, self.i2 = at[:len(b1)], at[len(b1):]

    def heads(self):
        L = self.lay
        buf = self.srv.read_db_items_at(0, 8, self.items).reshape(len(self.items), POLY)
        heads = buf[:, :8 * L.slots].view("<u8")
        return buf, heads, heads[self.i1] == self.tag[:, None], heads[self.i2] == self.tag[:, None]

    def pieces(self, item, slot):
        """per trial t that holds value bytes: (t, the keys with bytes there, their byte range in the polynomial, where it starts in the value)"""
        v0 = 8 * self.lay.slots + slot.astype(np.int64) * V
        for t in range(int(v0.min()) // POLY, (int(v0.max()) + V - 1) // POLY + 1):
            lo, hi = np.maximum(v0, t * POLY), np.minimum(v0 + V, (t + 1) * POLY)
            sel = np.flatnonzero(lo < hi)
            if len(sel):
                yield t, sel, lo[sel] - t * POLY, hi[sel] - t * POLY, lo[sel] - v0[sel]

    def get(self, out):
        buf0, _, hit1, hit2 = self.heads()
        in1, in2 = hit1.any(axis=1), hit2.any(axis=1)
        found = np.flatnonzero(in1 | in2)
        item, slot = np.where(in1, self.i1, self.i2)[found], np.where(in1, hit1.argmax(axis=1), hit2.argmax(axis=1))[found]
        for t, sel, a, b, at in self.pieces(item, slot):
            if t == 0:  # (read already)
                buf, rows = buf0, item[sel]
            else:
                ids, rows = np.unique(self.items[item[sel]], return_inverse=True)
                buf = self.srv.read_db_items_at(t, 8, ids).reshape(len(ids), POLY)
            r, c, k, z = spans(rows, a, b, at)
            out[found[sel][k], z] = buf[r, c]
        return np.where(in1, 1, np.where(in2, 2, 0)).astype(np.uint8)

    def put(self, values):
        L = self.lay
        buf0, heads, hit1, hit2 = self.heads()
        in1, in2 = hit1.any(axis=1), hit2.any(axis=1)
        item, slot = np.where(in1, self.i1, self.i2), np.where(in1, hit1.argmax(axis=1), hit2.argmax(axis=1))
        occ = (heads != 0).astype(np.uint64)
        masks = [int(x) for x in (occ << np.arange(L.slots, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)]  # one occupancy bitmap per item
        full = (1 << L.slots) - 1
        for k in np.flatnonzero(~(in1 | in2)).tolist():  # the placement rule, in the order of the call
            x, y = int(self.i1[k]), int(self.i2[k])
            ux, uy = bin(masks[x]).count("1"), bin(masks[y]).count("1")
            if ux >= L.slots and uy >= L.slots:
                raise RuntimeError(f"key {k} cannot be placed")
            i = y if uy < ux else x
            free = ~masks[i] & full
            s = (free & -free).bit_length() - 1
            masks[i] |= 1 << s
            item[k], slot[k] = i, s
        heads[item, slot] = self.tag  # (a view of buf0: trial 0's polynomials now hold the new tags)
        for t, sel, a, b, at in self.pieces(item, slot):
            if t == 0:  # (read already; it goes out below, with the tags)
                buf, rows, ids = buf0, item[sel], None
            else:
                ids, rows = np.unique(self.items[item[sel]], return_inverse=True)
                buf = self.srv.read_db_items_at(t, 8, ids).reshape(len(ids), POLY)
            r, c, k, z = spans(rows, a, b, at)
            buf[r, c] = values[sel[k], z]
            if ids is not None:
                self.srv.update_db_items(t, buf, 8, ids)
        touched = np.unique(item)
        self.srv.update_db_items(0, np.ascontiguousarray(buf0[touched]), 8, self.items[touched])
        self.sync()


def pack_rows(pg, srv, sync, lay, n_loaded):
    rows = []
    for form, fmt in (("packed", P.DB_PACKED), ("limbs", P.DB_LIMBS)):
        if fmt == P.DB_LIMBS and not P.has_limb_form(pg, OUT_N):
            continue
        srv.set_db_format(fmt)
        for n in (1, 4096):
            new = key_array(n_loaded + 10_000, n)
            vals = values_of(n_loaded + 10_000, n, V)
            old = OldRoute(srv, sync, lay, *hashes(pg, new, OUT_N))

            def new_put():
                srv.kv_put(TK, new, vals)
                sync()

            row = dict(form=form, n_keys=n, n_candidate_items=int(len(old.items)))
            row["put"] = alternated({"kv_put": new_put, "per-trial read_db_items_at+scan+place+splice+update_db_items": lambda: old.put(vals)},
                                    between=lambda: srv.kv_delete(TK, new, V))
            have = key_array(5000, n)
            oldg = OldRoute(srv, sync, lay, *hashes(pg, have, OUT_N))
            out_new, out_old = np.zeros((n, V), dtype=np.uint8), np.zeros((n, V), dtype=np.uint8)
            found = {}

            def new_get():
                found["new"] = srv.kv_get(TK, have, V, out=out_new)[1]

            def old_get():
                found["old"] = oldg.get(out_old)

            row["get"] = alternated({"kv_get": new_get, "per-trial read_db_items_at+scan+cut": old_get})
            assert (found["new"] == found["old"]).all() and found["new"].all() and (out_new == out_old).all(), "the two routes return the same values"
            assert (out_new == values_of(5000, n, V)).all(), "and they are the loaded values"
            assert srv.db_format() == fmt
            rows.append(row)
            print(json.dumps(row), flush=True)
    return rows


def decode_rows(pg, srv, lay):
    cl = sa.Client(pg, bytes(range(32)), out_n=OUT_N)
    srv.set_pub_params_seeded(cl.pub_params("seeded"))
    rows = []
    keys = key_array(7000, 64)
    tag, _, _ = hashes(pg, keys, OUT_N)
    resp = np.stack([srv.answer_seeded(q, want_packed=False)[0].copy() for q in cl.kv_queries(TK, keys, "seeded")])  # [128][out_n + 1][out_n][N]
    for n in (1, 8, 64):
        got = {}

        def new_decode():
            got["new"] = cl.kv_decode(TK, keys[:n], resp[:2 * n], V)

        def old_decode():
            plain = cl.decode(resp[:2 * n]).reshape(2 * n, -1).astype(np.uint8)  # (p_db = 256: a coefficient is a byte of the stream, polynomials in trial order)
            heads = np.ascontiguousarray(plain[:, :8 * lay.slots]).view("<u8").reshape(n, 2, lay.slots)
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


def stats_row(name, srv, lay, vb, n_loaded, forms):
    """kv_stats of the whole table against the probe of about as many buckets (kv_get of absent keys) and fingerprint_items of the image"""
    absent = key_array(n_loaded + 5_000_000, int(lay.buckets) // 2)  # two candidate buckets per key: about nb buckets, a few twice
    out = np.zeros((len(absent), vb), dtype=np.uint8)
    rows = []
    for form, fmt in forms:
        srv.set_db_format(fmt)
        got = {}

        def new_stats():
            got["stats"] = srv.kv_stats(vb)

        def probe():
            got["found"] = srv.kv_get(TK, absent, vb, out=out)[1]

        row = dict(server=name, form=form, buckets=int(lay.buckets), slots=int(lay.slots), probe_keys=len(absent))
        row["stats"] = alternated({"kv_stats": new_stats, "kv_get of absent keys (the probe)": probe,
                                   "fingerprint_items of the image": lambda: srv.fingerprint_items((1, 2))})
        assert not got["found"].any() and got["stats"].used == n_loaded and got["stats"].buckets == lay.buckets
        row["load"] = got["stats"].load()
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def new_rows():
    pg = sa.make_params(NU1, NU2, **PACK)
    lay = sa.pack_kv_layout(pg, OUT_N, V)
    n_loaded = int(int(lay.capacity) * LOAD)
    srv = sa.PackServer(pg, OUT_N)
    st = torch.cuda.Stream()
    srv.set_stream(st.cuda_stream)
    t0 = time.perf_counter()
    srv.kv_load(TK, key_array(0, n_loaded), values_of(0, n_loaded, V))
    load_ms = (time.perf_counter() - t0) * 1e3
    rows = pack_rows(pg, srv, st.synchronize, lay, n_loaded) + decode_rows(pg, srv, lay)
    forms = [("packed", P.DB_PACKED)] + ([("limbs", P.DB_LIMBS)] if P.has_limb_form(pg, OUT_N) else [])
    rows += stats_row("pack", srv, lay, V, n_loaded, forms)
    srv.close()
    table = dict(load=LOAD, slots=int(lay.slots), buckets=int(lay.buckets), item_bytes=int(lay.item_bytes), keys_loaded=n_loaded, kv_load_ms=load_ms)
    # the base server at configs[1], V = 248
    kw = dict(CONFIG1)
    pb = sa.make_params(kw.pop("nu1"), kw.pop("nu2"), **kw)
    lb = sa.kv_layout(pb, 248)
    nb_loaded = int(lb.capacity) * 3 // 4
    base = sa.Server(pb)
    base.kv_load(TK, key_array(0, nb_loaded), values_of(0, nb_loaded, 248))
    rows += stats_row("base configs[1]", base, lb, 248, nb_loaded, [("packed", SV.DB_PACKED), ("limbs", SV.DB_LIMBS)])
    base.close()
    return table, rows


def existing_calls():
    """calls that existed before this change, median wall ms of five runs each after a warm-up: keyed records on a base server at configs[1], and the
    SpiralPack record calls"""
    res = {}

    def timed(calls):
        for name, fn in calls.items():
            fn()
            ms = []
            for _ in range(5):
                t0 = time.perf_counter()
                fn()
                ms.append((time.perf_counter() - t0) * 1e3)
            res[name] = float(np.median(ms))

    kw = dict(CONFIG1)
    pb = sa.make_params(kw.pop("nu1"), kw.pop("nu2"), **kw)
    lb = sa.kv_layout(pb, 248)
    n_loaded = int(lb.capacity) * 3 // 4
    base = sa.Server(pb)
    base.kv_load(TK, key_array(0, n_loaded), values_of(0, n_loaded, 248))
    cl = sa.Client(pb, bytes(range(32)))
    base.set_pub_params(*cl.pub_params())
    have, new, vals = key_array(5000, 4096), key_array(n_loaded + 10_000, 4096), values_of(1, 4096, 248)
    resp = np.stack([base.answer(q)[1] for q in cl.kv_queries(TK, have[:64], "ntt")])
    out = np.zeros((4096, 248), dtype=np.uint8)

    def put(n):
        base.kv_put(TK, new[:n], vals[:n])  # (the first run inserts, the timed ones overwrite: the same probe and the same write)
        base.sync()

    timed({"base kv_put_1": lambda: put(1), "base kv_put_4096": lambda: put(4096), "base kv_get_1": lambda: base.kv_get(TK, have[:1], 248, out=out[:1]),
           "base kv_get_4096": lambda: base.kv_get(TK, have, 248, out=out), "base kv_decode_1": lambda: cl.kv_decode(TK, have[:1], resp[:2], 248),
           "base kv_decode_64": lambda: cl.kv_decode(TK, have[:64], resp, 248)})
    cl.close()
    base.close()
    pg = sa.make_params(NU1, NU2, **PACK)
    lay = sa.record_layout(pg, 256, OUT_N)
    srv = sa.PackServer(pg, OUT_N)
    srv.gen_db(3)
    st = torch.cuda.Stream()
    srv.set_stream(st.cuda_stream)
    rng = np.random.default_rng(5)
    ids = rng.choice(lay.capacity, size=4096, replace=False).astype(np.uint64)
    recs = rng.integers(0, 256, size=(4096, 256), dtype=np.uint8)
    rout = np.zeros((4096, 256), dtype=np.uint8)

    def update(n):
        srv.update_records(recs[:n], 256, ids[:n])
        st.synchronize()

    timed({"pack update_records_1": lambda: update(1), "pack update_records_4096": lambda: update(4096),
           "pack read_records_at_1": lambda: srv.read_records_at(256, ids[:1], out=rout[:1]), "pack read_records_at_4096": lambda: srv.read_records_at(256, ids, out=rout)})
    srv.close()
    return res


def against_parent(parent_root):
    """children of the two trees in turn, each a fresh process"""
    import subprocess

    runs = {"parent": [], "tree": []}
    env = {k: v for k, v in os.environ.items() if k != "SPIRAL_LIB"}
    for rep in range(reps):
        for name, root in (("parent", parent_root), ("tree", HERE))[:: 1 if rep % 2 == 0 else -1]:  # (which goes first alternates too)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing=" + os.path.abspath(root), f"--nu={NU1},{NU2}", f"--outn={OUT_N}"],
                               capture_output=True, text=True, env=env, timeout=300)
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
    table, rows = (None, []) if "parent-only" in opts else new_rows()
    res = dict(tool="tools/pack_kv.py", reps=reps, value_bytes=V, geometry=dict(nu1=NU1, nu2=NU2, out_n=OUT_N, **PACK), table=table,
               device=torch.cuda.get_device_name(0), rows=rows)
    if opts.get("parent"):
        res["existing_calls_against_the_parent_build"] = dict(reps=reps, order="which build's child goes first alternates from repetition to repetition",
                                                              rows=against_parent(opts["parent"]))
    text = json.dumps(res, indent=1)
    print(text)
    if "out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
        with open(opts["out"], "w") as f:
            f.write(text + "\n")
