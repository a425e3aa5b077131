"""Cost of the tracked fingerprint (spiral_gpu_server_fingerprint_track and what keeps it current; include/spiral_gpu.h "Fingerprints", Tracked) at
bench.py's default geometry, from the packed image and from the limb planes, in one process:
  - update_db_items and update_records (256-byte records) of 1 and 4096 scattered ids on a TRACKED server against the same call on an UNTRACKED server of
    the same database, the two taking turns; a one-item fingerprint_items_at beside them (what a caller without tracking pays to learn an item's value);
  - whole-image fingerprint_track and fingerprint_scrub, each against fingerprint_items of the same image;
  - fingerprint_tracked against fingerprint_items (combined only).
Device time = HIP events on the servers' stream around a call's launches (for the three whole-image calls: option "db_fingerprint_ns", the events around
their passes); call time = host wall clock until the call returns, `done` = until the stream is idle.  Medians of --reps repetitions with min and max.
--existing: update_db_items, update_records, read_db_items_at and fingerprint_items with tracking OFF, alone -- the calls a parent build has too.
--compare=DIR: fresh processes of this tree and of the tree at DIR (a checkout of the parent commit, built) run --existing in turn, --turns times each;
    per measurement the tree's median, the parent's median and min..max, and whether the first lies inside the second's spread.
--tree=DIR: import spiral_amd from DIR instead of this file's tree (what --compare starts its children with).
usage: tools/db_track.py [--reps=7] [--existing] [--compare=DIR [--turns=3]] [--out=FILE]      (prints one JSON document; --out also writes it)"""
import json
import os
import subprocess
import sys
import time

opts = dict((a[2:].split("=", 1) + ["1"])[:2] for a in sys.argv[1:] if a.startswith("--"))
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(opts.get("tree", HERE)))
import numpy as np

PARAMS = dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256)  # bench.py's default: 2^15 items of 8 KiB
reps = int(opts.get("reps", 7))
BITS, S = 8, 256
KEY = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F)


def stat(xs):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)))


def measure():
    import torch  # (before the library initialises the device)

    import spiral_amd as sa
    from spiral_amd import server as SV

    assert sa.lib().spiral_gpu_device_count() > 0, "needs a GPU"
    kw = dict(PARAMS)
    pg = sa.make_params(kw.pop("nu1"), kw.pop("nu2"), **kw)
    s = sa.get_shape(pg)
    total = s.dim0 * s.num_per
    rng = np.random.default_rng(1)
    st = torch.cuda.Stream()
    existing = "existing" in opts
    servers = {}
    for name in (("untracked",) if existing else ("tracked", "untracked")):
        servers[name] = sa.Server(pg)
        servers[name].gen_db(7)
        servers[name].set_stream(st.cuda_stream)
    per_item = sa.record_layout(pg, S).per_item if hasattr(sa, "record_layout") else 8192 // S

    def timed(fn):
        """(device ms between events around fn on the stream, host ms of the call, host ms until the stream is idle)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        e0.record(st)
        t0 = time.perf_counter()
        r = fn()
        call = (time.perf_counter() - t0) * 1e3
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1), call, (time.perf_counter() - t0) * 1e3, r

    out = dict(params=PARAMS, items=total, device=torch.cuda.get_device_name(0), table_bytes=total * 4 * 8, rows={})
    rows = out["rows"]

    def add(name, samples):
        for kind, k in (("ms", 0), ("call_ms", 1), ("done_ms", 2)):
            rows[f"{name}_{kind}"] = stat([x[k] for x in samples])

    for form, fmt in (("packed", SV.DB_PACKED), ("limbs", SV.DB_LIMBS)):
        for srv in servers.values():
            srv.set_db_format(fmt)
        if not existing:
            servers["tracked"].fingerprint_track(KEY)
        for n in (1, 4096):
            legs = {(call, name): [] for call in ("update_db_items", "update_records") for name in servers}
            for rep in range(reps + 1):  # (the first repetition warms up: workspaces, code objects)
                ids = rng.permutation(total)[:n]
                items = np.frombuffer(rng.bytes(n * 8192), dtype=np.uint8)
                rids = rng.permutation(total * per_item)[:n]
                recs = np.frombuffer(rng.bytes(n * S), dtype=np.uint8)
                # the two servers take turns at going first, behind a call nobody times: the first launch after the host's pause above is the slow one,
                # whichever server makes it
                servers["untracked"].read_db_items_at(BITS, ids[:1])
                for name, srv in (list(servers.items())[::-1] if rep % 2 else list(servers.items())):
                    a = timed(lambda: srv.update_db_items(items, BITS, ids))
                    b = timed(lambda: srv.update_records(recs, S, rids))
                    if rep:
                        legs[("update_db_items", name)].append(a)
                        legs[("update_records", name)].append(b)
            for (call, name), samples in legs.items():
                add(f"{call}_{n}_{form}_{name}", samples)
            ids = rng.permutation(total)[:n]
            servers["untracked"].read_db_items_at(BITS, ids)
            add(f"read_db_items_at_{n}_{form}", [timed(lambda: servers["untracked"].read_db_items_at(BITS, ids)) for _ in range(reps)])
            servers["untracked"].fingerprint_items_at(KEY, ids)
            add(f"fingerprint_items_at_{n}_{form}", [timed(lambda: servers["untracked"].fingerprint_items_at(KEY, ids)) for _ in range(reps)])
        servers["untracked"].fingerprint_items(KEY)
        whole = {"fingerprint_items": (servers["untracked"], lambda srv: srv.fingerprint_items(KEY))}
        if not existing:
            whole["fingerprint_track"] = (servers["tracked"], lambda srv: srv.fingerprint_track(KEY))
            whole["fingerprint_scrub"] = (servers["tracked"], lambda srv: srv.fingerprint_scrub())
            whole["fingerprint_tracked"] = (servers["tracked"], lambda srv: srv.fingerprint_tracked())
        samples = {k: [] for k in whole}
        values = {}
        for rep in range(reps + 1):
            for k, (srv, fn) in whole.items():
                x = timed(lambda: fn(srv))
                dev = sa.get_option("db_fingerprint_ns") / 1e6 if k != "fingerprint_tracked" else x[0]  # (the events around the passes' launches alone)
                values[k] = x[3]
                if rep:
                    samples[k].append((dev, x[1], x[2]))
        for k, v in samples.items():
            add(f"{k}_{form}", v)
        if not existing:
            assert values["fingerprint_scrub"] == (0, None), "the tracked image does not scrub clean"
            F, n_upd = values["fingerprint_tracked"]
            assert F == servers["tracked"].fingerprint_items(KEY), "the tracked value differs from a recomputation"
            assert values["fingerprint_items"] == servers["untracked"].fingerprint_items(KEY)
            assert F == values["fingerprint_items"], "the two servers took the same updates"
            out[f"fingerprint_{form}"] = F
    if not existing:
        med = lambda k: rows[k]["median"]
        out["summary"] = {}
        for form in ("packed", "limbs"):
            for call in ("update_db_items", "update_records"):
                for n in (1, 4096):
                    for kind in ("ms", "call_ms"):
                        t, u = med(f"{call}_{n}_{form}_tracked_{kind}"), med(f"{call}_{n}_{form}_untracked_{kind}")
                        out["summary"][f"{call}_{n}_{form}_{kind}"] = dict(tracked=t, untracked=u, extra=t - u)
            alt = med(f"update_records_1_{form}_untracked_done_ms") + med(f"fingerprint_items_at_1_{form}_done_ms")
            out["summary"][f"single_record_{form}_done_ms"] = dict(tracked=med(f"update_records_1_{form}_tracked_done_ms"), untracked_plus_one_item_fingerprint=alt)
    for srv in servers.values():
        srv.close()
    return out


def compare(parent):
    """fresh processes of the two trees in turn; every sample of a measurement's medians pooled per tree"""
    turns = int(opts.get("turns", 3))
    runs = {"tree": [], "parent": []}
    for turn in range(turns):
        for who, tree in (("parent", parent), ("tree", HERE))[::-1 if turn % 2 else 1]:  # (each goes first every other turn)
            print(f"turn {turn + 1} of {turns}: {who}", file=sys.stderr, flush=True)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--existing", f"--tree={tree}", f"--reps={reps}"], capture_output=True, text=True, timeout=240)
            if p.returncode:
                sys.stderr.write(p.stderr[-2000:])
                raise SystemExit(f"the {who} run failed with status {p.returncode}")
            runs[who].append(json.loads(p.stdout)["rows"])
    table, outside = {}, []
    for k in runs["tree"][0]:
        if not k.endswith("done_ms"):
            continue
        t = float(np.median([r[k]["median"] for r in runs["tree"]]))
        pm = float(np.median([r[k]["median"] for r in runs["parent"]]))
        lo, hi = min(r[k]["min"] for r in runs["parent"]), max(r[k]["max"] for r in runs["parent"])
        table[k] = dict(tree_median=t, parent_median=pm, parent_min=lo, parent_max=hi, inside=bool(lo <= t <= hi),
                        tree_medians=[r[k]["median"] for r in runs["tree"]], parent_medians=[r[k]["median"] for r in runs["parent"]])
        if not lo <= t <= hi:
            outside.append(k)
    return dict(turns=turns, measurements=table, outside_the_parents_spread=outside)


if __name__ == "__main__":
    res = dict(tool="tools/db_track.py", reps=reps)
    res.update(dict(existing_against_parent=compare(os.path.abspath(opts["compare"]))) if "compare" in opts else measure())
    text = json.dumps(res, indent=1)
    print(text)
    if "out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
        with open(opts["out"], "w") as f:
            f.write(text + "\n")
