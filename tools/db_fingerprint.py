"""Cost of the database fingerprint (spiral_gpu_server_fingerprint_items / _at) beside the export of the same image in the same process
(read_db_items(8) / read_db_items_at): the same gather and inverse transform, 8 bytes per polynomial in place of the byte-wide stores and the copy.
Per geometry, after a warm-up, --reps alternations of the two legs from the packed image and from the limb planes; then the _at forms of 1 and 4096
scattered items.  Device time = HIP events around each call's launches, copies excluded (options "db_fingerprint_ns" / "db_export_ns"); call time =
host wall clock to completion.  Medians with min and max.  The fingerprint of each leg is also compared with the other form's: they must agree.
--existing: update_db_items, read_db_items and read_db_items_at of 1 and 4096 items alone (for runs of this tree and of the parent's taking turns).
usage: tools/db_fingerprint.py [--configs=1,2] [--reps=7] [--existing] [--out=FILE]          (prints one JSON document; --out also writes it)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # (before the library initialises the device)

import spiral_amd as sa
from spiral_amd import server as SV

CONFIGS = {  # bench.py's default geometry (2^20 x 256 B) and the 2^24 x 256 B one (a 30 GB image)
    1: dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256),
    2: dict(nu1=9, nu2=10, t_gsw=10, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=22, p_db=256),
}
opts = dict((a[2:].split("=", 1) + ["1"])[:2] for a in sys.argv[1:] if a.startswith("--"))
which = [int(c) for c in opts.get("configs", "1").split(",")]
reps = int(opts.get("reps", 7))
BITS = 8
KEY = (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F)


def stat(xs):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)))


def wall_of(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def run(cfg):
    kw = dict(CONFIGS[cfg])
    pg = sa.make_params(kw.pop("nu1"), kw.pop("nu2"), **kw)
    s = sa.get_shape(pg)
    total = s.dim0 * s.num_per
    rng = np.random.default_rng(cfg)
    srv = sa.Server(pg)
    srv.gen_db(7)
    buf = np.zeros(sa.db_items_bytes(pg, BITS, total), dtype=np.uint8)
    out = dict(config=cfg, params=CONFIGS[cfg], items=total, image_bytes=srv.db_device_bytes(), exported_bytes=int(buf.size))
    forms = (("packed", SV.DB_PACKED), ("limbs", SV.DB_LIMBS))
    if "existing" in opts:
        item = np.frombuffer(rng.bytes(4096 * 8192), dtype=np.uint8)
        rows = {}
        for form, fmt in forms:
            srv.set_db_format(fmt)
            for n in (1, 4096):
                ids = rng.permutation(total)[:n]
                for name, fn in (("update_db_items", lambda: (srv.update_db_items(item[:n * 8192], BITS, ids), srv.sync())),
                                 ("read_db_items_at", lambda: srv.read_db_items_at(BITS, ids)), ("read_db_items", lambda: srv.read_db_items(BITS, 5, n))):
                    fn()
                    rows[f"{name}_{n}_{form}_call_ms"] = stat([wall_of(fn)[0] for _ in range(reps)])
        out["existing"] = rows
        srv.close()
        return out
    values = {}
    for form, fmt in forms:  # warm-up: the workspaces, the kernels' code objects
        srv.set_db_format(fmt)
        srv.read_db_items(BITS, out=buf)
        values[form] = srv.fingerprint_items(KEY)
    assert values["packed"] == values["limbs"], "the two forms of one image give different fingerprints"
    out["fingerprint"] = values["packed"]
    rows = {f"{leg}_{form}_{kind}": [] for leg in ("fingerprint", "read") for form, _ in forms for kind in ("ms", "call_ms")}
    for rep in range(reps):
        print(f"config {cfg}: repetition {rep + 1} of {reps}", file=sys.stderr, flush=True)
        for form, fmt in forms:
            srv.set_db_format(fmt)
            w, F = wall_of(lambda: srv.fingerprint_items(KEY))
            assert F == values[form]
            rows[f"fingerprint_{form}_ms"].append(sa.get_option("db_fingerprint_ns") / 1e6)
            rows[f"fingerprint_{form}_call_ms"].append(w)
            w, _ = wall_of(lambda: srv.read_db_items(BITS, out=buf))
            rows[f"read_{form}_ms"].append(sa.get_option("db_export_ns") / 1e6)
            rows[f"read_{form}_call_ms"].append(w)
    out["full"] = {k: stat(v) for k, v in rows.items()}
    out["fingerprint_over_read"] = {f"{form}_{kind}": out["full"][f"fingerprint_{form}_{kind}"]["median"] / out["full"][f"read_{form}_{kind}"]["median"]
                                    for form, _ in forms for kind in ("ms", "call_ms")}
    out["at"] = []
    for n in (1, 4096):
        row = dict(n_items=n)
        for form, fmt in forms:
            srv.set_db_format(fmt)
            ids = rng.integers(0, total, size=n)
            srv.read_db_items_at(BITS, ids)
            srv.fingerprint_items_at(KEY, ids)
            r = {k: [] for k in ("fingerprint_at_ms", "fingerprint_at_call_ms", "read_at_ms", "read_at_call_ms")}
            for _ in range(reps):
                ids = rng.integers(0, total, size=n)
                r["fingerprint_at_call_ms"].append(wall_of(lambda: srv.fingerprint_items_at(KEY, ids))[0])
                r["fingerprint_at_ms"].append(sa.get_option("db_fingerprint_ns") / 1e6)
                r["read_at_call_ms"].append(wall_of(lambda: srv.read_db_items_at(BITS, ids))[0])
                r["read_at_ms"].append(sa.get_option("db_export_ns") / 1e6)
            row[form] = {k: stat(v) for k, v in r.items()}
        out["at"].append(row)
    srv.close()
    return out


if __name__ == "__main__":
    assert sa.lib().spiral_gpu_device_count() > 0, "needs a GPU"
    res = dict(tool="tools/db_fingerprint.py", reps=reps, device=torch.cuda.get_device_name(0), results=[run(c) for c in which])
    text = json.dumps(res, indent=1)
    print(text)
    if "out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
        with open(opts["out"], "w") as f:
            f.write(text + "\n")
