"""Cost of reading the database back as plaintexts (spiral_gpu_server_read_db_items / _at) from either image form, beside the forward direction on
the same image in the same process: gen_db (as many transforms, a scatter where the export has a gather) and load_db_items of the exported bytes.
Per geometry, after a warm-up, --reps alternations of: gen_db, read_db_items (packed), read_db_items (limb planes), load_db_items; then
read_db_items_at of 1 and 4096 scattered items in both forms.  Device time = HIP events around the export launches, copies excluded (option
"db_export_ns"); call time = host wall clock, copies included.  Medians with min and max.  Beside them two bounds from shapes alone: image bytes
over 8 TB/s, and exported polynomials x the standalone inverse transform (time_ntt, what bench.py's roofline_ntt prices).
usage: tools/db_export.py [--configs=1,2] [--reps=7] [--out=FILE]          (prints one JSON document; --out also writes it)"""
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
opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--"))
which = [int(c) for c in opts.get("configs", "1,2").split(",")]
reps = int(opts.get("reps", 7))
BITS, HBM_PEAK = 8, 8e12


def stat(xs):
    return dict(median=float(np.median(xs)), min=float(min(xs)), max=float(max(xs)))


def run(cfg):
    kw = dict(CONFIGS[cfg])
    pg = sa.make_params(kw.pop("nu1"), kw.pop("nu2"), **kw)
    s = sa.get_shape(pg)
    total = s.dim0 * s.num_per
    rng = np.random.default_rng(cfg)
    st = torch.cuda.Stream()
    srv = sa.Server(pg)
    srv.set_stream(st.cuda_stream)

    def timed(fn):
        """(device ms between events around fn on the server's stream, host wall ms of the call, what fn returned)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        e0.record(st)
        t0 = time.perf_counter()
        r = fn()
        wall = (time.perf_counter() - t0) * 1e3
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1), wall, r

    def export(fn):
        """(device ms of the export launches alone, host wall ms of the call, the bytes)"""
        _, wall, r = timed(fn)
        return sa.get_option("db_export_ns") / 1e6, wall, r

    buf = np.zeros(sa.db_items_bytes(pg, BITS, total), dtype=np.uint8)
    srv.gen_db(7)
    image_bytes = srv.db_device_bytes()
    srv.read_db_items(BITS, out=buf)  # warm-up: the workspace, the kernels' code objects
    srv.set_db_format(SV.DB_LIMBS)
    srv.read_db_items(BITS, out=buf)
    rows = {k: [] for k in ("gen_db_ms", "read_packed_ms", "read_packed_call_ms", "read_limbs_ms", "read_limbs_call_ms", "load_db_items_call_ms")}
    for rep in range(reps):
        print(f"config {cfg}: repetition {rep + 1} of {reps}", file=sys.stderr, flush=True)
        rows["gen_db_ms"].append(timed(lambda: srv.gen_db(7))[0])
        d, w, _r = export(lambda: srv.read_db_items(BITS, out=buf))
        rows["read_packed_ms"].append(d)
        rows["read_packed_call_ms"].append(w)
        srv.set_db_format(SV.DB_LIMBS)
        d, w, _r = export(lambda: srv.read_db_items(BITS, out=buf))
        rows["read_limbs_ms"].append(d)
        rows["read_limbs_call_ms"].append(w)
        srv.set_db_format(SV.DB_PACKED)
        rows["load_db_items_call_ms"].append(timed(lambda: srv.load_db_items(buf, BITS))[1])
    fwd_ms, inv_ms = sa.time_ntt(1 << 14, 10)
    out = dict(config=cfg, params=CONFIGS[cfg], items=total, coeff_bits=BITS, image_bytes=image_bytes, exported_bytes=int(buf.size),
               full={k: stat(v) for k, v in rows.items()},
               bounds=dict(image_over_hbm_peak_ms=image_bytes / HBM_PEAK * 1e3, polys_times_inverse_transform_ms=4 * total * inv_ms / (1 << 14),
                           inverse_transform_ns=inv_ms / (1 << 14) * 1e6, forward_transform_ns=fwd_ms / (1 << 14) * 1e6))
    g = out["full"]["gen_db_ms"]["median"]
    out["ratio_to_gen_db"] = dict(packed=out["full"]["read_packed_ms"]["median"] / g, limbs=out["full"]["read_limbs_ms"]["median"] / g)
    out["at"] = []
    for n in (1, 4096):
        row = dict(n_items=n)
        for form, fmt in (("packed", SV.DB_PACKED), ("limbs", SV.DB_LIMBS)):
            srv.set_db_format(fmt)
            srv.read_db_items_at(BITS, rng.integers(0, total, size=n))  # (the bounce buffer of this size)
            dev, wall = [], []
            for _ in range(reps):
                ids = rng.integers(0, total, size=n)
                d, w, _r = export(lambda: srv.read_db_items_at(BITS, ids))
                dev.append(d)
                wall.append(w)
            row[f"read_at_{form}_ms"] = stat(dev)
            row[f"read_at_{form}_call_ms"] = stat(wall)
        out["at"].append(row)
    print(json.dumps(out), flush=True)
    srv.close()
    return out


if __name__ == "__main__":
    assert sa.lib().spiral_gpu_device_count() > 0, "needs a GPU"
    res = dict(tool="tools/db_export.py", reps=reps, device=torch.cuda.get_device_name(0), results=[run(c) for c in which])
    text = json.dumps(res, indent=1)
    print(text)
    if "out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
        with open(opts["out"], "w") as f:
            f.write(text + "\n")
