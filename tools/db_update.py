"""Cost of changing a few database items on a server that batches: the in-place update (spiral_gpu_server_update_db_items) in either image form
against the route that existed before it -- a partial load_db_items, which takes a limb-plane image back to the packed form, and the next batch,
which converts it to limb planes again.  Device-event times on the owner's stream (warm-up first), medians of --reps runs.
usage: tools/db_update.py [--configs=1,2] [--reps=3] [--out=FILE]          (prints one JSON document; --out also writes it)"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch  # (before the library initialises the device)

import spiral_amd as sa
from spiral_amd import server as SV

CONFIGS = {  # bench.py WORKLOADS config2 / config3
    1: dict(nu1=8, nu2=7, t_gsw=8, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=20, p_db=256),
    2: dict(nu1=9, nu2=10, t_gsw=10, t_conv=4, t_exp=8, t_exp_right=56, qprime_bits=22, p_db=256),
}
opts = dict(a[2:].split("=", 1) for a in sys.argv[1:] if a.startswith("--"))
which = [int(c) for c in opts.get("configs", "1,2").split(",")]
reps = int(opts.get("reps", 3))
LANES, BITS = 4, 8


def run(cfg):
    kw = dict(CONFIGS[cfg])
    pg = sa.make_params(kw.pop("nu1"), kw.pop("nu2"), **kw)
    s = sa.get_shape(pg)
    total = s.dim0 * s.num_per
    rng = np.random.default_rng(cfg)
    mk = lambda shape: np.stack([rng.integers(0, m, size=shape + (sa.N,), dtype=np.uint64) for m in (sa.P, sa.B)], axis=-2)
    st = torch.cuda.Stream()
    owner = sa.Server(pg)
    owner.fill_db_random(3)
    lanes = [owner] + [sa.Server(pg, share_db_of=owner) for _ in range(LANES - 1)]
    for ln in lanes:
        ln.set_pub_params(mk((s.n_left, 2, pg.t_exp)), mk((s.n_right, 2, pg.t_exp_right)), mk((3, 2 * pg.t_conv)), mk((3, 2 * pg.t_conv)))
        ln.set_query(mk((s.n_query_cts, 2)))
        ln.use_graphs(True)
        ln.set_stream(st.cuda_stream)

    def timed(fn):
        """(device ms between events around fn on the owner's stream, host wall ms of the call)"""
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        st.synchronize()
        e0.record(st)
        t0 = time.perf_counter()
        fn()
        wall = (time.perf_counter() - t0) * 1e3
        e1.record(st)
        st.synchronize()
        return e0.elapsed_time(e1), wall

    batch = lambda: sa.run_query_batch(lanes)

    def batches_after():
        first = timed(batch)[0]
        steady = float(np.median([timed(batch)[0] for _ in range(3)]))
        return first, steady

    def items_for(n):
        return rng.integers(0, 256, size=n * 4 * sa.N, dtype=np.uint8)

    out = dict(config=cfg, params=CONFIGS[cfg], lanes=LANES, coeff_bits=BITS, image_bytes=owner.db_device_bytes(), rows=[])
    owner.set_db_format(SV.DB_LIMBS)
    batch()  # captures the batch graph on the limb planes
    owner.sync()
    owner.update_db_items(items_for(1), BITS, [0])  # (allocates the update workspace)
    owner.sync()
    for n in (1, 64, 4096):
        row = dict(n_items=n)
        for form, fmt in (("packed", SV.DB_PACKED), ("limbs", SV.DB_LIMBS)):
            owner.set_db_format(fmt)
            dev, wall = [], []
            for _ in range(reps):
                ids = rng.choice(total, size=n, replace=False)
                items = items_for(n)
                d, w = timed(lambda: owner.update_db_items(items, BITS, ids))
                dev.append(d)
                wall.append(w)
            assert owner.db_format() == fmt
            row[f"update_{form}_ms"] = float(np.median(dev))
            row[f"update_{form}_call_ms"] = float(np.median(wall))
            if fmt == SV.DB_LIMBS:
                row["batch_after_update_first_ms"], row["batch_after_update_steady_ms"] = batches_after()
        # the route before: a partial load (n consecutive items) takes the limb planes back to packed, the next batch converts them again
        load, first, steady = [], [], []
        for _ in range(reps):
            assert owner.db_format() == SV.DB_LIMBS
            first_item = int(rng.integers(0, total - n + 1))
            items = items_for(n)
            load.append(timed(lambda: owner.load_db_items(items, BITS, first_item=first_item, n_items=n))[1])
            assert owner.db_format() == SV.DB_PACKED
            f, stdy = batches_after()
            first.append(f)
            steady.append(stdy)
        row["partial_load_ms"] = float(np.median(load))
        row["batch_after_load_first_ms"] = float(np.median(first))
        row["batch_after_load_steady_ms"] = float(np.median(steady))
        out["rows"].append(row)
        print(json.dumps(dict(config=cfg, **row)), flush=True)
    for ln in lanes[1:] + [owner]:
        ln.close()
    return out


if __name__ == "__main__":
    assert sa.lib().spiral_gpu_device_count() > 0, "needs a GPU"
    res = dict(tool="tools/db_update.py", reps=reps, device=torch.cuda.get_device_name(0), results=[run(c) for c in which])
    text = json.dumps(res, indent=1)
    print(text)
    if "out" in opts:
        os.makedirs(os.path.dirname(os.path.abspath(opts["out"])), exist_ok=True)
        with open(opts["out"], "w") as f:
            f.write(text + "\n")
