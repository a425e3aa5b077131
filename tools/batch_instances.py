"""Batched item queries at the configs[3] geometry (SpiralStream 2^20 x 100 KB: nu1=11, nu2=9, direct upload, 56 GiB per database instance, generated
on the device): for B = 1, 2, 4, 8 clients (an owner and its lanes), one spiral_gpu_server_run_query_batch_instances call against n instances, beside
the same B clients answered one at a time by spiral_gpu_server_run_query_instances on the same images, the two alternating in the same process.

    python tools/batch_instances.py [--reps 5] [--sizes 1,2,4,8] [--max-instances 4] [--out profiles/batch_instances.json]

Instances: as many as fit beside the B lanes' buffers (up to --max-instances).  Both paths are timed at 1 and at n instances; the per-instance cost is
the slope between the two and the fixed part (upload-free expansion + conversion) the rest, so items/s are scaled to the 7 instances of a real 100 KB
item.  The batched sweep of one image alone (time_sweep_batch) gives the sweep's share of the 8 TB/s HBM peak in algorithmic bytes.  Prints one JSON
line (and writes it to --out).  Synthetic keys and queries (uniform residues, as bench.py): timing only.  --trace: one batch per size and nothing
else (for rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK_GBPS = 8000.0
WORDS = 6 * 2048


def synth(rng, sa, shape):
    return np.stack([rng.integers(0, m, size=shape + (sa.N,), dtype=np.uint64) for m in (sa.P, sa.B)], axis=-2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--sizes", default="1,2,4,8")
    ap.add_argument("--max-instances", type=int, default=4)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch

    torch.cuda.is_available()
    import spiral_amd as sa
    from spiral_amd._lib import SpiralGpuError

    sizes = [int(x) for x in args.sizes.split(",")]
    B_max = max(sizes)
    pg = sa.make_params(11, 9, t_gsw=4, t_conv=56, t_exp=2, t_exp_right=56, qprime_bits=27, p_db=32768, direct_upload=1)
    s = sa.get_shape(pg)
    free0 = torch.cuda.mem_get_info()[0]
    inst = [sa.Server(pg)]
    inst[0].fill_db_random(4000)
    servers = [inst[0]] + [sa.Server(pg, share_db_of=inst[0]) for _ in range(B_max - 1)]  # the clients: lanes of instance 0 (no image of their own)
    free1 = torch.cuda.mem_get_info()[0]
    image = inst[0].db_device_bytes()
    lane_bytes = (free0 - free1 - image) // B_max  # one client's own buffers (keys, expanded query, GSW matrices, accumulators, fold scratch)
    reserve = B_max * 2 * 6 * WORDS * 8 * args.max_instances + (2 << 30)  # outputs + headroom for the runtime
    while len(inst) < args.max_instances and torch.cuda.mem_get_info()[0] > image + reserve:
        try:
            sv = sa.Server(pg)
        except SpiralGpuError:
            break
        sv.fill_db_random(4000 + len(inst))
        inst.append(sv)
    n = len(inst)
    assert n >= 2, "needs at least two instances on the device"
    rng = np.random.default_rng(1)
    for sv in servers:
        sv.set_pub_params(synth(rng, sa, (s.n_left, 2, pg.t_exp)), synth(rng, sa, (s.n_right, 2, pg.t_exp_right)), synth(rng, sa, (3, 2 * pg.t_conv)),
                          synth(rng, sa, (3, 2 * pg.t_conv)))
        sv.set_query(synth(rng, sa, (s.n_query_cts, 2)))
        sv.set_stream(sa.lib().spiral_gpu_server_get_stream(servers[0].h))  # one stream: no event ordering around the launch sequence
        sv.use_graphs(True)
    resp = torch.zeros(B_max * n * WORDS, dtype=torch.int64, device="cuda")
    wb = sa.lib().spiral_gpu_response_wire_bytes(__import__("ctypes").byref(pg), 2)
    wire = torch.zeros(B_max * n * wb, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def batch(B, k):
        sa.run_query_batch_instances(servers[:B], inst[:k], resp.data_ptr(), 0, wire.data_ptr())

    def singles(B, k):
        for b in range(B):
            servers[b].run_query_instances(inst[:k], resp.data_ptr() + b * k * WORDS * 8)

    def timed(f, B, k, reps):
        f(B, k)
        servers[0].sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            f(B, k)
        servers[0].sync()
        return (time.perf_counter() - t0) * 1e3 / reps

    if args.trace:  # one warm-up and one replayed batch per size, then the singles of B = 1 (what the kernel trace is for)
        for B in sizes:
            for _ in range(2):
                batch(B, n)
            servers[0].sync()
        for _ in range(2):
            singles(1, n)
        servers[0].sync()
        print(json.dumps({"tool": "batch_instances", "trace": True, "instances": n, "sizes": sizes}), flush=True)
        return
    rows = []
    for B in sizes:
        batch(B, n)  # (the first batch of two or more converts every image in place)
        servers[0].sync()
        t = {"batch": {1: [], n: []}, "singles": {1: [], n: []}}
        for _ in range(3):  # alternating: batch, singles, batch, singles ...
            for k in (1, n):
                t["batch"][k].append(timed(batch, B, k, args.reps))
                t["singles"][k].append(timed(singles, B, k, args.reps))
        row = {"B": B}
        for name in ("batch", "singles"):
            t1, tn = float(np.median(t[name][1])), float(np.median(t[name][n]))
            per_inst = (tn - t1) / (n - 1)
            fixed = t1 - per_inst
            t7 = fixed + 7 * per_inst
            row[name] = {"ms_1_instance": round(t1, 3), f"ms_{n}_instances": round(tn, 3), "ms_per_instance": round(per_inst, 3), "ms_fixed": round(fixed, 3),
                         "ms_per_item_batch_7_instances": round(t7, 3), "items_per_s_7_instances": round(B / (t7 * 1e-3), 1)}
        row["speedup_vs_singles"] = round(row["batch"]["items_per_s_7_instances"] / row["singles"]["items_per_s_7_instances"], 2)
        for sv in servers[:B]:
            sv.run_pre()
        sw = sa.time_sweep_batch(servers[:B], args.reps)  # the matrix-core pass over instance 0's image for the B clients, alone
        gbs = inst[0].sweep_bytes() / (sw * 1e-3) / 1e9
        row["sweep_ms_one_image"] = round(sw, 3)
        row["sweep_algorithmic_GBps"] = round(gbs, 1)
        row["sweep_frac_of_peak"] = round(gbs / HBM_PEAK_GBPS, 4)
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"tool": "batch_instances", "config": "configs[3] geometry: SpiralStream nu1=11, nu2=9, direct upload, t_gsw=4, t_conv=56, q'=27 bits, p=32768; "
                                                "images generated on the device", "reps": args.reps, "instances": n,
           "db_device_bytes_per_instance": int(image), "lane_device_bytes": int(lane_bytes), "sweep_algorithmic_bytes_per_instance": int(inst[0].sweep_bytes()),
           "image_form": "limbs" if inst[0].db_format() == 1 else "packed", "wire_bytes_per_response": int(wb), "raw_bytes_per_response": WORDS * 8,
           "sizes": rows}
    line = json.dumps(out)
    print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    for sv in servers[1:] + inst:
        sv.close()


if __name__ == "__main__":
    main()
