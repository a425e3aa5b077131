"""Condenses two `hipcc -Rpass-analysis=kernel-resource-usage` logs of one source file -- the parent commit's and this tree's -- into one line per kernel:
`same` / `DIFF` / `GONE` for every kernel of the parent (a `NoLanes` instantiation is matched with the parent's kernel of that name without the
argument; trailing template flags that are `false` are dropped from both sides, and so is sweep_mfma_kernel's trailing waves-per-workgroup argument
at its default 8), then the kernels only the tree has.  The logs are the compiler's stderr:

    hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage -c pack.hip -o /dev/null 2> tree_pack.rpass   (in spiral_amd/csrc)
    python tools/resource_usage_diff.py pack.hip parent_pack.rpass tree_pack.rpass [poly.hip parent_poly.rpass tree_poly.rpass ...]
"""
import re
import subprocess
import sys

KEYS = [("TotalSGPRs", "TotalSGPRs"), ("VGPRs", "VGPRs"), ("AGPRs", "AGPRs"), ("ScratchSize [bytes/lane]", "ScratchSize"), ("Occupancy [waves/SIMD]", "Occupancy"),
        ("SGPRs Spill", "SGPRs_Spill"), ("VGPRs Spill", "VGPRs_Spill"), ("LDS Size [bytes/block]", "LDS_Size")]


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark:\s+Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+(.*?): (\S+) \[-Rpass", line)
        if m and cur:
            out[cur][m.group(1)] = m.group(2)
    names = subprocess.run(["c++filt"], input="\n".join(out), capture_output=True, text=True).stdout.split("\n")
    res = {}
    for mangled, dem in zip(out, names):
        dem = re.sub(r"\(.*$", "", dem.replace("(anonymous namespace)::", "")).replace("void ", "").replace("spiral::", "")
        if dem.startswith("sweep_mfma_kernel<"):
            dem = re.sub(r", 8>$", ">", dem)  # W at its default: the wide form, the parent's only one
        dem = re.sub(r"(, false)+>$", ">", dem)  # trailing flags at their default: a template that gained one keeps its kernels' names
        res[dem] = " ".join(f"{short}={out[mangled].get(k)}" for k, short in KEYS)
    return res


def norm(name):  # the parent's name of a NoLanes instantiation
    n = name.replace(", NoLanes>", ">").replace("<NoLanes>", "")
    return n


for f, parent_log, tree_log in zip(sys.argv[1::3], sys.argv[2::3], sys.argv[3::3]):
    par, tree = parse(parent_log), parse(tree_log)
    tmap = {}
    for k, v in tree.items():
        if k in par:
            tmap[k] = (k, v)
        elif "NoLanes" in k and norm(k) in par:
            tmap[norm(k)] = (k, v)
    rows, differ = [], 0
    for k, v in par.items():
        if k not in tmap:
            rows.append(f"GONE  {k}: {v}")
            differ += 1
            continue
        tk, tv = tmap[k]
        label = k if tk == k else f"{k} -> {tk}"
        if tv == v:
            rows.append(f"same  {label}: {v}")
        else:
            rows.append(f"DIFF  {label}: {v}  ->  {tv}")
            differ += 1
    print(f"## {f}: {len(par)} kernels of the parent compared, {differ} differ")
    print("\n".join(rows))
    new = [k for k in tree if k not in par and not ("NoLanes" in k and norm(k) in par)]
    print(f"new kernels of {f}:")
    for k in new:
        print(f"new   {k}: {tree[k]}")
