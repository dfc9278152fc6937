"""Summarise the rocprofv3 kernel trace of `tools/dfit_time.py --no-host --steps K`: per kernel
(and per launch shape) calls and times over the last K update_disc steps, i.e. from the K-th last
k_dfit_gather to the read-back behind the last refresh of the inference copies (the warm-up steps
come before, compute_chi2_distance after), and their sum per step.

usage: python tools/dfit_trace.py <run_kernel_trace.csv> K
"""
import csv
import sys
from collections import defaultdict

path, K = sys.argv[1], int(sys.argv[2])
rows = sorted(csv.DictReader(open(path)), key=lambda x: int(x["Start_Timestamp"]))


def short(name):
    name = name.replace("(anonymous namespace)::", "").replace("void ", "").replace("(amx::OptimKind)", "kind ")
    return name.replace("amx::", "").split("(")[0][:44]


gathers = [i for i, x in enumerate(rows) if "k_dfit_gather" in x["Kernel_Name"]]
last = max(i for i, x in enumerate(rows) if "k_optim_update" in x["Kernel_Name"])  # a step's last launch
end = last + 1
while end < len(rows) and ("k_split" in rows[end]["Kernel_Name"] or "copyBuffer" in rows[end]["Kernel_Name"]):
    end += 1
rows = rows[gathers[-K]:end]
agg, shapes = defaultdict(list), defaultdict(list)
for x in rows:
    d = (int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1000
    k = short(x["Kernel_Name"])
    agg[k].append(d)
    try:
        wg = tuple(int(x[f"Grid_Size_{a}"]) // int(x[f"Workgroup_Size_{a}"]) for a in "XYZ")
    except (KeyError, ValueError, ZeroDivisionError):
        wg = (0, 0, 0)
    shapes[(k, wg)].append(d)
tot = sum(sum(v) for v in agg.values())
span = (int(rows[-1]["End_Timestamp"]) - int(rows[0]["Start_Timestamp"])) / 1000
print(f"{'kernel':44s} {'calls':>6s} {'total us':>11s} {'avg us':>8s} {'min us':>8s} {'max us':>8s} {'%':>5s}")
for k, v in sorted(agg.items(), key=lambda kv: -sum(kv[1])):
    print(f"{k:44s} {len(v):6d} {sum(v):11.1f} {sum(v) / len(v):8.2f} {min(v):8.2f} {max(v):8.2f} "
          f"{100 * sum(v) / tot:5.1f}")
print("\nper launch shape (workgroups x, y, z; calls; avg us):")
for (k, wg), v in sorted(shapes.items()):
    if "dfit" in k or "gemm64" in k or "optim" in k:
        print(f"{k:44s} {wg[0]:4d} x {wg[1]:3d} x {wg[2]:2d} {len(v):6d} {sum(v) / len(v):8.2f}")
print(f"\nsum of kernel time per step: {tot / K:.1f} us; span of the {K} steps per step: {span / K:.1f} us")
