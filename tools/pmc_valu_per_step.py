#!/usr/bin/env python3
"""Dynamic VALU instructions per wave and pipeline step of every k_scan build in a counter run:

    rocprofv3 --pmc SQ_INSTS_VALU SQ_WAVES --output-format csv -d OUT -- python3 tools/iso_batch.py 1024
    tools/pmc_valu_per_step.py OUT [columns per unit, default 5000]

(counters in a run of their own: no tracing options beside --pmc).  A launch of k_scan takes 8 units per workgroup of 4 waves
(scan.hip, launch_scan_t) and a unit of n columns is n + 127 steps, so a launch of G workgroups ran about 8 G (n + 127) steps, the
last workgroup's missing units aside.  Printed per kernel name: launches, SQ_WAVES, SQ_INSTS_VALU, VALU per wave, VALU per step.
Set the last figure against the static count of tools/count_step_valu.py: the difference is what the rare blocks execute."""
import collections
import csv
import glob
import os
import sys

out = sys.argv[1]
ncol = int(sys.argv[2]) if len(sys.argv) > 2 else 5000
files = glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True)
if not files:
    sys.exit(f"no *counter_collection.csv under {out}")
tot = collections.defaultdict(lambda: collections.defaultdict(float))
steps = collections.defaultdict(float)
launches = collections.defaultdict(set)
for path in files:
    for row in csv.DictReader(open(path, newline="")):
        name = row["Kernel_Name"]
        if "k_scan<" not in name and "k_scanI" not in name:
            continue
        name = name.split("(")[0].replace("fasim::", "").replace("void ", "")
        tot[name][row["Counter_Name"]] += float(row["Counter_Value"])
        key = (path, row.get("Dispatch_Id"))
        if key not in launches[name]:
            launches[name].add(key)
            wg = int(row["Grid_Size"]) // max(1, int(row["Workgroup_Size"]))
            steps[name] += 8.0 * wg * (ncol + 127)
print(f"{'kernel':40s} {'launches':>8s} {'SQ_WAVES':>12s} {'SQ_INSTS_VALU':>14s} {'VALU/wave':>12s} {'VALU/step':>10s}")
for name in sorted(tot):
    c = tot[name]
    valu, waves = c.get("SQ_INSTS_VALU", 0.0), c.get("SQ_WAVES", 0.0)
    print(f"{name:40s} {len(launches[name]):8d} {waves:12.0f} {valu:14.4e} {valu / max(waves, 1):12.1f} {valu / max(steps[name], 1):10.2f}")
