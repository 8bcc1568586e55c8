#!/usr/bin/env python3
"""Cost of giving every site of an oligo panel its hit (fasim_scan_oligos_aligned).  Run from the root of a
built tree:

    python3 tools/oligo_hits_bench.py [MB] [OLIGOS] [ROUNDS] [SITES]
        a record of MB Mb (default 5) planted with pieces of the panel, and two panels of OLIGOS oligos (default 64) of 20 nt and
        of 112 nt.  Per panel V is the smallest value at which an oligo has at most SITES sites (default 10 000; the panel's mean,
        found by bisection with scan_oligos), then a warm-up round and ROUNDS alternating rounds (default 4) of three arms,
            A = scan_oligos (the sites alone),
            B = scan_oligos_aligned                       (k_site_ends_short: a problem per lane, a window of the unit),
            C = scan_oligos_aligned with site_short = 0   (k_site_ends: a workgroup per problem, the unit's prefix);
        every round compares B's and C's arrays.  Medians and ranges, the hits phase of B and C (B - A, C - A), their ratio and
        the spread of the rounds; and per arm the phase's own counts -- sites, problems, executed cells -- and the HIP-event time
        of its kernels (family 4), from the `[fasim prof] site hits:` lines of FASIM_PROFILE=1.
The arms run in a child process, which alone initialises the GPU.
"""
import os
import re
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
sys.path.insert(0, "tests")

args = sys.argv[1:]
child = bool(args) and args[0] == "child"
if child:
    args = args[1:]
mb = float(args[0]) if len(args) > 0 else 5
npanel = int(args[1]) if len(args) > 1 else 64
rounds = int(args[2]) if len(args) > 2 else 4
target = int(args[3]) if len(args) > 3 else 10000

if not child:
    env = dict(os.environ, FASIM_PROFILE="1")
    r = subprocess.run([sys.executable, __file__, "child"] + args, env=env, stderr=subprocess.PIPE, text=True)      # (its stdout is this one's)
    if r.returncode:
        sys.stdout.write(r.stderr[-4000:])
        sys.exit(r.returncode)
    # the phase's own counters, by the markers the child wrote in front of every measured call
    arm, stat = None, {}
    for ln in r.stderr.splitlines():
        mk = re.match(r"\[bench\] (\S+) (\S)", ln)
        if mk:
            arm = (mk.group(1), mk.group(2))
        mk = re.search(r"site hits: (\d+) sites, (\d+) problems, (\d+) cells, ([0-9.]+) ms of kernels", ln)
        if mk and arm and arm[0] != "warmup":
            stat.setdefault(arm, []).append((int(mk.group(1)), int(mk.group(2)), int(mk.group(3)), float(mk.group(4))))
    for (panel, a), v in sorted(stat.items()):
        ms = [x[3] for x in v]
        print(f"{panel} arm {a}: {v[0][0]} sites, {v[0][1]} problems, {v[0][2]:.3e} executed cells, family-4 kernel time median "
              f"{statistics.median(ms):.1f} ms (min {min(ms):.1f}, max {max(ms):.1f}, n {len(ms)})")
    sys.exit(0)

import __graft_entry__ as entry  # noqa: E402
import synth  # noqa: E402

mod = entry.load()
p = mod.default_params()
rng = np.random.default_rng(1800)
panels = {m: [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=m).tobytes()) for _ in range(npanel)] for m in (20, 112)}
source = b"".join(panels[112] + panels[20])
dna = synth.planted_dna(int(mb * 1000000), 12345, source, every=1500, min_len=15, max_len=112)
engines = {"A": mod.Engine(0), "B": mod.Engine(0), "C": mod.Engine(0)}
engines["C"].set_option("site_short", 0)
print(f"planted record of {len(dna)} nt, {mod.segment_count(len(dna), p)} segments, panels of {npanel} oligos", flush=True)


def line(name, ts):
    print(f"{name:28s}: median {statistics.median(ts):.3f} s  min {min(ts):.3f}  max {max(ts):.3f}  n {len(ts)}   "
          f"({' '.join(f'{t:.3f}' for t in ts)})", flush=True)


for m, oligos in panels.items():
    lo, hi = 5, 5 * m
    while lo < hi:                               # the smallest V with at most `target` sites per oligo, the panel's mean
        mid = (lo + hi) // 2
        if sum(len(s[0]) for s in engines["A"].scan_oligos(oligos, dna, p, min_value=mid)) > target * len(oligos):
            lo = mid + 1
        else:
            hi = mid
    v = lo
    keep = {}

    def arm_a():
        keep["A"] = [s[0].array() for s in engines["A"].scan_oligos(oligos, dna, p, min_value=v)]

    def arm(key):
        s, h = engines[key].scan_oligos_aligned(oligos, dna, p, min_value=v)
        keep[key] = ([x[0].array() for x in s], [x[0].array() for x in h], sum(x[0].unaligned for x in h))

    arms = {"A": arm_a, "B": lambda: arm("B"), "C": lambda: arm("C")}
    times = {k: [] for k in arms}
    for i in range(rounds + 1):
        for name, fn in arms.items():
            if i:
                sys.stderr.write(f"[bench] {m}nt {name}\n")
                sys.stderr.flush()
            else:
                sys.stderr.write("[bench] warmup -\n")
                sys.stderr.flush()
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if i:
                times[name].append(dt)
            print(f"{m} nt, {'round ' + str(i) if i else 'warm-up'}, arm {name}: {dt:.3f} s", flush=True)
        for q in range(len(oligos)):
            if not (np.array_equal(keep["A"][q], keep["B"][0][q]) and np.array_equal(keep["B"][0][q], keep["C"][0][q])):
                sys.exit("the sites of the arms differ")
            if not np.array_equal(keep["B"][1][q], keep["C"][1][q]):
                sys.exit("the hits of site_short = 1 and 0 differ")
    nsites = sum(len(x) for x in keep["A"])
    print(f"{m}-nt panel: V = {v}, {nsites} sites ({nsites // len(oligos)} per oligo), {keep['B'][2]} unaligned", flush=True)
    line(f"{m} nt A scan_oligos", times["A"])
    line(f"{m} nt B aligned, site_short 1", times["B"])
    line(f"{m} nt C aligned, site_short 0", times["C"])
    ta, tb, tc = (statistics.median(times[k]) for k in "ABC")
    spread = max(max(times[k]) - min(times[k]) for k in "ABC")
    print(f"{m}-nt panel: hits phase B - A = {tb - ta:.3f} s ({nsites / max(tb - ta, 1e-9):.0f} sites/s), C - A = {tc - ta:.3f} s; "
          f"(C - A) / (B - A) = {(tc - ta) / max(tb - ta, 1e-9):.2f}; (C - A) - (B - A) = {tc - tb:.3f} s against a spread of the rounds of {spread:.3f} s",
          flush=True)
