#!/usr/bin/env python3
"""Cost of the per-base profile and of the screen of an oligo panel (fasim_scan_oligos_profile, fasim_scan_oligos_peaks, DESIGN.md
section 24).  Run from the root of a built tree:

    python3 tools/oligo_profile_bench.py [MB] [OLIGOS] [ROUNDS]
        a record of MB Mb (default 5) planted with pieces of the panels, and three panels of OLIGOS oligos (default 64) of 20, 48 and
        112 nt.  Per panel a warm-up round and ROUNDS alternating rounds (default 4) of four arms,
            A = scan_oligos, sites only (min_value = 4 m: k_scan_short and k_sites, what the parent does on this record),
            B = scan_oligos_profile                        (k_scan_short_rows and k_rowfold_parts),
            C = scan_oligos with track_bin = 1 and argmax in numpy (k_scan_short, k_sites and k_track; 4 x 2 x N bytes per oligo),
            D = scan_oligos_peaks                          (k_scan_short and k_track's peak variant; 64 bytes per slice);
        every round checks that D's values and positions are C's maxima and first argmaxima and that B's largest row maximum per
        class is D's value.  Medians and ranges, B / A and D / C.
"""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
sys.path.insert(0, "tests")

import __graft_entry__ as entry  # noqa: E402
import synth  # noqa: E402

args = sys.argv[1:]
mb = float(args[0]) if len(args) > 0 else 5
npanel = int(args[1]) if len(args) > 1 else 64
rounds = int(args[2]) if len(args) > 2 else 4

mod = entry.load()
p = mod.default_params()
rng = np.random.default_rng(2500)
panels = {m: [bytes(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=m).tobytes()) for _ in range(npanel)] for m in (20, 48, 112)}
source = b"".join(panels[112] + panels[48] + panels[20])
dna = synth.planted_dna(int(mb * 1000000), 12345, source, every=1500, min_len=15, max_len=112)
eng = mod.Engine(0)
print(f"planted record of {len(dna)} nt, {mod.segment_count(len(dna), p)} segments, panels of {npanel} oligos", flush=True)


def line(name, ts):
    print(f"{name:34s}: median {statistics.median(ts):.3f} s  min {min(ts):.3f}  max {max(ts):.3f}  n {len(ts)}   "
          f"({' '.join(f'{t:.3f}' for t in ts)})", flush=True)


for m, oligos in panels.items():
    keep = {}

    def arm_a():
        keep["A"] = eng.scan_oligos(oligos, dna, p, min_value=4 * m)

    def arm_b():
        keep["B"] = np.array([x.array().max(axis=1) for x in eng.scan_oligos_profile(oligos, dna, p)], dtype=np.int64)

    def arm_c():
        _, tracks = eng.scan_oligos(oligos, dna, p, min_value=4 * m, track_bin=1)
        arrs = [t[0].array() for t in tracks]
        keep["C"] = np.array([[[int(a[c].max()), int(np.argmax(a[c]))] for c in range(4)] for a in arrs], dtype=np.int64)

    def arm_d():
        keep["D"] = eng.scan_oligos_peaks(oligos, dna, p)[:, 0, :, :2]

    arms = {"A": arm_a, "B": arm_b, "C": arm_c, "D": arm_d}
    times = {k: [] for k in arms}
    for i in range(rounds + 1):
        for name, fn in arms.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if i:
                times[name].append(dt)
            print(f"{m} nt, {'round ' + str(i) if i else 'warm-up'}, arm {name}: {dt:.3f} s", flush=True)
        c = keep["C"].copy()
        c[c[:, :, 0] == 0, 1] = -1
        if not np.array_equal(c, keep["D"]):
            sys.exit("the peaks differ from the tracks' maxima")
        if not np.array_equal(keep["B"], keep["D"][:, :, 0]):
            sys.exit("the largest row maxima differ from the peaks' values")
    line(f"{m} nt A scan_oligos, sites", times["A"])
    line(f"{m} nt B scan_oligos_profile", times["B"])
    line(f"{m} nt C scan_oligos, tracks + argmax", times["C"])
    line(f"{m} nt D scan_oligos_peaks", times["D"])
    ta, tb, tc, td = (statistics.median(times[k]) for k in "ABCD")
    print(f"{m}-nt panel: B / A = {tb / ta:.2f}, D / C = {td / tc:.2f}; spread of the rounds "
          f"{max(max(times[k]) - min(times[k]) for k in 'ABCD'):.3f} s", flush=True)
