#!/usr/bin/env python3
"""Cost of giving every site its hit (fasim_scan_records_sites_aligned).  Run from the root of a built tree:

    python3 tools/site_align_bench.py scan [MB] [N] [dense]
        a planted record of MB Mb (default 50) x H19, a warm-up round and N alternating rounds (default 4) of two arms,
            A = scan_sites(records=False), the parent's call, in the same build,
            B = scan_sites_aligned(records=False),
        at V = int(0.8 x the record's largest potential); with `dense` the same two arms again at V = the median of the non-zero
        potential (hundreds of thousands of sites: every site runs its own forward pass, so this takes long).  Medians and ranges,
        sites per second and executed DP cells per second of the align phase (B - A).
    python3 tools/site_align_bench.py phase [MB] [V]
        one warm-up and one measured aligned call in a child process under FASIM_PROFILE=1, whose `[fasim prof] site hits:` line
        carries the phase's own counts (sites, problems, executed cells) and the HIP-event time of its kernels.
The expectation from the cell counts is printed before anything is measured: pass (i) is m * (jp + 1) cells per problem, pass (ii)
(i1 + 1) * (j1 - j0 + 1), pass (iii) the rectangle.
"""
import os
import statistics
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
sys.path.insert(0, "tests")
import __graft_entry__ as entry  # noqa: E402
import synth  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "scan"
mb = int(sys.argv[2]) if len(sys.argv) > 2 else 50

if mode == "phase":
    # the child initialises the GPU; this process never does
    env = dict(os.environ, FASIM_PROFILE="1")
    r = subprocess.run([sys.executable, __file__, "phase-child", str(mb)] + sys.argv[3:4], env=env, capture_output=True, text=True)
    sys.stdout.write(r.stdout)
    for ln in r.stderr.splitlines():
        if "site hits:" in ln:
            print(ln)
    sys.exit(r.returncode)

mod = entry.load()
p = mod.default_params()
rna = synth.read_fasta("tests/golden/H19.fa")[1]
dna = synth.planted_dna(mb * 1000000, 12345, rna)
eng = mod.Engine(0)
eng.set_query(rna)
print(f"planted record of {len(dna)} nt x H19 ({len(rna)} nt), {mod.segment_count(len(dna), p)} segments", flush=True)

if mode == "phase-child":
    if len(sys.argv) > 3:
        v = int(sys.argv[3])
    else:
        v = int(0.8 * int(eng.scan_track(dna, p, bin=1, records=False)[1].array().max()))
    for k in range(2):
        t0 = time.perf_counter()
        _, s, h = eng.scan_sites_aligned(dna, p, min_value=v, records=False)
        print(f"call {k}: V = {v}, {len(s[0])} sites, {h[0].unaligned} unaligned, {time.perf_counter() - t0:.3f} s", flush=True)
    sys.exit(0)

rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 4
track0 = eng.scan_track(dna, p, bin=1, records=False)[1].array()
top = int(track0.max())
cases = [("sparse", int(0.8 * top))]
if "dense" in sys.argv[4:]:
    cases.append(("dense", int(np.median(track0[track0 > 0]))))
del track0


def line(name, ts):
    print(f"{name:18s}: median {statistics.median(ts):.3f} s  min {min(ts):.3f}  max {max(ts):.3f}  n {len(ts)}   "
          f"({' '.join(f'{t:.3f}' for t in ts)})", flush=True)


for what, v in cases:
    _, s = eng.scan_sites(dna, p, min_value=v, records=False)
    a = s[0].array()
    step = p.cutLength - p.overlapLength
    off = a[:, 4] % step
    jp = np.where(a[:, 5] & 1, p.cutLength - 1 - off, off)
    cells = int((len(rna) * (jp + 1)).sum())
    print(f"{what}: V = {v}, {len(a)} sites; expectation: pass (i) alone is about {cells:.3e} cells "
          f"(m x (jp + 1) per site, one problem per site outside the overlaps)", flush=True)
    keep = {}

    def arm_a():
        keep["a"] = eng.scan_sites(dna, p, min_value=v, records=False)[1][0].array()

    def arm_b():
        _, s, h = eng.scan_sites_aligned(dna, p, min_value=v, records=False)
        keep["b"] = (s[0].array(), h[0].array(), h[0].unaligned)

    arms = {"A scan_sites": arm_a, "B scan_sites_aligned": arm_b}
    times = {k: [] for k in arms}
    for i in range(rounds + 1):
        for name, fn in arms.items():
            t0 = time.perf_counter()
            fn()
            dt = time.perf_counter() - t0
            if i:
                times[name].append(dt)
        if not np.array_equal(keep["a"], keep["b"][0]):
            sys.exit("the sites of the two calls differ")
    for name in arms:
        line(name, times[name])
    ta, tb = (statistics.median(times[k]) for k in arms)
    hb = keep["b"][1]
    rect = int(((hb[:, 3] - hb[:, 2] + 1) * (hb[:, 5] - hb[:, 4] + 1) + (hb[:, 3] + 1) * (hb[:, 5] - hb[:, 4] + 1))[hb[:, 7] >= 0].sum())
    print(f"{what}: align phase (B - A) {tb - ta:.3f} s for {len(hb)} sites ({keep['b'][2]} unaligned): {len(hb) / max(tb - ta, 1e-9):.0f} sites/s, "
          f"{(cells + rect) / max(tb - ta, 1e-9):.3e} executed cells/s (pass (i) {cells:.3e} + passes (ii), (iii) {rect:.3e})", flush=True)
