#!/usr/bin/env python3
"""Cost of the site counts on the device (fasim_scan_records_site_counts, k_hist_pairs) against the histogram it extends.  Run from the
root of a built tree:

    python3 tools/site_counts_bench.py scan [MB] [N] [V ...]   a planted record of MB Mb (default 50) x H19, N alternating rounds
                                                   (default 4) of
                                                   hist    = scan_hist(records=False), the yardstick,
                                                   counts  = scan_site_counts(records=False),
                                                   sites   = one scan_sites(min_value=V, max_gap=0, records=False) call per threshold V
                                                             (default 20 40 60 80 100): what there was for sites per threshold
    python3 tools/site_counts_bench.py kernel      one worker, one batch of 384 full segments: the HIP-event time of kernel family 4
                                                   for a histogram call and a site-counts call (k_hist against k_hist_pairs)
The first round of every arm is a warm-up and is not reported.  Every round compares the arrays: the positions of the site counts
with the histogram, and sites()[c][V] with the number of class-c sites of the call for V.  Bytes copied back per batch and query:
the histogram's 4 x 4 x (min(16383, 5 x 16 ceil(m / 16)) + 1) counters twice, 2 x 4 x 2 x (overlapLength + 1) zone values rounded up
to 8 per segment, 16 border values per slice of 2 040 positions and one byte per unit.
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

mode = sys.argv[1] if len(sys.argv) > 1 else "scan"
mod = entry.load()
eng = mod.Engine(0)
p = mod.default_params()
rna = synth.read_fasta("tests/golden/H19.fa")[1]


def line(name, ts):
    print(f"{name:8s}: median {statistics.median(ts):.3f} s  min {min(ts):.3f}  max {max(ts):.3f}  n {len(ts)}   "
          f"({' '.join(f'{t:.3f}' for t in ts)})", flush=True)


if mode == "kernel":
    eng.set_option("workers", 1)
    eng.set_option("seg_batch", 384)
    eng.set_query(rna)
    dnas = [mod.synth_dna(5000, 500 + k) for k in range(384)]
    for what in ("hist", "counts"):
        for _ in range(2):
            t0 = time.perf_counter()
            if what == "hist":
                eng.scan_hist(dnas, p)
            else:
                eng.scan_site_counts(dnas, p)
            dt = time.perf_counter() - t0
        st = eng.last_totals[0]
        print(f"{what}: {st['segments']} segments, {st['units']} units, call {dt:.3f} s, family-4 kernel_ms {st['kernel_ms'][4]:.3f} in "
              f"{st['kernel_launches'][4]} launches (k_encode and the fold), k_scan {st['kernel_ms'][0]:.3f} ms", flush=True)
    sys.exit(0)

mb = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 4
values = [int(v) for v in sys.argv[4:]] or [20, 40, 60, 80, 100]
dna = synth.planted_dna(mb * 1000000, 12345, rna)
nseg = mod.segment_count(len(dna), p)
eng.set_query(rna)
keep = {}
print(f"scan: planted record of {len(dna)} nt x H19 ({len(rna)} nt), {nseg} segments, thresholds {values}", flush=True)


def hist():
    keep["hist"] = eng.scan_hist(dna, p)[1].array()


def counts():
    keep["counts"] = eng.scan_site_counts(dna, p)[1]


def sites():
    out = []
    for v in values:
        st = eng.scan_sites(dna, p, min_value=v, max_gap=0, records=False)[1]
        rows = (st[0] if isinstance(st, (list, tuple)) else st).array()
        out.append([int((rows[:, 0] == c).sum()) for c in range(4)])
    keep["sites"] = out


arms = {"hist": hist, "counts": counts, "sites": sites}
times = {k: [] for k in arms}
for i in range(rounds + 1):
    for name, fn in arms.items():
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i:
            times[name].append(dt)
    if not np.array_equal(keep["counts"].array()[0], keep["hist"]):
        sys.exit("the positions of the site counts differ from the histogram")
    per_v = keep["counts"].sites()
    if [[int(per_v[c, v]) for c in range(4)] for v in values] != keep["sites"]:
        sys.exit("sites() differs from the number of sites scan_sites() reports")
for name in arms:
    line(name, times[name])
th, tc, ts = (statistics.median(times[k]) for k in ("hist", "counts", "sites"))
spread = max(times["hist"]) - min(times["hist"])
print(f"site counts against the histogram: {tc:.3f} s against {th:.3f} s, {tc - th:+.3f} s (spread of the histogram rounds {spread:.3f} s); "
      f"{len(values)} scan_sites calls {ts:.3f} s = {ts / tc:.2f} x", flush=True)
top = min(mod.HIST_BINS - 1, 5 * 16 * ((len(rna) + 15) // 16))
batches = (nseg + 383) // 384
zs = (p.overlapLength + 1 + 7) & ~7
print(f"bytes copied back: histogram about {batches * 16 * (top + 1) + nseg * 16 * p.overlapLength + nseg * 48}; site counts about "
      f"{batches * 32 * (top + 1) + nseg * 16 * zs + nseg * 16 * -(-p.cutLength // 2040) + nseg * 48} ({batches} batches or more)", flush=True)
