#!/usr/bin/env python3
"""Cost of an oligo panel (fasim_scan_oligos, k_scan_short) against the cheapest thing k_scan can do.  Run from the root of a built
tree, on one GPU:

    python3 tools/oligo_bench.py [MB] [N] [NQ]     a planted record of MB Mb (default 5), one warm-up round and N alternating rounds
                                                   (default 4) of
                                                   o20   = scan_oligos of a panel of NQ (default 64) oligos of 20 nt, sites at V = 60,
                                                   o112  = the same for NQ oligos of 112 nt, sites at V = 200,
                                                   q113  = scan_sites(records=False) of ONE 113-nt query at V = 200: k_scan's smallest
                                                           query, the same encode / k_sites / merge around it
The oligos are windows of H19.  Reported: seconds per oligo and Mb for o20 and o112, seconds per Mb for q113, each as the median
with the smallest and largest round, the spread (max - min) of the rounds, and the kernel time of family 0 (the scan kernels) of
the last round.  The bar of DESIGN.md section 16: a 20-nt oligo must cost less than the 113-nt k_scan query by more than the spread.
"""
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import __graft_entry__ as entry  # noqa: E402
import synth  # noqa: E402

mb = int(sys.argv[1]) if len(sys.argv) > 1 else 5
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 4
nq = int(sys.argv[3]) if len(sys.argv) > 3 else 64
mod = entry.load()
eng = mod.Engine(0)
p = mod.default_params()
h19 = synth.read_fasta("tests/golden/H19.fa")[1]
dna = synth.planted_dna(mb * 1000000, 12345, h19)
panel20 = [h19[100 + 31 * k:100 + 31 * k + 20] for k in range(nq)]
panel112 = [h19[100 + 31 * k:100 + 31 * k + 112] for k in range(nq)]
q113 = h19[700:813]
print(f"planted record of {len(dna)} nt, {mod.segment_count(len(dna), p)} segments, 48 encodings; panels of {nq} oligos", flush=True)
keep = {}


def o20():
    keep["o20"] = sum(len(s[0]) for s in eng.scan_oligos(panel20, dna, p, min_value=60))
    keep["o20_ms"] = sum(t["kernel_ms"][0] for t in eng.last_totals)


def o112():
    keep["o112"] = sum(len(s[0]) for s in eng.scan_oligos(panel112, dna, p, min_value=200))
    keep["o112_ms"] = sum(t["kernel_ms"][0] for t in eng.last_totals)


def k113():
    keep["q113"] = len(eng.scan_sites(dna, p, min_value=200, records=False, rnas=[q113])[1][0][0])
    keep["q113_ms"] = sum(t["kernel_ms"][0] for t in eng.last_totals)


arms = {"o20": (o20, nq), "o112": (o112, nq), "q113": (k113, 1)}
times = {k: [] for k in arms}
for i in range(rounds + 1):
    for name, (fn, _) in arms.items():
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i:
            times[name].append(dt)
per = {}
for name, (_, n) in arms.items():
    ts = [t / n / mb for t in times[name]]
    per[name] = ts
    print(f"{name:5s}: median {statistics.median(ts) * 1e3:9.4f} ms per {'oligo and ' if n > 1 else ''}Mb   min {min(ts) * 1e3:9.4f}  max {max(ts) * 1e3:9.4f}  "
          f"spread {(max(ts) - min(ts)) * 1e3:8.4f}  n {len(ts)}   calls: {' '.join(f'{t:.3f}' for t in times[name])} s   "
          f"scan kernels of the last round {keep[name + '_ms']:.1f} ms   sites {keep[name]}", flush=True)
m20, m113 = statistics.median(per["o20"]), statistics.median(per["q113"])
spread = max(max(per[k]) - min(per[k]) for k in ("o20", "q113"))
verdict = "below it by more than the spread" if m113 - m20 > spread else "NOT below it by more than the spread"
print(f"a 20-nt oligo costs {m20 * 1e3:.4f} ms per Mb, the 113-nt k_scan query {m113 * 1e3:.4f} ms per Mb ({m113 / m20:.2f} x): {verdict} "
      f"({spread * 1e3:.4f} ms)", flush=True)
