#!/usr/bin/env python3
"""Cost of scoring variants by the triplex potential through them (fasim_score_variants).  Run from the root
of a built tree:

    python3 tools/variants_bench.py [VARIANTS] [ROUNDS] [MB]
        VARIANTS random SNVs (default 2 000) on a synthetic record of MB Mb (default 2), flank 300, all 48 encodings, once with H19
        and once with a 20-nt oligo cut from it.  After a warm-up round, ROUNDS alternating rounds (default 5) of two arms:
            A = Engine.score_variants (resident record),
            B = the route the project had before: one window record per allele, 2 x VARIANTS records of 601 nt, through
                scan_records_track(bin=0, records=False) for H19 and through scan_oligos (one track bin per window) for the oligo.
        B computes the peak of each window, not the value through the variant, so the comparison is of cost only.
        Medians and ranges of the wall clock, and for A the problems, the cells and the HIP-event time of k_touch.
"""
import os
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")

import numpy as np  # noqa: E402

import synth  # noqa: E402
import __graft_entry__ as entry  # noqa: E402

args = sys.argv[1:]
nvar = int(args[0]) if len(args) > 0 else 2000
rounds = int(args[1]) if len(args) > 1 else 5
mb = float(args[2]) if len(args) > 2 else 2
FLANK = 300

mod = entry.load()
h19 = synth.read_fasta(os.path.join(entry.ROOT, "tests", "golden", "H19.fa"))[1]
oligo = h19[1000:1020]
n = int(mb * 1e6)
dna = synth.random_dna(n, 18)
rng = np.random.default_rng(18)
pos = np.sort(rng.integers(FLANK, n - FLANK - 1, size=nvar))
other = {65: "C", 67: "G", 71: "T", 84: "A"}
variants = [mod.Variant(k + 1, "chrS", int(a), f"v{k}", chr(dna[a]), other[dna[a]]) for k, a in enumerate(pos)]
windows = []
for v in variants:
    lo, hi = v.pos - FLANK, v.pos + 1 + FLANK
    windows.append(dna[lo:hi])
    windows.append(dna[lo:v.pos] + v.alt.encode() + dna[v.pos + 1:hi])
p = mod.default_params()
eng = mod.Engine(0)
eng.load_dna(dna)
print(f"{nvar} SNVs, flank {FLANK}, record of {n} nt, 48 encodings; {rounds} rounds after a warm-up")


def arm_a(query):
    t0 = time.perf_counter()
    values, _, _ = eng.score_variants(variants, None, p, flank=FLANK, queries=[query])
    return time.perf_counter() - t0, dict(eng.last_variant_stats), int(values.max())


def arm_b(query):
    t0 = time.perf_counter()
    if len(query) > mod.MAX_OLIGO:
        _, _, peaks = eng.scan_records_track(windows, p, rnas=[query], bin=0, records=False)
        top = int(peaks[0, :, :, 0].max())
    else:
        _, tracks = eng.scan_oligos([query], windows, p, min_value=16383, track_bin=1024)
        top = max(int(t.array().max()) for t in tracks[0])
    return time.perf_counter() - t0, top


for name, query in (("H19 (2 812 nt)", h19), ("oligo (20 nt)", oligo)):
    arm_a(query), arm_b(query)
    ta, tb, st = [], [], None
    for _ in range(rounds):
        dt, st, top_a = arm_a(query)
        ta.append(dt)
        dt, top_b = arm_b(query)
        tb.append(dt)
    ks = st["kernel_s"]
    print(f"{name}: A score_variants median {statistics.median(ta) * 1e3:.1f} ms (min {min(ta) * 1e3:.1f}, max {max(ta) * 1e3:.1f}); "
          f"{st['problems']} problems, {st['cells']:.3e} cells, k_touch {ks * 1e3:.1f} ms = {st['cells'] / ks / 1e9:.2f} Gcells/s; "
          f"largest value {top_a}")
    print(f"{name}: B window records median {statistics.median(tb) * 1e3:.1f} ms (min {min(tb) * 1e3:.1f}, max {max(tb) * 1e3:.1f}); "
          f"largest window peak {top_b}; A / B = {statistics.median(ta) / statistics.median(tb):.2f}")
eng.close()
