#!/usr/bin/env python3
"""Cost of the alignment behind every variant score (fasim_score_variants_aligned) against the scores alone.
Run from the root of a built tree:

    python3 tools/variant_hits_bench.py [VARIANTS] [ROUNDS] [MB]
        The workload of tools/variants_bench.py: VARIANTS random SNVs (default 2 000) on a synthetic record of MB Mb (default 2),
        flank 300, all 48 encodings, once with H19 and once with a 20-nt oligo cut from it.  After a warm-up round, ROUNDS
        alternating rounds (default 5) of two arms:
            A = Engine.score_variants (resident record),
            B = Engine.score_variants_aligned of the same call.
        Medians and ranges of the wall clock, the HIP-event time of the kernels of each arm (B: k_touch and k_touch_path), the
        number of hits and how many of them are unaligned.  The scores of the two arms are compared.
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
p = mod.default_params()
eng = mod.Engine(0)
eng.load_dna(dna)
print(f"{nvar} SNVs, flank {FLANK}, record of {n} nt, 48 encodings; {rounds} rounds after a warm-up")


def arm_a(query):
    t0 = time.perf_counter()
    values, _, _ = eng.score_variants(variants, None, p, flank=FLANK, queries=[query])
    return time.perf_counter() - t0, dict(eng.last_variant_stats), values


def arm_b(query):
    t0 = time.perf_counter()
    values, _, _, _, hits = eng.score_variants_aligned(variants, None, p, flank=FLANK, queries=[query])
    dt = time.perf_counter() - t0
    return dt, dict(eng.last_variant_stats), values, int((values > 0).sum()), hits[0].unaligned


for name, query in (("H19 (2 812 nt)", h19), ("oligo (20 nt)", oligo)):
    arm_a(query), arm_b(query)
    ta, tb, sa, sb, nh, un = [], [], None, None, 0, 0
    for _ in range(rounds):
        dt, sa, va = arm_a(query)
        ta.append(dt)
        dt, sb, vb, nh, un = arm_b(query)
        tb.append(dt)
        assert np.array_equal(va, vb)
    ma, mb_ = statistics.median(ta), statistics.median(tb)
    print(f"{name}: A score_variants median {ma * 1e3:.1f} ms (min {min(ta) * 1e3:.1f}, max {max(ta) * 1e3:.1f}); "
          f"kernels {sa['kernel_s'] * 1e3:.1f} ms; {sa['problems']} problems, {sa['cells']:.3e} cells")
    print(f"{name}: B score_variants_aligned median {mb_ * 1e3:.1f} ms (min {min(tb) * 1e3:.1f}, max {max(tb) * 1e3:.1f}); "
          f"kernels {sb['kernel_s'] * 1e3:.1f} ms; {nh} hits, {un} unaligned; B / A = {mb_ / ma:.2f}")
eng.close()
