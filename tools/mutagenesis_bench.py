#!/usr/bin/env python3
"""Cost of an in-silico saturation mutagenesis (fasim_score_mutagenesis) against the route the project had
before: a generated list of the same SNVs through fasim_score_variants.  Run from the root of a built tree:

    python3 tools/mutagenesis_bench.py [INTERVALS] [ROUNDS] [POSITIONS] [ARMS]
        INTERVALS intervals (default 20) of POSITIONS positions (default 1 000) spread over a synthetic record of 2 Mb, all 48
        encodings, once with H19 and once with a 20-nt oligo cut from it.  Arms (ARMS: a comma list, default all):
            a300, a2048   uniform random DNA, flank 300 and 2 048
            b300          A/G-only DNA (a purine tract never lets a problem die), flank 300
        Per arm and query, after a warm-up round, ROUNDS alternating rounds (default 5) of
            M = Engine.score_mutagenesis(intervals),
            V = Engine.score_variants(mutagenesis_variants(intervals)) with the same flank -- each SNV in its own, smaller window,
                so V's values may be lower; the comparison is of cost.
        Medians and max / min spreads of the wall clock, M's HIP-event times of k_mut_prefix and k_mut_touch, cont_cols /
        cont_cols_bound and the columns per problem.  The record is passed, not resident, in both arms.
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
nint = int(args[0]) if len(args) > 0 else 20
rounds = int(args[1]) if len(args) > 1 else 5
npos = int(args[2]) if len(args) > 2 else 1000
arms = args[3].split(",") if len(args) > 3 else ["a300", "a2048", "b300"]

mod = entry.load()
h19 = synth.read_fasta(os.path.join(entry.ROOT, "tests", "golden", "H19.fa"))[1]
oligo = h19[1000:1020]
N = 2_000_000
random_dna = synth.random_dna(N, 26)
purine_dna = bytes(np.where(np.random.default_rng(27).integers(0, 2, N) == 1, ord("A"), ord("G")).astype(np.uint8))
step = (N - 10_000) // nint
intervals = [(0, 5000 + k * step, 5000 + k * step + npos) for k in range(nint)]
p = mod.default_params()
eng = mod.Engine(0)
print(f"{nint} intervals of {npos} positions on a record of {N} nt, 48 encodings; {rounds} rounds after a warm-up")


def spread(t):
    return max(t) / min(t)


for arm in arms:
    dna = purine_dna if arm[0] == "b" else random_dna
    flank = int(arm[1:])
    variants = mod.mutagenesis_variants(intervals, [dna])
    for name, query in (("H19 (2 812 nt)", h19), ("oligo (20 nt)", oligo)):
        def run_m():
            t0 = time.perf_counter()
            values = eng.score_mutagenesis(intervals, [dna], p, flank=flank, queries=[query])[0]
            return time.perf_counter() - t0, dict(eng.last_mutagenesis_stats), int(values.max())

        def run_v():
            t0 = time.perf_counter()
            values = eng.score_variants(variants, [dna], p, flank=flank, queries=[query])[0]
            return time.perf_counter() - t0, dict(eng.last_variant_stats), int(values.max())
        run_m(), run_v()
        tm, tv, sm, sv = [], [], None, None
        for _ in range(rounds):
            dt, sm, top_m = run_m()
            tm.append(dt)
            dt, sv, top_v = run_v()
            tv.append(dt)
        mm, mv = statistics.median(tm), statistics.median(tv)
        print(f"{arm} {name}: M score_mutagenesis median {mm * 1e3:.1f} ms (spread {spread(tm):.3f}); {sm['problems']} problems in {sm['launches']} launches, "
              f"k_mut_prefix {sm['prefix_s'] * 1e3:.1f} ms for {sm['prefix_cols']} columns, k_mut_touch {sm['cont_s'] * 1e3:.1f} ms for {sm['cont_cols']} columns = "
              f"{sm['cont_cols'] / sm['cont_cols_bound']:.4f} of the bound, {sm['cont_cols'] / sm['problems']:.1f} columns per problem; largest value {top_m}")
        print(f"{arm} {name}: V score_variants on {len(variants)} SNVs median {mv * 1e3:.1f} ms (spread {spread(tv):.3f}); {sv['problems']} problems, "
              f"k_touch {sv['kernel_s'] * 1e3:.1f} ms; largest value {top_v}; V / M = {mv / mm:.2f} "
              f"({'above' if mv / mm > spread(tv) else 'NOT above'} V's own spread)", flush=True)
eng.close()
