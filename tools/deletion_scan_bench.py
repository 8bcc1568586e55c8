#!/usr/bin/env python3
"""Cost of a deletion scan (fasim_score_deletions) against the route the project had before: a generated list
of the same deletions through fasim_score_variants.  Run from the root of a built tree:

    python3 tools/deletion_scan_bench.py [INTERVALS] [ROUNDS] [POSITIONS] [ARMS] [LENGTHS]
        INTERVALS intervals (default 4) of POSITIONS positions (default 1 000) spread over a synthetic record of 2 Mb, all 48
        encodings, deletion lengths LENGTHS (default 1,5,20), once with H19 and once with a 20-nt oligo cut from it.  Arms (ARMS: a
        comma list, default all):
            a300, a2048   uniform random DNA, flank 300 and 2 048
            b300          A/G-only DNA (a purine tract never lets a problem die), flank 300
        Per arm and query, after a warm-up round, ROUNDS alternating rounds (default 5) of
            D = Engine.score_deletions(intervals, lengths),
            V = Engine.score_variants(deletion_variants(intervals, lengths)) with the same flank -- each deletion in its own,
                smaller window, so V's values may be lower; the comparison is of cost.
        Every round checks D against V: no value of D is below V's, and, where the context fits score_variants' widest window (at
        most 2 048 letters on either side of every deletion), the first interval's first deletions on the cut-out context
        dna[lo:hi] give D's values and encodings exactly.
        Medians and max / min spreads of the wall clock, D's HIP-event times of k_mut_prefix_pm and k_mut_jump, cont_cols /
        cont_cols_bound and the columns per jump problem.  The record is passed, not resident, in both arms.
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
nint = int(args[0]) if len(args) > 0 else 4
rounds = int(args[1]) if len(args) > 1 else 5
npos = int(args[2]) if len(args) > 2 else 1000
arms = args[3].split(",") if len(args) > 3 else ["a300", "a2048", "b300"]
lengths = tuple(int(d) for d in args[4].split(",")) if len(args) > 4 else (1, 5, 20)

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
print(f"{nint} intervals of {npos} positions on a record of {N} nt, lengths {lengths}, 48 encodings; {rounds} rounds after a warm-up")
SUBSET = 24      # deletions of the first interval that every round scores on the cut-out context as well


def spread(t):
    return max(t) / min(t)


for arm in arms:
    dna = purine_dna if arm[0] == "b" else random_dna
    flank = int(arm[1:])
    variants = mod.deletion_variants(intervals, [dna], lengths)
    # (position, length index) of every variant in D's arrays: deletion_variants lists the clean deletions in table order
    where = [(k * npos + x, li) for k in range(nint) for x in range(npos) for li, d in enumerate(lengths) if x + d < npos]
    assert len(where) == len(variants)
    at = tuple(np.array(w) for w in zip(*where))
    lo, hi = max(0, intervals[0][1] - flank), min(N, intervals[0][2] + flank)
    fits = intervals[0][1] - lo + SUBSET <= mod.MAX_FLANK and hi - intervals[0][1] <= mod.MAX_FLANK      # the cut-out record lies inside every window
    cut_out = [v._replace(pos=v.pos - lo) for v in variants[:SUBSET]]
    for name, query in (("H19 (2 812 nt)", h19), ("oligo (20 nt)", oligo)):
        def run_d():
            t0 = time.perf_counter()
            values, encs = eng.score_deletions(intervals, [dna], p, flank=flank, lengths=lengths, queries=[query])[:2]
            return time.perf_counter() - t0, dict(eng.last_deletion_stats), values[0], encs[0]

        def run_v():
            t0 = time.perf_counter()
            values = eng.score_variants(variants, [dna], p, flank=flank, queries=[query])[0]
            return time.perf_counter() - t0, dict(eng.last_variant_stats), values[0]
        run_d(), run_v()
        td, tv, sd, sv = [], [], None, None
        for _ in range(rounds):
            dt, sd, vd, ed = run_d()
            td.append(dt)
            dt, sv, vv = run_v()
            tv.append(dt)
            assert (vd[at] >= vv).all(), "a value of score_deletions is below score_variants'"
            if fits:
                vc, ec, _ = eng.score_variants(cut_out, [dna[lo:hi]], p, flank=mod.MAX_FLANK, queries=[query])
                sub = tuple(a[:SUBSET] for a in at)
                assert np.array_equal(vd[sub], vc[0]) and np.array_equal(ed[sub], ec[0]), "score_deletions differs from score_variants on the cut-out context"
        md, mv = statistics.median(td), statistics.median(tv)
        jumps = sd["own_problems"] + sd["alt_problems"]
        print(f"{arm} {name}: D score_deletions median {md * 1e3:.1f} ms (spread {spread(td):.3f}); {sd['deletions']} deletions, {sd['own_problems']} own-letter and "
              f"{sd['alt_problems']} ALT problems in {sd['launches']} launches, k_mut_prefix_pm {sd['prefix_s'] * 1e3:.1f} ms for {sd['prefix_cols']} columns, "
              f"k_mut_jump {sd['cont_s'] * 1e3:.1f} ms for {sd['cont_cols']} columns = {sd['cont_cols'] / sd['cont_cols_bound']:.4f} of the bound, "
              f"{sd['cont_cols'] / jumps:.1f} columns per problem; largest value {int(vd.max())}")
        print(f"{arm} {name}: V score_variants on {len(variants)} deletions median {mv * 1e3:.1f} ms (spread {spread(tv):.3f}); {sv['problems']} problems, "
              f"k_touch {sv['kernel_s'] * 1e3:.1f} ms; largest value {int(vv.max())}; V / D = {mv / md:.2f} "
              f"({'above' if mv / md > spread(tv) else 'NOT above'} V's own spread); cut-out check {'passed every round' if fits else 'not possible at this flank (D >= V checked)'}",
              flush=True)
eng.close()
