#!/usr/bin/env python3
"""Cost of scoring variants on a sample's haplotypes (fasim_score_haplotypes) beside fasim_score_variants.  Run
from the root of a built tree:

    python3 tools/haplotypes_bench.py [VARIANTS] [ROUNDS] [MB] [PARENT]
        VARIANTS SNVs (default 2 000) in pairs 100 bases apart on a synthetic record of MB Mb (default 2), flank 300, all 48
        encodings, once with H19 and once with a 20-nt oligo cut from it.  After a warm-up round, ROUNDS alternating rounds
        (default 5) of the arms
            V  = Engine.score_variants of this build (resident record),
            P  = Engine.score_variants of the built tree PARENT (the commit before; left out, as PHa and PHb, when no PARENT is
                 given),
            Ha = Engine.score_haplotypes, genotypes (a): every SNV an unphased heterozygote (0/1), so no window has an applied
                 neighbour in reach and every haplotype takes the plain windows,
            Hb = Engine.score_haplotypes, genotypes (b): all SNVs on haplotype 0, so every window of haplotype 0 holds one
                 neighbour and haplotype 1 takes the plain windows,
            PHa, PHb = Engine.score_haplotypes of PARENT on the same genotypes.
        Medians and ranges of the wall clock and of k_touch's time, the ratios Ha / V and Hb / V, every arm against its parent arm
        with the parent arm's own spread (max / min of its rounds), problems and cells.
"""
import importlib.util
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
parent_dir = args[3] if len(args) > 3 else None
FLANK = 300

mod = entry.load()
h19 = synth.read_fasta(os.path.join(entry.ROOT, "tests", "golden", "H19.fa"))[1]
oligo = h19[1000:1020]
n = int(mb * 1e6)
dna = synth.random_dna(n, 26)
step = (n - 4 * FLANK) // (nvar // 2)
assert step > 2 * FLANK + 200, "the pairs must be out of each other's reach"
pos = [2 * FLANK + k * step + d for k in range(nvar // 2) for d in (0, 100)]
other = {65: "C", 67: "G", 71: "T", 84: "A"}
variants = [mod.Variant(k + 1, "chrS", a, f"v{k}", chr(dna[a]), other[dna[a]]) for k, a in enumerate(pos)]
gt_a = np.array([(0, 1, 0)] * len(variants), dtype=np.int8)
gt_b = np.array([(1, 0, 1)] * len(variants), dtype=np.int8)
p = mod.default_params()
eng = mod.Engine(0)
eng.load_dna(dna)
parent = peng = None
if parent_dir:
    spec = importlib.util.spec_from_file_location("fasim_parent", os.path.join(parent_dir, "fasim-longtarget_amd", "__init__.py"))
    parent = importlib.util.module_from_spec(spec)
    sys.modules["fasim_parent"] = parent
    spec.loader.exec_module(parent)
    peng = parent.Engine(0)
    peng.load_dna(dna)
    pvars = [parent.Variant(*v) for v in variants]
    pp = parent.default_params()
print(f"{len(variants)} SNVs in pairs 100 apart, flank {FLANK}, record of {n} nt, 48 encodings; {rounds} rounds after a warm-up")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


for name, query in (("H19 (2 812 nt)", h19), ("oligo (20 nt)", oligo)):
    arms = {"V": lambda: eng.score_variants(variants, None, p, flank=FLANK, queries=[query]),
            "Ha": lambda: eng.score_haplotypes(variants, gt_a, None, p, flank=FLANK, queries=[query]),
            "Hb": lambda: eng.score_haplotypes(variants, gt_b, None, p, flank=FLANK, queries=[query])}
    if peng:
        arms["P"] = lambda: peng.score_variants(pvars, None, pp, flank=FLANK, queries=[query])
        arms["PHa"] = lambda: peng.score_haplotypes(pvars, gt_a, None, pp, flank=FLANK, queries=[query])
        arms["PHb"] = lambda: peng.score_haplotypes(pvars, gt_b, None, pp, flank=FLANK, queries=[query])
    times = {k: [] for k in arms}
    kernel = {k: [] for k in arms}
    stats = {}
    for r in range(rounds + 1):
        for k, fn in arms.items():
            dt, out = timed(fn)
            stats[k] = (dict((peng if k.startswith("P") else eng).last_variant_stats), out)
            if r:
                times[k].append(dt)
                kernel[k].append(stats[k][0]["kernel_s"])
    plain = stats["V"][1]
    assert np.array_equal(stats["Ha"][1][0][:, :, 0], plain[0]) and np.array_equal(stats["Ha"][1][0][:, :, 1], plain[0])
    assert np.array_equal(stats["Hb"][1][0][:, :, 1], plain[0]) and (stats["Hb"][1][2][0, :, 0, 1] == 1).all()
    if peng:
        assert np.array_equal(stats["P"][1][0], plain[0]) and np.array_equal(stats["P"][1][1], plain[1])
        for k in ("Ha", "Hb"):
            assert all(np.array_equal(a, b) for a, b in zip(stats[k][1], stats["P" + k][1])) and stats[k][0]["problems"] == stats["P" + k][0]["problems"]
    med = {k: statistics.median(t) for k, t in times.items()}
    for k, t in times.items():
        st = stats[k][0]
        print(f"{name}: {k:2s} median {med[k] * 1e3:8.1f} ms (min {min(t) * 1e3:.1f}, max {max(t) * 1e3:.1f}); {st['problems']} problems, "
              f"{st['cells']:.3e} cells, k_touch median {statistics.median(kernel[k]) * 1e3:.1f} ms (min {min(kernel[k]) * 1e3:.1f}, max {max(kernel[k]) * 1e3:.1f})")
    ratios = {k: [a / b for a, b in zip(times[k], times["V"])] for k in ("Ha", "Hb")}
    print(f"{name}: Ha / V = {med['Ha'] / med['V']:.3f} (rounds {min(ratios['Ha']):.3f} .. {max(ratios['Ha']):.3f}); "
          f"Hb / V = {med['Hb'] / med['V']:.3f} (rounds {min(ratios['Hb']):.3f} .. {max(ratios['Hb']):.3f})"
          + (f"; V / P = {med['V'] / med['P']:.3f}" if peng else ""))
    for k, pk in (("V", "P"), ("Ha", "PHa"), ("Hb", "PHb")) if peng else ():
        print(f"{name}: {k} / {pk} = {med[k] / med[pk]:.3f} wall, {statistics.median(kernel[k]) / statistics.median(kernel[pk]):.3f} k_touch; "
              f"spread of {pk}: {max(times[pk]) / min(times[pk]):.3f} wall, {max(kernel[pk]) / min(kernel[pk]):.3f} k_touch")
eng.close()
if peng:
    peng.close()
