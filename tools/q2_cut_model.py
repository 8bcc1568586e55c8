#!/usr/bin/env python3
"""CPU model of how often k_scan's Q2 hazard branch (q2_rows, csrc/systolic.h) runs, and how much of that lies behind the unit's
overflow cut, where scan.hip leaves the branch out (option q2_past_cut = 0).  A model of the step count, not the kernel:

    tools/q2_cut_model.py [segments, default 20] [rna.fa, default H19] [random | genome]

Per unit (segment x one of the 48 encodings) the textbook Gotoh recurrence (+5 / -4, gap 16 / 4) runs a column at a time, all 48
units of a segment at once.  It notes
  * events: F >= 132 entering the first row of stripe k (row k * ceil(m/16)) in column c.  Virtual lane 8 k (vs = 8: queries up to
    3 072 rows) sees that column at pipeline step c + 8 k.  The chain such an F starts decays by 4 a row, so it is alive in
    1 + (F - 132) // (4 * rows per lane) lanes, plus one for the lane that receives a dead chain's last state (lower bound), and in
    at most the 8 lanes of the stripe (upper bound): the branch is wave-uniform and runs in every step of that range;
  * the cut: the first column whose maximum reaches 251, and the step at which the kernel can know it: the block of 64 steps that
    holds the first cell >= 251 (row r of column c is computed at step c + r // rows per lane) closes at step B, and the branch is
    left out from step B + 128 on.
Printed: units with a cut, the share of all steps behind "cut + 127" and behind B + 128, and the share of all steps in which the
branch would run before and after either line (lower - upper bound)."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import synth  # noqa: E402

nseg = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rna_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "H19.fa")
kind = sys.argv[3] if len(sys.argv) > 3 else "random"
SEG, STEP, OPEN, EXT, CUT, FMIN = 5000, 4900, 16, 4, 251, 132

_, rna = synth.read_fasta(rna_path)
m = len(rna)
seg16 = (m + 15) // 16
assert seg16 >= 96 and m <= 3072, "the model covers single-tile queries with the row analysis (1 521 ... 3 072 rows)"
rpl = (seg16 + 7) // 8                                   # rows per virtual lane
n = nseg * STEP + (SEG - STEP)
dna = synth.random_dna(n, 12345) if kind == "random" else synth.genome_like(n, 12345, soft_mask=False)
code = np.full(256, 4, dtype=np.int8)
for i, ch in enumerate(b"ACGT"):
    code[ch] = i
q = code[np.frombuffer(rna.upper().replace(b"U", b"T"), dtype=np.uint8)]
idx4 = (EXT * np.arange(m)).astype(np.int16)
starts = seg16 * np.arange(1, 16)
starts = starts[starts < m]

tot_steps = units = units_cut = 0
after_skew = after_rule = 0
run = {k: [0, 0] for k in ("before_skew", "after_skew", "before_rule", "after_rule")}      # [lower, upper] bound
for s in range(nseg):
    piece = np.frombuffer(dna[s * STEP:s * STEP + SEG], dtype=np.uint8)
    t = np.empty((48, SEG), dtype=np.int8)
    for enc in range(48):
        lut = np.full(256, 4, dtype=np.int8)
        for base, o in zip(b"ATGC", synth.RULE_OUT[enc].encode()):
            lut[base] = code[o]
        row = lut[piece]
        t[enc] = row[::-1] if synth.enc_reversed(enc) else row
    hp = np.zeros((48, m), dtype=np.int16)
    ep = np.zeros((48, m), dtype=np.int16)
    fstart = np.zeros((48, SEG, len(starts)), dtype=np.int16)
    cut = np.full(48, SEG, dtype=np.int64)
    known = np.full(48, 1 << 30, dtype=np.int64)          # step at which the first cell >= 251 is computed
    for c in range(SEG):
        tc = t[:, c, None]
        sc = np.where((q[None, :] == tc) & (tc < 4), 5, -4).astype(np.int16)
        e = np.maximum(np.maximum(ep - EXT, hp - OPEN), 0)
        d = np.concatenate((np.zeros((48, 1), dtype=np.int16), hp[:, :-1]), axis=1) + sc
        h0 = np.maximum(np.maximum(d, e), 0)
        acc = np.maximum.accumulate(h0 + idx4, axis=1)
        f = np.maximum(np.concatenate((np.zeros((48, 1), dtype=np.int16), acc[:, :-1] - idx4[1:] - (OPEN - EXT)), axis=1), 0)
        hp, ep = np.maximum(h0, f), e
        fstart[:, c, :] = f[:, starts]
        over = hp >= CUT
        hit = over.any(axis=1)
        if hit.any():
            first_row = over.argmax(axis=1)
            cut = np.where(hit & (cut == SEG), c, cut)
            known = np.where(hit, np.minimum(known, c + first_row // rpl), known)
    for u in range(48):
        nsteps = SEG + 127
        lo = np.zeros(nsteps + 16, dtype=bool)
        hi = np.zeros(nsteps + 16, dtype=bool)
        cs, ks = np.nonzero(fstart[u] >= FMIN)
        for c, k in zip(cs, ks):
            s0 = c + 8 * (k + 1)
            lanes = 2 + (int(fstart[u, c, k]) - FMIN) // (EXT * rpl)
            lo[s0:s0 + min(8, lanes)] = True
            hi[s0:s0 + 8] = True
        lo, hi = lo[:nsteps], hi[:nsteps]
        units += 1
        tot_steps += nsteps
        skew = min(nsteps, cut[u] + 127) if cut[u] < SEG else nsteps
        rule = min(nsteps, (int(known[u]) | 63) + 128) if cut[u] < SEG else nsteps
        units_cut += cut[u] < SEG
        after_skew += nsteps - skew
        after_rule += nsteps - rule
        for name, line in (("skew", skew), ("rule", rule)):
            for b, arr in enumerate((lo, hi)):
                run["before_" + name][b] += int(arr[:line].sum())
                run["after_" + name][b] += int(arr[line:].sum())
    print(f"segment {s + 1} of {nseg} done", file=sys.stderr, flush=True)

pct = lambda x: 100.0 * x / tot_steps
print(f"{os.path.basename(rna_path)} ({m} rows, {rpl} rows per lane) x {nseg} segments of {kind} DNA, {units} units, {tot_steps} steps")
print(f"units with a column maximum >= {CUT}                              {100.0 * units_cut / units:5.1f} %")
print(f"steps behind cut + 127                                           {pct(after_skew):5.2f} % of all steps")
print(f"steps behind the kernel's switch (block close + 128)             {pct(after_rule):5.2f} %")
for key, text in (("before_skew", "branch steps before cut + 127"), ("after_skew", "branch steps behind cut + 127"),
                  ("before_rule", "branch steps before the kernel's switch"), ("after_rule", "branch steps behind the kernel's switch")):
    print(f"{text:64s} {pct(run[key][0]):5.2f} - {pct(run[key][1]):5.2f} %")
