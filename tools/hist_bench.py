#!/usr/bin/env python3
"""Cost of the potential histogram on the device (fasim_scan_records_hist, fasim_scan_oligos_hist).  Run from the root of a built tree:

    python3 tools/hist_bench.py scan [MB] [N]      a planted record of MB Mb (default 50) x H19, N alternating rounds (default 4) of
                                                   hist    = scan_hist(records=False),
                                                   track   = scan_track(bin=1, records=False), the call alone,
                                                   numpy   = np.bincount per class over that track (track + numpy: what there was),
                                                   hist4   = scan_hist(controls=4, records=False): the lncRNA and four controls,
                                                   track5  = five track-only calls, the lncRNA and the same four shuffles
    python3 tools/hist_bench.py oligos [MB] [N]    a 64 x 20 nt panel: scan_oligos_hist against scan_oligos(track_bin=1) + bincount
    python3 tools/hist_bench.py kernel             one worker, one batch of 384 full segments: the HIP-event time of kernel family 4
                                                   for a track-only and a histogram-only call (k_track against k_hist)
The first round of every arm is a warm-up and is not reported.  Every round compares the arrays of the two paths before anything is
printed.  Bytes copied back: 4 x 2 x N for a track; per batch and query 4 x 4 x (min(16383, 5 x 16 ceil(m / 16)) + 1) counters,
2 x 4 x 2 x overlapLength zone values per segment and one byte per unit for a histogram.
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


def bincount4(a):
    return np.stack([np.bincount(a[c], minlength=mod.HIST_BINS) for c in range(4)]).astype(np.int64)


def hist_bytes(m, nseg, nenc, batches):
    top = min(mod.HIST_BINS - 1, 5 * 16 * ((m + 15) // 16))
    return batches * 16 * (top + 1) + nseg * 16 * p.overlapLength + nseg * nenc


if mode == "kernel":
    eng.set_option("workers", 1)
    eng.set_option("seg_batch", 384)
    eng.set_query(rna)
    dnas = [mod.synth_dna(5000, 500 + k) for k in range(384)]
    for what in ("track", "hist"):
        for _ in range(2):
            t0 = time.perf_counter()
            if what == "track":
                eng.scan_records_track(dnas, p, bin=1, records=False)
            else:
                eng.scan_hist(dnas, p)
            dt = time.perf_counter() - t0
        st = eng.last_totals[0]
        print(f"{what}: {st['segments']} segments, {st['units']} units, call {dt:.3f} s, family-4 kernel_ms {st['kernel_ms'][4]:.3f} in "
              f"{st['kernel_launches'][4]} launches (k_encode and the fold), k_scan {st['kernel_ms'][0]:.3f} ms", flush=True)
    sys.exit(0)

mb = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 4
dna = synth.planted_dna(mb * 1000000, 12345, rna)
nseg = mod.segment_count(len(dna), p)
keep = {}

if mode == "oligos":
    panel = [rna[100 + 20 * k:120 + 20 * k] for k in range(64)]
    print(f"oligos: planted record of {len(dna)} nt x a panel of {len(panel)} oligos of 20 nt, {nseg} segments", flush=True)

    def hist():
        keep["hist"] = [h.array() for h in eng.scan_oligos_hist(panel, dna, p)]

    def track():
        keep["track"] = [t[0] for t in eng.scan_oligos(panel, dna, p, min_value=16383, track_bin=1)[1]]

    def numpy_side():
        keep["counts"] = [bincount4(t.array()) for t in keep["track"]]

    arms = {"hist": hist, "track": track, "numpy": numpy_side}
else:
    eng.set_query(rna)
    ctl = [mod.shuffle_query(rna, 1, k) for k in (1, 2, 3, 4)]
    print(f"scan: planted record of {len(dna)} nt x H19 ({len(rna)} nt), {nseg} segments", flush=True)

    def hist():
        keep["hist"] = [eng.scan_hist(dna, p)[1].array()]

    def track():
        eng.set_query(rna)
        keep["track"] = [eng.scan_track(dna, p, bin=1, records=False)[1]]

    def numpy_side():
        keep["counts"] = [bincount4(t.array()) for t in keep["track"]]

    def hist4():
        _, h, c = eng.scan_hist(dna, p, controls=4, seed=1)
        keep["hist4"] = [h.array()] + [x.array() for x in c]

    def track5():
        out = []
        for q in [rna] + ctl:
            eng.set_query(q)
            out.append(bincount4(eng.scan_track(dna, p, bin=1, records=False)[1].array()))      # (the bincount is inside this arm)
        eng.set_query(rna)
        keep["counts5"] = out

    arms = {"hist": hist, "track": track, "numpy": numpy_side, "hist4": hist4, "track5": track5}

times = {k: [] for k in arms}
for i in range(rounds + 1):
    for name, fn in arms.items():
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i:
            times[name].append(dt)
    if not all(np.array_equal(a, b) for a, b in zip(keep["hist"], keep["counts"])):
        sys.exit("the device's histogram differs from the bincount of the track")
    if "hist4" in keep and not all(np.array_equal(a, b) for a, b in zip(keep["hist4"], keep["counts5"])):
        sys.exit("the histograms of the controls differ from the bincounts of their tracks")
for name in arms:
    line(name, times[name])
th, tt, tn = (statistics.median(times[k]) for k in ("hist", "track", "numpy"))
spread = max(times["track"]) - min(times["track"])
print(f"histogram-only against track-only alone: {th:.3f} s against {tt:.3f} s (spread of the track-only rounds {spread:.3f} s); "
      f"track + numpy {tt + tn:.3f} s = {(tt + tn) / th:.2f} x", flush=True)
if "hist4" in times:
    t4, t5 = statistics.median(times["hist4"]), statistics.median(times["track5"])
    print(f"the lncRNA and four controls: one histogram call {t4:.3f} s against five track calls with their bincounts {t5:.3f} s = {t5 / t4:.2f} x", flush=True)
nq = len(keep["hist"])
batches = (nseg + 383) // 384
m = 20 if mode == "oligos" else len(rna)
print(f"bytes copied back per query: track {8 * len(dna)}; histogram about {hist_bytes(m, nseg, 48, batches)} "
      f"({batches} batches or more; {nq} quer{'y' if nq == 1 else 'ies'} in the call)", flush=True)
