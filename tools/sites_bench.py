#!/usr/bin/env python3
"""Cost of calling sites on the device (fasim_scan_records_sites).  Run from the root of a built tree:

    python3 tools/sites_bench.py scan [MB] [N]     a planted record of MB Mb (default 50) x H19, N alternating rounds (default 4) of
                                                   sites  = scan_sites(records=False) at V = int(0.8 x the record's largest potential),
                                                   track  = scan_track(bin=1, records=False), the call alone (what there was before),
                                                   numpy  = the run extraction from that track on the host (start, end, value, pos of
                                                            every run of every class; no encoding: the track does not carry it),
                                                   dense  = scan_sites(records=False) at V = the median of the non-zero potential
    python3 tools/sites_bench.py trace [V]         one worker, one batch of 384 full segments: track only at bin 1, then sites only at
                                                   V (default 100) and at V = 30 (for rocprofv3 --kernel-trace --stats)
The first round of every arm is a warm-up and is not reported.  The runs of the numpy side and the sites of the device side are
compared (class, start, end, value, pos) before anything is printed.  Bytes copied back: 4 x 2 x N for the track; 16 per raw run plus
16 per slice (4 counts of 4 bytes) and one byte per unit for the sites.
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


if mode == "trace":
    eng.set_option("workers", 1)
    eng.set_option("seg_batch", 384)
    eng.set_query(rna)
    dnas = [mod.synth_dna(5000, 500 + k) for k in range(384)]
    v = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    for what in ("track", v, 30):
        for _ in range(2):
            t0 = time.perf_counter()
            if what == "track":
                eng.scan_records_track(dnas, p, bin=1, records=False)
                runs = 0
            else:
                runs = sum(s.raw_runs for s in eng.scan_sites(dnas, p, min_value=what, records=False)[1])
            dt = time.perf_counter() - t0
        st = eng.last_totals[0]
        print(f"{what}: {st['segments']} segments, {st['units']} units, {runs} raw runs, call {dt:.3f} s, family-4 kernel_ms "
              f"{st['kernel_ms'][4]:.3f} in {st['kernel_launches'][4]} launches, k_scan {st['kernel_ms'][0]:.3f} ms", flush=True)
    sys.exit(0)

mb = int(sys.argv[2]) if len(sys.argv) > 2 else 50
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 4
dna = synth.planted_dna(mb * 1000000, 12345, rna)
eng.set_query(rna)
print(f"scan: planted record of {len(dna)} nt x H19 ({len(rna)} nt), {mod.segment_count(len(dna), p)} segments", flush=True)


def host_runs(a, v):
    """(n, 5) rows (cls, start, end, value, pos) of the runs of a (4, N) track, ordered by (start, cls)"""
    out = []
    for c in range(4):
        on = np.concatenate(([0], (a[c] >= v).astype(np.int8), [0]))
        d = np.diff(on)
        starts, ends = np.flatnonzero(d == 1), np.flatnonzero(d == -1)
        if not len(starts):
            continue
        value = np.maximum.reduceat(a[c], starts)
        # (reduceat runs to the next start: positions between a run's end and the next start are below v, so the maximum is the run's)
        pos = np.array([s + int(np.argmax(a[c, s:e])) for s, e in zip(starts.tolist(), ends.tolist())], dtype=np.int64)
        out.append(np.stack([np.full(len(starts), c, dtype=np.int64), starts, ends, value.astype(np.int64), pos], axis=1))
    rows = np.concatenate(out) if out else np.zeros((0, 5), dtype=np.int64)
    return rows[np.lexsort((rows[:, 0], rows[:, 1]))]


track0 = eng.scan_track(dna, p, bin=1, records=False)[1].array()
top = int(track0.max())
v_sparse, v_dense = int(0.8 * top), int(np.median(track0[track0 > 0]))
units = eng.scan_track(dna[:5000], p, bin=1, records=False)[1].units * mod.segment_count(len(dna), p)
print(f"largest potential {top}: V = {v_sparse}; dense case V = {v_dense} (the median of the non-zero potential)", flush=True)
del track0
keep = {}


def sites():
    s = eng.scan_sites(dna, p, min_value=v_sparse, records=False)[1][0]
    keep["sites"] = (s.array(), s.raw_runs)


def track():
    keep["track"] = eng.scan_track(dna, p, bin=1, records=False)[1]


def numpy_side():
    keep["runs"] = host_runs(keep["track"].array(), v_sparse)


def dense():
    s = eng.scan_sites(dna, p, min_value=v_dense, records=False)[1][0]
    keep["dense"] = (len(s), s.raw_runs)


arms = {"sites": sites, "track": track, "numpy": numpy_side, "dense": dense}
times = {k: [] for k in arms}
for i in range(rounds + 1):
    for name, fn in arms.items():
        t0 = time.perf_counter()
        fn()
        dt = time.perf_counter() - t0
        if i:
            times[name].append(dt)
    if not np.array_equal(keep["sites"][0][:, :5], keep["runs"]):
        sys.exit("the device's sites differ from the runs of the track")
for name in arms:
    line(name, times[name])
ts, tt, tn = (statistics.median(times[k]) for k in ("sites", "track", "numpy"))
spread = max(times["track"]) - min(times["track"])
nslice = mod.segment_count(len(dna), p) * ((p.cutLength + 2039) // 2040)
print(f"sites-only against track-only alone: {ts:.3f} s against {tt:.3f} s (spread of the track-only rounds {spread:.3f} s); "
      f"track + numpy {tt + tn:.3f} s = {(tt + tn) / ts:.2f} x", flush=True)
print(f"bytes copied back: track {8 * len(dna)}; sites at V = {v_sparse}: {16 * keep['sites'][1] + 16 * nslice + units} "
      f"({len(keep['sites'][0])} sites from {keep['sites'][1]} raw runs); dense V = {v_dense}: "
      f"{16 * keep['dense'][1] + 16 * nslice + units} ({keep['dense'][0]} sites from {keep['dense'][1]} raw runs)", flush=True)
