#!/usr/bin/env python3
"""Cost of screening a record set by potential (fasim_scan_records_track).  Run from the root of a built tree:

    python3 tools/screen_bench.py peaks [N]            the 532 real MEG3 peak records x MEG3, N alternating rounds (default 5) of
                                                       grouped = one scan_records_track(bin 0, records=False) call,
                                                       loop    = scan_track(bin 1, records=False) per record on the same engine,
                                                                 peaks taken from each track with numpy (the only way without the
                                                                 record-set call),
                                                       full    = scan_records (stage 3 included)
    python3 tools/screen_bench.py synth [COUNT] [N] [NLOOP]   the same for COUNT (default 20 000) seeded synthetic 2 kb windows x H19;
                                                       the per-record loop is timed NLOOP times only (default 1)
    python3 tools/screen_bench.py trace                one worker, one batch of 384 full segments: peaks only, tracks + peaks at
                                                       bin 25 and at bin 1 (for rocprofv3 --kernel-trace --stats)
The first round of every arm is a warm-up and is not reported.  Grouped and loop peaks are compared before anything is printed.
"""
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
sys.path.insert(0, "tests")
import __graft_entry__ as entry  # noqa: E402
import helpers  # noqa: E402
import synth  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "peaks"
mod = entry.load()
eng = mod.Engine(0)
p = mod.default_params()


def line(name, ts):
    if not ts:
        print(f"{name:8s}: not measured", flush=True)
        return
    print(f"{name:8s}: median {statistics.median(ts):.3f} s  min {min(ts):.3f}  max {max(ts):.3f}  n {len(ts)}   "
          f"({' '.join(f'{t:.3f}' for t in ts)})", flush=True)


if mode == "trace":
    eng.set_option("workers", 1)
    eng.set_option("seg_batch", 384)
    eng.set_query(synth.read_fasta("tests/golden/H19.fa")[1])
    dnas = [mod.synth_dna(5000, 500 + k) for k in range(384)]
    for width, records in ((0, False), (25, False), (1, False)):
        for _ in range(2):
            t0 = time.perf_counter()
            eng.scan_records_track(dnas, p, bin=width, records=records)
            dt = time.perf_counter() - t0
        st = eng.last_totals[0]
        print(f"bin {width}: {st['segments']} segments, {st['units']} units, call {dt:.3f} s, family-4 kernel_ms "
              f"{st['kernel_ms'][4]:.3f} in {st['kernel_launches'][4]} launches, k_scan {st['kernel_ms'][0]:.3f} ms", flush=True)
    sys.exit(0)

if mode == "peaks":
    rna = synth.read_fasta("tests/golden/MEG3.fa")[1]
    dnas = [s for _, s in helpers.read_peaks("tests/golden/meg3_peaks.fa.gz")]
    rounds, loop_rounds = (int(sys.argv[2]) if len(sys.argv) > 2 else 5), None
else:
    rna = synth.read_fasta("tests/golden/H19.fa")[1]
    count = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    dnas = [mod.synth_dna(2000, 900000 + k) for k in range(count)]
    rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    loop_rounds = int(sys.argv[4]) if len(sys.argv) > 4 else 1
eng.set_query(rna)
print(f"{mode}: {len(dnas)} records, {sum(len(d) for d in dnas)} nt, query {len(rna)} nt", flush=True)


def grouped():
    return eng.scan_records_track(dnas, p, bin=0, records=False)[2]


def loop():
    out = np.zeros((len(dnas), 4, 2), dtype=np.int64)
    for r, d in enumerate(dnas):
        a = eng.scan_track(d, p, bin=1, records=False)[1].array()
        v = a.max(axis=1)
        out[r, :, 0] = v
        out[r, :, 1] = np.where(v > 0, a.argmax(axis=1), -1)
    return out


def full():
    return eng.scan_records(dnas, p)


arms = {"grouped": grouped, "loop": loop, "full": full}
times = {k: [] for k in arms}
ref = None
for i in range(rounds + 1):
    for name, fn in arms.items():
        if name == "loop" and loop_rounds is not None and i > loop_rounds:
            continue
        t0 = time.perf_counter()
        r = fn()
        dt = time.perf_counter() - t0
        if name == "grouped":
            ref = r
        elif name == "loop" and not np.array_equal(r, ref[:, :, :2]):
            sys.exit("the grouped peaks differ from the per-record loop's")
        if i:
            times[name].append(dt)
        del r
for name in arms:
    line(name, times[name])
g, lp, fu = (statistics.median(times[k]) if times[k] else None for k in ("grouped", "loop", "full"))
if g and lp:
    print(f"grouped screen against the per-record loop: {lp / g:.2f} x", flush=True)
if g and fu:
    print(f"grouped screen against the full scan_records: {fu / g:.2f} x", flush=True)
