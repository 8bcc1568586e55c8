#!/usr/bin/env python3
"""Cost of the potential tracks (fasim_scan_track).  Run from the root of a built tree, so that two trees can be compared:

    python3 <repo>/tools/track_bench.py LABEL plain|track|only [N]    N timed 50 Mb scans (random DNA x H19, resident) after a warm-up:
                                                                     plain = scan(), track = scan_track(bin 25) with records,
                                                                     only = scan_track(bin 25, records=False)
    python3 <repo>/tools/track_bench.py LABEL batch                   one batch of 384 segments, records + track at bin 25 and 1
                                                                     (for rocprofv3 --kernel-trace --stats)
"""
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import __graft_entry__ as entry  # noqa: E402
import synth  # noqa: E402

label, mode = sys.argv[1], sys.argv[2]
mod = entry.load()
eng = mod.Engine(0)
_, rna = synth.read_fasta("tests/golden/H19.fa")
p = mod.default_params()
if mode == "batch":
    eng.set_option("workers", 1)
    eng.set_option("seg_batch", 384)
    eng.set_query(rna)
    eng.load_dna(mod.synth_dna(384 * 4900 + 100, 12345))
    for width in (25, 1):
        for _ in range(2):
            t0 = time.perf_counter()
            res, trk = eng.scan_track(None, p, bin=width)
            dt = time.perf_counter() - t0
        st = res.stats
        print(f"bin {width}: {st['segments']} segments, {st['units']} units, {trk.nbins} bins, scan {dt:.3f} s, "
              f"kernel_ms {[round(x, 2) for x in st['kernel_ms']]} launches {st['kernel_launches']}", flush=True)
    sys.exit(0)
n = int(sys.argv[3]) if len(sys.argv) > 3 else 5
eng.set_query(rna)
eng.load_dna(mod.synth_dna(50_000_000, 12345))


def one():
    if mode == "plain":
        return eng.scan(None, p)
    return eng.scan_track(None, p, bin=25, records=(mode == "track"))


r = one()
del r
ts = []
for _ in range(n):
    t0 = time.perf_counter()
    r = one()
    ts.append(time.perf_counter() - t0)
    del r
print(f"{label:28s} {mode:6s}: mean {sum(ts) / len(ts):.3f} s  min {min(ts):.3f}  max {max(ts):.3f}   ({' '.join(f'{t:.3f}' for t in ts)})", flush=True)
