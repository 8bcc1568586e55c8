#!/usr/bin/env python3
"""Cost of the lncRNA's per-base profile (fasim_scan_tfo_profile).  Run from the root of a built tree:

    python3 tools/tfo_profile_bench.py scan [MB] [N]   H19 x one seeded synthetic record of MB Mb (default 50), N alternating rounds
                                                       (default 5) of
                                                       profile = scan_tfo_profile(records=False)   ends after the scan phase
                                                       track   = scan_track(bin 25, records=False) ends after the scan phase
                                                       both    = scan_tfo_profile(records=True)    profile + stage 3
                                                       plain   = scan()                            the default path
    python3 tools/tfo_profile_bench.py trace           one worker, one batch of 384 full segments, dp_f16 1 and 0: profile only and
                                                       track only (for rocprofv3 --kernel-trace --stats)
The first round of every arm is a warm-up and is not reported; the arms alternate within a round, in one process.  Before anything
is printed the profile's class maxima are compared with the track's (max_i R == max_x P).
"""
import statistics
import sys
import time

sys.path.insert(0, ".")
sys.path.insert(0, "tools")
import __graft_entry__ as entry  # noqa: E402
import synth  # noqa: E402

mode = sys.argv[1] if len(sys.argv) > 1 else "scan"
mod = entry.load()
p = mod.default_params()
rna = synth.read_fasta("tests/golden/H19.fa")[1]


def line(name, ts):
    if not ts:
        print(f"{name:8s}: not measured", flush=True)
        return
    print(f"{name:8s}: median {statistics.median(ts):.3f} s  min {min(ts):.3f}  max {max(ts):.3f}  n {len(ts)}   "
          f"({' '.join(f'{t:.3f}' for t in ts)})", flush=True)


if mode == "trace":
    dnas = [mod.synth_dna(5000, 500 + k) for k in range(384)]
    for f16 in (1, 0):
        eng = mod.Engine(0)
        eng.set_option("workers", 1)
        eng.set_option("seg_batch", 384)
        eng.set_option("dp_f16", f16)
        eng.set_query(rna)
        for what in ("profile", "track"):
            for _ in range(2):
                t0 = time.perf_counter()
                if what == "profile":
                    eng.scan_tfo_profile(dnas, p, records=False)
                else:
                    eng.scan_records_track(dnas, p, bin=25, records=False)
                dt = time.perf_counter() - t0
            st = eng.last_totals[0]
            print(f"dp_f16 {f16} {what:7s}: {st['units']} units, call {dt:.3f} s, k_scan {st['kernel_ms'][0]:.3f} ms in "
                  f"{st['kernel_launches'][0]} launches, family-4 kernels {st['kernel_ms'][4]:.3f} ms", flush=True)
        eng.close()
    sys.exit(0)

mb = float(sys.argv[2]) if len(sys.argv) > 2 else 50.0
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 5
dna = mod.synth_dna(int(mb * 1e6), 12345)
eng = mod.Engine(0)
eng.set_query(rna)
print(f"scan: H19 ({len(rna)} nt) x {len(dna)} nt, {mod.segment_count(len(dna), p)} segments", flush=True)

arms = {
    "profile": lambda: eng.scan_tfo_profile(dna, p, records=False)[1],
    "track": lambda: eng.scan_track(dna, p, bin=25, records=False)[1],
    "both": lambda: eng.scan_tfo_profile(dna, p, records=True)[1],
    "plain": lambda: eng.scan(dna, p),
}
times = {k: [] for k in arms}
for rnd in range(rounds + 1):
    got = {}
    for name, fn in arms.items():
        t0 = time.perf_counter()
        got[name] = fn()
        dt = time.perf_counter() - t0
        if rnd:
            times[name].append(dt)
    if rnd == 0:
        tops = got["track"].array().max(axis=1).tolist()
        assert got["profile"].array().max(axis=1).tolist() == tops, "class maxima of profile and track differ"
        assert (got["profile"].array() == got["both"].array()).all(), "the profile depends on stage 3"
        print(f"class maxima {tops}, units {got['profile'].units}, saturated {got['profile'].saturated_units}", flush=True)
for name in arms:
    line(name, times[name])
if times["profile"] and times["track"]:
    print(f"profile / track (medians): {statistics.median(times['profile']) / statistics.median(times['track']):.3f}", flush=True)
if times["both"] and times["plain"]:
    print(f"both / plain (medians):    {statistics.median(times['both']) / statistics.median(times['plain']):.3f}", flush=True)
eng.close()
