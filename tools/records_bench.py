"""Record sets against single-record scans (profiles/r05_records.txt).

  python tools/records_bench.py peaks        (a) 532 peaks x MEG3 / H19 / MALAT1: scan loop, one scan_records call, joined record
  python tools/records_bench.py synth        (b) 20 000 seeded 5 kb records x H19: scan_records against the same bases as one record
  python tools/records_bench.py cli          (c) fasim --all-records --stats on the peaks x H19, FASIM_RECORD_GROUP=0 and default

Each mode prints its lines; run every mode as its own GPU step.  Wall seconds include the host side (packing the results)."""
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers  # noqa: E402
import synth  # noqa: E402
import __graft_entry__ as entry  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden")


def _rna(name):
    return synth.read_fasta(os.path.join(GOLD, name + ".fa"))[1]


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def peaks():
    mod = entry.load()
    e = mod.Engine(0)
    dnas = [s for _, s in helpers.read_peaks()]
    joined = b"".join(dnas)
    mb = len(joined) / 1e6
    p = mod.default_params()
    print(f"(a) {len(dnas)} peak records, {len(joined)} nt; default parameters")
    for q in ("MEG3", "H19", "MALAT1"):
        e.set_query(_rna(q))
        e.scan(dnas[0], p)                                   # warm-up: workers created, buffers sized
        e.scan_records(dnas[:40], p)
        _, t_loop = _timed(lambda: [e.scan(d, p) for d in dnas])
        res, t_rec = _timed(lambda: e.scan_records(dnas, p))
        _, t_join = _timed(lambda: e.scan(joined, p))
        n = sum(r.count for r in res)
        print(f"  {q:7s} scan loop {t_loop:7.3f} s {mb / t_loop:7.2f} Mbp/s | scan_records {t_rec:6.3f} s {mb / t_rec:7.2f} Mbp/s "
              f"| joined {t_join:6.3f} s {mb / t_join:7.2f} Mbp/s | records/joined {t_rec / t_join:5.2f}x, loop/records "
              f"{t_loop / t_rec:6.1f}x ({n} triplexes)")
    e.close()


def synth_set():
    mod = entry.load()
    e = mod.Engine(0)
    n, ln = 20000, 5000
    dnas = [synth.genome_like(ln, 1000 + k, every=2000, telomere=0, soft_mask=False) for k in range(n)]
    joined = b"".join(dnas)
    p = mod.default_params()
    e.set_query(_rna("H19"))
    e.scan_records(dnas[:200], p)                            # warm-up
    e.scan(joined[:2_000_000], p)
    res, t_rec = _timed(lambda: e.scan_records(dnas, p))
    cells_rec = e.last_totals[0]["logical_cells"]
    one, t_join = _timed(lambda: e.scan(joined, p))
    cells_join = one.stats["logical_cells"]
    g_rec, g_join = cells_rec / t_rec / 1e9, cells_join / t_join / 1e9
    print(f"(b) {n} records x {ln} nt ({len(joined) / 1e6:.0f} Mb) x H19: scan_records {t_rec:6.3f} s {g_rec:7.0f} Gcells/s "
          f"({e.last_totals[0]['units']} units) | one record {t_join:6.3f} s {g_join:7.0f} Gcells/s ({one.stats['units']} units) "
          f"| ratio {g_rec / g_join:4.2f} (Gcells/s), {t_join / t_rec:4.2f} (wall); logical cells counted per segment, so the "
          f"100-nt tail segment of every 5 kb record counts as work")
    e.close()


def cli():
    exe = os.path.join(entry.PKG_DIR, "fasim")
    with tempfile.TemporaryDirectory() as d:
        with open(os.path.join(d, "peaks.fa"), "wb") as f:
            f.write(helpers.gunzip(os.path.join(GOLD, "meg3_peaks.fa.gz")))
        with open(os.path.join(d, "H19.fa"), "wb") as f:
            f.write(open(os.path.join(GOLD, "H19.fa"), "rb").read())
        out = {}
        for name, group in (("per-record (FASIM_RECORD_GROUP=0)", "0"), ("grouped (default)", None)):
            os.makedirs(os.path.join(d, name[:5]), exist_ok=True)
            env = dict(os.environ)
            env.pop("FASIM_RECORD_GROUP", None)
            if group is not None:
                env["FASIM_RECORD_GROUP"] = group
            r, t = _timed(lambda: subprocess.run([exe, "-f1", "peaks.fa", "-f2", "H19.fa", "-O", name[:5] + "/", "--all-records", "--stats"],
                                                 cwd=d, env=env, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE))
            end = [l for l in r.stderr.decode().splitlines() if "end to end" in l]
            groups = [l for l in r.stderr.decode().splitlines() if l.startswith("[fasim] group")]
            out[name] = t
            print(f"(c) fasim --all-records peaks x H19, {name}: {t:7.3f} s wall; {len(groups)} group line(s)")
            for l in end + groups[:3]:
                print("    " + l)
        a, b = out.values()
        print(f"(c) speed-up end to end: {a / b:5.1f}x")


if __name__ == "__main__":
    {"peaks": peaks, "synth": synth_set, "cli": cli}[sys.argv[1]]()
