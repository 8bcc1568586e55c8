"""`fasim --regions` against pre-extracted records (profiles/r06_regions.txt).

  python tools/regions_bench.py WORKDIR [N_INTERVALS]

A 309 Mb genome (tools/make_genome.py OUT 0.1, headers rewritten to UCSC form: >chr1 ...), N_INTERVALS (default 20 000)
promoter-like 5 kb intervals (BED6, seeded, sorted by chromosome and start, either strand) and H19, all with --upper (the genome
is soft-masked).  Three timings, each a fresh process:
  (b) the extraction step alone: the intervals cut out of the genome into >NAME|CHROM|START+1-END records (Python, streaming);
  (a) fasim --all-records on that FASTA;
  (r) fasim --regions on the genome and the BED file.
Wall seconds, the scan seconds of --stats and the peak host RSS of every step; (r) and (a) must write the same files."""
import filecmp
import os
import random
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "fasim-longtarget_amd", "fasim")
GOLD = os.path.join(ROOT, "tests", "golden")


def _run(cmd, cwd):
    """(wall s, peak RSS MB, stderr) of one child process."""
    t0 = time.perf_counter()
    p = subprocess.Popen(cmd, cwd=cwd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    err = p.stderr.read().decode()
    _, status, ru = os.wait4(p.pid, 0)
    p.returncode = os.waitstatus_to_exitcode(status)
    wall = time.perf_counter() - t0
    if p.returncode != 0:
        sys.exit(f"{cmd[0]} exited {p.returncode}:\n{err[-3000:]}")
    return wall, ru.ru_maxrss / 1024.0, err


def _genome(wd):
    raw, out = os.path.join(wd, "raw.fa"), os.path.join(wd, "genome.fa")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_genome.py"), raw, "0.1"], check=True, stdout=subprocess.DEVNULL)
    lens = {}
    with open(raw, "rb") as f, open(out, "wb") as g:
        chrom = None
        for line in f:
            if line.startswith(b">"):
                chrom = line[1:].split(b"|")[1].decode()
                lens[chrom] = 0
                g.write(f">{chrom} synthetic stand-in\n".encode())
            else:
                lens[chrom] += len(line) - 1
                g.write(line)
    os.remove(raw)
    return out, lens


def _bed(wd, lens, n):
    rng = random.Random(2024)
    chroms = list(lens)
    weights = [lens[c] for c in chroms]
    rows = []
    for k in range(n):
        c = rng.choices(chroms, weights)[0]
        tss = rng.randrange(2000, lens[c] - 3000)
        rows.append((chroms.index(c), tss - 2000, tss + 3000, f"prom{k}", rng.choice("+-")))
    rows.sort()
    path = os.path.join(wd, "promoters.bed")
    with open(path, "w") as f:
        for ci, s, e, name, strand in rows:
            f.write(f"{chroms[ci]}\t{s}\t{e}\t{name}\t0\t{strand}\n")
    return path


EXTRACT = r'''
import sys
bed, genome, out = sys.argv[1:4]
want = {}
for line in open(bed):
    c, s, e, name = line.split()[:4]
    want.setdefault(c, []).append((int(s), int(e), name))
def emit(f, chrom, parts):
    seq = b"".join(parts)
    for s, e, name in want.get(chrom, ()):
        f.write(b">%s|%s|%d-%d\n" % (name.encode(), chrom.encode(), s + 1, e) + seq[s:e] + b"\n")
with open(genome, "rb") as g, open(out, "wb") as f:
    chrom, parts = None, []
    for line in g:
        if line.startswith(b">"):
            if chrom is not None:
                emit(f, chrom, parts)
            chrom, parts = line[1:].split()[0].decode(), []
        else:
            parts.append(line.rstrip(b"\n"))
    if chrom is not None:
        emit(f, chrom, parts)
'''


def _scan_s(err):
    m = re.search(r"\[fasim\] end to end ([0-9.]+) s: parse ([0-9.]+), scan ([0-9.]+)", err)
    return (float(m.group(1)), float(m.group(3))) if m else (float("nan"), float("nan"))


def main():
    wd = os.path.abspath(sys.argv[1])
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 20000
    os.makedirs(wd, exist_ok=True)
    t0 = time.perf_counter()
    genome, lens = _genome(wd)
    bed = _bed(wd, lens, n)
    print(f"genome {sum(lens.values())} nt in {len(lens)} records (UCSC headers), {n} intervals x 5000 nt, H19, --upper; "
          f"setup {time.perf_counter() - t0:.1f} s", flush=True)
    with open(os.path.join(wd, "H19.fa"), "wb") as f:
        f.write(open(os.path.join(GOLD, "H19.fa"), "rb").read())
    wall_x, rss_x, _ = _run([sys.executable, "-c", EXTRACT, bed, genome, os.path.join(wd, "promoters.fa")], wd)
    print(f"(b) extraction alone        wall {wall_x:7.2f} s                         peak RSS {rss_x:8.1f} MB", flush=True)
    res = {}
    for key, args in (("a", ["-f1", "promoters.fa", "--all-records", "-O", "out_a/"]),
                      ("r", ["-f1", "genome.fa", "--regions", "promoters.bed", "-O", "out_r/"])):
        os.makedirs(os.path.join(wd, f"out_{key}"), exist_ok=True)
        wall, rss, err = _run([EXE, *args, "-f2", "H19.fa", "--upper", "--stats"], wd)
        e2e, scan = _scan_s(err)
        res[key] = (wall, scan)
        label = "(a) --all-records (extracted)" if key == "a" else "(r) --regions               "
        print(f"{label} wall {wall:7.2f} s  (end to end {e2e:7.2f}, scan {scan:7.2f})  peak RSS {rss:8.1f} MB", flush=True)
    # the same files under the same names, apart from the FASTA stem (promoters / genome) and the index
    a, r = os.path.join(wd, "out_a"), os.path.join(wd, "out_r")
    fa = sorted(os.listdir(a))
    fr = sorted(x for x in os.listdir(r) if not x.endswith(".regions.tsv"))
    same = [x.replace("-promoters.", "-genome.") for x in fa] == fr and \
        all(filecmp.cmp(os.path.join(a, x), os.path.join(r, x.replace("-promoters.", "-genome.")), shallow=False) for x in fa)
    print(f"files: {len(fr)} per run, identical: {same}")
    print(f"(r) / (a): scan {res['r'][1] / res['a'][1]:.3f}, wall {res['r'][0] / res['a'][0]:.3f}; "
          f"(r) / ((a) + (b)) wall {res['r'][0] / (res['a'][0] + wall_x):.3f}")
    if not same:
        sys.exit(1)


if __name__ == "__main__":
    main()
